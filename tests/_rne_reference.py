"""NumPy restatement of the clipped b-bit fake-quant with round-to-nearest (include/lq_hip.h: lq_fq_forward_clip_r /
lq_fq_backward_clip_r with LQ_ROUND_NEAREST_EVEN), the reference of tests/test_rounding_cpu.py (which pins it on a hand-written
table) and tests/test_gpu_rounding.py.  It is tests/_clip_reference.py with np.rint (round half to even) in place of np.floor:

    t = P / s (float32)    q0 = rint(t)     q = q0 < lo ? lo : (q0 > hi ? hi : q0)    out = q * s (float32)
    inside = (q0 >= lo) & (q0 <= hi)        dP = inside ? dy : +0
    r = inside ? q0 - t (ONE float32 subtraction, in [-1/2, 1/2]) : q     ds = k * sum dy * r (float64)     clipped = #{!inside}
"""
import numpy as np

from _clip_reference import bits_equal      # noqa: F401  (re-exported: the tests compare floats bit for bit)


def rne_reference(P, s, dy, qmin, qmax, k=1.0):
    """dict(out, q, dP, ds, terms, clipped, inside, q0, r): out / q / dP float32 in the shape of P; ds (float64), terms = k * sum|dy r|
    (float64) and clipped (int64) in the shape of ``s``.  ``s`` broadcasts against ``P`` (one non-unit axis, or one element)."""
    P, dy, s = np.asarray(P, np.float32), np.asarray(dy, np.float32), np.asarray(s, np.float32)
    sb = s if s.ndim == P.ndim else s.reshape((1,) * P.ndim)
    lo, hi = np.float32(qmin), np.float32(qmax)
    assert float(lo) == qmin and float(hi) == qmax
    with np.errstate(all="ignore"):
        t = P / sb
        q0 = np.rint(t)                                               # round half to even; -0.0 for t in [-1/2, -0]
        q = np.where(q0 < lo, lo, np.where(q0 > hi, hi, q0))          # comparisons: a NaN q0 stays NaN, +-Inf saturates
        out = q * sb
        inside = (q0 >= lo) & (q0 <= hi)
        dP = np.where(inside, dy, np.float32(0.0))
        r = np.where(inside, q0 - t, q)
        assert t.dtype == q.dtype == out.dtype == dP.dtype == r.dtype == np.float32
        prod = dy.astype(np.float64) * r.astype(np.float64)
        axes = tuple(a for a in range(P.ndim) if sb.shape[a] == 1)
        k64 = float(np.float32(k))                                    # the factor travels as a C float
        ds = prod.sum(axis=axes).reshape(s.shape) * k64
        terms = np.abs(prod).sum(axis=axes).reshape(s.shape) * abs(k64)
        clipped = (~inside).sum(axis=axes).reshape(s.shape).astype(np.int64)
    return dict(out=out, q=q, dP=dP, ds=ds, terms=terms, clipped=clipped, inside=inside, q0=q0, r=r, t=t)


def with_other_dy(ref, s, dy, k=1.0):
    """(dP, ds, terms) of the same P, s and range for another upstream gradient, from the parts ``rne_reference`` returned."""
    dy, s = np.asarray(dy, np.float32), np.asarray(s, np.float32)
    sb = s if s.ndim == dy.ndim else s.reshape((1,) * dy.ndim)
    axes = tuple(a for a in range(dy.ndim) if sb.shape[a] == 1)
    with np.errstate(all="ignore"):
        prod = dy.astype(np.float64) * ref["r"].astype(np.float64)
        k64 = float(np.float32(k))
        return (np.where(ref["inside"], dy, np.float32(0.0)), prod.sum(axis=axes).reshape(s.shape) * k64,
                np.abs(prod).sum(axis=axes).reshape(s.shape) * abs(k64))


def floor_integers(P, s, qmin, qmax):
    """clamp(floor(P/s)): what the floor pair stores, for the "a floor kernel cannot pass" condition of the GPU tests."""
    P, s = np.asarray(P, np.float32), np.asarray(s, np.float32)
    sb = s if s.ndim == P.ndim else s.reshape((1,) * P.ndim)
    with np.errstate(all="ignore"):
        q0 = np.floor(P / sb)
    return np.where(q0 < np.float32(qmin), np.float32(qmin), np.where(q0 > np.float32(qmax), np.float32(qmax), q0))


def tie_table(qmin, qmax):
    """Quotients for a power-of-two scale (P = t * s is exact): every half-integer from qmin - 1.5 to qmax + 1.5, the neighbours of
    qmin - 1/2 and qmax + 1/2 one ulp to either side, and +-0.  Returns (t, expected q0) with q0 written out by the rule itself
    -- a half-integer n + 1/2 goes to the even one of n and n + 1 -- not by np.rint."""
    ts, q0s = [], []
    for n in range(qmin - 2, qmax + 2):                     # t = n + 1/2
        ts.append(np.float32(n) + np.float32(0.5))
        q0s.append(np.float32(n if n % 2 == 0 else n + 1))
    for edge, below, above in ((np.float32(qmin) - np.float32(0.5), qmin - 1, qmin), (np.float32(qmax) + np.float32(0.5), qmax, qmax + 1)):
        ts += [np.nextafter(edge, np.float32(-np.inf)), np.nextafter(edge, np.float32(np.inf))]
        q0s += [np.float32(below), np.float32(above)]
    ts += [np.float32(0.0), np.float32(-0.0)]
    q0s += [np.float32(0.0), np.float32(-0.0)]
    t, q0 = np.array(ts, np.float32), np.array(q0s, np.float32)
    return t, np.where(q0 == 0, np.copysign(np.float32(0.0), t), q0)      # a zero result carries the sign of t: rint(-0.4) is -0
