"""NumPy restatement of the clipped b-bit fake-quant (include/lq_hip.h: lq_fq_forward_clip / lq_fq_backward_clip), the
reference of tests/test_clip_cpu.py (which pins it on hand-written tables) and tests/test_gpu_clip.py.

    t = P / s (float32)    q0 = floor(t)    q = q0 < lo ? lo : (q0 > hi ? hi : q0)    out = q * s (float32)
    inside = (q0 >= lo) & (q0 <= hi)        dP = inside ? dy : +0
    r = inside ? q0 - t (ONE float32 subtraction) : q          ds = k * sum dy * r (float64)       clipped = #{!inside}
"""
import numpy as np


def clip_reference(P, s, dy, qmin, qmax, k=1.0):
    """dict(out, q, dP, ds, terms, clipped, inside): out / q / dP float32 in the shape of P; ds (float64), terms = k * sum|dy r|
    (float64) and clipped (int64) in the shape of ``s``.  ``s`` broadcasts against ``P`` (one non-unit axis, or one element)."""
    P, dy, s = np.asarray(P, np.float32), np.asarray(dy, np.float32), np.asarray(s, np.float32)
    sb = s if s.ndim == P.ndim else s.reshape((1,) * P.ndim)
    lo, hi = np.float32(qmin), np.float32(qmax)
    assert float(lo) == qmin and float(hi) == qmax
    with np.errstate(all="ignore"):
        t = P / sb
        q0 = np.floor(t)
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
    return dict(out=out, q=q, dP=dP, ds=ds, terms=terms, clipped=clipped, inside=inside, q0=q0, r=r)


def with_other_dy(ref, s, dy, k=1.0):
    """(dP, ds, terms) of the same P, s and range for another upstream gradient, from the parts ``clip_reference`` returned."""
    dy, s = np.asarray(dy, np.float32), np.asarray(s, np.float32)
    sb = s if s.ndim == dy.ndim else s.reshape((1,) * dy.ndim)
    axes = tuple(a for a in range(dy.ndim) if sb.shape[a] == 1)
    with np.errstate(all="ignore"):
        prod = dy.astype(np.float64) * ref["r"].astype(np.float64)
        k64 = float(np.float32(k))
        return (np.where(ref["inside"], dy, np.float32(0.0)), prod.sum(axis=axes).reshape(s.shape) * k64,
                np.abs(prod).sum(axis=axes).reshape(s.shape) * abs(k64))


def bits_equal(a, b):
    """Bit-for-bit equality of two float32 arrays (the sign of zero and NaN payload-insensitive NaN == NaN included)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | both_nan))


def edge_table(qmin, qmax, s):
    """Quotients around both edges of [qmin, qmax] for a power-of-two ``s`` (P = t * s is then exact and P / s gives t back):
    (P, expected q, expected inside)."""
    s = np.float32(s)
    ulp_hi = np.spacing(np.float32(qmax + 1))
    eps = np.float32(2.0 ** -7)
    rows = [
        (qmin - 1, qmin, False), (qmin - eps, qmin, False), (qmin, qmin, True), (qmin + eps, qmin, True),
        (qmin + 1 - eps, qmin, True), (qmax, qmax, True), (qmax + eps, qmax, True),
        (np.float32(qmax + 1) - ulp_hi, qmax, True), (qmax + 1, qmax, False), (qmax + 5, qmax, False), (qmin - 7, qmin, False),
    ]
    t = np.array([r[0] for r in rows], np.float32)
    return t * s, np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], bool)
