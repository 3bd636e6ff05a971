"""NumPy restatement of the asymmetric group-wise quantizer and of its min-max initialisation (include/lq_hip.h:
lq_fq_forward_group_affine / lq_fq_backward_group_affine / lq_scale_init_group_minmax), float32 operation for operation: the
reference of tests/test_group_affine_cpu.py (which pins it on a hand-written table and against _group_reference.py at b = 0) and
of tests/test_gpu_group_affine.py.

Geometry as tests/_group_reference.py; the offset ``b`` has the scale's shape and is expanded to the element grid like it.

    u = P - b    t = u / s    q0 = floor(t) | rint(t)    q = q0 < lo ? lo : (q0 > hi ? hi : q0)    out = (q * s) + b   (float32 each)
    inside = (q0 >= lo) & (q0 <= hi)        dP = inside ? dy : +0        r = inside ? q0 - t : q
    ds = k * sum dy * r    db = kb * sum_{!inside} dy    (float64)       clipped = #{!inside}

    minmax:  mn, mx per group;  n = float32(qmax - qmin);  s = max(((mx - mn) / n) * (1 + 2^-22), min_value)   (float32 each)
             mid = 0.5 * mn + 0.5 * mx;  c = (qmin + qmax) / 2 (+ 1/2 for floor);  b = mid - c * s;  NaN / Inf in the group: s = b = NaN
"""
import numpy as np

from _group_reference import _per_group, expand_scale, scale_shape
from _scale_init_reference import MARGIN, MIN_VALUE, _groups, _to_scale


def group_affine_reference(P, s, b, dy, qmin, qmax, axis, gs, k=1.0, kb=1.0, rounding="floor"):
    """dict(out, q, dP, ds, terms, db, terms_b, clipped, inside, q0, r, t): out / q / dP float32 [R][C]; ds, db (float64), terms =
    |k| * sum|dy r|, terms_b = |kb| * sum_{!inside}|dy| (float64) and clipped (int64) in the shape of ``s``."""
    P, dy = np.asarray(P, np.float32), np.asarray(dy, np.float32)
    assert P.ndim == 2 and dy.shape == P.shape and axis in (0, 1) and gs >= 1 and rounding in ("floor", "nearest")
    R, C = P.shape
    sb = expand_scale(s, R, C, axis, gs)
    bb = expand_scale(b, R, C, axis, gs)
    lo, hi = np.float32(qmin), np.float32(qmax)
    assert float(lo) == qmin and float(hi) == qmax
    with np.errstate(all="ignore"):
        u = P - bb
        t = u / sb
        q0 = np.floor(t) if rounding == "floor" else np.rint(t)
        q = np.where(q0 < lo, lo, np.where(q0 > hi, hi, q0))          # comparisons: a NaN q0 stays NaN, +-Inf saturates
        m = q * sb
        out = m + bb
        inside = (q0 >= lo) & (q0 <= hi)
        dP = np.where(inside, dy, np.float32(0.0))
        r = np.where(inside, q0 - t, q)
        assert u.dtype == t.dtype == q.dtype == m.dtype == out.dtype == dP.dtype == r.dtype == np.float32
        prod = dy.astype(np.float64) * r.astype(np.float64)
        outside = np.where(inside, 0.0, dy.astype(np.float64))
        k64, kb64 = float(np.float32(k)), float(np.float32(kb))      # the factors travel as C floats
        ds = _per_group(prod, R, C, axis, gs) * k64
        terms = _per_group(np.abs(prod), R, C, axis, gs) * abs(k64)
        db = _per_group(outside, R, C, axis, gs) * kb64
        terms_b = _per_group(np.abs(outside), R, C, axis, gs) * abs(kb64)
        clipped = _per_group((~inside).astype(np.int64), R, C, axis, gs)
    return dict(out=out, q=q, dP=dP, ds=ds, terms=terms, db=db, terms_b=terms_b, clipped=clipped, inside=inside, q0=q0, r=r, t=t)


def minmax_center(qmin, qmax, rounding):
    c = (qmin + qmax) / 2.0 + (0.5 if rounding == "floor" else 0.0)
    assert float(np.float32(c)) == c
    return np.float32(c)


def minmax_reference(P, qmin, qmax, axis, gs, rounding="floor", min_value=MIN_VALUE):
    """dict(s, b: float32 in the shape of the scale; bad: bool, the group holds a NaN or an Inf)."""
    P = np.asarray(P, np.float32)
    assert P.ndim == 2 and axis in (0, 1) and gs >= 1 and rounding in ("floor", "nearest")
    assert qmax > qmin and -(1 << 22) <= qmin and qmax <= (1 << 22)
    x, m, _ = _groups(P, axis, gs)
    mv = np.float32(min_value)
    bad = (~np.isfinite(x)).any(axis=-1)
    n, c, half = np.float32(qmax - qmin), minmax_center(qmin, qmax, rounding), np.float32(0.5)
    with np.errstate(all="ignore"):
        mn = np.fmin.reduce(np.where(m, x, np.float32(np.inf)), axis=-1)      # fmin / fmax skip a NaN: the bad flag has it
        mx = np.fmax.reduce(np.where(m, x, np.float32(-np.inf)), axis=-1)
        s = np.maximum(((mx - mn) / n) * MARGIN, mv)
        mid = half * mn + half * mx
        b = mid - c * s
    assert s.dtype == b.dtype == np.float32
    nan = np.float32(np.nan)
    return dict(s=_to_scale(np.where(bad, nan, s).astype(np.float32), axis), b=_to_scale(np.where(bad, nan, b).astype(np.float32), axis),
                bad=_to_scale(bad, axis))


def make_affine_case(seed, R, C, axis, gs):
    """The inputs of the GPU tests: per-group s = 2^U(-9, -5), b = U(-6, 6) * s, P = N(0, 1) * 8 s + b, dy = N(0, 1)."""
    rng = np.random.default_rng(seed)
    shape = scale_shape(R, C, axis, gs)
    s = np.exp2(rng.uniform(-9.0, -5.0, size=shape)).astype(np.float32)
    b = (rng.uniform(-6.0, 6.0, size=shape).astype(np.float32) * s).astype(np.float32)
    sb, bb = expand_scale(s, R, C, axis, gs), expand_scale(b, R, C, axis, gs)
    P = (rng.standard_normal((R, C)).astype(np.float32) * (np.float32(8.0) * sb) + bb).astype(np.float32)
    dy = rng.standard_normal((R, C)).astype(np.float32)
    return P, s, b, dy


def edge_affine_case(seed, R, C, axis, gs, qmin, qmax, rounding):
    """(P, s, b, dy, want_q0): power-of-two scales 2^e (e in -8 .. -3), offsets j * s with integer j in [-40, 40], and
    P = (m + j) * s exactly with m cycling through lo, hi, hi + 1, lo - 1/2, hi + 1/2 and lo + 1 along the group: u = m * s and
    t = m without a rounding, so q0 is floor(m) or rint(m) exactly -- ``want_q0`` on the element grid."""
    rng = np.random.default_rng(seed)
    shape = scale_shape(R, C, axis, gs)
    s = np.exp2(rng.integers(-8, -2, size=shape)).astype(np.float32)
    j = rng.integers(-40, 41, size=shape).astype(np.float32)
    b = j * s
    sb, jb = expand_scale(s, R, C, axis, gs), expand_scale(j, R, C, axis, gs)
    ms = np.array([qmin, qmax, qmax + 1, qmin - 0.5, qmax + 0.5, qmin + 1], np.float32)
    along = (np.arange(R)[:, None] + np.arange(C)[None, :]) % ms.size
    m = ms[along]
    P = (m + jb) * sb
    assert P.dtype == np.float32
    assert np.array_equal((P.astype(np.float64) / sb.astype(np.float64)) - jb.astype(np.float64), m.astype(np.float64)), "P is not exact"
    want_q0 = np.floor(m) if rounding == "floor" else np.rint(m)
    return P, s, b, rng.standard_normal((R, C)).astype(np.float32), want_q0
