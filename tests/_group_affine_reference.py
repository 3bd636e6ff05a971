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

from _bounds import stable_seed
from _group_forms import edge_scales, interleave_bad_scales
from _group_reference import _per_group, expand_scale, make_case, scale_shape
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


# ------------------------------------------------------------ the inputs of tests/test_gpu_group_affine_forms.py: edge quotients
def edge_offset_data(sb, bb, pos, qmin, qmax, rounding):
    """_group_forms.edge_data with an offset: element with sequence position ``pos`` holds member pos % 3 of triple
    (pos // 3) % (qmax - qmin + 5): c = fl32(fl32(m * s) + b), the float below c, the float above c, with m = n (floor) or n + 1/2
    (nearest) and n running over [qmin - 2, qmax + 2]; ``sb`` / ``bb``: scale and offset of every element.  Returns (P, share): the
    share of the triples (by their c elements) whose two neighbours round to different integers under the reference's arithmetic,
    rnd((down - b) / s) != rnd((up - b) / s), every operation in float32.  An ulp of P is not an ulp of u = P - b: where |P| is
    well below |u| both neighbours give the same u, so the share is lower than edge_data's."""
    sb, bb = np.asarray(sb, np.float32), np.asarray(bb, np.float32)
    count = qmax - qmin + 5
    idx = np.asarray(pos, np.int64) % (3 * count)
    m = ((qmin - 2) + idx // 3).astype(np.float32) + np.float32(0.5 if rounding == "nearest" else 0.0)
    c = (m * sb) + bb
    assert c.dtype == np.float32
    down, up = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
    which = idx % 3
    P = np.where(which == 0, c, np.where(which == 1, down, up)).astype(np.float32)
    rnd = np.floor if rounding == "floor" else np.rint
    with np.errstate(all="ignore"):
        straddle = rnd((down - bb) / sb) != rnd((up - bb) / sb)
    return P, float(straddle[which == 0].mean())


def edge_offset_case(seed, R, C, axis, gs, qmin, qmax, rounding):
    """(P, s, b, dy, share): per-group s = 2^U(-12, 3) with full mantissas (_group_forms.edge_scales), b = fl32(U(-6, 6) * s), and
    the triples of edge_offset_data, every group starting at a random triple."""
    rng = np.random.default_rng(seed)
    shape = scale_shape(R, C, axis, gs)
    s = edge_scales(rng, shape)
    b = (rng.uniform(-6.0, 6.0, size=shape).astype(np.float32) * s).astype(np.float32)
    first = rng.integers(0, qmax - qmin + 5, size=shape).astype(np.float32)      # carried on the grid by the scale's index rule
    rot = expand_scale(first, R, C, axis, gs).astype(np.int64)
    along = (np.arange(R) % gs)[:, None] if axis == 0 else (np.arange(C) % gs)[None, :]
    P, share = edge_offset_data(expand_scale(s, R, C, axis, gs), expand_scale(b, R, C, axis, gs), 3 * rot + along, qmin, qmax, rounding)
    return P, s, b, rng.standard_normal((R, C)).astype(np.float32), share


# ------------------------------------------------------- u = P - b outside the fast-division window, bad scales next to offsets
def _pow2(e):
    return np.float32(2.0 ** e)


_BIG = np.float32(3e38)
_SMALL_B = np.float32(1.5 * 2.0 ** -120)      # a normal float whose neighbours are 2^-143 away
# (name, the group's offset or None for the ordinary one it has, P as a function of the offset, the u = fl32(P - b) this gives)
PLANTED_U = [
    ("2^-81", _pow2(-60), lambda b: b + _pow2(-81), _pow2(-81)),
    ("2^-80", -_pow2(-60), lambda b: b + _pow2(-80), _pow2(-80)),
    ("2^81", None, lambda b: _pow2(81), _pow2(81)),
    ("below 2^81", None, lambda b: np.nextafter(_pow2(81), np.float32(0)), np.nextafter(_pow2(81), np.float32(0))),
    ("denormal", _SMALL_B, lambda b: np.nextafter(b, np.float32(np.inf)), _pow2(-143)),      # from two ordinary (normal) operands
    ("+0", None, lambda b: b, np.float32(0.0)),                                             # P == b, b != 0
    ("+Inf", -_BIG, lambda b: _BIG, np.float32(np.inf)),                                    # overflow of two finite operands
    ("-Inf", _BIG, lambda b: -_BIG, np.float32(-np.inf)),
    ("NaN", np.float32(np.inf), lambda b: np.float32(np.inf), np.float32(np.nan)),          # Inf - Inf
]


def window_offset_case(seed, R, C, axis, gs, per_value=3):
    """(P, s, b, dy, bad, planted): make_affine_case with the values of BAD_SCALES interleaved (interleave_bad_scales: axis 0 one
    of the four divisors of a float4, axis 1 every other group; ``bad`` in the shape of s) and, in groups with an ordinary scale,
    elements planted so that u = fl32(P - b) is each value of PLANTED_U.  A value that needs an offset of its own (a tiny one
    for 2^-81, 2^-80 and the denormal, +-3e38 and Inf for the overflow and Inf - Inf) gets a whole group: its offset is replaced,
    and with a tiny offset the group's ordinary elements move along (P = fl32(fl32(P - b_old) + b_new)), so that they stay
    ordinary quotients.  Every offset stays non-zero.  ``planted``: {name: [(r, c)]}, up to ``per_value`` elements per value, no two
    planted elements in one aligned float4 of a row; on axis 0 no two chosen groups share a float4 of columns either."""
    P, s, b, dy = make_affine_case(seed, R, C, axis, gs)
    rng = np.random.default_rng(seed + 1)
    s, bad = interleave_bad_scales(s, C, axis)
    good = np.argwhere(~bad)
    good = good[rng.permutation(len(good))]
    groups, seen = [], set()
    for g0, g1 in good.tolist():
        key = g1 // 4 if axis == 0 else (g0, g1)
        if key not in seen:
            seen.add(key)
            groups.append((g0, g1))
        if len(groups) == len(PLANTED_U):
            break
    assert len(groups) == len(PLANTED_U), "too few groups with an ordinary scale"
    length = R if axis == 0 else C
    gs = min(gs, length)
    planted, quads = {}, set()
    for (name, b_new, make_p, _), (g0, g1) in zip(PLANTED_U, groups):
        g = g0 if axis == 0 else g1
        run = np.arange(g * gs, min((g + 1) * gs, length))
        els = [(int(r), g1) for r in run] if axis == 0 else [(g0, int(c)) for c in run]
        if b_new is not None:
            if abs(float(b_new)) < 1.0:
                for r, c in els:
                    P[r, c] = (P[r, c] - b[g0, g1]) + b_new
            b[g0, g1] = b_new
        planted[name] = []
        for j in rng.permutation(len(els)).tolist():
            r, c = els[j]
            if (r, c // 4) not in quads:
                quads.add((r, c // 4))
                P[r, c] = make_p(b[g0, g1])
                planted[name].append((r, c))
            if len(planted[name]) == per_value:
                break
    assert P.dtype == b.dtype == np.float32 and np.all(b != 0)
    return P, s, b, dy, bad, planted


# ------------------------------------------------------------------------------------------------ the two batches of that file
def form_batch_factors(n):
    """[(grad_scale, offset_grad_scale)] of the n tensors of the every-form batch: 1 + (i + 1) / 32 and 2 - (i + 1) / 64 (no
    tensor's two factors are equal, and no two tensors share one)."""
    return [(float(np.float32(1.0 + (i + 1) / 32.0)), float(np.float32(2.0 - (i + 1) / 64.0))) for i in range(n)]


FULL_BATCH = 256              # the capacity of the by-value tables PtrPack / CoefPack
FULL_BATCH_SYMMETRIC = 8      # every eighth tensor of the full batch has no offset


def full_batch_factors(i):
    """(grad_scale, offset_grad_scale) of tensor i of the full batch: 1 + i / 256 and 2 - i / 256, both exact in float32."""
    return float(np.float32(1.0 + i / 256.0)), float(np.float32(2.0 - i / 256.0))


def full_batch_inputs(i, geom):
    """(P, s, b | None, dy) of tensor i of the full batch, its own data; every FULL_BATCH_SYMMETRIC-th tensor is symmetric."""
    seed = stable_seed("affine full batch", i)
    if i % FULL_BATCH_SYMMETRIC == 0:
        P, s, dy = make_case(seed, *geom)
        return P, s, None, dy
    return make_affine_case(seed, *geom)
