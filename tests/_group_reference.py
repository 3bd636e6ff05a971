"""NumPy restatement of the clipped b-bit fake-quant with group-wise scales (include/lq_hip.h: lq_fq_forward_group /
lq_fq_backward_group), the reference of tests/test_groupwise_cpu.py (which pins it on a hand-written table and against
tests/_clip_reference.py where the two coincide) and tests/test_gpu_groupwise.py.

The parameter is a matrix [R][C]; axis 0: element (r, c) uses s[r // gs][c], s is [nb][C]; axis 1: s[r][c // gs], s is [R][nb];
nb = ceil(len / gs), the last group of a line may be short.  ``s`` is expanded to the element grid by that index rule, then the
float32 operations are those of _clip_reference.clip_reference (np.rint instead of np.floor for ``rounding="nearest"``):

    t = P / s (float32)    q0 = floor(t) | rint(t)    q = q0 < lo ? lo : (q0 > hi ? hi : q0)    out = q * s (float32)
    inside = (q0 >= lo) & (q0 <= hi)        dP = inside ? dy : +0
    r = inside ? q0 - t (ONE float32 subtraction) : q          ds = k * sum dy * r (float64)       clipped = #{!inside}
"""
import numpy as np

from _clip_reference import bits_equal      # noqa: F401  (re-exported: the tests compare floats bit for bit)


def group_count(length, gs):
    return -(-int(length) // int(gs))


def scale_shape(R, C, axis, gs):
    return (group_count(R, gs), C) if axis == 0 else (R, group_count(C, gs))


def expand_scale(s, R, C, axis, gs):
    """``s`` on the element grid [R][C] by the index rule."""
    s = np.asarray(s, np.float32)
    assert s.shape == scale_shape(R, C, axis, gs), (s.shape, scale_shape(R, C, axis, gs))
    if axis == 0:
        return s[np.arange(R) // gs, :]
    return s[:, np.arange(C) // gs]


def _per_group(x, R, C, axis, gs):
    """Sum of the element grid ``x`` over every group, in the shape of the scale (an explicit loop over the groups of a line)."""
    nb = group_count(R if axis == 0 else C, gs)
    parts = []
    for g in range(nb):
        sl = slice(g * gs, min((g + 1) * gs, R if axis == 0 else C))
        parts.append(x[sl, :].sum(axis=0) if axis == 0 else x[:, sl].sum(axis=1))
    return np.stack(parts, axis=axis)


def group_reference(P, s, dy, qmin, qmax, axis, gs, k=1.0, rounding="floor"):
    """dict(out, q, dP, ds, terms, clipped, inside, q0, r, t): out / q / dP float32 [R][C]; ds (float64), terms = |k| * sum|dy r|
    (float64) and clipped (int64) in the shape of ``s``."""
    P, dy = np.asarray(P, np.float32), np.asarray(dy, np.float32)
    assert P.ndim == 2 and dy.shape == P.shape and axis in (0, 1) and gs >= 1 and rounding in ("floor", "nearest")
    R, C = P.shape
    sb = expand_scale(s, R, C, axis, gs)
    lo, hi = np.float32(qmin), np.float32(qmax)
    assert float(lo) == qmin and float(hi) == qmax
    with np.errstate(all="ignore"):
        t = P / sb
        q0 = np.floor(t) if rounding == "floor" else np.rint(t)
        q = np.where(q0 < lo, lo, np.where(q0 > hi, hi, q0))          # comparisons: a NaN q0 stays NaN, +-Inf saturates
        out = q * sb
        inside = (q0 >= lo) & (q0 <= hi)
        dP = np.where(inside, dy, np.float32(0.0))
        r = np.where(inside, q0 - t, q)
        assert t.dtype == q.dtype == out.dtype == dP.dtype == r.dtype == np.float32
        prod = dy.astype(np.float64) * r.astype(np.float64)
        k64 = float(np.float32(k))                                    # the factor travels as a C float
        ds = _per_group(prod, R, C, axis, gs) * k64
        terms = _per_group(np.abs(prod), R, C, axis, gs) * abs(k64)
        clipped = _per_group((~inside).astype(np.int64), R, C, axis, gs)
    return dict(out=out, q=q, dP=dP, ds=ds, terms=terms, clipped=clipped, inside=inside, q0=q0, r=r, t=t)


def mixed_share(ref, R, C, axis, gs):
    """Share of the groups that hold both clipped and inside elements."""
    n_in = _per_group(ref["inside"].astype(np.int64), R, C, axis, gs)
    return float(np.mean((n_in > 0) & (ref["clipped"] > 0)))


def check_condition(ref, R, C, axis, gs, what):
    """On the REFERENCE, before any kernel runs: the case clips a sizeable share and leaves a sizeable share inside, group by group."""
    length = R if axis == 0 else C
    n = ref["inside"].size
    clipped, inside = int(ref["clipped"].sum()), int(ref["inside"].sum())
    assert clipped + inside == n
    assert clipped >= 0.1 * n and inside >= 0.1 * n, f"{what}: {clipped} clipped, {inside} inside of {n}"
    if min(gs, length) >= 8:
        sizes = np.minimum(gs, length - np.arange(ref["clipped"].shape[axis]) * min(gs, length))
        big = np.broadcast_to(sizes.reshape((-1, 1) if axis == 0 else (1, -1)) >= 8, ref["clipped"].shape)
        n_in = sizes.reshape((-1, 1) if axis == 0 else (1, -1)) - ref["clipped"]
        mixed = (ref["clipped"] > 0) & (n_in > 0)
        share = float(mixed[big].mean())
        assert share >= 0.9, f"{what}: only {share:.3f} of the groups of >= 8 elements hold both clipped and inside elements"
        assert abs(mixed_share(ref, R, C, axis, gs) - float(mixed.mean())) < 1e-12


def make_case(seed, R, C, axis, gs):
    """The inputs of the GPU tests: per-group s = 2^U(-9, -5), P = N(0, 1) * 8 s, dy = N(0, 1)."""
    rng = np.random.default_rng(seed)
    s = np.exp2(rng.uniform(-9.0, -5.0, size=scale_shape(R, C, axis, gs))).astype(np.float32)
    P = (rng.standard_normal((R, C)).astype(np.float32) * (np.float32(8.0) * expand_scale(s, R, C, axis, gs))).astype(np.float32)
    dy = rng.standard_normal((R, C)).astype(np.float32)
    return P, s, dy
