"""NumPy restatement of scale initialisation (include/lq_hip.h: lq_scale_init_group), float32 operation for operation, the
reference of tests/test_scale_init_cpu.py (which pins it on a hand-written table) and tests/test_gpu_scale_init.py.

Geometry as tests/_group_reference.py: P is [R][C]; axis 0: groups of ``gs`` rows per column, s is [nb][C]; axis 1: groups of ``gs``
consecutive elements of a row, s is [R][nb]; gs is clamped to the line length, the last group of a line may be short.  With n the
element count of a group, lo = float32(qmin), hi = float32(qmax), every result is max(s_raw, min_value):

    absmax   ap = max(max P, 0), an = max(max -P, 0);  a = max(qmax > 0 ? ap / hi : 0, qmin < 0 ? an / -lo : 0)   (float32 quotients)
             s_raw = a * float32(1 + 2^-22)                                                                        (one float32 product)
    lsq      s_raw = float32(2 * fsum(|P|) / (n * sqrt(qp))),  qp = qmax > 0 ? qmax : -qmin           (float64, the sum exact: fsum)
    mse      s0 = absmax's s_raw;  k = 0 .. 27:  s_k = max(float32(s0 * c_k), min_value),  c_k = (32 - k) / 32
             out = clamp(floor | rint (P / s_k)) * s_k  (float32, as _group_reference);  E_k = sum (float64(P) - float64(out))^2
             the s_k of the smallest E_k, the smallest k on equal E_k

A group that holds a NaN or an Inf gets NaN.
"""
import math

import numpy as np

from _group_reference import group_count, scale_shape

METHODS = ("absmax", "lsq", "mse")
MIN_VALUE = float(np.float32(float(np.finfo(np.float32).eps) * 100))      # the library's minimum scale
N_CANDIDATES = 28
MARGIN = np.float32(1.0 + 2.0 ** -22)
assert float(MARGIN) == 1.0 + 2.0 ** -22


def _groups(P, axis, gs):
    """(x, mask, nb): the groups of P as rows of ``x`` [lines][nb][gs] (padded with zeros where ``mask`` is False)."""
    P = np.asarray(P, np.float32)
    lines = P.T if axis == 0 else P
    L, n = lines.shape
    gs = min(int(gs), n)
    nb = group_count(n, gs)
    x = np.zeros((L, nb * gs), np.float32)
    m = np.zeros((L, nb * gs), bool)
    x[:, :n] = lines
    m[:, :n] = True
    return x.reshape(L, nb, gs), m.reshape(L, nb, gs), nb


def _to_scale(v, axis):
    """[lines][nb] -> the shape of the scale."""
    return np.ascontiguousarray(v.T if axis == 0 else v)


def _absmax_raw(x, qmin, qmax):
    lo, hi = np.float32(qmin), np.float32(qmax)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        ap = np.fmax(np.fmax.reduce(x, axis=-1), zero)            # fmax skips a NaN: the bad flag has it
        an = np.fmax(np.fmax.reduce(-x, axis=-1), zero)
        qa = ap / hi if qmax > 0 else np.zeros_like(ap)
        qb = an / -lo if qmin < 0 else np.zeros_like(an)
        raw = np.maximum(qa, qb) * MARGIN
    assert raw.dtype == np.float32
    return raw


def _fake_quant(x, s, qmin, qmax, rounding):
    lo, hi = np.float32(qmin), np.float32(qmax)
    with np.errstate(all="ignore"):
        t = x / s
        q0 = np.floor(t) if rounding == "floor" else np.rint(t)
        q = np.where(q0 < lo, lo, np.where(q0 > hi, hi, q0))
        out = q * s
        inside = (q0 >= lo) & (q0 <= hi)
    assert out.dtype == np.float32
    return out, inside


def candidate(s0, k, min_value=MIN_VALUE):
    ck = np.float32((32 - k) / 32.0)
    assert float(ck) == (32 - k) / 32.0
    with np.errstate(all="ignore"):
        return np.maximum(np.asarray(s0, np.float32) * ck, np.float32(min_value))


def scale_init_reference(P, qmin, qmax, axis, gs, method, rounding="floor", min_value=MIN_VALUE):
    """dict(s: float32 in the shape of the scale; bad: bool, the group holds a NaN or an Inf).  For "mse" also k (the chosen
    candidate), runner (the scale of the second-best candidate), gap (relative gap (E_second - E_best) / E_best, 0 when both
    are equal, inf when only E_best is 0) and E_best."""
    P = np.asarray(P, np.float32)
    assert P.ndim == 2 and axis in (0, 1) and gs >= 1 and method in METHODS and rounding in ("floor", "nearest")
    R, C = P.shape
    x, m, nb = _groups(P, axis, gs)
    mv = np.float32(min_value)
    assert mv > 0 and np.isfinite(mv)
    bad = (~np.isfinite(x)).any(axis=-1)
    nan = np.float32(np.nan)
    res = {}
    if method == "absmax":
        raw = _absmax_raw(x, qmin, qmax)
    elif method == "lsq":
        qp = qmax if qmax > 0 else -qmin
        n = m.sum(axis=-1)
        raw = np.zeros(bad.shape, np.float32)
        ax = np.abs(x).astype(np.float64)
        for i in range(raw.shape[0]):
            for g in range(nb):
                if not bad[i, g]:
                    raw[i, g] = np.float32(2.0 * math.fsum(ax[i, g, :n[i, g]]) / (float(n[i, g]) * math.sqrt(float(qp))))
    else:
        s0 = _absmax_raw(x, qmin, qmax)
        x64 = x.astype(np.float64)
        E = np.empty((N_CANDIDATES,) + s0.shape, np.float64)
        S = np.empty((N_CANDIDATES,) + s0.shape, np.float32)
        for k in range(N_CANDIDATES):
            S[k] = candidate(s0, k, min_value)
            out, _ = _fake_quant(x, S[k][..., None], qmin, qmax, rounding)
            with np.errstate(all="ignore"):
                d = x64 - out.astype(np.float64)
                E[k] = np.where(m, d * d, 0.0).sum(axis=-1)
        Ef = np.where(np.isnan(E), np.inf, E)
        k1 = np.argmin(Ef, axis=0)                                  # the first of equal minima: the smallest k
        e1 = np.take_along_axis(Ef, k1[None], axis=0)[0]
        rest = Ef.copy()
        np.put_along_axis(rest, k1[None], np.inf, axis=0)
        k2 = np.argmin(rest, axis=0)
        e2 = np.take_along_axis(Ef, k2[None], axis=0)[0]
        with np.errstate(all="ignore"):
            gap = np.where(e2 == e1, 0.0, np.where(e1 > 0, (e2 - e1) / e1, np.inf))
        raw = np.take_along_axis(S, k1[None], axis=0)[0]
        res.update(k=_to_scale(k1, axis), runner=_to_scale(np.take_along_axis(S, k2[None], axis=0)[0], axis),
                   gap=_to_scale(gap, axis), E_best=_to_scale(e1, axis))
    s = np.where(bad, nan, np.maximum(raw, mv)).astype(np.float32)
    res.update(s=_to_scale(s, axis), bad=_to_scale(bad, axis))
    assert res["s"].shape == scale_shape(R, C, axis, min(gs, R if axis == 0 else C))
    return res


def squared_error(P, out, axis, gs):
    """sum (P - out)^2 per group in float64, in the shape of the scale."""
    P = np.asarray(P, np.float32)
    d = P.astype(np.float64) - np.asarray(out, np.float32).astype(np.float64)
    x, m, _ = _groups(np.zeros_like(P), axis, gs)
    lines = (d * d).T if axis == 0 else d * d
    e = np.zeros(x.shape[0:1] + (x.shape[1] * x.shape[2],), np.float64)
    e[:, :lines.shape[1]] = lines
    return _to_scale(e.reshape(x.shape).sum(axis=-1), axis)


def clipped_after(P, s, qmin, qmax, axis, gs, rounding):
    """(clipped mask [R][C], P) of the clipped quantizer under the scale matrix ``s``."""
    from _group_reference import expand_scale
    P = np.asarray(P, np.float32)
    R, C = P.shape
    gs = min(gs, R if axis == 0 else C)
    _, inside = _fake_quant(P, expand_scale(s, R, C, axis, gs), qmin, qmax, rounding)
    return ~inside


# ---- the cases of tests/test_gpu_scale_init.py; tests/test_scale_init_cpu.py checks the conditions on them without a GPU ----
# the small shapes of test_gpu_groupwise.py, (33000, 4, 1): the second trip of the column form's grid-stride group loop (from
# 32 768 groups), (1, 130, 130): the bias line, (1, 70000, 70000): one team of 64 lanes walking a long line
AXIS0 = [(37, 5, 8), (256, 260, 32), (130, 1028, 128), (300, 64, 1), (96, 130, 96), (50, 12, 64), (33000, 4, 1)]
AXIS1 = [(7, 27, 8), (64, 576, 128), (33, 4100, 128), (40, 64, 4), (16, 100, 1), (20, 96, 96), (1, 130, 130), (1, 70000, 70000)]
RANGES = [(-8, 7), (0, 15), (-2, 1)]
ROUNDINGS = ("floor", "nearest")
GAP = 1e-9      # tie-insensitivity of the mse choice: 2000 x the f64 summation bound n * 2^-53 of the largest test group (70 000)
GEOMETRIES = [(R, C, 0, gs) for R, C, gs in AXIS0] + [(R, C, 1, gs) for R, C, gs in AXIS1]

_INPUTS = {}
_REFS = {}


def make_input(R, C, axis, gs):
    """P = N(0, 1) * 0.05 as float32, one array per geometry (shared, never modified)."""
    from _bounds import stable_seed
    key = (R, C, axis, gs)
    if key not in _INPUTS:
        rng = np.random.default_rng(stable_seed("scale_init", R, C, axis, gs))
        P = (rng.standard_normal((R, C)) * 0.05).astype(np.float32)
        P.setflags(write=False)
        _INPUTS[key] = P
    return _INPUTS[key]


def case_reference(R, C, axis, gs, qmin, qmax, method, rounding="floor"):
    """The reference of one case, computed once per process and shared."""
    key = (R, C, axis, gs, qmin, qmax, method, rounding if method == "mse" else "floor")
    if key not in _REFS:
        _REFS[key] = scale_init_reference(make_input(R, C, axis, gs), qmin, qmax, axis, gs, method, rounding=key[-1])
    return _REFS[key]
