"""NumPy restatement of the per-group quantization statistics (include/lq_hip.h: lq_group_stats), the reference of
tests/test_group_stats_cpu.py (which pins it on a hand-written table) and tests/test_gpu_group_stats.py.

q0, q and out are those of _group_reference.group_reference (no offset) or _group_affine_reference.group_affine_reference (with
one), float32 operation for operation.  On top of them, per group in the scale's shape:

    below = #{q0 < lo}    above = #{q0 > hi}    (int64)
    err2 = sum e * e with e = float64(P) - float64(out)    sig2 = sum float64(P) * float64(P)    (float64, _per_group; a group of one element is the element)

and per tensor hist[q - qmin] = #{elements whose q is a number} (int64, qmax - qmin + 1 bins).
"""
import numpy as np

from _group_affine_reference import group_affine_reference
from _group_reference import _per_group, group_reference

GEOMETRIES = [      # (R, C, axis, gs): the smallest that reach every launch form
    (200, 64, 0, 64), (33000, 4, 0, 1),                              # cols4: ragged last group; second trip of the group loop
    (50, 7, 0, 20), (96, 130, 0, 96),                                # cols1
    (9, 200, 1, 64), (5, 1100, 1, 256), (3, 2600, 1, 1024),          # rows4: team 4, 16, 64
    (70, 12, 1, 3), (7, 333, 1, 50), (3, 1001, 1, 333),              # rows1: team 1, 16, 64 (last group 2)
    (1, 130, 1, 130),                                                # a bias
]
RANGES = [(-8, 7, "floor"), (-8, 7, "nearest"), (0, 15, "floor"), (-2, 1, "floor")]
REL = 2.0 ** -30      # err2 / sig2 against float64: any order of at most 2^20 non-negative f64 terms stays within 2^-32 of the sum


def _sums(x, R, C, axis, gs):
    """_per_group(x); a group of one element is the element itself (its sum adds nothing), without the loop over 33000 groups."""
    return np.array(x) if gs == 1 else _per_group(x, R, C, axis, gs)


def group_stats_reference(P, s, qmin, qmax, axis, gs, b=None, rounding="floor"):
    """dict(below, above: int64 and err2, sig2: float64 in the shape of ``s``; hist: int64 [qmax - qmin + 1]; q0, q, out)."""
    P = np.asarray(P, np.float32)
    R, C = P.shape
    zeros = np.zeros_like(P)
    if b is None:
        ref = group_reference(P, s, zeros, qmin, qmax, axis, gs, rounding=rounding)
    else:
        ref = group_affine_reference(P, s, b, zeros, qmin, qmax, axis, gs, rounding=rounding)
    q0, q, out = ref["q0"], ref["q"], ref["out"]
    lo, hi = np.float32(qmin), np.float32(qmax)
    with np.errstate(all="ignore"):
        below = _sums((q0 < lo).astype(np.int64), R, C, axis, gs)
        above = _sums((q0 > hi).astype(np.int64), R, C, axis, gs)
        e = P.astype(np.float64) - out.astype(np.float64)
        err2 = _sums(e * e, R, C, axis, gs)
        sig2 = _sums(P.astype(np.float64) * P.astype(np.float64), R, C, axis, gs)
    number = ~np.isnan(q)
    hist = np.bincount((q[number].astype(np.int64) - qmin), minlength=qmax - qmin + 1).astype(np.int64)
    assert hist.size == qmax - qmin + 1 and err2.dtype == sig2.dtype == np.float64
    return dict(below=below, above=above, err2=err2, sig2=sig2, hist=hist, q0=q0, q=q, out=out)


def close(got, want, rel=REL):
    """got within ``rel`` of want element by element; NaN matches NaN and Inf matches Inf."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (np.isnan(got) & np.isnan(want)) | (got == want)
    with np.errstate(all="ignore"):
        near = np.abs(got - want) <= rel * np.abs(want)
    return bool(np.all(same | near))
