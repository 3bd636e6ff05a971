"""NumPy restatement of the per-group statistics of the microscaling quantizer (include/lq_hip.h: lq_mx_stats), the reference of
tests/test_mx_stats_cpu.py (which pins it on a hand-written table) and tests/test_gpu_mx_stats.py.

q0, q, out and code are those of _mx_reference.mx_reference, float32 operation for operation.  On top of them, per group in the
scale's shape:

    below = #{q0 < -mx}    above = #{q0 > mx}    flushed = #{P != 0 and q == 0}    (int64)
    err2 = sum e * e with e = float64(P) - float64(out)    sig2 = sum float64(P) * float64(P)    (float64, _per_group)

and per tensor hist[code] = #{elements whose q is a number} (int64, 2^bits bins).

Geometries, the bound on the two sums and its comparison are _group_stats_reference's: the launch rule is the same.
"""
import numpy as np

from _group_reference import _per_group
from _group_stats_reference import GEOMETRIES, REL, _sums, close      # noqa: F401  (re-exported for the two test files)
from _mx_reference import FORMATS, SCALE_FORMATS, loguniform_case, mx_reference

FORM_GEOMETRIES = [(200, 64, 0, 64), (50, 7, 0, 20), (9, 200, 1, 64), (7, 333, 1, 50)]      # one per launch form: cols4, cols1, rows4, rows1
BIAS = (1, 130, 1, 130)


def gpu_cases():
    """[(format, scale format, geometry)] of the parity test of tests/test_gpu_mx_stats.py, each once."""
    cases = [(n, sf, g) for n, sf in (("fp4_e2m1", "e8m0"), ("fp8_e4m3", "fp32")) for g in GEOMETRIES]
    cases += [(n, sf, g) for g in FORM_GEOMETRIES for n in FORMATS for sf in SCALE_FORMATS]
    return list(dict.fromkeys(cases))


def mx_stats_reference(P, s, fmt, scale_format, axis, gs):
    """dict(below, above, flushed: int64 and err2, sig2: float64 in the shape of ``s``; hist: int64 [2^bits]; q0, q, out, code and
    clipped of mx_reference)."""
    P = np.asarray(P, np.float32)
    R, C = P.shape
    ref = mx_reference(P, s, np.zeros_like(P), fmt, scale_format, axis, gs)
    q0, q, out, code = ref["q0"], ref["q"], ref["out"], ref["code"]
    gs = min(gs, R if axis == 0 else C)
    mx = np.float32(fmt.max)
    with np.errstate(all="ignore"):
        below = _sums((q0 < -mx).astype(np.int64), R, C, axis, gs)
        above = _sums((q0 > mx).astype(np.int64), R, C, axis, gs)
        flushed = _sums(((P != 0) & (q == 0)).astype(np.int64), R, C, axis, gs)
        e = P.astype(np.float64) - out.astype(np.float64)
        err2 = _sums(e * e, R, C, axis, gs)
        sig2 = _sums(P.astype(np.float64) * P.astype(np.float64), R, C, axis, gs)
    number = ~np.isnan(q)
    hist = np.bincount(code[number].astype(np.int64), minlength=1 << fmt.bits).astype(np.int64)
    assert hist.size == 1 << fmt.bits and err2.dtype == sig2.dtype == np.float64 and below.shape == np.shape(s)
    return dict(below=below, above=above, flushed=flushed, err2=err2, sig2=sig2, hist=hist, q0=q0, q=q, out=out, code=code,
                clipped=ref["clipped"])


def subnormal_codes(fmt):
    """bool [2^bits]: the codes with exponent field 0 and a non-zero mantissa."""
    mag = np.arange(1 << fmt.bits) & ((1 << (fmt.bits - 1)) - 1)
    return (mag >> fmt.M == 0) & (mag != 0)


_CASES, _REFS = {}, {}


def case(name, scale_format, geo):
    """(P, s) of _mx_reference.loguniform_case, made once per process and never modified."""
    key = (name, scale_format, geo)
    if key not in _CASES:
        P, s, _ = loguniform_case(name, scale_format, *geo)
        P.setflags(write=False)
        s.setflags(write=False)
        _CASES[key] = (P, s)
    return _CASES[key]


def reference(name, scale_format, geo):
    """The reference of ``case``, computed once per process and shared."""
    key = (name, scale_format, geo)
    if key not in _REFS:
        P, s = case(*key)
        _REFS[key] = mx_stats_reference(P, s, FORMATS[name], scale_format, geo[2], geo[3])
    return _REFS[key]
