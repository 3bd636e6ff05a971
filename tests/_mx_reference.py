"""NumPy restatement of the OCP microscaling quantizer (include/lq_hip.h: lq_fq_forward_mx / lq_fq_backward_mx /
lq_scale_init_mx), the reference of tests/test_mx_cpu.py (which pins it against independent sources) and tests/test_gpu_mx.py,
and the builders of their data sets, so that the CPU file can assert every data condition without a device.

Geometry is tests/_group_reference.py's: a matrix [R][C], axis 0: s[r // gs][c], axis 1: s[r][c // gs].  Per element, in float32:

    t = P / s_eff    a = |t|    e = max(exponent field of a, emin)    u = 2^(e - M)    q0 = copysign(rint(a / u) * u, t)
    inside = |q0| <= mx    q = q0 < -mx ? -mx : (q0 > mx ? mx : q0)    out = q * s_eff    dP = inside ? dy : +0
    r = inside ? q0 - t : q    ds = k * sum dy * r (float64)    clipped = #{!inside}
"""
from collections import namedtuple

import numpy as np

from _bounds import stable_seed
from _group_reference import _per_group, expand_scale, scale_shape

Format = namedtuple("Format", "id bits E M emin emax max mm")
FORMATS = {
    "fp4_e2m1": Format(0, 4, 2, 1, 0, 2, 6.0, 1.5),
    "fp6_e2m3": Format(1, 6, 2, 3, 0, 2, 7.5, 1.875),
    "fp6_e3m2": Format(2, 6, 3, 2, -2, 4, 28.0, 1.75),
    "fp8_e4m3": Format(3, 8, 4, 3, -6, 8, 448.0, 1.75),
    "fp8_e5m2": Format(4, 8, 5, 2, -14, 15, 57344.0, 1.75),
}
FINITE_CODES = {"fp4_e2m1": 16, "fp6_e2m3": 64, "fp6_e3m2": 64, "fp8_e4m3": 254, "fp8_e5m2": 248}
SCALE_FORMATS = ("e8m0", "fp32")
NAN32 = np.float32(np.nan)


def e8m0_round(s):
    """s_eff of LQ_SCALE_E8M0: the nearest power of two in the log domain, NaN for a scale that is not positive, normal and finite
    or that rounds past 2^127."""
    b = np.ascontiguousarray(s, np.float32).view(np.uint32).astype(np.uint64)
    valid = (b >= 0x00800000) & (b < 0x7F800000)
    nb = (b + 0x004AFB0D) & 0x7F800000
    ok = valid & (nb < 0x7F800000)
    return np.where(ok, nb.astype(np.uint32).view(np.float32), NAN32).astype(np.float32)


def effective_scale(s, scale_format):
    assert scale_format in SCALE_FORMATS
    return e8m0_round(s) if scale_format == "e8m0" else np.asarray(s, np.float32)


def round_to_grid(t, fmt):
    """q0: float32 ``t`` on the element grid of ``fmt``, unclamped, by the definition's own operations."""
    t = np.asarray(t, np.float32)
    a = np.abs(t)
    field = ((a.view(np.uint32) >> 23) & 0xFF).astype(np.int32) - 127
    e = np.maximum(field, fmt.emin)
    u = np.ldexp(np.float32(1.0), e - fmt.M).astype(np.float32)
    with np.errstate(all="ignore"):
        q0 = np.copysign(np.rint(a / u) * u, t)
    assert q0.dtype == np.float32
    return q0


def encode(q, fmt):
    """The encoding of clamped grid values ``q`` (int64): sign, exponent and mantissa fields; a NaN gets all ones below the sign."""
    q = np.asarray(q, np.float32)
    nan = np.isnan(q)
    a = np.where(nan, np.float32(0), np.abs(q)).astype(np.float64)
    _, e2 = np.frexp(a)
    e = e2.astype(np.int64) - 1
    small = a < 2.0 ** fmt.emin
    mag_small = a * 2.0 ** (fmt.M - fmt.emin)
    mag_norm = (e - fmt.emin + 1) * 2.0 ** fmt.M + (a * np.exp2((fmt.M - e).astype(np.float64)) - 2.0 ** fmt.M)
    mag = np.where(small, mag_small, mag_norm)
    assert np.all(mag == np.floor(mag)), "a value off the element grid"
    code = np.signbit(q).astype(np.int64) * (1 << (fmt.bits - 1)) + mag.astype(np.int64)
    return np.where(nan, (1 << (fmt.bits - 1)) - 1, code)


def decode_table(fmt):
    """float32 [2^bits]: the value of every code (NaN and +-Inf where the format has them: the fp8 formats)."""
    codes = np.arange(1 << fmt.bits)
    sign = np.where(codes >> (fmt.bits - 1), -1.0, 1.0)
    mag = codes & ((1 << (fmt.bits - 1)) - 1)
    ef, mf = mag >> fmt.M, mag & ((1 << fmt.M) - 1)
    val = np.where(ef == 0, mf * 2.0 ** (fmt.emin - fmt.M), (1.0 + mf / 2.0 ** fmt.M) * np.exp2((ef - 1 + fmt.emin).astype(np.float64)))
    if fmt.id == 3:                                    # e4m3fn: S.1111.111 is NaN, there is no Inf
        val = np.where(mag == 127, np.nan, val)
    if fmt.id == 4:                                    # e5m2: the top exponent holds Inf and NaN
        val = np.where(ef == 31, np.where(mf == 0, np.inf, np.nan), val)
    return (sign * val).astype(np.float32)


def grid(fmt):
    """The non-negative finite values of the format in ascending order (float64)."""
    v = decode_table(fmt)[: 1 << (fmt.bits - 1)].astype(np.float64)
    return np.sort(v[np.isfinite(v)])


def mx_reference(P, s, dy, fmt, scale_format, axis, gs, k=1.0):
    """dict(out, code, dP, ds, terms, clipped, inside, q0, q, t, s_eff): out / dP float32 [R][C], code int64 [R][C]; ds (float64),
    terms = |k| * sum|dy r| (float64) and clipped (int64) in the shape of ``s``; s_eff on the element grid."""
    P, dy = np.asarray(P, np.float32), np.asarray(dy, np.float32)
    assert P.ndim == 2 and dy.shape == P.shape and axis in (0, 1) and gs >= 1
    R, C = P.shape
    gs = min(gs, R if axis == 0 else C)
    sb = expand_scale(effective_scale(s, scale_format), R, C, axis, gs)
    mx = np.float32(fmt.max)
    with np.errstate(all="ignore"):
        t = P / sb
        q0 = round_to_grid(t, fmt)
        inside = np.abs(q0) <= mx
        q = np.where(q0 < -mx, -mx, np.where(q0 > mx, mx, q0))
        out = q * sb
        dP = np.where(inside, dy, np.float32(0.0))
        r = np.where(inside, q0 - t, q)
        assert t.dtype == q.dtype == out.dtype == dP.dtype == r.dtype == np.float32
        prod = dy.astype(np.float64) * r.astype(np.float64)
        k64 = float(np.float32(k))
        ds = _per_group(prod, R, C, axis, gs) * k64
        terms = _per_group(np.abs(prod), R, C, axis, gs) * abs(k64)
        clipped = _per_group((~inside).astype(np.int64), R, C, axis, gs)
    return dict(out=out, code=encode(q, fmt), dP=dP, ds=ds, terms=terms, clipped=clipped, inside=inside, q0=q0, q=q, t=t, s_eff=sb)


def init_reference(P, fmt, method, axis, gs, min_value):
    """lq_scale_init_mx: float32 in the scale's shape.  method "mx": 2^(e - emax); "cover": one binade up where m > mm."""
    assert method in ("mx", "cover")
    P = np.asarray(P, np.float32)
    R, C = P.shape
    length = R if axis == 0 else C
    gs = min(gs, length)
    out = np.empty(scale_shape(R, C, axis, gs), np.float32)
    for g in range(out.shape[axis]):
        sl = slice(g * gs, min((g + 1) * gs, length))
        block = P[sl, :] if axis == 0 else P[:, sl]
        bad = ~np.isfinite(block).all(axis=axis)
        A = np.abs(np.where(np.isfinite(block), block, 0)).max(axis=axis).astype(np.float64)
        mant, ex = np.frexp(A)                           # A = mant * 2^ex, mant in [0.5, 1): m = 2 mant, e = ex - 1
        m, e = 2.0 * mant, ex.astype(np.int64) - 1
        pe = e - fmt.emax + ((m > fmt.mm) if method == "cover" else 0)
        p = np.exp2(np.maximum(pe, -126).astype(np.float64))
        res = np.where(A == 0, min_value, np.maximum(p, float(np.float32(min_value))))
        res = np.where(bad, np.nan, res).astype(np.float32)
        if axis == 0:
            out[g, :] = res
        else:
            out[:, g] = res
    return out


# ----------------------------------------------------------------------------------------------------------------- data sets
GAUSS_SHAPES = [(96, 64, 0, 32), (9, 200, 1, 64)]
FULL_COVER_SHAPE = (96, 64, 0, 32)
WINDOW_SHAPES = [(200, 64, 0, 64), (96, 130, 0, 96), (9, 200, 1, 64), (11, 203, 1, 30)]      # tests/_group_forms.py: cols4, cols1, rows4, rows1
RAGGED_SHAPES = [(69, 128, 0, 32), (5, 100, 1, 32)]      # a last group of 5 rows on the column form; of one float4 on the row form


LAYER_CASES = [("fp4_e2m1", "e8m0", (70, 40, 0, 32)), ("fp8_e4m3", "fp32", (70, 40, 0, 32)), ("fp6_e2m3", "e8m0", (8, 45, 1, 32))]
CONTRACT_CASES = [("fp6_e3m2", "e8m0", (69, 128, 0, 32)), ("fp6_e3m2", "e8m0", (9, 200, 1, 64))]


def gaussian_cases():
    """[(format, scale format, (R, C, axis, gs))]: every Gaussian data set tests/test_gpu_mx.py runs, each once."""
    from _group_forms import FORM_CASES, LARGE
    cases = [("fp4_e2m1", "e8m0", g) for g in FORM_CASES if g != LARGE]
    cases += [(n, sf, g) for g in WINDOW_SHAPES for n in FORMATS for sf in SCALE_FORMATS]
    cases += [(n, "e8m0", g) for g in RAGGED_SHAPES for n in FORMATS]
    return list(dict.fromkeys(cases + LAYER_CASES + CONTRACT_CASES))


def loguniform_shapes(name):
    """Where the log-uniform set runs: the window shapes (1800 elements and more) in every format; the two ragged shapes where the
    tensor can hold 95 % of the codes at all -- (5, 100, 1, 32) has 500 elements, fewer than two per code of an fp8 format and
    eight per code of an fp6 one, so it runs in fp4_e2m1 alone (the Gaussian set runs there in every format)."""
    return WINDOW_SHAPES + [RAGGED_SHAPES[0]] + ([RAGGED_SHAPES[1]] if name == "fp4_e2m1" else [])


def _scales(rng, R, C, axis, gs):
    return np.exp2(rng.uniform(-9.0, -5.0, size=scale_shape(R, C, axis, min(gs, R if axis == 0 else C)))).astype(np.float32)


def gaussian_case(name, scale_format, R, C, axis, gs):
    """(P, s, dy): s = 2^U(-9, -5), P = N(0, 1) * 2^(emax + 1) * s_eff, dy = N(0, 1)."""
    fmt = FORMATS[name]
    rng = np.random.default_rng(stable_seed("mx-gauss", name, scale_format, R, C, axis, gs))
    s = _scales(rng, R, C, axis, gs)
    sb = expand_scale(effective_scale(s, scale_format), R, C, axis, min(gs, R if axis == 0 else C))
    P = (rng.standard_normal((R, C)).astype(np.float32) * (np.float32(2.0 ** (fmt.emax + 1)) * sb)).astype(np.float32)
    return P, s, rng.standard_normal((R, C)).astype(np.float32)


def loguniform_case(name, scale_format, R, C, axis, gs):
    """(P, s, dy): |P| = s_eff * 2^U(emin - M - 3, emax + 2), random sign: subnormals, flush to zero, every binade, saturation."""
    fmt = FORMATS[name]
    rng = np.random.default_rng(stable_seed("mx-loguniform", name, scale_format, R, C, axis, gs))
    s = _scales(rng, R, C, axis, gs)
    sb = expand_scale(effective_scale(s, scale_format), R, C, axis, min(gs, R if axis == 0 else C))
    mag = np.exp2(rng.uniform(fmt.emin - fmt.M - 3, fmt.emax + 2, size=(R, C))).astype(np.float32)
    sign = np.where(rng.random((R, C)) < 0.5, np.float32(-1), np.float32(1))
    return (sign * mag * sb).astype(np.float32), s, rng.standard_normal((R, C)).astype(np.float32)


def code_coverage(ref, name):
    """Share of the format's finite codes that occur in the reference's code view."""
    finite = np.isfinite(decode_table(FORMATS[name]))
    seen = np.zeros(finite.size, bool)
    seen[np.unique(ref["code"])] = True
    return float((seen & finite).sum()) / FINITE_CODES[name]


def midpoints(fmt):
    """Every midpoint between adjacent non-negative grid values, and the first one beyond the format's max (float64, exact)."""
    g = grid(fmt)
    beyond = g[-1] + 2.0 ** (fmt.emax - fmt.M)
    g = np.append(g, beyond)
    return (g[:-1] + g[1:]) / 2.0


def ties_case(name, R, C, axis, gs):
    """(P, s, dy, n_mid): E8M0 scales; the elements of every group run through (mid * s_eff, the float below, the float above) for
    the midpoints of the grid with both signs; group k (in the scale's memory order) starts where group k - 1 stopped, so that
    the tensor holds every midpoint; dy == 1 so that dP shows `inside`."""
    fmt = FORMATS[name]
    rng = np.random.default_rng(stable_seed("mx-ties", name, R, C, axis, gs))
    s = _scales(rng, R, C, axis, gs)
    gs_c = min(gs, R if axis == 0 else C)
    sb = expand_scale(e8m0_round(s), R, C, axis, gs_c)
    mid = midpoints(fmt)
    mids = np.concatenate([mid, -mid]).astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), np.concatenate([mid, -mid])), "a midpoint is not a float32"
    assert gs_c >= 3, "a group holds one triple at least"
    length = R if axis == 0 else C
    lens = np.minimum(gs_c, length - np.arange(s.shape[axis]) * gs_c)                 # the last group of a line may be short
    triples = np.broadcast_to((lens // 3).reshape((-1, 1) if axis == 0 else (1, -1)), s.shape).reshape(-1)
    assert triples.sum() >= mids.size, "too few whole triples for the midpoints"
    first = ((np.cumsum(triples) - triples) % mids.size).reshape(s.shape).astype(np.float32)
    rot = expand_scale(first, R, C, axis, gs_c).astype(np.int64)
    along = (np.arange(R) % gs_c)[:, None] if axis == 0 else (np.arange(C) % gs_c)[None, :]
    pos = 3 * rot + along
    idx = pos % (3 * mids.size)
    c = mids[idx // 3] * sb
    assert c.dtype == np.float32
    down, up = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
    which = idx % 3
    P = np.where(which == 0, c, np.where(which == 1, down, up)).astype(np.float32)
    return P, s, np.ones((R, C), np.float32), mids.size
