"""NumPy reference of the packed int8 operands and the int8 GEMM (include/lq_hip.h, "packed int8 operands and the int8 GEMM"), the
yardstick of tests/test_i8_cpu.py (which pins it on hand-worked cases) and tests/test_gpu_i8.py (which compares the device with it
bit for bit).  Everything here is written from the header's text:

  layout    codes [LT][KT][64][16], the byte of (line, k) at
            (((line >> 4) * KT + (k >> 6)) * 64 + 16 * ((k & 63) >> 4) + (line & 15)) * 16 + (k & 15); scales [nbs][16 LT] fp32;
            code 0 past L and K, scale 1.0 for lines past L
  pack      the codes are the int8 view of tests/_group_reference.py's clamped integers, the scales the stored ones
  quantize  tests/_scale_init_reference.py's "absmax" with [-127, 127] and min_value 2^-126, then pack with nearest rounding
  gemm      per period p (ascending k): I_p exact (int64 here, asserted to fit int32), t_p = sa * sb (float32),
            y = y + float32(I_p) * t_p with the product and the sum rounded separately; the bias last

An operand here is a dict(codes int8 [L][K], scales float32 [L][nbs], block).
"""
import numpy as np

from _group_reference import group_reference, scale_shape
from _scale_init_reference import scale_init_reference

MIN_SCALE = float(np.float32(2.0 ** -126))
UNIT = 64            # K of one instruction
MAX_PERIOD = 65536


# ---------------------------------------------------------------------------------------------------------------- layout
def layout_dims(L, K, block):
    assert L > 0 and K > 0 and block >= 0 and block % UNIT == 0
    return -(-L // 16), -(-K // UNIT), (-(-K // block) if block else 1)


def code_offset(KT, line, k):
    """The header's formula, on ints or arrays."""
    return (((line >> 4) * KT + (k >> 6)) * 64 + 16 * ((k & 63) >> 4) + (line & 15)) * 16 + (k & 15)


def pack_layout(op):
    """(code buffer uint8 [LT * KT * 1024], scale buffer float32 [nbs * 16 LT]) of an operand, padding included."""
    codes, scales, block = np.asarray(op["codes"], np.int8), np.asarray(op["scales"], np.float32), op["block"]
    L, K = codes.shape
    LT, KT, nbs = layout_dims(L, K, block)
    assert scales.shape == (L, nbs), (scales.shape, (L, nbs))
    cbuf = np.zeros(LT * KT * 1024, np.uint8)
    ln, k = np.meshgrid(np.arange(L), np.arange(K), indexing="ij")
    cbuf[code_offset(KT, ln, k)] = codes.view(np.uint8)
    sbuf = np.ones((nbs, 16 * LT), np.float32)
    sbuf[:, :L] = scales.T
    return cbuf, sbuf.reshape(-1)


def unpack_layout(cbuf, sbuf, L, K, block):
    LT, KT, nbs = layout_dims(L, K, block)
    cbuf, sbuf = np.asarray(cbuf, np.uint8).reshape(-1), np.asarray(sbuf, np.float32).reshape(nbs, 16 * LT)
    assert cbuf.size == LT * KT * 1024
    ln, k = np.meshgrid(np.arange(L), np.arange(K), indexing="ij")
    return dict(codes=cbuf[code_offset(KT, ln, k)].view(np.int8), scales=np.ascontiguousarray(sbuf[:, :L].T), block=block)


def buffers_mismatch(cbuf, sbuf, op):
    """None if the device buffers are the packed reference byte for byte (NaN scales compared by their bits), else a message."""
    rc, rs = pack_layout(op)
    cbuf = np.asarray(cbuf, np.uint8).reshape(-1)
    sbits = np.asarray(sbuf, np.float32).reshape(-1).view(np.uint32)
    if cbuf.shape != rc.shape or sbits.shape != rs.shape:
        return f"buffer sizes {cbuf.shape} {sbits.shape} != {rc.shape} {rs.shape}"
    if not np.array_equal(cbuf, rc):
        i = int(np.flatnonzero(cbuf != rc)[0])
        return f"{int((cbuf != rc).sum())} code bytes differ, first at {i}: {cbuf[i]} != {rc[i]}"
    same = (sbits == rs.view(np.uint32)) | (np.isnan(rs) & np.isnan(sbits.view(np.float32)))
    if not same.all():
        i = int(np.flatnonzero(~same)[0])
        return f"{int((~same).sum())} scales differ, first at {i}: {sbits.view(np.float32)[i]!r} != {rs[i]!r}"
    return None


# ---------------------------------------------------------------------------------------------------------------- operands
def i8_view(q):
    """The LQ_Q_I8 integer view of clamped grid values: NaN -> 0, else the two's-complement byte."""
    q = np.asarray(q, np.float32)
    return (np.where(np.isnan(q), 0, q).astype(np.int64) & 0xff).astype(np.uint8).view(np.int8)


def operand_of_parameter(P, s, qmin, qmax, axis, gs, rounding):
    """The operand lq_i8_operand_pack writes for parameter P [R][C] under scales s (lq_fq_forward_group's geometry)."""
    P = np.asarray(P, np.float32)
    R, C = P.shape
    length = R if axis == 0 else C
    assert -128 <= qmin <= qmax <= 127 and (gs >= length or gs % UNIT == 0)
    gs_eff = min(gs, length)
    s = np.asarray(s, np.float32).reshape(scale_shape(R, C, axis, gs_eff))
    q = group_reference(P, s, np.zeros_like(P), qmin, qmax, axis, gs_eff, rounding=rounding)["q"]
    codes = i8_view(q)
    return dict(codes=np.ascontiguousarray(codes.T if axis == 0 else codes), scales=np.ascontiguousarray(s.T if axis == 0 else s),
                block=0 if gs >= length else gs)


def fq_out_of_parameter(P, s, qmin, qmax, axis, gs, rounding):
    R, C = P.shape
    gs_eff = min(gs, R if axis == 0 else C)
    return group_reference(P, np.asarray(s, np.float32).reshape(scale_shape(R, C, axis, gs_eff)), np.zeros_like(P), qmin, qmax, axis,
                           gs_eff, rounding=rounding)["out"]


def operand_of_activation(x, block):
    """The operand lq_i8_operand_quantize writes: the composition the header states."""
    x = np.asarray(x, np.float32)
    M, K = x.shape
    gs = block if block else K
    s = scale_init_reference(x, -127, 127, 1, gs, "absmax", min_value=MIN_SCALE)["s"]
    return operand_of_parameter(x, s, -127, 127, 1, gs, "nearest")


def decode(op, dtype=np.float32):
    codes, scales, block = op["codes"], op["scales"], op["block"]
    K = codes.shape[1]
    sb = scales[:, (np.arange(K) // block) if block else np.zeros(K, np.int64)]
    with np.errstate(all="ignore"):
        return codes.astype(dtype) * sb.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- GEMM
def period_of(a_block, b_block, K):
    lo, hi = min(a_block, b_block), max(a_block, b_block)
    if lo > 0 and hi % lo:
        raise ValueError("neither block divides the other")
    F = lo if lo > 0 else hi
    period = min(F, K) if F > 0 else K
    if period > MAX_PERIOD:
        raise ValueError("period above 65536")
    return period


def period_sums(a, b):
    """[(k slice, I int64 [M][N], sum |a||b| int64 [M][N])] per period in ascending k."""
    K = a["codes"].shape[1]
    assert b["codes"].shape[1] == K
    F = period_of(a["block"], b["block"], K)
    A, B = a["codes"].astype(np.int64), b["codes"].astype(np.int64)
    out = []
    for k0 in range(0, K, F):
        ks = slice(k0, min(k0 + F, K))
        out.append((ks, A[:, ks] @ B[:, ks].T, np.abs(A[:, ks]) @ np.abs(B[:, ks]).T))
    return out


def gemm_reference(a, b, bias=None):
    """float32 [M][N]: the definition of lq_i8_gemm."""
    M, N = a["codes"].shape[0], b["codes"].shape[0]
    y = np.zeros((M, N), np.float32)
    with np.errstate(all="ignore"):
        for ks, I, mag in period_sums(a, b):
            assert I.min() >= -2 ** 31 and I.max() < 2 ** 31, "a period sum leaves int32"
            pa = ks.start // a["block"] if a["block"] else 0
            pb = ks.start // b["block"] if b["block"] else 0
            t = a["scales"][:, pa].astype(np.float32)[:, None] * b["scales"][:, pb].astype(np.float32)[None, :]
            term = I.astype(np.float32) * t
            y = y + term
            assert t.dtype == term.dtype == y.dtype == np.float32
        if bias is not None:
            y = y + np.asarray(bias, np.float32)[None, :]
    return y


def gemm_f64(a, b, bias=None):
    """(float64 product of the decoded operands, sum of |terms|): the independent second check."""
    da, db = decode(a, np.float64), decode(b, np.float64)
    with np.errstate(all="ignore"):
        ref, terms = da @ db.T, np.abs(da) @ np.abs(db).T
        if bias is not None:
            ref, terms = ref + np.asarray(bias, np.float64)[None, :], terms + np.abs(np.asarray(bias, np.float64))[None, :]
    return ref, terms


# ---------------------------------------------------------------------------------------------------------------- the GPU data sets
# (M, N, K): one instruction; every edge masked and a third K step half full; the MNIST layer; an idle wave column; a 2 x 2 grid;
# three blocks on one axis, both ways (the kernel's block is 64 x 64 of Y, a wave 32 x 32)
GEMM_SHAPES = [(16, 16, 64), (19, 21, 160), (37, 10, 784), (64, 48, 512), (81, 70, 192), (129, 17, 128), (17, 129, 128)]
BLOCK_PAIRS = [(0, 0), (0, 64), (64, 0), (64, 128), (128, 64), (128, 128)]
BLOCK_PAIR_SHAPE = (37, 21, 320)      # K = 320: the last period of 128 is ragged
EXTREME_K = 65536
PACK_CASES = [(70, 40, 0, 70), (160, 17, 0, 64), (9, 200, 1, 64), (9, 200, 1, 128), (33, 320, 1, 64), (33, 320, 1, 128)]   # (R, C, axis, gs)
PACK_RANGES = [(-128, 127), (-8, 7), (-7, 7)]
QUANT_SHAPES = [(3, 70), (37, 784), (17, 320)]
QUANT_BLOCKS = [0, 64, 128]
LONG_QUANT_SHAPES = [(3, 4100), (2, 4160)]      # rows past the 4096 / 1024 elements a team keeps in registers, block == 0
EXTRA_GEMM_KEYS = [(81, 70, 192, 64, 128), (129, 17, 128, 64, 64)]      # (M, N, K, a_block, b_block)


def random_operand(rng, L, K, block):
    nbs = layout_dims(L, K, block)[2]
    scales = np.exp2(rng.uniform(-6.0, 2.0, (L, nbs))).astype(np.float32)
    return dict(codes=rng.integers(-128, 128, (L, K)).astype(np.int8), scales=scales, block=block)


def gemm_case(M, N, K, a_block=0, b_block=0, seed=0):
    """(a, b, bias) with random codes over the whole byte and random positive scales."""
    rng = np.random.default_rng([seed, M, N, K, a_block, b_block])
    return random_operand(rng, M, K, a_block), random_operand(rng, N, K, b_block), rng.normal(0.0, 50.0, N).astype(np.float32)


def all_gemm_cases():
    return [gemm_case(*s) for s in GEMM_SHAPES] + [gemm_case(*BLOCK_PAIR_SHAPE, a, b) for a, b in BLOCK_PAIRS]


def one_hot_case(k, K=128, M=16, N=16):
    """A is zero except column k = m + 1, B zero except column k = 3 n - 20 (asymmetric: a row / column swap shows)."""
    a, b = np.zeros((M, K), np.int8), np.zeros((N, K), np.int8)
    a[:, k] = np.arange(M) + 1
    b[:, k] = 3 * np.arange(N) - 20
    one = lambda L: np.ones((L, 1), np.float32)
    return dict(codes=a, scales=one(M), block=0), dict(codes=b, scales=one(N), block=0)


def code_sweep_case():
    """Every code -128 .. 127 (the lines of A) against {-128, -1, 1, 127} (the lines of B), one term per output, at k = 37."""
    a, b = np.zeros((256, 64), np.int8), np.zeros((4, 64), np.int8)
    a[:, 37] = np.arange(-128, 128)
    b[:, 37] = [-128, -1, 1, 127]
    return dict(codes=a, scales=np.ones((256, 1), np.float32), block=0), dict(codes=b, scales=np.ones((4, 1), np.float32), block=0)


def extreme_case(bcode):
    a = dict(codes=np.full((16, EXTREME_K), -128, np.int8), scales=np.ones((16, 1), np.float32), block=0)
    b = dict(codes=np.full((16, EXTREME_K), bcode, np.int8), scales=np.ones((16, 1), np.float32), block=0)
    return a, b


def pack_case(R, C, axis, gs, seed=0):
    """(P, s) of a stored parameter: elements over about +-1.3 ranges of an 8-bit grid, one NaN element and one NaN scale in
    different blocks."""
    rng = np.random.default_rng([seed, R, C, axis, gs])
    P = rng.normal(0.0, 1.0, (R, C)).astype(np.float32)
    length = R if axis == 0 else C
    shp = scale_shape(R, C, axis, min(gs, length))
    s = np.exp2(rng.uniform(-7.0, -5.0, shp)).astype(np.float32)
    P[R // 2, C // 3] = np.nan
    s[-1, -1] = np.nan
    return P, s


def quantize_case(M, K, seed=0):
    """x with a zero row, a NaN, an Inf and a row of 1e-40 (a subnormal: the scale is raised to 2^-126)."""
    rng = np.random.default_rng([seed, M, K])
    x = (rng.normal(0.0, 1.0, (M, K)) * np.exp2(rng.integers(-8, 8, (M, 1)))).astype(np.float32)
    x[0] = 0.0
    x[1, K // 2] = np.nan
    x[1, K - 1] = np.inf      # another scale block of the same row where there are blocks
    x[M - 1] = np.float32(1e-40)
    return x
