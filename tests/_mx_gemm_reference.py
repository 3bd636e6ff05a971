"""NumPy reference of the packed MX operands and the block-scaled GEMM (include/lq_hip.h: lq_mx_operand_pack /
lq_mx_operand_quantize / lq_mx_operand_decode / lq_mx_gemm), and the builders of the data sets of tests/test_gpu_mx_gemm.py, so
that tests/test_mx_gemm_cpu.py can assert every data condition without a device.

An operand is held in its LOGICAL form: codes int64 (L, K) and E8M0 bytes int64 (L, ceil(K / 32)), both taken from
tests/_mx_reference.py (mx_reference / init_reference: the definitions the quantizer itself is tested against).  The tile and lane
order of the device buffers enters in ONE place, pack_layout / unpack_layout: a restatement of the text of include/lq_hip.h ("packed
MX operands"), not of csrc/lq_mx_operand.hpp, so that the bytes the device writes are held to the documented format and buffers
built here can be handed to decode and to the GEMM.
Values come from learned_quantization_amd.ops.mx_decode_table; Y and sum|terms| are float64."""
from collections import namedtuple

import numpy as np

import _mx_reference as X
from _bounds import stable_seed

OPERAND_FORMATS = ("fp4_e2m1", "fp8_e4m3", "fp8_e5m2")
PAIRS = [(a, b) for a in OPERAND_FORMATS for b in OPERAND_FORMATS]
BLOCK = 32
MIN_SCALE = float(np.float32(2.0 ** -126))
RefOperand = namedtuple("RefOperand", "codes bytes name out")      # out: lq_fq_forward_mx's `out` in (L, K) order, float32


def scale_bytes(s_eff_lines):
    """E8M0 bytes (L, nb) of effective scales given per element in (L, K) order: the biased exponent, 255 for NaN."""
    s = np.ascontiguousarray(s_eff_lines[:, ::BLOCK], np.float32)
    return np.where(np.isnan(s), 255, (s.view(np.uint32) >> 23).astype(np.int64))


def operand_of_parameter(P, s, name, axis):
    """The operand of parameter P [R][C] under stored scales s (E8M0, blocks of 32 along ``axis``): lines are the columns for
    axis 0 (a Dense kernel (in, out)), the rows for axis 1."""
    ref = X.mx_reference(P, s, np.zeros_like(P), X.FORMATS[name], "e8m0", axis, BLOCK)
    turn = (lambda a: np.ascontiguousarray(a.T)) if axis == 0 else np.ascontiguousarray
    return RefOperand(turn(ref["code"]), scale_bytes(turn(ref["s_eff"])), name, turn(ref["out"]))


def operand_of_activation(x, name, method):
    """The operand of a row-major x (M, K) under lq_scale_init_mx(method, min_value = 2^-126, axis 1, gs 32) then lq_fq_forward_mx."""
    s = X.init_reference(x, X.FORMATS[name], method, 1, BLOCK, MIN_SCALE)
    return operand_of_parameter(x, s, name, 1), s


def decode(op, dtype=np.float64):
    """value(code) * 2^(byte - 127), (L, K): byte 255 is NaN, byte 0 is 2^-127 as OCP defines E8M0.  The float64 product is exact
    (at most 4 significant bits times a power of two); float32 is that product rounded ONCE, as the device's one fp32
    multiplication rounds it -- into the float32 subnormals below 2^-126, to +-Inf from 2^128."""
    from learned_quantization_amd import ops
    table = ops.mx_decode_table(op.name)
    K = op.codes.shape[1]
    with np.errstate(all="ignore"):
        scale = np.where(op.bytes == 255, np.nan, np.ldexp(1.0, (op.bytes - 127).astype(np.int64)))
        scale = np.repeat(scale, BLOCK, axis=1)[:, :K]
        return (table[op.codes].astype(np.float64) * scale).astype(dtype)


def gemm_reference(a, b, bias=None):
    """(Y, sum|terms|) in float64 of Y = A B^T (+ bias)."""
    A, B = decode(a), decode(b)
    Y, T = A @ B.T, np.abs(A) @ np.abs(B).T
    if bias is not None:
        Y, T = Y + bias.astype(np.float64)[None, :], T + np.abs(bias.astype(np.float64))[None, :]
    return Y, T


# ------------------------------------------------------------------------------------- the documented layout (include/lq_hip.h)
def layout_dims(L, K):
    """(LT, KT, KG): tiles of 16 lines, K steps of 128, scale dwords per lane."""
    KT = -(-K // 128)
    return -(-L // 16), KT, -(-KT // 4)


def _layout_offsets(name, L, K):
    """(code byte offset (L, K), nibble shift (L, K), scale byte offset (L, nb)) of every live element and block, from the header:
    fragment `lane` = 16 g + r of tile (lt, kt) holds line 16 lt + r; fp4: k = 32 g + j in nibble j & 1 of byte j >> 1; fp8:
    k = 16 g + j in byte j and k = 64 + 16 g + j in byte 16 + j; byte u of dword `lane` of cell (lt, kg) is block g of K step 4 kg + u."""
    LT, KT, KG = layout_dims(L, K)
    ln, k = np.arange(L, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    lt, r, kt, kk = ln >> 4, ln & 15, k >> 7, k & 127
    if name == "fp4_e2m1":
        g, j = kk >> 5, kk & 31
        off, shift = ((lt * KT + kt) * 64 + 16 * g + r) * 16 + (j >> 1), 4 * (j & 1) + 0 * ln
    else:
        h, g, j = kk >> 6, (kk & 63) >> 4, kk & 15
        off, shift = ((lt * KT + kt) * 64 + 16 * g + r) * 32 + 16 * h + j, 0 * (ln + k)
    kb = np.arange(-(-K // BLOCK), dtype=np.int64)[None, :]
    kt, g = kb >> 2, kb & 3
    soff = ((lt * KG + (kt >> 2)) * 64 + 16 * g + r) * 4 + (kt & 3)
    return off, shift, soff


def pack_layout(codes, bytes_, name):
    """The two uint8 buffers of lq_mx_operand_bytes' sizes that hold the logical operand codes (L, K), bytes (L, ceil(K / 32)) in
    the documented order.  Everything no live (line, k) addresses is code 0 and byte 127: the lines L .. 16 LT - 1, the elements
    past K and the scale bytes of the K steps KT .. 4 KG - 1."""
    codes, bytes_ = np.asarray(codes, np.int64), np.asarray(bytes_, np.int64)
    L, K = codes.shape
    assert name in OPERAND_FORMATS and bytes_.shape == (L, -(-K // BLOCK))
    assert codes.min() >= 0 and codes.max() < (16 if name == "fp4_e2m1" else 256) and bytes_.min() >= 0 and bytes_.max() <= 255
    LT, KT, KG = layout_dims(L, K)
    cbuf = np.zeros(LT * KT * 64 * (16 if name == "fp4_e2m1" else 32), np.uint8)
    sbuf = np.full(LT * KG * 256, 127, np.uint8)
    off, shift, soff = _layout_offsets(name, L, K)
    np.bitwise_or.at(cbuf, off.reshape(-1), (codes << shift).astype(np.uint8).reshape(-1))      # two nibbles share a byte
    assert np.unique(soff).size == soff.size
    sbuf[soff.reshape(-1)] = bytes_.astype(np.uint8).reshape(-1)
    return cbuf, sbuf


def unpack_layout(cbuf, sbuf, name, L, K):
    """The inverse of pack_layout on the live part: (codes (L, K), bytes (L, ceil(K / 32))), int64."""
    cbuf, sbuf = np.asarray(cbuf, np.uint8).reshape(-1), np.asarray(sbuf, np.uint8).reshape(-1)
    LT, KT, KG = layout_dims(L, K)
    assert name in OPERAND_FORMATS and cbuf.size == LT * KT * 64 * (16 if name == "fp4_e2m1" else 32) and sbuf.size == LT * KG * 256
    off, shift, soff = _layout_offsets(name, L, K)
    return (cbuf[off].astype(np.int64) >> shift) & (15 if name == "fp4_e2m1" else 255), sbuf[soff].astype(np.int64)


def layout_mismatch(cbuf, sbuf, ref):
    """None if the device buffers hold exactly pack_layout(ref), padding included; otherwise a message that names the first
    differing (line, k) or (line, block) through unpack_layout, or the first differing padding byte."""
    L, K = ref.codes.shape
    cbuf, sbuf = np.asarray(cbuf, np.uint8).reshape(-1), np.asarray(sbuf, np.uint8).reshape(-1)
    wc, ws = pack_layout(ref.codes, ref.bytes, ref.name)
    if cbuf.size != wc.size or sbuf.size != ws.size:
        return f"sizes ({cbuf.size}, {sbuf.size}), documented ({wc.size}, {ws.size})"
    if np.array_equal(cbuf, wc) and np.array_equal(sbuf, ws):
        return None
    codes, bytes_ = unpack_layout(cbuf, sbuf, ref.name, L, K)
    bad = np.argwhere(codes != ref.codes)
    if bad.size:
        ln, k = bad[0]
        return f"{len(bad)} codes differ, first at (line, k) = ({ln}, {k}): buffer holds {codes[ln, k]}, reference {ref.codes[ln, k]}"
    bad = np.argwhere(bytes_ != ref.bytes)
    if bad.size:
        ln, kb = bad[0]
        return f"{len(bad)} scale bytes differ, first at (line, block) = ({ln}, {kb}): buffer holds {bytes_[ln, kb]}, reference {ref.bytes[ln, kb]}"
    bc, bs = np.flatnonzero(cbuf != wc), np.flatnonzero(sbuf != ws)
    if bc.size:
        return f"{bc.size} padding code bytes are not 0, first at byte {bc[0]}: {cbuf[bc[0]]}"
    return f"{bs.size} padding scale bytes are not 127, first at byte {bs[0]}: {sbuf[bs[0]]}"


# ----------------------------------------------------------------------------------------------------------------- data sets
PACK_SHAPES = [(70, 40, 0), (160, 17, 0), (9, 200, 1), (33, 288, 1)]      # (R, C, axis): see tests/test_gpu_mx_gemm.py
QUANT_SHAPES = [(5, 100), (33, 288)]
EXACT_SHAPES = [(16, 16, 128), (19, 21, 160), (37, 10, 784), (64, 48, 512), (81, 70, 160), (17, 18, 1184), (129, 17, 160),
                (17, 129, 160)]      # (M, N, K)
EXACT_CASES = [(s, False) for s in EXACT_SHAPES] + [((19, 21, 160), True), ((81, 70, 160), True)]      # (shape, A is the identity pattern)
RANDOM_SHAPES =[(37, 10, 784), (64, 48, 1024)]
# the operand-out GEMM (M, N, K): what each exercises is in tests/test_gpu_mx_gemm_fused.py's docstring
FUSED_BIG = (81, 70, 160)
FUSED_SMALL = [(17, 33, 160), (16, 129, 160), (19, 513, 128), (129, 17, 160), (1, 1, 32)]
# Exact sets.  Elements are 0, +-1, +-1.5, +-2 (on the grid of all three formats), block scales 2^-2 .. 2^3 per block and line:
# a nonzero term |a b| sa sb lies in [2^-4, 2^8], a range of 2^12, and is a multiple of 2^-6.  A sum of K <= 1184 of them stays
# far below 2^24 * 2^-6 = 2^18, so every partial sum in every order is a float32: tests/test_mx_gemm_cpu.py asserts it.
EXACT_VALUES = np.array([0.0, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 1.0, -2.0], np.float32)


def _exact_matrix(rng, L, K):
    """(P (L, K) float32, s (L, nb) float32): P = value * scale with value in EXACT_VALUES and scale 2^(-2 .. 3) per (line, block)."""
    nb = -(-K // BLOCK)
    s = np.exp2(rng.integers(-2, 4, size=(L, nb))).astype(np.float32)
    v = EXACT_VALUES[rng.integers(0, EXACT_VALUES.size, size=(L, K))]
    return (v * np.repeat(s, BLOCK, axis=1)[:, :K]).astype(np.float32), s


def exact_case(M, N, K, identity=False):
    """dict(A (M, K), sa (M, nb), W (K, N), sw (nb, N), bias (N,)).  A is packed with axis 1, W -- the Dense kernel (in, out), B's
    lines are its columns -- with axis 0.  ``identity``: A[m][k] = scale * (k == (37 m + 5) mod K), one element per line (37 is
    prime to every K here, so the lines pick different k): Y[m][n] is then a single element of W, which shows any wrong lane map
    outright.  W is random, hence asymmetric."""
    rng = np.random.default_rng(stable_seed("mx-gemm-exact", M, N, K, identity))
    A, sa = _exact_matrix(rng, M, K)
    Bm, sb = _exact_matrix(rng, N, K)
    if identity:
        hot = (37 * np.arange(M) + 5) % K
        assert np.unique(hot).size == M
        A = np.where(np.arange(K)[None, :] == hot[:, None], np.repeat(sa, BLOCK, axis=1)[:, :K], np.float32(0)).astype(np.float32)
    bias = (rng.integers(-16, 17, size=N) * 0.25).astype(np.float32)
    return dict(A=A, sa=sa, W=np.ascontiguousarray(Bm.T), sw=np.ascontiguousarray(sb.T), bias=bias)


def exact_operands(case, aname, bname):
    return operand_of_parameter(case["A"], case["sa"], aname, 1), operand_of_parameter(case["W"], case["sw"], bname, 0)


def sums_f32(terms):
    """The float32 sum of terms (..., K) in natural, reversed and pairwise order."""
    t = np.asarray(terms, np.float32)
    nat, rev = np.zeros(t.shape[:-1], np.float32), np.zeros(t.shape[:-1], np.float32)
    for k in range(t.shape[-1]):
        nat = nat + t[..., k]
        rev = rev + t[..., t.shape[-1] - 1 - k]
    pw = t
    while pw.shape[-1] > 1:
        if pw.shape[-1] % 2:
            pw = np.concatenate([pw, np.zeros(pw.shape[:-1] + (1,), np.float32)], axis=-1)
        pw = pw[..., 0::2] + pw[..., 1::2]
    assert nat.dtype == rev.dtype == pw.dtype == np.float32
    return nat, rev, pw[..., 0]


def random_case(M, N, K, aname, bname, seed=0):
    """dict(x (M, K), W (K, N), sw (nb, N), bias): Gaussian activations (quantised dynamically by the test) and Gaussian weights
    under ``cover`` scales, so that no code saturates and no scale leaves 1 .. 254."""
    rng = np.random.default_rng(stable_seed("mx-gemm-random", M, N, K, aname, bname, seed))
    x = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    sw = X.init_reference(W, X.FORMATS[bname], "cover", 0, BLOCK, MIN_SCALE)
    return dict(x=x, W=W, sw=sw, bias=(rng.standard_normal(N) * 0.1).astype(np.float32))


def pack_case(kind, name, R, C, axis):
    """(P, s) of a pack test: tests/_mx_reference.py's Gaussian or log-uniform set under E8M0 scales."""
    P, s, _ = (X.gaussian_case if kind == "gauss" else X.loguniform_case)(name, "e8m0", R, C, axis, BLOCK)
    return P, s


def quantize_case(M, K):
    """x (M, K): Gaussian rows of very different magnitude, an all-zero block and a block holding an Inf."""
    rng = np.random.default_rng(stable_seed("mx-gemm-quantize", M, K))
    x = (rng.standard_normal((M, K)) * np.exp2(rng.integers(-12, 12, size=(M, 1)))).astype(np.float32)
    x[1, 32:64] = 0.0
    x[M - 1, K - 3] = np.inf
    return x


# ------------------------------------------------------------------------------- one term per output: every code, every scale byte
# Operands that are zero (code 0 under byte 127) except column k0, so that Y[m][n] is ONE product plus zeros and nothing is summed:
# K = 160 is two K steps, the second a quarter full; k0 = 5 and 77 lie in the first and the second half of an fp8 fragment, 133 in the
# second K step.  The buffers come from pack_layout, so codes and bytes no quantizer emits reach the instruction.
SWEEP_K = 160
CODE_K0S = (5, 77, 133)
SCALE_K0 = 77
SCALE_PAIRS = [("fp4_e2m1", "fp4_e2m1"), ("fp8_e4m3", "fp8_e5m2"), ("fp8_e5m2", "fp4_e2m1")]


def _sweep_operand(name, column, k0, line_bytes=None):
    L = len(column)
    codes = np.zeros((L, SWEEP_K), np.int64)
    codes[:, k0] = column
    bytes_ = np.full((L, -(-SWEEP_K // BLOCK)), 127, np.int64)
    if line_bytes is not None:
        bytes_[:, k0 // BLOCK] = line_bytes
    return RefOperand(codes, bytes_, name, None)


def code_sweep_operand(name, k0):
    """One line per code of the format (16 or 256 lines): line i holds code i at k0, every scale byte is 127."""
    return _sweep_operand(name, np.arange(16 if name == "fp4_e2m1" else 256), k0)


def code_of(name, value):
    """The code of a value the format holds exactly."""
    from learned_quantization_amd import ops
    hit = np.flatnonzero(ops.mx_decode_table(name) == np.float32(value))
    assert hit.size == 1, (name, value)
    return int(hit[0])


def scale_sweep_operand(name, negate_odd):
    """256 lines: line i holds 1.5 (-1.5 on odd lines when ``negate_odd``) at SCALE_K0 under byte i (0 .. 255) for that block."""
    sign = np.where((np.arange(256) & 1).astype(bool) & negate_odd, -1.5, 1.5)
    column = np.array([code_of(name, v) for v in sign])
    return _sweep_operand(name, column, SCALE_K0, np.arange(256))


def scale_sweep_classes(ref):
    """(normal, over, under): masks of the finite reference products in [2^-126, 2^128), from 2^128, below 2^-126."""
    mag = np.abs(ref)
    fin = ~np.isnan(ref)
    return fin & (mag >= 2.0 ** -126) & (mag < 2.0 ** 128), fin & (mag >= 2.0 ** 128), fin & (mag < 2.0 ** -126)


def decode_sweep_operand(name):
    """256 lines by K = 256: line i under byte i in all of its blocks, column c holding code c mod 2^bits."""
    n = 16 if name == "fp4_e2m1" else 256
    codes = np.broadcast_to(np.arange(256, dtype=np.int64) % n, (256, 256)).copy()
    return RefOperand(codes, np.repeat(np.arange(256, dtype=np.int64)[:, None], 256 // BLOCK, axis=1), name, None)
