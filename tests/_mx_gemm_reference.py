"""NumPy reference of the packed MX operands and the block-scaled GEMM (include/lq_hip.h: lq_mx_operand_pack /
lq_mx_operand_quantize / lq_mx_operand_decode / lq_mx_gemm), and the builders of the data sets of tests/test_gpu_mx_gemm.py, so
that tests/test_mx_gemm_cpu.py can assert every data condition without a device.

An operand is held in its LOGICAL form: codes int64 (L, K) and E8M0 bytes int64 (L, ceil(K / 32)), both taken from
tests/_mx_reference.py (mx_reference / init_reference: the definitions the quantizer itself is tested against).  The tile and lane
order of the device buffers never enters: the tests reach them through decode and through the GEMM's results only.
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
    """value(code) * 2^(byte - 127), (L, K); float32: one rounding, as the device multiplies."""
    from learned_quantization_amd import ops
    table = ops.mx_decode_table(op.name)
    K = op.codes.shape[1]
    with np.errstate(all="ignore"):
        scale = np.where(op.bytes == 255, np.nan, np.exp2(op.bytes.astype(np.float64) - 127.0))
        scale = np.repeat(scale, BLOCK, axis=1)[:, :K]
        return (table[op.codes].astype(dtype) * scale.astype(dtype)).astype(dtype)


def gemm_reference(a, b, bias=None):
    """(Y, sum|terms|) in float64 of Y = A B^T (+ bias)."""
    A, B = decode(a), decode(b)
    Y, T = A @ B.T, np.abs(A) @ np.abs(B).T
    if bias is not None:
        Y, T = Y + bias.astype(np.float64)[None, :], T + np.abs(bias.astype(np.float64))[None, :]
    return Y, T


# ----------------------------------------------------------------------------------------------------------------- data sets
PACK_SHAPES = [(70, 40, 0), (160, 17, 0), (9, 200, 1), (33, 288, 1)]      # (R, C, axis): see tests/test_gpu_mx_gemm.py
QUANT_SHAPES = [(5, 100), (33, 288)]
EXACT_SHAPES = [(16, 16, 128), (19, 21, 160), (37, 10, 784), (64, 48, 512)]      # (M, N, K)
EXACT_CASES = [(s, False) for s in EXACT_SHAPES] + [((19, 21, 160), True)]      # (shape, A is the identity pattern)
RANDOM_SHAPES =[(37, 10, 784), (64, 48, 1024)]
# Exact sets.  Elements are 0, +-1, +-1.5, +-2 (on the grid of all three formats), block scales 2^-2 .. 2^3 per block and line:
# a nonzero term |a b| sa sb lies in [2^-4, 2^8], a range of 2^12, and is a multiple of 2^-6.  A sum of K <= 784 of them stays
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
