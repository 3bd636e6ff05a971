"""NumPy reference of the int8 operands with offsets and of the int8 GEMM's offset term (include/lq_hip.h, "offsets on the B
operand"), the yardstick of tests/test_i8_affine_cpu.py (which pins it on a hand-worked case) and tests/test_gpu_i8_affine.py
(which compares the device with it bit for bit).  Written from the header's text, on top of tests/_i8_reference.py:

  operand   dict(codes int8 [L][K], scales float32 [L][nbs], offsets float32 [L][nbs], block); the offsets buffer has the layout of
            the scales buffer, +0 for lines past L
  pack      the codes are the int8 view of tests/_group_affine_reference.py's clamped integers, scales and offsets the stored ones
  decode    float32(float32(code * scale) + offset)
  gemm      everything of _i8_reference.gemm_reference, and per period p, directly after y = y + float32(I_p) * t_p:
            R_p = sum_{k in p} a[m][k] (exact), c_p = float32(R_p) * sa[m][p], y = y + c_p * ob[n][p], each product and sum rounded
            on its own; the bias last
"""
import numpy as np

import _i8_reference as G
from _group_affine_reference import group_affine_reference
from _group_reference import scale_shape


def offsets_layout(op):
    """The offsets buffer float32 [nbs * 16 LT] of an operand: the scales' layout, +0 for lines past L."""
    L, K = op["codes"].shape
    LT, _, nbs = G.layout_dims(L, K, op["block"])
    obuf = np.zeros((nbs, 16 * LT), np.float32)
    obuf[:, :L] = np.asarray(op["offsets"], np.float32).T
    return obuf.reshape(-1)


def offsets_mismatch(obuf, op):
    """None if the device's offsets buffer is the reference's bit for bit (a NaN equals a NaN), else a message."""
    ref = offsets_layout(op)
    got = np.asarray(obuf, np.float32).reshape(-1)
    if got.shape != ref.shape:
        return f"offset buffer size {got.shape} != {ref.shape}"
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        i = int(np.flatnonzero(~same)[0])
        return f"{int((~same).sum())} offsets differ, first at {i}: {got[i]!r} != {ref[i]!r}"
    return None


def operand_of_parameter_affine(P, s, b, qmin, qmax, axis, gs, rounding):
    """The operand lq_i8_operand_pack_affine writes for parameter P [R][C] under scales s and offsets b."""
    P = np.asarray(P, np.float32)
    R, C = P.shape
    length = R if axis == 0 else C
    assert -128 <= qmin <= qmax <= 127 and (gs >= length or gs % G.UNIT == 0)
    gs_eff = min(gs, length)
    shp = scale_shape(R, C, axis, gs_eff)
    s, b = np.asarray(s, np.float32).reshape(shp), np.asarray(b, np.float32).reshape(shp)
    q = group_affine_reference(P, s, b, np.zeros_like(P), qmin, qmax, axis, gs_eff, rounding=rounding)["q"]
    codes = G.i8_view(q)
    tr = (lambda m: np.ascontiguousarray(m.T)) if axis == 0 else np.ascontiguousarray
    return dict(codes=tr(codes), scales=tr(s), offsets=tr(b), block=0 if gs >= length else gs)


def fq_out_of_parameter_affine(P, s, b, qmin, qmax, axis, gs, rounding):
    R, C = P.shape
    gs_eff = min(gs, R if axis == 0 else C)
    shp = scale_shape(R, C, axis, gs_eff)
    return group_affine_reference(P, np.asarray(s, np.float32).reshape(shp), np.asarray(b, np.float32).reshape(shp), np.zeros_like(P),
                                  qmin, qmax, axis, gs_eff, rounding=rounding)["out"]


def _per_k(op, what, dtype):
    K, block = op["codes"].shape[1], op["block"]
    return np.asarray(op[what])[:, (np.arange(K) // block) if block else np.zeros(K, np.int64)].astype(dtype)


def decode_affine(op, dtype=np.float32):
    """code * scale + offset, two roundings in ``dtype``."""
    with np.errstate(all="ignore"):
        m = op["codes"].astype(dtype) * _per_k(op, "scales", dtype)
        out = m + _per_k(op, "offsets", dtype)
    assert m.dtype == out.dtype == dtype
    return out


def row_sums(a, b):
    """[R int64 [M]] per period of the product a b^T, in ascending k."""
    A = a["codes"].astype(np.int64)
    return [A[:, ks].sum(axis=1) for ks, _, _ in G.period_sums(a, b)]


def gemm_affine_reference(a, b, bias=None):
    """float32 [M][N]: the definition of lq_i8_gemm_affine.  Only ``b`` carries offsets."""
    assert "offsets" not in a, "only the B operand carries offsets"
    M, N = a["codes"].shape[0], b["codes"].shape[0]
    A = a["codes"].astype(np.int64)
    y = np.zeros((M, N), np.float32)
    with np.errstate(all="ignore"):
        for ks, I, _ in G.period_sums(a, b):
            assert I.min() >= -2 ** 31 and I.max() < 2 ** 31, "a period sum leaves int32"
            pa = ks.start // a["block"] if a["block"] else 0
            pb = ks.start // b["block"] if b["block"] else 0
            sa = a["scales"][:, pa].astype(np.float32)
            t = sa[:, None] * b["scales"][:, pb].astype(np.float32)[None, :]
            term = I.astype(np.float32) * t
            y = y + term
            R = A[:, ks].sum(axis=1)
            assert np.abs(R).max() <= 2 ** 23, "a row sum leaves 2^23"
            c = R.astype(np.float32) * sa
            oterm = c[:, None] * b["offsets"][:, pb].astype(np.float32)[None, :]
            y = y + oterm
            assert t.dtype == term.dtype == c.dtype == oterm.dtype == y.dtype == np.float32
        if bias is not None:
            y = y + np.asarray(bias, np.float32)[None, :]
    return y


def gemm_affine_f64(a, b, bias=None):
    """(float64 product of the decoded operands, sum of |terms| with the two parts of W counted separately): the second check."""
    da = G.decode(a, np.float64)
    qs = G.decode(b, np.float64)
    ob = _per_k(b, "offsets", np.float64)
    with np.errstate(all="ignore"):
        ref = da @ (qs + ob).T
        terms = np.abs(da) @ (np.abs(qs) + np.abs(ob)).T
        if bias is not None:
            ref, terms = ref + np.asarray(bias, np.float64)[None, :], terms + np.abs(np.asarray(bias, np.float64))[None, :]
    return ref, terms


# ---------------------------------------------------------------------------------------------------------------- the GPU data sets
def with_offsets(b, seed=0, zero=False):
    """``b`` with random normal offsets per (line, scale block): some negative, and exact zeros planted (every fifth line)."""
    rng = np.random.default_rng([seed, *b["codes"].shape, b["block"]])
    off = rng.normal(0.0, 0.5, b["scales"].shape).astype(np.float32)
    off[::5] = 0.0
    if zero:
        off[:] = 0.0
    return dict(b, offsets=off)


def gemm_affine_case(M, N, K, a_block=0, b_block=0, seed=0):
    a, b, bias = G.gemm_case(M, N, K, a_block, b_block, seed)
    return a, with_offsets(b, seed), bias


def all_gemm_affine_keys():
    return [(*s, 0, 0) for s in G.GEMM_SHAPES] + [(*G.BLOCK_PAIR_SHAPE, a, b) for a, b in G.BLOCK_PAIRS] + list(G.EXTRA_GEMM_KEYS)


PIN_K, PIN_BLOCK, PIN_N = 160, 64, 16


def pin_b(N=PIN_N, K=PIN_K, block=PIN_BLOCK):
    """B with codes 0, scales 1 and offsets distinct powers of two per column and block: Y = sum_p R_p ob[n][p] exactly."""
    nbs = G.layout_dims(N, K, block)[2]
    # column n, block p: 2^(n - 8 - 3 p), distinct along either axis; the exponents stay close enough that the sum over three
    # blocks of row sums up to 2^13 keeps fewer than 24 significant bits
    off = np.exp2(np.arange(N)[:, None] - 8.0 - 3.0 * np.arange(nbs)[None, :]).astype(np.float32)
    sign = np.where(np.arange(N) % 3 == 1, -1.0, 1.0).astype(np.float32)
    return dict(codes=np.zeros((N, K), np.int8), scales=np.ones((N, nbs), np.float32), offsets=off * sign[:, None], block=block)


def pin_one_hot_a(k, M=16, K=PIN_K):
    """A zero except column k = m - 7 (a negative row sum for m < 7, zero for m = 7), one scale per row, all 1."""
    a = np.zeros((M, K), np.int8)
    a[:, k] = np.arange(M) - 7
    return dict(codes=a, scales=np.ones((M, 1), np.float32), block=0)


def pin_random_a(M=33, K=PIN_K, seed=0):
    rng = np.random.default_rng([seed, M, K])
    return dict(codes=rng.integers(-128, 128, (M, K)).astype(np.int8), scales=np.ones((M, 1), np.float32), block=0)


def pin_extreme():
    """A == -128 over one period of 65536: R = -2^23; B codes 0, offsets 2^(n - 8)."""
    a = dict(codes=np.full((16, G.EXTREME_K), -128, np.int8), scales=np.ones((16, 1), np.float32), block=0)
    return a, pin_b(16, G.EXTREME_K, 0)


def exact_dense_case(M=19, K=192, N=21, gs=64, seed=0):
    """(x, W (K, N), scale (nb, N), offset (nb, N), bias) on which every partial sum is exact in float32: power-of-two scales,
    offsets that are small multiples of them, W on its grid (q s + b with q in [-8, 7]), integer activations whose row absmax is 127
    (so the activation scale is 1 and the codes are the integers)."""
    rng = np.random.default_rng([seed, M, K, N, gs])
    nb = -(-K // gs)
    s = np.exp2(rng.integers(-4, 0, (nb, N))).astype(np.float32)
    b = (rng.integers(-3, 4, (nb, N)) * s).astype(np.float32)
    q = rng.integers(-8, 8, (K, N)).astype(np.float32)
    g = np.arange(K) // gs
    W = (q * s[g] + b[g]).astype(np.float32)
    x = rng.integers(-20, 21, (M, K)).astype(np.float32)
    x[:, 0] = 127.0
    bias = rng.integers(-8, 8, N).astype(np.float32)      # on the bias's own 4-bit grid under scale 1
    return x, W, s, b, bias
