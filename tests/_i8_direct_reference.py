"""NumPy statement of the direct int8 convolution (include/lq_hip.h): the two operand layouts and the DEFINITION of lq_i8_conv2d.  The
codes are tests/_i8_reference.py's.  pixels: dict(codes int8 [B][H][W][CP], scales float32 [B][H][W]); kernel codes: int8 [co][ci][kh][kw]."""
import numpy as np

import _i8_reference as I
from learned_quantization_amd.layers import _same_padding

GEOMS = [(2, 32, 5, 7, 10, 3, 3, (1, 1), "SAME"), (1, 64, 6, 6, 33, 3, 3, (2, 2), "SAME"), (2, 96, 3, 5, 16, 1, 1, (1, 1), "VALID"),
         (1, 3, 9, 9, 8, 7, 7, (2, 2), "SAME"), (3, 128, 4, 4, 64, 3, 2, (1, 2), "VALID"), (5, 32, 4, 4, 70, 3, 3, (1, 1), "SAME")]      # (B, C, H, W, co, KH, KW, (sh, sw), padding)
PIXEL_SHAPES = [(2, 32, 5, 7), (1, 3, 4, 4), (2, 96, 3, 5), (1, 64, 6, 6)]
ONE_HOT = [(32, 3, 3), (64, 2, 1)]                      # (C, KH, KW): co = C KH KW, one launch per form
EXACT = GEOMS[:2]                                       # both STEP forms


def padding_of(g):
    return (*_same_padding(g[2], g[5], g[7][0]), *_same_padding(g[3], g[6], g[7][1])) if g[8] == "SAME" else (0, 0, 0, 0)


def pixels_of(x):
    """The pixel operand of x [B][C][H][W]: row (b H + h) W + w of operand_of_activation(x as [B H W][C], block 0)."""
    B, C, H, W = x.shape
    op = I.operand_of_activation(np.ascontiguousarray(np.asarray(x, np.float32).transpose(0, 2, 3, 1)).reshape(-1, C), 0)
    codes = np.zeros((B, H, W, 32 * -(-C // 32)), np.int8)
    codes[..., :C] = op["codes"].reshape(B, H, W, C)
    return dict(codes=codes, scales=np.ascontiguousarray(op["scales"].reshape(B, H, W)))


def kernel_codes(P, s, qmin, qmax, rounding):
    co, K = P.shape[0], P[0].size
    return I.operand_of_parameter(np.asarray(P, np.float32).reshape(co, K), np.asarray(s, np.float32).reshape(co, 1), qmin, qmax, 1, K,
                                  rounding)["codes"].reshape(P.shape)


def pack_kernel(q, s):
    """(codes uint8 [NT][KH KW][CS][64][FB], scales float32 [16 NT]): filter 16 nt + (l & 15), channel STEP cs + FB (l >> 4) + jj."""
    co, ci, kh, kw = q.shape
    CP = 32 * -(-ci // 32)
    STEP, NT = (64 if CP % 64 == 0 else 32), -(-co // 16)
    qp = np.zeros((16 * NT, CP, kh * kw), np.int8)
    qp[:co, :ci] = q.reshape(co, ci, kh * kw)
    nt, tap, cs, l, jj = np.meshgrid(np.arange(NT), np.arange(kh * kw), np.arange(CP // STEP), np.arange(64), np.arange(STEP // 4), indexing="ij")
    scales = np.ones(16 * NT, np.float32)
    scales[:co] = s
    return np.ascontiguousarray(qp[16 * nt + (l & 15), STEP * cs + (STEP // 4) * (l >> 4) + jj, tap]).reshape(-1).view(np.uint8), scales


def conv_reference(pix, q, sk, bias, strides, padding):
    """float32 [M][co], the DEFINITION: per tap in ascending (i, j) the exact integer sum over the channels times the pixel's scale,
    added in float32 (each product and sum rounds separately); the filter's scale last, then the bias.  padding: (top, bottom, left, right)."""
    a, sa = pix["codes"].astype(np.int64), pix["scales"]
    B, H, W, _ = a.shape
    co, ci, KH, KW = q.shape
    OH, OW = (H + padding[0] + padding[1] - KH) // strides[0] + 1, (W + padding[2] + padding[3] - KW) // strides[1] + 1
    y = np.zeros((B, OH, OW, co), np.float32)
    with np.errstate(all="ignore"):
        for i in range(KH):
            for j in range(KW):
                ih, iw = np.arange(OH) * strides[0] - padding[0] + i, np.arange(OW) * strides[1] - padding[2] + j
                vh, vw = np.flatnonzero((ih >= 0) & (ih < H)), np.flatnonzero((iw >= 0) & (iw < W))
                if vh.size and vw.size:                   # a tap outside the image is skipped
                    rows, cols = np.ix_(ih[vh], iw[vw])
                    isum = np.einsum("bhwc,nc->bhwn", a[:, rows, cols, :ci], q[:, :, i, j].astype(np.int64))
                    assert np.abs(isum).max() < 2 ** 31, "a tap's sum leaves int32"
                    sel = np.ix_(np.arange(B), vh, vw)
                    y[sel] = y[sel] + isum.astype(np.float32) * sa[:, rows, cols][..., None]
        y = y * np.asarray(sk, np.float32)
        if bias is not None:
            y = y + np.asarray(bias, np.float32)
    assert y.dtype == np.float32
    return y.reshape(B * OH * OW, co)


def gaussian_input(shape, seed=0, planted=False):      # every pixel on a binade of its own; planted: a zero pixel, a NaN, a -Inf
    B, C, H, W = shape
    rng = np.random.default_rng([seed, *shape])
    x = (rng.normal(0.0, 1.0, shape) * np.exp2(rng.integers(-6, 6, (B, 1, H, W)))).astype(np.float32)
    if planted:
        x[0, :, 0, 0], x[B - 1, C // 2, H // 2, W // 2], x[0, C - 1, H - 1, W - 1] = 0.0, np.nan, -np.inf
    return x


def conv_case(g, seed=0):      # (pixels, kernel codes, filter scales, bias); codes of +-50 to +-100 per sigma: some clip
    B, C, H, W, co, KH, KW = g[:7]
    rng = np.random.default_rng([seed, *g[:7]])
    P, sk = rng.normal(0.0, 0.05, (co, C, KH, KW)).astype(np.float32), np.exp2(rng.uniform(-11.0, -10.0, co)).astype(np.float32)
    return pixels_of(gaussian_input((B, C, H, W), seed)), kernel_codes(P, sk, -128, 127, "nearest"), sk, rng.normal(0.0, 1.0, co).astype(np.float32)


def one_hot_case(C, KH, KW):
    """(geometry, pixels, kernel codes): filter n holds a single code 1 at reduction position n = (c KH + i) KW + j."""
    co = C * KH * KW
    g = (2, C, 5, 6, co, KH, KW, (1, 1), "SAME")
    return g, pixels_of(gaussian_input(g[:4])), np.eye(co, dtype=np.int8).reshape(co, C, KH, KW)


def exact_case(g, seed=0):
    """(x, kernel HWIO, bias, kernel scale, bias scale).  x: integers and, in one channel per pixel, +-(127 - 2^-15): that absmax gives
    the scale RN(RN(a / 127) (1 + 2^-22)) = 1.0 exactly and the code +-127 (+-127 itself gives 1 + 2^-22).  Kernel: integers in
    [-16, 15] times 2^-7, so every output's integer sum stays below 2^24."""
    B, C, H, W, co, KH, KW = g[:7]
    rng = np.random.default_rng([seed, 7, *g[:7]])
    x = rng.integers(-126, 127, (B, C, H, W)).astype(np.float32)
    b, h, w = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    x[b, rng.integers(0, C, (B, H, W)), h, w] = np.where(rng.integers(0, 2, (B, H, W)) > 0, 1.0, -1.0) * np.float32(127.0 - 2.0 ** -15)
    scale, bscale = np.float32(2.0 ** -7), np.float32(2.0 ** -6)
    return (x, (rng.integers(-16, 16, (KH, KW, C, co)) * scale).astype(np.float32), (rng.integers(-128, 128, co) * bscale).astype(np.float32),
            scale, bscale)
