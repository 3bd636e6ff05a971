"""NumPy statement of the stem convolution (include/lq_hip.h, "stem"): the row operand, the stem kernel operand and the DEFINITION of
lq_i8_stem_conv2d, on tests/_i8_reference.py (codes) and tests/_i8_direct_reference.py / _i8_conv_fused_reference.py (kernel codes,
epilogue, pixel operand).  rows: dict(codes int8 [B][H][W][4], scales float32 [B][H]); kernel codes: int8 [co][ci][kh][kw]."""
import numpy as np

import _i8_conv_fused_reference as F
import _i8_direct_reference as D
import _i8_reference as I

# (B, C, H, W, co, KH, KW, (sh, sw), padding): a string as the layers pad, or (top, bottom, left, right)
GEOMS = [(2, 3, 9, 11, 10, 3, 3, (1, 1), "SAME"),            # partial line tile, partial column tile, lines straddling rows and images
         (1, 3, 16, 18, 64, 7, 7, (2, 2), "SAME"),           # the stem proper: asymmetric 2 / 3 padding, odd corners, four column tiles
         (2, 4, 6, 7, 33, 5, 8, (1, 1), (1, 3, 0, 2)),       # four channel bytes, KW = 8, rows skipped top and bottom, a masked tile
         (1, 1, 5, 40, 128, 1, 3, (1, 2), "VALID"),          # C = 1, one kernel row, eight column tiles, no padding
         (3, 3, 20, 20, 32, 3, 3, (1, 1), "SAME")]           # 75 line tiles: a wave walks more than one, more than one block runs
STEM = GEOMS[1]


def padding_of(g):
    return tuple(g[8]) if not isinstance(g[8], str) else D.padding_of(g)


def rows_of(x):
    """The row operand of x [B][C][H][W]: row b H + h of operand_of_activation(x as [B H][W C], block 0)."""
    B, C, H, W = x.shape
    op = I.operand_of_activation(np.ascontiguousarray(np.asarray(x, np.float32).transpose(0, 2, 3, 1)).reshape(B * H, W * C), 0)
    codes = np.zeros((B, H, W, 4), np.int8)
    codes[..., :C] = op["codes"].reshape(B, H, W, C)
    return dict(codes=codes, scales=np.ascontiguousarray(op["scales"].reshape(B, H)))


def pack_kernel(q, s):
    """(codes uint8 [NT][KH][64][8], scales float32 [16 NT]): lane l, byte jj holds filter 16 nt + (l & 15), tap column
    2 (l >> 4) + (jj >> 2), channel jj & 3 of kernel row i."""
    co, ci, kh, kw = q.shape
    NT = -(-co // 16)
    qp = np.zeros((16 * NT, 4, kh, 8), np.int8)
    qp[:co, :ci, :, :kw] = q
    nt, i, l, jj = np.meshgrid(np.arange(NT), np.arange(kh), np.arange(64), np.arange(8), indexing="ij")
    scales = np.ones(16 * NT, np.float32)
    scales[:co] = s
    return np.ascontiguousarray(qp[16 * nt + (l & 15), jj & 3, i, 2 * (l >> 4) + (jj >> 2)]).reshape(-1).view(np.uint8), scales


def conv_reference(rows, q, sk, bias, strides, padding):
    """float32 [M][co], the DEFINITION: per kernel row i ascending the exact integer sum over its taps inside the image and the
    channels, times the image row's scale, added in float32 (each product and sum rounds separately); the filter's scale last, then
    the bias.  padding: (top, bottom, left, right)."""
    a, sr = rows["codes"].astype(np.int64), rows["scales"]
    B, H, W, _ = a.shape
    co, ci, KH, KW = q.shape
    OH, OW = (H + padding[0] + padding[1] - KH) // strides[0] + 1, (W + padding[2] + padding[3] - KW) // strides[1] + 1
    ap = np.pad(a, ((0, 0), (0, 0), (padding[2], padding[3] + KW), (0, 0)))       # a column outside [0, W) holds zero: it adds nothing
    y = np.zeros((B, OH, OW, co), np.float32)
    with np.errstate(all="ignore"):
        for i in range(KH):
            ih = np.arange(OH) * strides[0] - padding[0] + i
            vh = np.flatnonzero((ih >= 0) & (ih < H))
            if not vh.size:                               # a row outside the image is skipped
                continue
            isum = np.zeros((B, vh.size, OW, co), np.int64)
            for j in range(KW):
                cols = np.arange(OW) * strides[1] + j     # in the padded row
                isum += np.einsum("bhwc,nc->bhwn", ap[:, ih[vh]][:, :, cols, :ci], q[:, :, i, j].astype(np.int64))
            assert np.abs(isum).max() < 2 ** 31, "a row's sum leaves int32"
            y[:, vh] = y[:, vh] + isum.astype(np.float32) * sr[:, ih[vh]][:, :, None, None]
        y = y * np.asarray(sk, np.float32)
        if bias is not None:
            y = y + np.asarray(bias, np.float32)
    assert y.dtype == np.float32
    return y.reshape(B * OH * OW, co)


def fused_reference(g, rows, q, sk, bias, activation=None, affine=None, affine_first=False):
    """The pixel operand lq_i8_stem_conv2d_quantize writes: pixels_of(epilogue(conv_reference)) seen as [B][co][OH][OW]."""
    pads = padding_of(g)
    v = F.epilogue(conv_reference(rows, q, sk, bias, g[7], pads), activation, affine, affine_first)
    OH, OW = (g[2] + pads[0] + pads[1] - g[5]) // g[7][0] + 1, (g[3] + pads[2] + pads[3] - g[6]) // g[7][1] + 1
    return D.pixels_of(v.reshape(g[0], OH, OW, g[4]).transpose(0, 3, 1, 2))


def row_input(shape, seed=0, planted=False):      # every image row on a binade of its own; planted: a zero row, a NaN row
    B, C, H, W = shape
    rng = np.random.default_rng([seed, *shape])
    x = (rng.normal(0.0, 1.0, shape) * np.exp2(rng.integers(-6, 6, (B, 1, H, 1)))).astype(np.float32)
    if planted:
        x[0, :, 0, :], x[B - 1, C // 2, H // 2, W // 2] = 0.0, np.nan
    return x


def conv_case(g, seed=0):      # (rows, kernel codes, filter scales, bias, (g, h))
    B, C, H, W, co, KH, KW = g[:7]
    rng = np.random.default_rng([seed, *g[:7]])
    P, sk = rng.normal(0.0, 0.05, (co, C, KH, KW)).astype(np.float32), np.exp2(rng.uniform(-11.0, -10.0, co)).astype(np.float32)
    return (rows_of(row_input((B, C, H, W), seed)), D.kernel_codes(P, sk, -128, 127, "nearest"), sk, rng.normal(0.0, 1.0, co).astype(np.float32),
            (rng.normal(1.0, 0.5, co).astype(np.float32), rng.normal(0.0, 1.0, co).astype(np.float32)))


def one_hot_case():
    """(geometry, rows, kernel codes) on the 7 x 7 stem: filter n holds a single code 1 at reduction position n = (c KH + i) KW + j."""
    B, C, H, W, _, KH, KW = STEM[:7]
    co = C * KH * KW
    return (B, C, H, W, co, KH, KW, *STEM[7:]), rows_of(row_input((B, C, H, W))), np.eye(co, dtype=np.int8).reshape(co, C, KH, KW)
