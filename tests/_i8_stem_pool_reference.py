"""NumPy statement of lq_i8_stem_conv2d_quantize_pool (include/lq_hip.h): pixels_of(pool3(v)), v of tests/_i8_stem_reference.py.  The
cases of tests/test_gpu_i8_stem_pool.py; their data conditions are asserted in tests/test_i8_stem_pool_cpu.py."""
import numpy as np

import _i8_conv_fused_reference as F
import _i8_direct_reference as D
import _i8_stem_reference as S

# (B, C, H, W, co, KH, KW, strides, padding) and the pool's (top, bottom, left, right)
GEOMS = [((2, 3, 37, 37, None, 7, 7, (2, 2), "SAME"), (1, 1, 1, 1)),      # 19 x 19 -> 10 x 10: two strips, the second ragged; three walks of rows
         ((1, 3, 24, 28, None, 7, 7, (2, 2), "SAME"), (0, 1, 0, 1)),      # 12 x 14 -> 6 x 7: even extents, the ResNet case; one full strip
         ((2, 1, 8, 18, None, 3, 3, (1, 1), "VALID"), (0, 0, 0, 0)),      # C = 1, 6 x 16 -> 2 x 7: a conv row and a conv column dropped
         ((3, 2, 5, 4, None, 3, 2, (1, 1), "VALID"), (0, 0, 0, 0))]       # 3 x 3 -> 1 x 1: a single pooled pixel per image


def pool3(v, pads):
    """[B][OH][OW][co] -> [B][PH][PW][co]: the window scanned row by row over v padded with -inf; if (u > m || u != u) m = u."""
    vp = np.pad(v, ((0, 0), (pads[0], pads[1]), (pads[2], pads[3]), (0, 0)), constant_values=-np.inf)
    PH, PW = (vp.shape[1] - 3) // 2 + 1, (vp.shape[2] - 3) // 2 + 1
    m = vp[:, 0:2 * PH - 1:2, 0:2 * PW - 1:2]
    with np.errstate(invalid="ignore"):
        for e in range(1, 9):
            u = vp[:, e // 3:e // 3 + 2 * PH - 1:2, e % 3:e % 3 + 2 * PW - 1:2]
            m = np.where((u > m) | (u != u), u, m)
    return m


def pooled_reference(g, pads, rows, q, sk, bias, activation=None, affine=None, affine_first=False):
    """(pixels dict of the pooled output, p [B][PH][PW][co], v [B][OH][OW][co])."""
    v = F.epilogue(S.conv_reference(rows, q, sk, bias, g[7], S.padding_of(g)), activation, affine, affine_first)
    pc = S.padding_of(g)
    v = v.reshape(g[0], (g[2] + pc[0] + pc[1] - g[5]) // g[7][0] + 1, (g[3] + pc[2] + pc[3] - g[6]) // g[7][1] + 1, g[4])
    p = pool3(v, pads)
    return D.pixels_of(p.transpose(0, 3, 1, 2)), p, v


def case(gi, co, planted=None):
    """(geometry, pool pads, rows, kernel codes, filter scales, bias, (g, h)).  planted "bad": a NaN row scale in the last image and a
    -Inf one in the first; "dead": zero inputs under pooled pixel (0, 0, 0) and every bias below -1, so relu leaves +0 in its window."""
    g, pads = (*GEOMS[gi][0][:4], co, *GEOMS[gi][0][5:]), GEOMS[gi][1]
    rows, q, sk, bias, affine = S.conv_case(g)
    if planted is not None:
        x = S.row_input(g[:4], planted=planted == "bad")
        if planted == "dead":
            x[0, :, :12, :12] = 0.0
            bias = -np.abs(bias) - np.float32(1.0)
        rows = S.rows_of(x)
        if planted == "bad":
            rows["scales"][0, 5] = -np.inf
    return g, pads, rows, q, sk, bias, affine


def argmax_case():
    """Nine images of 5 x 5 under a 1 x 1 kernel of code 1: v is the decoded input, pooled 2 x 2 without padding.  Image k holds its
    largest element at member k = 3 di + dj of window (0, 0)."""
    g, pads = (9, 1, 5, 5, 16, 1, 1, (1, 1), "VALID"), (0, 0, 0, 0)
    x = np.random.default_rng(9).uniform(0.0, 1.0, g[:4]).astype(np.float32)
    for k in range(9):
        x[k, 0, k // 3, k % 3] = 2.0 + k
    return g, pads, S.rows_of(x), np.ones((16, 1, 1, 1), np.int8), np.exp2(np.arange(16) - 8.0).astype(np.float32)
