"""NumPy statement of lq_i8_conv2d_quantize_pool (include/lq_hip.h): pixels_of(pool2(v)) with v of tests/_i8_conv_fused_reference.py.
The cases of tests/test_gpu_i8_conv_pool.py; their data conditions are asserted in tests/test_i8_conv_pool_cpu.py."""
import numpy as np

import _i8_conv_fused_reference as R

D = R.D
# OH x OW = 5 x 7 -> 2 x 3 (a row and a column dropped), PM = 12: a tile spans two images | PM = 18: a ragged last tile | STEP 64,
# 3 x 3 -> 1 x 1, PM = 1
GEOMS = [(2, 32, 5, 7, None, 3, 3, (1, 1), "SAME"), (3, 32, 5, 7, None, 3, 3, (1, 1), "SAME"), (1, 64, 6, 6, None, 3, 3, (2, 2), "SAME")]
SEEDS = {(0, 144): 1, (1, 144): 1}      # (geometry index, co) -> seed, where seed 0 fails a data condition (the four waves)


def pool2(v):
    """[B][OH][OW][co] -> [B][OH // 2][OW // 2][co]: m = v00; for u in (v01, v10, v11): if (u > m || u != u) m = u."""
    POH, POW = v.shape[1] // 2, v.shape[2] // 2
    w = v[:, :2 * POH, :2 * POW]
    m = w[:, 0::2, 0::2]
    with np.errstate(invalid="ignore"):
        for di, dj in ((0, 1), (1, 0), (1, 1)):
            u = w[:, di::2, dj::2]
            m = np.where((u > m) | (u != u), u, m)
    return m


def pooled_reference(g, pix, q, sk, bias, activation=None, affine=None, affine_first=False):
    """(pixels dict of the pooled output, p [B][POH][POW][co], v [B][OH][OW][co])."""
    _, v = R.fused_reference(g, pix, q, sk, bias, activation, affine, affine_first)
    v = v.reshape(g[0], *R.out_hw(g), g[4])
    p = pool2(v)
    return D.pixels_of(p.transpose(0, 3, 1, 2)), p, v


def case(gi, co, planted=None):
    """(geometry, pixels, kernel codes, filter scales, bias, (g, h)).  planted "bad": a NaN and a -Inf input pixel; "dead": the
    inputs under the four windows of pooled pixel (0, 0, 0) are zero and every bias is below -1."""
    g = (*GEOMS[gi][:4], co, *GEOMS[gi][5:])
    seed = SEEDS.get((gi, co), 0)
    rng = np.random.default_rng([seed, 13, gi, co])
    pix, q, sk, bias = D.conv_case(g, seed)
    if planted is not None:
        x = D.gaussian_input(g[:4], seed, planted=planted == "bad")
        if planted == "dead":
            x[0, :, :3, :3] = 0.0
            bias = -np.abs(bias) - np.float32(1.0)
        pix = D.pixels_of(x)
    return g, pix, q, sk, bias, (rng.normal(1.0, 0.5, co).astype(np.float32), rng.normal(0.0, 1.0, co).astype(np.float32))
