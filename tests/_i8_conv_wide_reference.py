"""The cases of tests/test_gpu_i8_conv_wide.py (lq_i8_conv2d_quantize_wide, include/lq_hip.h) on tests/_i8_conv_residual_reference.py
and tests/_i8_direct_reference.py: float32 throughout, each operation rounding separately.  Their data conditions are asserted in
tests/test_i8_conv_wide_cpu.py."""
import functools

import numpy as np

import _i8_conv_residual_reference as R
from _i8_conv_fused_reference import EPILOGUES      # name -> (activation, affine given, affine_first)    # noqa: F401

D = R.D
# (B, H, W, KH, KW, strides): 1 x 1 at M = 9, one partial A tile; 1 x 1 stride 2 on 2 x 5 x 5, M = 18; 3 x 3 at M = 18, padded taps
GEOMS = [(1, 3, 3, 1, 1, (1, 1)), (2, 5, 5, 1, 1, (2, 2)), (2, 3, 3, 3, 3, (1, 1))]
# (co, geometry, ci, epilogue, residual, seed).  co 513: OT = 34, a second chunk of two tiles (idle waves, a ragged tile); 1024: two
# full chunks; 1040: three, the last nearly empty; 2048: four, the LDS maximum.  ci 32: the 32-wide step; 128: the 64-wide, two
# steps.  Every width meets every geometry; both step forms meet both RES forms and all four epilogues.  A seed other than 0
# stands where seed 0 fails a data condition
CASES = [(513, 0, 32, "affine_relu", True, 318), (513, 1, 128, "relu", False, 53), (513, 2, 32, "relu_affine", True, 7),
         (1024, 0, 128, "none", True, 1), (1024, 1, 32, "affine_relu", False, 0), (1024, 2, 128, "relu", True, 0),
         (1040, 0, 32, "relu_affine", False, 69), (1040, 1, 128, "affine_relu", True, 1), (1040, 2, 32, "none", False, 2),
         (2048, 0, 128, "relu", False, 8), (2048, 1, 32, "none", True, 0), (2048, 2, 128, "relu_affine", True, 0)]
IDS = [f"co{co}-g{gi}-ci{ci}-{name}-{'res' if res else 'plain'}" for co, gi, ci, name, res, _ in CASES]


def geom(k):
    co, gi, ci = CASES[k][:3]
    B, H, W, KH, KW, strides = GEOMS[gi]
    return (B, ci, H, W, co, KH, KW, strides, "SAME")


@functools.lru_cache(maxsize=None)
def base(k):
    """(geometry, pixels, kernel codes, filter scales, bias, (g, h) or None, residual or None, Y): computed once, shared, never
    written to.  The residual: a Gaussian tensor of the output's shape, its pixel norms spread over two decades."""
    co, _, _, name, with_res, seed = CASES[k]
    g = geom(k)
    pix, q, sk, bias = D.conv_case(g, seed)
    rng = np.random.default_rng([seed, 29, k])
    affine = (rng.normal(1.0, 0.5, co).astype(np.float32), rng.normal(0.0, 1.0, co).astype(np.float32)) if EPILOGUES[name][1] else None
    shape = (g[0], co, *R.out_hw(g))
    res = R.pixels_of((rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-1.0, 1.0, (g[0], 1, *shape[2:]))).astype(np.float32)) \
        if with_res else None
    return g, pix, q, sk, bias, affine, res, R.conv_reference(pix, q, sk, bias, g[7], D.padding_of(g))


@functools.lru_cache(maxsize=None)
def reference(k):
    """(pixels dict of the output, v [M][co])."""
    g, _, _, _, _, affine, res, y = base(k)
    act, _, first = EPILOGUES[CASES[k][3]]
    if res is not None:
        return R.residual_reference(g, y, res, act, affine, first)[:2]
    v = R.epilogue(y, act, affine, first)
    return R.pixels_of(v.reshape(g[0], *R.out_hw(g), g[4]).transpose(0, 3, 1, 2)), v


def chunk_columns(co):      # the column range of every chunk of 32 column tiles that holds a channel
    return [(lo, min(lo + 512, co)) for lo in range(0, co, 512)]


def wave_columns(co):       # per wave the column ranges it owns: the tiles [32 c + 8 w, 32 c + 8 w + 8) of every chunk c
    return [[(lo, min(lo + 128, co)) for lo in range(128 * w, co, 512)] for w in range(4)]
