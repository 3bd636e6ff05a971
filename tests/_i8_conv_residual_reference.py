"""NumPy statement of lq_i8_conv2d_quantize_residual (include/lq_hip.h) on tests/_i8_direct_reference.py and
tests/_i8_conv_fused_reference.py: float32 throughout, each operation rounding separately.  The cases of
tests/test_gpu_i8_conv_residual.py; their data conditions are asserted in tests/test_i8_conv_residual_cpu.py."""
import functools

import numpy as np

from _i8_conv_fused_reference import D, GEOMS, case, epilogue, geom, out_hw, wave_columns      # noqa: F401

conv_reference, pixels_of = D.conv_reference, D.pixels_of
CO = [10, 33, 70, 128, 144, 512]       # NTT 2, 4, 8, 8 of the row-per-wave form; NTT 4 and 8 of the row-per-block form
EPILOGUES = {"add": (None, False, False), "add_relu": ("relu", False, False), "affine_add_relu": ("relu", True, True),
             "add_relu_affine": ("relu", True, False)}      # (activation, affine given, affine_first)
SEEDS = {(1, 144): 1, (1, 512): 13}    # (geometry index, co) -> seed of the residual, where seed 0 fails a data condition (M = 9)


def residual_of(gi, co):
    """The residual pixel operand: a Gaussian tensor of the output's shape, its pixel norms spread over two decades."""
    g = geom(gi, co)
    rng = np.random.default_rng([SEEDS.get((gi, co), 0), 23, gi, co])
    shape = (g[0], co, *out_hw(g))
    return pixels_of((rng.normal(0.0, 1.0, shape) * 10.0 ** rng.uniform(-1.0, 1.0, (g[0], 1, *shape[2:]))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def base(gi, co):
    """(geometry, pixels, kernel codes, filter scales, bias, (g, h), residual, Y): computed once, shared, never written to."""
    g, pix, q, sk, bias, affine = case(gi, co)
    return g, pix, q, sk, bias, affine, residual_of(gi, co), conv_reference(pix, q, sk, bias, g[7], D.padding_of(g))


def residual_reference(g, y, res, activation=None, affine=None, affine_first=False):
    """(pixels dict of the output, v, u before the add, u after it), [M][co] each: r = RN(code * scale); u = aff(Y) or Y;
    u = RN(u + r); v = act(u) or aff(act(u))."""
    co = g[4]
    with np.errstate(all="ignore"):
        r = (res["codes"][..., :co].astype(np.float32) * res["scales"][..., None]).reshape(-1, co)
        u0 = epilogue(y, None, affine, True) if affine_first else y
        u = u0 + r
    assert r.dtype == np.float32 and u.dtype == np.float32
    v = epilogue(u, activation, None if affine_first else affine, False)
    return pixels_of(v.reshape(g[0], *out_hw(g), co).transpose(0, 3, 1, 2)), v, u0, u


def reference(gi, co, name):
    g, _, _, _, _, affine, res, y = base(gi, co)
    act, with_affine, first = EPILOGUES[name]
    return residual_reference(g, y, res, act, affine if with_affine else None, first)


def cancelling_case(gi, co):
    """(geometry, pixels, q, sk, bias, (g, h), residual): the inputs under the window of output pixel (0, 0, 0) are zero, so its Y is
    the bias; bias, g and h are small multiples of powers of two, so aff(Y) = RN(RN(bias g) + h) is exactly -code * 2^-2 of the
    residual planted there, and u = +0 in every channel."""
    g, _, q, sk, _, _, res, _ = base(gi, co)
    x = D.gaussian_input(g[:4])
    x[0, :, :3, :3] = 0.0
    rng = np.random.default_rng([31, gi, co])
    kb, kh = rng.integers(-60, 61, co), rng.integers(-60, 61, co)
    bias, affine = (kb * 0.125).astype(np.float32), (np.full(co, 2.0, np.float32), (kh * 0.25).astype(np.float32))
    res = dict(codes=res["codes"].copy(), scales=res["scales"].copy())
    res["codes"][0, 0, 0, :co], res["scales"][0, 0, 0] = -(kb + kh), np.float32(0.25)
    return g, pixels_of(x), q, sk, bias, affine, res
