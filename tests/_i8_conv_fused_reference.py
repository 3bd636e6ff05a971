"""NumPy statement of lq_i8_conv2d_quantize (include/lq_hip.h): pixels_of(epilogue(conv_reference(...))) on tests/_i8_direct_reference.py,
float32 throughout, each operation rounding separately.  The cases of tests/test_gpu_i8_conv_fused.py and their data conditions."""
import numpy as np

import _i8_direct_reference as D

GEOMS = [(2, 32, 5, 7, None, 3, 3, (1, 1), "SAME"), (1, 64, 6, 6, None, 3, 3, (2, 2), "SAME")]      # M = 70 on STEP 32; M = 9 on STEP 64
WAVE_CO, BLOCK_CO = [10, 33, 70, 128], [144, 200, 512]
EPILOGUES = {"none": (None, False, False), "relu": ("relu", False, False), "relu_affine": ("relu", True, False),
             "affine_relu": ("relu", True, True)}      # (activation, affine given, affine_first)
SEEDS = {(1, 144): 1, (1, 200): 12, (1, 512): 2}       # (geometry index, co) -> seed, where seed 0 fails a data condition (M = 9)


def geom(gi, co):
    return (*GEOMS[gi][:4], co, *GEOMS[gi][5:])


def out_hw(g):
    top, bottom, left, right = D.padding_of(g)
    return (g[2] + top + bottom - g[5]) // g[7][0] + 1, (g[3] + left + right - g[6]) // g[7][1] + 1


def epilogue(y, activation, affine, affine_first):
    """v [M][co] float32: aff(act(Y)) or act(aff(Y)); aff(v) = RN(RN(v g) + h); relu(v) = v > 0 ? v : (v != v ? v : +0)."""
    relu = lambda v: np.where(v > 0, v, np.where(np.isnan(v), v, np.float32(0.0))).astype(np.float32)      # noqa: E731
    act = relu if activation == "relu" else (lambda v: v)
    with np.errstate(all="ignore"):
        aff = (lambda v: (v * affine[0]).astype(np.float32) + affine[1]) if affine is not None else (lambda v: v)
        v = act(aff(y)) if affine_first else aff(act(y))
    assert v.dtype == np.float32
    return v


def fused_reference(g, pix, q, sk, bias, activation=None, affine=None, affine_first=False):
    """(pixels dict of the output, v [M][co]): what lq_i8_pixels_quantize writes for v seen as [B][co][OH][OW]."""
    v = epilogue(D.conv_reference(pix, q, sk, bias, g[7], D.padding_of(g)), activation, affine, affine_first)
    OH, OW = out_hw(g)
    return D.pixels_of(v.reshape(g[0], OH, OW, g[4]).transpose(0, 3, 1, 2)), v


def case(gi, co):
    """(geometry, pixels, kernel codes, filter scales, bias, (g, h))."""
    g = geom(gi, co)
    seed = SEEDS.get((gi, co), 0)
    rng = np.random.default_rng([seed, 11, gi, co])
    return (g, *D.conv_case(g, seed), (rng.normal(1.0, 0.5, co).astype(np.float32), rng.normal(0.0, 1.0, co).astype(np.float32)))


def wave_columns(co):
    """The column ranges of the four waves of the row-per-block form: the padded row's OT = 2 ceil(co / 32) tiles of 16, wave w
    the tiles [w OT / 4, (w + 1) OT / 4)."""
    OT = 2 * -(-co // 32)
    return [(16 * (w * OT // 4), 16 * ((w + 1) * OT // 4)) for w in range(4)]


def planted_case(kind, gi, co):
    """(geometry, pixels, q, sk, bias): "bad" -- a NaN and a -Inf input pixel; "dead" -- the inputs under the window of output
    pixel (0, 0, 0) are zero and every bias is below -1, so under relu that pixel's Y is non-positive in every channel."""
    g, pix, q, sk, bias, _ = case(gi, co)
    x = D.gaussian_input(g[:4], SEEDS.get((gi, co), 0), planted=kind == "bad")
    if kind == "dead":
        x[0, :, :3, :3] = 0.0
        bias = -np.abs(bias) - np.float32(1.0)
    return g, D.pixels_of(x), q, sk, bias
