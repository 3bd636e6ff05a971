"""CPU tests of lq_i8_conv2d_quantize_residual: its refusals (every call fails in validation), the Python refusals, and the data
conditions of the GPU cases, asserted on the reference alone so that no case of tests/test_gpu_i8_conv_residual.py passes vacuously."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_residual_reference as R                                                       # noqa: E402
from test_i8_direct_cpu import LQ_EALIGN, LQ_EINVAL, P, _g                                    # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, models, ops                           # noqa: E402

_BUF = (ctypes.c_uint8 * (4 * 4096 + 16))()               # never dereferenced: every call fails in validation
RC = (ctypes.addressof(_BUF) + 15) & ~15                  # _g() and co = 10: M = 70 lines, 2240 code bytes, 280 scale bytes
RS, OC, OS = RC + 4096, RC + 8192, RC + 12288


def _call(co=10, act=0, rc=RC, rs=RS, oc=OC, osc=OS):
    return (P, P, P, P, None, ctypes.byref(_g()), co, None, None, act, 0, rc, rs, oc, osc, None)


REFUSALS = ([(_call(rc=None), LQ_EINVAL, "'res_codes' is NULL"), (_call(rs=None), LQ_EINVAL, "'res_scales' is NULL"),
             (_call(rc=None, rs=None), LQ_EINVAL, "without a residual is lq_i8_conv2d_quantize")]
            + [(_call(**kw), LQ_EINVAL, "overlaps a residual buffer") for kw in (
                dict(oc=RC), dict(osc=RS), dict(oc=RS), dict(osc=RC), dict(oc=RC + 2240 - 16), dict(oc=RC - 2240 + 16), dict(osc=RS + 280 - 8),
                dict(osc=RC + 2240 - 16))]
            + [(_call(rc=RC + 4), LQ_EALIGN, "res_codes is not 16-byte aligned"), (_call(rs=RS + 4), LQ_EALIGN, "res_scales is not 16-byte aligned")]
            + [(_call(co=513), LQ_EINVAL, "co = 513 is above 512"), (_call(act=2), LQ_EINVAL, "bad activation 2"), (_call(oc=None), LQ_EINVAL, "is NULL")])


@pytest.mark.parametrize("args,rc,why", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals_of_the_c_surface(args, rc, why):
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    assert lib.lq_i8_conv2d_quantize_residual(*args) == rc
    assert why in lib.lq_last_error().decode() and "lq_i8_conv2d_quantize_residual:" in lib.lq_last_error().decode()


def test_refusals_of_the_python_surface():
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8, orientation="scalar").eval()
    affine, x = L.bn_affine(m.bns[0]), torch.zeros(1, 3, 8, 8)
    res = ops.I8Pixels(torch.zeros(1, 8, 8, 32, dtype=torch.uint8), torch.ones(1, 8, 8), (1, 32, 8, 8))
    first = (m.convs[0], "relu", affine, False)
    with pytest.raises(ValueError, match="or the same and a residual, got 6 entries"):
        L.i8_conv_chain(x, [first + (res, None)], out_pixels=True)
    with pytest.raises(ValueError, match="the residual must be an ops.I8Pixels or None, got Tensor"):
        L.i8_conv_chain(x, [first + (res.codes,)], out_pixels=True)
    with pytest.raises(ValueError, match="has no epilogue to add a residual in"):
        L.i8_conv_chain(x, [first, (m.convs[1], None, None, False, res)])
    with pytest.raises(ValueError, match="the last layer writes fp32 and takes no epilogue"):      # out_pixels=False: as ever
        L.i8_conv_chain(x, [first, (m.convs[1], "relu", None, False)])
    with pytest.raises(ValueError, match="the fp32 result takes no epilogue"):
        m.convs[1].call_i8_direct(torch.zeros(1, 32, 8, 8), residual=res)
    with pytest.raises(ValueError, match=r"not the output's \(B, co, OH, OW\) = \(1, 32, 4, 4\)"):
        ops._check_i8_residual(res, (1, 32, 4, 4), (1, 4, 4, 32), torch.device("cpu"))


def test_the_blocks_state_their_chains():
    b = models._ResidualBlock(64, 128, (2, 2), 1, "ste", 0.0, 3, "scalar", None)
    assert b.i8_chains_out_pixels and b.i8_fused() is None
    assert b.i8_conv_chains() == [[(b.conv1, "relu", b.bn1, True), (b.conv2, "relu", b.bn2, True)], [(b.shortcut, None, b.bn_s, True)]]
    assert len(models._ResidualBlock(64, 64, (1, 1), 1, "ste", 0.0, 3, "scalar", None).i8_conv_chains()) == 1
    assert not hasattr(models._BottleneckBlock, "i8_conv_chains")      # co reaches 2048: ResNet50Like stays unfused


@pytest.mark.parametrize("co", R.CO)
@pytest.mark.parametrize("gi", [0, 1])
def test_data_conditions_of_the_gpu_cases(gi, co):
    """If a seed fails a condition, change the seed (R.SEEDS), not the condition."""
    g, _, _, _, _, affine, res, y = R.base(gi, co)
    for name, (act, with_affine, first) in R.EPILOGUES.items():
        out, v, u0, u = R.reference(gi, co, name)
        plain = R.pixels_of(R.epilogue(y, act, affine if with_affine else None, first).reshape(g[0], *R.out_hw(g), co).transpose(0, 3, 1, 2))
        assert np.isfinite(out["scales"]).all() and (out["scales"] != plain["scales"]).any(), name      # the residual moves a scale
        if act == "relu":     # the add comes before the activation: it brings elements across zero both ways
            assert ((u0 < 0) & (u > 0)).any() and ((u < 0) & (u0 > 0)).any(), name
        if co > 128:          # every wave's columns hold the absmax channel of some pixel AFTER the add
            top = np.abs(v).argmax(axis=1)
            assert all(((top >= lo) & (top < hi)).any() for lo, hi in R.wave_columns(co)), (name, np.bincount(top // 16))
    # some quad of some tile: 16 pairwise distinct residual bytes under four distinct row scales (a wrong transpose or a neighbour's
    # scale would show)
    codes, scales = res["codes"].reshape(-1, res["codes"].shape[-1]), res["scales"].reshape(-1)
    quads = [(m, n) for m in range(0, len(scales) - 3, 4) for n in range(0, co - 3, 4)
             if len(set(codes[m:m + 4, n:n + 4].reshape(-1).tolist())) == 16 and len(set(scales[m:m + 4].tolist())) == 4]
    assert quads
