"""CPU tests of lq_i8_conv2d_quantize: its refusals (every call fails in validation), the Python refusals, and the data conditions of
the GPU cases, asserted on the reference alone so that no case of tests/test_gpu_i8_conv_fused.py passes vacuously."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_fused_reference as R                                                          # noqa: E402
from test_i8_direct_cpu import LQ_EALIGN, LQ_EINVAL, P, _g                                    # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L                                        # noqa: E402


def _call(pc=P, ps=P, kc=P, ks=P, bias=None, g=None, co=10, post_scale=None, post_shift=None, act=0, first=0, oc=P, osc=P):
    return (pc, ps, kc, ks, bias, ctypes.byref(g or _g()) if g is not False else None, co, post_scale, post_shift, act, first, oc, osc, None)


REFUSALS = (
    [(_call(**{k: None}), LQ_EINVAL, "is NULL") for k in ("pc", "ps", "kc", "ks", "oc", "osc")] + [(_call(g=False), LQ_EINVAL, "'g' is NULL")]
    + [(_call(g=_g(**kw)), LQ_EINVAL, why) for kw, why in (
        (dict(B=0), "extents must be positive"), (dict(C=65537), "above 65536"), (dict(sh=0), "strides must be positive"),
        (dict(KH=8), "does not fit the padded input"), (dict(B=65536, H=9, W=9, pads=(0, 0, 0, 0), KH=1, KW=1), "above 65535 * 64"))]
    + [(_call(co=0), LQ_EINVAL, "extents must be positive"), (_call(co=513), LQ_EINVAL, "co = 513 is above 512"),
       (_call(act=2), LQ_EINVAL, "bad activation 2"), (_call(act=-1), LQ_EINVAL, "bad activation -1"), (_call(first=2), LQ_EINVAL, "affine_first"),
       (_call(post_scale=P), LQ_EINVAL, "both be given or both be NULL"), (_call(post_shift=P), LQ_EINVAL, "both be given or both be NULL")]
    + [(_call(**{k: P + 4}), LQ_EALIGN, "16-byte aligned") for k in ("pc", "ps", "kc", "ks", "oc", "osc")]
    + [(_call(bias=P + 2), LQ_EALIGN, "bias"), (_call(post_scale=P + 2, post_shift=P), LQ_EALIGN, "post_scale or post_shift"),
       (_call(post_scale=P, post_shift=P + 1), LQ_EALIGN, "post_scale or post_shift")])


@pytest.mark.parametrize("args,rc,why", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals_of_the_c_surface(args, rc, why):
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    assert lib.lq_i8_conv2d_quantize(*args) == rc and why in lib.lq_last_error().decode()


def test_refusals_of_the_python_surface():
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8, orientation="scalar").eval()
    assert [c[0][0] for c in m.i8_conv_chains()] == [m.convs[0], m.convs[2], m.convs[4]]
    affine, x = L.bn_affine(m.bns[0]), torch.zeros(1, 3, 8, 8)
    for last in ((m.convs[1], "relu", None, False), (m.convs[1], None, affine, False)):
        with pytest.raises(ValueError, match="the last layer writes fp32 and takes no epilogue"):
            L.i8_conv_chain(x, [(m.convs[0], "relu", affine, False), last])
    with pytest.raises(ValueError, match="needs convs=True and direct=True"):
        L.i8_hardware(m, convs=True, fused_convs=True)
    with pytest.raises(ValueError, match="emulate=True with fused_convs=True"):
        L.i8_hardware(m, convs=True, direct=True, emulate=True, fused_convs=True)
    assert L.i8_hardware(m, convs=True, direct=True).fused_convs is False


@pytest.mark.parametrize("co", R.WAVE_CO + R.BLOCK_CO)
@pytest.mark.parametrize("gi", [0, 1])
def test_data_conditions_of_the_gpu_cases(gi, co):
    """If a seed fails a condition, change the seed (R.SEEDS), not the condition."""
    g, pix, q, sk, bias, affine = R.case(gi, co)
    y = R.D.conv_reference(pix, q, sk, bias, g[7], R.D.padding_of(g))
    for name, (act, with_affine, first) in R.EPILOGUES.items():
        out, v = R.fused_reference(g, pix, q, sk, bias, act, affine if with_affine else None, first)
        codes = out["codes"].reshape(-1, out["codes"].shape[-1])
        assert np.isfinite(out["scales"]).all() and not codes[:, co:].any()
        if co > 128:      # every wave's columns hold the absmax channel of some pixel: dropping any wave's partial moves a scale
            top = np.abs(v).argmax(axis=1)
            assert all(((top >= lo) & (top < hi)).any() for lo, hi in R.wave_columns(co)), (name, np.bincount(top // 16))
        if act == "relu":
            cut = (y if not first else R.epilogue(y, None, affine, True)) < 0          # where relu acts
            assert cut.any() and (out["scales"] > np.float32(2.0 ** -126)).any(), name
            assert name == "relu_affine" or not codes[:, :co][cut].any(), name      # relu last: those codes are 0
    if co in (33, 144):       # the planted cases of the GPU file
        g, pix, q, sk, bias = R.planted_case("dead", gi, co)
        yd = R.D.conv_reference(pix, q, sk, bias, g[7], R.D.padding_of(g))
        dead = (yd <= 0).all(axis=1)
        assert dead[0] and not dead.all(), "the planted zero pixel is non-positive in every channel, and others are alive"
        g, pix, q, sk, bias = R.planted_case("bad", gi, co)
        assert int(np.isnan(pix["scales"]).sum()) == 2
