"""CPU tests of lq_i8_conv2d_quantize_wide: its refusals (every call fails in validation), the defaults of the Python opt-ins, and the
data conditions of the GPU cases, asserted on the reference alone so that no case of tests/test_gpu_i8_conv_wide.py passes vacuously."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_wide_reference as W                                                           # noqa: E402
from test_i8_conv_residual_cpu import OC, OS, RC, RS                                          # noqa: E402
from test_i8_direct_cpu import LQ_EALIGN, LQ_EINVAL, P, _g                                    # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, models, ops                           # noqa: E402


def _call(co=10, act=0, rc=RC, rs=RS, oc=OC, osc=OS, first=0, post=(None, None)):
    return (P, P, P, P, None, ctypes.byref(_g()), co, *post, act, first, rc, rs, oc, osc, None)


REFUSALS = [(_call(co=2049), LQ_EINVAL, "co = 2049 is above 2048"), (_call(co=2049, rc=None, rs=None), LQ_EINVAL, "co = 2049 is above 2048"),
            (_call(co=0), LQ_EINVAL, "extents must be positive"), (_call(act=2), LQ_EINVAL, "bad activation 2"),
            (_call(first=2), LQ_EINVAL, "affine_first = 2 is neither 0 nor 1"), (_call(post=(P, None)), LQ_EINVAL, "must both be given or both be NULL"),
            (_call(co=2048, oc=None), LQ_EINVAL, "is NULL"),      # co = 513 .. 2048 passes the width check: the next refusal speaks
            (_call(rc=None), LQ_EINVAL, "'res_codes' is NULL: res_codes and res_scales are given together or not at all"),
            (_call(rs=None), LQ_EINVAL, "'res_scales' is NULL: res_codes and res_scales are given together or not at all"),
            (_call(oc=RC), LQ_EINVAL, "overlaps a residual buffer"), (_call(osc=RS), LQ_EINVAL, "overlaps a residual buffer"),
            (_call(rc=RC + 4), LQ_EALIGN, "res_codes is not 16-byte aligned"), (_call(rs=RS + 4), LQ_EALIGN, "res_scales is not 16-byte aligned"),
            (_call(rc=None, rs=None, oc=OC + 4), LQ_EALIGN, "16-byte aligned")]


@pytest.mark.parametrize("args,rc,why", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals_of_the_c_surface(args, rc, why):
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    assert lib.lq_i8_conv2d_quantize_wide(*args) == rc
    assert why in lib.lq_last_error().decode() and "lq_i8_conv2d_quantize_wide:" in lib.lq_last_error().decode()


def test_the_opt_ins_default_to_off():
    assert ops.I8_CONV_QUANT_MAX_FILTERS == 512 and ops.I8_CONV_QUANT_WIDE_MAX_FILTERS == 2048
    for fn, name in ((ops.i8_conv2d_quantize, "wide"), (L._ConvBase.call_i8_direct, "wide"), (L.i8_conv_chain, "wide"),
                     (L.i8_hardware.__init__, "wide_convs")):
        assert inspect.signature(fn).parameters[name].default is False, fn
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8, orientation="scalar").eval()
    with pytest.raises(ValueError, match="wide_convs=True needs fused_convs=True"):
        L.i8_hardware(m, convs=True, direct=True, wide_convs=True)
    assert L.i8_hardware(m, convs=True, direct=True, fused_convs=True).wide_convs is False
    b = models._BottleneckBlock(64, 544, (1, 1), False, 1, (0.0,) * 4, 3, "scalar", None, "ste")      # conv3: 2176 filters
    for layer in b.modules():
        if isinstance(layer, (L.CustomQuantizedScaleLayer, L._HostLayer)):
            layer.q_range = (-128, 127)
    for kw, why in ((dict(), "at most 512"), (dict(wide=True), "at most 2048")):
        with pytest.raises(ValueError, match=why):
            L.i8_conv_chain(torch.zeros(1, 544, 4, 4), [(b.conv3, None, None, False)], out_pixels=True, **kw)


def test_the_bottleneck_block_states_wide_chains_only():
    b = models._BottleneckBlock(64, 64, (1, 1), True, 1, (0.0,) * 4, 3, "scalar", None, "ste")
    assert not hasattr(models._BottleneckBlock, "i8_conv_chains") and not hasattr(models._BottleneckBlock, "i8_chains_out_pixels")
    assert b.i8_fused() is None
    assert b.i8_wide_chains() == [[(b.conv1, "relu", b.bn1, True), (b.conv2, "relu", b.bn2, True), (b.conv3, "relu", b.bn3, True)],
                                  [(b.shortcut, None, b.bn_s, True)]]
    assert len(models._BottleneckBlock(256, 64, (1, 1), False, 2, (0.0,) * 4, 3, "scalar", None, "ste").i8_wide_chains()) == 1


@pytest.mark.parametrize("k", range(len(W.CASES)), ids=W.IDS)
def test_data_conditions_of_the_gpu_cases(k):
    """If a seed fails a condition, change the seed (W.CASES), not the condition."""
    co = W.CASES[k][0]
    out, v = W.reference(k)
    assert np.isfinite(out["scales"]).all() and len(W.chunk_columns(co)) == -(-co // 512) > 1
    # some pixel's absmax channel lies in every chunk, and in every wave's columns: dropping a chunk's or a wave's partial moves a scale
    top = np.abs(v).argmax(axis=1)
    hit = lambda lo, hi: bool(((top >= lo) & (top < hi)).any())                               # noqa: E731
    assert all(hit(*c) for c in W.chunk_columns(co)), np.bincount(top // 512)
    assert all(any(hit(*r) for r in cols) for cols in W.wave_columns(co)), np.bincount(top // 128)
