"""GPU tests of the stem convolution's pooled epilogue (csrc/lq_i8_stem_pool.hpp) against tests/_i8_stem_pool_reference.py: whole
buffers BYTE FOR BYTE the pixel operand of the pooled image."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_fused_reference as FR                                                         # noqa: E402
import _i8_stem_pool_reference as R                                                           # noqa: E402
from test_gpu_i8_stem import DEV, _bits, _np, _operands, _same_bits, _same_or_nan, _t         # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                      # noqa: E402

pytestmark = pytest.mark.gpu


def _check(got, ref, co):
    assert tuple(got.codes.shape) == ref["codes"].shape and got.shape == (ref["codes"].shape[0], co, *ref["codes"].shape[1:3])
    assert np.array_equal(_np(got.codes).view(np.int8), ref["codes"]), f"{int((_np(got.codes).view(np.int8) != ref['codes']).sum())} codes differ"
    assert _same_or_nan(_np(got.scales), ref["scales"])


def _run(g, pads, rows, q, sk, bias, act=None, affine=None, first=False):
    return ops.i8_stem_conv2d_quantize(*_operands(rows, q, sk), None if bias is None else _t(bias), g[7], R.S.padding_of(g), act,
                                       None if affine is None else (_t(affine[0]), _t(affine[1])), first, pool=3, pool_padding=pads)


@pytest.mark.parametrize("epilogue", ["none", "relu_affine", "affine_relu"])
@pytest.mark.parametrize("co", [16, 40, 64, 128])      # a dead tile, a ragged tile (its padding is written), NTT 4, NTT 8
@pytest.mark.parametrize("gi", range(len(R.GEOMS)))
def test_pooled_epilogue_is_the_pooled_pixel_operand(gi, co, epilogue):
    act, with_affine, first = FR.EPILOGUES[epilogue]
    g, pads, rows, q, sk, bias, affine = R.case(gi, co)
    ref, _, _ = R.pooled_reference(g, pads, rows, q, sk, bias, act, affine if with_affine else None, first)
    _check(_run(g, pads, rows, q, sk, bias, act, affine if with_affine else None, first), ref, co)


@pytest.mark.parametrize("planted", ["bad", "dead", "argmax"])
def test_planted_values(planted):
    """bad: NaN and -Inf in v; dead: a window of +0 gets scale 2^-126 and codes 0; argmax: the maximum at each of the nine members."""
    g, pads, rows, q, sk, bias, _ = (*R.argmax_case(), None, None) if planted == "argmax" else R.case(planted == "dead", 40, planted)
    act = "relu" if planted == "dead" else None
    got = _run(g, pads, rows, q, sk, bias, act)
    _check(got, R.pooled_reference(g, pads, rows, q, sk, bias, act)[0], g[4])
    if planted == "dead":
        assert _np(got.scales)[0, 0, 0] == np.float32(2.0 ** -126) and not _np(got.codes)[0, 0, 0].any()


def test_poisoned_surroundings_and_capture():
    """The C entry on views inside poisoned buffers; one captured launch, replayed twice after the input changed (the images swapped)."""
    import ctypes
    g, pads, rows, q, sk, bias, _ = R.case(0, 40)
    ref = R.pooled_reference(g, pads, rows, q, sk, bias, "relu")[0]
    r, k = _operands(rows, q, sk)
    cb, sb = ref["codes"].size, ref["scales"].size      # the views sit 256 bytes inside poisoned buffers
    cbuf, sbuf = torch.full((cb + 512,), 0xEE, dtype=torch.uint8, device=DEV), torch.full((sb + 128,), -7.0, device=DEV)
    codes, scales, bias_t = cbuf[256:256 + cb], sbuf[64:64 + sb], _t(bias)
    geom = ops._conv_geom(r.shape, (0, 0, 0, 0), k.kernel_size, g[7], R.S.padding_of(g))
    launch = lambda: _hip.check(_hip.load().lq_i8_stem_conv2d_quantize_pool(                  # noqa: E731
        r.codes.data_ptr(), r.scales.data_ptr(), k.codes.data_ptr(), k.scales.data_ptr(), bias_t.data_ptr(), ctypes.byref(geom), 40, None,
        None, 1, 0, *pads, codes.data_ptr(), scales.data_ptr(), _hip.stream_ptr(DEV)), "lq_i8_stem_conv2d_quantize_pool")
    same = lambda rc, rs: np.array_equal(_np(codes).view(np.int8), rc.reshape(-1)) and np.array_equal(_bits(_np(scales)), _bits(rs).reshape(-1))  # noqa: E731
    launch()
    assert same(ref["codes"], ref["scales"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    r.codes.copy_(r.codes.flip(0)), r.scales.copy_(r.scales.flip(0))
    for _ in range(2):
        codes.fill_(0xEE), scales.fill_(-7.0)
        assert bool((cbuf == 0xEE).all()) and bool((sbuf == -7.0).all())      # nothing outside the two views was written
        graph.replay()
        torch.cuda.synchronize()
        assert same(ref["codes"][::-1], ref["scales"][::-1])


def test_resnet18_under_stem_pool_is_the_forward_written_out():
    """call_i8_stem(pool=3) is the composition on the device; ResNet18Like under stem_pool=True is the forward written out, bit for bit."""
    model = lq.build_model("imagenette", mode="ste", value=0.0, seed=3, device=DEV, scale_init="absmax", kernel_storage="oihw", bits=8,
                           orientation="scalar", input_shape=(3, 32, 32)).eval()
    gen = torch.Generator(device=DEV).manual_seed(2)
    with torch.no_grad():
        model.bn0.running_mean.normal_(0.0, 0.1, generator=gen), model.bn0.running_var.uniform_(0.5, 2.0, generator=gen)
        x, (gg, hh) = torch.rand(2, 3, 32, 32, device=DEV, generator=gen), L.bn_affine(model.bn0)
        v = F.relu(model.stem.call_i8_stem(x).mul(gg.view(1, -1, 1, 1)).add(hh.view(1, -1, 1, 1)))
        a = ops.i8_pixels_quantize(F.max_pool2d(F.pad(v, (0, 1, 0, 1), value=float("-inf")), 3, 2))
        got = model.stem.call_i8_stem(x, out_pixels=True, activation="relu", affine=(gg, hh), affine_first=True, pool=3)
        assert got.shape == a.shape and torch.equal(got.codes, a.codes) and _same_bits(got.scales, a.scales)
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True, stem_convs=True, stem_pool=True) as hw:
            assert hw.fused_conv_layers[0] is model.stem and len(hw.fused_conv_layers) == 20
            got, fused = model(x), [b.i8_fused() for b in model.blocks]
            for b, f in zip(model.blocks[:-1], fused):
                a = b.forward_pixels(a, f)
            want = lq.losses.softmax(model.out(torch.mean(model.blocks[-1].forward_pixels(a, fused[-1], fp32_out=True), dim=(2, 3))), dim=1)
        assert _same_bits(got, want) and model._i8_stem_pool is None and model.stem._i8_chain_hw is None and model.stem._i8_stem_hw is None
