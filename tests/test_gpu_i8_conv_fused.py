"""GPU tests of the direct int8 convolution's pixel-operand epilogue (csrc/lq_i8_direct_quant.hpp) against
tests/_i8_conv_fused_reference.py: bytes and bits only.  The data conditions of the cases are tests/test_i8_conv_fused_cpu.py's."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_fused_reference as R                                                          # noqa: E402
from test_gpu_i8_direct import DEV, _bits, _layer, _np, _operands, _same_or_nan, _t           # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

D = R.D
pytestmark = pytest.mark.gpu
_same_bytes = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))  # noqa: E731


_is = lambda got, ref: np.array_equal(_np(got.codes).view(np.int8), ref["codes"]) and _same_or_nan(_np(got.scales), ref["scales"])  # noqa: E731


@pytest.mark.parametrize("name", list(R.EPILOGUES))
@pytest.mark.parametrize("co", R.WAVE_CO + R.BLOCK_CO)
@pytest.mark.parametrize("gi", [0, 1])
def test_the_definition(gi, co, name):
    """Byte for byte the NumPy reference, and the composition it replaces run on the device."""
    g, pix, q, sk, bias, affine = R.case(gi, co)
    act, with_affine, first = R.EPILOGUES[name]
    affine = affine if with_affine else None
    ref, _ = R.fused_reference(g, pix, q, sk, bias, act, affine, first)
    p, k = _operands(pix, q, sk)
    got = ops.i8_conv2d_quantize(p, k, _t(bias), g[7], D.padding_of(g), act, None if affine is None else (_t(affine[0]), _t(affine[1])), first)
    assert got.shape == (g[0], co, *R.out_hw(g)) and (got.codes.numel(), got.scales.numel() * 4) == ops.i8_pixels_bytes(*got.shape)
    assert _is(got, ref), f"{int((_np(got.codes).view(np.int8) != ref['codes']).sum())} codes, {int((_bits(_np(got.scales)) != _bits(ref['scales'])).sum())} scales differ"
    y = ops.i8_conv2d(p, k, _t(bias), g[7], D.padding_of(g))
    for step in (["aff", "act"] if first else ["act", "aff"]):
        if step == "act" and act == "relu":
            y = torch.relu(y)
        if step == "aff" and affine is not None:
            y = y.mul(_t(affine[0])).add(_t(affine[1]))
    comp = ops.i8_pixels_quantize(y.view(g[0], *R.out_hw(g), co).permute(0, 3, 1, 2))
    assert _same_bytes(got.codes, comp.codes) and _same_bytes(got.scales, comp.scales)


@pytest.mark.parametrize("kind", ["bad", "dead"])
@pytest.mark.parametrize("co", [33, 144])
@pytest.mark.parametrize("gi", [0, 1])
def test_planted_values(gi, co, kind):
    """bad: a NaN and a -Inf input pixel spoil exactly the output pixels whose windows cover them (NaN scale, codes 0).  dead: under
    relu a pixel whose Y is non-positive in every channel gets scale 2^-126 and codes 0."""
    g, pix, q, sk, bias = R.planted_case(kind, gi, co)
    ref, v = R.fused_reference(g, pix, q, sk, bias, "relu")
    got = ops.i8_conv2d_quantize(*_operands(pix, q, sk), _t(bias), g[7], D.padding_of(g), "relu")
    assert _is(got, ref)
    scales, codes = _np(got.scales), _np(got.codes)
    if kind == "bad":         # the reference's NaN rows are the windows that cover the two pixels (conv_reference skips no such tap)
        spoiled = np.isnan(ref["scales"])
        assert 0 < spoiled.sum() < spoiled.size and np.array_equal(np.isnan(scales), spoiled) and not codes[spoiled].any()
    else:
        dead = (v == 0).all(axis=1).reshape(scales.shape)
        assert dead[0, 0, 0] and not dead.all() and (_bits(scales[dead]) == 0x00800000).all() and not codes[dead].any()


@pytest.mark.parametrize("gi,co", [(0, 70), (1, 200)], ids=["wave", "block"])
def test_guard_bands(gi, co):
    """Exactly lq_i8_pixels_bytes are written: both out buffers inside one poisoned arena."""
    g, pix, q, sk, bias, affine = R.case(gi, co)
    ref, _ = R.fused_reference(g, pix, q, sk, bias, "relu", affine, False)
    p, k = _operands(pix, q, sk)
    cb, sb = ops.i8_pixels_bytes(g[0], co, *R.out_hw(g))
    pad = 256
    c0, s0 = pad, (2 * pad + cb + 15) // 16 * 16
    arena = torch.full((s0 + sb + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    assert arena.data_ptr() % 16 == 0
    bias_t, g_t, h_t = _t(bias), _t(affine[0]), _t(affine[1])
    geom = ops._conv_geom(p.shape, (0, 0, 0, 0), k.kernel_size, g[7], D.padding_of(g))
    rc = _hip.load().lq_i8_conv2d_quantize(p.codes.data_ptr(), p.scales.data_ptr(), k.codes.data_ptr(), k.scales.data_ptr(), bias_t.data_ptr(),
                                           ctypes.byref(geom), co, g_t.data_ptr(), h_t.data_ptr(), 1, 0, arena.data_ptr() + c0, arena.data_ptr() + s0,
                                           _hip.stream_ptr(DEV))
    assert rc == 0
    a = _np(arena)
    assert np.array_equal(a[c0:c0 + cb].view(np.int8), ref["codes"].reshape(-1)) and np.array_equal(a[s0:s0 + sb].view(np.uint32), _bits(ref["scales"]).reshape(-1))
    assert (a[:c0] == 0xA5).all() and (a[c0 + cb:s0] == 0xA5).all() and (a[s0 + sb:] == 0xA5).all()


def test_capture_and_replay():
    g, pix, q, sk, bias, affine = R.case(1, 144)
    p, k = _operands(pix, q, sk)
    args = (p, k, _t(bias), g[7], D.padding_of(g), "relu", (_t(affine[0]), _t(affine[1])), False)
    eager = ops.i8_conv2d_quantize(*args)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.i8_conv2d_quantize(*args)
    for _ in range(2):
        out.codes.fill_(0xEE)
        out.scales.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bytes(out.codes, eager.codes) and _same_bytes(out.scales, eager.scales)


def _by_hand(x, chain, channel_axis):
    """call_i8_direct -> relu -> .mul(g) -> .add(h) -> call_i8_direct, written out."""
    shape = [1, 1, 1, 1]
    shape[channel_axis] = -1
    for conv, act, affine, _ in chain:
        x = conv.call_i8_direct(x)
        x = torch.relu(x) if act == "relu" else x
        x = x.mul(affine[0].view(shape)).add(affine[1].view(shape)) if affine is not None else x
    return x


@pytest.mark.parametrize("data_format", ["NCHW", "NHWC"])
def test_conv_chain_is_the_unfused_composition(data_format):
    g1, g2 = R.geom(0, 70), (3, 70, 5, 7, 33, 3, 3, (2, 2), "SAME")
    a, b = _layer(lq.CustomConv2DLayer, (3, *g1[1:]), data_format), _layer(lq.CustomConv2DLayer, g2, data_format)
    rng = np.random.default_rng(5)
    affine = (_t(rng.normal(1.0, 0.5, 70).astype(np.float32)), _t(rng.normal(0.0, 1.0, 70).astype(np.float32)))
    x = _t(D.gaussian_input((3, *g1[1:4]), seed=4))
    x = x if data_format == "NCHW" else x.permute(0, 2, 3, 1)
    chain = [(a, "relu", affine, False), (b, None, None, False)]
    with torch.no_grad():
        want = _by_hand(x, chain, 1 if data_format == "NCHW" else 3)
        for max_lines in (None, 35, 70):                  # the result does not depend on the cut
            got = L.i8_conv_chain(x, chain, max_lines=max_lines)
            assert got.shape == want.shape and _same_bytes(got, want), max_lines


def test_the_cifar_model_under_fused_convs():
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=DEV, scale_init="absmax", kernel_storage="oihw", bits=8, orientation="scalar")
    x = torch.rand(2, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    with torch.no_grad():
        model.train()
        model(x)                                          # running statistics other than (0, 1)
        model.eval()
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True) as hw:
            assert hw.fused_conv_layers == [model.convs[0], model.convs[2], model.convs[4]]
            got = model(x)
        assert all(c._i8_chain_hw is None for c in model.convs) and model._i8_fused_convs is None
        h = x
        for blk, chain in enumerate(model.i8_conv_chains()):
            chain = [(c, act, None if bn is None else L.bn_affine(bn), first) for c, act, bn, first in chain]
            h = F.max_pool2d(model.bns[2 * blk + 1](torch.relu(_by_hand(h, chain, 1))), 2)
        h = torch.flatten(h.permute(0, 2, 3, 1), 1)
        want = lq.losses.softmax(model.out(model.bn_dense(torch.relu(model.dense_1(h)))), dim=1)
        assert _same_bytes(got, want) and torch.isfinite(got).all()
