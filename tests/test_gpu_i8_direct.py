"""GPU tests of the direct int8 convolution (csrc/lq_i8_direct.hpp) against tests/_i8_direct_reference.py: both operands BYTE FOR
BYTE, the product BIT FOR BIT the definition, call_i8_direct BIT FOR BIT the ops composition and, on exact data, F.conv2d in float64.
The one derived bound, against the layer's fake-quantised ``call``: |difference| <= sum_k |w_k| sa(pixel of k) / 2 + 1e-5 sum|terms| -- a
code is the nearest integer of x / sa (nothing clips): half a step of sa per element; the rest is the project's fp32 margin."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_direct_reference as D                                                              # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import layers as L, ops                                         # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                              # noqa: E731
_np = lambda t: t.detach().cpu().numpy()                                                      # noqa: E731
_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)                                     # noqa: E731
_same_bits = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))  # noqa: E731
_same_or_nan = lambda a, b: bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())      # noqa: E731


def _operands(pix, q, sk):
    B, H, W, _ = pix["codes"].shape
    buf, scales = D.pack_kernel(q, sk)
    return (ops.I8Pixels(_t(pix["codes"].view(np.uint8)), _t(pix["scales"]), (B, q.shape[1], H, W)),
            ops.I8ConvKernel(_t(buf), _t(scales), q.shape[0], q.shape[1], (q.shape[2], q.shape[3])))


def _case(g):      # (geometry, pixels, kernel codes, filter scales, bias); a (C, KH, KW) key is the one-hot case of that form
    if len(g) == 3:
        g, pix, q = D.one_hot_case(*g)
        return g, pix, q, np.ones(q.shape[0], np.float32), np.arange(q.shape[0], dtype=np.float32)
    return (g, *D.conv_case(g))


@pytest.mark.parametrize("layout", ["nchw", "channels_last", "cropped_view", "planted"])
@pytest.mark.parametrize("shape", D.PIXEL_SHAPES)
def test_pixels(shape, layout):
    """Whole buffers.  A read outside the view cut out of NaN would put a NaN scale on its pixel; planted: two NaN scales, no more."""
    x = D.gaussian_input(shape, planted=layout == "planted")
    xt = _t(x)
    if layout == "channels_last":
        xt = xt.contiguous(memory_format=torch.channels_last)
    elif layout == "cropped_view":
        xt = torch.full((shape[0], shape[1] + 2, shape[2] + 3, shape[3] + 2), float("nan"), device=DEV)[:, 1:-1, 2:-1, 1:-1].copy_(xt)
    got, ref = ops.i8_pixels_quantize(xt), D.pixels_of(x)
    assert tuple(got.codes.shape) == ref["codes"].shape and (got.codes.numel(), got.scales.numel() * 4) == ops.i8_pixels_bytes(*shape)
    assert np.array_equal(_np(got.codes).view(np.int8), ref["codes"]) and _same_or_nan(_np(got.scales), ref["scales"])
    assert int(np.isnan(_np(got.scales)).sum()) == (2 if layout == "planted" else 0)


@pytest.mark.parametrize("kh,kw", [(1, 1), (3, 3), (3, 2)])
@pytest.mark.parametrize("ci", [3, 32, 64, 96])
@pytest.mark.parametrize("co", [10, 33])
def test_kernel_pack(co, ci, kh, kw):
    rng = np.random.default_rng([co, ci, kh, kw])
    P, s = rng.normal(0.0, 1.0, (co, ci, kh, kw)).astype(np.float32), np.exp2(rng.uniform(-7.0, -5.0, co)).astype(np.float32)
    for qmin, qmax, rounding in ((-128, 127, "nearest"), (-8, 7, "floor")):
        got = ops.i8_conv_kernel_pack(_t(P), _t(s), qmin, qmax, rounding)
        buf, scales = D.pack_kernel(D.kernel_codes(P, s, qmin, qmax, rounding), s)
        assert np.array_equal(_np(got.codes), buf) and np.array_equal(_bits(_np(got.scales)), _bits(scales))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("key", D.GEOMS + D.ONE_HOT)
def test_product_is_the_definition(key, with_bias):
    """Bit for bit, with ldy > co inside a poisoned buffer.  A one-hot case pins every tap and every (lane, byte) of a step in one launch."""
    g, pix, q, sk, bias = _case(key)
    want = D.conv_reference(pix, q, sk, bias if with_bias else None, g[7], D.padding_of(g))
    buf = torch.full((want.shape[0] + 2, want.shape[1] + 5), -7.0, device=DEV)
    out = buf[1:-1, 2:2 + want.shape[1]]
    got = ops.i8_conv2d(*_operands(pix, q, sk), _t(bias) if with_bias else None, g[7], D.padding_of(g), out=out)
    assert got is out and np.array_equal(_bits(_np(got)), _bits(want)), f"{int((_bits(_np(got)) != _bits(want)).sum())} of {want.size} outputs differ"
    out.fill_(-7.0)
    assert bool((buf == -7.0).all())


def test_nan_pixel_spoils_exactly_its_windows():
    g, pix, q, sk, bias = _case(D.GEOMS[0])
    pix = dict(codes=pix["codes"].copy(), scales=pix["scales"].copy())
    pix["scales"][1, 2, 3], pix["codes"][1, 2, 3] = np.nan, 0
    got = _np(ops.i8_conv2d(*_operands(pix, q, sk), _t(bias), g[7], D.padding_of(g)))
    cover = np.pad(np.ones((1, 3, 3), bool), ((1, 0), (1, 1), (2, 2)))      # 3 x 3, stride 1, pad 1: the windows of pixel (1, 2, 3)
    assert np.array_equal(np.isnan(got).reshape(2, 5, 7, -1), np.repeat(cover[..., None], g[4], axis=3))
    assert _same_or_nan(got, D.conv_reference(pix, q, sk, bias, g[7], D.padding_of(g)))


def _layer(cls, g, data_format="NCHW", trained=None, **kw):
    layer = cls(filters=g[4], kernel_size=(g[5], g[6]), strides=g[7], padding=g[8].lower(), scale_gradient="ste", initializer=lq.RandomNormal(seed=3),
                input_shape=g[1], device=DEV, data_format=data_format, trained_weights=trained, **{"bits": 8, "orientation": "scalar", **kw})
    if trained is None:
        layer.init_scales("absmax")
    return layer.eval()


def test_capture_and_replay():
    g = D.GEOMS[1]
    layer, x = _layer(lq.CustomConv2DLayer, g), _t(D.gaussian_input(g[:4]))
    w, s = layer.kernel.detach().permute(3, 2, 0, 1).contiguous(), layer.nested_q_k_layer.scale.detach().reshape(-1)

    def run():
        pix, ker = ops.i8_pixels_quantize(x), ops.i8_conv_kernel_pack(w, s, -128, 127, "nearest")
        return [pix.codes, pix.scales, ker.codes, ker.scales, ops.i8_conv2d(pix, ker, layer.b.detach(), g[7], D.padding_of(g))]

    eager = run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for _ in range(2):
        for o in outs:
            o.fill_(0xEE if o.dtype == torch.uint8 else -7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.uint8), e.view(torch.uint8)) for o, e in zip(outs, eager))


@pytest.mark.parametrize("cls", [lq.CustomConv2DLayer, lq.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
@pytest.mark.parametrize("g", D.EXACT)
def test_call_i8_direct_on_exact_data_is_conv2d_in_float64(g, cls):
    """Every pixel scale is 1.0 and the kernel lies on its grid under a power-of-two scale: every term is an integer, every sum
    below 2^24.  The yardstick: F.conv2d in float64 of the pixels rounded to integers (+-(127 - 2^-15) is code 127)."""
    x, k, bias, scale, bscale = D.exact_case(g)
    layer = _layer(cls, g, trained=[k, bias])
    with torch.no_grad():
        layer.nested_q_k_layer.scale.fill_(float(scale))
        if layer._has_bias:
            layer.nested_q_b_layer.scale.fill_(float(bscale))
    top, bottom, left, right = D.padding_of(g)
    w = torch.from_numpy(np.ascontiguousarray(k.transpose(3, 2, 0, 1)).astype(np.float64))
    want = F.conv2d(F.pad(torch.from_numpy(np.round(x).astype(np.float64)), (left, right, top, bottom)), w, None, g[7]).float()
    want = want + torch.from_numpy(bias).view(1, -1, 1, 1) if layer._has_bias else want
    assert _same_bits(layer.call_i8_direct(_t(x)).cpu(), want)


@pytest.mark.parametrize("data_format", ["NCHW", "NHWC"])
@pytest.mark.parametrize("kw", [dict(bits=8, orientation="scalar"), dict(bits=4, orientation="groupwise", group_size=1000)], ids=["scalar", "per_filter"])
def test_call_i8_direct_is_the_composition_and_near_the_fake_quantised_call(kw, data_format):
    g = (3, *D.GEOMS[1][1:])
    B, C, H, W, co, KH, KW, strides, _ = g
    layer, x, pads = _layer(lq.CustomConv2DLayer, g, data_format, **kw), _t(D.gaussian_input(g[:4], seed=2)), D.padding_of(g)
    with torch.no_grad():
        qb, pix = layer.nested_q_b_layer(layer.b), ops.i8_pixels_quantize(x)
        want = ops.i8_conv2d(pix, layer.i8_direct_operand(), qb, strides, pads).view(B, -1, co)       # (B, OH OW, co)
        inp = x if data_format == "NCHW" else x.permute(0, 2, 3, 1)
        fake = (layer(inp) if data_format == "NCHW" else layer(inp).permute(0, 3, 1, 2)).double()
        for max_lines in (None, want.shape[1], 2 * want.shape[1]):        # the result does not depend on the cut
            got = layer.call_i8_direct(inp, max_lines=max_lines)
            got = got if data_format == "NCHW" else got.permute(0, 3, 1, 2)
            assert _same_bits(got.reshape(B, co, -1).permute(0, 2, 1), want) and got.stride(1) == 1, max_lines
        w = layer.nested_q_k_layer(layer.kernel).permute(3, 2, 0, 1).double().abs()
        pad = lambda t: F.pad(t, (pads[2], pads[3], pads[0], pads[1]))      # noqa: E731
        half = pix.scales.double().unsqueeze(1).expand(B, C, H, W) / 2
        bound = F.conv2d(pad(half), w, None, strides) + 1e-5 * (F.conv2d(pad(x.double().abs()), w, None, strides) + qb.double().abs().view(1, -1, 1, 1))
        err = (got.double() - fake).abs()
    assert bool((err <= bound).all()) and bool((err > 0).any()), float((err / bound).max())


def test_i8_hardware_direct_on_the_cifar_model():
    """Five convs on the direct path, the 3-channel one on im2col; direct=False leaves the bits of the im2col path."""
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=DEV, scale_init="absmax", kernel_storage="oihw", bits=8, orientation="scalar").eval()
    x, convs = torch.rand(2, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)), list(model.convs)
    with torch.no_grad():
        before = model(x)
        with L.i8_hardware(model, convs=True) as hw:
            im2col = model(x)
            assert hw.layers == convs and hw.direct_layers == []
        with L.i8_hardware(model, convs=True, direct=False) as hw:
            assert hw.direct_layers == [] and _same_bits(model(x), im2col)
        with L.i8_hardware(model, convs=True, direct=True) as hw:
            assert hw.layers == convs and hw.direct_layers == convs[1:] and convs[0]._i8_hw is not None and convs[0]._i8_direct_hw is None
            direct = model(x)
        assert all(m._i8_direct_hw is None and m._i8_hw is None for m in convs)
        assert torch.isfinite(direct).all() and not _same_bits(direct, im2col) and _same_bits(model(x), before)
