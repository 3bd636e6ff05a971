"""GPU tests of the stem convolution (csrc/lq_i8_stem.hpp) against tests/_i8_stem_reference.py: both operands BYTE FOR BYTE, the product
BIT FOR BIT the definition, the epilogue BYTE FOR BYTE the next conv's pixel operand, call_i8_stem BIT FOR BIT F.conv2d in float64 on
exact data, and the models BIT FOR BIT the chain written out with the public ops.  The one derived bound, against the layer's
fake-quantised ``call``: |difference| <= sum_k |w_k| sr(row of k) / 2 + 1e-5 sum|terms| -- a code is the nearest integer of x / sr
(nothing clips): half a step of the ROW scale sr per element; the rest is the project's fp32 margin (tests/test_gpu_i8_direct.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_fused_reference as FR                                                         # noqa: E402
import _i8_direct_reference as D                                                              # noqa: E402
import _i8_stem_reference as S                                                                # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import layers as L, ops                                         # noqa: E402
from learned_quantization_amd.losses import softmax                                           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                              # noqa: E731
_np = lambda t: t.detach().cpu().numpy()                                                      # noqa: E731
_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)                                     # noqa: E731
_same_bits = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))  # noqa: E731
_same_or_nan = lambda a, b: bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())      # noqa: E731
_ids = lambda g: "x".join(str(e) for e in g[:7])                                              # noqa: E731


def _operands(rows, q, sk):
    B, H, W, _ = rows["codes"].shape
    buf, scales = S.pack_kernel(q, sk)
    return (ops.I8Rows(_t(rows["codes"].view(np.uint8)), _t(rows["scales"]), (B, q.shape[1], H, W)),
            ops.I8StemKernel(_t(buf), _t(scales), q.shape[0], q.shape[1], (q.shape[2], q.shape[3])))


@pytest.mark.parametrize("layout", ["nchw", "channels_last", "planted"])
@pytest.mark.parametrize("shape", [g[:4] for g in S.GEOMS[:4]] + [(1, 3, 2, 300)], ids=str)      # W = 300: past the 256 pixels a wave keeps
def test_rows(shape, layout):
    """Whole buffers.  planted: a zero row (scale 2^-126, codes 0) and one NaN row, no more."""
    x = S.row_input(shape, planted=layout == "planted")
    xt = _t(x).contiguous(memory_format=torch.channels_last) if layout == "channels_last" else _t(x)
    got, ref = ops.i8_rows_quantize(xt), S.rows_of(x)
    assert tuple(got.codes.shape) == ref["codes"].shape and (got.codes.numel(), got.scales.numel() * 4) == ops.i8_rows_bytes(*shape)
    assert np.array_equal(_np(got.codes).view(np.int8), ref["codes"]) and _same_or_nan(_np(got.scales), ref["scales"])
    assert int(np.isnan(_np(got.scales)).sum()) == (1 if layout == "planted" else 0)
    if layout == "planted":
        assert _np(got.scales)[0, 0] == np.float32(2.0 ** -126) and not _np(got.codes)[0, 0].any()


@pytest.mark.parametrize("g", S.GEOMS[:4], ids=_ids)
def test_kernel_pack(g):
    co, ci, kh, kw = g[4], g[1], g[5], g[6]
    rng = np.random.default_rng([co, ci, kh, kw])
    P, s = rng.normal(0.0, 1.0, (co, ci, kh, kw)).astype(np.float32), np.exp2(rng.uniform(-7.0, -5.0, co)).astype(np.float32)
    for qmin, qmax, rounding in ((-128, 127, "nearest"), (-8, 7, "floor")):
        got = ops.i8_stem_kernel_pack(_t(P), _t(s), qmin, qmax, rounding)
        buf, scales = S.pack_kernel(D.kernel_codes(P, s, qmin, qmax, rounding), s)
        assert np.array_equal(_np(got.codes), buf) and np.array_equal(_bits(_np(got.scales)), _bits(scales))


def _case(key):
    if key == "one_hot":      # every (i, j, c) of the 7 x 7 stem is a filter of its own: 147 filters, ten column tiles on grid.y
        g, rows, q = S.one_hot_case()
        return g, rows, q, np.ones(q.shape[0], np.float32), np.arange(q.shape[0], dtype=np.float32), None
    return (key, *S.conv_case(key))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("key", S.GEOMS + ["one_hot"], ids=lambda k: k if isinstance(k, str) else _ids(k))
def test_product_is_the_definition(key, with_bias):
    """Bit for bit, with ldy > co inside a poisoned buffer."""
    g, rows, q, sk, bias, _ = _case(key)
    want = S.conv_reference(rows, q, sk, bias if with_bias else None, g[7], S.padding_of(g))
    buf = torch.full((want.shape[0] + 2, want.shape[1] + 5), -7.0, device=DEV)
    out = buf[1:-1, 2:2 + want.shape[1]]
    got = ops.i8_stem_conv2d(*_operands(rows, q, sk), _t(bias) if with_bias else None, g[7], S.padding_of(g), out=out)
    assert got is out and np.array_equal(_bits(_np(got)), _bits(want)), f"{int((_bits(_np(got)) != _bits(want)).sum())} of {want.size} outputs differ"
    out.fill_(-7.0)
    assert bool((buf == -7.0).all())


@pytest.mark.parametrize("epilogue", ["none", "relu", "relu_affine", "affine_relu", "affine"])
@pytest.mark.parametrize("g", S.GEOMS, ids=_ids)
def test_epilogue_is_the_next_pixel_operand(g, epilogue):
    """{none, relu} x {no affine, affine_first 0 / 1}, whole buffers: the padding of a ragged co is written, not left."""
    act, with_affine, first = {**FR.EPILOGUES, "affine": (None, True, False)}[epilogue]
    _, rows, q, sk, bias, affine = _case(g)
    ref = S.fused_reference(g, rows, q, sk, bias, act, affine if with_affine else None, first)
    got = ops.i8_stem_conv2d_quantize(*_operands(rows, q, sk), _t(bias), g[7], S.padding_of(g), act,
                                      (_t(affine[0]), _t(affine[1])) if with_affine else None, first)
    assert tuple(got.codes.shape) == ref["codes"].shape and got.shape[1] == g[4]
    assert np.array_equal(_np(got.codes).view(np.int8), ref["codes"]) and np.array_equal(_bits(_np(got.scales)), _bits(ref["scales"]))


def _layer(cls, g, data_format="NCHW", trained=None, **kw):
    pad = g[8].lower() if isinstance(g[8], str) else "same"
    layer = cls(filters=g[4], kernel_size=(g[5], g[6]), strides=g[7], padding=pad, scale_gradient="ste", initializer=lq.RandomNormal(seed=3),
                input_shape=g[1], device=DEV, data_format=data_format, trained_weights=trained, **{"bits": 8, "orientation": "scalar", **kw})
    if trained is None:
        layer.init_scales("absmax")
    return layer.eval()


def test_capture_and_replay():
    g = S.STEM
    layer, x = _layer(lq.CustomConv2DLayer, g), _t(S.row_input(g[:4]))
    operand, qb = layer.i8_stem_operand(), layer.b.detach()

    def run():
        rows = ops.i8_rows_quantize(x)
        nxt = ops.i8_stem_conv2d_quantize(rows, operand, qb, g[7], S.padding_of(g), "relu")
        return [rows.codes, rows.scales, ops.i8_stem_conv2d(rows, operand, qb, g[7], S.padding_of(g)), nxt.codes, nxt.scales]

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
@pytest.mark.parametrize("g", [S.GEOMS[0], S.STEM], ids=_ids)
def test_call_i8_stem_on_exact_data_is_conv2d_in_float64(g, cls):
    """Every row scale is 1.0 and the kernel lies on its grid under a power-of-two scale: every term is an integer, every sum below
    2^24.  The yardstick: F.conv2d in float64 of the pixels rounded to integers (+-(127 - 2^-15) is code 127)."""
    x, k, bias, scale, bscale = D.exact_case(g)      # +-(127 - 2^-15) in every pixel: every ROW scale is 1.0 too
    layer = _layer(cls, g, trained=[k, bias])
    with torch.no_grad():
        layer.nested_q_k_layer.scale.fill_(float(scale))
        if layer._has_bias:
            layer.nested_q_b_layer.scale.fill_(float(bscale))
    top, bottom, left, right = S.padding_of(g)
    w = torch.from_numpy(np.ascontiguousarray(k.transpose(3, 2, 0, 1)).astype(np.float64))
    want = F.conv2d(F.pad(torch.from_numpy(np.round(x).astype(np.float64)), (left, right, top, bottom)), w, None, g[7]).float()
    want = want + torch.from_numpy(bias).view(1, -1, 1, 1) if layer._has_bias else want
    assert _same_bits(layer.call_i8_stem(_t(x)).cpu(), want)


@pytest.mark.parametrize("data_format", ["NCHW", "NHWC"])
def test_call_i8_stem_is_the_composition_and_near_the_fake_quantised_call(data_format):
    g = (3, *S.STEM[1:])
    B, C, H, W, co, KH, KW, strides, _ = g
    layer, x, pads = _layer(lq.CustomConv2DLayer, g, data_format), _t(S.row_input(g[:4], seed=2)), S.padding_of(g)
    with torch.no_grad():
        qb, rows = layer.nested_q_b_layer(layer.b), ops.i8_rows_quantize(x)
        want = ops.i8_stem_conv2d(rows, layer.i8_stem_operand(), qb, strides, pads).view(B, -1, co)       # (B, OH OW, co)
        inp = x if data_format == "NCHW" else x.permute(0, 2, 3, 1)
        fake = (layer(inp) if data_format == "NCHW" else layer(inp).permute(0, 3, 1, 2)).double()
        for max_lines in (None, want.shape[1], 2 * want.shape[1]):        # the result does not depend on the cut
            got = layer.call_i8_stem(inp, max_lines=max_lines)
            got = got if data_format == "NCHW" else got.permute(0, 3, 1, 2)
            assert _same_bits(got.reshape(B, co, -1).permute(0, 2, 1), want) and got.stride(1) == 1, max_lines
        w = layer.nested_q_k_layer(layer.kernel).permute(3, 2, 0, 1).double().abs()
        pad = lambda t: F.pad(t, (pads[2], pads[3], pads[0], pads[1]))      # noqa: E731
        half = rows.scales.double().view(B, 1, H, 1).expand(B, C, H, W) / 2
        bound = F.conv2d(pad(half), w, None, strides) + 1e-5 * (F.conv2d(pad(x.double().abs()), w, None, strides) + qb.double().abs().view(1, -1, 1, 1))
        err = (got.double() - fake).abs()
    assert bool((err <= bound).all()) and bool((err > 0).any()), float((err / bound).max())


def test_i8_hardware_stem_convs_on_the_cifar_model():
    """pooled_convs + stem_convs: bit for bit the chain written out by hand with the public ops, conv 1 through the stem entry and
    no padded-channel product; stem_convs=False leaves the bits of the path without it, and the model as it was afterwards."""
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=DEV, scale_init="absmax", kernel_storage="oihw", bits=8, orientation="scalar").eval()
    x, convs = torch.rand(2, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)), list(model.convs)
    flags = dict(convs=True, direct=True, fused_convs=True, pooled_convs=True)
    with torch.no_grad():
        before = model(x)
        with L.i8_hardware(model, **flags) as hw:
            assert hw.stem_layers == [] and convs[0]._i8_stem_hw is None
            parent = model(x)
        with L.i8_hardware(model, **flags, stem_convs=False):
            assert _same_bits(model(x), parent)
        chain, pools = model.i8_pooled_chain()
        chain = [(c, act, L.bn_affine(bn) if bn is not None else None, first) for c, act, bn, first in chain]
        with L.i8_hardware(model, **flags, stem_convs=True) as hw:
            assert hw.stem_layers == [convs[0]] and hw.layers == convs and isinstance(convs[0]._i8_chain_hw[0], ops.I8StemKernel)
            got = model(x)
            c, act, affine, first = chain[0]
            a = ops.i8_stem_conv2d_quantize(ops.i8_rows_quantize(x), c.i8_stem_operand(), c.nested_q_b_layer(c.b), c.strides,
                                            c._mx_padding(32, 32), act, affine, first)
            rest = L.i8_conv_chain(a, chain[1:], pools=pools[1:])
        want = model.out(model.drop_dense(model.bn_dense(F.relu(model.dense_1(torch.flatten(
            F.max_pool2d(model.bns[5](F.relu(rest)), 2).permute(0, 2, 3, 1), 1))))))
        assert _same_bits(got, softmax(want, dim=1)) and not _same_bits(got, parent)
        assert all(m._i8_stem_hw is None and m._i8_chain_hw is None for m in convs) and not model._i8_stem_chain
        with L.i8_hardware(model, convs=True, direct=True, stem_convs=True):      # unfused: conv 1 leaves im2col for its call_i8_stem
            assert getattr(convs[0], "_i8_hw", None) is None and _same_bits(convs[0](x), convs[0].call_i8_stem(x))
        assert _same_bits(model(x), before)
