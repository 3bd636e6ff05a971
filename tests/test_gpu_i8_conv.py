"""GPU tests of the int8 im2col operand of a convolution (csrc/lq_i8_conv.hpp: k_i8_im2col; include/lq_hip.h: lq_i8_operand_im2col)
and of what is built on it: ops.i8_operand_im2col, the conv layers' i8_operand / call_i8, layers.i8_hardware(convs=True) and
train.i8_eval(convs=True).  The reference is tests/_i8_conv_reference.py (the im2col of tests/_mx_conv_reference.py under the operand
of tests/_i8_reference.py); the geometries and what each exercises are listed there, the proof that they reach every launch form
is tests/test_i8_conv_cpu.py's, which also asserts the conditions of every input used here without a device.

The bar: the operand is BYTE FOR BYTE, the padding of lines and of k and the scales of lines past M included, what the NumPy
reference packs and what ops.i8_operand_quantize writes for the unfolded matrix on the device; call_i8 is BIT FOR BIT the
composition unfold -> quantize -> i8_gemm, BIT FOR BIT tests/_i8_reference.py's gemm_reference of the two reference operands, and on
exact data BIT FOR BIT F.conv2d computed in float64.  The one derived exception: the hardware path against emulate=True on the same
input is held to tests/_bounds.py::assert_within_terms (1e-5 * sum|terms|) -- the integer sums are exact and only the per-period
fp32 product, the fp32 additions and the bias round: at K <= 1152 at most 19 roundings of 2^-24 relative, about 1.1e-6."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_reference as R                                                                # noqa: E402
import _i8_reference as I                                                                     # noqa: E402
import _mx_conv_reference as C                                                                # noqa: E402
from _arena import Arena                                                                      # noqa: E402
from _bounds import assert_within_terms, stable_seed                                          # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402

pytestmark = pytest.mark.gpu
_gid = C.geom_id


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _args(g):
    return (g.KH, g.KW), (g.sh, g.sw), C.padding_of(g)


def _unfolded(x, kernel_size, strides, padding):
    """The im2col matrix (M, K) as the parent can already build it on the device: F.pad -> F.unfold -> a transposing copy."""
    top, bottom, left, right = padding
    u = F.unfold(F.pad(x, (left, right, top, bottom)), kernel_size, stride=strides)
    return u.transpose(1, 2).reshape(-1, u.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def _input(g):
    x = R.gaussian_input(g)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(g, block):
    """(operand dict, documented code buffer, documented scale buffer) of the contiguous Gaussian input: computed once, shared."""
    return R.reference(_input(g), g, block)


def _scale_bits(t):
    return _np(t).view(np.uint32)


def _equal_buffers(op, wc, ws):
    return np.array_equal(_np(op.codes), wc) and np.array_equal(_scale_bits(op.scales), ws.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 1 operand bytes
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_operand_bytes(dev, case):
    g, block = case
    M, K, OH, OW = C.dims(g)
    ref, wc, ws = _reference(g, block)
    x = _t(_input(g), dev)
    op = ops.i8_operand_im2col(x, *_args(g), block)
    assert isinstance(op, ops.I8Operand) and (op.lines, op.K, op.block, op.out_hw) == (M, K, block, (OH, OW))
    assert (op.codes.numel(), op.scales.numel() * 4) == ops.i8_operand_bytes(M, K, block)
    bad = I.buffers_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, f"against the NumPy reference: {bad}"
    assert _equal_buffers(op, wc, ws)
    want = ops.i8_operand_quantize(_unfolded(x, *_args(g)), block)
    assert torch.equal(op.codes, want.codes) and torch.equal(op.scales.view(torch.int32), want.scales.view(torch.int32)), \
        "against i8_operand_quantize(unfold(x))"


# --------------------------------------------------------------------------------------------------------------- 2 input strides
@pytest.mark.parametrize("layout", ["channels_last", "cropped_view"])
@pytest.mark.parametrize("block", R.BLOCKS)
@pytest.mark.parametrize("g", R.STRIDED_GEOMS, ids=_gid)
def test_input_strides(dev, g, block, layout):
    """A channels-last input and a view cut out of a larger tensor of NaN give the bytes of the contiguous input: a read outside
    the view would put a NaN scale on its pair."""
    _, wc, ws = _reference(g, block)
    x = _t(_input(g), dev)
    if layout == "channels_last":
        xv = x.contiguous(memory_format=torch.channels_last)
        assert xv.stride(1) == 1 or g.C == 1
    else:
        full = torch.full((g.B, g.C + 2, g.H + 4, g.W + 2), float("nan"), device=dev)
        xv = full[:, 1:-1, 2:-2, 1:-1]
        xv.copy_(x)
        assert not xv.is_contiguous() and xv.data_ptr() != full.data_ptr()
    before = xv.clone()
    op = ops.i8_operand_im2col(xv, *_args(g), block)
    assert _equal_buffers(op, wc, ws)
    assert not torch.isnan(op.scales).any() and _same_bits(xv, before)


# -------------------------------------------------------------------------------------------------------------- 3 planted values
@pytest.mark.parametrize("block", R.BLOCKS)
@pytest.mark.parametrize("g,zero_channels", R.PLANTED, ids=["k245", "k576"])
def test_planted_values(dev, g, zero_channels, block):
    """One NaN pixel, one -Inf pixel, one -1e30 pixel and all-zero channels: a NaN scale sits on exactly the pairs whose taps cover
    one of the first two pixels (counted from the definition) and their codes are 0; scale 2^-126 on the all-zero pairs."""
    M, K, _, _ = C.dims(g)
    x, nan_at, inf_at, _ = R.planted_input(g, list(zero_channels))
    cover = R.windows_covering(g, block, *nan_at) | R.windows_covering(g, block, *inf_at)
    op = ops.i8_operand_im2col(_t(x, dev), *_args(g), block)
    got = I.unpack_layout(_np(op.codes), _np(op.scales), M, K, block)
    assert np.array_equal(np.isnan(got["scales"]), cover), f"{np.isnan(got['scales']).sum()} NaN scales, {cover.sum()} pairs cover a planted pixel"
    ref, _, _ = R.reference(x, g, block)
    assert np.array_equal(got["scales"] == R.MIN_SCALE, ref["scales"] == R.MIN_SCALE)
    assert not got["codes"][np.repeat(cover, R.span_of(g, block), axis=1)[:, :K]].any(), "the codes under a NaN scale are 0"
    bad = I.buffers_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, bad


# -------------------------------------------------------------------------------------------------------------- 4 memory contract
@pytest.mark.parametrize("block", [0, 64])
@pytest.mark.parametrize("g", R.STRIDED_GEOMS + [R.CHUNKED], ids=_gid)
def test_memory_contract(dev, g, block):
    """X (4 bytes off the 16-byte grid), codes and scales carved out of one poisoned arena, through the raw C call: the guards keep
    the sentinel and X its bits, and the two buffers are the same whatever they held before -- exactly code_bytes and scale_bytes
    are written, all of them."""
    M, K, _, _ = C.dims(g)
    cb, sb = ops.i8_operand_bytes(M, K, block)
    _, wc, ws = _reference(g, block)
    ar = Arena(dev)
    ar.add("X", "in", data=_input(g), residue=4, row_bytes=g.W * 4)
    ar.add("codes", "some", nbytes=cb)
    ar.add("scales", "some", nbytes=sb)
    ar.build()
    top, bottom, left, right = C.padding_of(g)
    geom = _hip.ConvGeom(g.B, g.C, g.H, g.W, g.C * g.H * g.W, g.H * g.W, g.W, 1, g.KH, g.KW, g.sh, g.sw, top, left, bottom, right)
    lib = _hip.load()
    for preset in (0xA5, 0x00, 0xFF):
        ar.fill("codes", preset)
        ar.fill("scales", preset)
        _hip.check(lib.lq_i8_operand_im2col(ar.ptr("X"), ctypes.byref(geom), block, ar.ptr("codes"), ar.ptr("scales"),
                                            _hip.stream_ptr(dev)), "lq_i8_operand_im2col")
        torch.cuda.synchronize()
        ar.check(f"i8 im2col {_gid(g)} block {block} preset {preset:#x}")
        assert np.array_equal(ar.numpy("codes", np.uint8), wc) and np.array_equal(ar.numpy("scales", np.uint32), ws.view(np.uint32)), hex(preset)


# --------------------------------------------------------------------------------------------------------------- 5 graph capture
def test_capture_and_replay(dev):
    """pack -> im2col -> gemm captured in one graph into pre-allocated buffers, replayed twice into poisoned buffers; two plain runs
    give the same bits."""
    g, co, gs, block = C.GEOMS[1], 24, 64, 128
    M, K, _, _ = C.dims(g)
    rng = np.random.default_rng(stable_seed("i8-conv-capture"))
    x = _t(_input(g), dev)
    W = _t((rng.standard_normal((co, K)) * 0.05).astype(np.float32), dev)
    sw = torch.empty((co, -(-K // gs)), device=dev)
    ops.scale_init_group(W, sw, -8, 7, gs, "absmax")
    bias = _t(rng.standard_normal(co).astype(np.float32), dev)
    eager = []
    for _ in range(2):
        b = ops.i8_operand_pack(W, sw, -8, 7, gs, "nearest")
        a = ops.i8_operand_im2col(x, *_args(g), block)
        eager.append([b.codes, b.scales, a.codes, a.scales, ops.i8_gemm(a, b, bias)])
    for p, q in zip(*eager):
        assert torch.equal(p.view(torch.uint8), q.view(torch.uint8)), "two plain runs differ"
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)      # noqa: E731
    (acb, asb), (bcb, bsb) = ops.i8_operand_bytes(M, K, block), ops.i8_operand_bytes(co, K, gs)
    bc, bs, ac, as_ = u8(bcb), u8(bsb), u8(acb), u8(asb)
    Y = torch.empty((M, co), device=dev)
    outs = [bc, bs, ac, as_, Y]
    top, bottom, left, right = C.padding_of(g)
    geom = _hip.ConvGeom(*x.shape, *x.stride(), g.KH, g.KW, g.sh, g.sw, top, left, bottom, right)
    lib, p = _hip.load(), _hip.ptr

    def launch():
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_i8_operand_pack(p(W), p(sw), -8, 7, 1, co, K, 1, gs, p(bc), p(bs), st), "pack")
        _hip.check(lib.lq_i8_operand_im2col(p(x), ctypes.byref(geom), block, p(ac), p(as_), st), "im2col")
        _hip.check(lib.lq_i8_gemm(p(ac), p(as_), block, p(bc), p(bs), gs, p(bias), p(Y), co, M, co, K, st), "gemm")

    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        for o in outs:
            o.fill_(0xEE if o.dtype == torch.uint8 else -7.0)
        graph.replay()
        torch.cuda.synchronize(dev)
        for k, (o, e) in enumerate(zip(outs, eager[0])):
            assert torch.equal(o.view(torch.uint8).reshape(-1), e.contiguous().view(torch.uint8).reshape(-1)), \
                f"output {k} of the replay differs from the eager call"


# -------------------------------------------------------------------------------------------------------------------- 6 the layer
def _layer(cls, dev, ci, co, kernel_size, strides, padding, data_format="NCHW", seed=3, trained=None, **kw):
    kw.setdefault("bits", 8)
    kw.setdefault("orientation", "scalar")
    layer = cls(filters=co, kernel_size=kernel_size, strides=strides, padding=padding, scale_gradient="ste",
                initializer=lq.RandomNormal(seed=seed), input_shape=ci, device=dev, data_format=data_format, trained_weights=trained, **kw)
    if trained is None:
        layer.init_scales("absmax")
    return layer.eval()


def _composition(layer, x_nchw, act_block):
    """i8_gemm(quantize(unfold(x)), layer.i8_operand(), qb) reshaped: what call_i8 must equal bit for bit.  (B, OH, OW, co)."""
    padding = layer._mx_padding(x_nchw.shape[2], x_nchw.shape[3])
    _, _, OH, OW = ops.mx_im2col_dims(x_nchw.shape, layer.kernel_size, layer.strides, padding)
    a = ops.i8_operand_quantize(_unfolded(x_nchw.contiguous(), layer.kernel_size, layer.strides, padding), act_block)
    with torch.no_grad():
        qb = layer.nested_q_b_layer(layer.b) if layer._has_bias else None
        return ops.i8_gemm(a, layer.i8_operand(), qb).reshape(x_nchw.shape[0], OH, OW, layer.filters)


@pytest.mark.parametrize("padding", ["same", "valid"])
@pytest.mark.parametrize("data_format", ["NCHW", "NHWC"])
@pytest.mark.parametrize("cls", [lq.CustomConv2DLayer, lq.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
def test_call_i8_is_the_composition(dev, cls, data_format, padding):
    """Every max_lines cut included: the result does not depend on it."""
    g = C.Geom(3, 5, 9, 10, 7, 7, 2, 2, padding.upper())
    layer = _layer(cls, dev, g.C, 24, (g.KH, g.KW), (g.sh, g.sw), padding, data_format, bits=4, orientation="groupwise", group_size=64)
    M, K, OH, OW = C.dims(g)
    x = _t(C.gaussian_input(g, seed=2), dev)                                     # logical NCHW
    cl = x.contiguous(memory_format=torch.channels_last)
    for act_block in (0, 128):
        want = _composition(layer, x, act_block)
        if data_format == "NCHW":
            inputs, want = [x, cl], want.permute(0, 3, 1, 2)
        else:                                              # (B, H, W, C): contiguous, and a view of the NCHW-contiguous tensor
            inputs = [cl.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1)]
            assert inputs[0].is_contiguous() and not inputs[1].is_contiguous()
        for inp in inputs:
            for max_lines in (None, OH * OW, OH * OW * 2):
                got = layer.call_i8(inp, act_block, max_lines=max_lines)
                assert not got.requires_grad and _same_bits(got, want), (act_block, tuple(inp.stride()), max_lines)
                if data_format == "NCHW":
                    assert tuple(got.shape) == (g.B, 24, OH, OW) and got.stride() == (OH * OW * 24, 1, OW * 24, 24)
                else:
                    assert tuple(got.shape) == (g.B, OH, OW, 24) and got.is_contiguous()
    assert not _same_bits(layer.call_i8(inputs[0]), layer(inputs[0]).detach()), "the hardware path rounds the activations"


@pytest.mark.parametrize("kw,act_block", [(dict(bits=8, orientation="scalar"), 0), (dict(bits=8, orientation="scalar"), 64),
                                          (dict(bits=4, orientation="groupwise", group_size=64), 0),
                                          (dict(bits=4, orientation="groupwise", group_size=64), 128)],
                         ids=["scalar_act0", "scalar_act64", "gs64_act0", "gs64_act128"])
@pytest.mark.parametrize("cls", [lq.CustomConv2DLayer, lq.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
def test_call_i8_is_the_reference_gemm_of_the_reference_operands(dev, cls, kw, act_block):
    g = C.GEOMS[1]                                         # K = 245: four groups of 64, the last of 53
    co = 24
    layer = _layer(cls, dev, g.C, co, (g.KH, g.KW), (g.sh, g.sw), "same", **kw)
    M, K, OH, OW = C.dims(g)
    x = C.gaussian_input(g, seed=4)
    Wm = _np(layer.kernel.detach().permute(3, 2, 0, 1).reshape(co, K))
    s = _np(layer.nested_q_k_layer.scale.detach())
    groupwise = kw["orientation"] == "groupwise"
    gs = kw["group_size"] if groupwise else K
    sw = s if groupwise else np.full((co, 1), s.reshape(-1)[0], np.float32)
    qmin, qmax = layer.q_range
    b = I.operand_of_parameter(Wm, sw, qmin, qmax, 1, gs, layer.rounding)
    op = layer.i8_operand()
    assert (op.lines, op.K, op.block) == (co, K, 64 if groupwise else 0)
    assert I.buffers_mismatch(_np(op.codes), _np(op.scales), b) is None
    with torch.no_grad():
        qb = _np(layer.nested_q_b_layer(layer.b)) if layer._has_bias else None
    a, _, _ = R.reference(x, g, act_block)
    want = I.gemm_reference(a, b, qb).reshape(g.B, OH, OW, co).transpose(0, 3, 1, 2)
    got = _np(layer.call_i8(_t(x, dev), act_block))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


@pytest.mark.parametrize("cls", [lq.CustomConv2DLayer, lq.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
@pytest.mark.parametrize("g", R.EXACT_GEOMS, ids=_gid)
def test_call_i8_on_exact_data_is_conv2d_in_float64(dev, g, cls):
    """Integer pixels with absmax exactly 127 in every im2col row, a kernel on its own grid under a power-of-two scalar scale,
    act_block = 0: the codes are the pixels and the kernel's integers, and one period covers K, so the layer's result has ONE
    rounding of the product and one of the bias (tests/test_i8_conv_cpu.py asserts the conditions).  LQ_INIT_ABSMAX carries a margin
    of 1 + 2^-22: the activation scale of every line is exactly that number, so the float64 yardstick is F.conv2d of the pixels
    times 1 + 2^-22 (exact in float64) with the kernel (exact), rounded to float32 once, plus the bias in float32.  Bit for bit."""
    co = 24
    k, bias, scale, bscale = R.exact_kernel(g, co)
    x = R.exact_input(g)
    layer = _layer(cls, dev, g.C, co, (g.KH, g.KW), (g.sh, g.sw), g.padding.lower(), trained=[k, bias])
    with torch.no_grad():
        layer.nested_q_k_layer.scale.fill_(float(scale))
        if layer._has_bias:
            layer.nested_q_b_layer.scale.fill_(float(bscale))
            assert torch.equal(layer.nested_q_b_layer(layer.b), layer.b)
        assert torch.equal(layer.nested_q_k_layer(layer.kernel), layer.kernel), "the kernel is not on its own grid"
    top, bottom, left, right = C.padding_of(g)
    w_oihw = torch.from_numpy(np.ascontiguousarray(k.transpose(3, 2, 0, 1)).astype(np.float64))
    x64 = torch.from_numpy(x.astype(np.float64)) * float(R.MARGIN)
    want = F.conv2d(F.pad(x64, (left, right, top, bottom)), w_oihw, None, (g.sh, g.sw)).float()
    if layer._has_bias:
        want = want + torch.from_numpy(bias).view(1, -1, 1, 1)
    got = layer.call_i8(_t(x, dev), 0).cpu()
    assert got.dtype == torch.float32 and _same_bits(got, want), float((got - want).abs().max())


# -------------------------------------------------------------------------------------------------------------------- 7 the model
@pytest.fixture(scope="module", params=[dict(bits=8, orientation="scalar"), dict(bits=4, group_size=64)], ids=["8bit_scalar", "4bit_gs64"])
def cifar(request, dev):
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", kernel_storage="oihw", **request.param)
    x = torch.rand(2, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    return model.eval(), x


def test_i8_hardware_convs_on_the_cifar_model(dev, cifar):
    model, x = cifar
    convs = list(model.convs)
    with torch.no_grad():
        before = model(x)
        conv_before = convs[0](x)
        with L.i8_hardware(model) as hw:                    # without convs: no layer switches
            assert hw.layers == [] and _same_bits(model(x), before)
        checked, seen = [], {}

        def hook(mod, inputs, output):
            operand, qb, act_block = mod._i8_hw
            padding = mod._mx_padding(inputs[0].shape[2], inputs[0].shape[3])
            a = ops.i8_operand_quantize(_unfolded(inputs[0].contiguous(), mod.kernel_size, mod.strides, padding), act_block)
            want = ops.i8_gemm(a, operand, qb).reshape(inputs[0].shape[0], *output.shape[2:], mod.filters).permute(0, 3, 1, 2)
            assert _same_bits(output, want), f"{mod.name}: the output differs from unfold -> quantize -> i8_gemm of its input"
            seen[mod] = (inputs[0].detach(), output.detach())
            checked.append(mod)

        for act_block in (0, 64):
            del checked[:]
            with L.i8_hardware(model, act_block=act_block, convs=True) as hw:
                assert hw.layers == convs and all(L.i8_conv_eligible(m) for m in hw.layers)
                hooks = [m.register_forward_hook(hook) for m in convs]
                inside = model(x)
                for h in hooks:
                    h.remove()
                assert checked == convs
                convs[0].train()                            # training-mode calls keep the fake-quantised path
                assert _same_bits(convs[0](x).detach(), conv_before)
                convs[0].eval()
                assert not _same_bits(convs[0](x), conv_before)
            assert all(m._i8_hw is None for m in convs)
            assert not _same_bits(inside, before), "the hardware path rounds the activations: the output must differ"
            assert torch.isfinite(inside).all()
            assert _same_bits(model(x), before), "forward outside the context changed"
        # the derived exception: hardware against emulate=True on the input each layer saw on the hardware path (act_block 64)
        with L.i8_hardware(model, act_block=64, emulate=True, convs=True) as hw:
            assert hw.layers == convs and isinstance(convs[0]._i8_hw[0], torch.Tensor)
            for m in convs:
                xin, hard = seen[m]
                emulated = m(xin)
                padding = m._mx_padding(xin.shape[2], xin.shape[3])
                A = _np(ops.i8_operand_decode(ops.i8_operand_im2col(xin, m.kernel_size, m.strides, padding, 64))).astype(np.float64)
                Wk = np.abs(_np(m._i8_hw[0]).astype(np.float64))
                terms = np.abs(A) @ Wk + np.abs(_np(m._i8_hw[1]).astype(np.float64))[None, :]
                assert A.shape[1] <= 1152
                assert_within_terms(_np(hard.permute(0, 2, 3, 1)).reshape(-1, m.filters), _np(emulated.permute(0, 2, 3, 1)).reshape(-1, m.filters)
                                    .astype(np.float64), terms, f"{m.name}: hardware against emulate=True")
            emulated = model(x)
        assert torch.isfinite(emulated).all() and not _same_bits(emulated, before) and _same_bits(model(x), before)


def test_i8_eval_convs(dev, cifar):
    """The cifar model has no quantised Dense layer: i8_eval without convs refuses it, as before; with convs=True it reports the six
    convs against their emulation, and its Dense fields are those of a model none of whose Dense layers switch."""
    model, x = cifar
    y = torch.arange(2, device=dev) % 10
    with pytest.raises(ValueError, match="no Dense layer"):
        train.i8_eval(model, x, y)
    with torch.no_grad():
        plain_acc = float((model(x).argmax(1) == y).float().mean())
    out = train.i8_eval(model, x, y, convs=True)
    assert out["i8_eval_conv_layers"] == 6 and np.isfinite(out["i8_eval_conv_max_logit_diff"])
    assert 0.0 <= out["i8_eval_conv_accuracy"] <= 1.0
    assert {k: v for k, v in out.items() if not k.startswith("i8_eval_conv")} == {
        "i8_eval_act_block": 0, "i8_eval_layers": 0, "i8_eval_accuracy": plain_acc, "i8_eval_accuracy_emulated": plain_acc,
        "i8_eval_accuracy_fake": plain_acc, "i8_eval_max_logit_diff": 0.0, "i8_eval_max_logit_diff_fake": 0.0}
    mnist = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", bits=8, orientation="columnwise")
    xm = torch.rand(4, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    with pytest.raises(ValueError, match="convs=True needs a model with a conv layer"):
        train.i8_eval(mnist, xm, torch.arange(4, device=dev) % 10, convs=True)
