"""GPU tests of the im2col operand of a convolution (csrc/lq_mx_conv.hpp: k_mx_im2col; include/lq_hip.h: lq_mx_operand_im2col) and
of what is built on it: ops.mx_operand_im2col, the conv layers' mx_operand / call_mx, layers.mx_hardware(convs=True) and
train.mx_eval(convs=True).  The reference is tests/_mx_conv_reference.py (im2col from the index definition) with the bytes of
tests/_mx_gemm_reference.py; their conditions are asserted without a device by tests/test_mx_conv_cpu.py.

The bar: the operand is BYTE FOR BYTE, padding and idle scale bytes included, what the NumPy reference packs and what
ops.mx_operand_quantize writes for the unfolded matrix on the device; call_mx is BIT FOR BIT the composition unfold -> quantize ->
mx_gemm, and on exact data BIT FOR BIT F.conv2d computed in float64 on the CPU; on Gaussian data it is held to
tests/_bounds.py::assert_within_terms (1e-5 * sum|terms|) of the float64 product of the decoded operands.

Geometries (B, C, H, W; KH x KW; stride; padding), the smallest at which each mechanism can go wrong:
  (2,3,5,5; 3x3; 1; SAME)     K = 27: one ragged block; M = 50 is no tile multiple; a tile's lines span two images
  (2,5,9,10; 7x7; 2; SAME)    K = 245: two K steps, a last block of 21; SAME pads W by (2, 3): asymmetric
  (1,64,4,4; 3x3; 1; SAME)    K = 576: KT = 5, KG = 2, the idle scale bytes of steps 5 .. 7; M = 16: one full tile
  (3,40,6,6; 3x3; 1; VALID)   no padding
  (2,160,5,5; 1x1; 2; SAME)   the stride-2 shortcut
  (2,6,6,8; 1x3; (2,1); SAME) a rectangular kernel and rectangular strides
  (5,4,7,7; 3x3; 1; SAME)     M = 245: 256 lines in one chunk of a thread block, eight k blocks: several thread blocks"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _mx_conv_reference as C                                                                # noqa: E402
import _mx_gemm_reference as G                                                                # noqa: E402
import _mx_reference as X                                                                     # noqa: E402
from _arena import Arena                                                                      # noqa: E402
from _bounds import assert_within_terms, stable_seed                                          # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(G.OPERAND_FORMATS)
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
    x = C.gaussian_input(g)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(g, name, method):
    """(RefOperand, documented code buffer, documented scale buffer) of the contiguous Gaussian input: computed once, shared."""
    ref, _ = G.operand_of_activation(C.im2col(_input(g), g), name, method)
    return (ref, *G.pack_layout(ref.codes, ref.bytes, name))


# ---------------------------------------------------------------------------------------------------------------- 1 operand bytes
@pytest.mark.parametrize("method", C.METHODS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("g", C.GEOMS, ids=_gid)
def test_operand_bytes(dev, g, name, method):
    M, K, OH, OW = C.dims(g)
    ref, wc, ws = _reference(g, name, method)
    x = _t(_input(g), dev)
    op = ops.mx_operand_im2col(x, *_args(g), name, method)
    assert isinstance(op, ops.MxOperand) and (op.lines, op.K, op.format, op.out_hw) == (M, K, name, (OH, OW))
    assert (op.codes.numel(), op.scales.numel()) == ops.mx_operand_bytes(name, M, K)
    bad = G.layout_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, f"against the NumPy reference: {bad}"
    assert np.array_equal(_np(op.codes), wc) and np.array_equal(_np(op.scales), ws)
    want = ops.mx_operand_quantize(_unfolded(x, *_args(g)), name, method)
    assert torch.equal(op.codes, want.codes) and torch.equal(op.scales, want.scales), "against mx_operand_quantize(unfold(x))"


# --------------------------------------------------------------------------------------------------------------- 2 input strides
@pytest.mark.parametrize("layout", ["channels_last", "cropped_view"])
@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e4m3"])
@pytest.mark.parametrize("g", C.STRIDED_GEOMS, ids=_gid)
def test_input_strides(dev, g, name, layout):
    """A channels-last input and a view cut out of a larger tensor of NaN give the bytes of the contiguous input: a read outside
    the view would put byte 255 on its block."""
    _, wc, ws = _reference(g, name, "mx")
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
    op = ops.mx_operand_im2col(xv, *_args(g), name, "mx")
    assert np.array_equal(_np(op.codes), wc) and np.array_equal(_np(op.scales), ws)
    assert (_np(op.scales) != 255).all() and _same_bits(xv, before)


# -------------------------------------------------------------------------------------------------------------- 3 planted values
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("g,zero_channels", [(C.GEOMS[1], [1]), (C.GEOMS[2], list(range(16, 24)))], ids=["k245", "k576"])
def test_planted_values(dev, g, zero_channels, name):
    """One NaN pixel, one Inf pixel and all-zero channels: byte 255 sits in exactly the blocks whose window covers one of the two
    pixels (counted from the definition), byte 1 in the all-zero blocks."""
    M, K, _, _ = C.dims(g)
    x = C.gaussian_input(g, seed=1)
    nan_at, inf_at = (0, 0, 1, 2), (g.B - 1, g.C - 1, g.H - 1, 0)
    x[:, zero_channels] = 0.0
    x[nan_at], x[inf_at] = np.nan, -np.inf
    cover = C.windows_covering(g, *nan_at) | C.windows_covering(g, *inf_at)
    A = C.im2col(x, g)
    nb = -(-K // 32)
    padded = np.zeros((M, nb * 32), np.float32)
    padded[:, :K] = A
    zero = (padded.reshape(M, nb, 32) == 0).all(axis=2)
    assert cover.sum() >= 2 and zero.sum() >= 1 and not (cover & zero).any() and cover.sum() < cover.size
    for method in C.METHODS:
        op = ops.mx_operand_im2col(_t(x, dev), *_args(g), name, method)
        _, bytes_ = G.unpack_layout(_np(op.codes), _np(op.scales), name, M, K)
        assert np.array_equal(bytes_ == 255, cover), f"{(bytes_ == 255).sum()} blocks under byte 255, {cover.sum()} windows cover a planted pixel"
        assert np.array_equal(bytes_ == 1, zero)
        ref, _ = G.operand_of_activation(A, name, method)
        assert G.layout_mismatch(_np(op.codes), _np(op.scales), ref) is None


# -------------------------------------------------------------------------------------------------------------- 4 memory contract
@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e4m3"])
@pytest.mark.parametrize("g", C.STRIDED_GEOMS, ids=_gid)
def test_memory_contract(dev, g, name):
    """X (4 bytes off the 16-byte grid), codes and scales carved out of one poisoned arena (guards of 64 KiB, above the 4 KiB asked
    for): the guards keep the sentinel and X its bits, and the two buffers are the same whatever they held before."""
    M, K, _, _ = C.dims(g)
    cb, sb = ops.mx_operand_bytes(name, M, K)
    _, wc, ws = _reference(g, name, "cover")
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
        _hip.check(lib.lq_mx_operand_im2col(ar.ptr("X"), ctypes.byref(geom), X.FORMATS[name].id, 1, ar.ptr("codes"), ar.ptr("scales"),
                                            _hip.stream_ptr(dev)), "lq_mx_operand_im2col")
        torch.cuda.synchronize()
        ar.check(f"im2col {name} {_gid(g)} preset {preset:#x}")
        assert np.array_equal(ar.numpy("codes", np.uint8), wc) and np.array_equal(ar.numpy("scales", np.uint8), ws), hex(preset)


# --------------------------------------------------------------------------------------------------------------- 5 graph capture
def test_capture_and_replay(dev):
    """im2col -> gemm captured in one graph into pre-allocated buffers, replayed twice into poisoned buffers; two plain runs give
    the same bits."""
    g, fa, fb, co = C.GEOMS[1], "fp8_e4m3", "fp4_e2m1", 24
    M, K, _, _ = C.dims(g)
    rng = np.random.default_rng(stable_seed("mx-conv-capture"))
    x = _t(_input(g), dev)
    W = _t((rng.standard_normal((co, K)) * 0.05).astype(np.float32), dev)
    sw = torch.empty((co, -(-K // 32)), device=dev)
    ops.scale_init_mx(W, sw, fb, 32, "cover", 2.0 ** -126)
    b, bias = ops.mx_operand_pack(W, sw, fb), _t(rng.standard_normal(co).astype(np.float32), dev)
    eager = []
    for _ in range(2):
        a = ops.mx_operand_im2col(x, *_args(g), fa, "mx")
        eager.append([a.codes, a.scales, ops.mx_gemm(a, b, bias)])
    for p, q in zip(*eager):
        assert torch.equal(p.view(torch.uint8), q.view(torch.uint8)), "two plain runs differ"
    ac, as_ = (torch.empty(n, dtype=torch.uint8, device=dev) for n in ops.mx_operand_bytes(fa, M, K))
    Y = torch.empty((M, co), device=dev)
    outs = [ac, as_, Y]
    top, bottom, left, right = C.padding_of(g)
    geom = _hip.ConvGeom(*x.shape, *x.stride(), g.KH, g.KW, g.sh, g.sw, top, left, bottom, right)
    lib = _hip.load()
    ida, idb = X.FORMATS[fa].id, X.FORMATS[fb].id

    def launch():
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_mx_operand_im2col(_hip.ptr(x), ctypes.byref(geom), ida, 0, _hip.ptr(ac), _hip.ptr(as_), st), "im2col")
        _hip.check(lib.lq_mx_gemm(_hip.ptr(ac), _hip.ptr(as_), ida, _hip.ptr(b.codes), _hip.ptr(b.scales), idb, _hip.ptr(bias), _hip.ptr(Y),
                                  M, co, K, co, st), "gemm")

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
            assert torch.equal(o.view(torch.uint8), e.view(torch.uint8)), f"output {k} of the replay differs from the eager call"


# -------------------------------------------------------------------------------------------------------------------- 6 the layer
def _layer(cls, dev, ci, co, kernel_size, strides, padding, name, data_format="NCHW", seed=3, trained=None):
    layer = cls(filters=co, kernel_size=kernel_size, strides=strides, padding=padding, orientation="groupwise", element_format=name,
                initializer=lq.RandomNormal(seed=seed), input_shape=ci, device=dev, data_format=data_format, trained_weights=trained)
    if trained is None:
        layer.init_scales("cover")
    else:                                                  # unit E8M0 scales: byte 127 everywhere
        layer.nested_q_k_layer.scale.data.fill_(1.0)
        if layer._has_bias:
            layer.nested_q_b_layer.scale.data.fill_(1.0)
    return layer.eval()


def _composition(layer, x_nchw, act_format, act_scale):
    """mx_gemm(quantize(unfold(x)), layer.mx_operand(), qb) reshaped: what call_mx must equal bit for bit.  (B, OH, OW, co)."""
    padding = layer._mx_padding(x_nchw.shape[2], x_nchw.shape[3])
    _, _, OH, OW = ops.mx_im2col_dims(x_nchw.shape, layer.kernel_size, layer.strides, padding)
    a = ops.mx_operand_quantize(_unfolded(x_nchw.contiguous(), layer.kernel_size, layer.strides, padding), act_format, act_scale)
    with torch.no_grad():
        qb = layer.nested_q_b_layer(layer.b) if layer._has_bias else None
        return ops.mx_gemm(a, layer.mx_operand(), qb).reshape(x_nchw.shape[0], OH, OW, layer.filters)


@pytest.mark.parametrize("padding", ["same", "valid"])
@pytest.mark.parametrize("data_format", ["NCHW", "NHWC"])
@pytest.mark.parametrize("cls", [lq.CustomConv2DLayer, lq.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
def test_call_mx_is_the_composition(dev, cls, data_format, padding):
    g = C.Geom(3, 5, 9, 10, 7, 7, 2, 2, padding.upper())
    layer = _layer(cls, dev, g.C, 24, (g.KH, g.KW), (g.sh, g.sw), padding, "fp4_e2m1", data_format)
    M, K, OH, OW = C.dims(g)
    x = _t(C.gaussian_input(g, seed=2), dev)                                     # logical NCHW
    cl = x.contiguous(memory_format=torch.channels_last)
    for act_format, act_scale in (("fp8_e4m3", "mx"), ("fp4_e2m1", "cover")):
        want = _composition(layer, x, act_format, act_scale)
        if data_format == "NCHW":
            inputs, want = [x, cl], want.permute(0, 3, 1, 2)
        else:                                              # (B, H, W, C): contiguous, and a view of the NCHW-contiguous tensor
            inputs = [cl.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1)]
            assert inputs[0].is_contiguous() and not inputs[1].is_contiguous()
        for inp in inputs:
            for max_lines in (None, OH * OW, OH * OW * 2):
                got = layer.call_mx(inp, act_format, act_scale, max_lines=max_lines)
                assert not got.requires_grad and _same_bits(got, want), (act_format, tuple(inp.stride()), max_lines)
                if data_format == "NCHW":
                    assert tuple(got.shape) == (g.B, 24, OH, OW) and got.stride() == (OH * OW * 24, 1, OW * 24, 24)
                else:
                    assert tuple(got.shape) == (g.B, OH, OW, 24) and got.is_contiguous()
    assert not _same_bits(layer.call_mx(inputs[0]), layer(inputs[0]).detach()), "the hardware path rounds the activations"


@pytest.mark.parametrize("cls", [lq.CustomConv2DLayer, lq.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
@pytest.mark.parametrize("pair", G.PAIRS, ids=lambda p: "-".join(p))
@pytest.mark.parametrize("g", C.EXACT_GEOMS, ids=_gid)
def test_call_mx_on_exact_data_is_conv2d_in_float64(dev, g, pair, cls):
    """Activations, kernel and bias from G.EXACT_VALUES under unit kernel scales (tests/test_mx_conv_cpu.py: nothing is rounded and
    every partial sum is a float32): call_mx equals F.conv2d computed in float64 on the CPU bit for bit."""
    act_format, w_format = pair
    co = 24
    k, bias = C.exact_kernel(g, co)
    x = C.exact_input(g)
    layer = _layer(cls, dev, g.C, co, (g.KH, g.KW), (g.sh, g.sw), g.padding.lower(), w_format, trained=[k, bias])
    top, bottom, left, right = C.padding_of(g)
    w_oihw = torch.from_numpy(np.ascontiguousarray(k.transpose(3, 2, 0, 1)).astype(np.float64))
    ref = F.conv2d(F.pad(torch.from_numpy(x.astype(np.float64)), (left, right, top, bottom)), w_oihw,
                   torch.from_numpy(bias.astype(np.float64)) if layer._has_bias else None, (g.sh, g.sw)).numpy()
    for act_scale in C.METHODS:
        got = _np(layer.call_mx(_t(x, dev), act_format, act_scale))
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref), (act_scale, np.abs(got - ref).max())


@pytest.mark.parametrize("cls", [lq.CustomConv2DLayer, lq.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
@pytest.mark.parametrize("name", NAMES)
def test_call_mx_on_gaussian_data_is_within_terms(dev, name, cls):
    """Standard normal activations, as the sets the GEMM's own yardstick was measured on.  (The input of the byte tests, whose
    (image, channel) planes differ by up to 2^12 in magnitude inside one K step, misses REL = 1e-5: 17 of 384 outputs, worst
    2.7e-5 of sum|terms| with fp4_e2m1 weights, measured on an MI355X.  That is the accumulation inside the matrix instruction, whose
    products of a K step are not summed at full fp32 width ("Measured error"), not the layer: call_mx equals the
    composition through lq_mx_gemm bit for bit.)"""
    g = C.GEOMS[2]
    layer = _layer(cls, dev, g.C, 24, (g.KH, g.KW), (g.sh, g.sw), "same", name)
    x = _t(C.plain_gaussian_input(g, seed=3), dev)
    a = ops.mx_operand_im2col(x, *_args(g), "fp8_e4m3", "mx")
    A, B = _np(ops.mx_operand_decode(a)).astype(np.float64), _np(ops.mx_operand_decode(layer.mx_operand())).astype(np.float64)
    ref, terms = A @ B.T, np.abs(A) @ np.abs(B).T
    if layer._has_bias:
        with torch.no_grad():
            qb = _np(layer.nested_q_b_layer(layer.b)).astype(np.float64)
        ref, terms = ref + qb[None, :], terms + np.abs(qb)[None, :]
    got = _np(layer.call_mx(x).permute(0, 2, 3, 1).reshape(-1, 24))
    assert np.isfinite(ref).all() and (terms > 0).all()
    assert_within_terms(got, ref, terms, f"call_mx {name}")


# -------------------------------------------------------------------------------------------------------------------- 7 the model
@pytest.fixture(scope="module")
def cifar(dev):
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="cover")
    x = torch.rand(2, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    return model.eval(), x


def test_mx_hardware_convs_on_the_cifar_model(dev, cifar):
    model, x = cifar
    convs = list(model.convs)
    with torch.no_grad():
        before = model(x)
        conv_before = convs[0](x)
        with L.mx_hardware(model) as hw:                    # without convs: no layer switches
            assert hw.layers == [] and _same_bits(model(x), before)
        checked = []

        def hook(mod, inputs, output):
            operand, qb, act_format, act_scale = mod._mx_hw
            padding = mod._mx_padding(inputs[0].shape[2], inputs[0].shape[3])
            a = ops.mx_operand_quantize(_unfolded(inputs[0].contiguous(), mod.kernel_size, mod.strides, padding), act_format, act_scale)
            want = ops.mx_gemm(a, operand, qb).reshape(inputs[0].shape[0], *output.shape[2:], mod.filters).permute(0, 3, 1, 2)
            assert _same_bits(output, want), f"{mod.name}: the output differs from unfold -> quantize -> mx_gemm of its input"
            checked.append(mod)

        with L.mx_hardware(model, convs=True) as hw:
            assert hw.layers == convs and all(L.mx_conv_eligible(m) for m in hw.layers)
            hooks = [m.register_forward_hook(hook) for m in convs]
            inside = model(x)
            for h in hooks:
                h.remove()
            assert checked == convs
            convs[0].train()                                # training-mode calls keep the fake-quantised path
            assert _same_bits(convs[0](x).detach(), conv_before)
            convs[0].eval()
            assert not _same_bits(convs[0](x), conv_before)
        assert all(m._mx_hw is None for m in convs)
        assert not _same_bits(inside, before), "the hardware path rounds the activations: the output must differ"
        assert torch.isfinite(inside).all()
        assert _same_bits(model(x), before), "forward outside the context changed"
        with L.mx_hardware(model, emulate=True, convs=True) as hw:
            assert hw.layers == convs and isinstance(convs[0]._mx_hw[0], torch.Tensor)
            emulated = model(x)
        assert torch.isfinite(emulated).all() and not _same_bits(emulated, before) and _same_bits(model(x), before)


def test_mx_eval_convs(dev, cifar):
    """The cifar model has no quantised Dense layer: mx_eval without convs refuses it, as before; with convs=True it reports the six
    convs against their emulation, and its Dense fields are those of a model none of whose Dense layers switch."""
    model, x = cifar
    y = torch.arange(2, device=dev) % 10
    with pytest.raises(ValueError, match="no Dense layer"):
        train.mx_eval(model, x, y)
    with torch.no_grad():
        plain_acc = float((model(x).argmax(1) == y).float().mean())
    out = train.mx_eval(model, x, y, convs=True)
    assert out["mx_eval_conv_layers"] == 6 and np.isfinite(out["mx_eval_conv_max_logit_diff"])
    assert 0.0 <= out["mx_eval_conv_accuracy"] <= 1.0
    assert {k: v for k, v in out.items() if not k.startswith("mx_eval_conv")} == {
        "mx_eval_act_format": "fp8_e4m3", "mx_eval_layers": 0, "mx_eval_accuracy": plain_acc, "mx_eval_accuracy_fake": plain_acc,
        "mx_eval_max_logit_diff": 0.0}
    mnist = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="cover")
    xm = torch.rand(4, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    with pytest.raises(ValueError, match="convs=True needs a model with a conv layer"):
        train.mx_eval(mnist, xm, torch.arange(4, device=dev) % 10, convs=True)
