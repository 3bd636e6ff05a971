"""GPU tests of the direct int8 convolution's residual epilogue (csrc/lq_i8_direct_quant.hpp, RES) against
tests/_i8_conv_residual_reference.py: bytes and bits only.  The data conditions of the cases are tests/test_i8_conv_residual_cpu.py's."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_residual_reference as R                                                       # noqa: E402
from test_gpu_i8_direct import DEV, _bits, _layer, _np, _operands, _same_or_nan, _t           # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

D = R.D
pytestmark = pytest.mark.gpu
_same_bytes = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))  # noqa: E731
_same_pixels = lambda a, b: a.shape == b.shape and _same_bytes(a.codes, b.codes) and _same_bytes(a.scales, b.scales)      # noqa: E731
_is = lambda got, ref: np.array_equal(_np(got.codes).view(np.int8), ref["codes"]) and _same_or_nan(_np(got.scales), ref["scales"])  # noqa: E731
_pixels = lambda res, g: ops.I8Pixels(_t(res["codes"].view(np.uint8)), _t(res["scales"]), (g[0], g[4], *R.out_hw(g)))      # noqa: E731
_decode = lambda px: px.codes[..., :px.shape[1]].view(torch.int8).float() * px.scales.unsqueeze(-1)      # NHWC; one rounding  # noqa: E731
_pair = lambda affine: None if affine is None else (_t(affine[0]), _t(affine[1]))             # noqa: E731


@pytest.mark.parametrize("name", list(R.EPILOGUES))
@pytest.mark.parametrize("co", R.CO)
@pytest.mark.parametrize("gi", [0, 1])
def test_the_definition(gi, co, name):
    """Byte for byte the NumPy reference, and the composition it replaces run on the device."""
    g, pix, q, sk, bias, affine, res, _ = R.base(gi, co)
    act, with_affine, first = R.EPILOGUES[name]
    affine = _pair(affine if with_affine else None)
    ref = R.reference(gi, co, name)[0]
    (p, k), rp = _operands(pix, q, sk), _pixels(res, g)
    got = ops.i8_conv2d_quantize(p, k, _t(bias), g[7], D.padding_of(g), act, affine, first, residual=rp)
    assert got.shape == rp.shape and (got.codes.numel(), got.scales.numel() * 4) == ops.i8_pixels_bytes(*got.shape)
    assert _is(got, ref), f"{int((_np(got.codes).view(np.int8) != ref['codes']).sum())} codes, {int((_bits(_np(got.scales)) != _bits(ref['scales'])).sum())} scales differ"
    y = ops.i8_conv2d(p, k, _t(bias), g[7], D.padding_of(g))
    if first and affine is not None:
        y = y.mul(affine[0]).add(affine[1])
    y = y.add(_decode(rp).reshape(-1, co))
    y = torch.relu(y) if act == "relu" else y
    if not first and affine is not None:
        y = y.mul(affine[0]).add(affine[1])
    assert _same_pixels(got, ops.i8_pixels_quantize(y.view(g[0], *R.out_hw(g), co).permute(0, 3, 1, 2)))


def test_a_residual_of_another_shape_is_refused():
    g, pix, q, sk, bias, _, res, _ = R.base(1, 10)
    p, k = _operands(pix, q, sk)
    rp = _pixels(res, g)
    for bad in (rp._replace(shape=(1, 33, 3, 3)), ops.I8Pixels(rp.codes[:, :2], rp.scales[:, :2], (1, 10, 2, 3))):
        with pytest.raises(ValueError, match="not the output's"):
            ops.i8_conv2d_quantize(p, k, _t(bias), g[7], D.padding_of(g), residual=bad)
    with pytest.raises(ValueError, match="residual.codes must be a contiguous"):
        ops.i8_conv2d_quantize(p, k, _t(bias), g[7], D.padding_of(g), residual=rp._replace(codes=rp.codes.view(torch.int8)))


@pytest.mark.parametrize("kind", ["nan", "zero", "cancel"])
@pytest.mark.parametrize("gi,co", [(0, 33), (1, 144)], ids=["wave", "block"])
def test_planted_values(gi, co, kind):
    """nan: a NaN residual scale spoils exactly its own output pixel (NaN scale, codes 0).  zero: a residual pixel of zero codes
    under 2^-126 leaves its output pixel what the op without a residual writes.  cancel: a residual that is exactly -aff(Y) in
    every channel of a pixel gives u = +0 there: scale 2^-126, codes 0."""
    g, pix, q, sk, bias, affine, res, y = R.base(gi, co)
    at = (g[0] - 1, R.out_hw(g)[0] - 1, 1) if kind != "cancel" else (0, 0, 0)
    if kind == "cancel":
        g, pix, q, sk, bias, affine, res = R.cancelling_case(gi, co)
        y = R.conv_reference(pix, q, sk, bias, g[7], D.padding_of(g))
    else:
        res = dict(codes=res["codes"].copy(), scales=res["scales"].copy())
        res["scales"][at] = np.float32(np.nan if kind == "nan" else 2.0 ** -126)
        if kind == "zero":
            res["codes"][at] = 0
    ref, _, u0, u = R.residual_reference(g, y, res, "relu", affine, True)
    args = (*_operands(pix, q, sk), _t(bias), g[7], D.padding_of(g), "relu", _pair(affine), True)
    got = ops.i8_conv2d_quantize(*args, residual=_pixels(res, g))
    assert _is(got, ref)
    scales, codes = _np(got.scales), _np(got.codes)
    if kind == "nan":
        assert np.isnan(scales[at]) and int(np.isnan(scales).sum()) == 1 and not codes[at].any()
    elif kind == "zero":
        plain = ops.i8_conv2d_quantize(*args)
        assert _bits(scales[at]) == _bits(_np(plain.scales)[at]) and np.array_equal(codes[at], _np(plain.codes)[at]) and codes[at].any()
    else:
        assert (u0[0] != 0).any() and not u[0].any() and _bits(scales[at]) == 0x00800000 and not codes[at].any()


@pytest.mark.parametrize("gi,co", [(0, 70), (1, 144)], ids=["wave", "block"])
def test_memory_contract(gi, co):
    """Exactly lq_i8_pixels_bytes are written (both outputs inside one poisoned arena), and nothing outside the residual's buffers
    is read: they are cut out of allocations poisoned with 0x80 codes and NaN scales, which would move a code or spoil a scale."""
    g, pix, q, sk, bias, affine, res, _ = R.base(gi, co)
    ref = R.reference(gi, co, "add_relu_affine")[0]
    p, k = _operands(pix, q, sk)
    cb, sb = ops.i8_pixels_bytes(g[0], co, *R.out_hw(g))
    pad = 256
    c0, s0 = pad, (2 * pad + cb + 15) // 16 * 16
    arena = torch.full((s0 + sb + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    rc_arena = torch.full((cb + 2 * pad,), 0x80, dtype=torch.uint8, device=DEV)
    rs_arena = torch.full((sb // 4 + 2 * pad // 4,), float("nan"), dtype=torch.float32, device=DEV)
    rc_arena[pad:pad + cb].copy_(_t(res["codes"].view(np.uint8)).reshape(-1))
    rs_arena[pad // 4:pad // 4 + sb // 4].copy_(_t(res["scales"]).reshape(-1))
    assert arena.data_ptr() % 16 == 0 and rc_arena.data_ptr() % 16 == 0 and rs_arena.data_ptr() % 16 == 0
    bias_t, g_t, h_t = _t(bias), _t(affine[0]), _t(affine[1])
    geom = ops._conv_geom(p.shape, (0, 0, 0, 0), k.kernel_size, g[7], D.padding_of(g))
    rc = _hip.load().lq_i8_conv2d_quantize_residual(
        p.codes.data_ptr(), p.scales.data_ptr(), k.codes.data_ptr(), k.scales.data_ptr(), bias_t.data_ptr(), ctypes.byref(geom), co,
        g_t.data_ptr(), h_t.data_ptr(), 1, 0, rc_arena.data_ptr() + pad, rs_arena.data_ptr() + pad, arena.data_ptr() + c0,
        arena.data_ptr() + s0, _hip.stream_ptr(DEV))
    assert rc == 0
    a = _np(arena)
    assert np.array_equal(a[c0:c0 + cb].view(np.int8), ref["codes"].reshape(-1)) and np.array_equal(a[s0:s0 + sb].view(np.uint32), _bits(ref["scales"]).reshape(-1))
    assert (a[:c0] == 0xA5).all() and (a[c0 + cb:s0] == 0xA5).all() and (a[s0 + sb:] == 0xA5).all()


def test_capture_and_replay():
    """One graph with a residual input, replayed after the residual buffers' contents change."""
    g, pix, q, sk, bias, affine, res, _ = R.base(1, 144)
    rp, other = _pixels(res, g), _pixels(R.base(0, 144)[6], g)      # another residual's first bytes: same buffers, other contents
    args = (*_operands(pix, q, sk), _t(bias), g[7], D.padding_of(g), "relu", _pair(affine), True)
    first = ops.i8_conv2d_quantize(*args, residual=rp)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.i8_conv2d_quantize(*args, residual=rp)
    rp.codes.copy_(other.codes.reshape(-1)[:rp.codes.numel()].view_as(rp.codes))
    rp.scales.copy_(other.scales.reshape(-1)[:rp.scales.numel()].view_as(rp.scales))
    second = ops.i8_conv2d_quantize(*args, residual=rp)
    assert not _same_pixels(first, second)
    for _ in range(2):
        out.codes.fill_(0xEE)
        out.scales.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_pixels(out, second)


@pytest.mark.parametrize("stride", [1, 2], ids=["identity", "stride2"])
def test_conv_chain_of_a_residual_block(stride):
    """A step's fifth entry and ``out_pixels=True`` against the composition written out with public ops; the identity block also
    with the batch cut into runs, which slices the residual by the same images."""
    ci, co = (32, 32) if stride == 1 else (64, 70)
    g1 = (2, ci, 5, 7, co, 3, 3, (stride, stride), "SAME")
    c1 = _layer(lq.CustomConv2DLayer, g1)
    c2 = _layer(lq.CustomConv2DLayer, (2, co, 5, 7, co, 3, 3, (1, 1), "SAME"))
    rng = np.random.default_rng(7)
    a1, a2, a_s = ((_t(rng.normal(1.0, 0.5, co).astype(np.float32)), _t(rng.normal(0.0, 1.0, co).astype(np.float32))) for _ in range(3))
    view = lambda a: (a[0].view(1, -1, 1, 1), a[1].view(1, -1, 1, 1))                          # noqa: E731
    with torch.no_grad():
        px = ops.i8_pixels_quantize(_t(D.gaussian_input(g1[:4], seed=4)))
        if stride == 1:
            sc = sc_hand = px
        else:
            short = _layer(lq.CustomConv2DLayer, (2, ci, 5, 7, co, 1, 1, (2, 2), "SAME"))
            sc = L.i8_conv_chain(px, [(short, None, a_s, True)], out_pixels=True)
            y = short.call_i8_direct(px)
            sc_hand = ops.i8_pixels_quantize(y * view(a_s)[0] + view(a_s)[1])
            assert _same_pixels(sc, sc_hand)
        y = c1.call_i8_direct(px)
        y = c2.call_i8_direct(ops.i8_pixels_quantize(torch.relu(y * view(a1)[0] + view(a1)[1])))
        want = ops.i8_pixels_quantize(torch.relu(y * view(a2)[0] + view(a2)[1] + _decode(sc_hand).permute(0, 3, 1, 2)))
        chain = [(c1, "relu", a1, True), (c2, "relu", a2, True, sc)]
        for max_lines in (None, 35) if stride == 1 else (None,):
            assert _same_pixels(L.i8_conv_chain(px, chain, max_lines=max_lines, out_pixels=True), want), max_lines


def _block_by_hand(b, px, last):
    """The block without any epilogue: every conv to fp32 (ops.i8_conv2d), the affine, add and relu in torch, ops.i8_pixels_quantize."""
    def aff(y, bn):
        g, h = L.bn_affine(bn)
        return y * g.view(1, -1, 1, 1) + h.view(1, -1, 1, 1)
    sc = px if b.shortcut is None else ops.i8_pixels_quantize(aff(b.shortcut.call_i8_direct(px), b.bn_s))
    p1 = ops.i8_pixels_quantize(torch.relu(aff(b.conv1.call_i8_direct(px), b.bn1)))
    v = torch.relu(aff(b.conv2.call_i8_direct(p1), b.bn2) + _decode(sc).permute(0, 3, 1, 2))
    return v if last else ops.i8_pixels_quantize(v)


def test_the_resnet18_model_under_fused_convs():
    model = lq.build_model("imagenette", mode="ste", value=0.0, seed=3, device=DEV, scale_init="absmax", kernel_storage="oihw", bits=8,
                           orientation="scalar", input_shape=(3, 32, 32))
    gen = torch.Generator(device=DEV).manual_seed(2)
    rand = lambda n, lo, hi: torch.rand(n, device=DEV, generator=gen) * (hi - lo) + lo        # noqa: E731
    x = torch.rand(2, 3, 32, 32, device=DEV, generator=gen)
    with torch.no_grad():
        for m in model.modules():                         # affines other than the identity
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(rand(n, -0.5, 0.5)), m.running_var.copy_(rand(n, 0.5, 2.0)), m.weight.copy_(rand(n, 0.5, 1.5)), m.bias.copy_(rand(n, -0.5, 0.5))
        model.eval()
        before, state = model(x), {k: v.clone() for k, v in model.state_dict().items()}
        convs = [c for b in model.blocks for c in ([b.conv1, b.conv2] + ([b.shortcut] if b.shortcut is not None else []))]
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True) as hw:
            assert len(hw.fused_conv_layers) == 19 and hw.fused_conv_layers == convs
            got = model(x)
        assert all(c._i8_chain_hw is None and c._i8_direct_hw is None for c in convs) and all(b._i8_fused_convs is None for b in model.blocks)
        assert all(b.i8_fused() is None for b in model.blocks) and all(_same_bytes(v.reshape(-1), state[k].reshape(-1)) for k, v in model.state_dict().items())
        with L.i8_hardware(model, convs=True, direct=True):            # the stem, bn0, relu and the pool are where direct=True puts them
            h = torch.relu(model.bn0(model.stem(x)))
        h = torch.nn.functional.max_pool2d(torch.nn.functional.pad(h, (0, 1, 0, 1), value=float("-inf")), 3, 2)
        a = ops.i8_pixels_quantize(h)
        for k, b in enumerate(model.blocks):
            a = _block_by_hand(b, a, k == len(model.blocks) - 1)
        want = lq.losses.softmax(model.out(a.mean(dim=(2, 3))), dim=1)
        assert _same_bytes(got, want) and torch.isfinite(got).all() and not _same_bytes(got, before)
