"""GPU tests of the direct int8 convolution's pooled pixel-operand epilogue (csrc/lq_i8_direct_quant_pool.hpp) against
tests/_i8_conv_pool_reference.py: bytes and bits only.  The data conditions of the cases are tests/test_i8_conv_pool_cpu.py's."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_pool_reference as PR                                                          # noqa: E402
from test_gpu_i8_direct import DEV, _bits, _layer, _np, _operands, _same_or_nan, _t           # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

R, D = PR.R, PR.D
pytestmark = pytest.mark.gpu
_same_bytes = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))  # noqa: E731
_is = lambda got, ref: np.array_equal(_np(got.codes).view(np.int8), ref["codes"]) and _same_or_nan(_np(got.scales), ref["scales"])  # noqa: E731


@pytest.mark.parametrize("name", list(R.EPILOGUES))
@pytest.mark.parametrize("co", R.WAVE_CO + R.BLOCK_CO)
@pytest.mark.parametrize("gi", [0, 1, 2])
def test_the_definition(gi, co, name):
    """Byte for byte the NumPy reference, and the composition it replaces run on the device."""
    g, pix, q, sk, bias, affine = PR.case(gi, co)
    act, with_affine, first = R.EPILOGUES[name]
    affine = affine if with_affine else None
    ref = PR.pooled_reference(g, pix, q, sk, bias, act, affine, first)[0]
    p, k = _operands(pix, q, sk)
    got = ops.i8_conv2d_quantize(p, k, _t(bias), g[7], D.padding_of(g), act, None if affine is None else (_t(affine[0]), _t(affine[1])), first, pool=2)
    OH, OW = R.out_hw(g)
    assert got.shape == (g[0], co, OH // 2, OW // 2) and (got.codes.numel(), got.scales.numel() * 4) == ops.i8_pixels_bytes(*got.shape)
    assert _is(got, ref), f"{int((_np(got.codes).view(np.int8) != ref['codes']).sum())} codes, {int((_bits(_np(got.scales)) != _bits(ref['scales'])).sum())} scales differ"
    y = ops.i8_conv2d(p, k, _t(bias), g[7], D.padding_of(g))
    for step in (["aff", "act"] if first else ["act", "aff"]):
        if step == "act" and act == "relu":
            y = torch.relu(y)
        if step == "aff" and affine is not None:
            y = y.mul(_t(affine[0])).add(_t(affine[1]))
    comp = ops.i8_pixels_quantize(F.max_pool2d(y.view(g[0], OH, OW, co).permute(0, 3, 1, 2), 2))
    assert _same_bytes(got.codes, comp.codes) and _same_bytes(got.scales, comp.scales)


@pytest.mark.parametrize("kind", ["bad", "dead", "members"])
@pytest.mark.parametrize("co", [33, 144])
def test_planted_values(co, kind):
    """bad: a NaN and a -Inf input pixel spoil exactly the pooled pixels whose windows cover them (NaN scale, codes 0).  dead: under
    relu a window whose four v are non-positive in every channel gets scale 2^-126 and codes 0.  members: the kernel is the centre
    tap of input channel 0 alone, so an output pixel sees its own input pixel, and window e of image 0 has member e lit."""
    g, pix, q, sk, bias, _ = PR.case(0, co, None if kind == "members" else kind)
    windows = [(0, 0), (0, 1), (0, 2), (1, 0)]             # (ph, pw) of the window whose member e = 2 di + dj holds the maximum
    if kind == "members":
        x = np.zeros(g[:4], np.float32)
        for e, (ph, pw) in enumerate(windows):
            x[0, 0, 2 * ph + e // 2, 2 * pw + e % 2] = 100.0
        pix, q, sk = D.pixels_of(x), np.zeros_like(q), np.ones_like(sk)
        q[:, 0, 1, 1] = 1
    ref, p, v = PR.pooled_reference(g, pix, q, sk, bias, "relu")
    got = ops.i8_conv2d_quantize(*_operands(pix, q, sk), _t(bias), g[7], D.padding_of(g), "relu", pool=2)
    assert _is(got, ref)
    scales, codes = _np(got.scales), _np(got.codes)
    if kind == "bad":
        spoiled = np.isnan(ref["scales"])
        assert 0 < spoiled.sum() < spoiled.size and np.array_equal(np.isnan(scales), spoiled) and not codes[spoiled].any()
    elif kind == "dead":
        dead = (p == 0).all(axis=-1)
        assert dead[0, 0, 0] and not dead.all() and (_bits(scales[dead]) == 0x00800000).all() and not codes[dead].any()
    else:
        members = np.stack([v[0, di:4:2, dj:6:2] for di in (0, 1) for dj in (0, 1)])      # [e][ph][pw][co]
        assert all((members[:, ph, pw].argmax(axis=0) == e).all() and (p[0, ph, pw] > 50).all() for e, (ph, pw) in enumerate(windows))


@pytest.mark.parametrize("gi,co", [(1, 70), (2, 200), (1, 200)], ids=["wave", "block-one-line", "block"])
def test_guard_bands(gi, co):
    """Exactly lq_i8_pixels_bytes of the pooled image are written: both out buffers inside one poisoned arena."""
    g, pix, q, sk, bias, affine = PR.case(gi, co)
    ref = PR.pooled_reference(g, pix, q, sk, bias, "relu", affine, False)[0]
    p, k = _operands(pix, q, sk)
    cb, sb = ops.i8_pixels_bytes(g[0], co, *(d // 2 for d in R.out_hw(g)))
    pad = 256
    c0, s0 = pad, (2 * pad + cb + 15) // 16 * 16
    arena = torch.full((s0 + sb + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    assert arena.data_ptr() % 16 == 0
    bias_t, g_t, h_t = _t(bias), _t(affine[0]), _t(affine[1])
    geom = ops._conv_geom(p.shape, (0, 0, 0, 0), k.kernel_size, g[7], D.padding_of(g))
    rc = _hip.load().lq_i8_conv2d_quantize_pool(p.codes.data_ptr(), p.scales.data_ptr(), k.codes.data_ptr(), k.scales.data_ptr(), bias_t.data_ptr(),
                                                ctypes.byref(geom), co, g_t.data_ptr(), h_t.data_ptr(), 1, 0, 2, arena.data_ptr() + c0,
                                                arena.data_ptr() + s0, _hip.stream_ptr(DEV))
    assert rc == 0
    a = _np(arena)
    assert np.array_equal(a[c0:c0 + cb].view(np.int8), ref["codes"].reshape(-1)) and np.array_equal(a[s0:s0 + sb].view(np.uint32), _bits(ref["scales"]).reshape(-1))
    assert (a[:c0] == 0xA5).all() and (a[c0 + cb:s0] == 0xA5).all() and (a[s0 + sb:] == 0xA5).all()


def test_capture_and_replay():
    g, pix, q, sk, bias, affine = PR.case(1, 144)
    p, k = _operands(pix, q, sk)
    args = (p, k, _t(bias), g[7], D.padding_of(g), "relu", (_t(affine[0]), _t(affine[1])), False)
    ops.i8_conv2d_quantize(*args, pool=2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.i8_conv2d_quantize(*args, pool=2)
    for seed in (0, 1):                                  # the replay reads the operand as it is then
        p.codes.copy_(_t(D.pixels_of(D.gaussian_input(g[:4], seed + 7))["codes"].view(np.uint8)))
        eager = ops.i8_conv2d_quantize(*args, pool=2)
        out.codes.fill_(0xEE)
        out.scales.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bytes(out.codes, eager.codes) and _same_bytes(out.scales, eager.scales)


def test_conv_chain_with_pools_is_the_unfused_composition():
    g1, g2 = (3, 32, 5, 7, 70, 3, 3, (1, 1), "SAME"), (3, 70, 2, 3, 33, 3, 3, (1, 1), "SAME")
    a, b = _layer(lq.CustomConv2DLayer, g1), _layer(lq.CustomConv2DLayer, g2)
    rng = np.random.default_rng(5)
    affine = (_t(rng.normal(1.0, 0.5, 70).astype(np.float32)), _t(rng.normal(0.0, 1.0, 70).astype(np.float32)))
    x = _t(D.gaussian_input(g1[:4], seed=4))
    with torch.no_grad():
        mid = F.max_pool2d(torch.relu(a.call_i8_direct(x)).mul(affine[0].view(1, -1, 1, 1)).add(affine[1].view(1, -1, 1, 1)), 2)
        want, want_pixels = b.call_i8_direct(mid), ops.i8_pixels_quantize(mid)
        for max_lines in (None, 35, 70):                  # the result does not depend on the cut
            got = L.i8_conv_chain(x, [(a, "relu", affine, False), (b, None, None, False)], max_lines=max_lines, pools=[2, None])
            assert got.shape == want.shape and _same_bytes(got, want), max_lines
            px = a.call_i8_direct(x, max_lines, out_pixels=True, activation="relu", affine=affine, pool=2)
            assert px.shape == (3, 70, 2, 3) and _same_bytes(px.codes, want_pixels.codes) and _same_bytes(px.scales, want_pixels.scales)


def test_the_cifar_model_under_pooled_convs():
    """``pooled_convs=False`` is ``fused_convs`` alone, bit for bit; ``pooled_convs=True`` is the chain written out, bit for bit.  From
    ``fused_convs`` alone it differs (7.5e-9 at the largest on these probabilities, printed): the BatchNorm after convs 1 and 3 is
    ``bn_affine``'s in the epilogue, torch's kernel there."""
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=DEV, scale_init="absmax", kernel_storage="oihw", bits=8, orientation="scalar")
    x = torch.rand(2, 3, 32, 32, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    with torch.no_grad():
        model.train()
        model(x)                                          # running statistics other than (0, 1)
        model.eval()
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True) as hw:
            want = model(x)
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True, pooled_convs=False) as hw:
            assert hw.fused_conv_layers == [model.convs[0], model.convs[2], model.convs[4]] and _same_bytes(model(x), want)
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True, pooled_convs=True) as hw:
            assert hw.fused_conv_layers == list(model.convs[:5])
            got = model(x)
        assert all(c._i8_chain_hw is None for c in model.convs) and model._i8_pooled_convs is None and model._i8_fused_convs is None
        h = x                                             # the chain written out: bn_affine's (g, h) where the epilogue applies them
        for (conv, act, bn, _), pool in zip(*model.i8_pooled_chain()):
            h = torch.relu(conv.call_i8_direct(h)) if act == "relu" else conv.call_i8_direct(h)
            if bn is not None:
                g_, h_ = L.bn_affine(bn)
                h = h.mul(g_.view(1, -1, 1, 1)).add(h_.view(1, -1, 1, 1))
            h = F.max_pool2d(h, 2) if pool else h
        h = torch.flatten(F.max_pool2d(model.bns[5](torch.relu(h)), 2).permute(0, 2, 3, 1), 1)
        by_hand = lq.losses.softmax(model.out(model.bn_dense(torch.relu(model.dense_1(h)))), dim=1)
        print("largest |pooled_convs - fused_convs| of the outputs:", float((got - want).abs().max()))
        # NOT bit for bit `want`: fused_convs alone runs torch's BatchNorm kernel on the fp32 result of convs 1 and 3, here the epilogue
        # applies bn_affine's (g, h); the two agree to an ulp or so and an ulp can move a code.  What holds bit for bit is the chain
        assert _same_bytes(got, by_hand) and torch.isfinite(got).all()


def test_refusals_through_python():
    g, pix, q, sk, bias, _ = PR.case(0, 33)
    p, k = _operands(pix, q, sk)
    args = (p, k, _t(bias), g[7], D.padding_of(g))
    res = ops.i8_conv2d_quantize(*args)
    for kw, why in ((dict(pool=3), "pool=3"), (dict(pool=2, residual=res), "not built"), (dict(pool=2, wide=True), "not built")):
        with pytest.raises(ValueError, match=why):
            ops.i8_conv2d_quantize(*args, **kw)
    thin = ops.I8Pixels(p.codes[:, :1].contiguous(), p.scales[:, :1].contiguous(), (2, 32, 1, 7))      # OH = 1
    with pytest.raises(ValueError, match="holds no 2 x 2 window"):
        ops.i8_conv2d_quantize(thin, k, _t(bias), g[7], (1, 1, 1, 1), pool=2)
    with pytest.raises(ValueError, match="without out_pixels=True"):
        _layer(lq.CustomConv2DLayer, g).call_i8_direct(_t(D.gaussian_input(g[:4])), pool=2)
