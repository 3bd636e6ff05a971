"""GPU tests of the wide pixel-operand epilogue of the direct int8 convolution (csrc/lq_i8_direct_quant_wide.hpp) against
tests/_i8_conv_wide_reference.py: bytes and bits only.  The data conditions of the cases are tests/test_i8_conv_wide_cpu.py's."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_wide_reference as W                                                           # noqa: E402
from test_gpu_i8_conv_residual import _decode, _is, _pair, _pixels, _same_bytes, _same_pixels  # noqa: E402
from test_gpu_i8_direct import DEV, _bits, _np, _operands, _t                                 # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

D, R = W.D, W.R
pytestmark = pytest.mark.gpu


def _case(k):
    """(operands, keyword arguments of ops.i8_conv2d_quantize) of case k."""
    g, pix, q, sk, bias, affine, res, _ = W.base(k)
    act, _, first = W.EPILOGUES[W.CASES[k][3]]
    return _operands(pix, q, sk), dict(bias=_t(bias), strides=g[7], padding=D.padding_of(g), activation=act, affine=_pair(affine),
                                       affine_first=first, residual=None if res is None else _pixels(res, g))


def _c_call(p, kn, a, co, out_codes, out_scales):
    """lq_i8_conv2d_quantize_wide itself, with the operands and epilogue of ``_case``, into the two addresses."""
    geom = ops._conv_geom(p.shape, (0, 0, 0, 0), kn.kernel_size, a["strides"], a["padding"])
    ptr = lambda t: None if t is None else t.data_ptr()                                       # noqa: E731
    post, rp = a["affine"] or (None, None), a["residual"] or ops.I8Pixels(None, None, None)
    return _hip.load().lq_i8_conv2d_quantize_wide(
        ptr(p.codes), ptr(p.scales), ptr(kn.codes), ptr(kn.scales), ptr(a["bias"]), ctypes.byref(geom), co, ptr(post[0]), ptr(post[1]),
        int(a["activation"] == "relu"), int(a["affine_first"]), ptr(rp.codes), ptr(rp.scales), out_codes, out_scales, _hip.stream_ptr(DEV))


@pytest.mark.parametrize("k", range(len(W.CASES)), ids=W.IDS)
def test_the_definition(k):
    """Byte for byte the NumPy reference, and the composition it replaces run on the device."""
    g, co, ref = W.geom(k), W.CASES[k][0], W.reference(k)[0]
    (p, kn), a = _case(k)
    got = ops.i8_conv2d_quantize(p, kn, wide=True, **a)
    assert got.shape == (g[0], co, *R.out_hw(g)) and (got.codes.numel(), got.scales.numel() * 4) == ops.i8_pixels_bytes(*got.shape)
    assert _is(got, ref), f"{int((_np(got.codes).view(np.int8) != ref['codes']).sum())} codes, {int((_bits(_np(got.scales)) != _bits(ref['scales'])).sum())} scales differ"
    y = ops.i8_conv2d(p, kn, a["bias"], g[7], a["padding"])
    aff = (lambda v: v.mul(a["affine"][0]).add(a["affine"][1])) if a["affine"] is not None else (lambda v: v)
    y = aff(y) if a["affine_first"] else y
    y = y.add(_decode(a["residual"]).reshape(-1, co)) if a["residual"] is not None else y
    y = torch.relu(y) if a["activation"] == "relu" else y
    y = y if a["affine_first"] else aff(y)
    assert _same_pixels(got, ops.i8_pixels_quantize(y.view(g[0], *R.out_hw(g), co).permute(0, 3, 1, 2)))


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
def test_the_match_at_512_and_the_refusals(with_res):
    """``wide=True`` at co = 512 goes where the call without it goes, and the C entry point itself gives the same bytes there (one
    chunk through the wide kernel); it refuses co = 2049, and co = 513 is refused without the flag as ever."""
    g, pix, q, sk, bias, affine, res, _ = R.base(1, 512)
    (p, kn), a = _operands(pix, q, sk), dict(bias=_t(bias), strides=g[7], padding=D.padding_of(g), activation="relu", affine=_pair(affine),
                                             affine_first=True, residual=_pixels(res, g) if with_res else None)
    plain = ops.i8_conv2d_quantize(p, kn, **a)
    assert _same_pixels(ops.i8_conv2d_quantize(p, kn, wide=True, **a), plain)
    out = ops.I8Pixels(torch.full_like(plain.codes, 0xEE), torch.full_like(plain.scales, -7.0), plain.shape)
    assert _c_call(p, kn, a, 512, out.codes.data_ptr(), out.scales.data_ptr()) == 0 and _same_pixels(out, plain)
    assert _c_call(p, kn, a, 2049, out.codes.data_ptr(), out.scales.data_ptr()) != 0 and b"co = 2049 is above 2048" in _hip.load().lq_last_error()
    (p, kn), a = _case(int(with_res))
    with pytest.raises(RuntimeError, match="co = 513 is above 512"):
        ops.i8_conv2d_quantize(p, kn, **a)


@pytest.mark.parametrize("k", [2, 11], ids=[W.IDS[2], W.IDS[11]])
def test_memory_contract(k):
    """Exactly lq_i8_pixels_bytes are written (both outputs inside one poisoned arena), and nothing outside the residual's buffers
    is read: they are cut out of allocations poisoned with 0x80 codes and NaN scales, which would move a code or spoil a scale."""
    g, ref = W.geom(k), W.reference(k)[0]
    (p, kn), a = _case(k)
    cb, sb = ops.i8_pixels_bytes(g[0], g[4], *R.out_hw(g))
    pad = 256
    c0, s0 = pad, (2 * pad + cb + 15) // 16 * 16
    arena = torch.full((s0 + sb + pad,), 0xA5, dtype=torch.uint8, device=DEV)
    rc_arena = torch.full((cb + 2 * pad,), 0x80, dtype=torch.uint8, device=DEV)
    rs_arena = torch.full((sb // 4 + 2 * pad // 4,), float("nan"), dtype=torch.float32, device=DEV)
    rc_arena[pad:pad + cb].copy_(a["residual"].codes.reshape(-1))
    rs_arena[pad // 4:pad // 4 + sb // 4].copy_(a["residual"].scales.reshape(-1))
    assert arena.data_ptr() % 16 == 0 and rc_arena.data_ptr() % 16 == 0 and rs_arena.data_ptr() % 16 == 0
    a["residual"] = ops.I8Pixels(rc_arena[pad:], rs_arena[pad // 4:], None)
    assert _c_call(p, kn, a, g[4], arena.data_ptr() + c0, arena.data_ptr() + s0) == 0
    got = _np(arena)
    assert np.array_equal(got[c0:c0 + cb].view(np.int8), ref["codes"].reshape(-1)) and np.array_equal(got[s0:s0 + sb].view(np.uint32), _bits(ref["scales"]).reshape(-1))
    assert (got[:c0] == 0xA5).all() and (got[c0 + cb:s0] == 0xA5).all() and (got[s0 + sb:] == 0xA5).all()


def test_capture_and_replay():
    """One graph of the widest case with a residual, replayed twice after the residual buffers' contents change."""
    (p, kn), a = _case(11)
    first, rp = ops.i8_conv2d_quantize(p, kn, wide=True, **a), a["residual"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.i8_conv2d_quantize(p, kn, wide=True, **a)
    rp.codes.copy_(rp.codes.flip(0))
    rp.scales.copy_(rp.scales.flip(0))
    second = ops.i8_conv2d_quantize(p, kn, wide=True, **a)
    assert not _same_pixels(first, second)
    for _ in range(2):
        out.codes.fill_(0xEE)
        out.scales.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_pixels(out, second)


def _block_by_hand(b, px, last):
    """The bottleneck block without any epilogue: every conv to fp32 (ops.i8_conv2d), the affine, add and relu in torch,
    ops.i8_pixels_quantize."""
    def aff(y, bn):
        g, h = L.bn_affine(bn)
        return y * g.view(1, -1, 1, 1) + h.view(1, -1, 1, 1)
    sc = px if b.shortcut is None else ops.i8_pixels_quantize(aff(b.shortcut.call_i8_direct(px), b.bn_s))
    p1 = ops.i8_pixels_quantize(torch.relu(aff(b.conv1.call_i8_direct(px), b.bn1)))
    p2 = ops.i8_pixels_quantize(torch.relu(aff(b.conv2.call_i8_direct(p1), b.bn2)))
    v = torch.relu(aff(b.conv3.call_i8_direct(p2), b.bn3) + _decode(sc).permute(0, 3, 1, 2))
    return v if last else ops.i8_pixels_quantize(v)


def test_the_resnet50_model_under_wide_convs():
    model = lq.build_model("resnet50", mode="ste", value=0.0, seed=3, device=DEV, scale_init="absmax", kernel_storage="oihw", bits=8,
                           orientation="scalar", input_shape=(3, 64, 64))
    gen = torch.Generator(device=DEV).manual_seed(2)
    rand = lambda n, lo, hi: torch.rand(n, device=DEV, generator=gen) * (hi - lo) + lo        # noqa: E731
    x = torch.rand(2, 3, 64, 64, device=DEV, generator=gen)
    with torch.no_grad():
        for m in model.modules():                         # affines other than the identity
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(rand(n, -0.5, 0.5)), m.running_var.copy_(rand(n, 0.5, 2.0)), m.weight.copy_(rand(n, 0.5, 1.5)), m.bias.copy_(rand(n, -0.5, 0.5))
        model.eval()
        convs = [c for b in model.blocks for c in ([b.conv1, b.conv2, b.conv3] + ([b.shortcut] if b.shortcut is not None else []))]
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True) as hw:       # without the opt-in: unfused, as ever
            assert hw.fused_conv_layers == [] and all(b.i8_fused() is None for b in model.blocks)
            unfused = model(x)
        with L.i8_hardware(model, convs=True, direct=True, fused_convs=True, wide_convs=True) as hw:
            assert len(hw.fused_conv_layers) == 52 and hw.fused_conv_layers == convs
            got = model(x)
        assert all(c._i8_chain_hw is None and c._i8_direct_hw is None for c in convs) and all(b.i8_fused() is None for b in model.blocks)
        with L.i8_hardware(model, convs=True, direct=True):            # the stem, bn0, relu, the pool and the classifier are where direct=True puts them
            h = torch.relu(model.bn0(model.stem(x)))
            a = ops.i8_pixels_quantize(torch.nn.functional.max_pool2d(torch.nn.functional.pad(h, (0, 1, 0, 1), value=float("-inf")), 3, 2))
            for k, b in enumerate(model.blocks):
                a = _block_by_hand(b, a, k == len(model.blocks) - 1)
            want = lq.losses.softmax(model.out(a.mean(dim=(2, 3))), dim=1)
        assert _same_bytes(got, want) and torch.isfinite(got).all() and not _same_bytes(got, unfused)
