"""GPU tests of the packed MX operands and the block-scaled GEMM (csrc/lq_mx_operand.hpp, csrc/lq_mx_gemm.hpp; include/lq_hip.h:
lq_mx_operand_pack / lq_mx_operand_quantize / lq_mx_operand_decode / lq_mx_gemm) against tests/_mx_gemm_reference.py.

The bar: pack -> decode and quantize -> decode equal the fake-quantised values BIT FOR BIT (so the codes and the scale bytes are
the quantizer's); the GEMM on exact data equals the float64 product BIT FOR BIT for all nine format pairs -- the test that pins the
lane map of v_mfma_scale_f32_16x16x128_f8f6f4, its scale bytes and op-sel, the K order, the padding and the masked store --; on
random data it is held to tests/_bounds.py::assert_within_terms (1e-5 * sum|terms|); two runs give the same bits.  The data sets and
their conditions are tests/_mx_gemm_reference.py's, asserted without a device by tests/test_mx_gemm_cpu.py.

Shapes, the smallest at which each mechanism can go wrong:  pack (70, 40) axis 0: one K step, a last block of 6 elements, 40 lines are
no tile multiple; (160, 17) axis 0: a second K step that is a quarter full; (9, 200) and (33, 288) axis 1: the float4 loads, a ragged
block, three line tiles.  GEMM (16, 16, 128): one instruction; (19, 21, 160): every edge masked, a second K step; (37, 10, 784): the
MNIST layer, seven K steps -- a second scale dword, op-sel 0 .. 3; (64, 48, 512): a full block of four waves, an idle wave column;
(81, 70, 160): MT = 6, NT = 5, a grid of 2 x 2 blocks -- blockIdx 1 on both axes, where block 1 has a clamped second N tile and a wave
that leaves on each axis; (17, 18, 1184): KT = 10, KG = 3, a third scale dword that holds two steps, the last a quarter full;
(129, 17, 160) and (17, 129, 160): nine tiles, THREE blocks on one axis -- with two blocks a block stride of one wave instead of two
(blockIdx * 2 -> blockIdx) still covers every tile, twice over, and every result is right; the third block's last tile shows it.

The buffers of pack and quantize are also compared BYTE FOR BYTE, padding included, with the NumPy packer of the layout that
include/lq_hip.h documents (G.pack_layout): the device's decode shares its offset functions with pack and cannot see a wrong order.
Every code and every scale byte through the instruction, one term per output: tests/test_gpu_mx_gemm_codes.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _mx_gemm_reference as G                                                                # noqa: E402
import _mx_reference as X                                                                     # noqa: E402
from _arena import SENTINEL_WORD, Arena                                                       # noqa: E402
from _bounds import REL, assert_within_terms                                                  # noqa: E402
from _clip_reference import bits_equal                                                        # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(G.OPERAND_FORMATS)
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------- 1 pack, then decode
@pytest.mark.parametrize("shape", G.PACK_SHAPES, ids=_ids)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", ["gauss", "loguniform"])
def test_pack_then_decode_is_the_fake_quantised_parameter(dev, kind, name, shape):
    R, C, axis = shape
    P, s = G.pack_case(kind, name, R, C, axis)
    if kind == "gauss":                                    # one NaN element and one bad scale, in different blocks
        P, s = P.copy(), s.copy()
        P[R - 1, C - 2] = np.nan
        s.reshape(-1)[1] = -1.0
    ref = G.operand_of_parameter(P, s, name, axis)
    assert (ref.bytes == 255).sum() == (1 if kind == "gauss" else 0)
    Pt, st = _t(P, dev), _t(s, dev)
    op = ops.mx_operand_pack(Pt, st, name)
    L_, K = (C, R) if axis == 0 else (R, C)
    assert (op.lines, op.K, op.format) == (L_, K, name) and (op.codes.numel(), op.scales.numel()) == ops.mx_operand_bytes(name, L_, K)
    got = _np(ops.mx_operand_decode(op))
    # codes and bytes, through decode: value(code) * 2^(byte - 127) of the reference's code view and scale bytes
    assert bits_equal(got, G.decode(ref, np.float32)), "decode differs from the reference's codes and scale bytes"
    # the buffers themselves, byte for byte, padding included, against the layout include/lq_hip.h documents
    bad = G.layout_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, f"the buffers are not the documented layout of the reference operand: {bad}"
    # and the device's own forward: `out` bit for bit, its code view through the table
    out, code = ops.fq_forward_mx(Pt, st, name, 32, "e8m0", q_dtype=torch.int32)
    turn = (lambda a: np.ascontiguousarray(a.T)) if axis == 0 else np.ascontiguousarray
    assert np.array_equal(turn(_np(code)).astype(np.int64), ref.codes)
    out = turn(_np(out))
    # a NaN element under a valid scale has no code in fp4: there `out` is NaN and the operand holds the NaN code rule's 7 (= 6.0)
    no_code = np.isnan(turn(P)) & (np.repeat(ref.bytes, 32, axis=1)[:, :K] != 255) if name == "fp4_e2m1" else np.zeros(out.shape, bool)
    assert no_code.sum() == (1 if kind == "gauss" and name == "fp4_e2m1" else 0)
    assert bits_equal(np.where(no_code, 0, got), np.where(no_code, 0, out)), "decode differs from lq_fq_forward_mx's out"
    assert (ref.codes[no_code] == 7).all() and np.array_equal(np.isnan(got), np.isnan(out) & ~no_code)
    again = ops.mx_operand_pack(Pt, st, name)
    assert torch.equal(again.codes, op.codes) and torch.equal(again.scales, op.scales), "two packs differ"


# ----------------------------------------------------------------------------------------------------- 2 dynamic quantize
@pytest.mark.parametrize("shape", G.QUANT_SHAPES, ids=_ids)
@pytest.mark.parametrize("method", ["mx", "cover"])
@pytest.mark.parametrize("name", NAMES)
def test_quantize_is_scale_init_then_forward(dev, name, method, shape):
    M, K = shape
    x = G.quantize_case(M, K)
    xt = _t(x, dev)
    op = ops.mx_operand_quantize(xt, name, method)
    got = _np(ops.mx_operand_decode(op))
    # the composition, on the device
    s = torch.empty((M, -(-K // 32)), dtype=torch.float32, device=dev)
    ops.scale_init_mx(xt, s, name, 32, method, min_value=G.MIN_SCALE)
    out = _np(ops.fq_forward_mx(xt, s, name, 32, "e8m0"))
    assert bits_equal(got, out), "quantize -> decode differs from scale_init_mx -> fq_forward_mx"
    assert np.isnan(got[M - 1, ((K - 3) // 32) * 32:]).all() and np.isnan(got).sum() == K - ((K - 3) // 32) * 32      # the Inf's block
    assert not got[1, 32:64].any()                                                                                     # the zero block
    # and the NumPy reference of both steps
    ref, s_ref = G.operand_of_activation(x, name, method)
    assert bits_equal(_np(s), s_ref) and bits_equal(got, G.decode(ref, np.float32))
    bad = G.layout_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, f"the buffers are not the documented layout of the reference operand: {bad}"
    again = ops.mx_operand_quantize(xt, name, method)
    assert torch.equal(again.codes, op.codes) and torch.equal(again.scales, op.scales), "two quantizations differ"


# --------------------------------------------------------------------------------------------------------- 3 GEMM, exact
_EXACT = {}


def _exact(shape, identity):
    key = (shape, identity)
    if key not in _EXACT:
        _EXACT[key] = G.exact_case(*shape, identity)
    return _EXACT[key]


@pytest.mark.parametrize("case", G.EXACT_CASES, ids=lambda c: _ids(c[0]) + ("-identity" if c[1] else ""))
@pytest.mark.parametrize("pair", G.PAIRS, ids=lambda p: "-".join(p))
def test_gemm_exact_is_the_float64_product_bit_for_bit(dev, pair, case):
    shape, identity = case
    M, N, K = shape
    c = _exact(shape, identity)
    ra, rb = G.exact_operands(c, *pair)
    a = ops.mx_operand_pack(_t(c["A"], dev), _t(c["sa"], dev), pair[0])      # axis 1: the lines are the rows
    b = ops.mx_operand_pack(_t(c["W"], dev), _t(c["sw"], dev), pair[1])      # axis 0: the lines are the columns of (in, out)
    assert (a.lines, a.K, b.lines, b.K) == (M, K, N, K)
    for bias in (None, c["bias"]):
        ref, _ = G.gemm_reference(ra, rb, bias)
        Y = _np(ops.mx_gemm(a, b, None if bias is None else _t(bias, dev)))
        assert Y.shape == (M, N) and Y.dtype == np.float32
        bad = np.argwhere(Y.astype(np.float64) != ref)
        assert bad.size == 0, (f"{len(bad)} of {M * N} outputs differ from the exact product, first at (m, n) = {tuple(bad[0])}: got "
                               f"{Y[tuple(bad[0])]!r}, exact {ref[tuple(bad[0])]!r}")


# -------------------------------------------------------------------------------------------------------- 4 GEMM, random
# The accumulation inside the instruction is not documented; the yardstick is the project's REL = 1e-5 on sum|terms|, unchanged.
# Measured on an MI355X (worst err / sum|terms| over the seeds below, K <= 1024; DESIGN.md section 4, "Measured error"): 5.4e-9 and
# 7.8e-9 for fp4 x fp4, 1.0e-6 .. 1.7e-6 with one fp8 side, 2.0e-6 .. 3.2e-6 with two -- a property of the instruction (an fp32
# fmaf chain sits near 1e-7 at this K), a factor of three inside the bound.
@pytest.mark.parametrize("shape", G.RANDOM_SHAPES, ids=_ids)
@pytest.mark.parametrize("pair", G.PAIRS, ids=lambda p: "-".join(p))
def test_gemm_random_within_the_yardstick(dev, pair, shape):
    M, N, K = shape
    worst = 0.0
    for seed in (0, 1):
        c = G.random_case(M, N, K, *pair, seed=seed)
        a = ops.mx_operand_quantize(_t(c["x"], dev), pair[0], "mx")
        b = ops.mx_operand_pack(_t(c["W"], dev), _t(c["sw"], dev), pair[1])
        bias = _t(c["bias"], dev)
        Y = ops.mx_gemm(a, b, bias)
        A, B = _np(ops.mx_operand_decode(a)).astype(np.float64), _np(ops.mx_operand_decode(b)).astype(np.float64)
        ref = A @ B.T + c["bias"].astype(np.float64)[None, :]
        terms = np.abs(A) @ np.abs(B).T + np.abs(c["bias"].astype(np.float64))[None, :]
        ratio = float((np.abs(_np(Y).astype(np.float64) - ref) / terms).max())
        worst = max(worst, ratio)
        print(f"mx_gemm {pair[0]} x {pair[1]} {M}x{N}x{K} seed {seed}: worst err / sum|terms| = {ratio:.3e} (REL = {REL:g})")
        assert_within_terms(_np(Y), ref, terms, f"mx_gemm {pair} {shape} seed {seed}")
        assert torch.equal(ops.mx_gemm(a, b, bias).view(torch.int32), Y.view(torch.int32)), "two runs differ"
    print(f"mx_gemm {pair[0]} x {pair[1]} {M}x{N}x{K}: worst over the seeds {worst:.3e}")


# ------------------------------------------------------------------------------------------------------ 5 memory contract
def _sizes(name, L_, K):
    return ops.mx_operand_bytes(name, L_, K)


@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e4m3"])
@pytest.mark.parametrize("shape", [(70, 40, 0), (33, 288, 1)], ids=_ids)
def test_memory_contract_of_pack(dev, name, shape):
    """Guard bands around the code and scale buffers at their exact sizes; P and s 4 bytes off the 16-byte grid."""
    R, C, axis = shape
    P, s = G.pack_case("gauss", name, R, C, axis)
    L_, K = (C, R) if axis == 0 else (R, C)
    cb, sb = _sizes(name, L_, K)
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=4, row_bytes=C * 4)
    ar.add("s", "in", data=s, residue=4)
    ar.add("codes", "out", nbytes=cb)
    ar.add("scales", "some", nbytes=sb)                    # a padding dword of bytes 127 IS the arena's sentinel word
    ar.build()
    lib = _hip.load()
    _hip.check(lib.lq_mx_operand_pack(ar.ptr("P"), ar.ptr("s"), X.FORMATS[name].id, 0, R, C, axis, 32, ar.ptr("codes"), ar.ptr("scales"),
                                      _hip.stream_ptr(dev)), "lq_mx_operand_pack")
    torch.cuda.synchronize()
    ar.check(f"pack {name} {shape}")
    want = ops.mx_operand_pack(_t(P, dev), _t(s, dev), name)
    assert torch.equal(ar.bytes("codes"), want.codes) and torch.equal(ar.bytes("scales"), want.scales)


@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e4m3"])
@pytest.mark.parametrize("shape", [(5, 100), (33, 288)], ids=_ids)
def test_memory_contract_of_quantize(dev, name, shape):
    """Gaussian rows without an Inf: four NaN codes of fp8_e4m3 in a row (0x7F each) are the arena's sentinel word."""
    M, K = shape
    x = G.random_case(M, 16, K, name, name)["x"]
    cb, sb = _sizes(name, M, K)
    ar = Arena(dev)
    ar.add("X", "in", data=x, residue=4, row_bytes=K * 4)
    ar.add("codes", "out", nbytes=cb)
    ar.add("scales", "some", nbytes=sb)
    ar.build()
    lib = _hip.load()
    _hip.check(lib.lq_mx_operand_quantize(ar.ptr("X"), X.FORMATS[name].id, 1, M, K, ar.ptr("codes"), ar.ptr("scales"),
                                          _hip.stream_ptr(dev)), "lq_mx_operand_quantize")
    torch.cuda.synchronize()
    ar.check(f"quantize {name} {shape}")
    want = ops.mx_operand_quantize(_t(x, dev), name, "cover")
    assert torch.equal(ar.bytes("codes"), want.codes) and torch.equal(ar.bytes("scales"), want.scales)


@pytest.mark.parametrize("shape", [(19, 21, 160), (37, 10, 784), (81, 70, 160)], ids=_ids)
def test_memory_contract_of_gemm(dev, shape):
    """Guard bands around Y with ldy = N + 3: the three columns between the rows keep the sentinel; the bias 4 bytes off the grid."""
    M, N, K = shape
    c = _exact(shape, False)
    a = ops.mx_operand_pack(_t(c["A"], dev), _t(c["sa"], dev), "fp8_e4m3")
    b = ops.mx_operand_pack(_t(c["W"], dev), _t(c["sw"], dev), "fp4_e2m1")
    ldy = N + 3
    ar = Arena(dev)
    for key, t in (("a_codes", a.codes), ("a_scales", a.scales), ("b_codes", b.codes), ("b_scales", b.scales)):
        ar.add(key, "in", data=_np(t))
    ar.add("bias", "in", data=c["bias"], residue=4)
    ar.add("Y", "some", nbytes=((M - 1) * ldy + N) * 4, residue=4, row_bytes=ldy * 4)
    ar.build()
    lib = _hip.load()
    _hip.check(lib.lq_mx_gemm(ar.ptr("a_codes"), ar.ptr("a_scales"), X.FORMATS["fp8_e4m3"].id, ar.ptr("b_codes"), ar.ptr("b_scales"),
                              X.FORMATS["fp4_e2m1"].id, ar.ptr("bias"), ar.ptr("Y"), M, N, K, ldy, _hip.stream_ptr(dev)), "lq_mx_gemm")
    torch.cuda.synchronize()
    ar.check(f"gemm {shape}")
    flat = np.concatenate([ar.numpy("Y", np.uint32), np.full(3, SENTINEL_WORD, np.uint32)]).reshape(M, ldy)
    assert (flat[:, N:] == SENTINEL_WORD).all(), "the columns between the rows of Y were written"
    ref, _ = G.gemm_reference(*G.exact_operands(c, "fp8_e4m3", "fp4_e2m1"), c["bias"])
    assert np.array_equal(np.ascontiguousarray(flat[:, :N]).view(np.float32).astype(np.float64), ref)


# ------------------------------------------------------------------------------------------------------ 6 capture and out=
def test_capture_and_replay(dev):
    """pack -> quantize -> gemm -> decode, one launch each, captured into pre-allocated buffers in one graph; the outputs are
    poisoned before each of two replays and equal the eager results bit for bit."""
    M, N, K = 19, 21, 160
    fa, fb = "fp8_e4m3", "fp4_e2m1"
    c = G.random_case(M, N, K, fa, fb)
    x, W, sw, bias = _t(c["x"], dev), _t(c["W"], dev), _t(c["sw"], dev), _t(c["bias"], dev)
    ea, eb = ops.mx_operand_quantize(x, fa, "mx"), ops.mx_operand_pack(W, sw, fb)
    eager = [eb.codes, eb.scales, ea.codes, ea.scales, ops.mx_gemm(ea, eb, bias), ops.mx_operand_decode(ea)]
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)      # noqa: E731
    ac, as_, bc, bs = (u8(n) for n in ops.mx_operand_bytes(fa, M, K) + ops.mx_operand_bytes(fb, N, K))
    Y, D = torch.empty((M, N), device=dev), torch.empty((M, K), device=dev)
    outs = [bc, bs, ac, as_, Y, D]
    lib = _hip.load()
    ida, idb = X.FORMATS[fa].id, X.FORMATS[fb].id

    def launch():
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_mx_operand_pack(_hip.ptr(W), _hip.ptr(sw), idb, 0, K, N, 0, 32, _hip.ptr(bc), _hip.ptr(bs), st), "pack")
        _hip.check(lib.lq_mx_operand_quantize(_hip.ptr(x), ida, ops.check_mx_scale_init("mx"), M, K, _hip.ptr(ac), _hip.ptr(as_), st), "quantize")
        _hip.check(lib.lq_mx_gemm(_hip.ptr(ac), _hip.ptr(as_), ida, _hip.ptr(bc), _hip.ptr(bs), idb, _hip.ptr(bias), _hip.ptr(Y), M, N, K,
                                  N, st), "gemm")
        _hip.check(lib.lq_mx_operand_decode(_hip.ptr(ac), _hip.ptr(as_), ida, M, K, _hip.ptr(D), st), "decode")

    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        for o in outs:
            o.fill_(0xEE if o.dtype == torch.uint8 else -7.0)
        g.replay()
        torch.cuda.synchronize(dev)
        for k, (o, e) in enumerate(zip(outs, eager)):
            assert torch.equal(o.view(torch.uint8), e.view(torch.uint8)), f"output {k} of the replay differs from the eager call"
    ref, terms = G.gemm_reference(*(G.operand_of_activation(c["x"], fa, "mx")[0], G.operand_of_parameter(c["W"], c["sw"], fb, 0)), c["bias"])
    assert_within_terms(_np(Y), ref, terms, "captured mx_gemm")


def test_gemm_out_with_a_row_stride(dev):
    """out= a view of a wider matrix: its row stride is the leading dimension, the spare columns keep their contents."""
    M, N, K = 19, 21, 160
    c = _exact((M, N, K), False)
    a = ops.mx_operand_pack(_t(c["A"], dev), _t(c["sa"], dev), "fp8_e4m3")
    b = ops.mx_operand_pack(_t(c["W"], dev), _t(c["sw"], dev), "fp4_e2m1")
    bias = _t(c["bias"], dev)
    want = ops.mx_gemm(a, b, bias)
    buf = torch.full((M, N + 3), -7.0, device=dev)
    out = buf[:, :N]
    assert out.stride() == (N + 3, 1)
    got = ops.mx_gemm(a, b, bias, out=out)
    assert got is out
    assert torch.equal(buf[:, :N].contiguous().view(torch.int32), want.view(torch.int32)) and (buf[:, N:] == -7.0).all()
    ref, _ = G.gemm_reference(*G.exact_operands(c, "fp8_e4m3", "fp4_e2m1"), c["bias"])
    assert np.array_equal(_np(want).astype(np.float64), ref)
    for bad in (torch.empty((M, N + 1), device=dev), torch.empty((M + 1, N), device=dev), torch.empty((N, M), device=dev),
                torch.empty((M, N), dtype=torch.float64, device=dev), torch.empty((M, N), dtype=torch.int32, device=dev),
                torch.empty((N, M), device=dev).t(), torch.empty((M, 2 * N), device=dev)[:, ::2]):
        with pytest.raises(ValueError, match="out must be a float32 device matrix"):
            ops.mx_gemm(a, b, bias, out=bad)
    assert (buf[:, N:] == -7.0).all()


# ----------------------------------------------------------------------------------------------------------------- 7 layers
def _layer_reference(layer, x, act_format, act_scale):
    """(Y, sum|terms|) in float64: quantize -> decode -> matmul with the fake-quantised weight, plus the fake-quantised bias."""
    with torch.no_grad():
        A = _np(ops.mx_operand_decode(ops.mx_operand_quantize(x.reshape(-1, x.shape[-1]), act_format, act_scale))).astype(np.float64)
        qw, qb = _np(layer.nested_q_w_layer(layer.W)).astype(np.float64), _np(layer.nested_q_b_layer(layer.b)).astype(np.float64)
    return A @ qw + qb[None, :], np.abs(A) @ np.abs(qw) + np.abs(qb)[None, :]


def test_dense_layer_call_mx(dev):
    layer = lq.CustomDenseLayer(units=40, orientation="groupwise", element_format="fp4_e2m1", initializer=lq.RandomNormal(seed=5),
                                input_shape=70, device=dev)
    layer.init_scales("cover")
    op = layer.mx_operand()
    assert (op.lines, op.K, op.format) == (40, 70, "fp4_e2m1")
    with torch.no_grad():
        qw = layer.nested_q_w_layer(layer.W)
    assert bits_equal(_np(ops.mx_operand_decode(op)), _np(qw).T), "the operand is not the fake-quantised kernel"
    x = torch.randn(37, 70, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for act_format, act_scale in (("fp8_e4m3", "mx"), ("fp4_e2m1", "cover")):
        y = layer.call_mx(x, act_format, act_scale)
        assert y.shape == (37, 40) and not y.requires_grad
        ref, terms = _layer_reference(layer, x, act_format, act_scale)
        assert_within_terms(_np(y), ref, terms, f"call_mx {act_format} {act_scale}")
    y3 = layer.call_mx(x.reshape(1, 37, 70))
    assert y3.shape == (1, 37, 40) and torch.equal(y3[0], layer.call_mx(x))
    # mx_hardware(emulate=True), the stock-arithmetic yardstick of train.py --mx-eval: the same operations through torch.matmul
    layer.eval()
    with L.mx_hardware(layer, "fp8_e4m3", "mx", emulate=True) as hw, torch.no_grad():
        assert hw.layers == [layer]
        fake = layer(x)
        want = torch.add(torch.matmul(ops.mx_operand_decode(ops.mx_operand_quantize(x, "fp8_e4m3", "mx")), qw), layer.nested_q_b_layer(layer.b))
    assert torch.equal(fake.view(torch.int32), want.view(torch.int32))
    ref, terms = _layer_reference(layer, x, "fp8_e4m3", "mx")
    assert_within_terms(_np(fake), ref, terms, "mx_hardware(emulate=True)")


def test_mx_hardware_on_the_mnist_model(dev):
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="cover")
    x = torch.rand(37, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    model.eval()
    with torch.no_grad():
        before = model(x)
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, i, o, k=k: seen.__setitem__(k, (i[0].detach(), o.detach())))
             for k, m in (("dense_1", model.dense_1), ("dense_2", model.dense_2))]
    with L.mx_hardware(model, act_format="fp8_e4m3", act_scale="mx") as hw:
        assert hw.layers == [model.dense_1, model.dense_2]
        with torch.no_grad():
            inside = model(x)
        for k, m in (("dense_1", model.dense_1), ("dense_2", model.dense_2)):      # per layer, from the input the layer saw
            xin, out = seen[k]
            ref, terms = _layer_reference(m, xin, "fp8_e4m3", "mx")
            assert_within_terms(_np(out), ref, terms, f"mx_hardware {k}")
        model.train()                                       # training-mode calls keep the fake-quantised path
        assert torch.equal(model(x).detach().view(torch.int32), before.view(torch.int32))
        model.eval()
    for h in hooks:
        h.remove()
    assert model.dense_1._mx_hw is None and model.dense_2._mx_hw is None
    assert not torch.equal(inside, before), "the hardware path quantises the activations: it cannot equal the fake-quantised forward"
    with torch.no_grad():
        assert torch.equal(model(x).view(torch.int32), before.view(torch.int32)), "forward outside the context changed"
