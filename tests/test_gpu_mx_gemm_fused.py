"""GPU tests of the operand-out epilogue of the block-scaled GEMM (csrc/lq_mx_gemm.hpp: k_mx_gemm_quantize; include/lq_hip.h:
lq_mx_gemm_quantize) and of what is built on it: ops.mx_gemm_quantize, CustomDenseLayer.call_mx(out_format=...),
layers.mx_dense_chain, layers.mx_hardware(fused=True), train.mx_eval(fused=True).

The bar, everywhere: ``codes`` and ``scales`` equal BYTE FOR BYTE, whole buffers and so padding included, what the composition
ops.mx_gemm -> activation in torch -> ops.mx_operand_quantize writes on the same device.  There is no tolerance: lq_mx_gemm is
run-to-run bit-stable, the fused kernel's K loop issues the same instructions on the same fragments in the same order, and the scale
rule and the element step are the quantizer's own functions.  relu is v > 0 ? v : (v != v ? v : +0), as the header defines it.

Shapes (M, N, K), the smallest at which each mechanism can go wrong:  (81, 70, 160): MT = 6, NT = 5 -- a clamped second tile on both
axes and waves that leave; lines 81 .. 95 are non-zero once the bias is added and must still be code 0 under byte 127; columns
70 .. 95 are masked inside live blocks and block 3 of K' step 0 lies wholly past N.  It runs all nine input pairs x three output formats
x two methods x {none, relu}, with and without a bias, so every one of the 18 instantiations is launched.  (17, 33, 160): a block with
ONE live column.  (16, 129, 160): KT' = 2 -- block 4 has one live element, blocks 5 .. 7 are padding written by waves that run no K
loop.  (19, 513, 128): KT' = 5, KG' = 2 -- the scale bytes of the idle K steps 5 .. 7.  (129, 17, 160): three blocks along m.
(1, 1, 32): the smallest case."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _mx_gemm_reference as G                                                                # noqa: E402
import _mx_reference as X                                                                     # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(G.OPERAND_FORMATS)
METHODS = ("mx", "cover")
BIG, SMALL = G.FUSED_BIG, G.FUSED_SMALL
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def relu(v):
    return torch.where(v > 0, v, torch.where(v != v, v, torch.zeros_like(v)))


_CASES = {}


def _case(dev, shape, aname, bname):
    """(a, b, bias) on the device, built once per (shape, pair): Gaussian X through mx_operand_quantize, Gaussian W under ``cover``
    scales through mx_operand_pack, a Gaussian bias."""
    key = (shape, aname, bname)
    if key not in _CASES:
        c = G.random_case(*shape, aname, bname)
        _CASES[key] = (ops.mx_operand_quantize(_t(c["x"], dev), aname, "mx"), ops.mx_operand_pack(_t(c["W"], dev), _t(c["sw"], dev), bname),
                       _t(c["bias"], dev))
    return _CASES[key]


def _composition(a, b, bias, activation, out_format, method):
    y = ops.mx_gemm(a, b, bias)
    return ops.mx_operand_quantize(relu(y) if activation == "relu" else y, out_format, method)


def _assert_same(got, want, what):
    assert (got.format, got.lines, got.K) == (want.format, want.lines, want.K), what
    assert got.codes.shape == want.codes.shape and got.scales.shape == want.scales.shape, what
    if torch.equal(got.codes, want.codes) and torch.equal(got.scales, want.scales):
        return
    bad = G.layout_mismatch(_np(got.codes), _np(got.scales),
                            G.RefOperand(*G.unpack_layout(_np(want.codes), _np(want.scales), want.format, want.lines, want.K), want.format, None))
    raise AssertionError(f"{what}: the fused buffers differ from the composition's: {bad}")


def _replant(op, dev, edit):
    """``op`` with its logical (codes, bytes) changed in place by ``edit``, packed again in the documented layout."""
    codes, bytes_ = G.unpack_layout(_np(op.codes), _np(op.scales), op.format, op.lines, op.K)
    edit(codes, bytes_)
    cbuf, sbuf = G.pack_layout(codes, bytes_, op.format)
    return ops.MxOperand(_t(cbuf, dev), _t(sbuf, dev), op.format, op.lines, op.K)


def _logical(op):
    return G.unpack_layout(_np(op.codes), _np(op.scales), op.format, op.lines, op.K)


# ------------------------------------------------------------------------------------------ 1 the fused call against the composition
@pytest.mark.parametrize("out_format", NAMES)
@pytest.mark.parametrize("pair", G.PAIRS, ids=lambda p: "-".join(p))
def test_every_instantiation_equals_the_composition(dev, pair, out_format):
    a, b, bias = _case(dev, BIG, *pair)
    for method in METHODS:
        for activation in (None, "relu"):
            for bv in (bias, None):
                got = ops.mx_gemm_quantize(a, b, bv, activation, out_format, method)
                what = f"{pair} -> {out_format} {method} {activation} bias={bv is not None}"
                _assert_same(got, _composition(a, b, bv, activation, out_format, method), what)
    assert (got.lines, got.K) == (81, 70) and (got.codes.numel(), got.scales.numel()) == ops.mx_operand_bytes(out_format, 81, 70)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("out_format", ["fp8_e4m3", "fp4_e2m1"])
@pytest.mark.parametrize("shape", SMALL, ids=_ids)
def test_edge_shapes_equal_the_composition(dev, shape, out_format, method):
    a, b, bias = _case(dev, shape, "fp8_e4m3", "fp4_e2m1")
    got = ops.mx_gemm_quantize(a, b, bias, "relu", out_format, method)
    _assert_same(got, _composition(a, b, bias, "relu", out_format, method), f"{shape} -> {out_format} {method}")
    M, N, _ = shape
    assert (got.codes.numel(), got.scales.numel()) == ops.mx_operand_bytes(out_format, M, N)


# ------------------------------------------------------------------------------------------------------------ 2 planted cases
@pytest.mark.parametrize("out_format", ["fp8_e4m3", "fp4_e2m1"])
def test_a_zero_row_of_A_gives_zero_blocks_under_byte_1(dev, out_format):
    a, b, _ = _case(dev, BIG, "fp8_e4m3", "fp4_e2m1")

    def edit(codes, bytes_):
        codes[3, :] = 0
    a0 = _replant(a, dev, edit)
    for activation in (None, "relu"):
        got = ops.mx_gemm_quantize(a0, b, None, activation, out_format, "mx")
        _assert_same(got, _composition(a0, b, None, activation, out_format, "mx"), f"zero row {activation}")
        codes, bytes_ = _logical(got)
        assert (codes[3] == 0).all() and (bytes_[3] == 1).all(), "a block of zeros takes min_value = 2^-126: byte 1"
        if activation is None:                             # relu may empty the six live columns of another row's last block
            assert (bytes_[np.arange(81) != 3] > 1).all()


@pytest.mark.parametrize("out_format", ["fp8_e4m3", "fp4_e2m1"])
def test_a_block_that_relu_empties(dev, out_format):
    a, b, bias = _case(dev, BIG, "fp8_e4m3", "fp4_e2m1")
    low = bias.clone()
    low[32:64] = -1e30
    got = ops.mx_gemm_quantize(a, b, low, "relu", out_format, "cover")
    _assert_same(got, _composition(a, b, low, "relu", out_format, "cover"), "relu over a bias of -1e30")
    codes, bytes_ = _logical(got)
    assert (codes[:, 32:64] == 0).all() and (bytes_[:, 1] == 1).all() and (bytes_[:, 0] > 1).all()


@pytest.mark.parametrize("out_format", ["fp8_e5m2", "fp4_e2m1"])
def test_an_inf_code_in_A_marks_its_row_only(dev, out_format):
    a, b, bias = _case(dev, BIG, "fp8_e5m2", "fp4_e2m1")

    def edit(codes, bytes_):
        codes[5, 10] = 0x7C                                # +Inf of fp8_e5m2
    ai = _replant(a, dev, edit)
    for activation in (None, "relu"):
        got = ops.mx_gemm_quantize(ai, b, bias, activation, out_format, "mx")
        _assert_same(got, _composition(ai, b, bias, activation, out_format, "mx"), f"Inf in A {activation}")
        _, bytes_ = _logical(got)
        # relu turns -Inf into +0: the six live columns of the last block may all be that, the 32 of the others are not
        assert (bytes_[5, :2] == 255).all() and (activation == "relu" or bytes_[5, 2] == 255)
        assert (bytes_[np.arange(81) != 5] != 255).all()


@pytest.mark.parametrize("out_format", ["fp8_e4m3", "fp4_e2m1"])
def test_a_nan_line_of_B_marks_one_block_per_row_and_relu_keeps_it(dev, out_format):
    a, b, bias = _case(dev, BIG, "fp8_e4m3", "fp4_e2m1")

    def edit(codes, bytes_):
        bytes_[40, :] = 255                                # line 40 of B under a NaN scale: column 40 of Y is NaN
    bn = _replant(b, dev, edit)
    for activation in (None, "relu"):
        got = ops.mx_gemm_quantize(a, bn, bias, activation, out_format, "mx")
        _assert_same(got, _composition(a, bn, bias, activation, out_format, "mx"), f"NaN line of B {activation}")
        _, bytes_ = _logical(got)
        assert (bytes_[:, 1] == 255).all() and (bytes_[:, [0, 2]] != 255).all(), f"{activation}: block 1 of every row is NaN"


# ------------------------------------------------------------------------------------------------------------ 3 memory contract
@pytest.mark.parametrize("out_format", ["fp8_e4m3", "fp4_e2m1"])
@pytest.mark.parametrize("shape", [BIG, (19, 513, 128)], ids=_ids)
def test_memory_contract(dev, shape, out_format):
    """The output buffers carved out of one allocation with 4 KiB guards: the guards keep their preset, and the buffers do not
    depend on theirs (0xA5, 0x00, 0xFF) -- every byte of them is written."""
    M, N, K = shape
    a, b, bias = _case(dev, shape, "fp8_e4m3", "fp4_e2m1")
    cb, sb = ops.mx_operand_bytes(out_format, M, N)
    guard = 4096
    c0, s0 = guard, 2 * guard + cb                         # cb is a multiple of 16: both starts stay on the 16-byte grid
    total = s0 + sb + guard
    lib = _hip.load()
    want = _composition(a, b, bias, "relu", out_format, "mx")
    for preset in (0xA5, 0x00, 0xFF):
        buf = torch.full((total,), preset, dtype=torch.uint8, device=dev)
        codes, scales = buf[c0:c0 + cb], buf[s0:s0 + sb]
        _hip.check(lib.lq_mx_gemm_quantize(_hip.ptr(a.codes), _hip.ptr(a.scales), X.FORMATS["fp8_e4m3"].id, _hip.ptr(b.codes),
                                           _hip.ptr(b.scales), X.FORMATS["fp4_e2m1"].id, _hip.ptr(bias), 1, X.FORMATS[out_format].id, 0,
                                           _hip.ptr(codes), _hip.ptr(scales), M, N, K, _hip.stream_ptr(dev)), "lq_mx_gemm_quantize")
        torch.cuda.synchronize(dev)
        for lo, hi in ((0, c0), (c0 + cb, s0), (s0 + sb, total)):
            assert (buf[lo:hi] == preset).all(), f"guard [{lo}, {hi}) was written (preset {preset:#x})"
        assert torch.equal(codes, want.codes) and torch.equal(scales, want.scales), f"preset {preset:#x}"


# --------------------------------------------------------------------------------------------------------------------- 4 capture
def test_capture_and_replay(dev):
    """quantize -> gemm_quantize -> gemm, one launch each, captured in one graph and replayed twice into poisoned buffers."""
    M, H, N, K = 19, 40, 10, 70
    fa, fw = "fp8_e4m3", "fp4_e2m1"
    c1, c2 = G.random_case(M, H, K, fa, fw), G.random_case(M, N, H, fa, fw)
    x, b1, b2 = _t(c1["x"], dev), _t(c1["bias"], dev), _t(c2["bias"], dev)
    w1, w2 = ops.mx_operand_pack(_t(c1["W"], dev), _t(c1["sw"], dev), fw), ops.mx_operand_pack(_t(c2["W"], dev), _t(c2["sw"], dev), fw)
    ea = ops.mx_operand_quantize(x, fa, "mx")
    eh = ops.mx_gemm_quantize(ea, w1, b1, "relu", fa, "mx")
    eager = [ea.codes, ea.scales, eh.codes, eh.scales, ops.mx_gemm(eh, w2, b2)]
    assert torch.equal(eager[4].view(torch.int32),
                       ops.mx_gemm(ops.mx_operand_quantize(relu(ops.mx_gemm(ea, w1, b1)), fa, "mx"), w2, b2).view(torch.int32))
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)      # noqa: E731
    ac, as_, hc, hs = (u8(n) for n in ops.mx_operand_bytes(fa, M, K) + ops.mx_operand_bytes(fa, M, H))
    Y = torch.empty((M, N), device=dev)
    outs = [ac, as_, hc, hs, Y]
    lib = _hip.load()
    ida, idw = X.FORMATS[fa].id, X.FORMATS[fw].id

    def launch():
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_mx_operand_quantize(_hip.ptr(x), ida, 0, M, K, _hip.ptr(ac), _hip.ptr(as_), st), "quantize")
        _hip.check(lib.lq_mx_gemm_quantize(_hip.ptr(ac), _hip.ptr(as_), ida, _hip.ptr(w1.codes), _hip.ptr(w1.scales), idw, _hip.ptr(b1), 1,
                                           ida, 0, _hip.ptr(hc), _hip.ptr(hs), M, H, K, st), "gemm_quantize")
        _hip.check(lib.lq_mx_gemm(_hip.ptr(hc), _hip.ptr(hs), ida, _hip.ptr(w2.codes), _hip.ptr(w2.scales), idw, _hip.ptr(b2), _hip.ptr(Y),
                                  M, N, H, N, st), "gemm")

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


# ---------------------------------------------------------------------------------------------------------- 5 layers and models
def _dense(dev, n_in, units, seed):
    layer = lq.CustomDenseLayer(units=units, orientation="groupwise", element_format="fp4_e2m1", initializer=lq.RandomNormal(seed=seed),
                                input_shape=n_in, device=dev)
    layer.init_scales("cover")
    return layer


def test_dense_chain_equals_the_layers_one_by_one(dev):
    d1, d2 = _dense(dev, 70, 40, 5), _dense(dev, 40, 10, 6)
    x = torch.randn(37, 70, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for act_scale in METHODS:
        want = d2.call_mx(F.relu(d1.call_mx(x, "fp8_e4m3", act_scale)), "fp8_e4m3", act_scale)
        got = L.mx_dense_chain(x, [(d1, "relu"), (d2, None)], "fp8_e4m3", act_scale)
        assert got.shape == (37, 10) and not got.requires_grad
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), act_scale
        # the same through call_mx: an operand out of the first layer, an operand into the second
        h = d1.call_mx(x, "fp8_e4m3", act_scale, out_format="fp8_e4m3", activation="relu")
        assert isinstance(h, ops.MxOperand) and (h.lines, h.K, h.format) == (37, 40, "fp8_e4m3")
        assert torch.equal(d2.call_mx(h, "fp8_e4m3", act_scale).view(torch.int32), want.view(torch.int32))
    y3 = L.mx_dense_chain(x.reshape(1, 37, 70), [(d1, "relu"), (d2, None)])
    assert y3.shape == (1, 37, 10) and torch.equal(y3[0], L.mx_dense_chain(x, [(d1, "relu"), (d2, None)]))
    # no activation between the layers
    want = d2.call_mx(d1.call_mx(x))
    assert torch.equal(L.mx_dense_chain(x, [(d1, None), (d2, None)]).view(torch.int32), want.view(torch.int32))


def test_mx_hardware_fused_on_the_mnist_model(dev):
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="cover")
    x = torch.rand(5, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    model.eval()
    with torch.no_grad():
        before = model(x)
        with L.mx_hardware(model) as hw:
            assert hw.fused_layers == []
            unfused = model(x)
        calls = []
        hooks = [m.register_forward_hook(lambda mod, i, o: calls.append(mod)) for m in (model.dense_1, model.dense_2)]
        with L.mx_hardware(model, fused=True) as hw:
            assert hw.layers == [model.dense_1, model.dense_2] and hw.fused_layers == [model.dense_1, model.dense_2]
            fused = model(x)
            assert calls == [], "the fused tail goes through mx_dense_chain, not through the layers' calls"
            model.train()                                   # training-mode calls keep the fake-quantised path
            assert torch.equal(model(x).detach().view(torch.int32), before.view(torch.int32))
            model.eval()
        for h in hooks:
            h.remove()
        assert model._mx_fused is None and model.dense_1._mx_hw is None
        assert torch.equal(fused.view(torch.int32), unfused.view(torch.int32))
        assert not torch.equal(fused, before)
        assert torch.equal(model(x).view(torch.int32), before.view(torch.int32)), "forward outside the context changed"


def test_mx_hardware_fused_leaves_the_cifar_model_alone(dev):
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="cover")
    x = torch.rand(2, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    model.eval()
    with torch.no_grad():
        before = model(x)
        with L.mx_hardware(model, fused=True) as hw:
            assert hw.fused_layers == []
            inside = model(x)
    assert torch.equal(inside.view(torch.int32), before.view(torch.int32))


def test_mx_eval_fused_reports_no_difference(dev):
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="cover")
    x = torch.rand(16, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    y = torch.arange(16, device=dev) % 10
    plain = train.mx_eval(model, x, y)
    assert not any(k.startswith("mx_eval_fused") for k in plain)
    out = train.mx_eval(model, x, y, fused=True)
    assert out["mx_eval_fused_layers"] == 2 and out["mx_eval_fused_max_logit_diff"] == 0.0
    assert out["mx_eval_fused_accuracy"] == out["mx_eval_accuracy"]
    assert {k: v for k, v in out.items() if not k.startswith("mx_eval_fused")} == plain
