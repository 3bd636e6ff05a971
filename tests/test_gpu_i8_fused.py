"""GPU tests of the operand-out epilogue of the int8 GEMM (csrc/lq_i8_gemm_quant.hpp: k_i8_gemm_quantize; include/lq_hip.h:
lq_i8_gemm_quantize) and of what is built on it: ops.i8_gemm_quantize, CustomDenseLayer.call_i8(out_block=64),
layers.i8_dense_chain, layers.i8_hardware(fused=True), train.i8_eval(fused=True).

The bar, everywhere: ``codes`` and ``scales`` equal BYTE FOR BYTE, whole buffers and so padding included, the NumPy reference
(tests/_i8_fused_reference.py: the composition of tests/_i8_reference.py's functions) and what the composition ops.i8_gemm ->
activation in torch -> ops.i8_operand_quantize(block=64) writes on the same device.  There is no tolerance: lq_i8_gemm's Y has a
bit-exact definition that does not depend on a tiling, and the scale rule and the element step are the quantizer's own functions.
The cases and what each reaches are stated beside the table in tests/_i8_fused_reference.py; tests/test_i8_fused_cpu.py asserts on
the reference that they exercise the codes and that the planted ones give the pattern claimed."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_fused_reference as FR                                                             # noqa: E402
import _i8_reference as R                                                                     # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402

pytestmark = pytest.mark.gpu
_ids = lambda k: "x".join(map(str, k)) if isinstance(k, tuple) else str(k)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _upload(op, dev):
    """A reference operand as the device's, through the NumPy packer."""
    cbuf, sbuf = R.pack_layout(op)
    return ops.I8Operand(_t(cbuf, dev), _t(sbuf, dev), op["codes"].shape[0], op["codes"].shape[1], op["block"])


def relu(v):
    return torch.where(v > 0, v, torch.where(v != v, v, torch.zeros_like(v)))


def _composition(a, b, bias, activation):
    y = ops.i8_gemm(a, b, bias)
    return ops.i8_operand_quantize(relu(y) if activation == "relu" else y, 64)


def _assert_same(got, want, ref, what):
    """``got`` against the composition on the device (bytes) and against the reference operand (bytes, a NaN scale equal to a NaN)."""
    assert (got.lines, got.K, got.block) == (want.lines, want.K, 64), what
    assert got.codes.shape == want.codes.shape and got.scales.shape == want.scales.shape, what
    bad = R.buffers_mismatch(_np(got.codes), _np(got.scales), ref)
    assert bad is None, f"{what}: the fused buffers differ from the reference: {bad}"
    assert torch.equal(got.codes, want.codes), f"{what}: codes differ from the composition's"
    assert torch.equal(got.scales.view(torch.int32), want.scales.view(torch.int32)), f"{what}: scales differ from the composition's"


_CASES = {}


def _case(dev, key):
    """(reference a, b, bias; device a, b, bias), built once per case."""
    if key not in _CASES:
        a, b, bias = FR.case(key)
        _CASES[key] = (a, b, bias, _upload(a, dev), _upload(b, dev), _t(bias, dev))
    return _CASES[key]


# ------------------------------------------------------------------------------------------ 1 the fused call against both yardsticks
@pytest.mark.parametrize("key", FR.CASES, ids=_ids)
def test_whole_buffers_equal_the_reference_and_the_composition(dev, key):
    a, b, bias, da, db, dbias = _case(dev, key)
    M, N = key[:2]
    for activation in FR.ACTIVATIONS:
        for rb, bv in ((bias, dbias), (None, None)):
            got = ops.i8_gemm_quantize(da, db, bv, activation)
            what = f"{key} {activation} bias={bv is not None}"
            _assert_same(got, _composition(da, db, bv, activation), FR.reference(a, b, rb, activation), what)
            assert (got.codes.numel(), got.scales.numel() * 4) == ops.i8_operand_bytes(M, N, 64)
            again = ops.i8_gemm_quantize(da, db, bv, activation)
            assert torch.equal(again.codes, got.codes) and torch.equal(again.scales.view(torch.int32), got.scales.view(torch.int32)), what


# ------------------------------------------------------------------------------------------------------------ 2 planted cases
@pytest.mark.parametrize("name", FR.PLANTED)
def test_planted_cases(dev, name):
    a, b, bias, activation, want = FR.planted(name)
    da, db, dbias = _upload(a, dev), _upload(b, dev), (None if bias is None else _t(bias, dev))
    got = ops.i8_gemm_quantize(da, db, dbias, activation)
    _assert_same(got, _composition(da, db, dbias, activation), FR.reference(a, b, bias, activation), name)
    M, N = FR.PLANT_SHAPE[:2]
    logical = R.unpack_layout(_np(got.codes), _np(got.scales), M, N, 64)
    assert np.array_equal(FR.scale_pattern(logical["scales"]), want), f"{name}: the scale pattern"
    nan_pairs = np.repeat(want == 2, 64, axis=1)[:, :N]
    assert (logical["codes"][nan_pairs] == 0).all() and (logical["codes"][np.repeat(want == 1, 64, axis=1)[:, :N]] == 0).all()


# ------------------------------------------------------------------------------------------------------------ 3 memory contract
@pytest.mark.parametrize("key", [(70, 130, 200, 64, 128), (17, 65, 65, 0, 0), (1, 1, 1, 0, 0)], ids=_ids)
def test_memory_contract(dev, key):
    """The output buffers carved out of one allocation with 4 KiB guards: the guards keep their preset, and the buffers do not
    depend on theirs (0xA5, 0x00, 0xFF) -- every byte of them, the padding included, is written."""
    M, N, K, a_block, b_block = key
    a, b, bias, da, db, dbias = _case(dev, key)
    cb, sb = ops.i8_operand_bytes(M, N, 64)
    guard = 4096
    c0, s0 = guard, 2 * guard + cb                         # cb is a multiple of 1024: both starts stay on the 16-byte grid
    total = s0 + sb + guard
    lib = _hip.load()
    rc, rs = FR.reference_buffers(a, b, bias, "relu")
    for preset in (0xA5, 0x00, 0xFF):
        buf = torch.full((total,), preset, dtype=torch.uint8, device=dev)
        codes, scales = buf[c0:c0 + cb], buf[s0:s0 + sb]
        _hip.check(lib.lq_i8_gemm_quantize(_hip.ptr(da.codes), _hip.ptr(da.scales), a_block, _hip.ptr(db.codes), _hip.ptr(db.scales),
                                           b_block, _hip.ptr(dbias), 1, 64, _hip.ptr(codes), _hip.ptr(scales), M, N, K,
                                           _hip.stream_ptr(dev)), "lq_i8_gemm_quantize")
        torch.cuda.synchronize(dev)
        for lo, hi in ((0, c0), (c0 + cb, s0), (s0 + sb, total)):
            assert (buf[lo:hi] == preset).all(), f"guard [{lo}, {hi}) was written (preset {preset:#x})"
        assert np.array_equal(_np(codes), rc) and np.array_equal(_np(scales).view(np.uint32), rs.view(np.uint32)), f"preset {preset:#x}"


# --------------------------------------------------------------------------------------------------------------------- 4 capture
def test_capture_and_replay(dev):
    """quantize -> gemm_quantize -> gemm, one launch each, captured in one graph and replayed twice into poisoned buffers."""
    M, H, N, K = 19, 70, 10, 200
    rng = np.random.default_rng(11)
    w1, w2 = _upload(R.random_operand(rng, H, K, 64), dev), _upload(R.random_operand(rng, N, H, 0), dev)
    x, b1, b2 = _t(rng.normal(0, 1, (M, K)).astype(np.float32), dev), _t(rng.normal(0, 50, H).astype(np.float32), dev), \
        _t(rng.normal(0, 50, N).astype(np.float32), dev)
    ea = ops.i8_operand_quantize(x, 64)
    eh = ops.i8_gemm_quantize(ea, w1, b1, "relu")
    eager = [ea.codes, ea.scales, eh.codes, eh.scales, ops.i8_gemm(eh, w2, b2)]
    assert torch.equal(eager[4].view(torch.int32),
                       ops.i8_gemm(ops.i8_operand_quantize(relu(ops.i8_gemm(ea, w1, b1)), 64), w2, b2).view(torch.int32))
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)      # noqa: E731
    ac, as_, hc, hs = (u8(n) for n in ops.i8_operand_bytes(M, K, 64) + ops.i8_operand_bytes(M, H, 64))
    Y = torch.empty((M, N), device=dev)
    outs = [ac, as_, hc, hs, Y]
    lib = _hip.load()

    def launch():
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_i8_operand_quantize(_hip.ptr(x), M, K, 64, _hip.ptr(ac), _hip.ptr(as_), st), "quantize")
        _hip.check(lib.lq_i8_gemm_quantize(_hip.ptr(ac), _hip.ptr(as_), 64, _hip.ptr(w1.codes), _hip.ptr(w1.scales), 64, _hip.ptr(b1), 1, 64,
                                           _hip.ptr(hc), _hip.ptr(hs), M, H, K, st), "gemm_quantize")
        _hip.check(lib.lq_i8_gemm(_hip.ptr(hc), _hip.ptr(hs), 64, _hip.ptr(w2.codes), _hip.ptr(w2.scales), 0, _hip.ptr(b2), _hip.ptr(Y), N,
                                  M, N, H, st), "gemm")

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
            assert torch.equal(o.view(torch.uint8).reshape(-1), e.contiguous().view(torch.uint8).reshape(-1)), \
                f"output {k} of the replay differs from the eager call"


# ---------------------------------------------------------------------------------------------------------- 5 layers and models
def _dense(dev, n_in, units, seed, **kw):
    layer = lq.CustomDenseLayer(units=units, scale_gradient="ste", initializer=lq.RandomNormal(seed=seed), input_shape=n_in, device=dev, **kw)
    layer.init_scales("absmax")
    return layer


def test_call_i8_takes_an_operand_as_it_is(dev):
    d1, d2 = _dense(dev, 70, 130, 5, bits=8), _dense(dev, 130, 10, 6, bits=8)
    x = torch.randn(37, 70, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    h = d1.call_i8(x, act_block=0, out_block=64, activation="relu")
    assert isinstance(h, ops.I8Operand) and (h.lines, h.K, h.block) == (37, 130, 64)
    # the decoded-then-requantised path: the fp32 activation, relu in torch, quantised again by the second layer's call
    want = d2.call_i8(F.relu(d1.call_i8(x, act_block=0)), act_block=64)
    got = d2.call_i8(h, act_block=128)                     # act_block is not read
    assert got.shape == (37, 10) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # and the next operand again, without an activation
    h2 = d2.call_i8(h, out_block=64)
    assert torch.equal(h2.codes, ops.i8_operand_quantize(want, 64).codes)


@pytest.mark.parametrize("kw", [dict(bits=8), dict(bits=4, orientation="groupwise", group_size=64)], ids=["8bit-scalar", "4bit-gs64"])
def test_dense_chain_equals_the_layers_one_by_one(dev, kw):
    d1, d2, d3 = _dense(dev, 64, 128, 5, **kw), _dense(dev, 128, 192, 6, **kw), _dense(dev, 192, 10, 7, **kw)
    x = torch.randn(37, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    chain = [(d1, "relu"), (d2, "relu"), (d3, None)]
    for act_block in (64, 0):
        want = d3.call_i8(F.relu(d2.call_i8(F.relu(d1.call_i8(x, act_block)), 64)), 64)
        got = L.i8_dense_chain(x, chain, act_block)
        assert got.shape == (37, 10) and not got.requires_grad
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), act_block
    y3 = L.i8_dense_chain(x.reshape(1, 37, 64), chain)
    assert y3.shape == (1, 37, 10) and torch.equal(y3[0], L.i8_dense_chain(x, chain))
    # no activation between the layers
    want = d3.call_i8(d2.call_i8(d1.call_i8(x, 64), 64), 64)
    assert torch.equal(L.i8_dense_chain(x, [(d1, None), (d2, None), (d3, None)]).view(torch.int32), want.view(torch.int32))


def test_i8_hardware_fused_on_the_mnist_model(dev):
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", bits=8, orientation="scalar")
    x = torch.rand(37, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    model.eval()
    with torch.no_grad():
        before = model(x)
        with L.i8_hardware(model, act_block=64) as hw:
            assert hw.fused_layers == []
            unfused = model(x)
        calls = []
        hooks = [m.register_forward_hook(lambda mod, i, o: calls.append(mod)) for m in (model.dense_1, model.dense_2)]
        with L.i8_hardware(model, act_block=64, fused=True) as hw:
            assert hw.layers == [model.dense_1, model.dense_2] and hw.fused_layers == [model.dense_1, model.dense_2]
            fused = model(x)
            assert calls == [], "the fused tail goes through i8_dense_chain, not through the layers' calls"
            model.train()                                   # training-mode calls keep the fake-quantised path
            assert torch.equal(model(x).detach().view(torch.int32), before.view(torch.int32))
            model.eval()
        for h in hooks:
            h.remove()
        assert model._i8_fused is None and model.dense_1._i8_hw is None
        assert torch.equal(fused.view(torch.int32), unfused.view(torch.int32))
        assert not torch.equal(fused, before)
        assert torch.equal(model(x).view(torch.int32), before.view(torch.int32)), "forward outside the context changed"


def test_i8_eval_fused_reports_no_difference(dev):
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", bits=8, orientation="scalar")
    x = torch.rand(16, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    y = torch.arange(16, device=dev) % 10
    plain = train.i8_eval(model, x, y, act_block=64)
    assert not any(k.startswith("i8_eval_fused") for k in plain)
    out = train.i8_eval(model, x, y, act_block=64, fused=True)
    assert out["i8_eval_fused_layers"] == 2 and out["i8_eval_fused_max_logit_diff"] == 0.0
    assert out["i8_eval_fused_accuracy"] == out["i8_eval_accuracy"]
    assert {k: v for k, v in out.items() if not k.startswith("i8_eval_fused")} == plain
