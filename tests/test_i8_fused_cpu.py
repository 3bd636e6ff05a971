"""CPU tests of the operand-out epilogue of the int8 GEMM (include/lq_hip.h: lq_i8_gemm_quantize): the entry point is declared,
exported and bound; every refusal through the C surface with its message (the pointers are never dereferenced: each call fails in
validation, before any launch); the refusals of ops.i8_gemm_quantize, CustomDenseLayer.call_i8, layers.i8_dense_chain,
layers.i8_hardware(fused=True) and the driver; and the data conditions of the inputs tests/test_gpu_i8_fused.py runs, asserted on
the reference alone (tests/_i8_fused_reference.py).  What the kernel writes is that file's."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_fused_reference as FR                                                             # noqa: E402
import _i8_reference as R                                                                     # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402
from learned_quantization_amd.models import build_model                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ_EINVAL, LQ_EALIGN = -1, -4


def _err():
    return _hip.load().lq_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                          # an addition only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    assert "lq_i8_gemm_quantize" in declared and hasattr(lib, "lq_i8_gemm_quantize") and "lq_i8_gemm_quantize" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["lq_i8_gemm_quantize"][1]) == 15
    not_built = header[header.index("Not built: epilogue output blocks"):]
    assert "an operand-out epilogue" not in not_built[:not_built.index("*/")]
    assert lq.i8_gemm_quantize is ops.i8_gemm_quantize and lq.i8_dense_chain is L.i8_dense_chain
    assert ops.I8_ACTIVATIONS == (None, "relu") and ops.check_activation("relu") == 1 and ops.check_mx_activation(None) == 0
    assert L._I8.operand_type is ops.I8Operand and L._MX.operand_type is ops.MxOperand


def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    fused = lib.lq_i8_gemm_quantize

    def call(**kw):
        a = dict(ac=p, as_=p, ab=0, bc=p, bs=p, bb=0, bias=None, act=1, ob=64, oc=p, os_=p, M=16, N=16, K=128)
        a.update(kw)
        return fused(a["ac"], a["as_"], a["ab"], a["bc"], a["bs"], a["bb"], a["bias"], a["act"], a["ob"], a["oc"], a["os_"], a["M"], a["N"],
                     a["K"], None)

    for ob in (0, 128, 32, -64, 192):
        assert call(ob=ob) == LQ_EINVAL and f"out_block = {ob}" in _err() and "scale blocks of 64" in _err(), ob
    for act in (-1, 2):
        assert call(act=act) == LQ_EINVAL and "bad activation" in _err()
    # every pointer but the bias
    for key in ("ac", "as_", "bc", "bs", "oc", "os_"):
        assert call(**{key: None}) == LQ_EINVAL and "NULL" in _err(), key
    # extents, blocks and periods: lq_i8_gemm's
    for key in ("M", "N", "K"):
        for v in (0, -1):
            assert call(**{key: v}) == LQ_EINVAL and "extents must be positive" in _err(), (key, v)
    assert call(M=1 << 20, K=1 << 11) == LQ_EINVAL and "not below 2^31" in _err()          # M * K
    assert call(N=1 << 20, K=1 << 11) == LQ_EINVAL and "not below 2^31" in _err()          # N * K
    assert call(M=1 << 16, N=1 << 15, K=128) == LQ_EINVAL and "not below 2^31" in _err()   # M * N alone
    assert call(M=65535 * 64 + 1, N=16, K=128) == LQ_EINVAL and "is above 65535 * 64" in _err()
    for key in ("ab", "bb"):
        for v in (-64, 32, 100):
            assert call(**{key: v}) == LQ_EINVAL and "neither 0 (one scale per line) nor a multiple of 64" in _err(), (key, v)
    assert call(ab=128, bb=192, K=512) == LQ_EINVAL and "the larger must be a multiple of the smaller" in _err()
    assert call(K=65536 + 64) == LQ_EINVAL and "is above 65536" in _err()
    assert call(ab=1 << 17, K=1 << 18) == LQ_EINVAL and "is above 65536" in _err()
    # alignment
    for key in ("ac", "bc", "oc"):
        assert call(**{key: p + 8}) == LQ_EALIGN and "codes is not 16-byte aligned" in _err(), key
    for key in ("as_", "bs", "os_"):
        assert call(**{key: p + 4}) == LQ_EALIGN and "scales is not 16-byte aligned" in _err(), key
    assert call(bias=p + 1) == LQ_EALIGN and "bias is not 4-byte aligned" in _err()


def _dense(units=4, n_in=70, **kw):
    return L.CustomDenseLayer(units=units, initializer=L.RandomNormal(seed=1), input_shape=n_in, **kw)


def test_refusals_of_the_python_surface():
    u8, f32 = torch.zeros(16, dtype=torch.uint8), torch.zeros(16)
    a, b = ops.I8Operand(u8, f32, 16, 128, 0), ops.I8Operand(u8, f32, 16, 128, 64)
    with pytest.raises(ValueError, match="different K: 128 and 160"):
        ops.i8_gemm_quantize(a, ops.I8Operand(u8, f32, 16, 160, 0))
    for bad in (0, 128, 32, None, 64.0, True):
        with pytest.raises(ValueError, match="writes scale blocks of 64"):
            ops.i8_gemm_quantize(a, b, out_block=bad)
    for bad in ("gelu", "RELU", 1, ""):
        with pytest.raises(ValueError, match="activation must be one of"):
            ops.i8_gemm_quantize(a, b, activation=bad)
    with pytest.raises(ValueError, match="the larger must be a multiple of the smaller"):
        ops.i8_gemm_quantize(ops.I8Operand(u8, f32, 16, 512, 128), ops.I8Operand(u8, f32, 16, 512, 192))
    # layers: an operand as input must reduce over the layer's in; act_block is then not read
    good = _dense(bits=8)
    with pytest.raises(ValueError, match=re.escape("reduces over K = 128, the layer over in = 70")):
        good.call_i8(a, act_block=7)
    with pytest.raises(ValueError, match="block=7"):
        good.call_i8(torch.zeros(3, 70), act_block=7)
    with pytest.raises(ValueError, match="activation must be one of"):
        good.call_i8(torch.zeros(3, 70), out_block=64, activation="tanh")
    with pytest.raises(ValueError, match="writes scale blocks of 64"):
        good.call_i8(torch.zeros(3, 70), out_block=128)
    with pytest.raises(ValueError, match="writes scale blocks of 64"):
        good.call_i8(torch.zeros(3, 70), out_block=0)
    unbuilt = L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), bits=8)
    with pytest.raises(ValueError, match="not built yet"):
        unbuilt.call_i8(a)
    # the chain: ineligible layers and activations, named
    x = torch.zeros(3, 70)
    last = _dense(units=3, n_in=4, bits=8)
    for kw, needle in ((dict(), "needs a layer with bits or q_range"),
                       (dict(bits=8, signed=False), "is not inside [-128, 127]"),
                       (dict(bits=4, orientation="rowwise"), 'orientation="rowwise"'),
                       (dict(bits=4, orientation="groupwise", group_size=16), "group_size=16"),
                       (dict(orientation="groupwise", element_format="fp4_e2m1"), "element_format")):
        bad = _dense(**kw)
        with pytest.raises(ValueError, match=re.escape(needle)) as e:
            L.i8_dense_chain(x, [(bad, "relu"), (last, None)])
        assert bad.name in str(e.value) and str(e.value).startswith("i8_dense_chain: ")
    with pytest.raises(ValueError, match="only Dense layers run on the int8 GEMM"):
        L.i8_dense_chain(x, [(torch.nn.Linear(70, 4), "relu"), (last, None)])
    with pytest.raises(ValueError, match="activation must be one of"):
        L.i8_dense_chain(x, [(good, "sigmoid"), (last, None)])
    with pytest.raises(ValueError, match="the last layer writes fp32"):
        L.i8_dense_chain(x, [(good, "relu"), (last, "relu")])
    with pytest.raises(ValueError, match="the chain is empty"):
        L.i8_dense_chain(x, [])
    with pytest.raises(ValueError, match="block=100"):
        L.i8_dense_chain(x, [(good, "relu"), (last, None)], act_block=100)
    # i8_hardware
    m = build_model("mnist", mode="ste", value=0.0, bits=8)
    with pytest.raises(ValueError, match="emulate=True with fused=True"):
        L.i8_hardware(m, 64, emulate=True, fused=True)
    for act_block in (0, 128):
        with pytest.raises(ValueError, match=re.escape(f"fused=True with act_block={act_block}: the epilogue writes scale blocks of 64, so "
                                                       "the fused model would not be the unfused one")):
            L.i8_hardware(m, act_block, fused=True)
    hw = L.i8_hardware(m, 64, fused=True)
    assert hw.fused and hw.fused_layers == [] and L.i8_hardware(m).fused is False and L.i8_hardware(m, 128).fused is False
    assert [layer for layer, _ in m.i8_chain()] == [m.dense_1, m.dense_2] and [act for _, act in m.i8_chain()] == ["relu", None]
    assert m.mx_chain() == m.i8_chain()


def test_driver_refusals_and_flag(capsys):
    from learned_quantization_amd import train
    base = ["--config", "mnist", "--mode", "ste", "--bits", "8"]
    for argv, needle in ((base + ["--i8-eval-fused"], "--i8-eval-fused needs --i8-eval"),
                         (base + ["--i8-eval", "--i8-eval-fused"], "--i8-eval-fused needs --i8-eval-act-block 64"),
                         (base + ["--i8-eval", "--i8-eval-act-block", "128", "--i8-eval-fused"], "--i8-eval-fused needs --i8-eval-act-block 64")):
        with pytest.raises(SystemExit):
            train.main(argv)
        assert needle in capsys.readouterr().err
    ns = train.build_parser().parse_args(["--i8-eval", "--i8-eval-act-block", "64", "--i8-eval-fused"])
    assert ns.i8_eval and ns.i8_eval_act_block == 64 and ns.i8_eval_fused is True
    assert train.build_parser().parse_args([]).i8_eval_fused is False


# ------------------------------------------------------------------------------------- the data of the GPU tests, on the reference
def test_act_is_the_headers_relu():
    v = np.array([1.5, -2.0, -0.0, 0.0, np.nan, np.inf, -np.inf], np.float32)
    got = FR.act(v, "relu")
    assert np.array_equal(got.view(np.uint32), np.array([1.5, 0.0, 0.0, 0.0, np.nan, np.inf, 0.0], np.float32).view(np.uint32))
    assert FR.act(v, None) is not None and np.array_equal(FR.act(v, None).view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("key", FR.CASES, ids=lambda k: "x".join(map(str, k)))
def test_random_cases_exercise_the_codes(key):
    a, b, bias = FR.case(key)
    M, N = key[:2]
    for activation in FR.ACTIVATIONS:
        for bv in (bias, None):
            op = FR.reference(a, b, bv, activation)
            # the reference calls one block that covers the row block 0: the same buffers
            assert op["codes"].shape == (M, N) and op["scales"].shape == (M, -(-N // 64)) and op["block"] == (64 if N > 64 else 0)
            assert (op["codes"] != 0).any(), (key, activation)
            distinct = len(np.unique(op["codes"]))
            assert distinct >= FR.DEGENERATE.get((key, activation), FR.MIN_DISTINCT), (key, activation, distinct)
            assert not np.isnan(op["scales"]).any()
            cbuf, sbuf = R.pack_layout(op)
            assert (cbuf.size, sbuf.size * 4) == ops.i8_operand_bytes(M, N, 64)
    if key == (1, 1, 1, 0, 0):
        assert R.gemm_reference(a, b)[0, 0] > 0 and R.gemm_reference(a, b, bias)[0, 0] > 0


@pytest.mark.parametrize("name", FR.PLANTED)
def test_planted_cases_give_the_pattern_claimed(name):
    a, b, bias, activation, want = FR.planted(name)
    op = FR.reference(a, b, bias, activation)
    assert np.array_equal(FR.scale_pattern(op["scales"]), want), name
    nan_pairs = np.repeat(want == 2, 64, axis=1)[:, :op["codes"].shape[1]]
    assert (op["codes"][nan_pairs] == 0).all(), "a NaN scale stores code 0"
    counts = {"relu_empties_a_block": (70, 0), "nan_scale_in_a": (None, 3), "nan_scale_in_b": (None, 70), "inf_bias": (None, 70),
              "huge_negative_bias": (0, 0), "zero_row": (None, 0)}[name]
    assert counts[0] is None or (want[:, 1] == 1).sum() == counts[0]
    assert (want == 2).sum() == counts[1]
    if name == "nan_scale_in_a":
        assert (want[5] == 2).all() and not (np.delete(want, 5, 0) == 2).any()
    if name in ("nan_scale_in_b", "relu_empties_a_block"):
        assert (want[:, 1] == (2 if name == "nan_scale_in_b" else 1)).all() and not (want[:, [0, 2]] == 2).any()
    if name == "zero_row":
        assert (want[7] == 1).all() and (op["codes"][7] == 0).all()
    if name == "huge_negative_bias":      # the block's scale follows the one huge value and every other code of the block is 0
        assert np.isfinite(op["scales"][:, 2]).all() and (op["scales"][:, 2] > 1e27).all()
        assert (op["codes"][:, 129] == -127).all() and (op["codes"][:, 128] == 0).all()
