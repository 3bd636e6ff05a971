"""CPU tests of the operand-out epilogue of the block-scaled GEMM (include/lq_hip.h: lq_mx_gemm_quantize): the entry point is
declared, exported and bound; every refusal through the C surface with its message (the pointers are never dereferenced: each call
fails in validation, before any launch); the refusals of ops.mx_gemm_quantize, CustomDenseLayer.call_mx, layers.mx_dense_chain,
layers.mx_hardware(fused=True) and the driver.  What the kernel writes is tests/test_gpu_mx_gemm_fused.py's."""
import ctypes
import os
import re

import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, layers as L, ops
from learned_quantization_amd.models import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ_EINVAL, LQ_EALIGN = -1, -4
FP4, FP6A, FP6B, E4M3, E5M2 = 0, 1, 2, 3, 4


def _err():
    return _hip.load().lq_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                          # an addition only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    assert "lq_mx_gemm_quantize" in declared and hasattr(lib, "lq_mx_gemm_quantize") and "lq_mx_gemm_quantize" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["lq_mx_gemm_quantize"][1]) == 16
    assert re.search(r"LQ_ACT_NONE = 0, LQ_ACT_RELU = 1", header)
    assert lq.mx_gemm_quantize is ops.mx_gemm_quantize and lq.mx_dense_chain is L.mx_dense_chain
    assert ops.MX_ACTIVATIONS == (None, "relu")


def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    fused = lib.lq_mx_gemm_quantize

    def call(**kw):
        a = dict(ac=p, as_=p, fa=E4M3, bc=p, bs=p, fb=FP4, bias=None, act=1, fo=E4M3, method=0, oc=p, os_=p, M=16, N=16, K=128)
        a.update(kw)
        return fused(a["ac"], a["as_"], a["fa"], a["bc"], a["bs"], a["fb"], a["bias"], a["act"], a["fo"], a["method"], a["oc"], a["os_"],
                     a["M"], a["N"], a["K"], None)

    # an unknown or fp6 format on any of the three sides
    for side in ("fa", "fb", "fo"):
        for bad, needle in ((FP6A, "fp6 operands are not supported"), (FP6B, "fp6 operands are not supported"), (-1, "bad element format"),
                            (5, "bad element format")):
            assert call(**{side: bad}) == LQ_EINVAL and needle in _err(), (side, bad)
    for method in (-1, 2):
        assert call(method=method) == LQ_EINVAL and "bad method" in _err()
    for act in (-1, 2):
        assert call(act=act) == LQ_EINVAL and "bad activation" in _err()
    # every pointer but the bias
    for key in ("ac", "as_", "bc", "bs", "oc", "os_"):
        assert call(**{key: None}) == LQ_EINVAL and "NULL" in _err(), key
    # extents
    for key in ("M", "N", "K"):
        for v in (0, -1):
            assert call(**{key: v}) == LQ_EINVAL and "extents must be positive" in _err(), (key, v)
    assert call(M=1 << 20, K=1 << 11) == LQ_EINVAL and "not below 2^31" in _err()          # M * K
    assert call(N=1 << 20, K=1 << 11) == LQ_EINVAL and "not below 2^31" in _err()          # N * K
    assert call(M=1 << 16, N=1 << 15, K=128) == LQ_EINVAL and "not below 2^31" in _err()   # M * N alone
    assert call(M=65535 * 64 + 1, N=16, K=128) == LQ_EINVAL and "is above 65535 * 64" in _err()
    # alignment
    for key in ("ac", "bc", "oc"):
        assert call(**{key: p + 8}) == LQ_EALIGN and "codes is not 16-byte aligned" in _err(), key
    for key in ("as_", "bs", "os_"):
        assert call(**{key: p + 2}) == LQ_EALIGN and "scales is not 4-byte aligned" in _err(), key
    assert call(bias=p + 1) == LQ_EALIGN and "bias is not 4-byte aligned" in _err()


def _dense(units=4, n_in=70, **kw):
    return L.CustomDenseLayer(units=units, initializer=L.RandomNormal(seed=1), input_shape=n_in, **kw)


def test_refusals_of_the_python_surface():
    u8 = torch.zeros(16, dtype=torch.uint8)
    a, b = ops.MxOperand(u8, u8, "fp8_e4m3", 16, 128), ops.MxOperand(u8, u8, "fp4_e2m1", 16, 128)
    with pytest.raises(ValueError, match="different K: 128 and 160"):
        ops.mx_gemm_quantize(a, ops.MxOperand(u8, u8, "fp4_e2m1", 16, 160))
    for kw in (dict(out_format="fp6_e2m3"), dict(out_format="fp6_e3m2")):
        with pytest.raises(ValueError, match="fp6 operands are not supported"):
            ops.mx_gemm_quantize(a, b, **kw)
    with pytest.raises(ValueError, match="fp6 operands are not supported"):
        ops.mx_gemm_quantize(a, ops.MxOperand(u8, u8, "fp6_e2m3", 16, 128))
    with pytest.raises(ValueError, match="must be one of"):
        ops.mx_gemm_quantize(a, b, method="absmax")
    for bad in ("gelu", "RELU", 1, ""):
        with pytest.raises(ValueError, match="activation must be one of"):
            ops.mx_gemm_quantize(a, b, activation=bad)
    # layers: an operand as input must reduce over the layer's in
    good = _dense(orientation="groupwise", element_format="fp4_e2m1")
    with pytest.raises(ValueError, match=re.escape("reduces over K = 128, the layer over in = 70")):
        good.call_mx(a)
    with pytest.raises(ValueError, match="activation must be one of"):
        good.call_mx(torch.zeros(3, 70), out_format="fp8_e4m3", activation="tanh")
    with pytest.raises(ValueError, match="fp6 operands are not supported"):
        good.call_mx(torch.zeros(3, 70), out_format="fp6_e2m3")
    # the chain: ineligible layers and activations, named
    x = torch.zeros(3, 70)
    last = _dense(units=3, n_in=4, orientation="groupwise", element_format="fp4_e2m1")
    for kw, needle in ((dict(), "needs a layer with an element_format"),
                       (dict(orientation="groupwise", element_format="fp4_e2m1", scale_format="fp32"), "E8M0"),
                       (dict(orientation="groupwise", element_format="fp6_e2m3"), "fp6 operands are not supported"),
                       (dict(orientation="groupwise", element_format="fp8_e4m3", group_size=16), "group_size=16")):
        bad = _dense(**kw)
        with pytest.raises(ValueError, match=re.escape(needle)) as e:
            L.mx_dense_chain(x, [(bad, "relu"), (last, None)])
        assert bad.name in str(e.value)
    with pytest.raises(ValueError, match="only Dense layers"):
        L.mx_dense_chain(x, [(torch.nn.Linear(70, 4), "relu"), (last, None)])
    with pytest.raises(ValueError, match="activation must be one of"):
        L.mx_dense_chain(x, [(good, "sigmoid"), (last, None)])
    with pytest.raises(ValueError, match="the last layer writes fp32"):
        L.mx_dense_chain(x, [(good, "relu"), (last, "relu")])
    with pytest.raises(ValueError, match="the chain is empty"):
        L.mx_dense_chain(x, [])
    with pytest.raises(ValueError, match="fp6 operands"):
        L.mx_dense_chain(x, [(good, "relu"), (last, None)], act_format="fp6_e3m2")
    # mx_hardware
    m = build_model("mnist", mode="ste", value=0.0, element_format="fp4_e2m1")
    with pytest.raises(ValueError, match="emulate=True with fused=True"):
        L.mx_hardware(m, emulate=True, fused=True)
    hw = L.mx_hardware(m, fused=True)
    assert hw.fused and hw.fused_layers == [] and L.mx_hardware(m).fused is False
    assert [layer for layer, _ in m.mx_chain()] == [m.dense_1, m.dense_2] and [act for _, act in m.mx_chain()] == ["relu", None]


def test_driver_refusal_and_flag():
    from learned_quantization_amd import train
    with pytest.raises(SystemExit):
        train.main(["--config", "mnist", "--mode", "ste", "--element-format", "fp4_e2m1", "--mx-eval-fused"])
    ns = train.build_parser().parse_args(["--mx-eval", "--mx-eval-fused"])
    assert ns.mx_eval == "fp8_e4m3" and ns.mx_eval_fused is True
    assert train.build_parser().parse_args([]).mx_eval_fused is False
