"""CPU tests of the straight-through scale gradient: C-ABI surface, argument validation without a launch, and the Python
plumbing that needs no device (no GPU here)."""
import ctypes
import os
import re

import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, models, ops
from learned_quantization_amd.batch import FakeQuantBatch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("lq_fq_scale_grad_ste", "lq_batch_scale_grad_ste")
LQ_EINVAL, LQ_EWORKSPACE, LQ_EALIGN = -1, -3, -4


def _err():
    return _hip.load().lq_last_error().decode()


def test_abi_version_stays_3():
    assert _hip.load().lq_version() == 3            # additions only


def test_new_entry_points_are_declared_exported_and_bound():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/lq_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.SIGNATURES, f"{name} is not in the binding table"
    assert "fq_scale_grad_ste" in dir(lq) and lq.fq_scale_grad_ste is ops.fq_scale_grad_ste


def test_header_states_the_definition_and_the_missing_bit_identity():
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    doc = header[header.index("straight-through scale gradient"):header.index("int lq_fq_scale_grad_ste")]
    for needle in ("floorf(t_i)", "ONE fp32 subtraction", "(double)grad_scale", "NO bit-identity across traversals", "2^23"):
        assert needle in doc, needle


def test_single_tensor_entry_point_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    p16 = (p + 15) // 16 * 16
    fn = lib.lq_fq_scale_grad_ste
    need = lib.lq_workspace_bytes(1, 3, 100)
    assert need > 0
    # NULLs
    assert fn(None, p, p, 1.0, p, p16, need, 1, 3, 100, None) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fn(p, None, p, 1.0, p, p16, need, 1, 3, 100, None) == LQ_EINVAL and "'s' is NULL" in _err()
    assert fn(p, p, None, 1.0, p, p16, need, 1, 3, 100, None) == LQ_EINVAL and "'dy' is NULL" in _err()
    assert fn(p, p, p, 1.0, None, p16, need, 1, 3, 100, None) == LQ_EINVAL and "'ds' is NULL" in _err()
    assert _err().startswith("lq_fq_scale_grad_ste:")
    # non-positive extents
    for desc in ((0, 3, 100), (1, 0, 100), (1, 3, 0), (-1, 3, 100)):
        assert fn(p, p, p, 1.0, p, p16, need, *desc, None) == LQ_EINVAL and "extents must be positive" in _err()
    # pointers off the float grid
    assert fn(p + 2, p, p, 1.0, p, p16, need, 1, 3, 100, None) == LQ_EALIGN
    assert fn(p, p, p + 1, 1.0, p, p16, need, 1, 3, 100, None) == LQ_EALIGN
    # workspace: missing, misaligned, short
    assert fn(p, p, p, 1.0, p, None, 0, 1, 3, 100, None) == LQ_EWORKSPACE and "workspace is NULL" in _err()
    assert fn(p, p, p, 1.0, p, p16 + 8, need, 1, 3, 100, None) == LQ_EALIGN and "16-byte aligned" in _err()
    assert fn(p, p, p, 1.0, p, p16, need - 1, 1, 3, 100, None) == LQ_EWORKSPACE and "too small" in _err()


def test_batch_entry_point_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    dys = (ctypes.c_void_p * 2)(p, p)
    gs = (ctypes.c_float * 2)(1.0, 0.5)
    assert lib.lq_batch_scale_grad_ste(None, dys, gs, p, 1024, None) == LQ_EINVAL and _err() == "lq_batch_scale_grad_ste: NULL batch"
    assert lib.lq_batch_scale_grad_ste(None, None, None, None, 0, None) == LQ_EINVAL and "NULL batch" in _err()


def test_ste_needs_the_two_argument_op():
    P = torch.zeros(4, 4)
    s = torch.ones(1, 4)
    with pytest.raises(ValueError, match="penalty_threshold=None"):
        ops.my_custom_gradient(P, s, 1e-11, scale_gradient="ste")
    with pytest.raises(ValueError, match="scale_gradient must be one of"):
        ops.my_custom_gradient(P, s, scale_gradient="lsq")
    with pytest.raises(ValueError, match="penalty_threshold=None"):
        lq.CustomQuantizedScaleLayer(penalty_threshold=1e-11, scale_gradient="ste")
    with pytest.raises(ValueError, match="scale_gradient must be one of"):
        lq.CustomDenseLayer(units=4, scale_gradient="lsq")


def test_kw_accepts_the_two_modes():
    assert models._kw("ste", 123.0) == dict(penalty_threshold=None, scale_gradient="ste")       # value ignored
    assert models._kw("stecl", 1e-7) == dict(penalty_threshold=None, penalty_rate=1e-7, scale_gradient="ste")
    assert models._kw("cl", 1e-7) == dict(penalty_threshold=None, penalty_rate=1e-7)             # the existing modes are unchanged
    assert models._kw("nq", 1e-11) == dict(penalty_threshold=1e-11)
    with pytest.raises(ValueError):
        models._kw("lsq", 0.0)


def test_layers_pass_rule_and_factor_through():
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=1)
    m = lq.build_model("mnist", mode="ste", value=0.0, seed=1, grad_scale="rsqrt_group")
    for layer in lq.custom_layers_of(m):
        for nested, param in ((layer.nested_q_w_layer, layer.W), (layer.nested_q_b_layer, layer.b)):
            assert nested.scale_gradient == "ste" and nested.penalty_threshold is None and nested.grad_scale == "rsqrt_group"
            per_group = param.numel() / nested.scale.numel()
            assert nested.grad_scale_value(param.numel()) == pytest.approx(per_group ** -0.5, rel=1e-12)
    d = lq.CustomDenseLayer(units=3, orientation="columnwise", initializer=init, input_shape=5, scale_gradient="ste", grad_scale=0.25)
    assert d.nested_q_w_layer.grad_scale_value(15) == 0.25 and d.nested_q_b_layer.scale_gradient == "ste"
    c = lq.CustomConv2DLayer(filters=4, initializer=init, input_shape=2, scale_gradient="ste")
    assert c.nested_q_k_layer.scale_gradient == "ste" and c.nested_q_k_layer.grad_scale == 1.0
    plain = lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, penalty_threshold=1e-11)
    assert plain.nested_q_w_layer.scale_gradient is None                                         # the default is today's behaviour


def test_a_batch_mixing_rules_raises():
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=2)
    a = lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, scale_gradient="ste")
    b = lq.CustomDenseLayer(units=3, initializer=init, input_shape=3, penalty_threshold=1e-11)
    c = lq.CustomDenseLayer(units=3, initializer=init, input_shape=3, penalty_rate=1e-7)
    for pair in ([a, b], [a, c]):
        with pytest.raises(ValueError, match="one scale-gradient rule"):
            FakeQuantBatch(pair)


def test_trainer_refuses_the_exact_data_parallel_mode():
    from learned_quantization_amd.train import Trainer
    for mode, loss in (("ste", None), ("stecl", "maxbin")):
        with pytest.raises(ValueError, match="linear in dy"):
            Trainer("mnist", mode, 1e-7, "rowwise", loss, device=torch.device("cpu"), ddp_mode="B")
