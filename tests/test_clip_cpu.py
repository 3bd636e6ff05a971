"""CPU tests of the clipped b-bit fake-quant: C-ABI surface, argument validation without a launch, the bits / q_range
arithmetic, the refusals, the plumbing through layers and models, and the NumPy reference itself pinned on hand-written
tables (no GPU here)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, ops
from learned_quantization_amd.batch import FakeQuantBatch

sys.path.insert(0, os.path.dirname(__file__))
from _clip_reference import bits_equal, clip_reference, edge_table      # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("lq_fq_forward_clip", "lq_fq_backward_clip")
LQ_EINVAL = -1
LIM = 1 << 24


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
    assert lq.fq_forward_clip is ops.fq_forward_clip and lq.fq_backward_clip is ops.fq_backward_clip


def test_header_states_the_definition():
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    doc = header[header.index("clipped b-bit fake-quant"):header.index("int lq_fq_forward_clip")]
    for needle in ("floorf(t)", "q0 < lo ? lo : (q0 > hi ? hi : q0)", "inside_i ? dy_i : +0.0f", "ONE fp32 subtraction",
                   "(double)grad_scale", "clipped[g]", "mask only", "LQ_EINVAL"):
        assert needle in doc, needle


def test_forward_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    fn = lib.lq_fq_forward_clip
    ok = (-8, 7, 1, 3, 100, None)
    assert fn(None, p, p, None, 0, *ok) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fn(p, None, p, None, 0, *ok) == LQ_EINVAL and "'s' is NULL" in _err()
    assert fn(p, p, None, None, 0, *ok) == LQ_EINVAL and "'out' is NULL" in _err()
    assert _err().startswith("lq_fq_forward_clip:")
    assert fn(p, p, p, None, 0, 8, 7, 1, 3, 100, None) == LQ_EINVAL and "qmin 8 > qmax 7" in _err()
    assert fn(p, p, p, None, 0, -LIM - 1, 7, 1, 3, 100, None) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, p, None, 0, -8, LIM + 1, 1, 3, 100, None) == LQ_EINVAL and "outside +-2^24" in _err()
    for desc in ((0, 3, 100), (1, 0, 100), (1, 3, 0), (-1, 3, 100)):
        assert fn(p, p, p, None, 0, -8, 7, *desc, None) == LQ_EINVAL and "extents must be positive" in _err()
    assert fn(p, p, p, p, 0, *ok) == LQ_EINVAL and "q and q_dtype disagree" in _err()
    assert fn(p, p, p, None, 2, *ok) == LQ_EINVAL and "q and q_dtype disagree" in _err()
    assert fn(p, p, p, p, 9, *ok) == LQ_EINVAL and "bad q_dtype" in _err()


def test_backward_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) // 16 * 16
    fn = lib.lq_fq_backward_clip
    need = lib.lq_workspace_bytes(1, 3, 100)
    assert need > 0
    tail = (p16, need, 1, 3, 100, None)
    assert fn(None, p, p, -8, 7, 1.0, p, p, p, *tail) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fn(p, None, p, -8, 7, 1.0, p, p, p, *tail) == LQ_EINVAL and "'s' is NULL" in _err()
    assert fn(p, p, None, -8, 7, 1.0, p, p, p, *tail) == LQ_EINVAL and "'dy' is NULL" in _err()
    assert fn(p, p, p, -8, 7, 1.0, None, p, p, *tail) == LQ_EINVAL and "'dP' is NULL" in _err()
    assert _err().startswith("lq_fq_backward_clip:")
    assert fn(p, p, p, 1, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "qmin 1 > qmax 0" in _err()
    assert fn(p, p, p, -LIM - 1, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, p, 0, LIM + 1, 1.0, p, p, p, *tail) == LQ_EINVAL and "outside +-2^24" in _err()
    for desc in ((0, 3, 100), (1, 0, 100), (1, 3, 0)):
        assert fn(p, p, p, -8, 7, 1.0, p, p, p, p16, need, *desc, None) == LQ_EINVAL and "extents must be positive" in _err()
    # the workspace is required also for mask-only calls (ds == NULL, clipped == NULL)
    assert fn(p, p, p, -8, 7, 1.0, p, p, p, None, 0, 1, 3, 100, None) == LQ_EINVAL and "workspace is NULL" in _err()
    assert fn(p, p, p, -8, 7, 1.0, p, None, None, p16, need - 1, 1, 3, 100, None) == LQ_EINVAL and "too small" in _err()
    assert fn(p, p, p, -8, 7, 1.0, p, p, p, p16, 0, 1, 3, 100, None) == LQ_EINVAL and "too small" in _err()


def test_bits_signed_and_q_range_arithmetic():
    assert ops.q_range_of(4) == (-8, 7)
    assert ops.q_range_of(4, signed=False) == (0, 15)
    assert ops.q_range_of(1) == (-1, 0) and ops.q_range_of(1, signed=False) == (0, 1)
    assert ops.q_range_of(8) == (-128, 127) and ops.q_range_of(2) == (-2, 1)
    assert ops.q_range_of(24) == (-(1 << 23), (1 << 23) - 1) and ops.q_range_of(24, signed=False) == (0, LIM - 1)
    assert ops.q_range_of(q_range=(-LIM, LIM)) == (-LIM, LIM) and ops.q_range_of(q_range=(3, 3)) == (3, 3)
    assert ops.q_range_of() is None
    for bad in (0, 25, -1, 2.5):
        with pytest.raises(ValueError, match="bits must be"):
            ops.q_range_of(bad)
    with pytest.raises(ValueError, match="qmin <= qmax"):
        ops.q_range_of(q_range=(1, 0))
    with pytest.raises(ValueError, match="outside"):
        ops.q_range_of(q_range=(-LIM - 1, 0))
    with pytest.raises(ValueError, match="not both"):
        ops.q_range_of(4, q_range=(-8, 7))
    init = lq.RandomNormal(seed=1)
    with pytest.raises(ValueError, match="not both"):
        lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, bits=4, q_range=(-8, 7))
    with pytest.raises(ValueError, match="bits must be"):
        lq.CustomConv2DLayer(filters=4, initializer=init, input_shape=2, bits=25)
    with pytest.raises(ValueError, match="qmin <= qmax"):
        lq.CustomQuantizedScaleLayer(q_range=(1, 0))


def test_a_threshold_is_refused():
    P, s = torch.zeros(4, 4), torch.ones(1, 4)
    with pytest.raises(ValueError, match="unclipped"):
        ops.my_custom_gradient(P, s, 1e-11, q_range=(-8, 7))
    with pytest.raises(ValueError, match="unclipped"):
        lq.CustomQuantizedScaleLayer(penalty_threshold=1e-11, bits=4)
    with pytest.raises(ValueError, match="unclipped"):
        lq.CustomDenseLayer(units=3, initializer=lq.RandomNormal(seed=1), input_shape=5, penalty_threshold=1e-11, bits=4)
    for mode, value in (("nq", 1e-11), ("nqcl", (1e-11, 1e-7))):
        with pytest.raises(ValueError, match="unclipped"):
            lq.build_model("mnist", mode=mode, value=value, bits=4)
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="unclipped"):
        Trainer("mnist", "nq", 1e-11, "rowwise", device=torch.device("cpu"), bits=4)


def test_the_exact_data_parallel_mode_is_refused():
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="clipped elements"):
        Trainer("mnist", "cl", 1e-7, "rowwise", "maxbin", device=torch.device("cpu"), ddp_mode="B", bits=4)
    lq.reset_layer_names()
    m = lq.build_model("mnist", mode="cl", value=1e-7, bits=4)
    with pytest.raises(ValueError, match="clipped elements"):
        lq.DataParallel(m, mode="B")
    with pytest.raises(ValueError, match="defer_scale_grad"):
        ops.my_custom_gradient(torch.zeros(4, 4), torch.ones(1, 4), q_range=(-8, 7), defer_scale_grad=True)


def test_the_batch_is_refused():
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="masked copy"):
        Trainer("mnist", "ste", 0.0, "rowwise", device=torch.device("cpu"), batched=True, bits=4)
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=2)
    a = lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, scale_gradient="ste", bits=4)
    b = lq.CustomDenseLayer(units=3, initializer=init, input_shape=3, scale_gradient="ste")
    with pytest.raises(ValueError, match="masked copy"):
        FakeQuantBatch([a])
    with pytest.raises(ValueError, match="masked copy"):
        FakeQuantBatch([b, a])
    with pytest.raises(ValueError, match="masked copy"):
        FakeQuantBatch(lq.build_model("mnist", mode="ste", value=0.0, q_range=(0, 15)))


def test_layers_and_models_carry_the_range():
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=3)
    d = lq.CustomDenseLayer(units=3, orientation="columnwise", initializer=init, input_shape=5, scale_gradient="ste", bits=4)
    assert d.q_range == d.nested_q_w_layer.q_range == d.nested_q_b_layer.q_range == (-8, 7)
    assert "q_range=(-8, 7)" in repr(d.nested_q_w_layer) and "q_range=(-8, 7)" in repr(d)
    c = lq.CustomConv2DLayer(filters=4, initializer=init, input_shape=2, bits=4, signed=False, penalty_rate=1e-7)
    assert c.q_range == c.nested_q_k_layer.q_range == c.nested_q_b_layer.q_range == (0, 15)
    nb = lq.CustomConv2DLayerNoBias(filters=4, initializer=init, input_shape=2, q_range=(-3, 5))
    assert nb.nested_q_k_layer.q_range == (-3, 5) and "q_range=(-3, 5)" in repr(nb)
    plain = lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, penalty_threshold=1e-11)
    assert plain.q_range is None and plain.nested_q_w_layer.q_range is None and "q_range" not in repr(plain)
    # the import-path mirrors pick the arguments up by inheritance
    from learned_quantization_amd.nested_quantization_layer import custom_layers as NQ
    from learned_quantization_amd.custom_loss_terms import custom_layers as CL
    layer = NQ.CustomDenseLayer(units=3, initializer=init, input_shape=5, bits=2)
    assert layer.nested_q_w_layer.q_range == layer.nested_q_b_layer.q_range == (-2, 1)
    layer = CL.CustomDenseLayer(1, 3, 1e-7, "rowwise", init, "d", None, input_shape=5, bits=2)
    assert layer.nested_q_w_layer.q_range == layer.nested_q_b_layer.q_range == (-2, 1) and layer.nested_q_w_layer.penalty_rate == 1e-7
    conv = CL.CustomConv2DLayer(1, 1e-7, "channelwise", init, 4, (3, 3), (1, 1), "same", "c", None, input_shape=2, q_range=(0, 3))
    assert conv.nested_q_k_layer.q_range == conv.nested_q_b_layer.q_range == (0, 3)
    for config, kw in (("mnist", dict(mode="ste", value=0.0, bits=4)), ("cifar", dict(mode="stecl", value=1e-7, bits=8)),
                       ("mnist", dict(mode="cl", value=1e-7, bits=4, signed=False)),
                       ("mnist", dict(mode="ste", value=0.0, q_range=(-5, 9), grad_scale="rsqrt_group"))):
        lq.reset_layer_names()
        m = lq.build_model(config, seed=1, **kw)
        want = ops.q_range_of(kw.get("bits"), kw.get("signed", True), kw.get("q_range"))
        layers = lq.custom_layers_of(m)
        assert layers
        for layer in layers:
            assert layer.q_range == want
            for a in ("nested_q_w_layer", "nested_q_k_layer", "nested_q_b_layer"):
                if hasattr(layer, a):
                    assert getattr(layer, a).q_range == want
        if kw.get("grad_scale"):
            assert layers[0].nested_q_w_layer.grad_scale == "rsqrt_group"
    lq.reset_layer_names()
    assert all(l.q_range is None for l in lq.custom_layers_of(lq.build_model("mnist", mode="ste", value=0.0)))


# ---------------------------------------------------------------------------------------------- the NumPy reference, pinned
@pytest.mark.parametrize("qmin,qmax", [(-8, 7), (0, 15), (-2, 1), (-128, 127)])
def test_reference_on_the_edge_table(qmin, qmax):
    s = np.float32(2.0 ** -7)
    P, q_want, inside_want = edge_table(qmin, qmax, s)
    dy = np.arange(1, P.size + 1, dtype=np.float32)
    ref = clip_reference(P, np.array([s], np.float32), dy, qmin, qmax)
    assert np.array_equal(P / s, P * np.float32(128.0))                      # quotients are exact
    assert np.array_equal(ref["q"], q_want)
    assert np.array_equal(ref["inside"], inside_want)
    assert np.array_equal(ref["out"], q_want * s)
    assert bits_equal(ref["dP"], np.where(inside_want, dy, np.float32(0.0)))
    assert not np.any(np.signbit(ref["dP"][~inside_want]))                   # +0, not -0
    assert int(ref["clipped"][0]) == int((~inside_want).sum()) == 5
    t = P / s
    r = np.where(inside_want, np.floor(t) - t, q_want).astype(np.float64)
    assert ref["ds"][0] == np.sum(dy.astype(np.float64) * r)
    assert ref["terms"][0] == np.sum(np.abs(dy.astype(np.float64) * r))
    # hand-checked rows: t = qmin - 2^-7 floors to qmin - 1 (outside, r = qmin); t = qmax + 1 - ulp floors to qmax (inside)
    assert not ref["inside"][1] and ref["q"][1] == qmin
    assert ref["inside"][7] and ref["q"][7] == qmax and -1.0 <= (np.floor(t[7]) - t[7]) < 0.0


def test_reference_on_special_values():
    s = np.array([1.0], np.float32)
    P = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 3e38, -3e38, 1e-45, -1e-45, 2.5], np.float32)
    dy = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10], np.float32)
    ref = clip_reference(P, s, dy, -8, 7)
    q = ref["q"]
    assert q[0] == 7 and q[1] == -8 and np.isnan(q[2])                        # +-Inf saturates, NaN stays NaN
    assert q[3] == 0 and q[4] == 0 and np.signbit(q[4]) and not np.signbit(q[3])      # floor(-0) = -0
    assert q[5] == 7 and q[6] == -8 and q[7] == 0 and q[8] == -1 and q[9] == 2
    assert list(ref["inside"]) == [False, False, False, True, True, False, False, True, True, True]
    assert bits_equal(ref["dP"], np.array([0, 0, 0, 4, 5, 0, 0, 8, 9, 10], np.float32))
    assert not np.any(np.signbit(ref["dP"][:3]))
    assert int(ref["clipped"][0]) == 5
    assert np.isnan(ref["ds"][0]) and np.isnan(ref["terms"][0])               # the NaN element poisons its group's sum
    assert np.isnan(ref["out"][2]) and ref["out"][0] == 7.0 and ref["out"][1] == -8.0
    clean = clip_reference(np.delete(P, 2), s, np.delete(dy, 2), -8, 7)
    # terms: 1*7, 2*-8, 4*0, 5*(-0 - -0 = 0), 6*7, 7*-8, 8*(0 - 1e-45), 9*(-1 - -1e-45 = -1), 10*(2 - 2.5)
    want = 7.0 - 16.0 + 0.0 + 0.0 + 42.0 - 56.0 + 8.0 * -float(np.float32(1e-45)) - 9.0 - 5.0
    assert clean["ds"][0] == want and int(clean["clipped"][0]) == 4
    # the degenerate range: everything saturates at 0, inside only where floor(t) == 0
    deg = clip_reference(np.array([-1.5, -0.5, 0.0, 0.5, 1.0], np.float32), s, np.ones(5, np.float32), 0, 0)
    assert np.all(deg["out"] == 0.0) and list(deg["inside"]) == [False, False, True, True, False]
