"""CPU tests of the group-wise (block) scales of the clipped b-bit quantizer: the NumPy reference pinned on a hand-written table and
against tests/_clip_reference.py where the two coincide, the C-ABI surface, argument validation without a launch, the second
descriptor (descriptor.group_geometry / groupwise_scale_shape) and every refusal (no GPU here)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, ops
from learned_quantization_amd.descriptor import group_geometry, groupwise_scale_shape

sys.path.insert(0, os.path.dirname(__file__))
from _clip_reference import bits_equal, clip_reference                              # noqa: E402
from _group_reference import expand_scale, group_reference, make_case, scale_shape  # noqa: E402
from _rne_reference import rne_reference                                            # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("lq_group_workspace_bytes", "lq_fq_forward_group", "lq_fq_backward_group")
LQ_EINVAL = -1
LIM = 1 << 24


def _err():
    return _hip.load().lq_last_error().decode()


# ------------------------------------------------------------------------------------------------------- the reference, pinned
# quotients of a 5 x 3 matrix, range [-2, 1]; the scales are powers of two, so P = t * s is exact and P / s gives t back
T = np.array([[0.5, -1.25, 1.0],
              [-2.0, 2.5, -0.75],
              [1.5, -3.0, 0.25],
              [-0.5, 0.75, -2.5],
              [3.0, -1.0, 1.75]], np.float32)
DY = np.arange(1, 16, dtype=np.float32).reshape(5, 3)
# floor: q0 and, written out by hand, the clamped integers, the inside mask and dy * r with r = q0 - t inside and q outside
Q_FLOOR = np.array([[0, -2, 1], [-2, 1, -1], [1, -2, 0], [-1, 0, -2], [1, -1, 1]], np.float32)
INSIDE_FLOOR = np.array([[1, 1, 1], [1, 0, 1], [1, 0, 1], [1, 1, 0], [0, 1, 1]], bool)
PROD_FLOOR = np.array([[-0.5, -1.5, 0.0], [0.0, 5.0, -1.5], [-3.5, -16.0, -2.25], [-5.0, -8.25, -24.0], [13.0, 0.0, -11.25]])
S_AXIS0 = np.array([[0.5, 1.0, 2.0], [1.0, 1.0, 1.0], [0.25, 0.5, 1.0]], np.float32)                  # [nb = 3][C = 3]
S_AXIS1 = np.array([[0.5, 1.0], [2.0, 0.25], [1.0, 1.0], [0.125, 4.0], [1.0, 0.5]], np.float32)      # [R = 5][nb = 2]


def test_reference_on_the_hand_written_table_axis0():
    # gs = 2 along the rows: groups {0, 1}, {2, 3} and the ragged {4}
    sb = np.array([S_AXIS0[0], S_AXIS0[0], S_AXIS0[1], S_AXIS0[1], S_AXIS0[2]], np.float32)
    assert np.array_equal(expand_scale(S_AXIS0, 5, 3, 0, 2), sb)
    P = T * sb
    ref = group_reference(P, S_AXIS0, DY, -2, 1, axis=0, gs=2)
    assert np.array_equal(ref["t"], T) and np.array_equal(ref["q"], Q_FLOOR) and np.array_equal(ref["inside"], INSIDE_FLOOR)
    assert bits_equal(ref["out"], Q_FLOOR * sb)
    assert bits_equal(ref["dP"], np.where(INSIDE_FLOOR, DY, np.float32(0.0))) and not np.any(np.signbit(ref["dP"][~INSIDE_FLOOR]))
    assert np.array_equal(ref["ds"], [[-0.5, 3.5, -1.5], [-8.5, -24.25, -26.25], [13.0, 0.0, -11.25]])
    assert np.array_equal(ref["terms"], [[0.5, 6.5, 1.5], [8.5, 24.25, 26.25], [13.0, 0.0, 11.25]])
    assert np.array_equal(ref["clipped"], [[0, 1, 0], [0, 1, 1], [1, 0, 0]])
    assert np.array_equal(ref["ds"][2], PROD_FLOOR[4])                                   # the ragged group is row 4 alone
    half = group_reference(P, S_AXIS0, DY, -2, 1, axis=0, gs=2, k=0.5)
    assert np.array_equal(half["ds"], ref["ds"] * 0.5) and np.array_equal(half["terms"], ref["terms"] * 0.5)


def test_reference_on_the_hand_written_table_axis1():
    # gs = 2 along the columns: groups {0, 1} and the ragged {2}
    sb = np.stack([S_AXIS1[:, 0], S_AXIS1[:, 0], S_AXIS1[:, 1]], axis=1)
    assert np.array_equal(expand_scale(S_AXIS1, 5, 3, 1, 2), sb)
    P = T * sb
    ref = group_reference(P, S_AXIS1, DY, -2, 1, axis=1, gs=2)
    assert np.array_equal(ref["t"], T) and np.array_equal(ref["q"], Q_FLOOR) and np.array_equal(ref["inside"], INSIDE_FLOOR)
    assert bits_equal(ref["out"], Q_FLOOR * sb)
    assert bits_equal(ref["dP"], np.where(INSIDE_FLOOR, DY, np.float32(0.0)))
    assert np.array_equal(ref["ds"], [[-2.0, 0.0], [5.0, -1.5], [-19.5, -2.25], [-13.25, -24.0], [13.0, -11.25]])
    assert np.array_equal(ref["terms"], [[2.0, 0.0], [5.0, 1.5], [19.5, 2.25], [13.25, 24.0], [13.0, 11.25]])
    assert np.array_equal(ref["clipped"], [[0, 0], [1, 0], [1, 0], [0, 1], [1, 0]])
    assert np.array_equal(ref["ds"][:, 1], PROD_FLOOR[:, 2])                             # the ragged group is column 2 alone


def test_reference_nearest_on_the_hand_written_table():
    # rint: 0.5 -> 0, 2.5 -> 2, 1.5 -> 2, -0.5 -> -0, -2.5 -> -2 (ties to even); -1.25 -> -1, 0.75 -> 1, 1.75 -> 2
    q = np.array([[0, -1, 1], [-2, 1, -1], [1, -2, 0], [-0.0, 1, -2], [1, -1, 1]], np.float32)
    inside = np.array([[1, 1, 1], [1, 0, 1], [0, 0, 1], [1, 1, 1], [0, 1, 0]], bool)
    sb = expand_scale(S_AXIS0, 5, 3, 0, 2)
    ref = group_reference(T * sb, S_AXIS0, DY, -2, 1, axis=0, gs=2, rounding="nearest")
    assert bits_equal(ref["q"], q) and np.signbit(ref["q"][3, 0]) and np.array_equal(ref["inside"], inside)
    assert np.array_equal(ref["clipped"], [[0, 1, 0], [1, 1, 0], [1, 0, 1]])
    # column 0: rows {0, 1}: 1 * (0 - 0.5) + 4 * (-2 - -2) ; rows {2, 3}: 7 * 1 (clipped at qmax) + 10 * (-0 - -0.5) ; row 4: 13 * 1
    assert np.array_equal(ref["ds"][:, 0], [-0.5, 12.0, 13.0])


def _same(a, b, keys=("out", "q", "dP")):
    return all(bits_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("rounding,one_axis", [("floor", clip_reference), ("nearest", rne_reference)])
def test_reference_coincides_with_the_one_axis_reference(rounding, one_axis):
    R, C = 12, 20
    rng = np.random.default_rng(5)
    P = rng.standard_normal((R, C)).astype(np.float32)
    dy = rng.standard_normal((R, C)).astype(np.float32)
    # axis 0 with gs >= R is column-wise
    for gs in (R, R + 7):
        s = np.exp2(rng.uniform(-4, -2, size=(1, C))).astype(np.float32)
        a, b = group_reference(P, s, dy, -8, 7, 0, gs, k=0.37, rounding=rounding), one_axis(P, s, dy, -8, 7, k=0.37)
        assert _same(a, b) and np.array_equal(a["ds"], b["ds"]) and np.array_equal(a["clipped"], b["clipped"])
        assert np.array_equal(a["terms"], b["terms"])
    # axis 1 with gs >= C is row-wise
    for gs in (C, 3 * C):
        s = np.exp2(rng.uniform(-4, -2, size=(R, 1))).astype(np.float32)
        a, b = group_reference(P, s, dy, -8, 7, 1, gs, rounding=rounding), one_axis(P, s, dy, -8, 7)
        assert _same(a, b) and np.array_equal(a["ds"], b["ds"]) and np.array_equal(a["clipped"], b["clipped"])
    # axis 1 with gs | C is the reshaped (R * C / gs, gs) row-wise case
    gs = 5
    s = np.exp2(rng.uniform(-4, -2, size=(R, C // gs))).astype(np.float32)
    a = group_reference(P, s, dy, -8, 7, 1, gs, rounding=rounding)
    b = one_axis(P.reshape(-1, gs), s.reshape(-1, 1), dy.reshape(-1, gs), -8, 7)
    assert all(bits_equal(a[k], b[k].reshape(R, C)) for k in ("out", "q", "dP"))
    assert np.array_equal(a["ds"], b["ds"].reshape(s.shape)) and np.array_equal(a["clipped"], b["clipped"].reshape(s.shape))


def test_make_case_shapes():
    P, s, dy = make_case(1, 37, 5, 0, 8)
    assert P.shape == dy.shape == (37, 5) and s.shape == scale_shape(37, 5, 0, 8) == (5, 5) and P.dtype == s.dtype == np.float32
    assert make_case(1, 7, 27, 1, 8)[1].shape == (7, 4)
    assert np.all(s >= 2.0 ** -9) and np.all(s <= 2.0 ** -5)


# ------------------------------------------------------------------------------------------------------------------ C ABI
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
    assert lq.fq_forward_group is ops.fq_forward_group and lq.fq_backward_group is ops.fq_backward_group
    assert lq.group_geometry is group_geometry and lq.groupwise_scale_shape is groupwise_scale_shape


def test_header_states_the_definition():
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    doc = header[header.index("group-wise (block) scales"):header.index("size_t lq_group_workspace_bytes")]
    for needle in ("[R][C]", "R * C < 2^31", "nb = ceil(len / gs)", "[nb][C]", "[R][nb]", "s[r / gs][c]", "s[r][c / gs]",
                   "floorf(t) or rintf(t)", "inside ? dy : +0.0f", "(double)grad_scale", "clipped[g]", "mask only", "LQ_EINVAL",
                   "LQ_EALIGN", "no bit-identity"):
        assert needle in doc, needle


def test_workspace_query_needs_no_gpu():
    lib = _hip.load()
    for R, C, axis, gs in ((37, 5, 0, 8), (4608, 512, 0, 128), (512, 4608, 1, 100), (96, 130, 0, 96)):
        assert lib.lq_group_workspace_bytes(R, C, axis, gs) >= 0


def test_forward_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    fn = lib.lq_fq_forward_group
    rng, geo = (-8, 7, 0), (5, 3, 0, 2, None)
    assert fn(None, p, p, None, 0, *rng, *geo) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fn(p, None, p, None, 0, *rng, *geo) == LQ_EINVAL and "'s' is NULL" in _err()
    assert fn(p, p, None, None, 0, *rng, *geo) == LQ_EINVAL and "'out' is NULL" in _err()
    assert _err().startswith("lq_fq_forward_group:")
    assert fn(p, p, p, None, 0, 8, 7, 0, *geo) == LQ_EINVAL and "qmin 8 > qmax 7" in _err()
    assert fn(p, p, p, None, 0, -LIM - 1, 7, 0, *geo) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, p, None, 0, -8, LIM + 1, 0, *geo) == LQ_EINVAL and "outside +-2^24" in _err()
    for bad in (2, -1, 7):
        assert fn(p, p, p, None, 0, -8, 7, bad, *geo) == LQ_EINVAL and "bad rounding" in _err()
    for axis in (2, -1):
        assert fn(p, p, p, None, 0, *rng, 5, 3, axis, 2, None) == LQ_EINVAL and "bad axis" in _err()
    for gs in (0, -4):
        assert fn(p, p, p, None, 0, *rng, 5, 3, 0, gs, None) == LQ_EINVAL and "group size" in _err()
    for R, C in ((0, 3), (5, 0), (-1, 3), (5, -2)):
        assert fn(p, p, p, None, 0, *rng, R, C, 0, 2, None) == LQ_EINVAL and "extents must be positive" in _err()
    for R, C in ((1 << 31, 1), (1 << 16, 1 << 15), (46341, 46341)):
        assert fn(p, p, p, None, 0, *rng, R, C, 1, 2, None) == LQ_EINVAL and "not below 2^31" in _err()
    assert fn(p, p, p, p, 0, *rng, *geo) == LQ_EINVAL and "q and q_dtype disagree" in _err()
    assert fn(p, p, p, None, 2, *rng, *geo) == LQ_EINVAL and "q and q_dtype disagree" in _err()
    assert fn(p, p, p, p, 9, *rng, *geo) == LQ_EINVAL and "bad q_dtype" in _err()
    assert fn(p + 2, p, p, None, 0, *rng, *geo) == -4 and "not 4-byte aligned" in _err()       # LQ_EALIGN


def test_backward_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    fn = lib.lq_fq_backward_group
    tail = (None, 0, 5, 3, 1, 2, None)
    assert fn(None, p, p, -8, 7, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fn(p, None, p, -8, 7, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "'s' is NULL" in _err()
    assert fn(p, p, None, -8, 7, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "'dy' is NULL" in _err()
    assert fn(p, p, p, -8, 7, 0, 1.0, None, p, p, *tail) == LQ_EINVAL and "'dP' is NULL" in _err()
    assert _err().startswith("lq_fq_backward_group:")
    assert fn(p, p, p, 1, 0, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "qmin 1 > qmax 0" in _err()
    assert fn(p, p, p, -LIM - 1, 0, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, p, 0, LIM + 1, 0, 1.0, p, p, p, *tail) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, p, -8, 7, 3, 1.0, p, p, p, *tail) == LQ_EINVAL and "bad rounding" in _err()
    assert fn(p, p, p, -8, 7, 0, 1.0, p, p, p, None, 0, 5, 3, 2, 2, None) == LQ_EINVAL and "bad axis" in _err()
    assert fn(p, p, p, -8, 7, 0, 1.0, p, p, p, None, 0, 5, 3, 1, 0, None) == LQ_EINVAL and "group size" in _err()
    for R, C in ((0, 3), (5, 0), (-5, 3)):
        assert fn(p, p, p, -8, 7, 0, 1.0, p, p, p, None, 0, R, C, 1, 2, None) == LQ_EINVAL and "extents must be positive" in _err()
    assert fn(p, p, p, -8, 7, 0, 1.0, p, p, p, None, 0, 1 << 20, 1 << 11, 0, 2, None) == LQ_EINVAL and "not below 2^31" in _err()
    assert fn(p, p, p + 1, -8, 7, 0, 1.0, p, p, p, *tail) == -4 and "not 4-byte aligned" in _err()


# ---------------------------------------------------------------------------------------------------------- the descriptor
def test_groupwise_scale_shape():
    assert groupwise_scale_shape((784, 128), 64) == (13, 128)            # Dense: (nb, out), 784 = 12.25 * 64
    assert groupwise_scale_shape((128, 10), 64) == (2, 10)
    assert groupwise_scale_shape((128, 10), 1000) == (1, 10)
    assert groupwise_scale_shape((3, 3, 16, 32), 32) == (32, 5)          # conv HWIO shape: (co, nb), 144 = 4.5 * 32
    assert groupwise_scale_shape((3, 3, 3, 64), 128) == (64, 1)
    assert groupwise_scale_shape((5, 7), 1) == (5, 7)
    for bad in (0, -1, 2.5, None, True):
        with pytest.raises((ValueError, TypeError)):
            groupwise_scale_shape((4, 4), bad)
    with pytest.raises(ValueError, match="at least two"):
        groupwise_scale_shape((10,), 4)
    assert lq.ORIENTATIONS == ("rowwise", "columnwise", "channelwise", "scalar")       # unchanged
    with pytest.raises(ValueError, match="Invalid scaler application"):
        lq.scale_shape((4, 4), "groupwise")                                            # scale_shape stays the reference's


def test_group_geometry_dense_conv_and_non_dense():
    w = torch.empty(784, 128)
    assert group_geometry(w.shape, w.stride(), (13, 128), 64) == (784, 128, 0)
    assert group_geometry(w.shape, w.stride(), (1, 128), 784) == (784, 128, 0)
    assert group_geometry(w.shape, w.stride(), (784, 2), 64) == (784, 128, 1)          # groups along the contiguous axis
    k = torch.empty(32, 16, 3, 3).permute(2, 3, 1, 0)                                  # HWIO shape, OIHW memory
    assert tuple(k.shape) == (3, 3, 16, 32)
    assert group_geometry(k.shape, k.stride(), (32, 5), 32) == (32, 144, 1)
    assert group_geometry(k.shape, k.stride(), groupwise_scale_shape(k.shape, 1000), 1000) == (32, 144, 1)
    with pytest.raises(ValueError, match="memory order"):                              # the same scale on an HWIO-stored kernel
        group_geometry(k.shape, k.contiguous().stride(), (32, 5), 32)
    with pytest.raises(ValueError, match="dense"):
        group_geometry((4, 4), (8, 1), (2, 4), 2)                                      # a gap between the rows
    with pytest.raises(ValueError, match="dense"):
        group_geometry((4, 4), (0, 1), (2, 4), 2)                                      # a broadcast stride
    with pytest.raises(ValueError, match="matrix"):
        group_geometry(w.shape, w.stride(), (128,), 64)
    with pytest.raises(ValueError, match="memory order"):
        group_geometry(w.shape, w.stride(), (12, 128), 64)
    with pytest.raises(ValueError, match="group_size"):
        group_geometry(w.shape, w.stride(), (13, 128), 0)
    with pytest.raises(ValueError, match="more than one non-unit axis"):               # the flat descriptor still rejects it
        lq.group_descriptor((784, 128), (13, 128))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_the_op_refuses_with_the_reason():
    P, s = torch.zeros(8, 4), torch.ones(2, 4)
    with pytest.raises(ValueError, match="needs a q_range"):
        ops.my_custom_gradient(P, s, group_size=4)
    with pytest.raises(ValueError, match="unclipped"):
        ops.my_custom_gradient(P, s, 1e-11, q_range=(-8, 7), group_size=4)
    with pytest.raises(ValueError, match="defer_scale_grad"):
        ops.my_custom_gradient(P, s, q_range=(-8, 7), group_size=4, defer_scale_grad=True)


def test_the_layers_refuse_with_the_reason():
    init = lq.RandomNormal(seed=1)
    with pytest.raises(ValueError, match="needs bits or q_range"):
        lq.CustomQuantizedScaleLayer(orientation="groupwise", group_size=64)
    with pytest.raises(ValueError, match="needs bits or q_range"):
        lq.CustomDenseLayer(units=3, orientation="groupwise", group_size=4, initializer=init, input_shape=5, scale_gradient="ste")
    with pytest.raises(ValueError, match="needs group_size"):
        lq.CustomDenseLayer(units=3, orientation="groupwise", initializer=init, input_shape=5, bits=4)
    with pytest.raises(ValueError, match='needs orientation="groupwise"'):
        lq.CustomDenseLayer(units=3, orientation="rowwise", group_size=4, initializer=init, input_shape=5, bits=4)
    with pytest.raises(ValueError, match="integer >= 1"):
        lq.CustomDenseLayer(units=3, orientation="groupwise", group_size=0, initializer=init, input_shape=5, bits=4)
    with pytest.raises(ValueError, match="one-axis scales"):
        lq.CustomDenseLayer(units=3, orientation="groupwise", group_size=4, initializer=init, input_shape=5, bits=4, penalty_rate=1e-7)
    with pytest.raises(ValueError, match="memory order"):
        lq.CustomConv2DLayer(filters=4, orientation="groupwise", group_size=8, initializer=init, input_shape=2, bits=4,
                             kernel_storage="hwio")
    with pytest.raises(ValueError, match="memory order"):
        lq.CustomConv2DLayerNoBias(filters=4, orientation="groupwise", group_size=8, initializer=init, input_shape=2, bits=4,
                                   kernel_storage="hwio")


def test_layers_and_models_carry_the_group_size():
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=3)
    d = lq.CustomDenseLayer(units=6, orientation="groupwise", group_size=4, initializer=init, input_shape=10, scale_gradient="ste", bits=4)
    assert d.group_size == d.nested_q_w_layer.group_size == 4 and d.nested_q_b_layer.group_size is None
    assert tuple(d.nested_q_w_layer.scale.shape) == (3, 6) and tuple(d.nested_q_b_layer.scale.shape) == (1,)
    assert "group_size=4" in repr(d) and d.nested_q_w_layer.scale_name == "Groupwise-scaler"
    c = lq.CustomConv2DLayer(filters=8, orientation="groupwise", group_size=16, initializer=init, input_shape=5, bits=4,
                             scale_gradient="ste", grad_scale="rsqrt_group")
    assert tuple(c.nested_q_k_layer.scale.shape) == (8, 3) and tuple(c.nested_q_b_layer.scale.shape) == (1,)      # 45 = 2.8 * 16
    assert c.nested_q_k_layer.grad_scale_value(c.kernel.numel()) == 1.0 / np.sqrt(360 / 24)
    k = c.kernel
    assert group_geometry(k.shape, k.stride(), c.nested_q_k_layer.scale.shape, 16) == (8, 45, 1)
    plain = lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, bits=4)
    assert plain.group_size is None and "group_size" not in repr(plain)
    for config, gs in (("mnist", 64), ("cifar", 128)):
        lq.reset_layer_names()
        m = lq.build_model(config, seed=1, mode="ste", value=0.0, bits=4, group_size=gs)
        layers = lq.custom_layers_of(m)
        assert layers
        for layer in layers:
            conv = hasattr(layer, "nested_q_k_layer")
            nested = layer.nested_q_k_layer if conv else layer.nested_q_w_layer
            param = layer.kernel if conv else layer.W
            assert layer.group_size == nested.group_size == gs and nested.orientation == "groupwise" and layer.q_range == (-8, 7)
            assert tuple(nested.scale.shape) == groupwise_scale_shape(param.shape, gs)
            assert group_geometry(param.shape, param.stride(), nested.scale.shape, gs)[2] == (1 if conv else 0)
            assert layer.nested_q_b_layer.orientation == "scalar" and tuple(layer.nested_q_b_layer.scale.shape) == (1,)
            assert getattr(nested.scale, "lq_is_scale", False)
    lq.reset_layer_names()
    assert all(l.group_size is None for l in lq.custom_layers_of(lq.build_model("mnist", mode="ste", value=0.0, bits=4)))


def test_the_harness_refuses_with_the_reason():
    from learned_quantization_amd.train import Trainer, build_parser
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="needs bits"):
        lq.build_model("mnist", mode="ste", value=0.0, group_size=64)
    with pytest.raises(ValueError, match="needs bits"):
        Trainer("mnist", "ste", 0.0, device=cpu, group_size=64)
    for mode, value, loss in (("cl", 1e-7, "maxbin"), ("stecl", 1e-7, "difference")):
        with pytest.raises(ValueError, match="penalty kernels broadcast one-axis scales"):
            lq.build_model("mnist", mode=mode, value=value, bits=4, group_size=64)
        with pytest.raises(ValueError, match="penalty kernels broadcast one-axis scales"):
            Trainer("mnist", mode, value, "rowwise", loss, device=cpu, bits=4, group_size=64)
    with pytest.raises(ValueError, match="group_size with mode 'nq'"):
        lq.build_model("mnist", mode="nq", value=1e-11, bits=4, group_size=64)
    with pytest.raises(ValueError, match="multi-tensor batch"):
        Trainer("mnist", "ste", 0.0, device=cpu, bits=4, group_size=64, batched=True)
    with pytest.raises(ValueError, match="multi-tensor batch"):
        Trainer("mnist", "ste", 0.0, device=cpu, bits=4, group_size=64, batched=True, clipped_batch=True)
    with pytest.raises(ValueError, match="ddp_mode 'B'"):
        Trainer("mnist", "ste", 0.0, device=cpu, bits=4, group_size=64, ddp_mode="B")
    with pytest.raises(ValueError, match="memory order"):
        lq.build_model("cifar", mode="ste", value=0.0, bits=4, group_size=128, kernel_storage="hwio")
    assert build_parser().parse_args(["--bits", "4", "--mode", "ste", "--group-size", "64"]).group_size == 64
    assert build_parser().parse_args([]).group_size is None
    from learned_quantization_amd.experiment import build_parser as experiment_parser
    args = experiment_parser().parse_args(["--seed", "1", "--orientation", "rowwise", "--training", "from_scratch", "--group-size", "32"])
    assert args.group_size == 32
