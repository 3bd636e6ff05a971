"""CPU tests of the asymmetric group-wise quantizer: the NumPy reference (tests/_group_affine_reference.py) on a hand-written table
and against tests/_group_reference.py at b = 0, the conditions on the inputs of tests/test_gpu_group_affine.py, min-max
initialisation on the reference, the refusals of the Python surface and the argument checks of the three C entry points.  No
test here needs a device: every C call below fails in validation, before any launch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, ops

sys.path.insert(0, os.path.dirname(__file__))
from _bounds import stable_seed                                                                   # noqa: E402
from _clip_reference import bits_equal                                                            # noqa: E402
from _group_affine_reference import (edge_affine_case, group_affine_reference, make_affine_case,   # noqa: E402
                                     minmax_center, minmax_reference)
from _group_forms import LARGE, VARIANTS, WINDOW_SHAPES, form_variants                            # noqa: E402
from _group_reference import check_condition, expand_scale, group_reference, make_case            # noqa: E402
from _scale_init_reference import GEOMETRIES, RANGES, ROUNDINGS, make_input                       # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("lq_fq_forward_group_affine", "lq_fq_backward_group_affine", "lq_scale_init_group_minmax")
LQ_EINVAL, LQ_EALIGN = -1, -4
LIM = 1 << 24


def _err():
    return _hip.load().lq_last_error().decode()


# ------------------------------------------------------------------------------------------------------- the reference, pinned
# quotients of a 4 x 2 matrix, range [-2, 1], groups of two rows; scales are powers of two and offsets multiples of the scale, so
# P = t * s + b is exact and (P - b) / s gives t back
T = np.array([[0.5, -1.25], [-2.0, 2.5], [1.5, -3.0], [-0.5, 0.75]], np.float32)
DY = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], np.float32)
S = np.array([[0.5, 1.0], [2.0, 0.25]], np.float32)
B = np.array([[1.0, -3.0], [4.0, 0.5]], np.float32)
Q_FLOOR = np.array([[0, -2], [-2, 1], [1, -2], [-1, 0]], np.float32)
INSIDE_FLOOR = np.array([[1, 1], [1, 0], [1, 0], [1, 1]], bool)


def test_reference_on_the_hand_written_table():
    sb, bb = expand_scale(S, 4, 2, 0, 2), expand_scale(B, 4, 2, 0, 2)
    P = T * sb + bb
    ref = group_affine_reference(P, S, B, DY, -2, 1, axis=0, gs=2)
    assert np.array_equal(ref["t"], T) and np.array_equal(ref["q"], Q_FLOOR) and np.array_equal(ref["inside"], INSIDE_FLOOR)
    assert bits_equal(ref["out"], np.array([[1.0, -5.0], [0.0, -2.0], [6.0, 0.0], [2.0, 0.5]], np.float32))
    assert bits_equal(ref["dP"], np.array([[1, 2], [3, 0], [5, 0], [7, 8]], np.float32))
    assert np.array_equal(ref["ds"], [[-0.5, 2.5], [-6.0, -18.0]])           # dy * r: -0.5 -1.5 | 0 4 | -2.5 -12 | -3.5 -6
    assert np.array_equal(ref["terms"], [[0.5, 5.5], [6.0, 18.0]])
    assert np.array_equal(ref["db"], [[0.0, 4.0], [0.0, 6.0]])               # dy of the two clipped elements
    assert np.array_equal(ref["clipped"], [[0, 1], [0, 1]])
    scaled = group_affine_reference(P, S, B, DY, -2, 1, axis=0, gs=2, k=0.5, kb=0.25)
    assert np.array_equal(scaled["ds"], ref["ds"] * 0.5) and np.array_equal(scaled["db"], ref["db"] * 0.25)
    near = group_affine_reference(P, S, B, DY, -2, 1, axis=0, gs=2, rounding="nearest")
    assert np.array_equal(near["q0"], [[0, -1], [-2, 2], [2, -3], [-0.0, 1]])      # ties to even: 0.5 -> 0, 2.5 -> 2, 1.5 -> 2
    assert np.array_equal(near["clipped"], [[0, 1], [1, 1]]) and np.array_equal(near["db"], [[0.0, 4.0], [5.0, 6.0]])


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("geom", [(37, 5, 0, 8), (7, 27, 1, 8), (64, 60, 1, 16)], ids=str)
def test_zero_offset_reduces_to_the_symmetric_reference(geom, rounding):
    P, s, dy = make_case(stable_seed("affine b0", *geom), *geom)
    sym = group_reference(P, s, dy, -8, 7, geom[2], geom[3], k=0.75, rounding=rounding)
    ref = group_affine_reference(P, s, np.zeros_like(s), dy, -8, 7, geom[2], geom[3], k=0.75, kb=0.75, rounding=rounding)
    for key in ("q", "dP", "t", "q0", "r"):
        assert bits_equal(ref[key], sym[key]), key
    assert np.array_equal(ref["ds"], sym["ds"]) and np.array_equal(ref["clipped"], sym["clipped"])
    assert np.array_equal(ref["out"], sym["out"]) and not np.signbit(ref["out"][ref["out"] == 0]).any()      # -0 comes back as +0
    assert np.signbit(sym["out"]).any()


# ------------------------------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("case,variant", [cv for cv in form_variants() if cv[0] != LARGE], ids=str)
def test_the_cases_clip_and_keep(case, variant):
    """check_condition's rule on every case the GPU file runs (it asserts the large one itself): at least 10 % clipped and 10 %
    inside, overall and in at least 90 % of the groups of 8 or more elements."""
    (qmin, qmax), rounding = VARIANTS[variant]
    P, s, b, dy = make_affine_case(stable_seed("affineforms", *case), *case)
    ref = group_affine_reference(P, s, b, dy, qmin, qmax, case[2], case[3], rounding=rounding)
    check_condition(ref, *case, f"{case} {variant}")
    assert np.abs(ref["db"]).max() > 0 and np.abs(b).max() > 0


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("range_", [(-8, 7), (0, 15)], ids=str)
def test_edge_cases_sit_on_the_edges(range_, rounding):
    qmin, qmax = range_
    for case in WINDOW_SHAPES:
        P, s, b, dy, want_q0 = edge_affine_case(stable_seed("affine edge", case), *case, qmin, qmax, rounding)
        ref = group_affine_reference(P, s, b, dy, qmin, qmax, case[2], case[3], rounding=rounding)
        assert np.array_equal(ref["q0"], want_q0)
        seen = set(np.unique(ref["t"] - np.float32(qmin)).tolist())
        assert {0.0, float(qmax - qmin), float(qmax - qmin + 1), -0.5, float(qmax - qmin) + 0.5} <= seen
        assert 0 < int(ref["clipped"].sum()) < P.size


# ------------------------------------------------------------------------------------------------------- min-max
def _clipped_after_minmax(P, qmin, qmax, axis, gs, rounding):
    mm = minmax_reference(P, qmin, qmax, axis, gs, rounding=rounding)
    gs = min(gs, P.shape[axis])
    ref = group_affine_reference(P, mm["s"], mm["b"], np.zeros_like(P), qmin, qmax, axis, gs, rounding=rounding)
    return mm, ref


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("geom", [g for g in GEOMETRIES if g[0] * g[1] <= 200000], ids=str)
def test_minmax_leaves_nothing_clipped(geom, rounding):
    R, C, axis, gs = geom
    base = make_input(R, C, axis, gs)
    for qmin, qmax in RANGES:
        for name, P in (("centred", base), ("shifted", (base + np.float32(0.5)).astype(np.float32)), ("one-sided", np.abs(base))):
            mm, ref = _clipped_after_minmax(P, qmin, qmax, axis, gs, rounding)
            assert not mm["bad"].any() and int(ref["clipped"].sum()) == 0, f"{geom} [{qmin}, {qmax}] {rounding} {name}"
            q = ref["q"]
            assert q.min() >= qmin and q.max() <= qmax


def test_minmax_special_groups():
    P = np.array(make_input(7, 27, 1, 8))
    P[0, 3], P[1, 9], P[2, 17] = np.nan, np.inf, -np.inf
    P[3, 0:8] = np.float32(0.25)
    P[4, 8:16] = np.float32(0.0)
    mm = minmax_reference(P, -8, 7, 1, 8, rounding="floor")
    bad = np.zeros((7, 4), bool)
    bad[0, 0] = bad[1, 1] = bad[2, 2] = True
    assert np.array_equal(mm["bad"], bad) and np.array_equal(np.isnan(mm["s"]), bad) and np.array_equal(np.isnan(mm["b"]), bad)
    mv = np.float32(ops.SCALE_INIT)
    assert mm["s"][3, 0] == mv and mm["b"][3, 0] == np.float32(0.25) - minmax_center(-8, 7, "floor") * mv
    assert mm["s"][4, 1] == mv and mm["b"][4, 1] == np.float32(0.0) - minmax_center(-8, 7, "floor") * mv
    assert minmax_center(-8, 7, "floor") == 0.0 and minmax_center(-8, 7, "nearest") == -0.5 and minmax_center(0, 15, "floor") == 8.0


# ------------------------------------------------------------------------------------------------------- refusals
def test_the_op_refuses_with_the_reason():
    p, s = torch.zeros(8, 4), torch.ones(2, 4)      # CPU tensors: a call that got past the checks would raise RuntimeError instead
    b = torch.zeros(2, 4)
    with pytest.raises(ValueError, match="group_size of the line length or more gives per-channel offsets"):
        lq.my_custom_gradient(p, s, q_range=(-8, 7), scale_gradient="ste", offset=b)
    with pytest.raises(ValueError, match="offset needs a q_range"):
        lq.my_custom_gradient(p, s, scale_gradient="ste", group_size=4, offset=b)
    with pytest.raises(ValueError, match="nested-quantization vote"):
        lq.my_custom_gradient(p, s, 1e-3, q_range=(-8, 7), group_size=4, offset=b)
    with pytest.raises(ValueError, match="loss-term-only rule has no gradient for an offset"):
        lq.my_custom_gradient(p, s, q_range=(-8, 7), group_size=4, offset=b)
    with pytest.raises(ValueError, match="has one"):
        lq.scale_init_group_minmax(p, s, b, 3, 3, 4)
    with pytest.raises(ValueError, match=r"outside \+-2\^22"):
        lq.scale_init_group_minmax(p, s, b, 0, (1 << 22) + 1, 4)
    with pytest.raises(ValueError, match="rounding"):
        lq.scale_init_group_minmax(p, s, b, -8, 7, 4, rounding="up")
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # past the checks: the device requirement
        lq.fq_forward_group_affine(p, s, b, -8, 7, 4)


def test_the_layers_refuse_with_the_reason():
    init = lq.RandomNormal(seed=1)
    ok = dict(units=3, initializer=init, input_shape=8, scale_gradient="ste", bits=4, orientation="groupwise", group_size=4, asymmetric=True)
    lq.reset_layer_names()
    layer = lq.CustomDenseLayer(**ok)                       # builds on the CPU; only a call needs the device
    nested = layer.nested_q_w_layer
    assert layer.asymmetric and nested.asymmetric and tuple(nested.offset.shape) == tuple(nested.scale.shape) == (2, 3)
    assert bool((nested.offset == 0).all()) and nested.offset.lq_is_scale and nested.offset.lq_is_offset
    assert not hasattr(nested.offset, "lq_constraint") and hasattr(nested.scale, "lq_constraint")
    assert layer.nested_q_b_layer.offset is None and not layer.nested_q_b_layer.asymmetric      # biases stay symmetric and scalar
    assert [id(p) for p in lq.scale_parameters(layer)] == [id(nested.scale), id(nested.offset), id(layer.nested_q_b_layer.scale)]
    assert "asymmetric=True" in repr(layer)
    for cls, kw in ((lq.CustomDenseLayer, ok), (lq.CustomConv2DLayer, {**ok, "units": None, "filters": 3}),
                    (lq.CustomConv2DLayerNoBias, {**ok, "units": None, "filters": 3})):
        kw = {k: v for k, v in kw.items() if v is not None}
        for orientation in ("rowwise", "scalar"):
            with pytest.raises(ValueError, match="group_size of the line length or more gives per-channel offsets"):
                cls(**{**kw, "orientation": orientation, "group_size": None})
        with pytest.raises(ValueError, match="asymmetric=True needs bits or q_range"):
            cls(**{**kw, "bits": None})
        with pytest.raises(ValueError, match="penalty_threshold"):
            cls(**{**kw, "penalty_threshold": 1e-3, "scale_gradient": None})
        with pytest.raises(ValueError, match="loss term"):
            cls(**{**kw, "penalty_rate": 1e-7})
        with pytest.raises(ValueError, match="no gradient for an offset"):
            cls(**{**kw, "scale_gradient": None})
    with pytest.raises(ValueError, match="hwio"):
        lq.CustomConv2DLayer(**{**{k: v for k, v in ok.items() if k != "units"}, "filters": 3, "kernel_storage": "hwio"})
    with pytest.raises(ValueError, match="per-channel offsets"):
        lq.CustomQuantizedScaleLayer(orientation="rowwise", bits=4, scale_gradient="ste", asymmetric=True)
    # scale initialisation
    sym = lq.CustomDenseLayer(**{**ok, "asymmetric": False})
    with pytest.raises(ValueError, match='"minmax" on a symmetric layer'):
        sym.init_scales("minmax")
    with pytest.raises(ValueError, match='"minmax" on a symmetric layer'):
        sym.nested_q_w_layer.init_scale(sym.W, "minmax")
    with pytest.raises(ValueError, match='"minmax" on a symmetric layer'):
        lq.init_scales(torch.nn.Sequential(layer, sym), "minmax")
    one = lq.CustomDenseLayer(**{**ok, "bits": None, "q_range": (3, 3)})
    with pytest.raises(ValueError, match="has one"):
        one.init_scales("minmax")
    with pytest.raises(ValueError, match="scale_init must be one of"):
        layer.init_scales("max")
    for method in ("minmax", "absmax"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # past the checks
            layer.init_scales(method)
    # data-parallel mode B sets defer_scale_grad on nested-quantization layers only; an asymmetric layer refuses it outright
    nested.defer_scale_grad = True
    with pytest.raises(ValueError, match="mode B"):
        layer(torch.zeros(1, 8))
    nested.defer_scale_grad = False
    with pytest.raises(ValueError, match="mode 'B'"):
        lq.DataParallel(layer, mode="B")
    for kw in (dict(clipped=True), dict(group_batch=True), dict()):
        with pytest.raises(ValueError, match="asymmetric"):
            lq.FakeQuantBatch(torch.nn.Sequential(layer), **kw)


def test_the_models_and_the_harness_refuse_with_the_reason():
    from learned_quantization_amd.train import Trainer
    base = dict(mode="ste", value=0.0, bits=4, group_size=64, asymmetric=True)
    model = lq.build_model("mnist", **base)
    for layer in lq.custom_layers_of(model):
        assert layer.asymmetric and layer.weight_nested().offset is not None and layer.nested_q_b_layer.offset is None
    conv = lq.build_model("cifar", **{**base, "group_size": 128})
    assert all(layer.weight_nested().asymmetric for layer in lq.custom_layers_of(conv))
    for make in (lambda **kw: lq.build_model("mnist", **kw), lambda **kw: Trainer(config="mnist", device=torch.device("cpu"), **kw)):
        with pytest.raises(ValueError, match="per-channel offsets"):
            make(**{**base, "group_size": None})
        with pytest.raises(ValueError, match="asymmetric=True needs bits"):
            make(**{**base, "bits": None})
        for mode in ("cl", "stecl", "nqcl"):
            with pytest.raises(ValueError, match="loss-term"):
                make(**{**base, "mode": mode})
        with pytest.raises(ValueError, match="vote"):
            make(**{**base, "mode": "nq"})
        with pytest.raises(ValueError, match='"minmax" on a symmetric model'):
            make(**{**base, "asymmetric": False, "scale_init": "minmax"})
        with pytest.raises(ValueError, match="has one"):
            make(**{**base, "bits": None, "q_range": (5, 5), "scale_init": "minmax"})
        with pytest.raises(ValueError, match="hwio"):
            make(**{**base, "kernel_storage": "hwio"})
    for kw, why in ((dict(batched=True, group_batch=True), "batched=True"), (dict(batched=True, clipped_batch=True), "batched=True"),
                    (dict(ddp_mode="B"), "ddp_mode 'B'")):
        with pytest.raises(ValueError, match=why):
            Trainer(config="mnist", device=torch.device("cpu"), **base, **kw)


def test_the_drivers_parse_the_flags():
    import inspect
    from learned_quantization_amd.experiment import build_parser as experiment_parser
    from learned_quantization_amd.train import Trainer, build_parser
    line = ["--mode", "ste", "--bits", "4", "--group-size", "64", "--asymmetric", "--scale-init", "minmax"]
    args = build_parser().parse_args(line)
    assert args.asymmetric and args.scale_init == "minmax" and not build_parser().parse_args([]).asymmetric
    exp = ["--seed", "1", "--orientation", "scalar", "--training", "from_scratch", "--bits", "4", "--scale-gradient", "ste", "--group-size", "64"]
    args = experiment_parser().parse_args(exp + ["--asymmetric", "--scale-init", "minmax"])
    assert args.asymmetric and args.scale_init == "minmax" and not experiment_parser().parse_args(exp).asymmetric
    for parser, head in ((build_parser, ["--mode", "ste", "--bits", "4", "--group-size", "64"]), (experiment_parser, exp)):
        with pytest.raises(SystemExit):
            parser().parse_args(head + ["--scale-init", "minmax"])                  # a symmetric model
        with pytest.raises(SystemExit):
            parser().parse_args([a for a in head if a not in ("--group-size", "64")] + ["--asymmetric"])
    assert inspect.signature(Trainer.__init__).parameters["asymmetric"].default is False
    assert inspect.signature(lq.build_model).parameters["asymmetric"].default is False


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
    assert lq.fq_forward_group_affine is ops.fq_forward_group_affine and lq.fq_backward_group_affine is ops.fq_backward_group_affine
    assert lq.scale_init_group_minmax is ops.scale_init_group_minmax


def test_header_states_the_definition():
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    doc = header[header.index("asymmetric group-wise scales"):header.index("int lq_fq_forward_group_affine")]
    for needle in ("u  = P - b", "t  = u / s", "floorf(t) | rintf(t)", "out = (q * s) + b", "inside ? dy : +0.0f", "r  = inside ? q0 - t : q",
                   "(double)grad_scale", "(double)offset_grad_scale", "!inside_i", "clipped[g]", "mask only", "LQ_EINVAL", "LQ_EALIGN",
                   "bit-identical to lq_fq_backward_group", "-0.0 comes back as +0.0", "mn = min_i P_i", "(1 + 2^-22)", "0.5f*mn + 0.5f*mx",
                   "b   = RN(mid - RN(c * s))", "+-2^22", "s = b = NaN", "2 M / s + 4 |c| + n <= 2^22"):
        assert needle in doc, needle


def test_forward_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    fn = lib.lq_fq_forward_group_affine
    rng, geo = (-8, 7, 0), (5, 3, 0, 2, None)
    assert fn(None, p, p, p, None, 0, *rng, *geo) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fn(p, None, p, p, None, 0, *rng, *geo) == LQ_EINVAL and "'s' is NULL" in _err()
    assert fn(p, p, None, p, None, 0, *rng, *geo) == LQ_EINVAL and "'b' is NULL" in _err()
    assert fn(p, p, p, None, None, 0, *rng, *geo) == LQ_EINVAL and "'out' is NULL" in _err()
    assert fn(p, p, p, p, None, 0, 8, 7, 0, *geo) == LQ_EINVAL and "qmin 8 > qmax 7" in _err()
    assert fn(p, p, p, p, None, 0, -LIM - 1, 7, 0, *geo) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, p, p, None, 0, -8, LIM + 1, 0, *geo) == LQ_EINVAL and "outside +-2^24" in _err()
    for bad in (-1, 2):
        assert fn(p, p, p, p, None, 0, -8, 7, bad, *geo) == LQ_EINVAL and "bad rounding" in _err()
    for axis in (-1, 2):
        assert fn(p, p, p, p, None, 0, *rng, 5, 3, axis, 2, None) == LQ_EINVAL and "bad axis" in _err()
    for gs in (0, -3):
        assert fn(p, p, p, p, None, 0, *rng, 5, 3, 0, gs, None) == LQ_EINVAL and "group size" in _err()
    for R, C in ((0, 3), (5, 0), (-1, 3)):
        assert fn(p, p, p, p, None, 0, *rng, R, C, 0, 2, None) == LQ_EINVAL and "extents must be positive" in _err()
    assert fn(p, p, p, p, None, 0, *rng, 1 << 20, 1 << 11, 1, 2, None) == LQ_EINVAL and "not below 2^31" in _err()
    assert fn(p, p, p, p, p, 0, *rng, *geo) == LQ_EINVAL and "q and q_dtype disagree" in _err()
    assert fn(p, p, p, p, p, 9, *rng, *geo) == LQ_EINVAL and "bad q_dtype" in _err()
    for k in range(4):
        args = [p, p, p, p]
        args[k] = p + 2
        assert fn(*args, None, 0, *rng, *geo) == LQ_EALIGN and "not 4-byte aligned" in _err()


def test_backward_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    fn = lib.lq_fq_backward_group_affine
    mid, outs, tail = (-8, 7, 0, 1.0, 1.0), (p, p, p, p), (None, 0, 5, 3, 0, 2, None)
    for k, name in enumerate(("P", "s", "b", "dy")):
        args = [p, p, p, p]
        args[k] = None
        assert fn(*args, *mid, *outs, *tail) == LQ_EINVAL and f"'{name}' is NULL" in _err()
        args[k] = p + 2
        assert fn(*args, *mid, *outs, *tail) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert fn(p, p, p, p, *mid, None, p, p, p, *tail) == LQ_EINVAL and "'dP' is NULL" in _err()
    for k, name in ((1, "ds"), (2, "db"), (3, "clipped")):
        o = [p, p, p, p]
        o[k] = p + 1
        assert fn(p, p, p, p, *mid, *o, *tail) == LQ_EALIGN and f"{name} is not 4-byte aligned" in _err()
    assert fn(p, p, p, p, 1, 0, 0, 1.0, 1.0, *outs, *tail) == LQ_EINVAL and "qmin 1 > qmax 0" in _err()
    assert fn(p, p, p, p, -LIM - 1, 0, 0, 1.0, 1.0, *outs, *tail) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, p, p, -8, 7, 3, 1.0, 1.0, *outs, *tail) == LQ_EINVAL and "bad rounding" in _err()
    assert fn(p, p, p, p, *mid, *outs, None, 0, 5, 3, 2, 2, None) == LQ_EINVAL and "bad axis" in _err()
    assert fn(p, p, p, p, *mid, *outs, None, 0, 5, 3, 1, 0, None) == LQ_EINVAL and "group size" in _err()
    assert fn(p, p, p, p, *mid, *outs, None, 0, 0, 3, 1, 2, None) == LQ_EINVAL and "extents must be positive" in _err()
    assert fn(p, p, p, p, *mid, *outs, None, 0, 1 << 20, 1 << 11, 0, 2, None) == LQ_EINVAL and "not below 2^31" in _err()
    assert lib.lq_group_workspace_bytes(5, 3, 0, 2) == 0


def test_minmax_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    fn = lib.lq_scale_init_group_minmax
    mv, geo = float(ops.SCALE_INIT), (5, 3, 0, 2, None)
    for k, name in enumerate(("P", "s", "b")):
        args = [p, p, p]
        args[k] = None
        assert fn(*args, -8, 7, 0, mv, *geo) == LQ_EINVAL and f"'{name}' is NULL" in _err()
        args[k] = p + 2
        assert fn(*args, -8, 7, 0, mv, *geo) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert fn(p, p, p, 3, 3, 0, mv, *geo) == LQ_EINVAL and "qmax > qmin" in _err()
    assert fn(p, p, p, 4, 3, 0, mv, *geo) == LQ_EINVAL and "qmax > qmin" in _err()
    assert fn(p, p, p, -(1 << 22) - 1, 3, 0, mv, *geo) == LQ_EINVAL and "outside +-2^22" in _err()
    assert fn(p, p, p, 0, (1 << 22) + 1, 0, mv, *geo) == LQ_EINVAL and "outside +-2^22" in _err()
    assert fn(p, p, p, -8, 7, 2, mv, *geo) == LQ_EINVAL and "bad rounding" in _err()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert fn(p, p, p, -8, 7, 0, bad, *geo) == LQ_EINVAL and "min_value" in _err()
    assert fn(p, p, p, -8, 7, 0, mv, 5, 3, 2, 2, None) == LQ_EINVAL and "bad axis" in _err()
    assert fn(p, p, p, -8, 7, 0, mv, 5, 3, 0, 0, None) == LQ_EINVAL and "group size" in _err()
    assert fn(p, p, p, -8, 7, 0, mv, 0, 3, 0, 2, None) == LQ_EINVAL and "extents must be positive" in _err()
