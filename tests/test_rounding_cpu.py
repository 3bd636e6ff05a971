"""CPU tests of round-to-nearest for the clipped b-bit quantizer: the C-ABI surface and its validation without a launch, the
``rounding`` argument on every Python surface, and the NumPy reference itself pinned on a hand-written table (no GPU here)."""
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
from _rne_reference import bits_equal, floor_integers, rne_reference, tie_table      # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("lq_fq_forward_clip_r", "lq_fq_backward_clip_r")
LQ_EINVAL = -1
CPU = torch.device("cpu")


def _err():
    return _hip.load().lq_last_error().decode()


# ---------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_are_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                                       # additions only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/lq_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.SIGNATURES, f"{name} is not in the binding table"
    assert re.search(r"LQ_ROUND_FLOOR\s*=\s*0\s*,\s*LQ_ROUND_NEAREST_EVEN\s*=\s*1", header)
    assert ops.ROUNDINGS == ("floor", "nearest")


def test_a_bad_rounding_is_refused_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    p16 = (p + 15) // 16 * 16
    need = lib.lq_workspace_bytes(1, 3, 100)
    fwd, bwd = lib.lq_fq_forward_clip_r, lib.lq_fq_backward_clip_r
    for bad in (2, -1, 7):
        assert fwd(p, p, p, None, 0, -8, 7, bad, 1, 3, 100, None) == LQ_EINVAL and f"bad rounding {bad}" in _err()
        assert _err().startswith("lq_fq_forward_clip_r:")
        assert bwd(p, p, p, -8, 7, bad, 1.0, p, p, p, p16, need, 1, 3, 100, None) == LQ_EINVAL and f"bad rounding {bad}" in _err()
        assert _err().startswith("lq_fq_backward_clip_r:")
    # the floor pair's validation holds for either rounding
    for rnd in (0, 1):
        assert fwd(None, p, p, None, 0, -8, 7, rnd, 1, 3, 100, None) == LQ_EINVAL and "'P' is NULL" in _err()
        assert fwd(p, p, p, None, 0, 8, 7, rnd, 1, 3, 100, None) == LQ_EINVAL and "qmin 8 > qmax 7" in _err()
        assert fwd(p, p, p, p, 0, -8, 7, rnd, 1, 3, 100, None) == LQ_EINVAL and "q and q_dtype disagree" in _err()
        assert fwd(p, p, p, None, 0, -8, 7, rnd, 1, 0, 100, None) == LQ_EINVAL and "extents must be positive" in _err()
        assert bwd(p, p, p, -8, 7, rnd, 1.0, None, p, p, p16, need, 1, 3, 100, None) == LQ_EINVAL and "'dP' is NULL" in _err()
        assert bwd(p, p, p, 0, (1 << 24) + 1, rnd, 1.0, p, p, p, p16, need, 1, 3, 100, None) == LQ_EINVAL and "outside +-2^24" in _err()
        assert bwd(p, p, p, -8, 7, rnd, 1.0, p, p, p, None, 0, 1, 3, 100, None) == LQ_EINVAL and "workspace is NULL" in _err()
        assert bwd(p, p, p, -8, 7, rnd, 1.0, p, None, None, p16, need - 1, 1, 3, 100, None) == LQ_EINVAL and "too small" in _err()


def test_header_states_the_definition():
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    doc = header[header.index("the clipped pair with a choice of rounding"):header.index("int lq_fq_forward_clip_r")]
    for needle in ("rintf(t)", "round half to even", "[-1/2, 1/2]", "-0.0", "LQ_EINVAL", "LQ_ROUND_FLOOR runs exactly"):
        assert needle in doc, needle


# ---------------------------------------------------------------------------------------------- argument errors, four surfaces
def test_nearest_without_a_range_is_refused_everywhere():
    from learned_quantization_amd.train import Trainer
    P, s = torch.zeros(4, 4), torch.ones(1, 4)
    init = lq.RandomNormal(seed=1)
    need = "rounding='nearest' needs bits or q_range"
    with pytest.raises(ValueError, match=need):
        ops.my_custom_gradient(P, s, rounding="nearest")
    with pytest.raises(ValueError, match=need):
        ops.my_custom_gradient(P, s, 1e-11, rounding="nearest")
    with pytest.raises(ValueError, match=need):
        ops.my_custom_gradient(P, s, scale_gradient="ste", rounding="nearest")
    with pytest.raises(ValueError, match=need):
        lq.CustomQuantizedScaleLayer(rounding="nearest")
    with pytest.raises(ValueError, match=need):
        lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, rounding="nearest")
    with pytest.raises(ValueError, match=need):
        lq.CustomConv2DLayer(filters=4, initializer=init, input_shape=2, rounding="nearest")
    with pytest.raises(ValueError, match=need):
        lq.CustomConv2DLayerNoBias(filters=4, initializer=init, input_shape=2, rounding="nearest")
    with pytest.raises(ValueError, match=need):
        lq.build_model("mnist", mode="ste", value=0.0, rounding="nearest")
    with pytest.raises(ValueError, match=need):
        Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, rounding="nearest")


def test_an_unknown_rounding_is_refused_everywhere():
    from learned_quantization_amd.train import Trainer
    P, s = torch.zeros(4, 4), torch.ones(1, 4)
    init = lq.RandomNormal(seed=1)
    bad = "rounding must be one of"
    for value in ("round", "stochastic", None, 1):
        with pytest.raises(ValueError, match=bad):
            ops.my_custom_gradient(P, s, q_range=(-8, 7), rounding=value)
        with pytest.raises(ValueError, match=bad):
            ops.my_custom_gradient(P, s, rounding=value)
        with pytest.raises(ValueError, match=bad):
            lq.CustomQuantizedScaleLayer(bits=4, rounding=value)
        with pytest.raises(ValueError, match=bad):
            lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, bits=4, rounding=value)
        with pytest.raises(ValueError, match=bad):
            lq.CustomConv2DLayer(filters=4, initializer=init, input_shape=2, bits=4, rounding=value)
        with pytest.raises(ValueError, match=bad):
            lq.CustomConv2DLayerNoBias(filters=4, initializer=init, input_shape=2, bits=4, rounding=value)
        with pytest.raises(ValueError, match=bad):
            lq.build_model("mnist", mode="ste", value=0.0, bits=4, rounding=value)
        with pytest.raises(ValueError, match=bad):
            Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, bits=4, rounding=value)
    # the raw wrappers check it before they touch a tensor
    with pytest.raises(ValueError, match=bad):
        ops.fq_forward_clip(P, s, -8, 7, rounding="up")
    with pytest.raises(ValueError, match=bad):
        ops.fq_backward_clip(P, s, P, -8, 7, rounding="up")


def test_the_range_rules_still_apply_to_a_nearest_layer():
    from learned_quantization_amd.train import Trainer
    P, s = torch.zeros(4, 4), torch.ones(1, 4)
    with pytest.raises(ValueError, match="unclipped"):
        ops.my_custom_gradient(P, s, 1e-11, q_range=(-8, 7), rounding="nearest")
    with pytest.raises(ValueError, match="defer_scale_grad"):
        ops.my_custom_gradient(P, s, q_range=(-8, 7), rounding="nearest", defer_scale_grad=True)
    with pytest.raises(ValueError, match="unclipped"):
        lq.build_model("mnist", mode="nq", value=1e-11, bits=4, rounding="nearest")
    with pytest.raises(ValueError, match="masked copy"):
        Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, batched=True, bits=4, rounding="nearest")
    with pytest.raises(ValueError, match="clipped elements"):
        Trainer("mnist", "cl", 1e-7, "rowwise", "maxbin", device=CPU, ddp_mode="B", bits=4, rounding="nearest")


# ---------------------------------------------------------------------------------------------- plumbing and repr
def test_layers_and_models_carry_the_rounding_and_repr_names_it_only_for_nearest():
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=3)
    d = lq.CustomDenseLayer(units=3, orientation="columnwise", initializer=init, input_shape=5, scale_gradient="ste", bits=4,
                            rounding="nearest")
    assert d.rounding == d.nested_q_w_layer.rounding == d.nested_q_b_layer.rounding == "nearest"
    assert "rounding='nearest'" in d.nested_q_w_layer.extra_repr() and "rounding='nearest'" in d.extra_repr()
    assert "rounding='nearest'" in repr(d)
    c = lq.CustomConv2DLayer(filters=4, initializer=init, input_shape=2, bits=4, signed=False, penalty_rate=1e-7, rounding="nearest")
    assert c.rounding == c.nested_q_k_layer.rounding == c.nested_q_b_layer.rounding == "nearest" and "rounding='nearest'" in repr(c)
    nb = lq.CustomConv2DLayerNoBias(filters=4, initializer=init, input_shape=2, q_range=(-3, 5), rounding="nearest")
    assert nb.nested_q_k_layer.rounding == "nearest" and "rounding='nearest'" in repr(nb)
    n = lq.CustomQuantizedScaleLayer(q_range=(-2 ** 24, 2 ** 24), rounding="nearest")       # the unbounded nearest quantizer
    assert n.rounding == "nearest" and "rounding='nearest'" in n.extra_repr()
    for floor_layer in (lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, bits=4),
                        lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, bits=4, rounding="floor"),
                        lq.CustomConv2DLayer(filters=4, initializer=init, input_shape=2, bits=4),
                        lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, penalty_threshold=1e-11),
                        lq.CustomQuantizedScaleLayer(bits=4), lq.CustomQuantizedScaleLayer()):
        assert floor_layer.rounding == "floor" and "rounding" not in repr(floor_layer)
    for config, kw in (("mnist", dict(mode="ste", value=0.0, bits=4)), ("cifar", dict(mode="stecl", value=1e-7, bits=8)),
                       ("mnist", dict(mode="cl", value=1e-7, q_range=(0, 15)))):
        for rounding in ("nearest", "floor"):
            lq.reset_layer_names()
            m = lq.build_model(config, seed=1, rounding=rounding, **kw)
            layers = lq.custom_layers_of(m)
            assert layers
            for layer in layers:
                assert layer.rounding == rounding
                for a in ("nested_q_w_layer", "nested_q_k_layer", "nested_q_b_layer"):
                    if hasattr(layer, a):
                        assert getattr(layer, a).rounding == rounding
            assert ("rounding='nearest'" in repr(m)) == (rounding == "nearest")
    lq.reset_layer_names()
    assert all(l.rounding == "floor" for l in lq.custom_layers_of(lq.build_model("mnist", mode="ste", value=0.0)))


class _Reached(Exception):
    pass


@pytest.mark.parametrize("which", ["train", "experiment"])
def test_the_command_lines_take_rounding(which, monkeypatch, tmp_path, capsys):
    """``main`` of both drivers, run up to the point where it builds its Trainer (replaced by a recorder; the GPU checks before it
    are answered for it): --rounding reaches Trainer(rounding=), defaults to "floor", and the parser refuses anything else."""
    import importlib
    mod = importlib.import_module(f"learned_quantization_amd.{which}")
    seen = {}

    def recorder(*args, **kwargs):
        seen.clear()
        seen.update(kwargs)
        raise _Reached()

    monkeypatch.setattr(mod, "Trainer", recorder)
    monkeypatch.setattr(mod.torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(mod.torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if which == "train":
        base = ["--config", "mnist", "--mode", "ste", "--bits", "4"]
    else:
        base = ["--config", "mnist", "--seed", "1", "--orientation", "rowwise", "--training", "from_scratch", "--scale-gradient", "ste",
                "--bits", "4", "--log-root", str(tmp_path)]
    with pytest.raises(_Reached):
        mod.main(base + ["--rounding", "nearest"])
    assert seen["rounding"] == "nearest" and seen["bits"] == 4
    with pytest.raises(_Reached):
        mod.main(base + ["--rounding", "floor"])
    assert seen["rounding"] == "floor"
    with pytest.raises(_Reached):
        mod.main(base)
    assert seen["rounding"] == "floor"
    with pytest.raises(SystemExit) as e:
        mod.main(base + ["--rounding", "up"])
    assert e.value.code == 2 and "--rounding" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------- the NumPy reference, pinned
def test_reference_on_the_hand_written_table():
    """The issue's table at s = 1 and (-8, 7): ties go to the even neighbour, so 7.5 is clipped and -8.5 is not."""
    rows = [(-8.5, -8, True), (-7.5, -8, True), (-0.5, -0.0, True), (0.5, 0, True), (1.5, 2, True), (2.5, 2, True),
            (6.5, 6, True), (7.49, 7, True), (7.5, 8, False), (-8.51, -9, False)]
    t = np.array([r[0] for r in rows], np.float32)
    q0_want = np.array([r[1] for r in rows], np.float32)
    inside_want = np.array([r[2] for r in rows], bool)
    dy = np.arange(1, t.size + 1, dtype=np.float32)
    for s in (np.float32(1.0), np.float32(2.0 ** -7)):
        P = t * s
        assert np.array_equal(P / s, t)                                       # the quotients are exact
        ref = rne_reference(P, np.array([s], np.float32), dy, -8, 7)
        assert np.array_equal(ref["q0"], q0_want)
        assert np.array_equal(ref["inside"], inside_want)
        assert np.array_equal(ref["q"], np.clip(q0_want, -8, 7))
        assert np.signbit(ref["q0"][2]) and np.signbit(ref["out"][2]) and ref["out"][2] == 0.0      # rint(-0.5) = -0, out = -0 * s
        assert not np.signbit(ref["q0"][3])
        assert bits_equal(ref["dP"], np.where(inside_want, dy, np.float32(0.0)))
        assert not np.any(np.signbit(ref["dP"][~inside_want]))                # +0, not -0
        assert int(ref["clipped"][0]) == 2
        r = np.where(inside_want, q0_want - t, np.clip(q0_want, -8, 7)).astype(np.float64)
        assert np.all(np.abs(r[inside_want]) <= 0.5)
        assert ref["ds"][0] == np.sum(dy.astype(np.float64) * r)
        assert ref["terms"][0] == np.sum(np.abs(dy.astype(np.float64) * r))
    # at (0, 15): -0.5 rounds to -0, which is inside (>= 0 holds for -0); 15.5 rounds to 16 and is clipped; 14.5 to 14
    ref = rne_reference(np.array([-0.5, -0.51, 14.5, 15.49, 15.5], np.float32), np.array([1.0], np.float32), np.ones(5, np.float32), 0, 15)
    assert list(ref["inside"]) == [True, False, True, True, False] and list(ref["q"]) == [0, 0, 14, 15, 15]


def test_reference_sign_of_out_and_the_residual():
    s = np.array([0.25], np.float32)
    ref = rne_reference(np.array([-0.3 * 0.25], np.float32), s, np.ones(1, np.float32), -8, 7)
    assert ref["q0"][0] == 0 and np.signbit(ref["q0"][0])
    assert ref["out"][0] == 0.0 and np.signbit(ref["out"][0])                 # out = -0.0 * s keeps the sign, as NumPy's does
    assert ref["q"].astype(np.int32)[0] == 0                                  # the integer outputs store 0
    rng = np.random.default_rng(11)
    P = rng.standard_normal(1 << 16).astype(np.float32) * np.float32(0.05)
    sv = np.array([0.05 / 4], np.float32)
    ref = rne_reference(P, sv, np.ones_like(P), -8, 7)
    r_in = ref["r"][ref["inside"]]
    assert r_in.size > 0.8 * P.size and r_in.min() >= -0.5 and r_in.max() <= 0.5
    assert abs(float(r_in.mean())) < 0.01                                     # centred, where floor's residual averages -1/2
    fl = floor_integers(P, sv, -8, 7)
    assert 0.3 < float((fl != ref["q"]).mean()) < 0.7


def test_reference_on_the_tie_table():
    for qmin, qmax in ((-8, 7), (0, 15)):
        t, q0_want = tie_table(qmin, qmax)
        ref = rne_reference(t, np.array([1.0], np.float32), np.ones_like(t), qmin, qmax)
        assert bits_equal(ref["q0"], q0_want)
        assert np.array_equal(ref["inside"], (q0_want >= qmin) & (q0_want <= qmax))


def test_reference_on_special_values():
    s = np.array([1.0], np.float32)
    big = np.float32(2.0 ** 23 + 1)
    P = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 3e38, -3e38, 1e-45, -1e-45, 2.5, big, -big], np.float32)
    dy = np.arange(1, P.size + 1, dtype=np.float32)
    ref = rne_reference(P, s, dy, -8, 7)
    q = ref["q"]
    assert q[0] == 7 and q[1] == -8 and np.isnan(q[2])                        # +-Inf saturates, NaN stays NaN
    assert q[3] == 0 and q[4] == 0 and np.signbit(q[4]) and not np.signbit(q[3])
    assert q[7] == 0 and q[8] == 0 and np.signbit(q[8]) and q[9] == 2         # -1e-45 rounds to -0 (floor gives -1)
    assert ref["q0"][10] == big and ref["q0"][11] == -big                     # |t| >= 2^23: q0 == t
    assert list(ref["inside"]) == [False, False, False, True, True, False, False, True, True, True, False, False]
    assert int(ref["clipped"][0]) == 7 and np.isnan(ref["ds"][0])
    wide = rne_reference(P[[10, 11]], s, dy[[10, 11]], -2 ** 24, 2 ** 24)
    assert list(wide["inside"]) == [True, True] and list(wide["r"]) == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------- the restore pre-image
def test_q_times_s_is_a_pre_image_below_2_to_the_22():
    """load_packed_parameters restores P = q * s for a nearest layer: rint(fl(fl(q * s) / s)) == q for |q| < 2^22 at every
    magnitude (IEEE float32 product and division: two roundings move the quotient by less than 1/2 there).  (q + 1/2) * s, the
    floor pre-image, is a tie under rint and does not come back."""
    rng = np.random.default_rng(5)
    for top in (8, 128, 1 << 12, 1 << 16, 1 << 20, (1 << 22) - 1):
        q = rng.integers(-top, top + 1, 200000).astype(np.float32)
        s = np.exp(rng.uniform(np.log(1e-8), np.log(1e3), q.size)).astype(np.float32)
        P = q * s
        assert P.dtype == np.float32
        back = np.rint(P / s)
        assert np.array_equal(back, q), f"|q| <= {top}: {(back != q).sum()} misses"
    q = np.arange(-8, 8, dtype=np.float32)
    s = np.float32(0.0125)
    tie = (q + np.float32(0.5)) * s
    assert np.any(np.rint(tie / s) != q)                                      # the floor pre-image misses under rint
    assert np.array_equal(np.floor(tie / s), q)
