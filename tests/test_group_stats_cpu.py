"""CPU tests of the per-group quantization statistics (include/lq_hip.h: lq_group_stats): the NumPy reference pinned on a
hand-written table, the C-ABI surface and its validation without a launch, ops.summarize_stats on hand-made records, the refusals
of the Python surface, and -- on the reference alone, over the inputs of tests/test_gpu_group_stats.py -- the conditions those GPU
tests rely on (no GPU here)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, layers, ops, tracking

sys.path.insert(0, os.path.dirname(__file__))
import _group_stats_reference as G                                                   # noqa: E402
import _scale_init_reference as S                                                    # noqa: E402
from _group_affine_reference import make_affine_case                                 # noqa: E402
from _group_reference import make_case                                                # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LQ_EINVAL, LQ_EALIGN = -1, -4
LIM = 1 << 24
SEED = 20


def _err():
    return _hip.load().lq_last_error().decode()


# ------------------------------------------------------------------------------------------------------- the reference, pinned
# twelve elements, 3 x 4, groups = rows (axis 1, gs = 4), range [-2, 1]; every value and every quotient is exact in float32
S34 = np.array([[0.5], [1.0], [0.25]], np.float32)
P34 = np.array([[0.25, -0.75, 1.5, -2.0],        # t = .5 -1.5  3 -4     floor  0 -2  3 -4    q  0 -2  1 -2    out  0  -1  .5  -1
                [0.5, 1.0, -0.5, -3.0],          # t = .5  1  -.5 -3     floor  0  1 -1 -3    q  0  1 -1 -2    out  0   1 -1  -2
                [0.0, 0.3125, -0.25, 1.0]],      # t =  0 1.25 -1  4     floor  0  1 -1  4    q  0  1 -1  1    out  0 .25 -.25 .25
               np.float32)
BELOW = np.array([[1], [1], [0]])
ABOVE = np.array([[1], [0], [1]])
ERR2 = np.array([[0.0625 + 0.0625 + 1.0 + 1.0], [0.25 + 0.0 + 0.25 + 1.0], [0.0 + 0.00390625 + 0.0 + 0.5625]])
SIG2 = np.array([[0.0625 + 0.5625 + 2.25 + 4.0], [0.25 + 1.0 + 0.25 + 9.0], [0.0 + 0.09765625 + 0.0625 + 1.0]])
HIST_FLOOR = np.array([3, 2, 3, 4])              # codes -2 -1 0 1
HIST_NEAREST = np.array([3, 1, 4, 4])            # rint(-.5) = -0: the second row's third element moves from -1 to 0, out = -0 either way


@pytest.mark.parametrize("rounding,hist", [("floor", HIST_FLOOR), ("nearest", HIST_NEAREST)])
def test_reference_on_a_hand_written_table(rounding, hist):
    ref = G.group_stats_reference(P34, S34, -2, 1, 1, 4, rounding=rounding)
    assert np.array_equal(ref["below"], BELOW) and np.array_equal(ref["above"], ABOVE)
    assert np.array_equal(ref["err2"], ERR2) and np.array_equal(ref["sig2"], SIG2)       # sums of a few dyadic numbers: exact
    assert np.array_equal(ref["hist"], hist) and ref["hist"].sum() == 12
    assert ref["below"].dtype == ref["above"].dtype == ref["hist"].dtype == np.int64
    # with an offset of 1 on data moved by 1 the codes, counts and errors are the same; the signal is the moved data's
    ref_b = G.group_stats_reference(P34 + np.float32(1.0), S34, -2, 1, 1, 4, b=np.ones_like(S34), rounding=rounding)
    for k in ("below", "above", "err2", "hist"):
        assert np.array_equal(ref_b[k], ref[k]), k
    assert np.array_equal(ref_b["sig2"], np.array([[8.875], [10.5], [7.28515625]]))


def test_reference_axis_0_ragged_and_non_finite():
    P = np.array([[1.0, -1.0], [3.0, 0.5], [-9.0, np.nan], [np.inf, 0.25]], np.float32)      # gs = 3 along R: groups of 3 and 1 rows
    s = np.ones((2, 2), np.float32)
    ref = G.group_stats_reference(P, s, -2, 1, 0, 3)
    assert np.array_equal(ref["below"], [[1, 0], [0, 0]]) and np.array_equal(ref["above"], [[1, 0], [1, 0]])
    assert ref["err2"][0, 0] == 0.0 + 4.0 + 49.0 and np.isnan(ref["err2"][0, 1]) and np.isinf(ref["err2"][1, 0])
    assert ref["err2"][1, 1] == 0.0625 and ref["hist"].sum() == 7                           # the NaN is not binned, the Inf saturates
    assert G.close(ref["err2"], ref["err2"]) and not G.close(ref["err2"] * (1 + 2.0 ** -29), ref["err2"])


# ------------------------------------------------------------------------------- what the GPU cases rely on, on the reference alone
@pytest.mark.parametrize("geo", G.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_conditions_of_the_gpu_cases(geo):
    R, C, axis, gs = geo
    P, s, _ = make_case(SEED, *geo)
    n = R * C
    for qmin, qmax, rounding in G.RANGES:
        ref = G.group_stats_reference(P, s, qmin, qmax, axis, gs, rounding=rounding)
        below, above = int(ref["below"].sum()), int(ref["above"].sum())
        if qmin == 0:
            assert below >= 0.4 * n and above >= 0.01 * n, (geo, qmin, below, above)
        else:
            assert below >= 0.1 * n and above >= 0.1 * n, (geo, qmin, rounding, below, above)
        assert ref["hist"].min() > 0 and ref["hist"].sum() == n, (geo, qmin, rounding, ref["hist"])
        assert np.all(ref["err2"] > 0) and np.all(np.isfinite(ref["sig2"]))
    P, s, b, _ = make_affine_case(SEED, *geo)
    for rounding in ("floor", "nearest"):
        ref = G.group_stats_reference(P, s, -8, 7, axis, gs, b=b, rounding=rounding)
        assert ref["below"].sum() >= 0.1 * n and ref["above"].sum() >= 0.1 * n, (geo, rounding)
    assert max(gs, 1) <= 1 << 20      # the derivation of G.REL: no group beyond 2^20 elements


@pytest.mark.parametrize("geo", [(256, 260, 0, 32), (64, 576, 1, 128)], ids=lambda g: "x".join(map(str, g)))
def test_mse_scales_never_lose_to_absmax_on_the_reference(geo):
    R, C, axis, gs = geo
    P = S.make_input(*geo)
    for qmin, qmax in S.RANGES:
        for rounding in S.ROUNDINGS:
            s_abs = S.case_reference(*geo, qmin, qmax, "absmax")["s"]
            s_mse = S.case_reference(*geo, qmin, qmax, "mse", rounding)["s"]
            e_abs = G.group_stats_reference(P, s_abs, qmin, qmax, axis, gs, rounding=rounding)
            e_mse = G.group_stats_reference(P, s_mse, qmin, qmax, axis, gs, rounding=rounding)
            assert np.all(e_mse["err2"] <= e_abs["err2"] * (1 + G.REL)), (geo, qmin, qmax, rounding)
            if qmin < 0 < qmax:      # absmax covers every side that has a bound other than zero
                assert e_abs["below"].sum() == 0 and e_abs["above"].sum() == 0
            else:
                assert e_abs["above"].sum() == 0


# ------------------------------------------------------------------------------------------------------------- the C ABI surface
def test_entry_point_is_declared_exported_and_bound():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    assert "lq_group_stats" in declared and hasattr(lib, "lq_group_stats") and "lq_group_stats" in _hip.SIGNATURES
    assert declared - {"lq_status", "lq_qdtype", "lq_adam_mode"} == set(_hip.SIGNATURES)
    assert len(_hip.SIGNATURES["lq_group_stats"][1]) == 16 and lib.lq_version() == 3            # an addition only
    doc = header[header.index("quantization statistics of the clipped pair"):header.index("int lq_group_stats")]
    for needle in ("below[g]", "above[g]", "err2[g]", "sig2[g]", "hist[q - qmin] += 1", "<= 4096", "LQ_EINVAL", "LQ_EALIGN", "ONE launch",
                   "no float\n * atomics", "8-byte grid"):
        assert needle in doc, needle
    assert lq.group_stats is ops.group_stats and lq.summarize_stats is ops.summarize_stats and lq.quant_stats is layers.quant_stats
    assert lq.GroupQuantTrackingCallback is tracking.GroupQuantTrackingCallback and ops.STATS_MAX_BINS == 4096
    from learned_quantization_amd import export
    assert export.quantized_tensors is layers.quantized_tensors                                 # one walk, not two


def test_validation_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    assert p % 8 == 0
    fn = lib.lq_group_stats

    def call(P=p, s=p, b=None, qmin=-8, qmax=7, rounding=0, below=p, above=p, err2=p, sig2=p, hist=p, R=5, C=3, axis=0, gs=2):
        return fn(P, s, b, qmin, qmax, rounding, below, above, err2, sig2, hist, R, C, axis, gs, None)

    for name in ("P", "s", "below", "above", "err2", "sig2"):
        assert call(**{name: None}) == LQ_EINVAL and f"'{name}' is NULL" in _err(), name
    assert call(qmin=8) == LQ_EINVAL and "qmin 8 > qmax 7" in _err()
    assert call(qmin=-LIM - 1) == LQ_EINVAL and "outside +-2^24" in _err()
    assert call(qmax=LIM + 1) == LQ_EINVAL and "outside +-2^24" in _err()
    for bad in (-1, 2, 7):
        assert call(rounding=bad) == LQ_EINVAL and "bad rounding" in _err()
    for axis in (-1, 2):
        assert call(axis=axis) == LQ_EINVAL and "bad axis" in _err()
    for gs in (0, -3):
        assert call(gs=gs) == LQ_EINVAL and "group size" in _err()
    for R, C in ((0, 3), (5, 0), (-1, 3)):
        assert call(R=R, C=C) == LQ_EINVAL and "extents must be positive" in _err()
    for R, C in ((1 << 20, 1 << 11), (1 << 31, 1)):
        assert call(R=R, C=C, axis=1) == LQ_EINVAL and "not below 2^31" in _err()
    assert call(qmin=-2048, qmax=2048) == LQ_EINVAL and "4097 codes" in _err() and "4096" in _err()      # with a histogram only
    assert call(qmin=0, qmax=4096) == LQ_EINVAL and "4097 codes" in _err()
    for name in ("P", "s", "b", "below", "above", "hist"):
        for off in (1, 2):
            assert call(**{name: p + off}) == LQ_EALIGN and "not 4-byte aligned" in _err(), name
    for name in ("err2", "sig2"):
        for off in (1, 4):
            assert call(**{name: p + off}) == LQ_EALIGN and "8-byte aligned" in _err(), name


# ------------------------------------------------------------------------------------------------------------- summarize_stats
def _record(below, above, err2, sig2, hist):
    return ops.GroupStats(np.array(below, np.int64), np.array(above, np.int64), np.array(err2, np.float64), np.array(sig2, np.float64),
                          None if hist is None else np.array(hist, np.int64))


def test_summarize_stats_on_hand_made_records():
    s = ops.summarize_stats(_record([[1, 0], [2, 0]], [[0, 0], [0, 5]], [[1.0, 0.5], [0.25, 0.25]], [[100.0, 5.0], [25.0, 70.0]],
                                    [10, 0, 20, 10]), 40)
    assert s["clip_low"] == 3 / 40 and s["clip_high"] == 5 / 40
    assert s["sqnr_db"] == 10 * math.log10(200.0 / 2.0) == 20.0
    assert s["worst_group_sqnr_db"] == 10 * math.log10(5.0 / 0.5)
    assert s["used_levels"] == 3 and s["entropy_bits"] == 1.5                    # shares 1/4, 1/2, 1/4
    # zero error: inf; one used level: zero entropy
    s = ops.summarize_stats(_record([0], [0], [0.0], [4.0], [0, 8, 0]), 8)
    assert s["sqnr_db"] == math.inf and s["worst_group_sqnr_db"] == math.inf and s["used_levels"] == 1 and s["entropy_bits"] == 0.0
    assert s["clip_low"] == 0.0 and s["clip_high"] == 0.0
    # one exact group next to a lossy one: the tensor's value is finite, the worst group's is the lossy one's
    s = ops.summarize_stats(_record([0, 0], [0, 0], [0.0, 1.0], [4.0, 10.0], None), 8)
    assert s["sqnr_db"] == 10 * math.log10(14.0) and s["worst_group_sqnr_db"] == 10.0 and s["used_levels"] is None and s["entropy_bits"] is None
    # a NaN group spoils the tensor's value and is the worst group; uint32 counts above 2^31 arrive as int32 bit patterns
    s = ops.summarize_stats(_record([0, 0], [0, 0], [math.nan, 1.0], [4.0, 10.0], [1, 1]), 2)
    assert math.isnan(s["sqnr_db"]) and math.isnan(s["worst_group_sqnr_db"]) and s["entropy_bits"] == 1.0
    big = ops.GroupStats(torch.tensor([-(1 << 31)], dtype=torch.int32), torch.tensor([0], dtype=torch.int32),
                         torch.tensor([1.0], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64), None)
    assert ops.summarize_stats(big, 1 << 32)["clip_low"] == 0.5
    with pytest.raises(ValueError, match="numel"):
        ops.summarize_stats(big, 0)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_python_surface():
    P, s = torch.zeros(8, 4), torch.ones(2, 4)
    with pytest.raises(ValueError, match="4096"):
        ops.group_stats(P, s, -2048, 2048, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # like every other op; 4097 codes without a histogram
        ops.group_stats(P, s, -2048, 2048, 4, want_hist=False)
    with pytest.raises(ValueError, match="rounding"):
        ops.group_stats(P, s, -8, 7, 4, rounding="up")
    with pytest.raises(ValueError, match="qmin <= qmax"):
        ops.group_stats(P, s, 7, -8, 4)
    lq.reset_layer_names()
    plain = lq.CustomDenseLayer(units=3, initializer=lq.RandomNormal(seed=1), input_shape=5, scale_gradient="ste")
    with pytest.raises(ValueError, match="needs bits or q_range.*q_minmax"):
        plain.nested_q_w_layer.quant_stats(plain.W)
    with pytest.raises(ValueError, match="has no range"):
        layers.quant_stats(plain)
    with pytest.raises(ValueError, match="has no range"):
        tracking.GroupQuantTrackingCallback(plain, "unused")


def test_group_sizes_of_the_callback():
    w = torch.empty(10, 3)
    assert np.array_equal(tracking.group_sizes(w, torch.empty(3, 3), 4), [[4] * 3, [4] * 3, [2] * 3])
    assert np.array_equal(tracking.group_sizes(w, torch.empty(1), None), [30])
    assert np.array_equal(tracking.group_sizes(w, torch.empty(10, 1), None), [[3]] * 10)
    k = torch.empty(8, 4, 3, 3).permute(2, 3, 1, 0)          # HWIO shape, OIHW memory
    assert np.array_equal(tracking.group_sizes(k, torch.empty(8, 3), 16), [[16, 16, 4]] * 8)


def test_train_driver_flag():
    from learned_quantization_amd import train
    ap = train.build_parser()
    assert ap.parse_args([]).quant_stats is False and ap.parse_args(["--bits", "4", "--quant-stats"]).quant_stats is True
