"""CPU tests of the per-group statistics of the microscaling quantizer (include/lq_hip.h: lq_mx_stats): the NumPy reference pinned
on a hand-written table, the identities and the data conditions tests/test_gpu_mx_stats.py leans on (on the reference alone), the
C-ABI surface and its validation without a launch, ops.summarize_mx_stats on hand-made records, and the refusals of the Python
surface (no GPU here)."""
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
import _mx_stats_reference as M                                                      # noqa: E402
from _mx_reference import FORMATS, SCALE_FORMATS                                     # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LQ_EINVAL, LQ_EALIGN = -1, -4
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


def _err():
    return _hip.load().lq_last_error().decode()


# ------------------------------------------------------------------------------------------------------- the reference, pinned
# fp4_e2m1 (grid 0, .5, 1, 1.5, 2, 3, 4, 6; codes 0..7, sign bit 8), E8M0, eight groups = rows of four (axis 1, gs = 4).  Every
# stored scale is a power of two but the last, every value and quotient is exact in float32.
NAN = np.nan
S84 = np.array([[1.0], [1.0], [1.0], [0.5], [0.5], [1.0], [1.0], [0.0]], np.float32)
P84 = np.array([
    [2.5, 3.5, -5.0, 0.75],        # ties: to the even mantissa 2 4 -4, and .75 -> 1 (codes 4 6 14 2)                       err .5 .5 1 .25
    [0.25, -0.25, 0.125, 0.0],     # flushed: |t| <= .25 -> +0 -0 +0 (the tie .25 goes to the even 0); a zero is not flushed  err = P
    [0.5, -0.5, 0.375, 0.625],     # subnormal .5 (codes 1 9); .375 and .625 -> .5                                          err 0 0 .125 .125
    [4.0, 3.25, 100.0, 3.0],       # s = .5, t = 8 6.5 200 6: q0 = 8 6 200 6, above = 2 (8 and 200)                           out 3 3 3 3
    [-4.0, -3.0, -3.5, 1.0],       # s = .5, t = -8 -6 -7 2: q0 = -8 -6 -8 2 (tie -7 -> -8): below = 2                        out -3 -3 -3 1
    [-0.0, -0.125, 1.0, -1.0],     # -0.0 keeps its sign (code 8) and is not flushed; -.125 -> -0 is (code 8)
    [NAN, 1.0, 2.0, 3.0],          # a NaN element: on no side, not flushed, not binned; err2 and sig2 of the group are NaN
    [1.0, 0.0, -2.0, 0.25],        # scale 0: invalid E8M0, s_eff = NaN: nothing counted or binned, err2 NaN, sig2 = 1 + 4 + 1/16
], np.float32)


def test_reference_on_a_hand_written_table():
    ref = M.mx_stats_reference(P84, S84, FORMATS["fp4_e2m1"], "e8m0", 1, 4)
    assert np.array_equal(ref["q"][:6], np.array([[2, 4, -4, 1], [0, -0.0, 0, 0], [0.5, -0.5, 0.5, 0.5], [6, 6, 6, 6], [-6, -6, -6, 2],
                                                  [-0.0, -0.0, 1, -1]], np.float32))
    assert np.array_equal(np.signbit(ref["q"][:6]), np.array([[0, 0, 1, 0], [0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0],
                                                              [1, 1, 0, 1]], bool))
    assert np.array_equal(ref["below"].reshape(-1), [0, 0, 0, 0, 2, 0, 0, 0])
    assert np.array_equal(ref["above"].reshape(-1), [0, 0, 0, 2, 0, 0, 0, 0])
    assert np.array_equal(ref["flushed"].reshape(-1), [0, 3, 0, 0, 0, 1, 0, 0])
    e2 = ref["err2"].reshape(-1)
    assert np.array_equal(e2[:6], [0.25 + 0.25 + 1.0 + 0.0625, 0.0625 + 0.0625 + 0.015625, 2 * 0.015625,
                                   1.0 + 0.0625 + 97.0 ** 2 + 0.0, 1.0 + 0.0 + 0.25 + 0.0, 0.015625])
    assert np.isnan(e2[6]) and np.isnan(e2[7])
    s2 = ref["sig2"].reshape(-1)
    assert s2[0] == 6.25 + 12.25 + 25.0 + 0.5625 and s2[5] == 0.015625 + 2.0 and np.isnan(s2[6]) and s2[7] == 5.0625
    hist = np.zeros(16, np.int64)
    for code, n in {4: 2, 6: 1, 14: 1, 2: 2,            # row 0; row 4's 2.0 -> code 4; row 5's 1.0 -> code 2
                    0: 3, 8: 3,                         # row 1: +0 -0 +0 +0 -> three 0 and one 8; row 5: -0 -0 -> two 8
                    1: 3, 9: 1,                         # row 2
                    7: 4, 15: 3,                        # rows 3 and 4: saturated at +-6
                    10: 1,                              # row 5's -1.0
                    }.items():
        hist[code] += n
    hist[2] += 1      # row 6's 1.0
    hist[4] += 1      # row 6's 2.0
    hist[5] += 1      # row 6's 3.0
    assert np.array_equal(ref["hist"], hist), (ref["hist"], hist)
    assert ref["hist"].sum() == 32 - 1 - 4          # the NaN element and the group under the invalid scale are not binned


# ----------------------------------------------------------------------------------- identities and data conditions of the GPU inputs
@pytest.mark.parametrize("geo", M.GEOMETRIES, ids=_ids)
def test_identities_and_data_conditions_of_the_gpu_inputs(geo):
    R, C, axis, gs = geo
    pairs = {(n, sf) for n, sf, g in M.gpu_cases() if g == geo}
    assert pairs >= {("fp4_e2m1", "e8m0"), ("fp8_e4m3", "fp32")}
    assert (len(pairs) == len(FORMATS) * len(SCALE_FORMATS)) == (geo in M.FORM_GEOMETRIES)
    for name, sf in sorted(pairs):
        fmt, what = FORMATS[name], f"{name} {sf} {geo}"
        P, _ = M.case(name, sf, geo)
        ref = M.reference(name, sf, geo)
        assert np.array_equal(ref["below"] + ref["above"], ref["clipped"]), what
        number = ~np.isnan(ref["q"])
        assert np.array_equal(ref["hist"], np.bincount(ref["code"][number], minlength=1 << fmt.bits)), what
        assert ref["hist"].sum() == P.size - np.isnan(ref["q"]).sum() == P.size, what
        below, above, flushed = (int(ref[k].sum()) for k in ("below", "above", "flushed"))
        sub = int(ref["hist"][M.subnormal_codes(fmt)].sum())
        if geo == M.BIAS:
            assert below + above >= 1 and flushed >= 1, (what, below, above, flushed)
        else:
            assert below >= 1 and above >= 1 and flushed >= 1 and sub >= 1, (what, below, above, flushed, sub)
        assert min(gs, R if axis == 0 else C) <= 1 << 20                  # REL's premise: no group has more than 2^20 elements


# ------------------------------------------------------------------------------------------------------------- the C ABI surface
def test_entry_point_is_declared_exported_and_bound():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    assert "lq_mx_stats" in declared and hasattr(lib, "lq_mx_stats") and "lq_mx_stats" in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["lq_mx_stats"][1]) == 15 and lib.lq_version() == 3            # an addition only
    doc = header[header.index("quantization statistics of the microscaling pair"):header.index("int lq_mx_stats")]
    for needle in ("below[g]", "above[g]", "flushed[g]", "err2[g]", "sig2[g]", "hist[code] += 1", "2^bits", "LQ_EINVAL", "LQ_EALIGN",
                   "ONE launch", "no float\n * atomics", "8-byte grid", "invalid E8M0 scale", "-0.0 keeps its sign bit"):
        assert needle in doc, needle
    assert lq.mx_stats is ops.mx_stats and lq.summarize_mx_stats is ops.summarize_mx_stats and lq.MxStats is ops.MxStats
    assert lq.mx_quant_stats is layers.mx_quant_stats and lq.MxQuantTrackingCallback is tracking.MxQuantTrackingCallback
    assert ops.MxStats._fields == ("below", "above", "flushed", "err2", "sig2", "hist")


def test_validation_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    assert p % 8 == 0
    fn = lib.lq_mx_stats

    def call(P=p, s=p, fmt=0, sf=0, below=p, above=p, flushed=p, err2=p, sig2=p, hist=p, R=5, C=3, axis=0, gs=2):
        return fn(P, s, fmt, sf, below, above, flushed, err2, sig2, hist, R, C, axis, gs, None)

    for name in ("P", "s", "below", "above", "flushed", "err2", "sig2"):
        assert call(**{name: None}) == LQ_EINVAL and f"'{name}' is NULL" in _err(), name
    for fmt in (-1, 5, 99):
        assert call(fmt=fmt) == LQ_EINVAL and "bad element format" in _err()
    for sf in (-1, 2):
        assert call(sf=sf) == LQ_EINVAL and "bad scale format" in _err()
    for axis in (-1, 2):
        assert call(axis=axis) == LQ_EINVAL and "bad axis" in _err()
    for gs in (0, -3):
        assert call(gs=gs) == LQ_EINVAL and "group size" in _err()
    for R, C in ((0, 3), (5, 0), (-1, 3)):
        assert call(R=R, C=C) == LQ_EINVAL and "extents must be positive" in _err()
    for R, C in ((1 << 20, 1 << 11), (1 << 31, 1)):
        assert call(R=R, C=C, axis=1) == LQ_EINVAL and "not below 2^31" in _err()
    for name in ("P", "s", "below", "above", "flushed", "hist"):
        for off in (1, 2):
            assert call(**{name: p + off}) == LQ_EALIGN and "not 4-byte aligned" in _err(), name
    for name in ("err2", "sig2"):
        for off in (1, 4):
            assert call(**{name: p + off}) == LQ_EALIGN and "8-byte aligned" in _err(), name


# ---------------------------------------------------------------------------------------------------------- summarize_mx_stats
def _record(below, above, flushed, err2, sig2, hist):
    return ops.MxStats(np.array(below, np.int64), np.array(above, np.int64), np.array(flushed, np.int64), np.array(err2, np.float64),
                       np.array(sig2, np.float64), None if hist is None else np.array(hist, np.int64))


def test_summarize_mx_stats_on_hand_made_records():
    # fp4_e2m1: codes 0 / 8 are +-0, 1 / 9 the one subnormal .5
    hist = [4, 2, 0, 0, 0, 0, 0, 8, 4, 6, 0, 0, 0, 0, 0, 8]
    s = ops.summarize_mx_stats(_record([[1, 0], [2, 0]], [[0, 0], [0, 5]], [[4, 0], [0, 4]], [[1.0, 0.5], [0.25, 0.25]],
                                       [[100.0, 5.0], [25.0, 70.0]], hist), 32, element_format="fp4_e2m1")
    assert set(s) == {"sat_low", "sat_high", "flushed", "sqnr_db", "worst_group_sqnr_db", "used_codes", "entropy_bits", "zero", "subnormal"}
    assert s["sat_low"] == 3 / 32 and s["sat_high"] == 5 / 32 and s["flushed"] == 8 / 32
    assert s["sqnr_db"] == 10 * math.log10(200.0 / 2.0) == 20.0 and s["worst_group_sqnr_db"] == 10 * math.log10(5.0 / 0.5)
    assert s["used_codes"] == 6 and s["zero"] == 8 / 32 and s["subnormal"] == 8 / 32
    pr = np.array([4, 2, 8, 4, 6, 8]) / 32
    assert abs(s["entropy_bits"] - float(-(pr * np.log2(pr)).sum())) < 1e-12
    # fp6_e3m2 (M = 2): the subnormals are codes 1..3 and 33..35, code 4 is the smallest normal
    h6 = np.zeros(64, np.int64)
    h6[[0, 1, 3, 4, 32, 35, 36]] = [1, 2, 3, 4, 5, 6, 7]
    s = ops.summarize_mx_stats(_record([0], [0], [0], [1.0], [4.0], h6), 28, element_format="fp6_e3m2")
    assert s["zero"] == 6 / 28 and s["subnormal"] == 11 / 28 and s["used_codes"] == 7
    with pytest.raises(ValueError, match="64 bins"):
        ops.summarize_mx_stats(_record([0], [0], [0], [1.0], [4.0], h6), 28, element_format="fp4_e2m1")
    # the SQNR conventions: zero error inf, zero signal under an error -inf, a NaN group spoils the tensor and is the worst
    s = ops.summarize_mx_stats(_record([0], [0], [0], [0.0], [4.0], None), 8, element_format="fp8_e4m3")
    assert s["sqnr_db"] == math.inf and s["worst_group_sqnr_db"] == math.inf
    assert s["used_codes"] is None and s["entropy_bits"] is None and s["zero"] is None and s["subnormal"] is None
    s = ops.summarize_mx_stats(_record([0, 0], [0, 0], [0, 2], [0.0, 1.0], [4.0, 0.0], None), 8, element_format="fp8_e4m3")
    assert s["sqnr_db"] == 10 * math.log10(4.0) and s["worst_group_sqnr_db"] == -math.inf and s["flushed"] == 0.25
    s = ops.summarize_mx_stats(_record([0, 0], [0, 0], [0, 0], [math.nan, 1.0], [4.0, 10.0], None), 2, element_format="fp8_e5m2")
    assert math.isnan(s["sqnr_db"]) and math.isnan(s["worst_group_sqnr_db"])
    # host tensors; uint32 counts above 2^31 arrive as int32 bit patterns
    big = ops.MxStats(torch.tensor([0], dtype=torch.int32), torch.tensor([0], dtype=torch.int32), torch.tensor([-(1 << 31)], dtype=torch.int32),
                      torch.tensor([1.0], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64), None)
    assert ops.summarize_mx_stats(big, 1 << 32, element_format="fp4_e2m1")["flushed"] == 0.5
    many = ops.summarize_mx_stats_many([big, big], [1 << 32, 1 << 33], ["fp4_e2m1", "fp6_e2m3"])
    assert [m["flushed"] for m in many] == [0.5, 0.25]
    with pytest.raises(ValueError, match="numel"):
        ops.summarize_mx_stats(big, 0, element_format="fp4_e2m1")
    with pytest.raises(ValueError, match="element_format must be"):
        ops.summarize_mx_stats(big, 1, element_format="fp5")
    with pytest.raises(TypeError):
        ops.summarize_mx_stats(big, 1)                                    # the fields of a code need the format


# ---------------------------------------------------------------------------------------------------------------- refusals
def _dense(**kw):
    return layers.CustomDenseLayer(units=4, initializer=layers.RandomNormal(seed=1), input_shape=70, **kw)


def test_refusals_of_the_python_surface(tmp_path):
    P, s = torch.zeros(64, 4), torch.ones(2, 4)
    with pytest.raises(ValueError, match="element_format must be"):
        ops.mx_stats(P, s, "fp5")
    with pytest.raises(ValueError, match="scale_format must be"):
        ops.mx_stats(P, s, "fp4_e2m1", 32, "ue8")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # like every other op
        ops.mx_stats(P, s, "fp4_e2m1")
    lq.reset_layer_names()
    plain = _dense(orientation="groupwise", group_size=32, bits=4, scale_gradient="ste")
    with pytest.raises(ValueError, match="mx_stats on a layer without an element format.*quant_stats"):
        plain.nested_q_w_layer.mx_stats(plain.W)
    unbuilt = layers.CustomQuantizedScaleLayer(orientation="groupwise", element_format="fp4_e2m1")
    assert not unbuilt.built
    with pytest.raises(ValueError, match="mx_stats before the layer is built"):
        unbuilt.mx_stats(torch.zeros(64, 4))
    assert layers.mx_quant_stats(plain) == {}                                      # layers without an element format are skipped
    assert layers.mx_quant_stats(torch.nn.Linear(3, 3)) == {}
    with pytest.raises(ValueError, match="has no element format.*GroupQuantTrackingCallback"):
        tracking.MxQuantTrackingCallback(plain, str(tmp_path / "logs"))
    assert not (tmp_path / "logs").exists()                                        # refused before any directory is made
    mx = _dense(orientation="groupwise", element_format="fp4_e2m1")
    with pytest.raises(ValueError, match=r"quant_stats on a layer with an element format.*mx_stats"):
        mx.nested_q_w_layer.quant_stats(mx.W)
    cb = tracking.MxQuantTrackingCallback(mx, str(tmp_path / "mx"))                # construction needs no device
    names = sorted(os.path.basename(f) for f in cb.epoch_files())
    assert len(names) == 18 and len(set(names)) == 18
    for prefix in ("Scale_exponent_", "Sat_low_", "Sat_high_", "Flushed_", "SQNR_dB_", "SQNR_dB_tensor_", "Used_codes_", "Code_entropy_bits_"):
        assert sum(n.startswith(prefix + "Weights") for n in names) == 1 and sum(n.startswith(prefix + "Bias") for n in names) == 1, prefix
    assert np.array_equal(cb.sizes["kernel"], [[32] * 4, [32] * 4, [6] * 4]) and np.array_equal(cb.sizes["bias"], [4])


def test_train_driver_flag(capsys):
    from learned_quantization_amd import train
    ap = train.build_parser()
    assert ap.parse_args([]).mx_stats is False
    assert ap.parse_args(["--element-format", "fp4_e2m1", "--mx-stats"]).mx_stats is True
    for argv in (["--mx-stats"], ["--bits", "4", "--mx-stats"]):
        with pytest.raises(SystemExit) as exc:
            train.main(argv)
        assert exc.value.code == 2 and "--mx-stats needs --element-format" in capsys.readouterr().err
