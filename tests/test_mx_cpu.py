"""CPU tests of the OCP microscaling quantizer (include/lq_hip.h: lq_fq_forward_mx / lq_fq_backward_mx / lq_scale_init_mx): the
NumPy reference (tests/_mx_reference.py) pinned against independent sources -- torch's float8 conversions, a brute-force nearest
over the enumerated grid, hand-written tables --, the C-ABI surface and its validation without a launch, the refusals of the
Python surface, and the conditions of every data set of tests/test_gpu_mx.py, asserted on the reference (no GPU here)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, layers as L, ops
from learned_quantization_amd.models import build_model

sys.path.insert(0, os.path.dirname(__file__))
import _mx_reference as X                                                            # noqa: E402
from _group_forms import FORM_CASES, LARGE, WINDOW_SHAPES                            # noqa: E402
from _group_reference import check_condition                                         # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LQ_EINVAL, LQ_EALIGN = -1, -4
NAMES = list(X.FORMATS)
EXTRA_SHAPES = [(69, 128, 0, 32), (5, 100, 1, 32)]


def _u2f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def _err():
    return _hip.load().lq_last_error().decode()


# ---------------------------------------------------------------------------------------------------------- 1 element rounding
@pytest.mark.parametrize("name,dtype", [("fp8_e4m3", torch.float8_e4m3fn), ("fp8_e5m2", torch.float8_e5m2)])
def test_rounding_against_torch_float8(name, dtype):
    """10^5 Gaussians spread over the format's binades and clamped to its range: torch's CPU conversion gives the grid value."""
    fmt = X.FORMATS[name]
    rng = np.random.default_rng(7)
    t = (rng.standard_normal(100000) * np.exp2(rng.uniform(fmt.emin - fmt.M - 2, fmt.emax, 100000))).astype(np.float32)
    t = np.clip(t, -np.float32(fmt.max), np.float32(fmt.max))
    want = torch.from_numpy(t).to(dtype).to(torch.float32).numpy()
    got = X.round_to_grid(t, fmt)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (np.abs(got) < 2.0 ** fmt.emin).any() and (np.abs(got) == fmt.max).any()      # subnormals and the top are reached


@pytest.mark.parametrize("name", NAMES)
def test_rounding_is_nearest_and_ties_go_to_the_even_mantissa(name):
    fmt = X.FORMATS[name]
    g = X.grid(fmt)
    assert g[0] == 0 and g[-1] == fmt.max and g.size == X.FINITE_CODES[name] // 2
    rng = np.random.default_rng(11)
    t = (rng.uniform(0, fmt.max, 20000) * rng.choice([-1.0, 1.0], 20000)).astype(np.float32)
    got = X.round_to_grid(t, fmt).astype(np.float64)
    dist = np.abs(np.abs(t.astype(np.float64))[:, None] - g[None, :])
    assert np.isin(np.abs(got), g).all() and np.array_equal(np.abs(np.abs(got) - np.abs(t.astype(np.float64))), dist.min(axis=1))
    assert np.array_equal(np.signbit(got), np.signbit(t))
    # every midpoint, the first beyond the max included: the neighbour with the even mantissa (even index on the grid)
    mid = X.midpoints(fmt)
    full = np.append(g, g[-1] + 2.0 ** (fmt.emax - fmt.M))
    lo = np.arange(mid.size)
    even = np.where(lo % 2 == 0, full[lo], full[lo + 1])
    for sign in (1.0, -1.0):
        q0 = X.round_to_grid((sign * mid).astype(np.float32), fmt).astype(np.float64)
        assert np.array_equal(q0, sign * even), name
    # the tie beyond the max is clipped exactly where the max has the odd mantissa (all formats but fp8_e4m3, whose max is S.1111.110)
    assert (X.round_to_grid(np.float32([mid[-1]]), fmt)[0] > fmt.max) == (name != "fp8_e4m3")


def test_rounding_special_values():
    for fmt in X.FORMATS.values():
        t = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38], np.float32)
        q0 = X.round_to_grid(t, fmt)
        assert q0[0] == 0 and not np.signbit(q0[0]) and q0[1] == 0 and np.signbit(q0[1])
        assert q0[2] == np.inf and q0[3] == -np.inf and np.isnan(q0[4])
        assert q0[5] == 0 and q0[6] == 0 and np.signbit(q0[6]) and q0[7] > fmt.max


# ------------------------------------------------------------------------------------------------------------------- 2 codes
@pytest.mark.parametrize("name", NAMES)
def test_encode_decode_identity(name):
    fmt = X.FORMATS[name]
    table = X.decode_table(fmt)
    finite = np.isfinite(table)
    assert int(finite.sum()) == X.FINITE_CODES[name] == {"fp4_e2m1": 16, "fp6_e2m3": 64, "fp6_e3m2": 64, "fp8_e4m3": 254, "fp8_e5m2": 248}[name]
    codes = np.arange(table.size)[finite]
    assert np.array_equal(X.encode(table[finite], fmt), codes)
    top = 1 << (fmt.bits - 1)
    assert table[top] == 0 and np.signbit(table[top]) and X.encode(np.float32([-0.0]), fmt)[0] == top
    assert np.abs(table[finite]).max() == fmt.max
    assert X.encode(np.float32([np.nan]), fmt)[0] == top - 1
    # rounding lands on the table
    t = np.linspace(-fmt.max, fmt.max, 4001).astype(np.float32)
    q = X.round_to_grid(t, fmt)
    assert np.array_equal(table[X.encode(q, fmt)].view(np.uint32), q.view(np.uint32))


def test_fp8_tables_are_the_ocp_ones():
    for name, dtype in (("fp8_e4m3", torch.float8_e4m3fn), ("fp8_e5m2", torch.float8_e5m2)):
        want = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(dtype).to(torch.float32).numpy()
        got = X.decode_table(X.FORMATS[name])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(got)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------- 3 E8M0 rounding
def test_e8m0_rounding():
    s = np.array([_u2f(0x3FB504F2), _u2f(0x3FB504F3), 1.0, 2.0 ** -126, _u2f(0x007FFFFF), 3e38, 0.0, -0.0, -1.0, -2.0 ** -10,
                  np.inf, np.nan, 2.0 ** 127, _u2f(0x7F3504F2), _u2f(0x7F3504F3), 1.4, 1.5, 0.7, 0.71], np.float32)
    got = X.e8m0_round(s)
    want = np.array([1.0, 2.0, 1.0, 2.0 ** -126, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, 2.0 ** 127,
                     2.0 ** 127, np.nan, 1.0, 2.0, 0.5, 1.0], np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    assert _u2f(0x3FB504F3) == np.float32(np.sqrt(2.0)) > _u2f(0x3FB504F2)                  # the threshold is the float32 sqrt(2)
    rng = np.random.default_rng(3)
    s = np.exp2(rng.uniform(-120, 120, 10000)).astype(np.float32)
    assert np.array_equal(X.e8m0_round(s).astype(np.float64), np.exp2(np.floor(np.log2(s.astype(np.float64)) + 0.5)))


# -------------------------------------------------------------------------------------------------------------------- 4 init
def test_init_table():
    """One group per row (axis 1, gs = C): A = max|P|.  fp4_e2m1: emax 2, mm 1.5; fp8_e4m3: emax 8, mm 1.75."""
    mv = np.float32(2.0 ** -20)
    P = np.array([[6.0, -1.0, 0.0],          # A = 1.5 * 2^2 == mm * 2^2: m == mm exactly
                  [0.5, 7.0, -2.0],          # 1.75 * 2^2
                  [4.0, 0.0, 0.0],           # 1.0 * 2^2
                  [0.0, -0.0, 0.0],          # zeros
                  [1.0, np.nan, 2.0],
                  [np.inf, 1.0, 2.0],
                  [1e-40, 0.0, 0.0],         # subnormal: p far below min_value
                  [-_u2f(0x40C00001), 1.0, 0.0]], np.float32)      # one ulp above 6
    ocp = X.init_reference(P, X.FORMATS["fp4_e2m1"], "mx", 1, 3, mv)[:, 0]
    cover = X.init_reference(P, X.FORMATS["fp4_e2m1"], "cover", 1, 3, mv)[:, 0]
    assert np.array_equal(ocp[[0, 1, 2, 3, 6, 7]], np.float32([1, 1, 1, mv, mv, 1]))
    assert np.array_equal(cover[[0, 1, 2, 3, 6, 7]], np.float32([1, 2, 1, mv, mv, 2]))
    assert np.isnan(ocp[4]) and np.isnan(ocp[5]) and np.isnan(cover[4]) and np.isnan(cover[5])
    e4 = X.init_reference(np.float32([[448.0, 1.0], [449.0, 1.0], [1e-30, 0.0]]) * np.float32(2.0 ** -8), X.FORMATS["fp8_e4m3"], "cover", 1, 2,
                          np.float32(2.0 ** -126))[:, 0]
    assert e4[0] == 2.0 ** -8 and e4[1] == 2.0 ** -7 and e4[2] == np.float32(2.0 ** -116)
    tiny = X.init_reference(np.float32([[1e-44, 0.0]]), X.FORMATS["fp8_e5m2"], "mx", 1, 2, np.float32(2.0 ** -126))
    assert tiny[0, 0] == np.float32(2.0 ** -126)          # raised to the smallest normal


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", [(192, 64, 0, 32), (40, 512, 1, 64)], ids=str)
def test_cover_clips_nothing_and_ocp_clips_some(name, case):
    fmt = X.FORMATS[name]
    R, C, axis, gs = case
    rng = np.random.default_rng(5)
    P = (rng.standard_normal((R, C)) * 0.05).astype(np.float32)
    dy = np.ones_like(P)
    mv = np.float32(2.0 ** -126)         # the rules themselves: the library's own minimum (1.19e-5) exceeds an fp8_e5m2 scale of such weights
    cover = X.init_reference(P, fmt, "cover", axis, gs, mv)
    ocp = X.init_reference(P, fmt, "mx", axis, gs, mv)
    assert np.all((cover == ocp) | (cover == 2 * ocp))
    assert X.mx_reference(P, cover, dy, fmt, "e8m0", axis, gs)["clipped"].sum() == 0
    assert X.mx_reference(P, ocp, dy, fmt, "e8m0", axis, gs)["clipped"].sum() > 0


# ----------------------------------------------------------------------------------------------------------- 5 entry points
def test_entry_points_are_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    for fn in ("lq_fq_forward_mx", "lq_fq_backward_mx", "lq_scale_init_mx"):
        assert fn in declared and hasattr(lib, fn) and fn in _hip.SIGNATURES, fn
    assert re.search(r"LQ_ELEM_FP4_E2M1 = 0, LQ_ELEM_FP6_E2M3 = 1, LQ_ELEM_FP6_E3M2 = 2, LQ_ELEM_FP8_E4M3 = 3, LQ_ELEM_FP8_E5M2 = 4", header)
    assert "LQ_SCALE_E8M0 = 0, LQ_SCALE_FP32 = 1" in header and "LQ_MX_INIT_OCP = 0, LQ_MX_INIT_COVER = 1" in header
    for needle in ("0x004AFB0D", "0x3504F3", "e4m3fn", "FNUZ", "copysign(rintf(a / u) * u, t)", "2^(E+M) - 1", "1.5, 1.875, 1.75, 1.75, 1.75"):
        assert needle in header, needle
    assert lq.ELEMENT_FORMATS is ops.ELEMENT_FORMATS and list(ops.ELEMENT_FORMATS) == NAMES
    for name, f in X.FORMATS.items():
        o = ops.check_element_format(name)
        assert (o.id, o.bits, o.E, o.M, o.emin, o.emax, o.max) == f[:7] and o.bits == 1 + o.E + o.M
    assert lq.fq_forward_mx is ops.fq_forward_mx and lq.fq_backward_mx is ops.fq_backward_mx and lq.scale_init_mx is ops.scale_init_mx


def test_validation_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    fwd, bwd, init = lib.lq_fq_forward_mx, lib.lq_fq_backward_mx, lib.lq_scale_init_mx
    geo = (5, 3, 0, 2, None)
    assert fwd(None, p, p, None, 0, 0, 0, *geo) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fwd(p, p, None, None, 0, 0, 0, *geo) == LQ_EINVAL and "'out' is NULL" in _err()
    assert fwd(p, p, p, p, 0, 0, 0, *geo) == LQ_EINVAL and "disagree" in _err()
    assert bwd(p, p, None, 0, 0, 1.0, p, p, p, *geo) == LQ_EINVAL and "'dy' is NULL" in _err()
    assert bwd(p, p, p, 0, 0, 1.0, None, p, p, *geo) == LQ_EINVAL and "'dP' is NULL" in _err()
    assert init(p, None, 0, 0, 1e-5, *geo) == LQ_EINVAL and "'s' is NULL" in _err()
    for bad in (-1, 5, 99):
        assert fwd(p, p, p, None, 0, bad, 0, *geo) == LQ_EINVAL and "bad element format" in _err()
        assert bwd(p, p, p, bad, 0, 1.0, p, p, p, *geo) == LQ_EINVAL and "bad element format" in _err()
        assert init(p, p, bad, 0, 1e-5, *geo) == LQ_EINVAL and "bad element format" in _err()
    for bad in (-1, 2):
        assert fwd(p, p, p, None, 0, 0, bad, *geo) == LQ_EINVAL and "bad scale format" in _err()
        assert bwd(p, p, p, 0, bad, 1.0, p, p, p, *geo) == LQ_EINVAL and "bad scale format" in _err()
        assert init(p, p, 0, bad, 1e-5, *geo) == LQ_EINVAL and "bad method" in _err()
    for bad in (0.0, -1e-5, float("inf"), float("nan")):
        assert init(p, p, 0, 0, bad, *geo) == LQ_EINVAL and "min_value" in _err()
    for fn, head in ((fwd, (p, p, p, None, 0, 0, 0)), (bwd, (p, p, p, 0, 0, 1.0, p, p, p)), (init, (p, p, 0, 0, 1e-5))):
        for gs in (0, -3):
            assert fn(*head, 5, 3, 0, gs, None) == LQ_EINVAL and "group size" in _err()
        for axis in (-1, 2):
            assert fn(*head, 5, 3, axis, 2, None) == LQ_EINVAL and "bad axis" in _err()
        for R, C in ((0, 3), (5, 0)):
            assert fn(*head, R, C, 0, 2, None) == LQ_EINVAL and "extents must be positive" in _err()
        assert fn(*head, 1 << 20, 1 << 11, 1, 2, None) == LQ_EINVAL and "not below 2^31" in _err()
        assert fn(p + 2, *head[1:], *geo) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert bwd(p, p, p, 0, 0, 1.0, p, p + 2, p, *geo) == LQ_EALIGN and "ds is not 4-byte aligned" in _err()
    assert bwd(p, p, p, 0, 0, 1.0, p, p, p + 1, *geo) == LQ_EALIGN and "clipped is not 4-byte aligned" in _err()


# ---------------------------------------------------------------------------------------------------------------- 6 refusals
def _dense(**kw):
    return L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), input_shape=70, **kw)


def test_layer_surface_without_a_device():
    d = _dense(orientation="groupwise", element_format="fp4_e2m1")
    assert d.group_size == 32 and d.scale_format == "e8m0" and d.nested_q_w_layer.scale.shape == (3, 4)
    assert d.nested_q_w_layer.scale_gradient == "ste" and d.nested_q_b_layer.element_format == "fp4_e2m1"
    assert d.nested_q_b_layer.scale.shape == (1,) and d.nested_q_b_layer.group_size is None
    c = L.CustomConv2DLayer(filters=8, kernel_size=(3, 3), initializer=L.RandomNormal(seed=1), input_shape=5, orientation="groupwise",
                            element_format="fp8_e4m3", scale_format="fp32", group_size=16)
    assert c.nested_q_k_layer.scale.shape == (8, 3) and c.scale_format == "fp32"
    m = build_model("mnist", mode="ste", value=0.0, element_format="fp6_e3m2")
    assert all(layer.element_format == "fp6_e3m2" and layer.group_size == 32 for layer in L.custom_layers_of(m))
    assert L.quant_stats(m) == {}                                     # layers with an element format are skipped


def test_refusals():
    ok = dict(orientation="groupwise", element_format="fp4_e2m1")
    for kw, needle in ((dict(bits=4), "bits / q_range / signed"), (dict(q_range=(-8, 7)), "bits / q_range / signed"),
                       (dict(signed=False), "bits / q_range / signed"), (dict(rounding="nearest"), "ties to even"),
                       (dict(asymmetric=True), "symmetric"), (dict(penalty_threshold=1e-10), "vote"),
                       (dict(penalty_rate=1e-7), "loss term"), (dict(orientation="rowwise"), 'needs orientation="groupwise"'),
                       (dict(orientation="scalar"), 'needs orientation="groupwise"'), (dict(element_format="fp5"), "element_format must be"),
                       (dict(scale_format="ue8"), "scale_format must be")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            _dense(**{**ok, **kw})
    with pytest.raises(ValueError, match="hwio"):
        L.CustomConv2DLayer(filters=8, kernel_size=(3, 3), initializer=L.RandomNormal(seed=1), input_shape=5, kernel_storage="hwio", **ok)
    d = _dense(**ok)
    for method in ("absmax", "lsq", "mse", "minmax"):
        with pytest.raises(ValueError, match="must be one of"):
            d.init_scales(method)
        with pytest.raises(ValueError, match="power of two"):
            L.init_scales(torch.nn.Sequential(d), method)
    plain = _dense(orientation="groupwise", group_size=32, bits=4, scale_gradient="ste")
    for method in ("mx", "cover"):
        with pytest.raises(ValueError, match="without an element format"):
            plain.init_scales(method)
        with pytest.raises(ValueError, match="without element formats"):
            L.init_scales(torch.nn.Sequential(plain), method)
    with pytest.raises(ValueError, match="quant_stats on a layer with an element format"):
        d.nested_q_w_layer.quant_stats(d.W)
    # models and trainers
    for kw, needle in ((dict(mode="nq"), "vote"), (dict(mode="cl"), "loss-term"), (dict(mode="stecl"), "loss-term"),
                       (dict(mode="nqcl"), "loss-term"), (dict(mode="ste", bits=4), "bits / q_range"),
                       (dict(mode="ste", rounding="nearest", bits=None), "ties to even"), (dict(mode="ste", asymmetric=True), "symmetric"),
                       (dict(mode="ste", kernel_storage="hwio"), "hwio"), (dict(mode="ste", scale_init="absmax"), "power of two"),
                       (dict(mode="ste", scale_init="minmax"), "power of two")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            build_model("mnist", value=0.0, element_format="fp4_e2m1", **kw)
    with pytest.raises(ValueError, match="without an element format"):
        build_model("mnist", mode="ste", value=0.0, bits=4, scale_init="cover")
    from learned_quantization_amd.batch import FakeQuantBatch
    from learned_quantization_amd.ddp import DataParallel
    m = build_model("mnist", mode="ste", value=0.0, element_format="fp4_e2m1")
    for kw in (dict(), dict(clipped=True), dict(group_batch=True)):
        with pytest.raises(ValueError, match="element format"):
            FakeQuantBatch(m, **kw)
    with pytest.raises(ValueError, match="mode 'B' over a layer with an element format"):
        DataParallel(m, mode="B")
    # the op
    P, s = torch.zeros(4, 4), torch.ones(1, 4)
    for kw, needle in ((dict(q_range=(-8, 7)), "q_range"), (dict(rounding="nearest"), "rounding"), (dict(offset=s), "offset"),
                       (dict(penalty_threshold=1e-10), "vote"), (dict(defer_scale_grad=True), "defer_scale_grad"),
                       (dict(element_format="e2m1"), "element_format must be"), (dict(scale_format="e8"), "scale_format must be")):
        args = dict(element_format="fp4_e2m1", group_size=4)
        args.update(kw)
        thr = args.pop("penalty_threshold", None)
        with pytest.raises(ValueError, match=re.escape(needle)):
            ops.my_custom_gradient(P, s, thr, **args)


def test_trainer_and_driver_refusals():
    from learned_quantization_amd import experiment, train
    dev = torch.device("cpu")
    for kw, needle in ((dict(batched=True), "batched=True"), (dict(batched=True, group_batch=True, group_size=32), "batched=True"),
                       (dict(ddp_mode="B"), "ddp_mode 'B'"), (dict(bits=4), "bits / q_range"), (dict(scale_init="mse"), "power of two")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            train.Trainer("mnist", "ste", 0.0, "scalar", None, device=dev, element_format="fp4_e2m1", **kw)
    with pytest.raises(ValueError, match="without an element format"):
        train.Trainer("mnist", "ste", 0.0, "scalar", None, device=dev, bits=4, scale_init="mx")
    ap = train.build_parser()
    ns = ap.parse_args(["--mode", "ste", "--element-format", "fp4_e2m1", "--scale-init", "cover", "--group-size", "16", "--scale-format", "fp32"])
    assert (ns.element_format, ns.scale_init, ns.group_size, ns.scale_format) == ("fp4_e2m1", "cover", 16, "fp32")
    for argv in (["--scale-init", "mx"], ["--scale-format", "fp32"], ["--element-format", "fp4_e2m1", "--bits", "4"],
                 ["--element-format", "fp4_e2m1", "--batched"], ["--element-format", "fp4_e2m1", "--scale-init", "absmax"],
                 ["--element-format", "fp4_e2m1", "--rounding", "nearest"], ["--element-format", "fp9"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--mode", "ste"] + argv)
    ep = experiment.build_parser()
    base = ["--seed", "1", "--orientation", "scalar", "--training", "from_scratch", "--scale-gradient", "ste"]
    assert ep.parse_args(base + ["--element-format", "fp8_e5m2", "--scale-init", "mx"]).element_format == "fp8_e5m2"
    with pytest.raises(SystemExit):
        ep.parse_args(base + ["--element-format", "fp8_e5m2", "--bits", "8"])


# -------------------------------------------------------------------------------------------------------- 7 data conditions
PARITY_FP4 = [c for c in FORM_CASES if c != LARGE]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", X.GAUSS_SHAPES, ids=str)
def test_gaussian_condition_every_format(name, case):
    for sf in X.SCALE_FORMATS:
        P, s, dy = X.gaussian_case(name, sf, *case)
        ref = X.mx_reference(P, s, dy, X.FORMATS[name], sf, case[2], case[3])
        check_condition(ref, *case, f"{name} {sf} {case}")
        share = ref["clipped"].sum() / P.size
        assert 0.3 <= share <= 0.42, share


@pytest.mark.parametrize("name,sf,case", X.gaussian_cases(), ids=str)
def test_gaussian_condition_of_every_gpu_case(name, sf, case):
    assert X.WINDOW_SHAPES == WINDOW_SHAPES and X.RAGGED_SHAPES == EXTRA_SHAPES and len(PARITY_FP4) == len(FORM_CASES) - 1
    P, s, dy = X.gaussian_case(name, sf, *case)
    ref = X.mx_reference(P, s, dy, X.FORMATS[name], sf, case[2], case[3])
    check_condition(ref, *case, f"{name} {sf} {case}")


@pytest.mark.parametrize("name", NAMES)
def test_loguniform_reaches_every_code(name):
    for sf in X.SCALE_FORMATS:
        P, s, dy = X.loguniform_case(name, sf, *X.FULL_COVER_SHAPE)
        ref = X.mx_reference(P, s, dy, X.FORMATS[name], sf, *X.FULL_COVER_SHAPE[2:])
        assert X.code_coverage(ref, name) == 1.0, (name, sf)
        for case in X.loguniform_shapes(name):
            P, s, dy = X.loguniform_case(name, sf, *case)
            ref = X.mx_reference(P, s, dy, X.FORMATS[name], sf, case[2], case[3])
            assert X.code_coverage(ref, name) >= 0.95, (name, sf, case, X.code_coverage(ref, name))
            assert ref["clipped"].sum() > 0 and (ref["q"] == 0).any() and (np.abs(ref["q"]) == X.FORMATS[name].max).any()


@pytest.mark.parametrize("name", NAMES)
def test_ties_data_holds_every_midpoint(name):
    fmt = X.FORMATS[name]
    for case in WINDOW_SHAPES:
        P, s, dy, n_mid = X.ties_case(name, *case)
        ref = X.mx_reference(P, s, dy, fmt, "e8m0", case[2], case[3])
        t = ref["t"]
        mids = np.concatenate([X.midpoints(fmt), -X.midpoints(fmt)])
        assert mids.size == n_mid and np.isin(mids, t.astype(np.float64)).all(), (name, case)      # P / s_eff gives every midpoint back exactly
        assert (~ref["inside"]).any() and ref["inside"].any()
        # the two neighbours of a tie round apart
        flat_t, flat_q = t.reshape(-1), ref["q0"].reshape(-1)
        at = np.flatnonzero(np.isin(flat_t.astype(np.float64), mids))
        assert at.size and np.isfinite(flat_q[at]).all()


@pytest.mark.parametrize("sf", X.SCALE_FORMATS)
@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e5m2"])
def test_bad_scale_data_spoils_its_own_groups_only(name, sf):
    """The bad-input set of the GPU file: every bad scale under E8M0 (and the non-finite, zero and NaN ones under fp32) gives a NaN
    ds in its own group; most of the ordinary groups stay finite (those holding a planted NaN do not)."""
    from _bounds import stable_seed
    from _group_forms import window_group_case
    for case in WINDOW_SHAPES:
        P, s, dy, bad = window_group_case(stable_seed("mx-window", case), *case)
        ref = X.mx_reference(P, s, dy, X.FORMATS[name], sf, case[2], case[3])
        assert np.isnan(ref["ds"]).any() and np.isfinite(ref["ds"][~bad]).mean() > 0.5, (name, sf, case)
        if sf == "e8m0":
            eff = X.e8m0_round(s)
            invalid = bad & ~((s >= np.float32(2.0 ** -126)) & (s < np.float32(2.0 ** 127) * np.float32(1.4)))
            assert np.isnan(eff[invalid]).all() and invalid.any() and np.isnan(ref["ds"][invalid]).all()
            assert np.isfinite(eff[~bad]).all()
