"""CPU tests of scale initialisation (include/lq_hip.h: lq_scale_init_group): the NumPy reference pinned on a hand-written table, the
C-ABI surface and its validation without a launch, descriptor.init_geometry for every orientation, the refusals of the Python
surface, the drivers' flag, and -- on the reference alone, over the inputs of tests/test_gpu_scale_init.py -- the conditions those
GPU tests rely on (no GPU here)."""
import ctypes
import math
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, ops
from learned_quantization_amd.descriptor import init_geometry

sys.path.insert(0, os.path.dirname(__file__))
import _scale_init_reference as S                                                    # noqa: E402
from _clip_reference import bits_equal                                               # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LQ_EINVAL, LQ_EALIGN = -1, -4
LIM = 1 << 24
MV = S.MIN_VALUE
M22 = np.float32(1.0 + 2.0 ** -22)


def _err():
    return _hip.load().lq_last_error().decode()


# ------------------------------------------------------------------------------------------------------- the reference, pinned
# a 5 x 3 matrix, range [-4, 3], gs = 2: three groups per column (axis 0) or two per row (axis 1), the last one short
P53 = np.array([[0.5, -1.0, 0.0],
                [-2.0, 3.0, 0.0],
                [1.5, -0.25, -1.0],
                [-0.5, 0.75, -3.0],
                [3.0, -6.0, 2.0]], np.float32)
TWO_THIRDS = np.float32(2.0) / np.float32(3.0)
# a = max(ap / 3, an / 4) per group, written out by hand; 0 marks the groups of zeros (they get min_value)
A_AXIS0 = np.array([[0.5, 1.0, 0.0],            # rows 0-1:  max(.5/3, 2/4)   max(3/3, 1/4)     zeros
                    [0.5, 0.25, 0.75],          # rows 2-3:  max(1.5/3, .5/4) max(.75/3, .25/4) max(0, 3/4)
                    [1.0, 1.5, TWO_THIRDS]],    # row 4:     3/3              6/4               2/3
                   np.float32)
A_AXIS1 = np.array([[0.25, 0.0],                # (c0 c1)  (c2)
                    [1.0, 0.0],
                    [0.5, 0.25],
                    [0.25, 0.75],
                    [1.5, TWO_THIRDS]], np.float32)
# sum |P| and n per group, by hand
SUM_AXIS0 = np.array([[2.5, 4.0, 0.0], [2.0, 1.0, 4.0], [3.0, 6.0, 2.0]])
N_AXIS0 = np.array([[2, 2, 2], [2, 2, 2], [1, 1, 1]])
SUM_AXIS1 = np.array([[1.5, 0.0], [5.0, 0.0], [1.75, 1.0], [1.25, 3.0], [9.0, 2.0]])
N_AXIS1 = np.array([[2, 1]] * 5)


@pytest.mark.parametrize("axis,a", [(0, A_AXIS0), (1, A_AXIS1)])
def test_absmax_on_the_hand_written_table(axis, a):
    want = np.maximum(a * M22, np.float32(MV))
    got = S.scale_init_reference(P53, -4, 3, axis, 2, "absmax")
    assert got["s"].shape == a.shape and bits_equal(got["s"], want)
    assert not got["bad"].any()
    # every quotient stays inside [-4, 3] under both roundings: the invariant
    for rounding in S.ROUNDINGS:
        assert not S.clipped_after(P53, got["s"], -4, 3, axis, 2, rounding).any()
    # one-sided range [0, 3]: only the positive side counts; an all-negative group gets min_value
    one = S.scale_init_reference(P53, 0, 3, axis, 2, "absmax")["s"]
    if axis == 0:
        assert one[2, 1] == np.float32(MV) and one[0, 1] == np.float32(1.0) * M22


@pytest.mark.parametrize("axis,sums,n", [(0, SUM_AXIS0, N_AXIS0), (1, SUM_AXIS1, N_AXIS1)])
def test_lsq_on_the_hand_written_table(axis, sums, n):
    want = np.maximum((2.0 * sums / (n * math.sqrt(3.0))).astype(np.float32), np.float32(MV))
    got = S.scale_init_reference(P53, -4, 3, axis, 2, "lsq")["s"]
    assert bits_equal(got, want)
    # qp = -qmin for a range without a positive side
    neg = S.scale_init_reference(P53, -4, 0, axis, 2, "lsq")["s"]
    assert bits_equal(neg, np.maximum((2.0 * sums / (n * 2.0)).astype(np.float32), np.float32(MV)))


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _mse_by_hand(xs, qmin, qmax, rounding, s0):
    """The definition with Python floats, every float32 operation rounded through struct: [(s_k, E_k)]."""
    rows = []
    for k in range(28):
        sk = max(_f32(s0 * ((32 - k) / 32.0)), MV)
        e = 0.0
        for x in xs:
            t = _f32(x / sk)
            q0 = math.floor(t) if rounding == "floor" else float(np.rint(np.float64(t)))
            q = min(max(q0, qmin), qmax)
            e += (x - _f32(q * sk)) ** 2
        rows.append((sk, e))
    return rows


def test_one_mse_group_worked_by_hand():
    """Column 1, rows 0-1 of the table: P = (-1, 3), range [-4, 3].  s0 = 1 + 2^-22.  Under floor, k = 0 puts 3 just below the
    integer 3 (quotient 2.9999993, floor 2, error 1); s = 0.75 s0 (k = 8) gives quotients -1.33 -> -2 and 3.99.. -> 3, errors
    0.5 and 0.75; the best candidate, k = 5, is worked out next to MSE_K_FLOOR below."""
    s0 = float(M22)
    for rounding in S.ROUNDINGS:
        rows = _mse_by_hand([-1.0, 3.0], -4, 3, rounding, s0)
        errs = [e for _, e in rows]
        k = min(range(28), key=lambda i: (errs[i], i))
        got = S.scale_init_reference(P53, -4, 3, 0, 2, "mse", rounding=rounding)
        assert int(got["k"][0, 1]) == k and float(got["s"][0, 1]) == rows[k][0], (rounding, k)
        assert abs(float(got["E_best"][0, 1]) - errs[k]) <= 1e-15
        if rounding == "floor":
            assert abs(errs[0] - 1.0) < 1e-5 and abs(errs[8] - (0.25 + 0.5625)) < 1e-5
            assert k == MSE_K_FLOOR and abs(errs[5] - 0.6923828125) < 1e-5
            assert abs(errs[4] - 0.703125) < 1e-5 and abs(errs[6] - 0.70703125) < 1e-5
        else:
            assert errs[0] < 1e-12 and k == 0          # nearest: absmax already puts both values on the grid
    # the whole table, both axes: the choice is the first minimum of the hand loop for every group
    for axis in (0, 1):
        got = S.scale_init_reference(P53, -4, 3, axis, 2, "mse")
        absmax = S.scale_init_reference(P53, -4, 3, axis, 2, "absmax")["s"]
        for idx in np.ndindex(got["s"].shape):
            g, line = (idx[0], idx[1]) if axis == 0 else (idx[1], idx[0])
            xs = (P53[:, line] if axis == 0 else P53[line, :])[2 * g:2 * g + 2]
            raw = float(absmax[idx]) if (xs != 0).any() else 0.0
            rows = _mse_by_hand([float(x) for x in xs], -4, 3, "floor", raw)
            k = min(range(28), key=lambda i: (rows[i][1], i))
            assert int(got["k"][idx]) == k and float(got["s"][idx]) == rows[k][0], (axis, idx)


# floor, by hand: s = (27/32) s0 = 0.84375: quotients -1.19 -> -2 and 3.56 -> 3, out -1.6875 and 2.53125, E = 0.6875^2 + 0.46875^2
# = 0.6924; its neighbours k = 4 (s = 0.875: 0.75^2 + 0.375^2 = 0.7031) and k = 6 (s = 0.8125: 0.625^2 + 0.5625^2 = 0.7070) are worse
MSE_K_FLOOR = 5


def test_reference_special_groups():
    P = np.array(P53)
    P[0, 0] = np.nan
    P[4, 2] = np.inf
    for method in S.METHODS:
        clean = S.scale_init_reference(P53, -4, 3, 0, 2, method)["s"]
        got = S.scale_init_reference(P, -4, 3, 0, 2, method)
        assert np.isnan(got["s"][0, 0]) and np.isnan(got["s"][2, 2]) and int(got["bad"].sum()) == 2
        keep = ~got["bad"]
        assert bits_equal(got["s"][keep], clean[keep])
        assert clean[0, 2] == np.float32(MV)                      # the group of zeros


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_abi_version_stays_3():
    assert _hip.load().lq_version() == 3            # an addition only


def test_entry_point_is_declared_exported_and_bound():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    assert "lq_scale_init_group" in declared and hasattr(lib, "lq_scale_init_group") and "lq_scale_init_group" in _hip.SIGNATURES
    assert re.search(r"LQ_INIT_ABSMAX = 0, LQ_INIT_LSQ = 1, LQ_INIT_MSE = 2", header)
    assert lq.scale_init_group is ops.scale_init_group and lq.SCALE_INITS == ("absmax", "lsq", "mse") == S.METHODS
    assert lq.init_geometry is init_geometry and ops.SCALE_INIT == lq.SCALE_INIT == MV
    doc = header[header.index("scale initialisation:"):header.index("int lq_scale_init_group")]
    for needle in ("1 + 2^-22", "c_k = (32 - k) / 32", "smallest k wins", "s = NaN", "min_value", "no\n * workspace", "LQ_EINVAL",
                   "LQ_EALIGN", "sqrt((double)qp)"):
        assert needle in doc, needle


def test_validation_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    fn = lib.lq_scale_init_group
    ok = (-8, 7, 0, 0, MV)
    geo = (5, 3, 0, 2, None)
    assert fn(None, p, *ok, *geo) == LQ_EINVAL and "'P' is NULL" in _err()
    assert fn(p, None, *ok, *geo) == LQ_EINVAL and "'s' is NULL" in _err()
    assert fn(p, p, 8, 7, 0, 0, MV, *geo) == LQ_EINVAL and "qmin 8 > qmax 7" in _err()
    assert fn(p, p, -LIM - 1, 7, 0, 0, MV, *geo) == LQ_EINVAL and "outside +-2^24" in _err()
    assert fn(p, p, -8, LIM + 1, 0, 0, MV, *geo) == LQ_EINVAL and "outside +-2^24" in _err()
    for bad in (-1, 2, 7):
        for method in (0, 1, 2):             # validated for every method
            assert fn(p, p, -8, 7, bad, method, MV, *geo) == LQ_EINVAL and "bad rounding" in _err()
    for bad in (-1, 3, 99):
        assert fn(p, p, -8, 7, 0, bad, MV, *geo) == LQ_EINVAL and "bad method" in _err()
    for bad in (0.0, -1e-5, float("inf"), float("nan")):
        assert fn(p, p, -8, 7, 0, 0, bad, *geo) == LQ_EINVAL and "min_value" in _err()
    for gs in (0, -3):
        assert fn(p, p, *ok, 5, 3, 0, gs, None) == LQ_EINVAL and "group size" in _err()
    for axis in (-1, 2):
        assert fn(p, p, *ok, 5, 3, axis, 2, None) == LQ_EINVAL and "bad axis" in _err()
    for R, C in ((0, 3), (5, 0), (-1, 3)):
        assert fn(p, p, *ok, R, C, 0, 2, None) == LQ_EINVAL and "extents must be positive" in _err()
    for R, C in ((1 << 20, 1 << 11), (1 << 31, 1)):
        assert fn(p, p, *ok, R, C, 1, 2, None) == LQ_EINVAL and "not below 2^31" in _err()
    assert fn(p + 2, p, *ok, *geo) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert fn(p, p + 1, *ok, *geo) == LQ_EALIGN and "not 4-byte aligned" in _err()


# ------------------------------------------------------------------------------------------------------------ init_geometry
def _oihw(kh, kw, ci, co):
    return torch.empty(co, ci, kh, kw).permute(2, 3, 1, 0)          # HWIO shape, OIHW memory


def test_init_geometry_every_orientation():
    w = torch.empty(20, 6)                                           # Dense (in, out)
    assert init_geometry(w.shape, w.stride(), (20, 1)) == (20, 6, 1, 6)            # rowwise: every row a group
    assert init_geometry(w.shape, w.stride(), (1, 6)) == (20, 6, 0, 20)            # columnwise: every column a group
    assert init_geometry(w.shape, w.stride(), (1,)) == (1, 120, 1, 120)            # scalar
    assert init_geometry(w.shape, w.stride(), (5, 6), 4) == (20, 6, 0, 4)          # groupwise
    assert init_geometry(w.shape, w.stride(), lq.scale_shape(w.shape, "channelwise")) == (1, 120, 1, 120)      # no axis 2: one group
    b = torch.empty(6)                                               # bias
    assert init_geometry(b.shape, b.stride(), (1,)) == (1, 6, 1, 6)
    assert init_geometry(b.shape, b.stride(), (6,)) == (6, 1, 1, 1)                # rowwise on a vector: one scale per element
    k = _oihw(3, 3, 4, 8)                                            # conv kernel, default OIHW storage
    assert init_geometry(k.shape, k.stride(), (1,)) == (1, 288, 1, 288)
    assert init_geometry(k.shape, k.stride(), (8, 3), 16) == (8, 36, 1, 16)        # groupwise
    # channelwise (the reference's axis 2 = ci): in OIHW memory the groups are co runs of kh * kw per channel -- not lines
    with pytest.raises(ValueError, match="not lines of a matrix"):
        init_geometry(k.shape, k.stride(), (1, 1, 4, 1))
    with pytest.raises(ValueError, match="not lines of a matrix"):   # the reference's row-wise scale of a 4-D kernel (kh)
        init_geometry(k.shape, k.stride(), (3, 1, 1, 1))
    # its column-wise scale (kw) is the fastest axis of OIHW memory: columns of the [co * ci * kh][kw] matrix
    assert init_geometry(k.shape, k.stride(), (1, 3, 1, 1)) == (96, 3, 0, 96)
    one =_oihw(3, 3, 1, 8)                                          # a single input channel: channelwise is one group
    assert init_geometry(one.shape, one.stride(), (1, 1, 1, 1)) == (1, 72, 1, 72)
    h = torch.empty(3, 3, 4, 8)                                      # conv kernel, HWIO storage
    assert init_geometry(h.shape, h.stride(), (1,)) == (1, 288, 1, 288)
    assert init_geometry(h.shape, h.stride(), (3, 1, 1, 1)) == (3, 96, 1, 96)      # rowwise (kh): rows of the memory matrix
    for scale in ((1, 3, 1, 1), (1, 1, 4, 1)):                       # columnwise (kw), channelwise (ci) on HWIO storage
        with pytest.raises(ValueError, match="not lines of a matrix"):
            init_geometry(h.shape, h.stride(), scale)
    with pytest.raises(ValueError, match="memory order"):                          # group-wise scales need OIHW storage
        init_geometry(h.shape, h.stride(), (8, 3), 16)
    with pytest.raises(ValueError, match="dense"):
        init_geometry((4, 4), (8, 1), (4, 1))
    per_co = _oihw(3, 3, 4, 8)                                       # one scale per output channel: rows of the OIHW matrix
    assert init_geometry(per_co.shape, per_co.stride(), (1, 1, 1, 8)) == (8, 36, 1, 36)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_python_surface():
    P, s = torch.zeros(8, 4), torch.ones(2, 4)
    with pytest.raises(ValueError, match="scale_init must be one of"):
        ops.scale_init_group(P, s, -8, 7, 4, "minmax")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # like every other op
        ops.scale_init_group(P, s, -8, 7, 4, "absmax")
    with pytest.raises(ValueError, match="min_value"):
        ops.scale_init_group(P, s, -8, 7, 4, "absmax", min_value=0.0)
    with pytest.raises(ValueError, match="rounding"):
        ops.scale_init_group(P, s, -8, 7, 4, "absmax", rounding="up")
    with pytest.raises(ValueError, match="qmin <= qmax"):
        ops.scale_init_group(P, s, 7, -8, 4, "absmax")
    with pytest.raises(ValueError, match="no bound to scale by"):
        ops.scale_init_group(P, s, 0, 0, 4, "lsq")
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=1)
    plain = lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, scale_gradient="ste")
    with pytest.raises(ValueError, match="needs bits or q_range"):
        plain.nested_q_w_layer.init_scale(plain.W, "absmax")
    with pytest.raises(ValueError, match="needs bits or q_range"):
        plain.init_scales("lsq")
    clipped = lq.CustomDenseLayer(units=3, initializer=init, input_shape=5, scale_gradient="ste", bits=4)
    with pytest.raises(ValueError, match="scale_init must be one of"):
        clipped.init_scales("max")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clipped.init_scales("absmax")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lq.init_scales(torch.nn.Sequential(clipped), "mse")
    with pytest.raises(ValueError, match="scale_init needs bits"):
        lq.build_model("mnist", mode="ste", value=0.0, scale_init="absmax")
    with pytest.raises(ValueError, match="scale_init must be one of"):
        lq.build_model("mnist", mode="ste", value=0.0, bits=4, scale_init="percentile")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                     # a model that was not put on the device
        lq.build_model("mnist", mode="ste", value=0.0, bits=4, scale_init="absmax")
    # the default changes nothing: every scale at the library's initial value
    m = lq.build_model("mnist", mode="ste", value=0.0, bits=4, group_size=64)
    for layer in lq.custom_layers_of(m):
        for _, nested, _ in layer.scale_pairs():
            assert bool((nested.scale == lq.SCALE_INIT).all())


def test_the_drivers_parse_the_flag():
    from learned_quantization_amd.experiment import build_parser as experiment_parser
    from learned_quantization_amd.train import build_parser
    for m in S.METHODS:
        assert build_parser().parse_args(["--mode", "ste", "--bits", "4", "--scale-init", m]).scale_init == m
        args = experiment_parser().parse_args(["--seed", "1", "--orientation", "scalar", "--training", "from_scratch", "--bits", "4",
                                               "--scale-gradient", "ste", "--scale-init", m])
        assert args.scale_init == m
    assert build_parser().parse_args([]).scale_init is None
    assert experiment_parser().parse_args(["--seed", "1", "--orientation", "scalar", "--training", "from_scratch"]).scale_init is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--scale-init", "minmax"])
    import inspect
    from learned_quantization_amd.train import Trainer
    assert inspect.signature(Trainer.__init__).parameters["scale_init"].default is None
    assert inspect.signature(lq.build_model).parameters["scale_init"].default is None


# ------------------------------------------------------------------------------------ conditions on the GPU cases' own inputs
@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_conditions_on_the_inputs_of_the_gpu_cases(geo):
    """What tests/test_gpu_scale_init.py relies on, on the reference alone: nothing clipped after absmax; exact ties of the mse
    choice do occur and are decided by the rule; at most 1 % of a case's groups have a gap in (0, 1e-9]."""
    R, C, axis, gs = geo
    P = S.make_input(*geo)
    assert P.dtype == np.float32 and P.shape == (R, C) and abs(float(P.std()) - 0.05) < 0.01
    for qmin, qmax in S.RANGES:
        absmax = S.case_reference(*geo, qmin, qmax, "absmax")["s"]
        assert np.isfinite(S.case_reference(*geo, qmin, qmax, "lsq")["s"]).all()
        for rounding in S.ROUNDINGS:
            clipped = S.clipped_after(P, absmax, qmin, qmax, axis, gs, rounding)
            if qmin < 0:
                assert not clipped.any(), f"{geo} [{qmin}, {qmax}] {rounding}: {int(clipped.sum())} clipped after absmax"
            else:
                assert not clipped[P >= 0].any()
            ref = S.case_reference(*geo, qmin, qmax, "mse", rounding)
            gap = ref["gap"]
            near = (gap > 0) & (gap <= S.GAP)
            assert near.mean() <= 0.01, f"{geo} [{qmin}, {qmax}] {rounding}: {int(near.sum())} of {gap.size} groups nearly tied"
            assert float(gap[gap > 0].min()) > 2e-8                     # the smallest nonzero gap of these inputs: 4.0e-8
            assert (ref["s"] <= absmax).all() and (ref["s"] >= np.float32(MV)).all()


def test_exact_ties_occur_and_the_rule_decides_them():
    # (130, 1028, 128) under [0, 15]: the short last group of a column has two elements; where both are negative every
    # candidate gives out == 0, all 28 sums are equal, and the smallest k -- the absmax scale, here min_value -- wins
    geo = (130, 1028, 0, 128)
    P = S.make_input(*geo)
    ref = S.case_reference(*geo, 0, 15, "mse", "floor")
    neg = (P[128:] < 0).all(axis=0)
    assert neg.sum() > 100
    assert (ref["gap"][1][neg] == 0).all() and (ref["k"][1][neg] == 0).all() and (ref["s"][1][neg] == np.float32(MV)).all()
