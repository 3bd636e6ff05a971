"""GPU tests of the asymmetric group-wise quantizer (csrc/lq_group.hpp; include/lq_hip.h: lq_fq_forward_group_affine /
lq_fq_backward_group_affine / lq_scale_init_group_minmax) and of everything built on it: the ops, the layers, the Trainer and both
exports.

The reference is tests/_group_affine_reference.py.  The bar: out, the integer views, dP and the clip counts equal it BIT FOR BIT
(NaN positional, the sign of zero kept); ds and db are held to tests/_bounds.py::assert_within_terms, |got - ref| <= 1e-5 *
sum|terms| (floor 2^-136; the terms of db are the |dy| of the clipped elements); two calls give the same bits; min-max scales and
offsets equal the reference bit for bit.  tests/test_group_affine_cpu.py asserts the conditions on these inputs without a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _arena import Arena                                                                         # noqa: E402
from _bounds import assert_within_terms, stable_seed                                             # noqa: E402
from _clip_reference import bits_equal                                                           # noqa: E402
from _group_affine_reference import (edge_affine_case, group_affine_reference, make_affine_case,  # noqa: E402
                                     minmax_center, minmax_reference)
from _group_forms import VARIANTS, WINDOW_SHAPES, form_variants                                  # noqa: E402
from _group_reference import check_condition, expand_scale, group_reference, make_case, scale_shape      # noqa: E402
import _scale_init_reference as S                                                                # noqa: E402

pytestmark = pytest.mark.gpu
ROUNDINGS = ("floor", "nearest")
MV = S.MIN_VALUE
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _counts(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _ratio(got, ref, terms):
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref) / np.maximum(terms, 1e-300)
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0


def _compare(got, ref, what, special=False):
    """got: dict(out, q (float32 view), qi (int32 view), dP, ds, db, clipped) as NumPy arrays; ``special``: NaN / Inf are expected.
    Returns the worst |err| / sum|terms| of ds and of db."""
    assert bits_equal(got["out"], ref["out"]), f"{what}: out"
    assert got["q"] is None or bits_equal(got["q"], ref["q"]), f"{what}: q (float32 view)"
    finite = np.isfinite(ref["q"])
    assert special or finite.all()
    with np.errstate(all="ignore"):
        want_int = np.where(finite, ref["q"], 0).astype(np.int32)
    assert np.array_equal(got["qi"][finite], want_int[finite]), f"{what}: q (int32 view)"
    assert bits_equal(got["dP"], ref["dP"]), f"{what}: dP"
    assert np.array_equal(got["clipped"].reshape(ref["clipped"].shape), ref["clipped"]), f"{what}: clipped"
    worst = []
    for key, terms in (("ds", "terms"), ("db", "terms_b")):
        g, nan = got[key].reshape(ref[key].shape), np.isnan(ref[key])
        assert special or not nan.any()
        assert np.array_equal(np.isnan(g), nan), f"{what}: {key} is NaN in other groups than the reference's"
        keep = ~nan & np.isfinite(ref[key])
        assert np.array_equal(g[~nan & ~keep].astype(np.float64), ref[key][~nan & ~keep]), f"{what}: infinite {key}"
        assert_within_terms(g[keep], ref[key][keep], ref[terms][keep], f"{what}: {key}")
        worst.append(_ratio(g[keep], ref[key][keep], ref[terms][keep]))
    return tuple(worst)


def _affine_pair(dev, P, s, b, dy, geom, qmin, qmax, rounding, k=1.0, kb=1.0):
    """Forward (both integer views) and backward through the C ABI, each called twice: the same bits."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = geom
    rnd, st = ROUNDINGS.index(rounding), _hip.stream_ptr(dev)
    Pt, st_, bt, dt = _t(P, dev), _t(s, dev), _t(b, dev), _t(dy, dev)
    assert Pt.data_ptr() % 16 == 0 and dt.data_ptr() % 16 == 0
    runs = []
    for q_dtype, code in ((torch.float32, _hip.LQ_Q_F32), (torch.int32, _hip.LQ_Q_I32)):
        out, q = torch.empty_like(Pt), torch.empty(Pt.shape, dtype=q_dtype, device=dev)
        dP, ds, db = torch.empty_like(Pt), torch.empty_like(st_), torch.empty_like(st_)
        cnt = torch.empty(st_.shape, dtype=torch.int32, device=dev)
        assert out.data_ptr() % 16 == 0 and dP.data_ptr() % 16 == 0
        _hip.check(lib.lq_fq_forward_group_affine(Pt.data_ptr(), st_.data_ptr(), bt.data_ptr(), out.data_ptr(), q.data_ptr(), code,
                                                  qmin, qmax, rnd, R, C, axis, gs, st), "lq_fq_forward_group_affine")
        _hip.check(lib.lq_fq_backward_group_affine(Pt.data_ptr(), st_.data_ptr(), bt.data_ptr(), dt.data_ptr(), qmin, qmax, rnd,
                                                   float(k), float(kb), dP.data_ptr(), ds.data_ptr(), db.data_ptr(), cnt.data_ptr(),
                                                   None, 0, R, C, axis, gs, st), "lq_fq_backward_group_affine")
        runs.append((out, q, dP, ds, db, cnt))
    (out, q, dP, ds, db, cnt), second = runs
    for name, x, y in zip(("out", "dP", "ds", "db", "clipped"), (out, dP, ds, db, cnt), (second[0],) + second[2:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"two calls differ in {name}"
    return dict(out=out.cpu().numpy(), q=q.cpu().numpy(), qi=second[1].cpu().numpy(), dP=dP.cpu().numpy(), ds=ds.cpu().numpy(),
                db=db.cpu().numpy(), clipped=_counts(cnt))


# ------------------------------------------------------------------------------------------------------------------ 1 forms
@pytest.mark.parametrize("case,variant", form_variants(), ids=lambda v: _ids(v))
def test_forms(dev, case, variant):
    """Every row of _group_forms.FORMS in its variants through the C ABI against the reference, grad_scale 0.75 and
    offset_grad_scale 1.25.  The printed ratios are the ones DESIGN.md quotes."""
    (qmin, qmax), rounding = VARIANTS[variant]
    P, s, b, dy = make_affine_case(stable_seed("affineforms", *case), *case)
    ref = group_affine_reference(P, s, b, dy, qmin, qmax, case[2], case[3], k=0.75, kb=1.25, rounding=rounding)
    check_condition(ref, *case, f"{case} {variant}")
    worst = _compare(_affine_pair(dev, P, s, b, dy, case, qmin, qmax, rounding, k=0.75, kb=1.25), ref, f"{case} {variant}")
    print(f"{case} {variant}: max err / sum|terms|: ds {worst[0]:.3e}, db {worst[1]:.3e}")


# ------------------------------------------------------------------------------------------------------------ 2 zero offset
@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("case", WINDOW_SHAPES + [(5, 1100, 1, 256), (2240, 1030, 0, 32)], ids=_ids)
def test_zero_offset_is_the_symmetric_pair(dev, case, rounding):
    """b == +0: dP, ds and clipped are lq_fq_backward_group's bits on the same buffers, the integer view is identical, out is equal
    as a value and holds no -0; db is the reference's."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = case
    P, s, dy = make_case(stable_seed("affine zero", *case), *case)
    b = np.zeros_like(s)
    got = _affine_pair(dev, P, s, b, dy, case, -8, 7, rounding, k=0.75, kb=0.75)
    Pt, st_, dt = _t(P, dev), _t(s, dev), _t(dy, dev)
    out, q = torch.empty_like(Pt), torch.empty(Pt.shape, dtype=torch.int32, device=dev)
    dP, ds, cnt = torch.empty_like(Pt), torch.empty_like(st_), torch.empty(st_.shape, dtype=torch.int32, device=dev)
    rnd, st = ROUNDINGS.index(rounding), _hip.stream_ptr(dev)
    _hip.check(lib.lq_fq_forward_group(Pt.data_ptr(), st_.data_ptr(), out.data_ptr(), q.data_ptr(), _hip.LQ_Q_I32, -8, 7, rnd,
                                       R, C, axis, gs, st), "lq_fq_forward_group")
    _hip.check(lib.lq_fq_backward_group(Pt.data_ptr(), st_.data_ptr(), dt.data_ptr(), -8, 7, rnd, 0.75, dP.data_ptr(), ds.data_ptr(),
                                        cnt.data_ptr(), None, 0, R, C, axis, gs, st), "lq_fq_backward_group")
    assert bits_equal(got["dP"], dP.cpu().numpy()) and bits_equal(got["ds"], ds.cpu().numpy())
    assert np.array_equal(got["clipped"], _counts(cnt)) and np.array_equal(got["qi"], q.cpu().numpy())
    sym = out.cpu().numpy()
    assert np.array_equal(got["out"], sym) and not np.signbit(got["out"][got["out"] == 0]).any()
    ref = group_affine_reference(P, s, b, dy, -8, 7, axis, gs, k=0.75, kb=0.75, rounding=rounding)
    _compare(got, ref, f"{case} {rounding} b = 0")


# ------------------------------------------------------------------------------------------------------------ 3 range edges
@pytest.mark.parametrize("range_", [(-8, 7), (0, 15)], ids=_ids)
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_range_edges_at_power_of_two_scales(dev, rounding, range_):
    """Power-of-two scales, offsets that are multiples of the scale: the quotients are exactly lo, hi, hi + 1, the ties lo - 1/2
    and hi + 1/2, and lo + 1; one shape per form."""
    qmin, qmax = range_
    for case in WINDOW_SHAPES:
        P, s, b, dy, want_q0 = edge_affine_case(stable_seed("affine edge", case), *case, qmin, qmax, rounding)
        ref = group_affine_reference(P, s, b, dy, qmin, qmax, case[2], case[3], rounding=rounding)
        assert np.array_equal(ref["q0"], want_q0) and 0 < int(ref["clipped"].sum()) < P.size
        got = _affine_pair(dev, P, s, b, dy, case, qmin, qmax, rounding)
        _compare(got, ref, f"{case} [{qmin}, {qmax}] {rounding}")
        sb, bb = expand_scale(s, *case), expand_scale(b, *case)
        assert np.array_equal(got["out"], np.clip(want_q0, qmin, qmax) * sb + bb)
        inside = (want_q0 >= qmin) & (want_q0 <= qmax)
        assert bits_equal(got["dP"], np.where(inside, dy, np.float32(0.0))) and not np.signbit(got["dP"][~inside]).any()


# -------------------------------------------------------------------------------------- 4 misaligned bases, guards, optional outputs
_RAW = {}


def _raw_inputs(case):
    if case not in _RAW:
        P, s, b, dy = make_affine_case(stable_seed("affine raw", *case), *case)
        _RAW[case] = (P, s, b, dy, group_affine_reference(P, s, b, dy, -8, 7, case[2], case[3]))
    return _RAW[case]


def _raw_case(dev, case, residue, want_ds=True, want_db=True, want_clipped=True):
    """Forward and backward through the C ABI with every dense tensor ``residue`` bytes off the 16-byte grid, each region between
    guard bands: the results equal the reference, every requested output is fully written, nothing else is touched."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = case
    P, s, b, dy, ref = _raw_inputs(case)
    nbytes, row = P.nbytes, C * 4
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=residue, row_bytes=row)
    ar.add("s", "in", data=s)
    ar.add("b", "in", data=b)
    ar.add("dy", "in", data=dy, residue=residue, row_bytes=row)
    ar.add("out", "out", nbytes=nbytes, residue=residue, row_bytes=row)
    ar.add("q", "out", nbytes=nbytes)
    ar.add("dP", "out", nbytes=nbytes, residue=residue, row_bytes=row)
    ar.add("ds", "out", nbytes=s.nbytes)
    ar.add("db", "out", nbytes=s.nbytes)
    ar.add("clipped", "out", nbytes=s.nbytes)
    ar.build()
    assert ar.ptr("P") % 16 == residue and ar.ptr("dy") % 16 == residue and ar.ptr("out") % 16 == residue and ar.ptr("dP") % 16 == residue
    assert lib.lq_group_workspace_bytes(R, C, axis, gs) == 0
    st = _hip.stream_ptr(dev)
    _hip.check(lib.lq_fq_forward_group_affine(ar.ptr("P"), ar.ptr("s"), ar.ptr("b"), ar.ptr("out"), ar.ptr("q"), _hip.LQ_Q_I32, -8, 7, 0,
                                              R, C, axis, gs, st), "lq_fq_forward_group_affine")
    _hip.check(lib.lq_fq_backward_group_affine(ar.ptr("P"), ar.ptr("s"), ar.ptr("b"), ar.ptr("dy"), -8, 7, 0, 1.0, 1.0, ar.ptr("dP"),
                                               ar.ptr("ds") if want_ds else None, ar.ptr("db") if want_db else None,
                                               ar.ptr("clipped") if want_clipped else None, None, 0, R, C, axis, gs, st),
               "lq_fq_backward_group_affine")
    torch.cuda.synchronize(dev)
    written = ["out", "q", "dP"] + [n for n, w in (("ds", want_ds), ("db", want_db), ("clipped", want_clipped)) if w]
    ar.check(f"{case} residue {residue} ds {want_ds} db {want_db} clipped {want_clipped}", written=written)
    assert bits_equal(ar.numpy("out", np.float32).reshape(R, C), ref["out"])
    assert np.array_equal(ar.numpy("q", np.int32).reshape(R, C), ref["q"].astype(np.int32))
    assert bits_equal(ar.numpy("dP", np.float32).reshape(R, C), ref["dP"])
    if want_ds:
        assert_within_terms(ar.numpy("ds", np.float32), ref["ds"], ref["terms"], "ds")
    if want_db:
        assert_within_terms(ar.numpy("db", np.float32), ref["db"], ref["terms_b"], "db")
    if want_clipped:
        assert np.array_equal(ar.numpy("clipped", np.uint32).astype(np.int64).reshape(s.shape), ref["clipped"])
    return {n: ar.numpy(n, np.uint32).copy() for n in written}


RAW_CASES = [(37, 5, 0, 8), (256, 260, 0, 32), (7, 27, 1, 8), (64, 576, 1, 128)]


@pytest.mark.parametrize("case", RAW_CASES, ids=_ids)
def test_misaligned_base(dev, case):
    """P, dy, out and dP one float off the 16-byte grid: the scalar forms, the reference's results, two runs the same bits -- and
    dP, the counts and the integers are the aligned run's bits (ds and db may differ in the last bit: another summation order)."""
    a, b2 = _raw_case(dev, case, residue=4), _raw_case(dev, case, residue=4)
    for name in a:
        assert np.array_equal(a[name], b2[name]), f"two runs differ in {name}"
    al = _raw_case(dev, case, residue=0)
    for name in ("out", "q", "dP", "clipped"):
        assert np.array_equal(a[name], al[name]), name


@pytest.mark.parametrize("case", RAW_CASES, ids=_ids)
def test_guard_bands_and_optional_outputs(dev, case):
    """Aligned bases between guard bands, every combination of ds, db and clipped being NULL (both gradients NULL: mask only): a
    region that was not asked for keeps the sentinel in every byte, the others hold the full run's bits."""
    full = _raw_case(dev, case, residue=0)
    again = _raw_case(dev, case, residue=0)
    for name in full:
        assert np.array_equal(full[name], again[name]), f"two runs differ in {name}"
    for want_ds in (True, False):
        for want_db in (True, False):
            for want_clipped in (True, False):
                if want_ds and want_db and want_clipped:
                    continue
                part = _raw_case(dev, case, residue=0, want_ds=want_ds, want_db=want_db, want_clipped=want_clipped)
                for name in part:
                    assert np.array_equal(part[name], full[name]), f"{name} with ds {want_ds} db {want_db} clipped {want_clipped}"


# -------------------------------------------------------------------------------------------------------- 5 special values
@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("case", RAW_CASES, ids=_ids)
def test_nan_and_inf_stay_in_their_groups(dev, case, rounding):
    """NaN and +Inf planted in P, NaN in one scale, NaN and -Inf in one offset each: five groups are spoiled as the reference's IEEE
    arithmetic says, every other group is the clean case's bit for bit."""
    R, C, axis, gs = case
    P, s, b, dy, _ = _raw_inputs(case)
    clean = _affine_pair(dev, P, s, b, dy, case, -8, 7, rounding)
    P, s, b = P.copy(), s.copy(), b.copy()
    group_of = lambda r, c: (r // gs, c) if axis == 0 else (r, c // gs)      # noqa: E731
    nb = s.shape[axis]
    assert nb >= 4 and min(s.shape) >= 2
    P[1, 2], P[R - 1, C - 1] = np.nan, np.inf                               # first group of a line and the (ragged) last one
    spoiled = {group_of(1, 2), group_of(R - 1, C - 1)}
    picks = [(1, 0), (2, 1), (nb - 2, 1)] if axis == 0 else [(0, 1), (1, 2), (2, nb - 1)]
    picks = [g for g in picks if g not in spoiled][:3]
    assert len(picks) == 3 and len(set(picks)) == 3
    s[picks[0]], b[picks[1]], b[picks[2]] = np.nan, np.nan, -np.inf
    spoiled |= set(picks)
    with np.errstate(all="ignore"):
        ref = group_affine_reference(P, s, b, dy, -8, 7, axis, gs, rounding=rounding)
    assert np.isnan(ref["ds"][group_of(1, 2)]) and np.isnan(ref["ds"][picks[0]]) and np.isnan(ref["ds"][picks[1]])
    assert np.isnan(ref["db"][picks[1]]) or int(ref["clipped"][picks[1]]) > 0
    got = _affine_pair(dev, P, s, b, dy, case, -8, 7, rounding)
    _compare(got, ref, f"{case} {rounding}", special=True)
    keep = np.ones(s.shape, bool)
    for g in spoiled:
        keep[g] = False
    for key in ("ds", "db", "clipped"):
        assert np.array_equal(got[key].reshape(s.shape).view(np.uint32 if key != "clipped" else np.int64)[keep],
                              clean[key].reshape(s.shape).view(np.uint32 if key != "clipped" else np.int64)[keep]), key
    keep_el = expand_scale(keep.astype(np.float32), R, C, axis, gs) > 0
    for key in ("out", "dP"):
        assert np.array_equal(got[key].view(np.uint32)[keep_el], clean[key].view(np.uint32)[keep_el]), key


# ---------------------------------------------------------------------------------------------------------------- 6 min-max
def _minmax(dev, P, geom, qmin, qmax, rounding, min_value=MV):
    """lq_scale_init_group_minmax through the C ABI on a fresh device copy of P; s and b start as NaN (an unwritten element shows)."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = geom
    p = _t(P, dev)
    shape = scale_shape(R, C, axis, min(gs, R if axis == 0 else C))
    s = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    b = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    _hip.check(lib.lq_scale_init_group_minmax(_hip.ptr(p), _hip.ptr(s), _hip.ptr(b), qmin, qmax, ROUNDINGS.index(rounding), min_value,
                                              R, C, axis, gs, _hip.stream_ptr(dev)), "lq_scale_init_group_minmax")
    return p, s, b


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("geom", S.GEOMETRIES, ids=_ids)
def test_minmax_matches_the_reference_and_clips_nothing(dev, geom, rounding):
    import learned_quantization_amd as lq
    R, C, axis, gs = geom
    P = S.make_input(*geom)
    g = min(gs, R if axis == 0 else C)
    for qmin, qmax in S.RANGES:
        ref = minmax_reference(P, qmin, qmax, axis, gs, rounding=rounding)
        p, s, b = _minmax(dev, P, geom, qmin, qmax, rounding)
        assert bits_equal(s.cpu().numpy(), ref["s"]) and bits_equal(b.cpu().numpy(), ref["b"]), f"{geom} [{qmin}, {qmax}] {rounding}"
        p2, s2, b2 = _minmax(dev, P, geom, qmin, qmax, rounding)
        assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(b.view(torch.int32), b2.view(torch.int32))
        _, _, _, clipped = lq.fq_backward_group_affine(p, s, b, torch.zeros_like(p), qmin, qmax, g, want_ds=False, want_db=False,
                                                       want_clipped=True, rounding=rounding)
        assert int(clipped.sum()) == 0, f"{geom} [{qmin}, {qmax}] {rounding}: {int(clipped.sum())} elements clipped after minmax"


@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("geom", RAW_CASES, ids=_ids)
def test_minmax_special_groups_and_one_sided_data(dev, geom, rounding):
    """Zero-spread, NaN and Inf groups as specified; on one-sided data (|N(0, 1)| * 0.05) the squared error of the min-max
    initialised asymmetric quantizer is not above that of the absmax-initialised symmetric one, group by group."""
    import learned_quantization_amd as lq
    R, C, axis, gs = geom
    P = np.array(S.make_input(*geom))
    group_of = lambda r, c: (r // gs, c) if axis == 0 else (r, c // gs)      # noqa: E731
    P[0, 1], P[R - 1, C - 1], P[R // 2, 0] = np.nan, np.inf, -np.inf
    bad = {group_of(0, 1), group_of(R - 1, C - 1), group_of(R // 2, 0)}
    flat = (1, 3) if axis == 0 else (3, 1)                                   # a group of equal values, away from the bad ones
    assert flat not in bad
    if axis == 0:
        P[flat[0] * gs:(flat[0] + 1) * gs, flat[1]] = np.float32(0.125)
    else:
        P[flat[0], flat[1] * gs:(flat[1] + 1) * gs] = np.float32(0.125)
    ref = minmax_reference(P, -8, 7, axis, gs, rounding=rounding)
    _, s, b = _minmax(dev, P, geom, -8, 7, rounding)
    s, b = s.cpu().numpy(), b.cpu().numpy()
    assert bits_equal(s, ref["s"]) and bits_equal(b, ref["b"])
    want_nan = np.zeros(s.shape, bool)
    for g in bad:
        want_nan[g] = True
    assert np.array_equal(np.isnan(s), want_nan) and np.array_equal(np.isnan(b), want_nan)
    assert s[flat] == np.float32(MV) and b[flat] == np.float32(0.125) - minmax_center(-8, 7, rounding) * np.float32(MV)
    # one-sided data against the symmetric layer under absmax
    A = np.abs(np.array(S.make_input(*geom)))
    p, s, b = _minmax(dev, A, geom, -8, 7, rounding)
    out_a = lq.fq_forward_group_affine(p, s, b, -8, 7, gs, rounding=rounding).cpu().numpy()
    s_sym = lq.scale_init_group(p, torch.empty_like(s), -8, 7, gs, "absmax", rounding=rounding)
    out_s = lq.fq_forward_group(p, s_sym, -8, 7, gs, rounding=rounding).cpu().numpy()
    # per tensor, not per group: the asymmetric step is about half the symmetric one (max - min over 15 codes against max over 7),
    # which wins by about 4 x in the sum, but a ragged group of three elements has one free element against two and can lose
    e_a, e_s = S.squared_error(A, out_a, axis, gs).sum(), S.squared_error(A, out_s, axis, gs).sum()
    print(f"{geom} {rounding}: squared error, asymmetric minmax / symmetric absmax = {e_a / e_s:.3f}")
    assert e_a <= e_s, f"min-max is worse than symmetric absmax: {e_a} > {e_s}"


# ------------------------------------------------------------------------------------------------------- 7 autograd and layers
def _load(param_view, nested, P, s, b, dev):
    with torch.no_grad():
        param_view.copy_(_t(P, dev))
        nested.scale.copy_(_t(s, dev))
        nested.offset.copy_(_t(b, dev))


@pytest.mark.parametrize("grad_scale", [1.0, "rsqrt_group"])
def test_dense_layer(dev, grad_scale):
    """Dense 784 x 128, gs = 64 (axis 0, scale and offset (13, 128)): forward and backward against the reference, offset.grad
    included, scaled like the scale's."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomDenseLayer(units=128, orientation="groupwise", group_size=64, initializer=lq.RandomNormal(seed=5), input_shape=784,
                                device=dev, scale_gradient="ste", grad_scale=grad_scale, bits=4, asymmetric=True)
    nested = layer.nested_q_w_layer
    assert tuple(nested.scale.shape) == tuple(nested.offset.shape) == (13, 128) and bool((nested.offset == 0).all())
    assert layer.nested_q_b_layer.offset is None and tuple(layer.nested_q_b_layer.scale.shape) == (1,)
    assert nested.offset.lq_is_scale and nested.offset.lq_is_offset and not hasattr(nested.offset, "lq_constraint")
    assert id(nested.offset) in {id(p) for p in lq.scale_parameters(layer)}
    assert id(nested.offset) not in {id(p) for p in lq.non_scale_parameters(layer)}
    k = 1.0 if grad_scale == 1.0 else 1.0 / np.sqrt(784 * 128 / (13 * 128))
    P, s, b, dy = make_affine_case(stable_seed("affine dense"), 784, 128, 0, 64)
    ref = group_affine_reference(P, s, b, dy, -8, 7, 0, 64, k=k, kb=k)
    _load(layer.W, nested, P, s, b, dev)
    qw = layer.quantized_parameters()[0]
    assert bits_equal(qw.detach().cpu().numpy(), ref["out"])
    (qw * _t(dy, dev)).sum().backward()
    assert bits_equal(layer.W.grad.cpu().numpy(), ref["dP"])
    assert_within_terms(nested.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], f"dense ds, grad_scale {grad_scale}")
    assert_within_terms(nested.offset.grad.cpu().numpy(), ref["db"], ref["terms_b"], f"dense db, grad_scale {grad_scale}")
    assert np.array_equal(nested.quantized_integers(layer.W.data, torch.int32).cpu().numpy(), ref["q"].astype(np.int32))
    x = torch.ones(3, 784, device=dev)
    assert torch.equal(layer(x), torch.matmul(x, nested(layer.W)) + layer.nested_q_b_layer(layer.b))


def test_conv_layer(dev):
    """Conv 3 x 3 x 16 x 32 stored OIHW, gs = 32 (axis 1, C = 144 = 4.5 groups, scale and offset (32, 5))."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomConv2DLayer(filters=32, orientation="groupwise", group_size=32, initializer=lq.RandomNormal(seed=6), input_shape=16,
                                 device=dev, scale_gradient="ste", bits=4, asymmetric=True, rounding="nearest")
    nested = layer.nested_q_k_layer
    assert tuple(layer.kernel.shape) == (3, 3, 16, 32) and tuple(nested.scale.shape) == tuple(nested.offset.shape) == (32, 5)
    P, s, b, dy = make_affine_case(stable_seed("affine conv"), 32, 144, 1, 32)
    ref = group_affine_reference(P, s, b, dy, -8, 7, 1, 32, rounding="nearest")
    oihw = lambda a: a.reshape(32, 16, 3, 3)                                      # noqa: E731  the memory-order matrix as OIHW
    _load(layer.kernel.data.permute(3, 2, 0, 1), nested, oihw(P), s, b, dev)
    w = layer.quantized_parameters()[0]
    assert tuple(w.shape) == (32, 16, 3, 3) and w.is_contiguous()
    assert bits_equal(w.detach().cpu().numpy().reshape(32, 144), ref["out"])
    (w * _t(oihw(dy), dev)).sum().backward()
    assert bits_equal(layer.kernel.grad.permute(3, 2, 0, 1).contiguous().cpu().numpy().reshape(32, 144), ref["dP"])
    assert_within_terms(nested.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], "conv ds")
    assert_within_terms(nested.offset.grad.cpu().numpy(), ref["db"], ref["terms_b"], "conv db")
    q = nested.quantized_integers(layer.kernel.data, torch.int32).permute(3, 2, 0, 1).contiguous().cpu().numpy().reshape(32, 144)
    assert np.array_equal(q, np.where(ref["q"] == 0, 0, ref["q"]).astype(np.int32))
    y = layer(torch.ones(2, 16, 8, 8, device=dev))
    assert tuple(y.shape) == (2, 32, 8, 8) and bool(torch.isfinite(y).all())


def test_layer_scale_init(dev):
    """layers.init_scales on asymmetric layers: "minmax" writes scale and offset of the kernel (the reference's bits, nothing
    clipped) and absmax for the bias; "absmax" writes the scale as for a symmetric layer and leaves the offset at zero."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    model = lq.build_model("mnist", seed=3, mode="ste", value=0.0, bits=4, group_size=64, device=dev, asymmetric=True, scale_init="minmax")
    sym = lq.build_model("mnist", seed=3, mode="ste", value=0.0, bits=4, group_size=64, device=dev, scale_init="absmax")
    for layer, twin in zip(lq.custom_layers_of(model), lq.custom_layers_of(sym)):
        nested = layer.nested_q_w_layer
        W = layer.W.detach().cpu().numpy()
        ref = minmax_reference(W, -8, 7, 0, 64)
        assert bits_equal(nested.scale.detach().cpu().numpy(), ref["s"]) and bits_equal(nested.offset.detach().cpu().numpy(), ref["b"])
        clipped = lq.fq_backward_group_affine(layer.W.data, nested.scale.data, nested.offset.data, torch.zeros_like(layer.W.data), -8, 7, 64,
                                              want_ds=False, want_db=False, want_clipped=True)[3]
        assert int(clipped.sum()) == 0
        assert torch.equal(layer.nested_q_b_layer.scale.detach(), twin.nested_q_b_layer.scale.detach())      # the bias: absmax
        with torch.no_grad():
            nested.offset.fill_(1.0)
        layer.init_scales("absmax")
        assert torch.equal(nested.scale.detach(), twin.nested_q_w_layer.scale.detach()) and bool((nested.offset == 0).all())
    with pytest.raises(ValueError, match="symmetric"):
        lq.init_scales(sym, "minmax")


# ------------------------------------------------------------------------------------------------------------------ 8 graph
def test_forward_and_backward_from_a_graph(dev):
    """Forward and backward of an asymmetric Dense layer and conv kernel recorded on one stream and replayed == the eager results."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    dense = lq.CustomDenseLayer(units=24, orientation="groupwise", group_size=16, initializer=lq.RandomNormal(seed=8), input_shape=50,
                                device=dev, scale_gradient="ste", bits=4, asymmetric=True)
    conv = lq.CustomConv2DLayerNoBias(filters=8, orientation="groupwise", group_size=32, initializer=lq.RandomNormal(seed=9),
                                      input_shape=5, device=dev, scale_gradient="ste", bits=4, asymmetric=True)
    P, s, b, _ = make_affine_case(8, 50, 24, 0, 16)
    _load(dense.W, dense.nested_q_w_layer, P, s, b, dev)
    P, s, b, _ = make_affine_case(9, 8, 45, 1, 32)
    _load(conv.kernel.data.permute(3, 2, 0, 1), conv.nested_q_k_layer, P.reshape(8, 5, 3, 3), s, b, dev)
    with torch.no_grad():
        dense.nested_q_b_layer.scale.fill_(2.0 ** -6)
    rng = np.random.default_rng(8)
    x = _t(rng.standard_normal((16, 50), dtype=np.float32), dev)
    cw = _t(rng.standard_normal((16, 24), dtype=np.float32), dev)
    ck = _t(rng.standard_normal((8, 5, 3, 3), dtype=np.float32), dev)
    params = [dense.W, dense.b, dense.nested_q_w_layer.scale, dense.nested_q_w_layer.offset, dense.nested_q_b_layer.scale, conv.kernel,
              conv.nested_q_k_layer.scale, conv.nested_q_k_layer.offset]

    def run():
        y = dense(x)
        w = conv.quantized_parameters()[0]
        return (y, w) + torch.autograd.grad((y * cw).sum() + (w * ck).sum(), params)

    eager = [t.detach().clone() for t in run()]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        for i, (a, c) in enumerate(zip(eager, captured)):
            assert torch.equal(a, c.detach()), f"result {i}: replay differs from the eager result"
    assert bool((eager[2] == 0).any()) and bool((eager[2] != 0).any())            # the mask is at work
    assert bool((eager[5] != 0).any()) and bool((eager[9] != 0).any())            # offsets have gradients


# ---------------------------------------------------------------------------------------------------------------- 9 harness
def _fixed_task_trainer(dev, log_dir, graph):
    """tests/_linear_task.py's trainer with ONE coefficient set: every step differentiates the same functional, so the step can
    be captured (the class itself refuses graph=True because it picks the step's coefficients on the host)."""
    from _linear_task import LinearTaskTrainer, make_coefficients
    from learned_quantization_amd.train import Trainer

    class FixedTask(LinearTaskTrainer):
        def __init__(self, *a, **kw):
            Trainer.__init__(self, *a, **kw)
            self.coefficients, self._n = None, 0

    tr = FixedTask(config="mnist", mode="ste", value=0.0, device=dev, log_dir=log_dir, graph=graph, seed=7, bits=4, group_size=64,
                   asymmetric=True, scale_init="minmax", lr=1e-3)
    tr.coefficients = make_coefficients(tr, 1, seed=7, lo=-3.0, hi=-1.0)
    return tr


def test_trainer_eager_and_graphed(dev, tmp_path):
    """Trainer(config="mnist", mode="ste", bits=4, group_size=64, asymmetric=True, scale_init="minmax") on injected gradients:
    three eager and three graphed steps from the same state agree bit for bit, every parameter included; offsets and scales move."""
    runs = []
    x = torch.zeros(2, 1, 28, 28, device=dev)
    y = torch.zeros(2, dtype=torch.long, device=dev)
    for graph in (False, True):
        tr = _fixed_task_trainer(dev, str(tmp_path / ("graph" if graph else "eager")), graph)
        start = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        step = tr.step_graphed if graph else tr.step
        losses = [step(x, y).detach().clone() for _ in range(3 + (0 if graph else 3))]      # step_graphed: 3 eager warm-up steps first
        torch.cuda.synchronize()
        runs.append((tr, losses[-3:], start))
    (eager, le, start), (graphed, lg, _) = runs
    assert all(np.isfinite(float(a)) for a in le)
    for a, c in zip(le, lg):
        assert torch.equal(a, c), f"losses differ: {float(a)!r} {float(c)!r}"
    for (n, p), (_, p2) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), n
    for layer in eager.custom_layers:
        nested = layer.nested_q_w_layer
        names = {id(p): n for n, p in eager.model.named_parameters()}
        b0, s0 = start[names[id(nested.offset)]], start[names[id(nested.scale)]]
        moved_b, moved_s = int((nested.offset.detach() != b0).sum()), int((nested.scale.detach() != s0).sum())
        print(f"{layer.name}: {moved_b} of {b0.numel()} offsets and {moved_s} scales moved")
        assert nested.offset.grad is not None and moved_b > 0 and moved_s > 0


def test_the_cli_line_runs(dev):
    from learned_quantization_amd import train
    train.main(["--config", "mnist", "--mode", "ste", "--bits", "4", "--group-size", "64", "--asymmetric", "--scale-init", "minmax",
                "--batch", "32", "--steps", "2", "--warmup", "1"])


def test_refusals_on_the_device(dev, tmp_path):
    """What needs a built model to be refused: both multi-tensor batches and data-parallel mode B over asymmetric layers."""
    import learned_quantization_amd as lq
    from learned_quantization_amd.train import Trainer
    lq.reset_layer_names()
    model = lq.build_model("mnist", seed=3, mode="ste", value=0.0, bits=4, group_size=64, device=dev, asymmetric=True)
    for kw in (dict(clipped=True), dict(group_batch=True)):
        with pytest.raises(ValueError, match="asymmetric"):
            lq.FakeQuantBatch(model, **kw)
    with pytest.raises(ValueError, match="mode 'B'"):
        lq.DataParallel(model, mode="B")
    for kw in (dict(batched=True, group_batch=True), dict(batched=True, clipped_batch=True), dict(ddp_mode="B")):
        with pytest.raises(ValueError, match="asymmetric"):
            Trainer(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path), bits=4, group_size=64, asymmetric=True, **kw)


# ----------------------------------------------------------------------------------------------------------------- 10 export
def _shake(model, dev, seed):
    """Offsets and scales off their initial values, so that a restore that dropped either would show."""
    import learned_quantization_amd as lq
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for layer in lq.custom_layers_of(model):
            nested = layer.weight_nested()
            f = rng.uniform(0.8, 1.25, tuple(nested.scale.shape)).astype(np.float32)
            nested.scale.mul_(torch.from_numpy(f).to(dev))
            nested.offset.add_(nested.scale * torch.from_numpy(rng.uniform(-2, 2, tuple(nested.scale.shape)).astype(np.float32)).to(dev))


@pytest.mark.parametrize("config,gs,rounding", [("mnist", 64, "floor"), ("cifar", 128, "floor"), ("cifar", 128, "nearest")])
def test_export_round_trips(dev, tmp_path, config, gs, rounding):
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    from learned_quantization_amd.models import INPUT_SHAPES
    kw = dict(mode="ste", value=0.0, device=dev, bits=4, group_size=gs, rounding=rounding)
    lq.reset_layer_names()
    model = lq.build_model(config, seed=3, asymmetric=True, scale_init="minmax", **kw)
    _shake(model, dev, 3)
    tensors = export.quantized_tensors(model)
    d = str(tmp_path)
    # the reference-format int8 file: the clamped integers of the affine view
    lq.save_compress_parameters(model, d)
    weights = np.load(os.path.join(d, "weights.npy"), allow_pickle=True).item()
    n_asym = 0
    for name, param, nested in tensors:
        if not nested.asymmetric:
            continue
        n_asym += 1
        want = lq.fq_forward_group_affine(param.data, nested.scale.data, nested.offset.data, -8, 7, gs, q_dtype=torch.int8, rounding=rounding)[1]
        assert weights[name].dtype == np.int8 and np.array_equal(weights[name], np.ascontiguousarray(want.cpu().numpy())), name
        assert weights[name].min() >= -8 and weights[name].max() <= 7
    assert n_asym == len(lq.custom_layers_of(model))
    with np.load(os.path.join(d, "scales.npz")) as z:
        assert sum(k.endswith("/W_offset") for k in z.files) == n_asym
    # the packed container: "asymmetric": true and the offset array per such tensor, an exact restore into a fresh model
    lq.save_packed_parameters(model, d)
    with np.load(os.path.join(d, "weights_packed.npz")) as z:
        manifest = export.read_packed_manifest(z)
        for e, (name, _, nested) in zip(manifest["tensors"], tensors):
            assert e.get("asymmetric", False) == nested.asymmetric and ((name + ".offset") in z.files) == nested.asymmetric
            if nested.asymmetric:
                assert bits_equal(z[name + ".offset"], nested.offset.detach().cpu().numpy())
    lq.reset_layer_names()
    fresh = lq.build_model(config, seed=99, asymmetric=True, **kw)
    lq.load_packed_parameters(fresh, d)
    for (name, p0, n0), (_, p1, n1) in zip(tensors, export.quantized_tensors(fresh)):
        assert torch.equal(n0.scale.detach(), n1.scale.detach()), name
        assert n0.offset is None or torch.equal(n0.offset.detach(), n1.offset.detach()), name
        assert torch.equal(n0(p0).detach(), n1(p1).detach()), f"{name}: fake-quantised output after the restore"
    x = torch.rand(4, *INPUT_SHAPES[config], device=dev)
    model.eval(), fresh.eval()
    with torch.no_grad():
        assert torch.equal(model(x), fresh(x))
    # a model whose `asymmetric` differs: refused, left untouched
    lq.reset_layer_names()
    other = lq.build_model(config, seed=99, **kw)
    before = [p.detach().clone() for p in other.parameters()]
    with pytest.raises(ValueError, match="asymmetric"):
        lq.load_packed_parameters(other, d)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, other.parameters()))
    sym_dir = os.path.join(d, "sym")
    lq.save_packed_parameters(other, sym_dir)
    with pytest.raises(ValueError, match="asymmetric"):
        lq.load_packed_parameters(fresh, sym_dir)


def test_export_of_a_symmetric_model_is_unchanged(dev, tmp_path):
    """A group-wise model without asymmetric layers: no key, no array and no side-file entry is added -- the manifest and the member
    list are rebuilt here from the symmetric ops alone and compared byte for byte."""
    import json
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    lq.reset_layer_names()
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, bits=4, group_size=64, scale_init="absmax")
    tensors = export.quantized_tensors(model)
    d = str(tmp_path)
    lq.save_compress_parameters(model, d)
    with np.load(os.path.join(d, "scales.npz")) as z:
        assert sorted(z.files) == sorted(layer.name + t for layer in lq.custom_layers_of(model) for t in ("/W_scale", "/b_scale"))
    lq.save_packed_parameters(model, d)
    entries, members = [], ["manifest"]
    for name, p, n in tensors:
        if n.group_size is not None:
            q = lq.fq_forward_group(p.data, n.scale.data, -8, 7, n.group_size, q_dtype=torch.float32)[1]
            unit = torch.ones(1, dtype=torch.float32, device=dev)
        else:
            q = lq.fq_forward_clip(p.data, n.scale.data, -8, 7, q_dtype=torch.float32)[1]
            unit = torch.ones_like(n.scale.data)
        lo, hi = (int(v) for v in lq.q_minmax(q, unit).tolist())
        entries.append({"name": name, "shape": list(p.shape), "scale_shape": list(n.scale.shape), "orientation": n.orientation,
                        "qmin": lo, "bits": (hi - lo).bit_length(), "numel": int(p.numel())})
        if n.group_size is not None:
            entries[-1]["group_size"] = n.group_size
        members += [name + ".codes", name + ".scale"]
    manifest = {"format": "lq-packed", "version": 1, "tensors": entries, "state": []}
    with np.load(os.path.join(d, "weights_packed.npz")) as z:
        assert z.files == members
        assert bytes(z["manifest"]) == json.dumps(manifest).encode("utf-8")
