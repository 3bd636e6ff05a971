"""GPU tests of the group-wise kernels WITH a learned offset per group (csrc/lq_group.hpp, lq_group_batch.hpp: lq_fq_*_group_affine,
k_group_batch_affine and its GroupAffineTask table, lq_group_stats with b) held to the battery tests/test_gpu_group_forms.py holds the
symmetric pair to: quotients one float to either side of an integer (or a tie) under full-mantissa scales and offsets, u = P - b
outside the fast-division window by cancellation and overflow next to bad scales, every launch form through ONE affine batch in
three orders, a full batch of 256 tensors with a grad_scale and an offset_grad_scale per slot, 64 random geometries off the 16-byte
grid in poisoned arenas and then through the batch, and the statistics kernel on the edge inputs.

The reference is tests/_group_affine_reference.py::group_affine_reference (tests/_group_reference.py::group_reference for the
tensors of a batch that have no offset).  The bar, everywhere: out, both integer views, dP and the clip counts equal it BIT FOR BIT
(NaN positional, the sign of zero kept); ds and db are held to tests/_bounds.py::assert_within_terms, |got - ref| <= 1e-5 *
sum|terms| (floor 2^-136; the terms of db are the |dy| of the clipped elements); two calls give the same bits; a batch gives the bits
of the single-tensor calls, ds and db included.  Conditions on the inputs are asserted on the reference before a kernel runs (and,
without a device, by tests/test_group_affine_forms_cpu.py).  The input builders live in tests/_group_affine_reference.py and
tests/_group_forms.py; Buf / Batch / _single / _results / _same are those of tests/test_gpu_group_affine_batch.py, _affine_pair and
_compare those of tests/test_gpu_group_affine.py.

conftest.py does not list this file: it runs in alphabetical order before test_gpu_parity.py, like the other unlisted files, and
needs nothing the later files establish (the reference is NumPy, the calls go through the C ABI).

Measured on the MI355X, worst |err| / sum|terms| (the bound is 1e-5):
  test_edge_quotients                  ds 5.06e-08 ((200, 64, 0, 64) [-8, 7] floor), db 5.33e-08 ((7, 333, 1, 50) [-8, 7] floor)
  test_forms_through_the_affine_batch  ds 5.96e-08, db 5.96e-08 (the single-tensor results of the floor run; 2^-24, the rounding of
                                       a one-element group's single term to float32)
Evidence that the tests bite: profiles/group_affine_forms/mutations.txt; the kernels the file launches:
profiles/group_affine_forms/kernel_coverage.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _group_stats_reference as G                                                            # noqa: E402
from _arena import Arena                                                                      # noqa: E402
from _bounds import assert_within_terms, stable_seed                                          # noqa: E402
from _clip_reference import bits_equal                                                        # noqa: E402
from _group_affine_reference import (FULL_BATCH, FULL_BATCH_SYMMETRIC, PLANTED_U, edge_offset_case, form_batch_factors,      # noqa: E402
                                     full_batch_factors, full_batch_inputs, group_affine_reference, make_affine_case, window_offset_case)
from _group_forms import (EDGE_RANGES, EDGE_SHAPES, FORM_CASES, GEOMETRY_DRAWS, LARGE, WINDOW_SHAPES, power_of_two_share,      # noqa: E402
                          random_geometry)
from _group_reference import expand_scale, group_reference, make_case                        # noqa: E402
from test_gpu_group_affine import _affine_pair, _compare, _ratio                              # noqa: E402
from test_gpu_group_affine_batch import SENTINEL, SET, Batch, Buf, _results, _same, _single  # noqa: E402

pytestmark = pytest.mark.gpu
ROUNDINGS = ("floor", "nearest")
STRADDLE = 0.65               # least share of the edge triples whose neighbours round differently (0.699 .. 0.904 with these seeds)
SYMMETRIC_FORMS = ((70, 12, 1, 3), (200, 64, 0, 64))      # the two tensors of the every-form batch without an offset: a row and a column form
STATS_SHAPES = (EDGE_SHAPES[0], EDGE_SHAPES[2])           # one column and one row shape of the edge inputs
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _f32_bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


# ------------------------------------------------------------------------------------------- 1 edge quotients with offsets
_EDGE = {}


def _edge(dev, case, range_, rounding):
    """Inputs, reference and the kernels' results of one edge case, computed once and shared (never modified) with the statistics
    test; the conditions are asserted here, on the reference, before the kernels run."""
    key = (case, range_, rounding)
    if key not in _EDGE:
        qmin, qmax = range_
        P, s, b, dy, share = edge_offset_case(stable_seed("affine edge forms", case, qmin, qmax, rounding), *case, qmin, qmax, rounding)
        what = f"{case} [{qmin}, {qmax}] {rounding}"
        assert share >= STRADDLE, f"{what}: the neighbours of only {share:.3f} of the triples round differently"
        assert power_of_two_share(s) < 0.01 and np.all(b != 0)
        ref = group_affine_reference(P, s, b, dy, qmin, qmax, case[2], case[3], rounding=rounding)
        assert 0 < int(ref["clipped"].sum()) < P.size
        got = _affine_pair(dev, P, s, b, dy, case, qmin, qmax, rounding)
        _EDGE[key] = (P, s, b, ref, got, share)
    return _EDGE[key]


@pytest.mark.parametrize("range_", EDGE_RANGES, ids=_ids)
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_edge_quotients(dev, rounding, range_):
    """P = fl32(fl32(m s) + b) and its two neighbours, m = n (floor) or n + 1/2 (nearest), n over [qmin - 2, qmax + 2], per-group
    scales 2^U(-12, 3) and offsets U(-6, 6) * s, both with full mantissas: u = P - b, t = u / s and out = (q s) + b each round on
    their own, and a contraction, a reassociation or another order of the roundings lands on the other integer or the other float.
    The straddle bar is 0.65, not the symmetric file's 0.85: an ulp of P is not an ulp of u."""
    for case in EDGE_SHAPES:
        what = f"{case} [{range_[0]}, {range_[1]}] {rounding}"
        P, s, b, ref, got, share = _edge(dev, case, range_, rounding)
        worst = _compare(got, ref, what)
        print(f"{what}: {share:.3f} of the triples straddle, max err / sum|terms|: ds {worst[0]:.3e}, db {worst[1]:.3e}")


# --------------------------------------------------------------------- 2 u outside the division window, bad scales next to offsets
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_u_outside_the_division_window(dev, rounding):
    """u = P - b equal to 2^-81, 2^-80, 2^81, the float below, a denormal from two normal operands, +0 from P == b != 0, +-Inf from
    the overflow of finite operands and NaN from Inf - Inf -- in the float4 forms in one lane of a float4 whose other lanes are not
    planted -- and the scales of BAD_SCALES next to non-zero offsets (axis 0: one of the four divisors of a float4; axis 1: every
    other group).  The window test of fq_quot4 / fq_quot4c sees u, not P; every comparison follows IEEE, as the reference's NumPy
    arithmetic does; the ordinary groups next to a spoiled one are held to the full bar."""
    for case in WINDOW_SHAPES:
        P, s, b, dy, bad, planted = window_offset_case(stable_seed("affine window", case), *case)
        with np.errstate(all="ignore"):
            u = P - expand_scale(b, *case)
            ref = group_affine_reference(P, s, b, dy, -8, 7, case[2], case[3], rounding=rounding)
        for name, _, _, want in PLANTED_U:
            at = planted[name]
            assert at, f"{case}: {name} is not reached"
            for r, c in at:
                assert (np.isnan(want) and np.isnan(u[r, c])) or _f32_bits(u[r, c])[0] == _f32_bits(want)[0], f"{case}: u at {(r, c)} is not {name}"
        assert np.isnan(ref["ds"]).any() and np.isfinite(ref["ds"][~bad]).any() and np.isnan(ref["out"]).any()
        _compare(_affine_pair(dev, P, s, b, dy, case, -8, 7, rounding), ref, f"{case} {rounding}", special=True)


# ----------------------------------------------------------------------------------------------- 3, 4 the forms in an affine batch
class Tensor:
    """Device buffers of one tensor of an affine batch (the interface of test_gpu_group_affine_batch.Buf) with a grad_scale ``k`` and
    an offset_grad_scale ``kb`` of its own; ``b`` None: a symmetric tensor.  Outputs are preset to the sentinel word, every dense
    base lies ``offset`` floats off a 16-byte aligned address."""
    desc, off, untouched = Buf.desc, Buf.off, Buf.untouched

    def __init__(self, dev, P, s, b, dy, geom, range_, k, kb, offset=0):
        self.geom, self.range, self.k, self.kb = geom, range_, float(np.float32(k)), float(np.float32(kb))
        self.s = _t(s, dev)
        self.b = None if b is None else _t(b, dev)
        self.P, self.dy = Buf._at(P, dev, offset), Buf._at(dy, dev, offset)
        self.out, self.dp = Buf._at(None, dev, offset, P.shape), Buf._at(None, dev, offset, P.shape)
        self.ds = torch.full(s.shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        self.db = torch.full(s.shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        self.pass_db = self.b is not None


def _run_batch(tensors, rounding, forward=True, mask_only=False):
    batch = Batch(tensors, rounding)
    if forward:
        batch.forward()
    batch.backward(mask_only=mask_only)
    return _results(batch)


def _reference_of(P, s, b, dy, geom, range_, k, kb, rounding="floor"):
    if b is None:
        return group_reference(P, s, dy, *range_, geom[2], geom[3], k=k, rounding=rounding)
    return group_affine_reference(P, s, b, dy, *range_, geom[2], geom[3], k=k, kb=kb, rounding=rounding)


def _hold_to_reference(got, ref, what):
    """(out, dP, ds, db | None, counts) of a tensor against its reference; returns the worst ratios of ds and db."""
    out, dP, ds, db, cnt = got
    assert bits_equal(out, ref["out"]), f"{what}: out"
    assert bits_equal(dP, ref["dP"]), f"{what}: dP"
    assert np.array_equal(cnt.reshape(ref["clipped"].shape), ref["clipped"]), f"{what}: counts"
    assert_within_terms(ds, ref["ds"], ref["terms"], f"{what}: ds")
    worst = [_ratio(ds, ref["ds"], ref["terms"]), 0.0]
    assert (db is None) == ("db" not in ref), f"{what}: db on one side only"
    if db is not None:
        assert_within_terms(db, ref["db"], ref["terms_b"], f"{what}: db")
        worst[1] = _ratio(db, ref["db"], ref["terms_b"])
    return worst


_FORM_INPUTS = {}


def _form_inputs(case):
    """(P, s, b | None, dy) of a FORMS case: make_affine_case, or make_case for the two symmetric tensors."""
    if case not in _FORM_INPUTS:
        if case in SYMMETRIC_FORMS:
            P, s, dy = make_case(stable_seed("groupforms", *case), *case)
            _FORM_INPUTS[case] = (P, s, None, dy)
        else:
            _FORM_INPUTS[case] = make_affine_case(stable_seed("affineforms", *case), *case)
    return _FORM_INPUTS[case]


def test_forms_through_the_affine_batch(dev):
    """Every FORMS case but the large one in ONE lq_group_batch_create_affine batch, a grad_scale and an offset_grad_scale of its
    own per tensor, two of the tensors without an offset: in table order (floor), shuffled (floor) and in the reversed shuffle
    (nearest) every tensor has the bits of its single-tensor call (lq_fq_*_group_affine, or lq_fq_*_group without an offset), ds,
    db and the counts included -- the host's index permutation carries b, db and kb along with the task.  For nb > 32768 this
    holds the looped single-tensor affine column kernel against the batch's loop-free blocks.  The single-tensor results of the
    floor run are held to the reference."""
    cases = [c for c in FORM_CASES if c != LARGE]
    assert all(c in cases for c in SYMMETRIC_FORMS) and sum(c[0] // c[3] > 32768 for c in cases if c[2] == 0) == 3
    factors = dict(zip(cases, form_batch_factors(len(cases))))
    assert len({k for k, _ in factors.values()}) == len({kb for _, kb in factors.values()}) == len(cases)
    order = [int(i) for i in np.random.default_rng(stable_seed("affine forms batch")).permutation(len(cases))]
    assert order != sorted(order)
    singles = {}
    for rounding, idx in (("floor", range(len(cases))), ("floor", order), ("nearest", order[::-1])):
        tensors = [Tensor(dev, *_form_inputs(cases[i]), cases[i], (-8, 7), *factors[cases[i]]) for i in idx]
        for t, got in zip(tensors, _run_batch(tensors, rounding)):
            key = (t.geom, rounding)
            if key not in singles:
                singles[key] = _single(t, rounding)
            assert t.untouched("db") == (t.b is None), f"{t.geom} {rounding}: the db buffer"
            _same(got, singles[key], f"{t.geom} {rounding}, batch against the single-tensor ops")
    worst = [0.0, 0.0]
    for c in cases:
        ref = _reference_of(*_form_inputs(c), c, (-8, 7), *factors[c])
        assert 0 < int(ref["clipped"].sum()) < _form_inputs(c)[0].size
        w = _hold_to_reference(singles[(c, "floor")], ref, f"{c} with factors {factors[c]}")
        worst = [max(a, b_) for a, b_ in zip(worst, w)]
    print(f"forms through the affine batch: max err / sum|terms|: ds {worst[0]:.3e}, db {worst[1]:.3e}")


def _full_batch(dev):
    geoms = [SET[(i + 3) % len(SET)] for i in range(FULL_BATCH)]
    inputs = [full_batch_inputs(i, g) for i, g in enumerate(geoms)]
    tensors = [Tensor(dev, *inp, g, (-8, 7), *full_batch_factors(i)) for i, (inp, g) in enumerate(zip(inputs, geoms))]
    return geoms, inputs, tensors


def test_full_affine_batch(dev):
    """256 tensors -- the capacity of the by-value tables PtrPack / CoefPack -- cycling through the ten shapes of the affine batch's
    set, every tensor with its own data, grad_scale = 1 + i / 256 (CoefPack, slots >= 128 included) and offset_grad_scale =
    2 - i / 256 (the task table's kb); every eighth tensor symmetric; tensor 254 a row form, tensor 255 a column form, both with an
    offset.  Every tensor equals its single-tensor call bit for bit, one tensor of every shape equals the reference; a second,
    fresh batch called with grad_scale = NULL writes dP and the counts and leaves ds, db and out alone."""
    n = FULL_BATCH
    geoms, inputs, tensors = _full_batch(dev)
    assert len(tensors) == n and len({t.k for t in tensors}) == n and len({t.kb for t in tensors}) == n
    assert geoms[254][2] == 1 and geoms[255][2] == 0 and tensors[254].b is not None and tensors[255].b is not None
    assert [t.b is None for t in tensors] == [i % FULL_BATCH_SYMMETRIC == 0 for i in range(n)]
    got = _run_batch(tensors, "floor")
    want = [_single(t, "floor") for t in tensors]
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"tensor {i} {geoms[i]} of {n}")
        assert tensors[i].untouched("db") == (tensors[i].b is None), f"tensor {i}: the db buffer"
    last = range(n - len(SET), n)              # one tensor of every shape, the last two slots and a symmetric tensor among them
    assert {geoms[i] for i in last} == set(SET) and any(tensors[i].b is None for i in last)
    for i in last:
        ref = _reference_of(*inputs[i], geoms[i], (-8, 7), tensors[i].k, tensors[i].kb)
        assert 0 < int(ref["clipped"].sum()) < inputs[i][0].size
        _hold_to_reference(got[i], ref, f"tensor {i} {geoms[i]}")
    _, _, fresh = _full_batch(dev)
    for i, (t, r) in enumerate(zip(fresh, _run_batch(fresh, "floor", forward=False, mask_only=True))):
        assert t.untouched("ds", "db", "out"), f"tensor {i}: the mask-only call wrote ds, db or out"
        assert bits_equal(r[1], want[i][1]) and np.array_equal(r[4], want[i][4]), f"tensor {i}: dP / counts of the mask-only call"


# ------------------------------------------------------------------------------------------------ 5 random geometry with offsets
def _arena_pair(dev, d, P, s, b, dy):
    """Forward and backward through the C ABI, P, dy, out and dP ``d["residue"]`` bytes off the 16-byte grid, s, b, q, ds, db and
    clipped regions of their own, all between guard bands (as test_gpu_group_affine._raw_case): outputs complete, guards and
    inputs untouched.  Returns the results as NumPy arrays."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = d["R"], d["C"], d["axis"], d["gs"]
    (qmin, qmax), rnd, residue, row = d["range"], ROUNDINGS.index(d["rounding"]), d["residue"], d["C"] * 4
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=residue, row_bytes=row)
    ar.add("s", "in", data=s)
    ar.add("b", "in", data=b)
    ar.add("dy", "in", data=dy, residue=residue, row_bytes=row)
    for name in ("out", "dP"):
        ar.add(name, "out", nbytes=P.nbytes, residue=residue, row_bytes=row)
    ar.add("q", "out", nbytes=P.nbytes)
    for name in ("ds", "db", "clipped"):
        ar.add(name, "out", nbytes=s.nbytes)
    ar.build()
    assert all(ar.ptr(n) % 16 == residue for n in ("P", "dy", "out", "dP"))
    assert lib.lq_group_workspace_bytes(R, C, axis, gs) == 0
    st = _hip.stream_ptr(dev)
    _hip.check(lib.lq_fq_forward_group_affine(ar.ptr("P"), ar.ptr("s"), ar.ptr("b"), ar.ptr("out"), ar.ptr("q"), _hip.LQ_Q_I32, qmin, qmax,
                                              rnd, R, C, axis, gs, st), "lq_fq_forward_group_affine")
    _hip.check(lib.lq_fq_backward_group_affine(ar.ptr("P"), ar.ptr("s"), ar.ptr("b"), ar.ptr("dy"), qmin, qmax, rnd, 1.0, 1.0, ar.ptr("dP"),
                                               ar.ptr("ds"), ar.ptr("db"), ar.ptr("clipped"), None, 0, R, C, axis, gs, st),
               "lq_fq_backward_group_affine")
    torch.cuda.synchronize(dev)
    ar.check(f"draw {d}")
    qi = ar.numpy("q", np.int32).reshape(R, C)      # the int32 view alone: it cannot tell the -0 that rint gives for t in [-1/2, -0]
    return dict(out=ar.numpy("out", np.float32).reshape(R, C), q=None, qi=qi, dP=ar.numpy("dP", np.float32).reshape(R, C),
                ds=ar.numpy("ds", np.float32).reshape(s.shape), db=ar.numpy("db", np.float32).reshape(s.shape),
                clipped=ar.numpy("clipped", np.uint32).astype(np.int64).reshape(s.shape))


def test_random_geometry_with_offsets(dev):
    """The 64 seeded draws of _group_forms.random_geometry (R, C, axis, gs, rounding, range, base residue) with the data of
    make_affine_case(k, ...), each inside a poisoned arena against the reference; then all of them through two affine batches (one
    per rounding, same residues: same forms) against those results, bit for bit.  A failing draw is reproduced alone from its
    ``k``.  make_affine_case's spread N(0, 1) * 8 s clips 58 % of all elements over the three ranges: no rescaling is needed."""
    draws = [random_geometry(i) for i in range(GEOMETRY_DRAWS)]
    clipped = total = 0
    singles, data = [], []
    for d in draws:
        P, s, b, dy = make_affine_case(d["k"], d["R"], d["C"], d["axis"], d["gs"])
        ref = group_affine_reference(P, s, b, dy, *d["range"], d["axis"], d["gs"], rounding=d["rounding"])
        clipped, total = clipped + int(ref["clipped"].sum()), total + P.size
        got = _arena_pair(dev, d, P, s, b, dy)
        _compare(got, ref, f"draw {d}")
        singles.append(got)
        data.append((P, s, b, dy))
    assert 0.1 * total <= clipped <= 0.9 * total, f"{clipped} of {total} elements clipped over the whole set"
    for rounding in ROUNDINGS:
        mine = [i for i, d in enumerate(draws) if d["rounding"] == rounding]
        tensors = [Tensor(dev, *data[i], (draws[i]["R"], draws[i]["C"], draws[i]["axis"], draws[i]["gs"]), draws[i]["range"], 1.0, 1.0,
                          offset=draws[i]["residue"] // 4) for i in mine]
        assert all(t.P.data_ptr() % 16 == draws[i]["residue"] for t, i in zip(tensors, mine))
        for i, got in zip(mine, _run_batch(tensors, rounding)):
            w = singles[i]
            _same(got, (w["out"], w["dP"], w["ds"], w["db"], w["clipped"]), f"draw {draws[i]} in the {rounding} batch")


# ------------------------------------------------------------------------------------------------ 6 statistics on the edge inputs
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_statistics_on_the_edge_inputs(dev, rounding):
    """ops.group_stats with the offset on the edge inputs, where the clipped / inside decision hangs on one ulp: below + above is
    the backward's clip count group by group, below and above are the reference's counts of q0 < lo and q0 > hi, the histogram is
    the bincount of the reference's clamped integers."""
    import learned_quantization_amd as lq
    for case in STATS_SHAPES:
        R, C, axis, gs = case
        P, s, b, ref, got, _ = _edge(dev, case, (-8, 7), rounding)
        want = G.group_stats_reference(P, s, -8, 7, axis, gs, b=b, rounding=rounding)
        assert want["below"].sum() > 0 and want["above"].sum() > 0
        st = lq.group_stats(_t(P, dev), _t(s, dev), -8, 7, gs, offset=_t(b, dev), rounding=rounding)
        u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)      # noqa: E731
        below, above, hist = u32(st.below), u32(st.above), u32(st.hist)
        what = f"{case} {rounding}"
        assert np.array_equal(below + above, got["clipped"].reshape(below.shape)), f"{what}: below + above against the backward's counts"
        assert np.array_equal(below, want["below"]) and np.array_equal(above, want["above"]), f"{what}: below / above"
        assert np.array_equal(below + above, ref["clipped"])
        q = ref["q"].astype(np.int64)
        assert np.array_equal(hist, np.bincount((q - (-8)).reshape(-1), minlength=16)) and np.array_equal(hist, want["hist"]), f"{what}: hist"
