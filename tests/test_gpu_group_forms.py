"""GPU tests of the group-wise kernels (csrc/lq_group.hpp, lq_group_batch.hpp) at every launch form the host rule can pick, on
quotients one ulp to either side of an integer (or a tie), on scales outside the fast-division window, and on random geometry.

The reference is tests/_group_reference.py (one-axis descriptors: tests/_clip_reference.py / _rne_reference.py).  The bar, everywhere:
out, q, dP and the clip counts equal it BIT FOR BIT (NaN positional, the sign of zero kept); ds is held to
tests/_bounds.py::assert_within_terms, |got - ref| <= 1e-5 * sum|dy_i r_i| (floor 2^-136); two calls give the same bits; a batch
gives the bits of the single-tensor call, ds included.  Conditions on the inputs are asserted on the reference before a kernel runs
(and, without a device, by tests/test_group_forms_cpu.py).

``FORMS`` (tests/_group_forms.py) is the case table: one row per run-time branch of group_launch (the host's one launch rule:
form, team width, forward row split, grid; launch_group and fill_group_task ask it) that the lists of tests/test_gpu_groupwise.py and test_gpu_group_batch.py do not reach --
team widths 2 to 64 of both row forms, a second trip of the column forms' grid-stride group loop (nb > 32768), the forward row split
decided by the 2048-block cap.  The integer view q of a NaN quotient is not defined by the reference (NumPy's cast of NaN to an integer
is not); the int32 view is therefore compared only where the reference q is finite, the float32 view everywhere."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _arena import Arena                                                                      # noqa: E402
from _bounds import assert_within_terms, stable_seed                                          # noqa: E402
from _clip_reference import bits_equal, clip_reference                                        # noqa: E402
from _group_forms import (CLIP_DESCRIPTORS, EDGE_RANGES, EDGE_SHAPES, FORM_CASES, GEOMETRY_DRAWS, LARGE, VARIANTS, WINDOW_SHAPES,      # noqa: E402
                          edge_clip_case, edge_group_case, form_variants, power_of_two_share, random_geometry, window_clip_cases,
                          window_group_case)
from _group_reference import check_condition, group_reference, make_case                     # noqa: E402
from _rne_reference import rne_reference                                                      # noqa: E402
from test_gpu_group_batch import SENTINEL, SET, Batch, Buf, _results, _same, _single      # noqa: E402

pytestmark = pytest.mark.gpu
ROUNDINGS = ("floor", "nearest")
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _counts(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _compare(got, ref, what, special=False):
    """got: dict(out, q (float32 view; None: not asked for), qi (int32 view), dP, ds, clipped) as NumPy arrays; ``special``: NaN / Inf
    are expected."""
    assert bits_equal(got["out"], ref["out"]), f"{what}: out"
    assert got["q"] is None or bits_equal(got["q"], ref["q"]), f"{what}: q (float32 view)"
    finite = np.isfinite(ref["q"])
    assert special or finite.all()
    with np.errstate(all="ignore"):
        want_int = np.where(finite, ref["q"], 0).astype(np.int32)
    assert np.array_equal(got["qi"][finite], want_int[finite]), f"{what}: q (int32 view)"
    assert bits_equal(got["dP"], ref["dP"]), f"{what}: dP"
    assert np.array_equal(got["clipped"].reshape(ref["clipped"].shape), ref["clipped"]), f"{what}: clipped"
    ds, nan = got["ds"].reshape(ref["ds"].shape), np.isnan(ref["ds"])
    assert special or not nan.any()
    assert np.array_equal(np.isnan(ds), nan), f"{what}: ds is NaN in other groups than the reference's"
    assert_within_terms(ds[~nan], ref["ds"][~nan], ref["terms"][~nan], f"{what}: ds")
    with np.errstate(all="ignore"):
        r = np.abs(ds[~nan].astype(np.float64) - ref["ds"][~nan]) / np.maximum(ref["terms"][~nan], 1e-300)
    return float(r.max()) if r.size else 0.0


def _group_pair(dev, P, s, dy, geom, qmin, qmax, rounding, k=1.0):
    """Forward (both integer views) and backward of the single-tensor kernels, each called twice: the same bits.  Through the C ABI,
    where the axis is an argument: the Python ops derive it from the shape of the scale (descriptor.group_geometry), and for gs = 1,
    where both axes describe the same groups, they pick axis 1 -- an axis-0 case of gs = 1 would never reach the column kernels."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = geom
    rnd, st = ROUNDINGS.index(rounding), _hip.stream_ptr(dev)
    Pt, st_, dt = _t(P, dev), _t(s, dev), _t(dy, dev)
    assert Pt.data_ptr() % 16 == 0 and dt.data_ptr() % 16 == 0
    runs = []
    for q_dtype, code in ((torch.float32, _hip.LQ_Q_F32), (torch.int32, _hip.LQ_Q_I32)):
        out, q = torch.empty_like(Pt), torch.empty(Pt.shape, dtype=q_dtype, device=dev)
        dP, ds, cnt = torch.empty_like(Pt), torch.empty_like(st_), torch.empty(st_.shape, dtype=torch.int32, device=dev)
        assert out.data_ptr() % 16 == 0 and dP.data_ptr() % 16 == 0
        _hip.check(lib.lq_fq_forward_group(Pt.data_ptr(), st_.data_ptr(), out.data_ptr(), q.data_ptr(), code, qmin, qmax, rnd,
                                           R, C, axis, gs, st), "lq_fq_forward_group")
        _hip.check(lib.lq_fq_backward_group(Pt.data_ptr(), st_.data_ptr(), dt.data_ptr(), qmin, qmax, rnd, float(k), dP.data_ptr(),
                                            ds.data_ptr(), cnt.data_ptr(), None, 0, R, C, axis, gs, st), "lq_fq_backward_group")
        runs.append((out, q, dP, ds, cnt))
    (out, q, dP, ds, cnt), second = runs
    for name, x, y in zip(("out", "dP", "ds", "clipped"), (out, dP, ds, cnt), (second[0],) + second[2:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"two calls differ in {name}"
    return dict(out=out.cpu().numpy(), q=q.cpu().numpy(), qi=second[1].cpu().numpy(), dP=dP.cpu().numpy(), ds=ds.cpu().numpy(),
                clipped=_counts(cnt))


def _clip_pair(dev, P, s, dy, qmin, qmax, rounding):
    """The one-axis clipped pair (lq_fq_forward_clip_r / lq_fq_backward_clip_r) on an (outer, G, inner) descriptor."""
    import learned_quantization_amd as lq
    Pt, st, dt = _t(P, dev), _t(s, dev), _t(dy, dev)
    out, q = lq.fq_forward_clip(Pt, st, qmin, qmax, q_dtype=torch.float32, rounding=rounding)
    out2, qi = lq.fq_forward_clip(Pt, st, qmin, qmax, q_dtype=torch.int32, rounding=rounding)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), "two forward calls differ"
    a = lq.fq_backward_clip(Pt, st, dt, qmin, qmax, want_clipped=True, rounding=rounding)
    b = lq.fq_backward_clip(Pt, st, dt, qmin, qmax, want_clipped=True, rounding=rounding)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), "two backward calls differ"
    return dict(out=out.cpu().numpy(), q=q.cpu().numpy(), qi=qi.cpu().numpy(), dP=a[0].cpu().numpy(), ds=a[1].cpu().numpy(),
                clipped=_counts(a[2]))


def _clip_ref(P, s, dy, qmin, qmax, rounding):
    return (clip_reference if rounding == "floor" else rne_reference)(P, s, dy, qmin, qmax)


# ------------------------------------------------------------------------------------------------------------------ 1 forms
_INPUTS, _REFS = {}, {}


def _inputs(case):
    if case not in _INPUTS:
        _INPUTS[case] = make_case(stable_seed("groupforms", *case), *case)
    return _INPUTS[case]


def _ref(case, variant):
    """Reference of one case and variant, computed once and shared (never modified); the condition is asserted here."""
    if (case, variant) not in _REFS:
        (qmin, qmax), rounding = VARIANTS[variant]
        P, s, dy = _inputs(case)
        ref = group_reference(P, s, dy, qmin, qmax, case[2], case[3], rounding=rounding)
        check_condition(ref, *case, f"{case} {variant}")
        _REFS[(case, variant)] = ref
    return _REFS[(case, variant)]


@pytest.mark.parametrize("case,variant", form_variants(), ids=lambda v: _ids(v))
def test_forms(dev, case, variant):
    """The single-tensor forward and backward of every row of FORMS against the reference: floor [-8, 7] for all, nearest for the
    teams of 16 and 64 and the second-trip cases, [0, 15] for four.  profiles/group_forms/kernel_coverage.txt lists kernel and grid
    of each of these launches."""
    (qmin, qmax), rounding = VARIANTS[variant]
    ref = _ref(case, variant)
    P, s, dy = _inputs(case)
    worst = _compare(_group_pair(dev, P, s, dy, case, qmin, qmax, rounding), ref, f"{case} {variant}")
    print(f"{case} {variant}: max err / sum|terms| = {worst:.3e}")


# ------------------------------------------------------------------------------------------------- 2, 3 the forms in a batch
class Tensor:
    """Device buffers of one tensor of a batch (the interface of test_gpu_group_batch.Buf): outputs preset to the sentinel word,
    every dense base ``offset`` floats off a 16-byte aligned address."""
    desc, untouched = Buf.desc, Buf.untouched

    def __init__(self, dev, P, s, dy, geom, range_, k, offset=0):
        self.geom, self.range, self.k = geom, range_, float(np.float32(k))
        self.s = _t(s, dev)
        self.P, self.dy = Buf._at(P, dev, offset), Buf._at(dy, dev, offset)
        self.out, self.dp = Buf._at(None, dev, offset, P.shape), Buf._at(None, dev, offset, P.shape)
        self.ds = torch.full(s.shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _run_batch(tensors, rounding, mask_only=False):
    batch = Batch(tensors, rounding)
    assert batch.need == 0
    batch.forward()
    batch.backward(mask_only=mask_only, ks=[t.k for t in tensors])
    return _results(batch)


def test_forms_through_the_batch(dev):
    """Every FORMS case but the large one in ONE batch, in table order and shuffled, a grad_scale of its own per tensor: the bits of
    the single-tensor calls.  For nb > 32768 this holds the looped single-tensor kernel against the batch's loop-free blocks."""
    cases = [c for c in FORM_CASES if c != LARGE]
    ks = {c: 1.0 + (i + 1) / 32.0 for i, c in enumerate(cases)}
    singles = {}
    order = [int(i) for i in np.random.default_rng(stable_seed("forms batch")).permutation(len(cases))]
    assert order != sorted(order)
    for rounding, idx in (("floor", range(len(cases))), ("floor", order), ("nearest", order[::-1])):
        tensors = [Tensor(dev, *_inputs(cases[i]), cases[i], (-8, 7), ks[cases[i]]) for i in idx]
        for t, got in zip(tensors, _run_batch(tensors, rounding)):
            key = (t.geom, rounding)
            if key not in singles:
                singles[key] = _single(t, rounding, k=t.k)
            _same(got, singles[key], f"{t.geom} {rounding}, batch against the single-tensor ops")
    for c in cases:                    # the single-tensor results are the reference's: out, dP, counts; ds within the bound
        ref = _ref(c, "floor")
        out, dP, ds, cnt = singles[(c, "floor")]
        assert bits_equal(out, ref["out"]) and bits_equal(dP, ref["dP"]) and np.array_equal(cnt.reshape(ref["clipped"].shape), ref["clipped"])
        k = float(np.float32(ks[c]))
        assert_within_terms(ds, ref["ds"] * k, ref["terms"] * k, f"{c}: ds with grad_scale {k}")


def test_full_batch(dev):
    """256 tensors -- the capacity of the by-value tables PtrPack / CoefPack -- cycling through the ten shapes of the group batch's
    set, every tensor with its own data and grad_scale = 1 + i / 256; tensor 254 a row form, tensor 255 a column form.  Every tensor
    equals its single-tensor call bit for bit; a second call with grad_scale = NULL writes dP and the counts and leaves ds alone."""
    n = 256
    geoms = [SET[(i + 3) % len(SET)] for i in range(n)]
    assert geoms[254][2] == 1 and geoms[255][2] == 0
    tensors = [Tensor(dev, *make_case(stable_seed("full batch", i), *g), g, (-8, 7), 1.0 + i / 256.0) for i, g in enumerate(geoms)]
    assert len({t.k for t in tensors}) == n
    got = _run_batch(tensors, "floor")
    want = [_single(t, "floor", k=t.k) for t in tensors]
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"tensor {i} {geoms[i]} of 256")
    for i in range(n - len(SET), n):          # one tensor of every shape, the last two slots among them, against the reference
        P, s, dy = make_case(stable_seed("full batch", i), *geoms[i])
        ref = group_reference(P, s, dy, -8, 7, geoms[i][2], geoms[i][3], k=tensors[i].k)
        assert 0 < int(ref["clipped"].sum()) < P.size
        assert bits_equal(got[i][0], ref["out"]) and bits_equal(got[i][1], ref["dP"]) and np.array_equal(got[i][3], ref["clipped"])
        assert_within_terms(got[i][2], ref["ds"], ref["terms"], f"tensor {i}: ds")
    fresh = [Tensor(dev, *make_case(stable_seed("full batch", i), *g), g, (-8, 7), 1.0 + i / 256.0) for i, g in enumerate(geoms)]
    batch = Batch(fresh, "floor")
    batch.backward(mask_only=True)
    for i, (t, r) in enumerate(zip(fresh, _results(batch))):
        assert t.untouched("ds", "out"), f"tensor {i}: the mask-only call wrote ds or out"
        assert bits_equal(r[1], want[i][1]) and np.array_equal(r[3], want[i][3]), f"tensor {i}: dP / counts of the mask-only call"


# ------------------------------------------------------------------------------------------------------- 4 edge quotients
@pytest.mark.parametrize("range_", EDGE_RANGES, ids=_ids)
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_edge_quotients(dev, rounding, range_):
    """P = fl32(m s) and its two neighbours, m = n (floor) or n + 1/2 (nearest), n over [qmin - 2, qmax + 2], per-group scales
    2^U(-12, 3) with full mantissas: a quotient that is off by one ulp lands on the other integer."""
    qmin, qmax = range_
    for case in EDGE_SHAPES:
        P, s, dy, share = edge_group_case(stable_seed("edge", case, qmin, qmax, rounding), *case, qmin, qmax, rounding)
        what = f"{case} [{qmin}, {qmax}] {rounding}"
        assert share >= 0.85, f"{what}: the neighbours of only {share:.3f} of the triples round differently"
        assert power_of_two_share(s) < 0.01
        ref = group_reference(P, s, dy, qmin, qmax, case[2], case[3], rounding=rounding)
        worst = _compare(_group_pair(dev, P, s, dy, case, qmin, qmax, rounding), ref, what)
        print(f"{what}: {share:.3f} of the triples straddle, max err / sum|terms| = {worst:.3e}")
    for desc in CLIP_DESCRIPTORS:
        P, s, dy, share = edge_clip_case(stable_seed("edge", desc, qmin, qmax, rounding), desc, qmin, qmax, rounding)
        what = f"{desc} [{qmin}, {qmax}] {rounding}"
        assert share >= 0.85 and power_of_two_share(s) < 0.01, f"{what}: {share:.3f}"
        _compare(_clip_pair(dev, P, s, dy, qmin, qmax, rounding), _clip_ref(P, s, dy, qmin, qmax, rounding), what)


# ---------------------------------------------------------------------------------- 5 scales outside the division window
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_scales_outside_the_division_window(dev, rounding):
    """Scales 2^-40, the float below, 2^40, the float above, an all-ones mantissa, -0.25, +-0, a denormal, 3e38, +Inf and NaN next
    to ordinary ones (axis 0: one of the four divisors of a float4; axis 1: every other group), and in P 2^-81, 2^-80, 2^81, the
    float below, +-0, a denormal, +-Inf and NaN: every comparison of the clamp, the mask, r and the counts follows IEEE, as the
    reference's NumPy arithmetic does; the ordinary groups next to a bad one are held to the same bar."""
    for case in WINDOW_SHAPES:
        P, s, dy, bad = window_group_case(stable_seed("window", case), *case)
        with np.errstate(all="ignore"):
            ref = group_reference(P, s, dy, -8, 7, case[2], case[3], rounding=rounding)
        assert np.isnan(ref["ds"]).any() and np.isfinite(ref["ds"][~bad]).any()
        _compare(_group_pair(dev, P, s, dy, case, -8, 7, rounding), ref, f"{case} {rounding}", special=True)
    for desc in CLIP_DESCRIPTORS:
        for k, (P, s, dy, bad) in enumerate(window_clip_cases(stable_seed("window", desc), desc)):
            with np.errstate(all="ignore"):
                ref = _clip_ref(P, s, dy, -8, 7, rounding)
            assert np.isfinite(ref["ds"][~bad]).any()
            _compare(_clip_pair(dev, P, s, dy, -8, 7, rounding), ref, f"{desc} pass {k} {rounding}", special=True)


# ------------------------------------------------------------------------------------------------------ 6 random geometry
def _arena_pair(dev, d, P, s, dy):
    """Forward and backward through the C ABI, every dense tensor ``d["residue"]`` bytes off the 16-byte grid between guard bands
    (as test_gpu_groupwise._raw_case): outputs complete, guards and inputs untouched.  Returns the results as NumPy arrays."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = d["R"], d["C"], d["axis"], d["gs"]
    (qmin, qmax), rnd, residue, row = d["range"], ROUNDINGS.index(d["rounding"]), d["residue"], d["C"] * 4
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=residue, row_bytes=row)
    ar.add("s", "in", data=s)
    ar.add("dy", "in", data=dy, residue=residue, row_bytes=row)
    for name in ("out", "dP"):
        ar.add(name, "out", nbytes=P.nbytes, residue=residue, row_bytes=row)
    ar.add("q", "out", nbytes=P.nbytes)
    ar.add("ds", "out", nbytes=s.nbytes)
    ar.add("clipped", "out", nbytes=s.nbytes)
    ar.build()
    assert ar.ptr("P") % 16 == residue and ar.ptr("dy") % 16 == residue and ar.ptr("out") % 16 == residue and ar.ptr("dP") % 16 == residue
    assert lib.lq_group_workspace_bytes(R, C, axis, gs) == 0
    st = _hip.stream_ptr(dev)
    _hip.check(lib.lq_fq_forward_group(ar.ptr("P"), ar.ptr("s"), ar.ptr("out"), ar.ptr("q"), _hip.LQ_Q_I32, qmin, qmax, rnd, R, C, axis, gs, st),
               "lq_fq_forward_group")
    _hip.check(lib.lq_fq_backward_group(ar.ptr("P"), ar.ptr("s"), ar.ptr("dy"), qmin, qmax, rnd, 1.0, ar.ptr("dP"), ar.ptr("ds"),
                                        ar.ptr("clipped"), None, 0, R, C, axis, gs, st), "lq_fq_backward_group")
    torch.cuda.synchronize(dev)
    ar.check(f"draw {d}")
    qi = ar.numpy("q", np.int32).reshape(R, C)      # the int32 view alone: it cannot tell the -0 that rint gives for t in [-1/2, -0]
    return dict(out=ar.numpy("out", np.float32).reshape(R, C), q=None, qi=qi, dP=ar.numpy("dP", np.float32).reshape(R, C),
                ds=ar.numpy("ds", np.float32).reshape(s.shape), clipped=ar.numpy("clipped", np.uint32).astype(np.int64).reshape(s.shape))


def test_random_geometry(dev):
    """64 seeded draws of (R, C, axis, gs, rounding, range, base residue) against the reference, each inside a poisoned arena; then
    all of them through two group batches (one per rounding, same residues: same forms) against those results, bit for bit.  A
    failing draw is reproduced alone from its ``k``: random_geometry(i) and make_case(k, R, C, axis, gs)."""
    draws = [random_geometry(i) for i in range(GEOMETRY_DRAWS)]
    clipped = total = 0
    singles, data = [], []
    for d in draws:
        P, s, dy = make_case(d["k"], d["R"], d["C"], d["axis"], d["gs"])
        ref = group_reference(P, s, dy, *d["range"], d["axis"], d["gs"], rounding=d["rounding"])
        clipped, total = clipped + int(ref["clipped"].sum()), total + P.size
        got = _arena_pair(dev, d, P, s, dy)
        _compare(got, ref, f"draw {d}")
        singles.append(got)
        data.append((P, s, dy))
    assert 0.1 * total <= clipped <= 0.9 * total, f"{clipped} of {total} elements clipped over the whole set"
    for rounding in ROUNDINGS:
        mine = [i for i, d in enumerate(draws) if d["rounding"] == rounding]
        tensors = [Tensor(dev, *data[i], (draws[i]["R"], draws[i]["C"], draws[i]["axis"], draws[i]["gs"]), draws[i]["range"], 1.0,
                          offset=draws[i]["residue"] // 4) for i in mine]
        assert all(t.P.data_ptr() % 16 == draws[i]["residue"] for t, i in zip(tensors, mine))
        for i, got in zip(mine, _run_batch(tensors, rounding)):
            w = singles[i]
            _same(got, (w["out"], w["dP"], w["ds"], w["clipped"]), f"draw {draws[i]} in the {rounding} batch")
