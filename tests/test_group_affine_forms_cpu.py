"""CPU side of tests/test_gpu_group_affine_forms.py: the inputs of its data-driven tests meet their conditions ON THE REFERENCE
(tests/_group_affine_reference.py), before any kernel is involved -- the straddle share and the scales of the edge quotients, every
special u = P - b reached exactly in every shape, every bad scale next to a non-zero offset, the clipped shares, and distinct
factors per slot of the two batches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _bounds import stable_seed                                                               # noqa: E402
from _group_affine_reference import (FULL_BATCH, FULL_BATCH_SYMMETRIC, PLANTED_U, edge_offset_case, form_batch_factors,      # noqa: E402
                                     full_batch_factors, full_batch_inputs, group_affine_reference, make_affine_case, window_offset_case)
from _group_forms import (BAD_SCALES, EDGE_RANGES, EDGE_SHAPES, FORM_CASES, GEOMETRY_DRAWS, LARGE, WINDOW_SHAPES, launch_shape,      # noqa: E402
                          power_of_two_share, random_geometry, window_group_case)
from _group_reference import expand_scale, group_reference, make_case                        # noqa: E402
import _group_stats_reference as G                                                            # noqa: E402

_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731
SET = [(37, 5, 0, 8), (256, 260, 0, 32), (96, 130, 0, 96), (7, 27, 1, 8), (64, 576, 1, 128), (33, 4100, 1, 128), (1, 10, 1, 10),
       (1, 512, 1, 512), (300, 64, 0, 1), (40, 64, 1, 4)]      # of tests/test_gpu_group_affine_batch.py


def _bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("rounding", ("floor", "nearest"))
def test_edge_offset_inputs(rounding):
    """In at least 65 % of the triples the two neighbours of c = fl32(fl32(m s) + b) round to different integers under the
    reference's float32 arithmetic (0.699 .. 0.904 with these seeds); fewer than 1 % of the scales are powers of two; some
    elements clip and some do not; both sides of the range are hit, so the statistics test has something to count."""
    for qmin, qmax in EDGE_RANGES:
        for case in EDGE_SHAPES:
            P, s, b, dy, share = edge_offset_case(stable_seed("affine edge forms", case, qmin, qmax, rounding), *case, qmin, qmax, rounding)
            what = f"{case} [{qmin}, {qmax}] {rounding}"
            assert share >= 0.65, f"{what}: {share:.3f}"
            assert power_of_two_share(s) < 0.01 and power_of_two_share(b) < 0.01 and np.all(b != 0), what
            assert float(s.min()) >= 2.0 ** -12 and float(s.max()) <= 8.0 and float(np.abs(b / s).max()) <= 6.0
            ref = group_affine_reference(P, s, b, dy, qmin, qmax, case[2], case[3], rounding=rounding)
            assert 0 < int(ref["clipped"].sum()) < P.size, what
            assert (ref["q0"] < qmin).any() and (ref["q0"] > qmax).any() and bool((ref["db"] != 0).any()), what
            # the triples are what they claim: the three members of a triple are consecutive floats
            sb, bb = expand_scale(s, *case), expand_scale(b, *case)
            t = (P - bb) / sb
            assert float(np.abs(t - np.rint(2 * t) / 2).max()) < 1e-2, f"{what}: a quotient is not next to an integer or a tie"


def test_window_offset_inputs():
    """Every value of PLANTED_U is u = fl32(P - b) of a planted element, exactly, in every shape; no aligned float4 of a row holds two
    planted elements; every planted group has an ordinary scale; every value of BAD_SCALES is reached, in the places
    window_group_case puts them, and every group keeps a non-zero offset."""
    for case in WINDOW_SHAPES:
        R, C, axis, gs = case
        seed = stable_seed("affine window", case)
        P, s, b, dy, bad, planted = window_offset_case(seed, *case)
        _, s_sym, _, bad_sym = window_group_case(seed, *case)
        assert np.array_equal(bad, bad_sym) and np.array_equal(_bits(s[bad]), _bits(s_sym[bad]))
        assert set(_bits(s[bad]).tolist()) == set(_bits(BAD_SCALES).tolist())
        assert np.all(b != 0) and np.all(b[bad] != 0) and np.isfinite(b[bad]).all()
        with np.errstate(all="ignore"):
            u = P - expand_scale(b, *case)
        assert u.dtype == np.float32
        quads = set()
        for name, _, _, want in PLANTED_U:
            assert len(planted[name]) >= 2, f"{case}: {name}"
            for r, c in planted[name]:
                got = u[r, c]
                assert (np.isnan(want) and np.isnan(got)) or _bits(got)[0] == _bits(want)[0], f"{case}: u at {(r, c)} is {got!r}, not {name}"
                assert (r, c // 4) not in quads
                quads.add((r, c // 4))
                g = (r // gs, c) if axis == 0 else (r, c // gs)
                assert not bad[g] and 2.0 ** -9 <= float(s[g]) <= 2.0 ** -5
        assert len(PLANTED_U) == 9 and {n for n, *_ in PLANTED_U} >= {"2^-81", "2^-80", "2^81", "below 2^81", "denormal", "+0", "+Inf", "-Inf", "NaN"}
        tiny = float(np.float32(2.0 ** -126))
        assert 0 < float(u[planted["denormal"][0]]) < tiny and abs(float(P[planted["denormal"][0]])) >= tiny
        assert np.isfinite(P[planted["+Inf"][0]]) and np.isfinite(P[planted["-Inf"][0]]) and np.isinf(P[planted["NaN"][0]])
        for rounding in ("floor", "nearest"):
            with np.errstate(all="ignore"):
                ref = group_affine_reference(P, s, b, dy, -8, 7, axis, gs, rounding=rounding)
            assert np.isnan(ref["ds"]).any() and np.isfinite(ref["ds"][~bad]).any() and np.isnan(ref["out"]).any()
            assert np.isfinite(ref["db"]).all()      # dy is finite: the offset's sum never sees u


def test_factors_of_the_two_batches_are_distinct():
    cases = [c for c in FORM_CASES if c != LARGE]
    f = form_batch_factors(len(cases))
    assert len({k for k, _ in f}) == len({kb for _, kb in f}) == len(cases) == 19
    assert all(k != kb for k, kb in f)
    full = [full_batch_factors(i) for i in range(FULL_BATCH)]
    assert len({k for k, _ in full}) == len({kb for _, kb in full}) == FULL_BATCH == 256
    assert all(k == 1.0 + i / 256.0 and kb == 2.0 - i / 256.0 for i, (k, kb) in enumerate(full))      # exact in float32
    # slot >= 128 and slot - 128 differ in both factors: an index taken modulo 128 shows
    assert all(full[i][0] != full[i - 128][0] and full[i][1] != full[i - 128][1] for i in range(128, 256))


def test_full_batch_inputs():
    """Every eighth tensor is symmetric, slots 254 and 255 are a row and a column form with an offset, the last ten slots hold every
    shape of the set, and each of them clips some elements and keeps some."""
    geoms = [SET[(i + 3) % len(SET)] for i in range(FULL_BATCH)]
    assert geoms[254][2] == 1 and geoms[255][2] == 0 and 254 % FULL_BATCH_SYMMETRIC and 255 % FULL_BATCH_SYMMETRIC
    assert {geoms[i] for i in range(FULL_BATCH - len(SET), FULL_BATCH)} == set(SET)
    assert {launch_shape(*g)["form"] for g in SET} == {"cols4", "cols1", "rows4", "rows1"}
    for i in range(FULL_BATCH - len(SET), FULL_BATCH):
        P, s, b, dy = full_batch_inputs(i, geoms[i])
        assert (b is None) == (i % FULL_BATCH_SYMMETRIC == 0)
        k, kb = full_batch_factors(i)
        if b is None:
            ref = group_reference(P, s, dy, -8, 7, geoms[i][2], geoms[i][3], k=k)
        else:
            ref = group_affine_reference(P, s, b, dy, -8, 7, geoms[i][2], geoms[i][3], k=k, kb=kb)
            assert bool((ref["db"] != 0).any())
        assert 0 < int(ref["clipped"].sum()) < P.size
    a, b_ = full_batch_inputs(17, geoms[17]), full_batch_inputs(27, geoms[27])      # the same shape, other data
    assert geoms[17] == geoms[27] and not np.array_equal(a[0], b_[0])


def test_random_geometry_with_offsets_clips_and_keeps():
    """Over the 64 draws between 10 % and 90 % of all elements clip with make_affine_case's spread N(0, 1) * 8 s, and so do the
    draws of each of the three ranges taken alone: no spread per range is needed."""
    per_range = {}
    for i in range(GEOMETRY_DRAWS):
        d = random_geometry(i)
        P, s, b, dy = make_affine_case(d["k"], d["R"], d["C"], d["axis"], d["gs"])
        assert np.all(b != 0)
        ref = group_affine_reference(P, s, b, dy, *d["range"], d["axis"], d["gs"], rounding=d["rounding"])
        c = per_range.setdefault(d["range"], [0, 0])
        c[0], c[1] = c[0] + int(ref["clipped"].sum()), c[1] + P.size
    assert len(per_range) == 3
    for range_, (clipped, total) in per_range.items():
        assert 0.1 * total <= clipped <= 0.9 * total, f"{range_}: {clipped} of {total} clipped"
    clipped, total = (sum(v[k] for v in per_range.values()) for k in (0, 1))
    assert 0.1 * total <= clipped <= 0.9 * total, f"{clipped} of {total} clipped"


def test_statistics_reference_on_the_edge_inputs():
    """What tests/test_gpu_group_affine_forms.py::test_statistics_on_the_edge_inputs relies on: below + above is the backward's clip
    count on the reference, and the histogram counts every element."""
    for rounding in ("floor", "nearest"):
        for case in (EDGE_SHAPES[0], EDGE_SHAPES[2]):
            P, s, b, dy, _ = edge_offset_case(stable_seed("affine edge forms", case, -8, 7, rounding), *case, -8, 7, rounding)
            ref = group_affine_reference(P, s, b, dy, -8, 7, case[2], case[3], rounding=rounding)
            st = G.group_stats_reference(P, s, -8, 7, case[2], case[3], b=b, rounding=rounding)
            assert np.array_equal(st["below"] + st["above"], ref["clipped"]) and st["below"].sum() > 0 and st["above"].sum() > 0
            assert int(st["hist"].sum()) == P.size and int(st["hist"].min()) > 0


def test_symmetric_window_inputs_are_unchanged():
    """interleave_bad_scales was cut out of window_group_case: the symmetric file's inputs keep their bits."""
    case = WINDOW_SHAPES[0]
    P, s, dy, bad = window_group_case(stable_seed("window", case), *case)
    Pm, sm, dym = make_case(stable_seed("window", case), *case)
    assert np.array_equal(_bits(s[~bad]), _bits(sm[~bad])) and np.array_equal(_bits(dy), _bits(dym))
    assert int(bad.sum()) == 64 and int((_bits(P) != _bits(Pm)).sum()) == 60      # 6 rounds of the 10 special values
