"""CPU side of tests/test_gpu_group_forms.py: the case table reaches every run-time branch of the group-wise launch rule, and the
inputs of the data-driven tests meet their conditions ON THE REFERENCE, before any kernel is involved.

``launch_shape`` (tests/_group_forms.py) restates the host rule of csrc/lq_kernels.hip; that it agrees with the library is
recorded launch by launch in profiles/group_forms/kernel_coverage.txt (kernel names and grids of a traced run of the GPU file)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _bounds import stable_seed                                                               # noqa: E402
from _clip_reference import clip_reference                                                    # noqa: E402
from _group_forms import (BAD_SCALES, CLIP_DESCRIPTORS, EDGE_RANGES, EDGE_SHAPES, FORMS, FORM_CASES, GEOMETRY_DRAWS, LARGE, TEAMS,      # noqa: E402
                          WINDOW_SHAPES, edge_clip_case, edge_group_case, edge_scales, form_variants, launch_shape, power_of_two_share,
                          random_geometry, window_clip_cases, window_group_case)
from _group_reference import check_condition, group_reference, make_case                     # noqa: E402
from test_gpu_groupwise import AXIS0, AXIS1                                                   # noqa: E402

_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731
OLD = [(R, C, 0, gs) for R, C, gs in AXIS0] + [(R, C, 1, gs) for R, C, gs in AXIS1]
ALL = [launch_shape(*c) for c in FORM_CASES + OLD]


def test_the_table_takes_the_branches_it_names():
    """Every row of FORMS against its own description: form, team, trips, row split, cap, last group."""
    want = [dict(form="rows4", team=4, last=8), dict(form="rows4", team=16, blocks=2, last=76), dict(form="rows4", team=64, last=552),
            dict(form="rows4", team=64, last=4), dict(form="rows1", team=1), dict(form="rows1", team=8), dict(form="rows1", team=16),
            dict(form="rows1", team=32), dict(form="rows1", team=64, last=2),
            dict(form="rows4", team=2, last=20), dict(form="rows4", team=32, last=100), dict(form="rows1", team=4, last=5),
            dict(form="cols4", nb=40000, trips=2, second_trip=7232), dict(form="cols1", trips=2, second_trip=232),
            dict(form="cols4", trips=2, last=1, second_trip=2233), dict(form="cols1", nz=2, nz_by_gs=2, capped=False),
            dict(form="cols4", nz=2, nz_by_gs=2, capped=False, last=8), dict(form="cols1", nz=2, nz_by_gs=4, capped=True),
            dict(form="cols1", nz=1, nz_by_gs=2, capped=True), dict(form="cols4", nz=2, nz_by_gs=4, capped=True)]
    assert len(want) == len(FORMS) and FORM_CASES[-1] == LARGE
    for (case, why, _), w in zip(FORMS, want):
        got = launch_shape(*case)
        assert {k: got[k] for k in w} == w, f"{case} ({why}): {got}"
    assert launch_shape(70, 12, 1, 3)["form"] == "rows1" and launch_shape(256, 260, 0, 32, aligned16=False)["form"] == "cols1"


def test_every_team_width_of_both_row_forms():
    for form in ("rows4", "rows1"):
        assert {d["team"] for d in ALL if d["form"] == form} == set(TEAMS), form
    # the widths the earlier case lists never launched are reached by FORMS itself
    new = [launch_shape(*c) for c in FORM_CASES]
    assert {4, 16, 64} <= {d["team"] for d in new if d["form"] == "rows4"}
    assert {8, 16, 32, 64} <= {d["team"] for d in new if d["form"] == "rows1"}


def test_group_loop_row_split_and_cap_of_both_column_forms():
    for form in ("cols4", "cols1"):
        mine = [d for d in ALL if d["form"] == form]
        assert any(d["trips"] == 2 and 0 < d["second_trip"] < d["grid_y"] for d in mine), f"{form}: no second trip of a part of the blocks"
        assert {d["nz"] for d in mine} == {1, 2, 4}, form
    capped = [d for d in ALL if d["form"].startswith("cols") and d["capped"]]
    assert {(d["nz"], d["nz_by_gs"]) for d in capped} == {(1, 2), (2, 4)}      # both outcomes of the cap
    assert all(d["blocks_fwd"] >= 2048 > d["blocks_fwd"] // 2 or d["nz"] == 1 for d in capped)
    # the earlier lists hold no second trip and no capped split: FORMS is what reaches them
    assert not any(d.get("trips", 1) > 1 or d.get("capped", False) for d in (launch_shape(*c) for c in OLD))


def test_dead_lanes_and_dead_teams():
    for form in ("cols4", "cols1", "rows4", "rows1"):
        assert any(d["dead"] > 0 for d in ALL if d["form"] == form), f"{form}: no case with dead lanes / teams in the last block"
    assert any(d["form"] == "rows4" and d["blocks"] > 1 and d["dead"] > 0 for d in ALL)


def test_variants():
    v = form_variants()
    assert sum(name == "floor" for _, name in v) == len(FORMS)
    assert sum(name == "unsigned" for _, name in v) == 4
    for case, why, extra in FORMS:
        d = launch_shape(*case)
        if d.get("team") in (16, 64) or d.get("trips", 1) > 1:
            assert "nearest" in extra, f"{case}: {why}"


@pytest.mark.parametrize("case", FORM_CASES, ids=_ids)
def test_inputs_of_the_forms_clip_and_stay_inside(case):
    """10 % clipped, 10 % inside, 90 % of the groups of >= 8 elements mixed -- on the reference alone."""
    P, s, dy = make_case(stable_seed("groupforms", *case), *case)
    check_condition(group_reference(P, s, dy, -8, 7, case[2], case[3]), *case, f"{case}")


def test_edge_quotient_inputs():
    """Fewer than 1 % of the scales are powers of two; in at least 85 % of the triples the two neighbours round differently."""
    s = edge_scales(np.random.default_rng(stable_seed("edge scales")), 4000)
    assert power_of_two_share(s) < 0.01 and float(s.min()) >= 2.0 ** -12 and float(s.max()) <= 8.0
    for rounding in ("floor", "nearest"):
        for qmin, qmax in EDGE_RANGES:
            for case in EDGE_SHAPES:
                P, s, dy, share = edge_group_case(stable_seed("edge", case, qmin, qmax, rounding), *case, qmin, qmax, rounding)
                assert share >= 0.85 and power_of_two_share(s) < 0.01, f"{case} [{qmin}, {qmax}] {rounding}: {share:.3f}"
                ref = group_reference(P, s, dy, qmin, qmax, case[2], case[3], rounding=rounding)
                assert 0 < int(ref["clipped"].sum()) < P.size
            for desc in CLIP_DESCRIPTORS:
                P, s, dy, share = edge_clip_case(stable_seed("edge", desc, qmin, qmax, rounding), desc, qmin, qmax, rounding)
                assert share >= 0.85 and power_of_two_share(s) < 0.01, f"{desc} [{qmin}, {qmax}] {rounding}: {share:.3f}"


def test_window_inputs():
    """Every scale value of BAD_SCALES is reached by every shape; axis 0: exactly one per aligned float4 of columns."""
    for case in WINDOW_SHAPES:
        P, s, dy, bad = window_group_case(stable_seed("window", case), *case)
        if case[2] == 0:
            C = case[1]
            full = bad[:, :C - C % 4].reshape(bad.shape[0], -1, 4)
            assert np.all(full.sum(axis=2) == 1)
        else:
            assert np.all(bad[:, 1:] != bad[:, :-1])
        ref = group_reference(P, s, dy, -8, 7, case[2], case[3])
        assert np.isnan(ref["ds"]).any() and np.isfinite(ref["ds"][~bad]).any() and np.isnan(ref["out"]).any()
    for desc in CLIP_DESCRIPTORS:
        cases = window_clip_cases(stable_seed("window", desc), desc)
        seen = np.concatenate([s[bad] for _, s, _, bad in cases])
        assert set(seen.view(np.uint32).tolist()) == set(BAD_SCALES.view(np.uint32).tolist())
        ref = clip_reference(*cases[0][:3], -8, 7)
        assert np.isfinite(ref["ds"][~cases[0][3]]).any()


def test_random_geometry_draws():
    """The 64 draws are reproducible, cover both axes, both roundings, every residue, every form and a ragged last group; over the
    whole set a tenth of the elements clips and a tenth stays inside."""
    draws = [random_geometry(i) for i in range(GEOMETRY_DRAWS)]
    assert draws == [random_geometry(i) for i in range(GEOMETRY_DRAWS)]
    assert {d["axis"] for d in draws} == {0, 1} and {d["rounding"] for d in draws} == {"floor", "nearest"}
    assert {d["residue"] for d in draws} == {0, 4, 8, 12} and len({d["range"] for d in draws}) == 3
    shapes = [launch_shape(d["R"], d["C"], d["axis"], d["gs"], d["residue"] == 0) for d in draws]
    assert {s["form"] for s in shapes} == {"cols4", "cols1", "rows4", "rows1"}
    assert any(s["last"] != s["gs"] for s in shapes) and any(d["C"] % 4 for d in draws if d["axis"] == 0)
    clipped = total = 0
    for d in draws:
        P, s, dy = make_case(d["k"], d["R"], d["C"], d["axis"], d["gs"])
        ref = group_reference(P, s, dy, *d["range"], d["axis"], d["gs"], rounding=d["rounding"])
        clipped, total = clipped + int(ref["clipped"].sum()), total + P.size
    assert 0.1 * total <= clipped <= 0.9 * total, f"{clipped} of {total} clipped"


def test_python_ops_send_group_size_1_to_axis_1():
    """Why the GPU file calls the C ABI: for gs = 1 both axes describe the same groups, the scale [R][C] fits both splits and
    descriptor.group_geometry answers axis 1 -- through the Python ops the second-trip cases of gs = 1 would run the row kernels."""
    from learned_quantization_amd.descriptor import group_geometry
    assert group_geometry((40000, 4), (4, 1), (40000, 4), 1) == (40000, 4, 1)
    assert group_geometry((33000, 3), (3, 1), (33000, 3), 1) == (33000, 3, 1)
    assert group_geometry((70001, 4), (4, 1), (35001, 4), 2) == (70001, 4, 0)
