"""CPU side of tests/test_gpu_matrix_forms.py: the case tables of tests/_matrix_forms.py reach every run-time branch of the launch
arithmetic around the matrix-path kernels, the rows that file adds are NEEDED for it (the same reach check fails on the shapes the
earlier GPU files run), the NumPy packers address every byte of the padded buffers of the new extents exactly once, and the inputs
of the new cases meet their conditions ON THE REFERENCE, before any kernel is involved.

The ``*_form`` functions restate the host rules of csrc/lq_kernels.hip; they describe which branch a case takes and are never used
to compute an expected output."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_reference as I                                                                     # noqa: E402
import _matrix_forms as MF                                                                    # noqa: E402
import _mx_conv_reference as C                                                                # noqa: E402
import _mx_gemm_reference as G                                                                # noqa: E402

LINE = MF.ONE_PER_LINE


def _sub(d, want):
    return {k: d[k] for k in want}


# ------------------------------------------------------------------------------------------------------------ the new rows
def test_the_new_rows_take_the_branches_they_name():
    want = [dict(V=4, team=64, step=256, nbs=3, cache=4096, nonlast_tail=True, dead_rows=14),
            dict(V=1, team=64, step=64, nbs=3, cache=1024, nonlast_tail=True),
            dict(V=1, team=64, nbs=3, cache=1024, nonlast_tail=True)]
    for (case, why), w in zip(MF.NEW_I8_QUANTIZE, want):
        assert _sub(MF.i8_quantize_form(*case), w) == w, f"{case} ({why})"
    blocks = lambda c: [(b["length"], b["written"] - b["length"] if b["last"] else 0, b["tail_read"], b["tail_write"])      # noqa: E731
                        for b in MF.i8_quantize_form(*c)["blocks_of_k"]]
    assert blocks((2, 8420, 4160, True)) == [(4160, 0, True, True), (4160, 0, True, True), (100, 28, False, False)]
    assert blocks((2, 8420, 4160, False)) == [(4160, 0, True, True), (4160, 0, True, True), (100, 28, False, False)]
    assert blocks((2, 2246, 1088, True)) == [(1088, 0, True, True), (1088, 0, True, True), (70, 58, False, False)]
    assert 4160 - 4096 == 64 and 4160 - 1024 == 3136 and 1088 - 1024 == 64      # the tails of the non-last blocks

    want = [dict(ps=2, a_every=1, b_every=2, steps=[2, 2, 2, 1]), dict(ps=2, a_every=2, b_every=1, steps=[2, 2, 2, 1]),
            dict(ps=1, a_every=1, b_every=3, periods=7), dict(ps=1, a_every=3, b_every=1, periods=7),
            dict(ps=3, a_every=1, b_every=1, steps=[3, 3, 1]),
            dict(ps=5, KT=5, a_every=1, b_every=LINE, a_whole=True, periods=1), dict(ps=5, KT=5, a_every=LINE, b_every=1, b_whole=True),
            dict(ps=2, a_every=3, b_every=1, a_whole=True, steps=[2, 2, 1])]
    assert len(want) == len(MF.NEW_I8_GEMM)
    for (case, why), w in zip(MF.NEW_I8_GEMM, want):
        assert _sub(MF.i8_gemm_form(*case), w) == w, f"{case} ({why})"
    # the end-to-end row: block 128 on K = 70 is one scale block, and the GEMM sees ps = KT
    e = MF.I8_END_TO_END
    assert MF.i8_quantize_form(*e["x"], e["act_block"])["nbs"] == 1 and MF.i8_pack_form(*e["w"], 0, e["gs"])["block"] == 0
    assert _sub(MF.i8_gemm_form(3, 40, 70, 128, 0), ("ps", "KT", "a_whole", "a_every", "b_every")) == \
        dict(ps=2, KT=2, a_whole=True, a_every=1, b_every=LINE)

    want = [dict(M=289, K=27, chunks=2, grid=8, dead_lines=15, dead_kblocks=3, idle_scale_bytes=3),
            dict(M=675, K=180, chunks=3, grid=24, idle_scale_bytes=2, dead_kblocks=2),
            dict(M=256, K=36, chunks=1, full_last_chunk=True, dead_lines=0, idle_threads=0),
            dict(M=2 * 64, K=27, padded_windows=2 * 28), dict(M=21, K=30, padded_windows=0),
            dict(M=18, K=70, wide_kernel=True, flat_block=True), dict(M=16, K=387, idle_scale_bytes=0, dead_kblocks=3)]
    for (g, why), w in zip(MF.NEW_IM2COL, want):
        assert _sub(MF.mx_im2col_form(g), w) == w, f"{C.geom_id(g)} ({why}): {MF.mx_im2col_form(g)}"
    assert C.padding_of(MF.NEW_GEOMS[4]) == (0, 2, 1, 0) and C.dims(MF.NEW_GEOMS[4])[2:] == (3, 7)
    assert _sub(MF.mx_im2col_form(MF.EXPANDED_GEOM), ("M", "chunks")) == dict(M=867, chunks=4)


# ------------------------------------------------------------------------------------------------------------------ reach
def _i8_quantize_reach(cases):
    f = [MF.i8_quantize_form(*c) for c in cases]
    return dict(V={d["V"] for d in f}, team={d["team"] for d in f}, nonlast_tail={d["V"] for d in f if d["nonlast_tail"]},
                last_tail=any(d["last_tail"] for d in f), dead_rows=any(d["dead_rows"] for d in f))


def test_i8_quantize_reach():
    r = _i8_quantize_reach(MF.FORMS_I8_QUANTIZE)
    assert r["V"] == {1, 4} and r["team"] == {16, 32, 64} and r["nonlast_tail"] == {1, 4} and r["last_tail"] and r["dead_rows"]
    f = [MF.i8_quantize_form(*c) for c in MF.FORMS_I8_QUANTIZE]
    assert any(d["blocks"] > 1 for d in f)
    # the kernel's ``pair >= pairs`` return is dead code under the host's rule: a scale block is at least 64 long, so a team is at
    # least 16 lanes, a thread block holds at most 16 pairs, and the pairs are a multiple of 16 (whole tiles of lines)
    assert all(d["dead_teams"] == 0 and d["per_block"] <= 16 for d in f)
    # the new rows are needed: the earlier shapes run the second tail loop to the padded end of the row only
    old = _i8_quantize_reach(MF.OLD_I8_QUANTIZE)
    assert old["nonlast_tail"] == set() and old["last_tail"] and old["V"] == {1, 4} and old["team"] == {16, 32, 64}


def _i8_gemm_reach(cases):
    f = [MF.i8_gemm_form(*c) for c in cases]
    return dict(ps={d["ps"] for d in f}, ps_is_kt=any(d["ps"] == d["KT"] for d in f), a_every={d["a_every"] for d in f},
                b_every={d["b_every"] for d in f},
                long_period_in_long_block=any(d["ps"] >= 2 and e != LINE and e >= 2 for d in f for e in (d["a_every"], d["b_every"])),
                short_last=any(d["short_last"] for d in f), full_last=any(not d["short_last"] for d in f),
                a_whole=any(d["a_whole"] for d in f), b_whole=any(d["b_whole"] for d in f),
                three_step_periods=any(d["ps"] == 3 and d["periods"] >= 2 for d in f))


def test_i8_gemm_reach():
    r = _i8_gemm_reach(MF.FORMS_I8_GEMM)
    assert {1, 2, 3} <= r["ps"] and r["ps_is_kt"] and r["a_every"] == {1, 2, 3, LINE} and r["b_every"] == {1, 2, 3, LINE}
    assert r["long_period_in_long_block"] and r["short_last"] and r["full_last"] and r["a_whole"] and r["b_whole"]
    assert r["three_step_periods"]
    f = [MF.i8_gemm_form(*c) for c in MF.FORMS_I8_GEMM]
    assert any(d["clamped_m"] for d in f) and any(d["clamped_n"] for d in f) and any(d["leaving"] for d in f)
    assert any(d["grid"][0] > 1 for d in f) and any(d["grid"][1] > 1 for d in f)
    # needed: the earlier block pairs know (ps, every) = (1, 1), (1, 2), (2, 1) and one scale per line only
    old = _i8_gemm_reach(MF.OLD_I8_GEMM)
    assert not old["long_period_in_long_block"] and 3 not in old["a_every"] | old["b_every"]
    assert not old["a_whole"] and not old["b_whole"] and not old["three_step_periods"]
    assert old["a_every"] == old["b_every"] == {1, 2, LINE}


def _im2col_reach(geoms):
    f = [MF.mx_im2col_form(g) for g in geoms]
    return dict(chunks={d["chunks"] for d in f}, full_last_chunk=any(d["full_last_chunk"] for d in f),
                padded=any(d["padded_windows"] for d in f), wide=any(d["wide_kernel"] and d["flat_block"] for d in f),
                short_k=any(d["K"] < 32 for d in f), idle={d["idle_scale_bytes"] for d in f}, j_wrap=any(d["j_wrap"] for d in f),
                i_wrap=any(d["i_wrap"] for d in f), asymmetric=any(len(set(C.padding_of(g))) > 1 for g in geoms))


def test_im2col_reach():
    r = _im2col_reach(MF.FORMS_IM2COL)
    assert {1, 2, 3} <= r["chunks"] and r["full_last_chunk"] and r["padded"] and r["wide"] and r["short_k"]
    assert r["idle"] == {0, 1, 2, 3} and r["j_wrap"] and r["i_wrap"] and r["asymmetric"]
    f = [MF.mx_im2col_form(g) for g in MF.FORMS_IM2COL]
    assert any(d["dead_lines"] and d["chunks"] > 1 for d in f) and any(d["dead_kblocks"] for d in f)
    # needed: every earlier geometry has at most 256 padded lines, none a window in the padding or a kernel row above 32 taps.
    # (More than one chunk IS reached outside this table, by the CIFAR model of tests/test_gpu_mx_conv.py, whose conv outputs are
    # compared bit for bit with the composition through unfold: profiles/matrix_forms/mutations.txt, (a).  The new rows hold the
    # operand's own bytes to the NumPy reference at those extents.)
    old = _im2col_reach(C.GEOMS)
    assert old["chunks"] == {1} and not old["full_last_chunk"] and not old["padded"] and not old["wide"]
    assert old["idle"] == {1, 2, 3}                          # no earlier K has a whole number of scale dwords (KT % 4 == 0)
    explicit = [g for g in MF.FORMS_IM2COL if not isinstance(g.padding, str)]
    assert len(explicit) == 2 and all(isinstance(g.padding, str) for g in C.GEOMS)


def _fused_reach(shapes):
    f = [MF.mx_gemm_quantize_form(*s) for s in shapes]
    return dict(no_k=any(d["no_k"] for d in f), idle=any(d["idle"] for d in f), odd_mt=any(d["odd_mt"] for d in f),
                even_mt=any(not d["odd_mt"] for d in f), n_mod32={min(d["n_mod32"], 2) for d in f},
                leaving=any(d["leaving"] for d in f), clamped_n=any(d["clamped_n"] for d in f))


def test_fused_gemm_reach():
    old = MF.OLD_FUSED
    r = _fused_reach(old + [s for s, _ in MF.NEW_FUSED])
    assert r["no_k"] and r["idle"] and r["odd_mt"] and r["even_mt"] and r["leaving"] and r["clamped_n"]
    assert r["n_mod32"] == {0, 1, 2}                         # 2 stands for every other residue
    # needed: no earlier shape has a whole number of output blocks, so every one of them masks columns in its last live block
    r = _fused_reach(old)
    assert r["n_mod32"] == {1, 2} and r["no_k"] and r["idle"] and r["odd_mt"]
    assert _sub(MF.mx_gemm_quantize_form(17, 32, 160), ("grid", "no_k", "idle_scale_bytes")) == dict(grid=(2, 1), no_k=3, idle_scale_bytes=3)


def test_the_earlier_shapes_reach_every_form_of_the_other_kernels():
    """k_mx_operand, k_mx_gemm and k_i8_pack take no branch from the extents beyond those below, and the shapes of
    tests/test_gpu_mx_gemm.py and tests/test_gpu_i8.py reach all of them: tests/test_gpu_matrix_forms.py adds no row for them."""
    f = [MF.mx_operand_form(*c) for c in MF.FORMS_MX_OPERAND]
    assert {(d["fp4"], d["vec"], d["line_fast"]) for d in f} == {(a, v, lf) for a in (True, False) for v, lf in
                                                                 ((False, True), (True, False), (False, False))}
    assert any(d["blocks"] > 1 for d in f) and any(d["dead_threads"] for d in f) and any(d["dead_lines"] for d in f)
    assert any(d["dead_kblocks"] for d in f) and {0, 1} <= {d["idle_scale_bytes"] for d in f} | {0}
    assert any(d["idle_scale_bytes"] for d in f) and any(d["dead_kblocks"] == 0 for d in f)
    f = [MF.mx_gemm_form(*s) for s in MF.FORMS_MX_GEMM]
    assert any(d["clamped_m"] for d in f) and any(d["clamped_n"] for d in f) and any(d["leaving"] for d in f)
    assert any(d["short_last_group"] for d in f) and any(not d["short_last_group"] for d in f) and any(d["KG"] > 1 for d in f)
    assert any(d["grid"][0] > 1 for d in f) and any(d["grid"][1] > 1 for d in f)
    f = [MF.i8_pack_form(*c) for c in MF.FORMS_I8_PACK]
    assert {d["line_fast"] for d in f} == {True, False} and {d["block"] for d in f} == {0, 64, 128}
    assert any(d["dead_threads"] for d in f) and any(d["dead_lines"] for d in f) and any(d["dead_runs"] for d in f)
    assert any(d["blocks"] > 1 for d in f)


# -------------------------------------------------------------------------------------------------------------- offsets
def test_the_packers_address_every_byte_of_the_new_buffers_once():
    e = MF.I8_END_TO_END
    i8 = {(c[0], c[1]) for c, _ in MF.NEW_I8_QUANTIZE} | {(L, c[2]) for c, _ in MF.NEW_I8_GEMM for L in c[:2]} | \
        {e["x"], (e["w"][1], e["w"][0])}
    for L, K in sorted(i8):
        LT, KT, _ = I.layout_dims(L, K, 0)
        ln, k = np.meshgrid(np.arange(16 * LT), np.arange(64 * KT), indexing="ij")
        assert np.array_equal(np.sort(I.code_offset(KT, ln, k).reshape(-1)), np.arange(LT * KT * 1024)), (L, K)
    mx = {C.dims(g)[:2] for g in MF.NEW_GEOMS + [MF.EXPANDED_GEOM]} | {(s[0], s[1]) for s, _ in MF.NEW_FUSED}
    for L, K in sorted(mx):
        LT, KT, KG = G.layout_dims(L, K)
        for name in G.OPERAND_FORMATS:
            off, shift, _ = G._layout_offsets(name, 16 * LT, 128 * KT)
            per_byte = 2 if name == "fp4_e2m1" else 1
            slot = (off * per_byte + shift // 4).reshape(-1)
            assert np.array_equal(np.sort(slot), np.arange(LT * KT * 64 * (16 if per_byte == 2 else 32) * per_byte)), (name, L, K)
            _, _, soff = G._layout_offsets(name, 16 * LT, 512 * KG)
            assert np.array_equal(np.sort(soff.reshape(-1)), np.arange(LT * KG * 256)), (name, L, K)


# ---------------------------------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("case", [c for c, _ in MF.NEW_I8_QUANTIZE if c[3]], ids=lambda c: "x".join(map(str, c[:3])))
def test_long_quantize_inputs(case):
    """Every scale block with a part the registers do not hold has its maximum there, in the 16-byte and in the 4-byte form, and the
    planted value alone fixes its scale; no case saturates more than half of its codes."""
    M, K, block, _ = case
    x, planted = MF.long_quantize_case(M, K, block)
    ref = I.operand_of_activation(x, block)
    forms = [MF.i8_quantize_form(M, K, block, al) for al in (True, False)]
    nbs = forms[0]["nbs"]
    assert sorted((r, b) for r, b, _ in planted) == [(r, b) for r in range(M) for b in range(nbs) if forms[0]["blocks_of_k"][b]["tail_read"]]
    assert len(planted) == 2 * M
    alone = np.zeros_like(x)
    for r, blk, col in planted:
        c0 = blk * block
        assert int(np.abs(x[r, c0:c0 + block]).argmax()) == col - c0
        assert all(col - c0 >= f["cache"] for f in forms), "the maximum lies in what a form caches"
        alone[r, col] = x[r, col]
    keep = np.array([[forms[0]["blocks_of_k"][b]["tail_read"] for b in range(nbs)]] * M)
    assert np.array_equal(ref["scales"][keep], I.operand_of_activation(alone, block)["scales"][keep])
    assert len(set(ref["scales"][keep].tolist())) == keep.sum(), "two planted scales agree: a swapped block would not show"
    assert MF.i8_saturated_share(ref) <= 0.5 and np.abs(ref["codes"][:, -1]).max() > 0


def test_gemm_inputs():
    """Random codes over the whole byte: every period sum fits int32 (asserted inside gemm_reference), under half saturated, and
    the scales of the blocks of a line all differ, so that a scale taken from the wrong block changes the result."""
    for (case, why) in MF.NEW_I8_GEMM:
        a, b, bias = I.gemm_case(*case)
        I.gemm_reference(a, b, bias)
        for op in (a, b):
            assert MF.i8_saturated_share(op) <= 0.5
            s = op["scales"]
            assert all(len(set(row.tolist())) == s.shape[1] for row in s), case


def test_end_to_end_inputs():
    """quantize(block = 128) of K = 70 into the GEMM: one scale block; most of A's and of B's codes are non-zero and under half of
    them saturated; the product holds many distinct finite values, so a GEMM that ignored an operand, a period or a scale shows."""
    e = MF.I8_END_TO_END
    x, P, s = MF.end_to_end_case()
    ra, rb = I.operand_of_activation(x, e["act_block"]), I.operand_of_parameter(P, s, -128, 127, 0, e["gs"], "nearest")
    assert ra["scales"].shape == (3, 1) and ra["codes"].shape == (3, 70) and rb["codes"].shape == (40, 70)
    assert np.isfinite(ra["scales"]).all() and ra["scales"][2, 0] == np.float32(2.0 ** -126) and not ra["codes"][2].any()
    assert len(set(ra["scales"][:, 0].tolist())) == 3
    for op in (ra, rb):
        assert (op["codes"] != 0).mean() > 0.5 and MF.i8_saturated_share(op) <= 0.5
    assert (ra["codes"][:2] != 0).mean() > 0.9 and (np.abs(ra["codes"][:2]).max(axis=1) == 127).all()
    y = I.gemm_reference(ra, rb)
    fin = y[np.isfinite(y)]
    assert np.isnan(y[:, -1]).all() and np.isfinite(y[:, :-1]).all()      # the NaN scale of the kernel's last column, and only it
    assert np.unique(fin[fin != 0]).size >= 70 and not y[2, :-1].any()


def test_fused_inputs():
    """The new row of the operand-out GEMM on the references alone: neither input operand nor, for either output format and method,
    the operand of relu(Y + bias) saturates more than half of its codes, and the output holds live codes."""
    fa, fb = MF.FUSED_PAIR
    for shape, _ in MF.NEW_FUSED:
        c = G.random_case(*shape, fa, fb)
        a, _ = G.operand_of_activation(c["x"], fa, "mx")
        b = G.operand_of_parameter(c["W"], c["sw"], fb, 0)
        assert MF.mx_saturated_share(a) <= 0.5 and MF.mx_saturated_share(b) <= 0.5
        y, _ = G.gemm_reference(a, b, c["bias"])
        y = np.maximum(y, 0.0).astype(np.float32)
        assert (y > 0).mean() > 0.25
        for out_format in G.OPERAND_FORMATS:
            for method in C.METHODS:
                out, _ = G.operand_of_activation(y, out_format, method)
                assert MF.mx_saturated_share(out) <= 0.5 and (out.codes != 0).mean() > 0.25, (shape, out_format, method)


def _ref_operand(g, name, method):
    return G.operand_of_activation(C.im2col(C.gaussian_input(g), g), name, method)[0]


@pytest.mark.parametrize("g", MF.NEW_GEOMS, ids=C.geom_id)
def test_im2col_inputs(g):
    """The reference's im2col with explicit padding is F.unfold of the padded input; no format saturates more than half of its
    codes; the windows in the padding are zero blocks: byte 1 under "mx" -- what the rule gives a zero block -- and code 0."""
    x = C.gaussian_input(g)
    top, bottom, left, right = C.padding_of(g)
    u = F.unfold(F.pad(torch.from_numpy(x), (left, right, top, bottom)), (g.KH, g.KW), stride=(g.sh, g.sw))
    A = C.im2col(x, g)
    assert np.array_equal(A, u.transpose(1, 2).reshape(-1, u.shape[1]).numpy())
    form = MF.mx_im2col_form(g)
    empty = ~np.abs(C.im2col(np.ones_like(x), g)).any(axis=1)
    assert int(empty.sum()) == form["padded_windows"]
    for name in G.OPERAND_FORMATS:
        for method in C.METHODS:
            ref = _ref_operand(g, name, method)
            assert MF.mx_saturated_share(ref) <= 0.5, (name, method)
            zero_byte = G.operand_of_activation(np.zeros((1, 32), np.float32), name, method)[0].bytes[0, 0]
            assert (ref.bytes[empty] == zero_byte).all() and not ref.codes[empty].any()
            if method == "mx":
                assert zero_byte == 1
    if g == MF.PADDED_GEOM:
        assert empty.sum() == 56 and not empty.all() and (_ref_operand(g, "fp8_e4m3", "mx").bytes[~empty] != 1).all()


def test_expanded_input():
    """The stride-0 case: three images that are one; its reference is that of the contiguous copy."""
    g = MF.EXPANDED_GEOM
    one = C.gaussian_input(MF.TWO_CHUNKS)
    x = np.ascontiguousarray(np.broadcast_to(one, (g.B, g.C, g.H, g.W)))
    A = C.im2col(x, g)
    assert A.shape == (867, 27) and np.array_equal(A[:289], A[289:578]) and np.array_equal(A[:289], C.im2col(one, MF.TWO_CHUNKS))
