"""CPU side of tests/test_gpu_i8_period_forms.py: the period bookkeeping of the int8 GEMMs -- ``left`` against ps, ``ca`` / ``cb``
against a_every / b_every, the scale-block indices ``ia`` / ``ib`` and the reload that reads them -- is carried by four kernels
(k_i8_gemm<false>, k_i8_gemm<true>, k_i8_gemm_quantize<false>, k_i8_gemm_quantize<true>), two loops and two host functions.
tests/test_matrix_forms_cpu.py proves the reach of the table that k_i8_gemm<false> runs.  This file proves, without a device,

 (a) that FORMS_I8_FUSED and FORMS_I8_GEMM_AFFINE of tests/_matrix_forms.py reach every branch of that bookkeeping and of the 1 x 4
     kernel's tiling, and that the shapes the earlier GPU files run (FR.CASES, all_gemm_affine_keys()) do NOT;
 (b) that the data can tell a wrong scale-block index from the right one: on the reference alone, an operand whose scales (or
     offsets) are shifted by one block gives another output.

The conditions of (b), fixed before any kernel ran:
  C1  a scale shift changes at least 40 % of the output codes;
  C2  an offset shift changes at least 30 bytes (counted on the codes alone, which is the stricter reading);
  C3  every new row, under each activation and bias choice, has at least FR.MIN_DISTINCT = 60 distinct code values and at most 5 % of
      its codes at magnitude 127.

The ``*_form`` functions describe which branch a case takes and are never used to compute an expected output."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import _i8_affine_reference as A                                                              # noqa: E402
import _i8_fused_reference as FR                                                              # noqa: E402
import _i8_reference as R                                                                     # noqa: E402
import _matrix_forms as MF                                                                    # noqa: E402

LINE = MF.ONE_PER_LINE
NEW_FUSED = [c for c, _ in MF.NEW_I8_FUSED]
NEW_GEMM = [c for c, _ in MF.NEW_I8_GEMM]
_ids = lambda k: "x".join(map(str, k))      # noqa: E731
SHIFT_SHARE, OFFSET_BYTES, MAX_SATURATED = 0.40, 30, 0.05


def _sub(d, want):
    return {k: d[k] for k in want}


def _everies(d):
    return [e for e in (d["a_every"], d["b_every"]) if e != LINE]


# ------------------------------------------------------------------------------------------------------------ the new rows
def test_the_new_rows_take_the_branches_they_name():
    want = [dict(ps=1, a_every=2, b_every=1, periods=5, a_changes=2, a_wraps=2, clamped_last=1, masked_cols=8, leaving=1, grid=(1, 1)),
            dict(ps=1, a_every=1, b_every=3, periods=7, b_changes=2, b_wraps=2),
            dict(ps=1, a_every=3, b_every=1, periods=7, a_changes=2, a_wraps=2, clamped_last=2, masked_cols=0, grid=(2, 1)),
            dict(ps=2, a_every=1, b_every=2, steps=[2, 2, 2, 1], b_changes=1),
            dict(ps=2, a_every=2, b_every=1, steps=[2, 2, 2, 1], a_changes=1),
            dict(ps=3, a_every=1, b_every=1, steps=[3, 3, 1]),
            dict(ps=5, KT=5, a_every=1, b_every=LINE, a_whole=True, a_above=True, periods=1),
            dict(ps=5, KT=5, a_every=LINE, b_every=1, b_whole=True, b_above=True, periods=1),
            dict(ps=2, a_every=3, b_every=1, a_whole=True, a_above=True, steps=[2, 2, 1], a_changes=0, b_changes=2),
            dict(ps=1, a_every=1, b_every=4, periods=7, a_changes=6, b_changes=1, grid=(3, 1), clamped_last=3, masked_cols=14, leaving=3)]
    assert len(want) == len(MF.NEW_I8_FUSED)
    for (case, why), w in zip(MF.NEW_I8_FUSED, want):
        assert _sub(MF.i8_gemm_quantize_form(*case), w) == w, f"{case} ({why}): {MF.i8_gemm_quantize_form(*case)}"
    # every table's scale-block index stays inside its buffer (_period_rule asserts it while it walks the loop), the size limit
    # holds, and the tables are what the GPU files import
    for case in MF.FORMS_I8_FUSED:
        MF.i8_gemm_quantize_form(*case)
    for case in MF.FORMS_I8_GEMM_AFFINE:
        MF.i8_gemm_form(*case)
    assert all(M <= 33 and N <= 130 and K <= 448 for M, N, K, _, _ in NEW_FUSED + NEW_GEMM)
    assert MF.FORMS_I8_FUSED[:len(FR.CASES)] == list(FR.CASES) and MF.FORMS_I8_FUSED[len(FR.CASES):] == NEW_FUSED
    assert MF.FORMS_I8_GEMM_AFFINE == A.all_gemm_affine_keys() + NEW_GEMM
    assert set(MF.I8_CONTRACT_KEYS) <= set(NEW_FUSED)
    # the row on which an index of B is in bounds as an index of A: three blocks of A against five of B, ib <= 4, ib / 2 <= 2
    a, b, _ = R.gemm_case(33, 40, 320, 128, 64)
    assert a["scales"].shape[1] == 3 and b["scales"].shape[1] == 5


# ------------------------------------------------------------------------------------------------------------------ reach
def _period_reach(forms):
    """What a table reaches of the loop over K, shared by the 2 x 2 and the 1 x 4 kernels."""
    return dict(a_changes_in_long_block=any(d["a_every"] != LINE and d["a_every"] >= 2 and d["a_changes"] >= 1 for d in forms),
                b_changes_in_long_block=any(d["b_every"] != LINE and d["b_every"] >= 2 and d["b_changes"] >= 1 for d in forms),
                a_wraps=max(d["a_wraps"] for d in forms), b_wraps=max(d["b_wraps"] for d in forms),
                every={e for d in forms for e in _everies(d)},
                long_periods=max([d["periods"] for d in forms if d["ps"] >= 2], default=0),
                long_period_in_long_block=any(d["ps"] >= 2 and e >= 2 for d in forms for e in _everies(d)),
                ps={d["ps"] for d in forms}, ps3=any(d["ps"] == 3 and d["periods"] >= 2 for d in forms),
                a_whole=any(d["a_whole"] for d in forms), b_whole=any(d["b_whole"] for d in forms),
                a_above=any(d["a_above"] for d in forms), b_above=any(d["b_above"] for d in forms),
                short_last=any(d["short_last"] for d in forms), full_last=any(not d["short_last"] for d in forms))


def _assert_full_period_reach(r):
    assert r["a_changes_in_long_block"] and r["b_changes_in_long_block"]
    assert r["a_wraps"] >= 2 and r["b_wraps"] >= 2
    assert {1, 2, 3} <= r["every"]
    assert r["long_periods"] >= 3 and r["long_period_in_long_block"] and r["ps3"] and {1, 2, 3} <= r["ps"]
    assert r["a_whole"] and r["b_whole"] and r["a_above"] and r["b_above"] and r["short_last"] and r["full_last"]


def test_fused_reach_and_need():
    full = [MF.i8_gemm_quantize_form(*c) for c in MF.FORMS_I8_FUSED]
    old = [MF.i8_gemm_quantize_form(*c) for c in FR.CASES]
    _assert_full_period_reach(_period_reach(full))
    assert {d["clamped_last"] for d in full} == {0, 1, 2, 3}
    assert {d["leaving"] // d["grid"][0] for d in full} == {0, 1, 2, 3}         # per block column
    assert any(d["masked_cols"] and d["clamped_last"] in (1, 2) for d in full), "live_n masks part of a block and part of a tile"
    assert any(d["grid"][0] > 1 for d in full) and any(d["grid"][1] > 1 for d in full) and any(d["dead_lines"] for d in full)
    # needed: every item that the new rows are there for is out of the earlier cases' reach
    r = _period_reach(old)
    assert not r["a_changes_in_long_block"], "A's scale never changes under a_every >= 2"
    assert r["a_wraps"] == 0 and r["b_wraps"] == 1, "cb wraps at most once before a read, ca never"
    assert r["every"] == {1, 2}
    assert r["long_periods"] == 2 and not r["long_period_in_long_block"] and not r["ps3"] and 3 not in r["ps"]
    # (64, 128, 128, 128, 64) has a_block == K, one scale block of A, so a_whole is reached; no block of either operand is above K,
    # which is where the host's min(F / 64, KT) cuts, and B never has a block of at least K
    assert r["a_whole"] and not r["b_whole"] and not r["a_above"] and not r["b_above"]
    assert MF.i8_gemm_quantize_form(64, 128, 128, 128, 64)["a_whole"] and R.gemm_case(64, 128, 128, 128, 64)[0]["scales"].shape[1] == 1
    assert {d["clamped_last"] for d in old} == {0, 3}
    # the leaving waves are the one item of the list the earlier cases reach already
    assert {d["leaving"] // d["grid"][0] for d in old} == {0, 1, 2, 3}


def test_affine_gemm_reach_and_need():
    full = [MF.i8_gemm_form(*c) for c in MF.FORMS_I8_GEMM_AFFINE]
    old = [MF.i8_gemm_form(*c) for c in A.all_gemm_affine_keys()]
    _assert_full_period_reach(_period_reach(full))
    assert any(d["clamped_m"] for d in full) and any(d["clamped_n"] for d in full) and any(d["leaving"] for d in full)
    assert any(d["grid"][0] > 1 for d in full) and any(d["grid"][1] > 1 for d in full)
    # needed: k_i8_gemm<true> never ran every == 3, a period of two steps in a block of two periods, ps == 3 or a block above K
    r = _period_reach(old)
    assert r["every"] == {1, 2} and not r["long_period_in_long_block"] and not r["ps3"]
    assert not (r["a_whole"] or r["b_whole"] or r["a_above"] or r["b_above"])
    # what the earlier keys reach already: two wraps on either side (K = 320 under blocks of 64 and 128), three periods of two steps
    assert r["a_wraps"] == 2 and r["b_wraps"] == 2 and r["long_periods"] == 3


def test_both_form_functions_state_one_period_rule():
    """The host writes the ps / a_every / b_every rule out twice (i8_gemm, i8_gemm_quantize); the two form functions give the same
    period keys for the same extents and blocks, and the keys i8_gemm_form gained agree with a count made by hand."""
    keys = ("ps", "KT", "a_every", "b_every", "periods", "steps", "short_last", "a_whole", "b_whole", "a_changes", "b_changes", "a_wraps",
            "b_wraps")
    for c in MF.FORMS_I8_FUSED + MF.FORMS_I8_GEMM:
        assert _sub(MF.i8_gemm_form(*c), keys) == _sub(MF.i8_gemm_quantize_form(*c), keys), c
    # K = 448 under blocks of 64 and 192: seven periods; B's block ends after periods 2 and 5, both followed by a read
    d = MF.i8_gemm_form(17, 18, 448, 64, 192)
    assert (d["a_changes"], d["a_wraps"], d["b_changes"], d["b_wraps"]) == (6, 0, 2, 2)
    # K = 128 under blocks of 128 and 64: A's counter reaches 2 at the end of K, where nothing is read any more
    d = MF.i8_gemm_form(64, 128, 128, 128, 64)
    assert (d["a_changes"], d["a_wraps"], d["b_changes"], d["b_wraps"]) == (0, 0, 1, 0)


# -------------------------------------------------------------------------------------------------- the data, on the reference
def _shifted(op, what):
    """``op`` with block j's scale (offset) in place of block j + 1's: what a kernel reads whose index lags one block behind."""
    s = op[what].copy()
    s[:, 1:] = op[what][:, :-1]
    return dict(op, **{what: s})


@functools.lru_cache(maxsize=None)
def _fused_case(key):
    a, b, bias = R.gemm_case(*key)
    return a, b, A.with_offsets(b), bias


def _operand(a, b, bias, activation):
    y = A.gemm_affine_reference(a, b, bias) if "offsets" in b else R.gemm_reference(a, b, bias)
    return R.operand_of_activation(FR.act(y, activation), FR.OUT_BLOCK)


@pytest.mark.parametrize("key", NEW_FUSED, ids=_ids)
def test_fused_rows_exercise_the_codes_and_tell_a_wrong_block(key):
    a, b, ba, bias = _fused_case(key)
    M, N = key[:2]
    sides = [s for s, op in (("a", a), ("b", b)) if op["scales"].shape[1] > 1]
    assert sides or MF.i8_gemm_quantize_form(*key)["periods"] == 1
    for activation in FR.ACTIVATIONS:
        for bv in (bias, None):
            what = f"{key} {activation} bias={bv is not None}"
            for bb in (b, ba):
                op = _operand(a, bb, bv, activation)
                assert op["codes"].shape == (M, N) and not np.isnan(op["scales"]).any()
                distinct = len(np.unique(op["codes"]))
                assert distinct >= FR.MIN_DISTINCT, (what, distinct)                               # C3
                assert MF.i8_saturated_share(op) <= MAX_SATURATED, (what, MF.i8_saturated_share(op))
                for side in sides:                                                                # C1
                    other = _operand(_shifted(a, "scales"), bb, bv, activation) if side == "a" else \
                        _operand(a, _shifted(bb, "scales"), bv, activation)
                    share = float((other["codes"] != op["codes"]).mean())
                    assert share >= SHIFT_SHARE, (what, side, share)
            if "b" in sides:                                                                      # C2
                op, other = _operand(a, ba, bv, activation), _operand(a, _shifted(ba, "offsets"), bv, activation)
                changed = int((other["codes"] != op["codes"]).sum())
                assert changed >= OFFSET_BYTES, (what, changed)
            # the offsets matter at all: the affine output is not the symmetric one
            assert not np.array_equal(_operand(a, ba, bv, activation)["codes"], _operand(a, b, bv, activation)["codes"]), what


@pytest.mark.parametrize("key", NEW_GEMM, ids=_ids)
def test_affine_gemm_rows_tell_a_wrong_block_and_zero_offsets_give_the_symmetric_bits(key):
    a, b, bias = R.gemm_case(*key)
    ba = A.with_offsets(b)
    bits = lambda y: y.view(np.uint32)      # noqa: E731
    y = A.gemm_affine_reference(a, ba, bias)
    assert np.isfinite(y).all() and len(np.unique(y)) >= y.size - 2
    assert not np.array_equal(bits(y), bits(R.gemm_reference(a, b, bias))), "the offsets change nothing"
    for side, op in (("a", a), ("b", ba)):
        if op["scales"].shape[1] > 1:
            other = A.gemm_affine_reference(_shifted(a, "scales"), ba, bias) if side == "a" else \
                A.gemm_affine_reference(a, _shifted(ba, "scales"), bias)
            assert float((bits(other) != bits(y)).mean()) >= SHIFT_SHARE, (key, side)            # C1 on the fp32 result
    if ba["scales"].shape[1] > 1:
        other = A.gemm_affine_reference(a, _shifted(ba, "offsets"), bias)
        assert int((other.view(np.uint8) != y.view(np.uint8)).sum()) >= OFFSET_BYTES, key         # C2
    # offsets of +0: the definition adds RN(c * 0) = +-0 per period, which changes no y (y is never -0: it starts at +0, and a sum
    # that cancels gives +0 under round-to-nearest), so the reference gives lq_i8_gemm's bits
    for bv in (bias, None):
        yz = A.gemm_affine_reference(a, A.with_offsets(b, zero=True), bv)
        assert np.array_equal(bits(yz), bits(R.gemm_reference(a, b, bv))), key
    for op in (a, b):
        assert all(len(set(row.tolist())) == op["scales"].shape[1] for row in op["scales"]), "two blocks of a line share a scale"
    off = ba["offsets"]
    live = off[(np.arange(off.shape[0]) % 5) != 0]
    assert (off[::5] == 0).all() and (live != 0).all() and all(len(set(row.tolist())) == off.shape[1] for row in live)
