"""The restated references of the memory-contract tests (tests/_contract.py) pinned to the float64 oracle
(oracle/lq_oracle_f64.py) where the two must agree exactly: power-of-two scales make the float32 and the float64 quotient, floor
and product the same numbers, so the only difference left is the order of a float64 sum."""
import numpy as np
import pytest

import _contract as C
from _arena import SENTINEL_BYTE
from _bounds import stable_seed
from oracle import lq_oracle_f64 as O64

DESCS = [(1, 1, 10), (6, 1, 1), (1, 50, 9), (128, 10, 1), (33, 5, 3), (2, 3, 900), (4, 3, 256)]


def _inputs(outer, G, inner):
    rng = np.random.default_rng(stable_seed("pin", outer, G, inner))
    n = outer * G * inner
    P = (rng.normal(0, 40.0, size=n)).astype(np.float32)
    dy = (rng.normal(0, 1, size=n) * 10.0 ** rng.uniform(-9, -2, size=n)).astype(np.float32)
    s = (2.0 ** rng.integers(-2, 3, size=G)).astype(np.float32)
    return P, dy, s


@pytest.mark.parametrize("lam", [1e-10, 1e-6, 3e-2])
@pytest.mark.parametrize("desc", DESCS)
def test_nq_reference_is_the_f64_oracle(desc, lam):
    P, dy, s = _inputs(*desc)
    ref = C.nq_reference(P, s, dy, lam, *desc)
    ds64 = O64.scale_grad(P, s, lam, dy, *desc)
    q64, _ = O64.forward(P, s, *desc)
    np.testing.assert_allclose(ref["ds"], ds64, rtol=1e-13, atol=0)
    assert np.array_equal(ref["maxq"].astype(np.float64), np.abs(q64).reshape(desc).max(axis=(0, 2)))
    np.testing.assert_allclose(ref["mean"] * ref["maxq"], ds64, rtol=1e-13, atol=0)
    assert np.all(ref["mean_terms"] >= np.abs(ref["mean"])) and np.all(ref["ds_terms"] == ref["mean_terms"] * ref["maxq"])
    lam64, voted = float(np.float32(lam)), ref["below"] > 0
    assert np.all(ref["mean_terms"][voted] <= 2.0 * lam64 * ref["below"][voted] / (desc[0] * desc[2]))      # r < lambda: at most 2 lambda each
    assert np.all(ref["mean_terms"][~voted] == abs(np.tanh(lam64)))
    assert ref["below"].shape == ref["unsure"].shape == (desc[1],) and ref["below"].max() <= desc[0] * desc[2]


@pytest.mark.parametrize("desc", DESCS)
def test_maxbin_reference_is_the_f64_oracle(desc):
    P, _, s = _inputs(*desc)
    ref = C.maxbin_reference(P, s, *desc)
    assert ref["term64"] == pytest.approx(O64.maxbin_term(P, s, *desc), rel=1e-14)
    assert np.array_equal(ref["mb"].astype(np.float64), ref["mb64"])             # power-of-two scales: the division is exact
    _, ds64, _ = O64.maxbin_term_grads(P, s, 0.3, *desc)
    np.testing.assert_allclose(-0.3 * ref["mb64"] / (desc[1] * s.astype(np.float64)), ds64, rtol=1e-13, atol=0)
    gid = O64.group_ids(*desc)
    t = np.abs(P.astype(np.float64)) / s.astype(np.float64)[gid]
    assert ref["ties"].tolist() == [int((t[gid == g] == t[gid == g].max()).sum()) for g in range(desc[1])]


def test_draw_is_stable_finite_and_in_range():
    P, dy, s = C.draw(3, 5, 7)
    P2, dy2, s2 = C.draw(3, 5, 7)
    assert P is P2 and not P.flags.writeable
    assert P.dtype == dy.dtype == s.dtype == np.float32 and P.shape == dy.shape == (105,) and s.shape == (5,)
    C.draw.cache_clear()
    P3, _, _ = C.draw(3, 5, 7)
    assert np.array_equal(P, P3)
    assert C.POISONS == (SENTINEL_BYTE, 0xFF) and C.descriptor((3, 3, 64, 128), "channelwise") == (9, 64, 128)
    assert C.dense_row_bytes(1, 5, 4100) == 4 * 4100 and C.dense_row_bytes(133, 10, 1) == 40


def test_same_bits_reports_the_first_difference():
    a = np.array([0.0, 1.0, 2.0], np.float32)
    b = np.array([-0.0, 1.0, 2.5], np.float32)
    C.same_bits(a, a.copy(), "same")
    with pytest.raises(AssertionError, match="2 of 3 elements differ, first at 0"):
        C.same_bits(a, b, "x")
