"""Memory contract of the single-tensor entry points (include/lq_hip.h, "Conventions"): the contents of `ws` on entry are
irrelevant; no call writes outside the stated extent of its outputs and of [ws, ws + lq_workspace_bytes); no byte outside the
stated extents of its inputs influences a result.

Every call goes through the C ABI with raw pointers into ONE poisoned allocation (tests/_arena.py): inputs, outputs and a workspace
of exactly lq_workspace_bytes() are regions between guards that hold a huge finite sentinel.  After the call the guards and the
inputs must be untouched, the outputs completely written, and the results equal to the reference under the suite's existing
yardsticks (bit for bit: out, q, max|q|, the clipped pair's dP and counts, mb, ties, packed words; tests/_bounds.py against the
float64 restatements: ds, means, penalty terms; the vote count as tests/test_gpu_reverse_walk.py).  A stray store lands in a
guard; a stray load that reaches a result pulls 3.4e38 into a max, a sum or a count.  Every call that takes a workspace runs twice,
the workspace prefilled with the sentinel and with 0xFF bytes (NaN, UINT32_MAX): both runs must pass and agree bit for bit, so a
finalize that reads a partial nobody wrote cannot pass.

The descriptors are the smallest the suite knows to reach each traversal form (tests/test_gpu_parity.py SHAPES / STREAM2_SHAPES,
tests/test_gpu_policy_mix.py); `mis`: P, dy and the dense outputs 4 bytes off a 16-byte base."""
import numpy as np
import pytest
import torch

import _contract as C
from _arena import SENTINEL_BYTE
from _bounds import assert_within_terms, stable_seed
from _clip_reference import clip_reference
from _rne_reference import rne_reference
from oracle import lq_oracle as O
from oracle import lq_oracle_f64 as O64

pytestmark = pytest.mark.gpu

SMALL = [((10,), "scalar"), ((6, 1), "rowwise"), ((50, 9), "rowwise"), ((128, 10), "rowwise"), ((128, 10), "columnwise"),
         ((33, 5, 3), "columnwise"), ((1000, 7, 2), "columnwise"), ((5, 1031), "rowwise"), ((3, 4100), "rowwise"),
         ((2, 3, 9000), "columnwise"), ((100003,), "scalar"), ((4, 3, 16, 16), "columnwise"), ((3, 3, 64, 128), "channelwise")]
# streaming forms (>= 4 M elements); True: the lsq and penalty families run on it too
STREAM = [((1100, 4099), "rowwise", True), ((3, 1500001), "rowwise", False), ((840001, 5), "rowwise", True),
          ((250001, 17), "rowwise", False), ((90001, 49), "rowwise", True), ((4300, 1023), "rowwise", False),
          ((70001, 63), "rowwise", True), ((70001, 64), "rowwise", False), ((2300, 1901), "rowwise", False),
          ((3, 30000, 61), "columnwise", False), ((3, 50000, 32), "columnwise", False),
          ((2100, 2100), "columnwise", True), ((4099, 1028), "columnwise", False), ((700, 1000, 6), "columnwise", False),
          ((2100001, 2), "columnwise", False), ((1398101, 3), "columnwise", True), ((1050001, 4), "columnwise", False),
          ((1030, 4100), "columnwise", True), ((70000, 67), "columnwise", True), ((1100, 4099), "columnwise", False),
          ((42001, 33, 3), "columnwise", True)]
NONTEMPORAL = [(C.descriptor((38001, 450), "columnwise"), "(38001, 450) columnwise"), ((112, 3, 50176), "(112, 3, 50176) channel form")]
MISALIGNED = [((5, 1031), "rowwise"), ((3, 4100), "rowwise"), ((100003,), "scalar"), ((1100, 4099), "rowwise"),
              ((2100, 2100), "columnwise")]


def _cases():
    """[(id, (outer, G, inner), misaligned, families)] in descriptor order: the families of one descriptor run back to back and
    share its inputs (C.draw keeps the last two)."""
    out = []
    for shape, orient in SMALL:
        out.append((f"{shape} {orient}", C.descriptor(shape, orient), False, ("nq", "lsq", "penalty")))
    for shape, orient, dagger in STREAM:
        out.append((f"{shape} {orient}", C.descriptor(shape, orient), False, ("nq", "lsq", "penalty") if dagger else ("nq",)))
    for desc, name in NONTEMPORAL:
        out.append((name, desc, False, ("nq",)))
    for shape, orient in MISALIGNED:
        out.append((f"{shape} {orient} mis", C.descriptor(shape, orient), True, ("nq", "lsq", "penalty")))
    return out


CASES = [pytest.param(desc, mis, fam, id=f"{name} {fam}".replace(" ", "")) for name, desc, mis, fams in _cases() for fam in fams]
LAMS = (1e-10, 3e-2)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from learned_quantization_amd import _hip
    return _hip.load()


class _Tensor:
    """One descriptor's inputs in a fresh arena: P, s, dy as inputs, then whatever the call needs."""

    def __init__(self, lib, desc, mis, with_dy=True):
        self.lib, self.desc, self.mis = lib, desc, mis
        outer, G, inner = desc
        self.n, self.G = outer * G * inner, G
        self.P, self.dy, self.s = C.draw(outer, G, inner)
        self.res = 4 if mis else 0
        self.row = C.dense_row_bytes(outer, G, inner)
        self.a = C.new_arena()
        self.a.add("P", "in", data=self.P, residue=self.res, row_bytes=self.row)
        self.a.add("s", "in", data=self.s)
        if with_dy:
            self.a.add("dy", "in", data=self.dy, residue=self.res, row_bytes=self.row)

    def dense(self, name, itemsize=4, kind="out"):
        return self.a.add(name, kind, nbytes=self.n * itemsize, residue=self.res, row_bytes=self.row)

    def small(self, name, nbytes, kind="out", data=None):
        return self.a.add(name, kind, nbytes=None if data is not None else nbytes, data=data)

    def ws(self):
        nbytes = self.lib.lq_workspace_bytes(*self.desc)
        assert nbytes > 0
        self.ws_bytes = nbytes
        return self.a.add("ws", "ws", nbytes=nbytes)

    def p(self, name):
        return self.a.ptr(name)


# ------------------------------------------------------------------------------------------ nq
def _nq(lib, desc, mis, what):
    outer, G, inner = desc
    t = _Tensor(lib, desc, mis)
    n = t.n
    small = n < C.STREAMING
    t.dense("out")
    t.dense("q")
    if small:
        for name, size in (("out8", 4), ("q8", 1), ("out32", 4), ("q32", 4), ("qf_only", 4), ("q8_only", 1)):
            t.dense(name, size)
    for i in range(len(LAMS)):
        t.small(f"ds{i}", 4 * G)
        t.small(f"parts{i}", 12 * G)
    t.dense("out_fused")
    t.small("ds_fused", 4 * G)
    t.ws()
    a = t.a.build()
    q_ref, out_ref = C.forward_reference(t.P, t.s, *desc)
    from learned_quantization_amd import _hip

    def fwd(out, q, qd):
        return lambda: lib.lq_fq_forward(t.p("P"), t.p("s"), t.p(out) if out else None, t.p(q), qd, outer, G, inner, None)

    def v_fwd(out, q, dtype, ref):
        def verify(get, tag):
            if out:
                C.same_bits(get(out, np.float32), out_ref, f"{tag}: out")
            C.same_bits(get(q, dtype), ref, f"{tag}: q")
        return verify
    C.run_call(a, f"{what} lq_fq_forward out + float32 q", fwd("out", "q", _hip.LQ_Q_F32), ["out", "q"], v_fwd("out", "q", np.float32, q_ref))
    if small:
        q8_ref = O.export_int8(t.P.reshape(outer, G, inner), t.s.reshape(1, G, 1)).reshape(-1)
        q32_ref = q_ref.astype(np.int32)
        C.run_call(a, f"{what} lq_fq_forward out + int8 q", fwd("out8", "q8", _hip.LQ_Q_I8), ["out8", "q8"], v_fwd("out8", "q8", np.int8, q8_ref))
        C.run_call(a, f"{what} lq_fq_forward out + int32 q", fwd("out32", "q32", _hip.LQ_Q_I32), ["out32", "q32"],
                   v_fwd("out32", "q32", np.int32, q32_ref))
        C.run_call(a, f"{what} lq_fq_forward float32 q alone", fwd(None, "qf_only", _hip.LQ_Q_F32), ["qf_only"], v_fwd(None, "qf_only", np.float32, q_ref))
        C.run_call(a, f"{what} lq_fq_forward int8 q alone", fwd(None, "q8_only", _hip.LQ_Q_I8), ["q8_only"], v_fwd(None, "q8_only", np.int8, q8_ref))
    refs = [C.nq_reference(t.P, t.s, t.dy, lam, *desc, q32=q_ref) for lam in LAMS]
    if outer * inner >= 16:
        assert refs[1]["below"].min() > 0, "every group has votes at the larger threshold: its mean is a sum of terms"
    for i, lam in enumerate(LAMS):
        def call(i=i, lam=lam):
            return lib.lq_fq_scale_grad(t.p("P"), t.p("s"), t.p("dy"), lam, t.p(f"ds{i}"), t.p(f"parts{i}"), t.p("ws"), t.ws_bytes,
                                        outer, G, inner, None)

        def verify(get, tag, i=i):
            C.check_nq(get(f"ds{i}", np.float32), get(f"parts{i}", np.float32), refs[i], tag)
        C.run_call(a, f"{what} lq_fq_scale_grad lambda={lam:g}", call, [f"ds{i}", f"parts{i}"], verify, ws="ws")

    def fused():
        return lib.lq_fq_fwd_bwd_fused(t.p("P"), t.p("s"), t.p("dy"), LAMS[1], t.p("out_fused"), t.p("ds_fused"), t.p("ws"), t.ws_bytes,
                                       outer, G, inner, None)

    def v_fused(get, tag):
        C.same_bits(get("out_fused", np.float32), out_ref, f"{tag}: out")
        C.check_nq(get("ds_fused", np.float32), None, refs[1], tag)
    C.run_call(a, f"{what} lq_fq_fwd_bwd_fused", fused, ["out_fused", "ds_fused"], v_fused, ws="ws")


# ------------------------------------------------------------------------------------------ lsq
QMIN, QMAX, GRAD_SCALE = -8, 7, 0.37
ROUNDINGS = ((0, "floor", clip_reference), (1, "nearest", rne_reference))


def _lsq(lib, desc, mis, what):
    outer, G, inner = desc
    t = _Tensor(lib, desc, mis)
    t.small("ds_ste", 4 * G)
    for _, name, _ in ROUNDINGS:
        t.dense(f"out_{name}")
        t.dense(f"q_{name}")
        t.dense(f"dP_{name}")
        t.small(f"ds_{name}", 4 * G)
        t.small(f"clipped_{name}", 4 * G)
    t.dense("dP_mask")
    t.ws()
    a = t.a.build()
    from learned_quantization_amd import _hip
    P3, dy3, s3 = t.P.reshape(outer, G, inner), t.dy.reshape(outer, G, inner), t.s.reshape(1, G, 1)
    # the straight-through gradient is the clipped one with the widest range (include/lq_hip.h), up to the summation order
    ste = clip_reference(P3, s3, dy3, -(1 << 24), 1 << 24, GRAD_SCALE)
    assert ste["inside"].all()

    def call_ste():
        return lib.lq_fq_scale_grad_ste(t.p("P"), t.p("s"), t.p("dy"), GRAD_SCALE, t.p("ds_ste"), t.p("ws"), t.ws_bytes, outer, G, inner, None)
    C.run_call(a, f"{what} lq_fq_scale_grad_ste", call_ste, ["ds_ste"],
               lambda get, tag: assert_within_terms(get("ds_ste", np.float32), ste["ds"], ste["terms"], f"{tag}: ds"), ws="ws")
    del ste
    for rnd, name, reference in ROUNDINGS:
        ref = reference(P3, s3, dy3, QMIN, QMAX, GRAD_SCALE)
        n_out = int((~ref["inside"]).sum())
        assert 0 < n_out < t.n or t.n < 16, "the inputs clip somewhere and pass somewhere"

        def call_fwd(rnd=rnd, name=name):
            return lib.lq_fq_forward_clip_r(t.p("P"), t.p("s"), t.p(f"out_{name}"), t.p(f"q_{name}"), _hip.LQ_Q_I32, QMIN, QMAX, rnd,
                                            outer, G, inner, None)

        def v_fwd(get, tag, name=name, ref=ref):
            C.same_bits(get(f"out_{name}", np.float32), ref["out"], f"{tag}: out")
            C.same_bits(get(f"q_{name}", np.int32), ref["q"].astype(np.int32), f"{tag}: q")
        C.run_call(a, f"{what} lq_fq_forward_clip_r {name}", call_fwd, [f"out_{name}", f"q_{name}"], v_fwd)

        def call_bwd(rnd=rnd, name=name):
            return lib.lq_fq_backward_clip_r(t.p("P"), t.p("s"), t.p("dy"), QMIN, QMAX, rnd, GRAD_SCALE, t.p(f"dP_{name}"), t.p(f"ds_{name}"),
                                             t.p(f"clipped_{name}"), t.p("ws"), t.ws_bytes, outer, G, inner, None)

        def v_bwd(get, tag, name=name, ref=ref):
            C.same_bits(get(f"dP_{name}", np.float32), ref["dP"], f"{tag}: dP")
            assert np.array_equal(get(f"clipped_{name}", np.uint32).astype(np.int64), ref["clipped"].reshape(-1)), f"{tag}: clip counts"
            assert_within_terms(get(f"ds_{name}", np.float32), ref["ds"], ref["terms"], f"{tag}: ds")
        C.run_call(a, f"{what} lq_fq_backward_clip_r {name}", call_bwd, [f"dP_{name}", f"ds_{name}", f"clipped_{name}"], v_bwd, ws="ws")
        if rnd == 0:
            def call_mask():
                return lib.lq_fq_backward_clip_r(t.p("P"), t.p("s"), t.p("dy"), QMIN, QMAX, 0, GRAD_SCALE, t.p("dP_mask"), None, None,
                                                 t.p("ws"), t.ws_bytes, outer, G, inner, None)
            C.run_call(a, f"{what} lq_fq_backward_clip_r mask only", call_mask, ["dP_mask"],
                       lambda get, tag, ref=ref: C.same_bits(get("dP_mask", np.float32), ref["dP"], f"{tag}: dP"), ws="ws")


# ------------------------------------------------------------------------------------------ penalty
C_DEV, C_SCALE = 0.6, 0.5


def _penalty(lib, desc, mis, what):
    outer, G, inner = desc
    t = _Tensor(lib, desc, mis, with_dy=False)
    n = t.n
    mbr = C.maxbin_reference(t.P, t.s, *desc)
    c32 = np.array([C_DEV], np.float32)
    c = float(c32[0]) * float(np.float32(C_SCALE))
    t.small("c_dev", 4, kind="in", data=c32)
    t.small("mb_in", 0, kind="in", data=mbr["mb"])
    t.small("ties_in", 0, kind="in", data=mbr["ties"].astype(np.uint32))
    for name, size in (("mb", 4 * G), ("ties", 4 * G), ("mb_term", 4), ("mb_ds", 4 * G), ("df_term", 4), ("df_ds", 4 * G), ("iv_term", 4),
                       ("iv_ds", 4 * G)):
        t.small(name, size)
    t.dense("mb_dP")
    t.dense("df_dP")
    t.ws()
    a = t.a.build()
    P3, s3 = t.P.reshape(outer, G, inner), t.s.reshape(1, G, 1)

    def v_mb_fwd(get, tag):
        C.same_bits(get("mb", np.float32), mbr["mb"], f"{tag}: mb")
        assert np.array_equal(get("ties", np.uint32).astype(np.int64), mbr["ties"]), f"{tag}: ties"
        assert_within_terms(get("mb_term", np.float32), mbr["term64"], abs(mbr["term64"]), f"{tag}: term")
    C.run_call(a, f"{what} lq_penalty_maxbin_fwd",
               lambda: lib.lq_penalty_maxbin_fwd(t.p("P"), t.p("s"), t.p("mb"), t.p("ties"), t.p("mb_term"), t.p("ws"), t.ws_bytes, outer, G, inner, None),
               ["mb", "ties", "mb_term"], v_mb_fwd, ws="ws")

    # dP: WHICH elements tie is the float32 decision of the reference, so it is held to the float32 oracle as tests/test_gpu_fuzz.py
    # holds it; ds = -c * mb / (G * s) has one term per group
    dp32, _ = O.maxbin_term_grads(P3, s3, c)
    ds64 = -c * mbr["mb64"] / (G * t.s.astype(np.float64))

    def v_mb_bwd(get, tag):
        np.testing.assert_allclose(get("mb_dP", np.float32), dp32.reshape(-1), rtol=1e-5, atol=0, err_msg=f"{tag}: dP")
        assert_within_terms(get("mb_ds", np.float32), ds64, None, f"{tag}: ds")
    C.run_call(a, f"{what} lq_penalty_maxbin_bwd",
               lambda: lib.lq_penalty_maxbin_bwd(t.p("P"), t.p("s"), t.p("mb_in"), t.p("ties_in"), t.p("c_dev"), C_SCALE, t.p("mb_dP"), t.p("mb_ds"),
                                                 outer, G, inner, None),
               ["mb_dP", "mb_ds"], v_mb_bwd)
    del dp32

    term64 = O64.difference_term(t.P, t.s, *desc)
    C.run_call(a, f"{what} lq_penalty_difference_fwd",
               lambda: lib.lq_penalty_difference_fwd(t.p("P"), t.p("s"), t.p("df_term"), t.p("ws"), t.ws_bytes, outer, G, inner, None),
               ["df_term"], lambda get, tag: assert_within_terms(get("df_term", np.float32), term64, abs(term64), f"{tag}: term"), ws="ws")
    dp64, dds64, ds_abs, dp_abs = O64.difference_term_grads(t.P, t.s, c, *desc, with_dP_abs=True)

    def v_df_bwd(get, tag):
        assert_within_terms(get("df_dP", np.float32), dp64, dp_abs, f"{tag}: dP")
        assert_within_terms(get("df_ds", np.float32), dds64, ds_abs, f"{tag}: ds")
    C.run_call(a, f"{what} lq_penalty_difference_bwd",
               lambda: lib.lq_penalty_difference_bwd(t.p("P"), t.p("s"), t.p("c_dev"), C_SCALE, t.p("df_dP"), t.p("df_ds"), t.p("ws"), t.ws_bytes,
                                                     outer, G, inner, None),
               ["df_dP", "df_ds"], v_df_bwd, ws="ws")

    iv64 = O64.inverse_term(t.s)
    C.run_call(a, f"{what} lq_penalty_inverse_fwd", lambda: lib.lq_penalty_inverse_fwd(t.p("s"), t.p("iv_term"), G, None), ["iv_term"],
               lambda get, tag: assert_within_terms(get("iv_term", np.float32), iv64, abs(iv64), f"{tag}: term"))
    ids64, ids_abs = O64.inverse_term_grads(t.s, c)
    C.run_call(a, f"{what} lq_penalty_inverse_bwd", lambda: lib.lq_penalty_inverse_bwd(t.p("s"), t.p("c_dev"), C_SCALE, t.p("iv_ds"), G, None),
               ["iv_ds"], lambda get, tag: assert_within_terms(get("iv_ds", np.float32), ids64, ids_abs, f"{tag}: ds"))


FAMILIES = {"nq": _nq, "lsq": _lsq, "penalty": _penalty}


@pytest.mark.parametrize("desc,mis,family", CASES)
def test_family_keeps_the_memory_contract(lib, desc, mis, family):
    FAMILIES[family](lib, desc, mis, f"{desc}{' misaligned' if mis else ''}")


# ------------------------------------------------------------------------------------------ the negative control
@pytest.mark.parametrize("shape,orient", [((3, 4100), "rowwise"), ((100003,), "scalar")])
def test_store_past_a_short_out_region_is_seen(lib, shape, orient):
    """`out` is declared ONE element shorter than the descriptor: the forward's store of the last element is a stray write from a
    real kernel -- into the guard, inside the arena's allocation, an ordinary in-bounds store -- and the arena must report exactly
    those 4 bytes."""
    from learned_quantization_amd import _hip
    outer, G, inner = desc = C.descriptor(shape, orient)
    P, _, s = C.draw(*desc)
    _, out_ref = C.forward_reference(P, s, *desc)
    assert SENTINEL_BYTE not in out_ref[-1:].tobytes(), "a byte equal to the sentinel's would hide in the guard"
    n = outer * G * inner
    a = C.new_arena()
    a.add("P", "in", data=P, row_bytes=4 * inner)
    a.add("s", "in", data=s)
    a.add("out", "out", nbytes=4 * (n - 1), row_bytes=4 * inner)
    a.build()
    _hip.check(lib.lq_fq_forward(a.ptr("P"), a.ptr("s"), a.ptr("out"), None, 0, outer, G, inner, None), "lq_fq_forward")
    torch.cuda.synchronize()
    assert a.violations() == [dict(region="out", where="after", first=0, last=3, count=4)]
    with pytest.raises(AssertionError, match="out: after, 4 bytes, offsets 0..3"):
        a.check("short out")
    C.same_bits(a.numpy("out", np.float32), out_ref[:-1], "the elements inside the region")


# ------------------------------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("n", [12289, 100003])
@pytest.mark.parametrize("nbits", [1, 3, 5, 8, 13, 32])
def test_pack_and_unpack_keep_the_memory_contract(lib, nbits, n):
    """`words` has exactly ceil(n * bits / 32) elements and, below 32 bits, n * bits is a multiple of neither 32 nor 128: the last
    word is partial.  Codes span the whole range of `bits` bits (32: 2^20 integers)."""
    from test_gpu_pack import np_pack_fast
    assert (n * nbits) % 32 != 0 or nbits == 32
    rng = np.random.default_rng(stable_seed("pack", nbits, n))
    G = 1
    s = np.array([2.0 ** -6], np.float32)                               # a power of two: (q + 1/2) * s divides back exactly
    span = min(1 << nbits, 1 << 20)
    qmin = -(span // 2) - 3
    codes = rng.integers(0, span, size=n)
    codes[:2] = (0, span - 1)
    q_ref = (codes + qmin).astype(np.int32)
    P = ((q_ref.astype(np.float64) + rng.uniform(0.1, 0.9, size=n)) * float(s[0])).astype(np.float32)   # ulp(2^19) is 1/32
    qf, out_ref = C.forward_reference(P, s, 1, 1, n)
    assert np.array_equal(qf.astype(np.int32), q_ref)
    words_ref = np_pack_fast(codes, nbits)
    nw = (n * nbits + 31) // 32
    assert words_ref.size == nw
    a = C.new_arena()
    a.add("P", "in", data=P, row_bytes=4 * n)
    a.add("s", "in", data=s)
    a.add("words", "out", nbytes=4 * nw)
    a.add("bad", "inout", data=np.zeros(1, np.uint64))
    a.add("words_in", "in", data=words_ref)
    for name in ("out", "q", "restore", "out3", "q3", "restore3"):
        a.add(name, "out", nbytes=4 * n, row_bytes=4 * n)
    a.build()
    zero = {"bad": np.zeros(1, np.uint64)}

    def v_pack(get, tag):
        C.same_bits(get("words", np.uint32), words_ref, f"{tag}: words")
        assert int(get("bad", np.uint64)[0]) == 0, f"{tag}: rejected elements"
    C.run_call(a, f"lq_q_pack bits={nbits} n={n}",
               lambda: lib.lq_q_pack(a.ptr("P"), a.ptr("s"), qmin, nbits, a.ptr("words"), a.ptr("bad"), 1, G, n, None), ["words"], v_pack,
               reupload=zero)
    restore_ref = ((q_ref.astype(np.float32) + np.float32(0.5)) * s[0]).astype(np.float32)
    out_pos = np.where(out_ref == 0, np.float32(0.0), out_ref)          # a -0 comes back as +0 (include/lq_hip.h)

    def unpack(out, q, pr):
        return lambda: lib.lq_q_unpack(a.ptr("words_in"), qmin, nbits, a.ptr("s"), a.ptr(out) if out else None, a.ptr(q) if q else None,
                                       a.ptr(pr) if pr else None, a.ptr("bad"), 1, G, n, None)

    def v_unpack(out, q, pr):
        def verify(get, tag):
            if out:
                C.same_bits(get(out, np.float32), out_pos, f"{tag}: out")
            if q:
                C.same_bits(get(q, np.int32), q_ref, f"{tag}: q")
            if pr:
                C.same_bits(get(pr, np.float32), restore_ref, f"{tag}: p_restore")
            assert int(get("bad", np.uint64)[0]) == 0, f"{tag}: restore misses"
        return verify
    for out, q, pr in (("out", None, None), (None, "q", None), (None, None, "restore"), ("out3", "q3", "restore3")):
        C.run_call(a, f"lq_q_unpack bits={nbits} n={n} {out} {q} {pr}", unpack(out, q, pr), [x for x in (out, q, pr) if x], v_unpack(out, q, pr),
                   reupload=zero)


# ------------------------------------------------------------------------------------------ conv kernels: HWIO parameter, OIHW consumer
@pytest.mark.parametrize("shape,orient", [((3, 3, 64, 128), "channelwise"), ((1, 1, 64, 128), "rowwise"), ((7, 7, 3, 64), "channelwise")])
def test_oihw_pair_keeps_the_memory_contract(lib, shape, orient):
    """LDS tiles (the first two) and the element-wise companion form ((7, 7, 3, 64): 49 taps).  Reference: the plain ops'
    oracle results, permuted."""
    kh, kw, ci, co = shape
    hw = kh * kw
    outer, G, inner = desc = C.descriptor(shape, orient)
    n = hw * ci * co
    P, dy, s = C.draw(*desc)
    tile = lib.lq_conv_tile_supported(hw, ci, co, outer, G, inner) == 1
    assert tile == (hw <= 9)
    q_ref, out_ref = C.forward_reference(P, s, *desc)

    def to_oihw(x):
        return np.ascontiguousarray(x.reshape(hw, ci, co).transpose(2, 1, 0)).reshape(-1)
    ws_bytes = lib.lq_conv_workspace_bytes(hw, ci, co, outer, G, inner)
    a = C.new_arena()
    row = C.dense_row_bytes(*desc)
    a.add("P", "in", data=P, row_bytes=row)
    a.add("s", "in", data=s)
    a.add("dy_oihw", "in", data=to_oihw(dy), row_bytes=4 * hw * ci)
    for name in ("out", "out_oihw", "only_oihw", "dP"):
        a.add(name, "out", nbytes=4 * n, row_bytes=row)
    for i in range(len(LAMS)):
        a.add(f"ds{i}", "out", nbytes=4 * G)
    a.add("ws", "ws", nbytes=ws_bytes)
    a.build()

    def v_fwd(get, tag):
        C.same_bits(get("out", np.float32), out_ref, f"{tag}: out")
        C.same_bits(get("out_oihw", np.float32), to_oihw(out_ref), f"{tag}: out_oihw")
    C.run_call(a, f"{shape} lq_fq_forward_oihw",
               lambda: lib.lq_fq_forward_oihw(a.ptr("P"), a.ptr("s"), a.ptr("out"), a.ptr("out_oihw"), hw, ci, co, outer, G, inner, None),
               ["out", "out_oihw"], v_fwd)
    if tile:
        C.run_call(a, f"{shape} lq_fq_forward_oihw without out",
                   lambda: lib.lq_fq_forward_oihw(a.ptr("P"), a.ptr("s"), None, a.ptr("only_oihw"), hw, ci, co, outer, G, inner, None),
                   ["only_oihw"], lambda get, tag: C.same_bits(get("only_oihw", np.float32), to_oihw(out_ref), f"{tag}: out_oihw"))
    for i, lam in enumerate(LAMS):
        ref = C.nq_reference(P, s, dy, lam, *desc, q32=q_ref)

        def verify(get, tag, i=i, ref=ref):
            C.same_bits(get("dP", np.float32), dy, f"{tag}: dP is dy in HWIO order")
            C.check_nq(get(f"ds{i}", np.float32), None, ref, tag)
        C.run_call(a, f"{shape} lq_fq_scale_grad_oihw lambda={lam:g}",
                   lambda i=i, lam=lam: lib.lq_fq_scale_grad_oihw(a.ptr("P"), a.ptr("s"), a.ptr("dy_oihw"), lam, a.ptr(f"ds{i}"), a.ptr("dP"),
                                                                 a.ptr("ws"), ws_bytes, hw, ci, co, outer, G, inner, None),
                   [f"ds{i}", "dP"], verify, ws="ws")


# ------------------------------------------------------------------------------------------ integer-view statistics
@pytest.mark.parametrize("shape,orient,axis", [((3, 3, 64, 128), "channelwise", 1), ((3, 3, 64, 128), "channelwise", 3), ((100003,), "scalar", 0)])
def test_statistics_keep_the_memory_contract(lib, shape, orient, axis):
    """lq_q_absmax_over_axis, lq_q_minmax, lq_q_histogram.  The histogram window is narrower than the integer range and sits inside
    a longer array of bins: bins on both sides of the counted window must stay as they were."""
    outer, G, inner = desc = C.descriptor(shape, orient)
    P, _, s = C.draw(*desc)
    q_ref, _ = C.forward_reference(P, s, *desc)
    qi = q_ref.astype(np.int64)
    n = qi.size
    pre, n_axis, post = int(np.prod(shape[:axis], dtype=np.int64)), shape[axis], int(np.prod(shape[axis + 1:], dtype=np.int64))
    absmax_ref = np.abs(q_ref).reshape(pre, n_axis, post).max(axis=1).reshape(-1)
    lo, hi = int(qi.min()), int(qi.max())
    win_lo, nbins, pad = lo + (hi - lo) // 4, (hi - lo) // 2, 7
    assert lo < win_lo and win_lo + nbins - 1 < hi and nbins > 0, "integers on both sides of the counted window"
    before = np.arange(1, nbins + 2 * pad + 1, dtype=np.uint32)          # bins that already hold counts: the call ADDS
    inside = (qi >= win_lo) & (qi < win_lo + nbins)
    bins_ref = before.copy()
    bins_ref[pad:pad + nbins] += np.bincount(qi[inside] - win_lo, minlength=nbins).astype(np.uint32)
    a = C.new_arena()
    a.add("P", "in", data=P, row_bytes=C.dense_row_bytes(*desc))
    a.add("s", "in", data=s)
    a.add("absmax", "out", nbytes=4 * pre * post)
    a.add("minmax", "inout", data=np.array([2 ** 31 - 1, -2 ** 31], np.int32))
    a.add("bins", "inout", data=before)
    a.build()
    C.run_call(a, f"{shape} lq_q_absmax_over_axis axis={axis}",
               lambda: lib.lq_q_absmax_over_axis(a.ptr("P"), a.ptr("s"), a.ptr("absmax"), pre, n_axis, post, outer, G, inner, None),
               ["absmax"], lambda get, tag: C.same_bits(get("absmax", np.float32), absmax_ref, f"{tag}: max|q|"))
    C.run_call(a, f"{shape} lq_q_minmax", lambda: lib.lq_q_minmax(a.ptr("P"), a.ptr("s"), a.ptr("minmax"), outer, G, inner, None), [],
               lambda get, tag: None)
    assert a.numpy("minmax", np.int32).tolist() == [lo, hi]
    C.run_call(a, f"{shape} lq_q_histogram",
               lambda: lib.lq_q_histogram(a.ptr("P"), a.ptr("s"), win_lo, nbins, a.ptr("bins") + 4 * pad, outer, G, inner, None), [],
               lambda get, tag: None)
    C.same_bits(a.numpy("bins", np.uint32), bins_ref, f"{shape}: bins (window of {nbins} inside {before.size})")
    assert int(inside.sum()) not in (0, n)


# ------------------------------------------------------------------------------------------ scale update
LR, B1, B2, EPS, STEP, MIN_VALUE = 1e-3, 0.9, 0.999, 1e-7, 3, 2e-3


@pytest.mark.parametrize("n", [1, 7, 1000, 65537])
def test_scale_update_keeps_the_memory_contract(lib, n):
    """lq_scale_adam_step, lq_scale_adam_step_dev (both modes) and lq_min_value_project on vectors of 1 .. 65537 elements (one
    partly filled block at either end of the range), against the float64 restatement of the header's formula under the bound
    tests/test_gpu_layers.py holds the scale update to (rtol 2e-6)."""
    rng = np.random.default_rng(stable_seed("adam", n))
    s0 = rng.uniform(1e-3, 3e-2, size=n).astype(np.float32)
    g = (rng.normal(0, 1, size=n) * 10.0 ** rng.integers(-6, 1, size=n)).astype(np.float32)
    m0 = (g * rng.uniform(0.5, 1.5, size=n)).astype(np.float32)
    v0 = (g * g * rng.uniform(0.5, 1.5, size=n)).astype(np.float32)
    a = C.new_arena()
    a.add("ds", "in", data=g)
    a.add("step", "in", data=np.array([STEP], np.int64))
    for name, data in (("s", s0), ("m", m0), ("v", v0), ("w", s0)):
        a.add(name, "inout", data=data)
    a.build()
    state = {"s": s0, "m": m0, "v": v0}
    for mode in (0, 1):
        ref = dict(zip("smv", C.adam64(s0, g, m0, v0, mode, LR, B1, B2, EPS, STEP, MIN_VALUE)))

        def verify(get, tag, ref=ref):
            for k in "smv":
                np.testing.assert_allclose(get(k, np.float32), ref[k], rtol=2e-6, atol=0, err_msg=f"{tag}: {k}")
            assert get("s", np.float32).min() >= np.float32(MIN_VALUE)
        C.run_call(a, f"lq_scale_adam_step n={n} mode={mode}",
                   lambda mode=mode: lib.lq_scale_adam_step(a.ptr("s"), a.ptr("ds"), a.ptr("m"), a.ptr("v"), n, LR, B1, B2, EPS, STEP, MIN_VALUE,
                                                            mode, None), [], verify, reupload=state)
        host = a.numpy("s", np.float32).copy()
        C.run_call(a, f"lq_scale_adam_step_dev n={n} mode={mode}",
                   lambda mode=mode: lib.lq_scale_adam_step_dev(a.ptr("s"), a.ptr("ds"), a.ptr("m"), a.ptr("v"), n, LR, B1, B2, EPS, a.ptr("step"),
                                                                MIN_VALUE, mode, None), [], verify, reupload=state)
        C.same_bits(a.numpy("s", np.float32), host, "the device-side step counter gives the host call's bits")
    floor = float(np.median(s0))
    C.run_call(a, f"lq_min_value_project n={n}", lambda: lib.lq_min_value_project(a.ptr("w"), n, floor, None), [],
               lambda get, tag: C.same_bits(get("w", np.float32), np.maximum(s0, np.float32(floor)), f"{tag}: w"), reupload={"w": s0})
