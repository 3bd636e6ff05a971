"""Memory contract of the multi-tensor batch (include/lq_hip.h: lq_batch_*), on the raw-ABI pattern of
tests/test_gpu_clip_batch.py::_AbiBatch.  ONE poisoned arena (tests/_arena.py) holds ten tensors back to back, each with its own
P, s, dy, out, ds, dp, m, v and gradient buffer, chosen to mix the batch's forms; the guards between the tensors are what catches a
block that writes into its neighbour's buffers.  The workspace has exactly lq_batch_workspace_bytes (queried again after
lq_batch_set_clip, as the header requires) and sits in a poisoned arena of its own, because its size is known only once the batch
exists; every call that takes it runs with both prefills of tests/_contract.py and must give the same bits.

References: the single-tensor references per tensor (tests/_contract.py, tests/_clip_reference.py, tests/_rne_reference.py,
oracle/lq_oracle_f64.py).  Where the header states bit-identity it is asserted -- out against the reference; ds at lambda = 1e-10
against lq_fq_scale_grad; lq_batch_scale_grad_step against the two calls; lq_batch_penalty_grads_values against
lq_batch_penalty_grads; the clipped pair's out, dP and counts --, tests/_bounds.py elsewhere."""
import ctypes

import numpy as np
import pytest
import torch

import _contract as C
from _bounds import assert_within_terms, stable_seed
from _clip_reference import clip_reference
from _rne_reference import rne_reference
from oracle import lq_oracle as O
from oracle import lq_oracle_f64 as O64

pytestmark = pytest.mark.gpu

DESCS = [(1, 1, 10),          # a bias
         (1, 5, 4100),        # float4 row stream
         (133, 10, 1),        # scalar column form
         (784, 128, 1),       # column
         (1, 128, 784),       # row
         (576, 128, 1),       # the kernel (3, 3, 64, 128) reshaped, column
         (27, 32, 1),         # (3, 3, 3, 32)
         (1, 1, 100003),      # one long ragged row
         (1, 2048, 1000),     # tile and fragment forms
         (2048, 1000, 1)]
N = len(DESCS)
LAM = 1e-10
LR, B1, B2, EPS, STEP, MIN_VALUE = 1e-3, 0.9, 0.999, 1e-7, 3, 2e-3
RANGES = [(-8, 7), (0, 15), (-3, 5), (-2, 1), (0, 1)]      # narrow: |P / s| reaches a few dozen in every tensor
GRAD_SCALES = [0.37, 1.0, 2.0, 0.5, 1.5, 0.25, 3.0, 0.125, 0.75, 1.25]
COEFFS = [0.3, 0.7, 1.3, 0.11, 0.9, 0.45, 2.0, 0.05, 0.6, 0.8]


class _Batch:
    def __init__(self):
        from learned_quantization_amd import _hip
        self.hip = _hip
        self.lib = _hip.load()
        self.a = a = C.new_arena()
        self.P, self.dy, self.s, self.m0, self.v0, self.ds0 = [], [], [], [], [], []
        for i, (outer, G, inner) in enumerate(DESCS):
            P, dy, s = C.draw.__wrapped__(outer, G, inner, f"batch {i}")
            rng = np.random.default_rng(stable_seed("batch state", i))
            g = (rng.normal(0, 1, size=G) * 10.0 ** rng.integers(-6, 1, size=G)).astype(np.float32)
            self.P.append(P), self.dy.append(dy), self.s.append(s), self.ds0.append(g)
            self.m0.append((g * rng.uniform(0.5, 1.5, size=G)).astype(np.float32))
            self.v0.append((g * g * rng.uniform(0.5, 1.5, size=G)).astype(np.float32))
            row = C.dense_row_bytes(outer, G, inner)
            n = outer * G * inner
            a.add(f"P{i}", "in", data=P, row_bytes=row)
            a.add(f"s{i}", "inout", data=s)
            a.add(f"dy{i}", "in", data=dy, row_bytes=row)
            a.add(f"out{i}", "out", nbytes=4 * n, row_bytes=row)
            a.add(f"ds{i}", "out", nbytes=4 * G)
            a.add(f"dp{i}", "out", nbytes=4 * n, row_bytes=row)
            a.add(f"m{i}", "inout", data=self.m0[i])
            a.add(f"v{i}", "inout", data=self.v0[i])
            a.add(f"grad{i}", "inout", data=dy, row_bytes=row)       # the parameter's gradient so far: the penalty's dP is ADDED
            a.add(f"ds1_{i}", "out", nbytes=4 * G)                    # the single-tensor call's ds, for the bit-identity statements
        a.add("terms", "out", nbytes=4 * N)
        a.add("penalty", "out", nbytes=4)
        self.ws1_bytes = max(self.lib.lq_workspace_bytes(*d) for d in DESCS)
        a.add("ws1", "ws", nbytes=self.ws1_bytes)
        a.build()
        arr = (_hip.TensorDesc * N)()
        for i, (outer, G, inner) in enumerate(DESCS):
            arr[i] = _hip.TensorDesc(a.ptr(f"P{i}"), a.ptr(f"s{i}"), a.ptr(f"dy{i}"), a.ptr(f"out{i}"), a.ptr(f"ds{i}"), a.ptr(f"m{i}"),
                                     a.ptr(f"v{i}"), outer, G, inner, LAM, MIN_VALUE, None, a.ptr(f"dp{i}"), 0, 0, 0)
        self.handle = ctypes.c_void_p()
        _hip.check(self.lib.lq_batch_create(arr, N, ctypes.byref(self.handle)), "lq_batch_create")
        self.state = {}
        for i in range(N):
            self.state.update({f"s{i}": self.s[i], f"m{i}": self.m0[i], f"v{i}": self.v0[i], f"grad{i}": self.dy[i]})
        self.new_workspace()
        self.fwd = [C.forward_reference(self.P[i], self.s[i], *DESCS[i]) for i in range(N)]

    def new_workspace(self):
        """A workspace arena of exactly lq_batch_workspace_bytes as the batch states it NOW."""
        self.ws_bytes = self.lib.lq_batch_workspace_bytes(self.handle)
        assert self.ws_bytes > 0
        self.wa = C.new_arena()
        self.wa.add("ws", "ws", nbytes=self.ws_bytes)
        self.wa.build()

    def ws(self):
        return self.wa.ptr("ws")

    def ptrs(self, prefix):
        return (ctypes.c_void_p * N)(*[self.a.ptr(f"{prefix}{i}") for i in range(N)])

    def run(self, what, call, outs, verify, ws=True, reupload=None):
        """Every call starts from the uploaded s, m, v and gradient buffers; ``verify`` also sees them."""
        state = dict(self.state)
        state.update(reupload or {})
        C.run_call(self.a, what, call, outs, verify, ws="ws" if ws else None, reupload=state, ws_arena=self.wa if ws else None)

    def unchanged(self, get, tag, names=("s", "m", "v", "grad")):
        for k in names:
            for i in range(N):
                C.same_bits(get(f"{k}{i}", np.float32), self.state[f"{k}{i}"], f"{tag}: {k} of tensor {i} must not change")

    def close(self):
        self.lib.lq_batch_destroy(self.handle)


@pytest.fixture(scope="module")
def batch():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    b = _Batch()
    yield b
    b.close()


def _all(prefix):
    return [f"{prefix}{i}" for i in range(N)]


def test_batch_forward(batch):
    b = batch

    def verify(get, tag):
        for i in range(N):
            C.same_bits(get(f"out{i}", np.float32), b.fwd[i][1], f"{tag}: out of tensor {i} {DESCS[i]}")
        b.unchanged(get, tag)
    b.run("lq_batch_forward", lambda: b.lib.lq_batch_forward(b.handle, None), _all("out"), verify, ws=False)


def test_batch_scale_grad_and_the_fused_step(batch):
    """lq_batch_scale_grad at lambda = 1e-10: ds within the bound of the float64 reference and bit-identical to lq_fq_scale_grad
    (every vote sum is exact below 4e-4).  Then lq_batch_scale_adam on those ds, and lq_batch_scale_grad_step: the same ds, s, m
    and v, bit for bit, as the two calls one after the other."""
    b, lib, a = batch, batch.lib, batch.a
    refs = [C.nq_reference(b.P[i], b.s[i], b.dy[i], LAM, *DESCS[i], q32=b.fwd[i][0]) for i in range(N)]
    single = {}
    for i, (outer, G, inner) in enumerate(DESCS):
        def call(i=i, outer=outer, G=G, inner=inner):
            return lib.lq_fq_scale_grad(a.ptr(f"P{i}"), a.ptr(f"s{i}"), a.ptr(f"dy{i}"), LAM, a.ptr(f"ds1_{i}"), None, a.ptr("ws1"),
                                        lib.lq_workspace_bytes(outer, G, inner), outer, G, inner, None)

        def keep(get, tag, i=i):
            single[i] = get(f"ds1_{i}", np.float32).copy()
            C.check_nq(single[i], None, refs[i], tag)
        C.run_call(a, f"lq_fq_scale_grad of tensor {i} {DESCS[i]}", call, [f"ds1_{i}"], keep, ws="ws1")
    got = {}

    def v_grad(get, tag):
        for i in range(N):
            got[i] = get(f"ds{i}", np.float32).copy()
            C.check_nq(got[i], None, refs[i], f"{tag}: tensor {i} {DESCS[i]}")
            C.same_bits(got[i], single[i], f"{tag}: ds of tensor {i} {DESCS[i]} against lq_fq_scale_grad")
        b.unchanged(get, tag)
    b.run("lq_batch_scale_grad", lambda: lib.lq_batch_scale_grad(b.handle, None, b.ws(), b.ws_bytes, None), _all("ds"), v_grad)
    # the Adam launch on exactly those gradients
    two = {}

    def v_adam(get, tag):
        for i in range(N):
            ref = C.adam64(b.s[i], got[i], b.m0[i], b.v0[i], 0, LR, B1, B2, EPS, STEP, MIN_VALUE)
            for k, r in zip("smv", ref):
                two[k, i] = get(f"{k}{i}", np.float32).copy()
                np.testing.assert_allclose(two[k, i], r, rtol=2e-6, atol=0, err_msg=f"{tag}: {k} of tensor {i}")
            C.same_bits(get(f"ds{i}", np.float32), got[i], f"{tag}: ds of tensor {i} is read, not written")
        b.unchanged(get, tag, ("grad",))
    b.run("lq_batch_scale_adam", lambda: lib.lq_batch_scale_adam(b.handle, LR, B1, B2, EPS, STEP, None, 0, None), _all("ds"), v_adam, ws=False,
          reupload={f"ds{i}": got[i] for i in range(N)})

    def v_step(get, tag):
        for i in range(N):
            C.same_bits(get(f"ds{i}", np.float32), got[i], f"{tag}: ds of tensor {i}")
            for k in "smv":
                C.same_bits(get(f"{k}{i}", np.float32), two[k, i], f"{tag}: {k} of tensor {i} against the two calls")
        b.unchanged(get, tag, ("grad",))
    b.run("lq_batch_scale_grad_step", lambda: lib.lq_batch_scale_grad_step(b.handle, None, 0, b.ws(), b.ws_bytes, LR, B1, B2, EPS, STEP, None, 0, None),
          _all("ds"), v_step)


def test_batch_scale_grad_ste(batch):
    b, lib = batch, batch.lib
    refs = []
    for i, (outer, G, inner) in enumerate(DESCS):
        refs.append(clip_reference(b.P[i].reshape(outer, G, inner), b.s[i].reshape(1, G, 1), b.dy[i].reshape(outer, G, inner), -(1 << 24), 1 << 24,
                                   GRAD_SCALES[i]))
        assert refs[-1]["inside"].all()
    gs = (ctypes.c_float * N)(*GRAD_SCALES)
    dys = b.ptrs("dy")

    def verify(get, tag):
        for i in range(N):
            assert_within_terms(get(f"ds{i}", np.float32), refs[i]["ds"], refs[i]["terms"], f"{tag}: ds of tensor {i} {DESCS[i]}")
        b.unchanged(get, tag)
    b.run("lq_batch_scale_grad_ste", lambda: lib.lq_batch_scale_grad_ste(b.handle, dys, gs, b.ws(), b.ws_bytes, None), _all("ds"), verify)


def _penalty_reference(b, kind, i):
    """(dP reference, dP terms, ds reference, ds terms, term value) of tensor i for the coefficient COEFFS[i]."""
    outer, G, inner = DESCS[i]
    c = float(np.float32(COEFFS[i]))
    P, s = b.P[i], b.s[i]
    if kind == 0:
        mbr = C.maxbin_reference(P, s, outer, G, inner)
        dp32, _ = O.maxbin_term_grads(P.reshape(outer, G, inner), s.reshape(1, G, 1), c)      # the tie split is a float32 decision
        ds64 = -c * mbr["mb64"] / (G * s.astype(np.float64))
        return dp32.reshape(-1).astype(np.float64), np.abs(dp32.reshape(-1)).astype(np.float64), ds64, np.abs(ds64), mbr["term64"]
    if kind == 1:
        dp64, ds64, ds_abs, dp_abs = O64.difference_term_grads(P, s, c, outer, G, inner, with_dP_abs=True)
        return dp64, dp_abs, ds64, ds_abs, O64.difference_term(P, s, outer, G, inner)
    ds64, ds_abs = O64.inverse_term_grads(s, c)
    return None, None, ds64, ds_abs, O64.inverse_term(s)


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["maxbin", "difference", "inverse"])
def test_batch_penalty_grads_and_values(batch, kind):
    """lq_batch_penalty_grads (ds written, then added with LQ_PENALTY_ACCUMULATE_DS; dP added to the gradient buffers) and
    lq_batch_penalty_grads_values: the same gradient bits, the per-tensor terms and the model penalty."""
    from learned_quantization_amd._hip import LQ_PENALTY_ACCUMULATE_DS
    b, lib = batch, batch.lib
    refs = [_penalty_reference(b, kind, i) for i in range(N)]
    coeff = (ctypes.c_float * N)(*COEFFS)
    grads = b.ptrs("grad")
    dims = [float(o * g * n) for o, g, n in DESCS]
    dims_c = (ctypes.c_float * N)(*dims)
    starts = (ctypes.c_uint8 * N)(*[1 - i % 2 for i in range(N)])              # kernel and bias of one layer are paired
    plain = {}

    def v_grads(accumulate, keep):
        def verify(get, tag):
            for i in range(N):
                dp, dp_abs, ds64, ds_abs, _ = refs[i]
                g0 = b.dy[i].astype(np.float64)
                got = get(f"grad{i}", np.float32)
                if dp is None:
                    C.same_bits(got, b.dy[i], f"{tag}: the gradient of tensor {i} is not touched")
                else:
                    assert_within_terms(got, g0 + dp, np.abs(g0) + dp_abs, f"{tag}: gradient of tensor {i} {DESCS[i]}")
                ds0 = b.ds0[i].astype(np.float64) if accumulate else 0.0
                assert_within_terms(get(f"ds{i}", np.float32), ds0 + ds64, np.abs(ds0) + ds_abs, f"{tag}: ds of tensor {i} {DESCS[i]}")
                if keep is not None:
                    keep[i] = (got.copy(), get(f"ds{i}", np.float32).copy())
            b.unchanged(get, tag, ("s", "m", "v"))
        return verify
    use_ws = kind != 2
    b.run(f"lq_batch_penalty_grads kind {kind}",
          lambda: lib.lq_batch_penalty_grads(b.handle, kind, coeff, grads, b.ws() if use_ws else None, b.ws_bytes if use_ws else 0, None),
          _all("ds"), v_grads(False, plain), ws=use_ws)
    b.run(f"lq_batch_penalty_grads kind {kind} | ACCUMULATE_DS",
          lambda: lib.lq_batch_penalty_grads(b.handle, kind | LQ_PENALTY_ACCUMULATE_DS, coeff, grads, b.ws() if use_ws else None,
                                             b.ws_bytes if use_ws else 0, None),
          _all("ds"), v_grads(True, None), ws=use_ws, reupload={f"ds{i}": b.ds0[i] for i in range(N)})
    terms64 = np.array([r[4] for r in refs])
    penalty64 = float((terms64 * np.array(dims)).sum() / sum(dims))

    def v_values(get, tag):
        v_grads(False, None)(get, tag)
        for i in range(N):
            C.same_bits(get(f"grad{i}", np.float32), plain[i][0], f"{tag}: gradient of tensor {i} against lq_batch_penalty_grads")
            C.same_bits(get(f"ds{i}", np.float32), plain[i][1], f"{tag}: ds of tensor {i} against lq_batch_penalty_grads")
        assert_within_terms(get("terms", np.float32), terms64, np.abs(terms64), f"{tag}: terms")
        assert_within_terms(get("penalty", np.float32), penalty64, abs(penalty64), f"{tag}: penalty")
    b.run(f"lq_batch_penalty_grads_values kind {kind}",
          lambda: lib.lq_batch_penalty_grads_values(b.handle, kind, coeff, grads, dims_c, starts, b.a.ptr("terms"), b.a.ptr("penalty"),
                                                    b.ws() if use_ws else None, b.ws_bytes if use_ws else 0, None),
          _all("ds") + ["terms", "penalty"], v_values, ws=use_ws)


@pytest.mark.parametrize("rounding", [0, 1], ids=["floor", "nearest"])
def test_batch_clipped_pair(batch, rounding):
    """lq_batch_set_clip, the workspace size queried again, then lq_batch_forward_clip and lq_batch_backward_clip with grad_scale
    given and NULL (mask only: ds is not written at all -- its regions must still hold the sentinel)."""
    from learned_quantization_amd.batch import _DeviceInts
    b, lib = batch, batch.lib
    reference = (clip_reference, rne_reference)[rounding]
    ranges = [RANGES[i % len(RANGES)] for i in range(N)]
    qmin, qmax = (ctypes.c_int32 * N)(*[r[0] for r in ranges]), (ctypes.c_int32 * N)(*[r[1] for r in ranges])
    b.hip.check(lib.lq_batch_set_clip(b.handle, qmin, qmax, N, rounding), "lq_batch_set_clip")
    before = b.ws_bytes
    b.new_workspace()
    assert b.ws_bytes >= before
    refs = []
    for i, (outer, G, inner) in enumerate(DESCS):
        refs.append(reference(b.P[i].reshape(outer, G, inner), b.s[i].reshape(1, G, 1), b.dy[i].reshape(outer, G, inner), *ranges[i], GRAD_SCALES[i]))
        n_out = int((~refs[-1]["inside"]).sum())
        assert 0 < n_out < refs[-1]["inside"].size or refs[-1]["inside"].size < 16, "the inputs clip somewhere and pass somewhere"

    def v_fwd(get, tag):
        for i in range(N):
            C.same_bits(get(f"out{i}", np.float32), refs[i]["out"], f"{tag}: out of tensor {i} {DESCS[i]}")
        b.unchanged(get, tag)
    b.run(f"lq_batch_forward_clip rounding {rounding}", lambda: lib.lq_batch_forward_clip(b.handle, None), _all("out"), v_fwd, ws=False)
    gs = (ctypes.c_float * N)(*GRAD_SCALES)
    dys = b.ptrs("dy")

    def counts(i):
        dv, groups = ctypes.c_void_p(), ctypes.c_int64()
        b.hip.check(lib.lq_batch_clip_counts(b.handle, i, ctypes.byref(dv), ctypes.byref(groups)), "lq_batch_clip_counts")
        assert groups.value == DESCS[i][1]
        return torch.as_tensor(_DeviceInts(dv.value, groups.value), device=b.a.device).cpu().numpy().view(np.uint32).astype(np.int64)

    def v_bwd(with_ds):
        def verify(get, tag):
            for i in range(N):
                C.same_bits(get(f"dp{i}", np.float32), refs[i]["dP"], f"{tag}: dP of tensor {i} {DESCS[i]}")
                assert np.array_equal(counts(i), refs[i]["clipped"].reshape(-1)), f"{tag}: clip counts of tensor {i} {DESCS[i]}"
                if with_ds:
                    assert_within_terms(get(f"ds{i}", np.float32), refs[i]["ds"], refs[i]["terms"], f"{tag}: ds of tensor {i} {DESCS[i]}")
            b.unchanged(get, tag)
        return verify
    b.run(f"lq_batch_backward_clip rounding {rounding}", lambda: lib.lq_batch_backward_clip(b.handle, dys, gs, b.ws(), b.ws_bytes, None),
          _all("dp") + _all("ds"), v_bwd(True))
    b.run(f"lq_batch_backward_clip rounding {rounding}, mask only", lambda: lib.lq_batch_backward_clip(b.handle, dys, None, b.ws(), b.ws_bytes, None),
          _all("dp"), v_bwd(False))
