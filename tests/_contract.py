"""Shared pieces of the memory-contract tests (tests/test_gpu_memory_contract.py, tests/test_gpu_memory_contract_batch.py):
the inputs, the references restated on (outer, G, inner) blocks, and the runner that holds one C-ABI call to tests/_arena.py.

References.  The header defines the integers by the float32 division (include/lq_hip.h: t = P / s, IEEE RN), so q and out are
NumPy float32 arithmetic, bit for bit (oracle/lq_oracle.py::fq_forward on a (outer, G, inner) view).  The vote of the nested-
quantization scale gradient is oracle/lq_oracle_f64.py::scale_grad restated with axis reductions instead of one boolean mask per
group (its loop is quadratic in practice: 4100 groups over 4.2 M elements) and taking q from the float32 division instead of a
float64 one -- at a random scale a float64 quotient can floor to the neighbouring integer, which moves max|q| by one; with
power-of-two scales the two agree exactly, and tests/test_contract_reference_cpu.py pins this restatement to the oracle there.
MaxBin's value and ds are restated the same way; the Difference terms call the float64 oracle, which is vectorised already."""
import functools

import numpy as np
import torch

from _arena import SENTINEL_BYTE, Arena
from _bounds import assert_within_terms, stable_seed
from oracle import lq_oracle as O
from oracle import lq_oracle_f64 as O64

POISONS = (SENTINEL_BYTE, 0xFF)        # the arena's own sentinel; NaN as float and double, UINT32_MAX as a count
STREAMING = 4 << 20                     # elements: from here the streaming forms of csrc/lq_stream2.hpp


def descriptor(shape, orient):
    return O.group_descriptor(shape, O.scale_shape(shape, orient))


@functools.lru_cache(maxsize=2)
def draw(outer, G, inner, tag="contract"):
    """(P, dy, s) flat float32, drawn as tests/test_gpu_parity.py::test_streaming_forms_parity draws them: finite,
    |P / s| < 2^22, dy spread over seven decades."""
    rng = np.random.default_rng(stable_seed(outer, G, inner, tag))
    n = outer * G * inner
    P = rng.normal(0, 0.05, size=n).astype(np.float32)
    dy = (rng.normal(0, 1, size=n) * 10.0 ** rng.uniform(-9, -2, size=n)).astype(np.float32)
    s = rng.uniform(1e-3, 3e-2, size=G).astype(np.float32)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(dy)) and np.abs(P).max() / s.min() < 2.0 ** 22
    for a in (P, dy, s):
        a.setflags(write=False)
    return P, dy, s


def forward_reference(P, s, outer, G, inner):
    """(q, out) float32, flat: NumPy's float32 division, floor and product."""
    q, out = O.fq_forward(P.reshape(outer, G, inner), s.reshape(1, G, 1))
    return q.reshape(-1), out.reshape(-1)


def nq_reference(P, s, dy, lam, outer, G, inner, q32=None):
    """dict(maxq float32[G]; mean, ds, mean_terms, ds_terms float64[G]; below, unsure int64[G]) of lq_fq_scale_grad (see the
    module docstring).  ``mean_terms`` is the sum of |terms| of the mean for tests/_bounds.py.  A vote -|tanh(lambda - r)| is a
    function of the DIFFERENCE of two float32 numbers, and |tanh'| <= 1: its terms are lambda and r, not |lambda - r| -- an
    element with r = 0.9999 lambda carries the rounding of r (2^-24 r from the product q * s and as much from the division)
    ten thousand times enlarged relative to its own vote.  With the inputs of tests/test_gpu_parity.py a group of a few
    thousand elements has a handful of votes at lambda = 1e-10, often one, so nothing averages this out (seen: 2.4e-4 of the
    group's only vote, r = 0.99993 lambda); tests/test_gpu_reverse_walk.py, whose groups hold 10^5 votes, can afford |mean|."""
    if q32 is None:
        q32, _ = forward_reference(P, s, outer, G, inner)
    q = q32.astype(np.float64).reshape(outer, G, inner)
    s64 = s.astype(np.float64).reshape(1, G, 1)
    pr = q * s64
    r = np.abs(dy.astype(np.float64).reshape(outer, G, inner)) / np.abs(np.where(pr == 0.0, O64.EPS_F32, pr))
    del pr
    lam64 = float(np.float32(lam))
    below = ~(r >= lam64)
    nb = below.sum(axis=(0, 2))
    votes = np.where(below, -np.abs(np.tanh(lam64 - r)), 0.0).sum(axis=(0, 2)) / float(outer * inner)
    mean = np.where(nb == 0, -abs(np.tanh(lam64)), votes)
    mean_terms = np.where(nb == 0, abs(np.tanh(lam64)), np.where(below, lam64 + r, 0.0).sum(axis=(0, 2)) / float(outer * inner))
    unsure = (np.abs(r - lam64) <= 2.0 ** -22 * lam64).sum(axis=(0, 2))
    maxq = np.abs(q).max(axis=(0, 2))
    return dict(maxq=maxq.astype(np.float32), mean=mean, ds=mean * maxq, below=nb, unsure=unsure, mean_terms=mean_terms,
                ds_terms=mean_terms * maxq)


def check_nq(got_ds, got_parts, ref, what):
    """ds (and, when given, `parts` = max|q|, mean, count): max|q| bit for bit, ds and the mean within tests/_bounds.py of the
    float64 reference with the terms of nq_reference, the vote count as tests/test_gpu_reverse_walk.py holds it.  A group in
    which no element votes but one sits within float32 rounding of lambda may go either way: it is left out."""
    ok = ~((ref["below"] == 0) & (ref["unsure"] > 0))
    assert_within_terms(np.asarray(got_ds)[ok], ref["ds"][ok], ref["ds_terms"][ok], f"{what}: ds")
    if got_parts is None:
        return
    parts = np.asarray(got_parts).reshape(3, -1)
    assert np.array_equal(parts[0].view(np.uint32), ref["maxq"].view(np.uint32)), f"{what}: max|q|"
    assert_within_terms(parts[1][ok], ref["mean"][ok], ref["mean_terms"][ok], f"{what}: mean")
    tol = ref["unsure"] + ref["below"] * 2.0 ** -24
    assert np.all(np.abs(parts[2].astype(np.float64) - ref["below"]) <= tol), f"{what}: vote count"


def maxbin_reference(P, s, outer, G, inner):
    """dict(mb float32[G] (the float32 quotients' maximum: division is monotone, so it is the kernel's, bit for bit), ties
    int64[G] (decided by the float32 quotients, as in the reference), term64 = mean_g max |P| / s in float64)."""
    t = np.abs(P).reshape(outer, G, inner) / s.reshape(1, G, 1)
    assert t.dtype == np.float32
    mb = t.max(axis=(0, 2))
    ties = (t == mb.reshape(1, G, 1)).sum(axis=(0, 2)).astype(np.int64)
    mb64 = np.abs(P).reshape(outer, G, inner).max(axis=(0, 2)).astype(np.float64) / s.astype(np.float64)
    return dict(mb=mb, ties=ties, term64=float(mb64.mean()), mb64=mb64)


def adam64(s, g, m, v, mode, lr, b1, b2, eps, step, min_value):
    """The header's formula in float64 (include/lq_hip.h, K6): the moments, then KERAS var -= lr * sqrt(1 - b2^t) / (1 - b1^t) * m /
    (sqrt(v) + eps), TORCH var -= lr * m_hat / (sqrt(v_hat) + eps); then max(var, min_value).  Returns (s, m, v)."""
    s, g, m, v = (np.asarray(x, np.float64) for x in (s, g, m, v))
    m = m + (g - m) * (1.0 - b1)
    v = v + (g * g - v) * (1.0 - b2)
    c1, c2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if mode == 0:
        s = s - lr * np.sqrt(c2) / c1 * m / (np.sqrt(v) + eps)
    else:
        s = s - lr * (m / c1) / (np.sqrt(v / c2) + eps)
    return np.maximum(s, float(np.float32(min_value))), m, v


# ------------------------------------------------------------------------------------------ one call, held to the arena
def dense_row_bytes(outer, G, inner):
    """The "row" of a dense region for the guards: inner * 4 of a row form (outer == 1), G * inner * 4 of a column form."""
    return 4 * inner * (G if outer > 1 else 1)


def run_call(arena, what, call, outs, verify, ws=None, reupload=None, ws_arena=None):
    """Runs ``call()`` (which enqueues on the default stream and returns the lq_status) and holds it to the arena: guards, inputs,
    every region of ``outs`` completely written, every other output region untouched.  With ``ws`` the call runs twice on the same
    inputs, the workspace prefilled with each of POISONS; ``verify(get, tag)`` -- get(name, dtype) returns that run's output as
    a NumPy array -- compares EACH run with the reference, and the two runs' outputs must be bit-identical.  ``reupload``:
    {name: array} of in-place regions restored before each run.  ``ws_arena``: the arena that holds ``ws`` when it is not ``arena``
    (the batch's workspace size is known only once the batch exists); it is checked as well."""
    from learned_quantization_amd import _hip
    runs = []
    for fill in (POISONS if ws else (None,)):
        tag = what if fill is None else f"{what} [ws prefilled with 0x{fill:02X}]"
        for name in arena.names():
            if arena.region(name).kind == "out":
                arena.fill(name, SENTINEL_BYTE)
        for name, data in (reupload or {}).items():
            arena.upload(name, data)
        if ws:
            (ws_arena or arena).fill(ws, fill)
        _hip.check(call(), tag)
        torch.cuda.synchronize()
        try:
            arena.check(tag, written=outs)
            if ws_arena is not None:
                ws_arena.check(tag + " (workspace arena)")
        except AssertionError:
            for damaged in (arena, ws_arena):                     # a shared arena: the calls after this one are judged on their own
                if damaged is not None:
                    damaged.repair()
            raise
        snap = {name: arena.bytes(name).clone() for name in list(outs) + list(reupload or {})}
        runs.append(snap)
        host = {}

        def get(name, dtype, snap=snap, host=host):
            if name not in host:
                host[name] = snap[name].cpu().numpy()
            return host[name].view(dtype)
        verify(get, tag)
    if ws:
        for name in runs[0]:
            assert torch.equal(runs[0][name], runs[1][name]), f"{what}: {name} differs between the two workspace prefills"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, f"{what}: {g.shape} vs {r.shape}"
    if not np.array_equal(g, r):
        bad = np.flatnonzero(g != r)
        raise AssertionError(f"{what}: {bad.size} of {g.size} elements differ, first at {int(bad[0])}: got "
                             f"{np.asarray(got).reshape(-1)[bad[0]]!r}, reference {np.asarray(ref).reshape(-1)[bad[0]]!r}")


def new_arena():
    return Arena(torch.device("cuda:0"))
