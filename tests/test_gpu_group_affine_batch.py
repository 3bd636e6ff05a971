"""GPU tests of asymmetric layers in the group batch (include/lq_hip.h: lq_group_batch_create_affine): tensors with a learned offset
per group, and the symmetric biases next to them, in ONE forward and ONE backward launch -- from the C ABI up to
FakeQuantBatch(group_batch=True, asymmetric=True) and Trainer(asymmetric_batch=True).

The references are tests/_group_affine_reference.py::group_affine_reference and tests/_group_reference.py::group_reference.  The
ten-tensor set (R, C, axis, gs) of tests/test_gpu_group_batch.py; tensor i has range [(-8, 7), (0, 15), (-3, 5)][i % 3],
grad_scale 0.37 * (i + 1) and offset_grad_scale 0.21 * (i + 1).  Tensors 6 and 7, the bias-shaped lines, are SYMMETRIC (b = NULL,
inputs from ``make_case(100 + i, ...)``); the other eight are affine (inputs from ``make_affine_case(200 + i, ...)``):

    0 (37, 5, 0, 8)        affine     scalar columns, ragged last group, one block per group
    1 (256, 260, 0, 32)    affine     float4 columns, 5 column tiles, the last of 4 columns
    2 (96, 130, 0, 96)     affine     scalar columns (C % 4 != 0), gs = len, forward row split over 4 blocks
    3 (7, 27, 1, 8)        affine     scalar rows, ragged last group, team of 2 lanes
    4 (64, 576, 1, 128)    affine     float4 rows, ragged last group (64 elements), team of 8 lanes
    5 (33, 4100, 1, 128)   affine     float4 rows, 35 blocks, a last group of 4 elements
    6 (1, 10, 1, 10)       symmetric  a bias-shaped line: scalar rows, one group, one block, team of 4 lanes
    7 (1, 512, 1, 512)     symmetric  a bias-shaped line: float4 rows, team of 32 lanes
    8 (300, 64, 0, 1)      affine     float4 columns, gs = 1: 300 blocks of one row each (15 of 16 row slots idle)
    9 (40, 64, 1, 4)       affine     float4 rows, team of ONE lane

Coverage: k_group_batch_affine has four instantiations, <RNE, BWD> in {floor, nearest} x {forward, backward}; each holds the four
forms as block-uniform branches, once with an offset and once without.  ``test_parity`` launches all four (its two roundings,
forward and backward), and in each of them tensors 1, 8 run the float4 column form with an offset, 0, 2 the scalar column form with
an offset, 4, 5, 9 the float4 row form with an offset and 7 without, 3 the scalar row form with an offset and 6 without.
``test_alignment`` moves tensor 1 to the scalar column form.  The symmetric column forms inside the affine kernel run in
``test_zero_offset_and_no_offsets`` (a batch in which one tensor has an offset and every other tensor is symmetric).

The bar: out, dP and the clip counts equal the reference AND the single-tensor ops bit for bit (lq_fq_*_group_affine for the affine
tensors, lq_fq_*_group for tensors 6 and 7: the sign of zero included); ds and db equal the single-tensor op's bit for bit (a block
runs the same device function on the same unit of work) and are held to tests/_bounds.py::assert_within_terms (1e-5 * sum|terms|;
the terms of db are the |dy| of the clipped elements) against the reference.  Condition, asserted on the reference before any
comparison: every tensor has 0 < clipped < numel, and every affine tensor has a group with db != 0.

Biases (``test_layers``, the trainer test): the per-tensor path of a bias is the one-axis clipped op, a different traversal of the
same sum -- out and P.grad are compared bit for bit, ds within the bound."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _arena import Arena                                                                  # noqa: E402
from _bounds import assert_within_terms                                                   # noqa: E402
from _clip_reference import bits_equal                                                    # noqa: E402
from _group_affine_reference import group_affine_reference, make_affine_case              # noqa: E402
from _group_reference import group_reference, make_case                                   # noqa: E402

pytestmark = pytest.mark.gpu

SET = [(37, 5, 0, 8), (256, 260, 0, 32), (96, 130, 0, 96), (7, 27, 1, 8), (64, 576, 1, 128), (33, 4100, 1, 128), (1, 10, 1, 10),
       (1, 512, 1, 512), (300, 64, 0, 1), (40, 64, 1, 4)]
SYMMETRIC = (6, 7)
RANGES = [(-8, 7), (0, 15), (-3, 5)]
ROUNDINGS = ("floor", "nearest")
EINVAL, EALIGN = -1, -4
SENTINEL = 0x7F7F7F7F
N = len(SET)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _k(i):
    return float(np.float32(0.37 * (i + 1)))


def _kb(i):
    return float(np.float32(0.21 * (i + 1)))


_INPUTS, _REFS = {}, {}


def _inputs(i):
    """(P, s, b | None, dy) of tensor i."""
    if i not in _INPUTS:
        if i in SYMMETRIC:
            P, s, dy = make_case(100 + i, *SET[i])
            _INPUTS[i] = (P, s, None, dy)
        else:
            _INPUTS[i] = make_affine_case(200 + i, *SET[i])
    return _INPUTS[i]


def _reference(i, rounding, P=None, b=None):
    Pn, s, bn, dy = _inputs(i)
    Pn, bn = (Pn if P is None else P), (bn if b is None else b)
    R, C, axis, gs = SET[i]
    if bn is None:
        return group_reference(Pn, s, dy, *RANGES[i % 3], axis, gs, k=_k(i), rounding=rounding)
    return group_affine_reference(Pn, s, bn, dy, *RANGES[i % 3], axis, gs, k=_k(i), kb=_kb(i), rounding=rounding)


def _ref(i, rounding):
    """Reference of tensor i, computed once and shared (never modified); the condition is asserted here."""
    if (i, rounding) not in _REFS:
        ref = _reference(i, rounding)
        clipped, numel = int(ref["clipped"].sum()), _inputs(i)[0].size
        assert 0 < clipped < numel, f"tensor {i} {rounding}: {clipped} of {numel} clipped"
        if i not in SYMMETRIC:
            assert bool((ref["db"] != 0).any()), f"tensor {i} {rounding}: db is zero in every group"
        _REFS[(i, rounding)] = ref
    return _REFS[(i, rounding)]


class Buf:
    """Device buffers of one tensor: inputs uploaded, outputs preset to the sentinel word.  ``b``: another offset than the
    inputs' (an array), or False for a symmetric tensor; ``db=False``: an affine tensor without a db buffer."""

    def __init__(self, i, dev, P=None, b=None, offset=0, db=True):
        Pn, sn, bn, dyn = _inputs(i)
        Pn = Pn if P is None else P
        bn = None if b is False else (bn if b is None else b)
        self.i, self.geom, self.range = i, SET[i], RANGES[i % 3]
        self.k, self.kb = _k(i), _kb(i)                               # grad_scale and offset_grad_scale of this tensor
        self.s = _t(sn, dev)
        self.b = None if bn is None else _t(bn, dev)
        self.P, self.dy = self._at(Pn, dev, offset), self._at(dyn, dev, offset)
        self.out, self.dp = self._at(None, dev, offset, Pn.shape), self._at(None, dev, offset, Pn.shape)
        self.ds = torch.full(sn.shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        self.db = torch.full(sn.shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        self.pass_db = db and self.b is not None

    @staticmethod
    def _at(a, dev, offset, shape=None):
        """A tensor whose base is ``offset`` floats past a 16-byte aligned address."""
        shape = a.shape if a is not None else shape
        n = int(np.prod(shape))
        raw = torch.full((n + 4,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        assert raw.data_ptr() % 16 == 0
        v = raw[offset:offset + n].view(shape)
        if a is not None:
            v.copy_(_t(a, dev))
        return v

    def desc(self, _hip):
        R, C, axis, gs = self.geom
        return _hip.GroupDesc(self.P.data_ptr(), self.s.data_ptr(), self.out.data_ptr(), self.dp.data_ptr(), self.ds.data_ptr(),
                              R, C, gs, axis, *self.range)

    def off(self, _hip):
        if self.b is None:
            return _hip.GroupOffset(None, None, 0.0)
        return _hip.GroupOffset(self.b.data_ptr(), self.db.data_ptr() if self.pass_db else None, self.kb)

    def untouched(self, *names):
        return all(bool((getattr(self, n).view(torch.int32) == SENTINEL).all()) for n in names)

    def reset(self):
        for t in (self.out, self.dp, self.ds, self.db):
            t.view(torch.int32).fill_(SENTINEL)


class Batch:
    """``offs``: "affine" (lq_group_batch_create_affine with every tensor's offset), "null" (the same call with offs = NULL) or
    "plain" (lq_group_batch_create)."""

    def __init__(self, bufs, rounding="floor", offs="affine"):
        from learned_quantization_amd import _hip
        self._hip, self.lib, self.bufs = _hip, _hip.load(), bufs
        n = len(bufs)
        arr = (_hip.GroupDesc * n)(*[b.desc(_hip) for b in bufs])
        self.handle = ctypes.c_void_p()
        rnd = ROUNDINGS.index(rounding)
        if offs == "plain":
            _hip.check(self.lib.lq_group_batch_create(arr, n, rnd, ctypes.byref(self.handle)), "lq_group_batch_create")
        else:
            oarr = (_hip.GroupOffset * n)(*[b.off(_hip) for b in bufs]) if offs == "affine" else None
            _hip.check(self.lib.lq_group_batch_create_affine(arr, oarr, n, rnd, ctypes.byref(self.handle)), "lq_group_batch_create_affine")
        assert self.lib.lq_group_batch_workspace_bytes(self.handle) == 0
        self.dev = bufs[0].P.device

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.lq_group_batch_destroy(self.handle)
            self.handle = None

    def forward(self):
        self._hip.check(self.lib.lq_group_batch_forward(self.handle, self._hip.stream_ptr(self.dev)), "lq_group_batch_forward")

    def backward_rc(self, dys=None, mask_only=False):
        n = len(self.bufs)
        ptrs = (ctypes.c_void_p * n)(*[(b.dy if dys is None else dys[j]).data_ptr() for j, b in enumerate(self.bufs)])
        gs = None if mask_only else (ctypes.c_float * n)(*[b.k for b in self.bufs])
        return self.lib.lq_group_batch_backward(self.handle, ptrs, gs, None, 0, self._hip.stream_ptr(self.dev))

    def backward(self, **kw):
        self._hip.check(self.backward_rc(**kw), "lq_group_batch_backward")


def _read_counts(batch, j):
    """The batch-owned counts of tensor j as int64 in the scale's shape (a copy through the CUDA array interface)."""
    from learned_quantization_amd.batch import _DeviceInts
    dev_p, groups = ctypes.c_void_p(), ctypes.c_int64()
    batch._hip.check(batch.lib.lq_group_batch_clip_counts(batch.handle, j, ctypes.byref(dev_p), ctypes.byref(groups)), "clip_counts")
    b = batch.bufs[j]
    assert groups.value == b.s.numel()
    view = torch.as_tensor(_DeviceInts(dev_p.value, groups.value), device=batch.dev)
    return view.clone().cpu().numpy().view(np.uint32).astype(np.int64).reshape(tuple(b.s.shape))


def _single(b, rounding):
    """The single-tensor ops on the same buffers: (out, dP, ds, db | None, counts) as NumPy arrays -- lq_fq_*_group_affine for a
    tensor with an offset, lq_fq_*_group for one without."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = b.geom
    rnd = ROUNDINGS.index(rounding)
    st = _hip.stream_ptr(b.P.device)
    out, dP = torch.empty_like(b.P), torch.empty_like(b.P)
    # the single-tensor call takes the batch's form: a misaligned P or dy alone sends both to the scalar form, aligned ones to float4
    assert out.data_ptr() % 16 == 0 and dP.data_ptr() % 16 == 0
    ds, cnt = torch.empty_like(b.s), torch.empty(b.s.shape, dtype=torch.int32, device=b.P.device)
    if b.b is None:
        db = None
        _hip.check(lib.lq_fq_forward_group(b.P.data_ptr(), b.s.data_ptr(), out.data_ptr(), None, 0, *b.range, rnd, R, C, axis, gs, st), "fwd")
        _hip.check(lib.lq_fq_backward_group(b.P.data_ptr(), b.s.data_ptr(), b.dy.data_ptr(), *b.range, rnd, b.k, dP.data_ptr(),
                                            ds.data_ptr(), cnt.data_ptr(), None, 0, R, C, axis, gs, st), "bwd")
    else:
        db = torch.empty_like(b.s)
        _hip.check(lib.lq_fq_forward_group_affine(b.P.data_ptr(), b.s.data_ptr(), b.b.data_ptr(), out.data_ptr(), None, 0, *b.range, rnd,
                                                  R, C, axis, gs, st), "affine fwd")
        _hip.check(lib.lq_fq_backward_group_affine(b.P.data_ptr(), b.s.data_ptr(), b.b.data_ptr(), b.dy.data_ptr(), *b.range, rnd,
                                                   b.k, b.kb, dP.data_ptr(), ds.data_ptr(), db.data_ptr(), cnt.data_ptr(),
                                                   None, 0, R, C, axis, gs, st), "affine bwd")
    return (out.cpu().numpy(), dP.cpu().numpy(), ds.cpu().numpy(), None if db is None else db.cpu().numpy(),
            cnt.cpu().numpy().view(np.uint32).astype(np.int64))


def _results(batch):
    """(out, dP, ds, db | None, counts) per tensor; db is None where the tensor has no offset or no db buffer."""
    torch.cuda.synchronize()
    return [(b.out.cpu().numpy(), b.dp.cpu().numpy(), b.ds.cpu().numpy(), b.db.cpu().numpy() if b.pass_db else None, _read_counts(batch, j))
            for j, b in enumerate(batch.bufs)]


def _same(a, b, what, db=True):
    for name, x, y in zip(("out", "dP", "ds", "db"), a[:4], b[:4]):
        if name == "db" and (not db or x is None or y is None):
            assert not db or (x is None and y is None), f"{what}: db on one side only"
            continue
        assert bits_equal(x, y), f"{what}: {name}"
    assert np.array_equal(a[4], b[4]), f"{what}: counts"


_BATCH_RESULTS = {}


def _run_set(dev, rounding):
    bufs = [Buf(i, dev) for i in range(N)]
    batch = Batch(bufs, rounding)
    batch.forward()
    batch.backward()
    return _results(batch), bufs


def _reference_run(dev, rounding):
    if rounding not in _BATCH_RESULTS:
        _BATCH_RESULTS[rounding] = _run_set(dev, rounding)[0]
    return _BATCH_RESULTS[rounding]


# ------------------------------------------------------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_parity(dev, rounding):
    refs = [_ref(i, rounding) for i in range(N)]                   # the condition holds for every tensor before any comparison
    got, bufs = _run_set(dev, rounding)
    _BATCH_RESULTS.setdefault(rounding, got)
    worst = [0.0, 0.0]
    for i, b in enumerate(bufs):
        out, dP, ds, db, cnt = got[i]
        ref = refs[i]
        what = f"tensor {i} {SET[i]} {rounding}"
        assert bits_equal(out, ref["out"]), f"{what}: out against the reference"
        assert bits_equal(dP, ref["dP"]), f"{what}: dP against the reference"
        assert np.array_equal(cnt, ref["clipped"]), f"{what}: counts against the reference"
        _same(got[i], _single(b, rounding), f"{what} against the single-tensor ops")
        assert (db is None) == (i in SYMMETRIC)
        assert b.untouched("db") == (i in SYMMETRIC), f"{what}: the db buffer of a symmetric tensor was written, or an affine one's not"
        pairs = [(ds, "ds", "terms")] + ([] if db is None else [(db, "db", "terms_b")])
        for n, (g, key, terms) in enumerate(pairs):
            with np.errstate(all="ignore"):
                worst[n] = max(worst[n], float(np.max(np.abs(g.astype(np.float64) - ref[key]) / np.maximum(ref[terms], 1e-300))))
            assert_within_terms(g, ref[key], ref[terms], f"{what}: {key} against the reference")
    print(f"{rounding}: worst |ds - ref| / sum|terms| = {worst[0]:.3e}, worst |db - ref| / sum|terms_b| = {worst[1]:.3e}")


# ---------------------------------------------------------------------------------------------------------- 2 memory contract
def test_memory_contract(dev):
    """Every pointer of the batch is a region of one poisoned arena.  A full forward + backward fills every output and leaves the
    guard bands alone; mask only writes neither ds nor db; tensor 4 without a db buffer has its ds and nothing else of its own."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    want = _reference_run(dev, "floor")
    ar = Arena(dev)
    for i, (R, C, axis, gs) in enumerate(SET):
        P, s, b, dy = _inputs(i)
        row = C * 4
        ar.add(f"P{i}", "in", data=P, row_bytes=row)
        ar.add(f"s{i}", "in", data=s)
        if b is not None:
            ar.add(f"b{i}", "in", data=b)
            ar.add(f"db{i}", "out", nbytes=s.nbytes)
        ar.add(f"dy{i}", "in", data=dy, row_bytes=row)
        ar.add(f"out{i}", "out", nbytes=P.nbytes, row_bytes=row)
        ar.add(f"dp{i}", "out", nbytes=P.nbytes, row_bytes=row)
        ar.add(f"ds{i}", "out", nbytes=s.nbytes)
    ar.build()
    arr = (_hip.GroupDesc * N)(*[_hip.GroupDesc(ar.ptr(f"P{i}"), ar.ptr(f"s{i}"), ar.ptr(f"out{i}"), ar.ptr(f"dp{i}"), ar.ptr(f"ds{i}"),
                                                SET[i][0], SET[i][1], SET[i][3], SET[i][2], *RANGES[i % 3]) for i in range(N)])
    affine = [i for i in range(N) if i not in SYMMETRIC]
    outs = [f"{n}{i}" for i in range(N) for n in ("out", "dp", "ds")]
    dys = (ctypes.c_void_p * N)(*[ar.ptr(f"dy{i}") for i in range(N)])
    ks = (ctypes.c_float * N)(*[_k(i) for i in range(N)])
    st = _hip.stream_ptr(dev)

    def run(no_db=(), mask_only=False):
        offs = (_hip.GroupOffset * N)(*[_hip.GroupOffset(None, None, 0.0) if i in SYMMETRIC else
                                        _hip.GroupOffset(ar.ptr(f"b{i}"), None if i in no_db else ar.ptr(f"db{i}"), _kb(i)) for i in range(N)])
        handle = ctypes.c_void_p()
        _hip.check(lib.lq_group_batch_create_affine(arr, offs, N, 0, ctypes.byref(handle)), "lq_group_batch_create_affine")
        try:
            assert lib.lq_group_batch_workspace_bytes(handle) == 0
            for name in outs + [f"db{i}" for i in affine]:
                ar.fill(name, 0x7F)
            _hip.check(lib.lq_group_batch_forward(handle, st), "forward")
            _hip.check(lib.lq_group_batch_backward(handle, dys, None if mask_only else ks, None, 0, st), "backward")
            torch.cuda.synchronize(dev)
        finally:
            lib.lq_group_batch_destroy(handle)

    run()
    ar.check("affine group batch")                                 # every out, dp, ds and db filled; guards and inputs intact
    for i in range(N):
        for name, w in zip(("out", "dp", "ds"), want[i][:3]):
            assert bits_equal(ar.numpy(f"{name}{i}", np.float32).reshape(w.shape), w), f"tensor {i}: {name} of the arena run"
        if i in affine:
            assert bits_equal(ar.numpy(f"db{i}", np.float32).reshape(want[i][3].shape), want[i][3]), f"tensor {i}: db of the arena run"
    run(mask_only=True)
    ar.check("affine group batch, mask only", written=[f"{n}{i}" for i in range(N) for n in ("out", "dp")])
    for i in range(N):
        assert bits_equal(ar.numpy(f"dp{i}", np.float32).reshape(want[i][1].shape), want[i][1]), f"tensor {i}: dP of the mask-only call"
    run(no_db=(4,))
    ar.check("affine group batch, tensor 4 without db", written=outs + [f"db{i}" for i in affine if i != 4])
    assert bits_equal(ar.numpy("ds4", np.float32).reshape(want[4][2].shape), want[4][2]), "tensor 4: ds without a db buffer"
    assert bits_equal(ar.numpy("db1", np.float32).reshape(want[1][3].shape), want[1][3]), "tensor 1: db next to a tensor without one"


# ---------------------------------------------------------------------------------------------------------------- 3 alignment
def test_alignment(dev):
    """Tensor 1 with every dense base 4 bytes off the 16-byte grid: the scalar column form, and the single-tensor ops' bits on the
    same buffers.  A misaligned dy for a tensor whose table entry is a float4 form: LQ_EALIGN before any launch."""
    want = _reference_run(dev, "floor")
    bufs = [Buf(0, dev), Buf(1, dev, offset=1), Buf(7, dev)]
    for t in (bufs[1].P, bufs[1].out, bufs[1].dp, bufs[1].dy):
        assert t.data_ptr() % 16 == 4
    batch = Batch(bufs, "floor")
    batch.forward()
    batch.backward()
    res = _results(batch)
    for b, r in zip(bufs, res):
        _same(r, _single(b, "floor"), f"tensor {b.i} (tensor 1 misaligned) against the single-tensor ops on these buffers")
    assert bits_equal(res[1][0], want[1][0]) and bits_equal(res[1][1], want[1][1]) and np.array_equal(res[1][4], want[1][4])
    ref = _ref(1, "floor")
    assert_within_terms(res[1][2], ref["ds"], ref["terms"], "ds of the scalar form")
    assert_within_terms(res[1][3], ref["db"], ref["terms_b"], "db of the scalar form")
    bufs = [Buf(0, dev), Buf(1, dev), Buf(7, dev)]
    batch = Batch(bufs, "floor")
    off = Buf._at(_inputs(1)[3], dev, 1)
    assert off.data_ptr() % 16 == 4
    assert batch.backward_rc(dys=[bufs[0].dy, off, bufs[2].dy]) == EALIGN and b"tensor 1" in batch.lib.lq_last_error()
    torch.cuda.synchronize()
    assert all(b.untouched("ds", "db", "dp", "out") for b in bufs), "a refused call launched"


# --------------------------------------------------------------------------------------------------------- 4 degenerate cases
def test_zero_offset_and_no_offsets(dev):
    """b == +0 on every tensor: dP, ds and the counts are the symmetric batch's bits, out is its value, db = kb * sum of dy over the
    clipped elements.  offs = NULL, and a batch in which only tensor 0 has an offset: the symmetric batch's bits for the rest."""
    sym = [Buf(i, dev, P=make_case(100 + i, *SET[i])[0], b=False) for i in range(N)]
    for b_ in sym:                                                  # the symmetric file's inputs for all ten: P and dy of make_case
        P, s, dy = make_case(100 + b_.i, *SET[b_.i])
        b_.s.copy_(_t(s, dev)), b_.dy.copy_(_t(dy, dev))
    plain = Batch(sym, "floor", offs="plain")
    plain.forward()
    plain.backward()
    want = _results(plain)
    for b_ in sym:
        b_.reset()
    null = Batch(sym, "floor", offs="null")
    null.forward()
    null.backward()
    for i, r in enumerate(_results(null)):
        _same(r, want[i], f"tensor {i}: offs = NULL against lq_group_batch_create")
    zero = []
    for b_ in sym:
        z = Buf(b_.i, dev, P=b_.P.cpu().numpy(), b=np.zeros(tuple(b_.s.shape), np.float32))
        z.s.copy_(b_.s), z.dy.copy_(b_.dy)
        zero.append(z)
    zb = Batch(zero, "floor")
    zb.forward()
    zb.backward()
    for i, (r, z) in enumerate(zip(_results(zb), zero)):
        assert np.array_equal(r[0], want[i][0]), f"tensor {i}: out at b = 0 (as a value)"
        for name, x, y in (("dP", r[1], want[i][1]), ("ds", r[2], want[i][2])):
            assert bits_equal(x, y), f"tensor {i}: {name} at b = 0 against the symmetric batch"
        assert np.array_equal(r[4], want[i][4]), f"tensor {i}: counts at b = 0"
        R, C, axis, gs = SET[i]
        ref = group_affine_reference(z.P.cpu().numpy(), z.s.cpu().numpy(), np.zeros(tuple(z.s.shape), np.float32), z.dy.cpu().numpy(),
                                     *RANGES[i % 3], axis, gs, k=_k(i), kb=_kb(i))
        assert bits_equal(r[1], ref["dP"])
        assert_within_terms(r[3], ref["db"], ref["terms_b"], f"tensor {i}: db = kb * sum of dy over the clipped elements")
    # one affine tensor among symmetric ones: the symmetric side of every form inside k_group_batch_affine
    mixed = [Buf(0, dev)] + [Buf(b_.i, dev, P=b_.P.cpu().numpy(), b=False) for b_ in sym[1:]]
    for m, b_ in zip(mixed[1:], sym[1:]):
        m.s.copy_(b_.s), m.dy.copy_(b_.dy)
    mb = Batch(mixed, "floor")
    mb.forward()
    mb.backward()
    res = _results(mb)
    _same(res[0], _reference_run(dev, "floor")[0], "tensor 0 with its offset")
    for i in range(1, N):
        _same(res[i], want[i], f"tensor {i}: a symmetric tensor of the affine kernel against lq_group_batch_create")
        assert mixed[i].untouched("db")


def test_nan_in_an_offset_stays_in_its_group(dev):
    want = _reference_run(dev, "floor")
    b4 = _inputs(4)[2].copy()
    b4[5, 1] = np.nan                                               # row 5, group 1 of tensor 4 (64, 576, 1, 128)
    bufs = [Buf(i, dev, b=b4 if i == 4 else None) for i in range(N)]
    batch = Batch(bufs, "floor")
    batch.forward()
    batch.backward()
    res = _results(batch)
    for i in range(N):
        if i != 4:
            _same(res[i], want[i], f"tensor {i} next to a NaN offset in tensor 4")
    spoiled = np.zeros(b4.shape, bool)
    spoiled[5, 1] = True
    ref = _reference(4, "floor", b=b4)
    assert np.array_equal(np.isnan(res[4][2]), spoiled), "ds: NaN in other groups than the spoiled one"
    # every element of the spoiled group is outside the range (no comparison with a NaN holds): its db is kb times the sum of all its dy
    assert not np.isnan(res[4][3]).any() and int(ref["clipped"][5, 1]) == 128
    assert_within_terms(res[4][3][spoiled], ref["db"][spoiled], ref["terms_b"][spoiled], "db of the spoiled group")
    for name, k in (("ds", 2), ("db", 3)):
        assert bits_equal(res[4][k][~spoiled], want[4][k][~spoiled]), f"{name} of the other groups"
    assert bits_equal(res[4][0], ref["out"]) and bits_equal(res[4][1], ref["dP"]) and np.array_equal(res[4][4], ref["clipped"])
    elems = np.zeros(SET[4][:2], bool)
    elems[5, 128:256] = True
    assert np.array_equal(np.isnan(res[4][0]), elems), "out: NaN outside the spoiled group"


# -------------------------------------------------------------------------------------------------------------------- 5 capture
def test_capture_and_replay(dev):
    """Forward + backward recorded on one stream and replayed twice: the eager bits, both times."""
    eager = _reference_run(dev, "nearest")
    bufs = [Buf(i, dev) for i in range(N)]
    batch = Batch(bufs, "nearest")
    batch.forward()
    batch.backward()                                                # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch.forward()
        batch.backward()
    for n in range(2):
        for b in bufs:
            b.reset()
        g.replay()
        for i, r in enumerate(_results(batch)):
            _same(r, eager[i], f"tensor {i}: replay {n} against the eager batch")


# --------------------------------------------------------------------------------------------------------------------- 6 layers
def _asymmetric_model(dev, seed=3):
    """The MNIST model with offsets: scales and offsets from min-max, then shaken off their initial values so that elements clip on
    both sides; biases (created at zero) and their scalar scales set so that some of their elements clip too."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    model = lq.build_model("mnist", seed=seed, mode="ste", value=0.0, bits=4, group_size=64, device=dev, asymmetric=True,
                           scale_init="minmax")
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for layer in lq.custom_layers_of(model):
            nested = layer.weight_nested()
            shape = tuple(nested.scale.shape)
            nested.scale.mul_(_t(rng.uniform(0.4, 0.8, shape).astype(np.float32), dev))
            nested.offset.add_(nested.scale * _t(rng.uniform(-2, 2, shape).astype(np.float32), dev))
            layer.b.copy_(_t((rng.standard_normal(tuple(layer.b.shape)) * 0.05).astype(np.float32), dev))
            layer.nested_q_b_layer.scale.fill_(0.05 / 4)
    return model


def _linear_objective(layers, cs):
    total, outs = None, []
    for layer, (ck, cb) in zip(layers, cs):
        w, qb = layer.quantized_parameters()
        outs += [w, qb]
        t = (w * ck).sum() + (qb * cb).sum()
        total = t if total is None else total + t
    return total, outs


@pytest.mark.parametrize("autograd", [True, False], ids=["autograd", "leaves"])
def test_layers(dev, autograd):
    """FakeQuantBatch(group_batch=True, asymmetric=True) against the per-tensor layers on injected upstream gradients.  Kernels: out,
    P.grad, scale.grad and offset.grad bit for bit.  Biases: out and P.grad bit for bit, ds within the bound against the reference
    of the bias geometry.  Then a preset contiguous offset.grad (a bucket view) is written in place."""
    import learned_quantization_amd as lq
    from learned_quantization_amd.batch import BatchedScaleAdam, FakeQuantBatch
    model = _asymmetric_model(dev)
    layers = lq.custom_layers_of(model)
    g = torch.Generator().manual_seed(17)
    cs = [(torch.randn(tuple(l.W.shape), generator=g).to(dev), torch.randn(tuple(l.b.shape), generator=g).to(dev)) for l in layers]

    def tensors():
        out = []
        for l in layers:
            n = l.weight_nested()
            out += [(l.W, n.scale, n.offset), (l.b, l.nested_q_b_layer.scale, None)]
        return out

    def clear():
        for p, s, o in tensors():
            p.grad = s.grad = None
            if o is not None:
                o.grad = None

    total, outs = _linear_objective(layers, cs)                    # the per-tensor path
    total.backward()
    want = [(w.detach().clone(), p.grad.detach().clone(), s.grad.detach().clone(), None if o is None else o.grad.detach().clone())
            for w, (p, s, o) in zip(outs, tensors())]
    clear()
    batch = FakeQuantBatch(model, autograd=autograd, group_batch=True, asymmetric=True)
    assert [e.offset is not None for e in batch.entries] == [True, False] * len(layers)
    opt = BatchedScaleAdam(batch)
    assert len(opt.param_groups[0]["params"]) == 3 * len(layers)

    def run():
        batch.quantize_all()
        total, outs = _linear_objective(layers, cs)
        total.backward()
        if not autograd:
            batch.finish_backward()
        return outs

    outs = run()
    for j, ((p, s, o), w, (wo, wp, ws, wb)) in enumerate(zip(tensors(), outs, want)):
        assert torch.equal(w.detach().view(torch.int32), wo.view(torch.int32)), f"tensor {j}: out"
        assert torch.equal(p.grad, wp), f"tensor {j}: P.grad"
        assert bool((p.grad == 0).any()) and bool((p.grad != 0).any()), f"tensor {j}: the mask is not at work"
        if o is not None:
            assert torch.equal(s.grad, ws), f"tensor {j}: scale.grad against the per-tensor layer"
            assert torch.equal(o.grad, wb) and bool((o.grad != 0).any()), f"tensor {j}: offset.grad against the per-tensor layer"
        else:
            n = p.numel()
            nested = layers[j // 2].nested_q_b_layer
            ref = group_reference(p.detach().cpu().numpy().reshape(1, n), s.detach().cpu().numpy().reshape(1, 1),
                                  cs[j // 2][1].cpu().numpy().reshape(1, n), -8, 7, 1, n, k=nested.grad_scale_value(n))
            assert 0 < int(ref["clipped"].sum()) < n
            assert bits_equal(p.grad.cpu().numpy().reshape(1, n), ref["dP"])
            for got, who in ((s.grad, "batched"), (ws, "per-tensor")):
                assert_within_terms(got.cpu().numpy(), ref["ds"], ref["terms"], f"tensor {j}: bias ds, {who}")
    opt.zero_grad()
    assert all(s.grad is None and (o is None or o.grad is None) for _, s, o in tensors())
    # a bucket view as the offset's gradient: the batch built over it writes db there
    clear()
    nested = layers[0].weight_nested()
    flat = torch.zeros(nested.offset.numel() + 8, device=dev)
    view = flat[4:4 + nested.offset.numel()].view_as(nested.offset)
    nested.offset.grad = view
    batch = FakeQuantBatch(model, autograd=autograd, group_batch=True, asymmetric=True)
    assert batch._external_grads and batch.entries[0].db is view
    run()
    assert nested.offset.grad is view
    assert torch.equal(flat[4:4 + view.numel()].view_as(view), want[0][3]) and bool((flat[:4] == 0).all()) and bool((flat[-4:] == 0).all())


# -------------------------------------------------------------------------------------------------------------------- 7 trainer
def _recipe(model, dev, seed):
    """Scales at which a sizeable share of the weights is inside the range (tests/test_gpu_group_batch.py::_recipe), and offsets a
    few steps off zero."""
    import learned_quantization_amd as lq
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for layer in lq.custom_layers_of(model):
            for name in ("nested_q_w_layer", "nested_q_k_layer", "nested_q_b_layer"):
                nested = getattr(layer, name, None)
                if nested is not None:
                    shape = tuple(nested.scale.shape)
                    v = np.float32(0.05 / 4) * rng.uniform(0.8, 1.25, shape).astype(np.float32)
                    nested.scale.copy_(torch.from_numpy(v).to(dev))
                    if nested.offset is not None:
                        nested.offset.copy_(torch.from_numpy(v * rng.uniform(-2, 2, shape).astype(np.float32)).to(dev))


def _linear_trainer(dev, tmp, steps, **kw):
    from _linear_task import LinearTaskTrainer, make_coefficients
    tr = LinearTaskTrainer(config="cifar", mode="ste", value=0.0, device=dev, log_dir=str(tmp), seed=3, bits=4, group_size=128, lr=1e-3,
                           asymmetric=True, **kw)
    _recipe(tr.model, dev, 3)
    with torch.no_grad():                                           # biases are created at zero: give them something to clip
        g = torch.Generator().manual_seed(11)
        for layer in tr.custom_layers:
            if getattr(layer, "b", None) is not None:
                layer.b.copy_((torch.randn(layer.b.shape, generator=g) * 0.05).to(dev))
    tr.coefficients = make_coefficients(tr, steps, lo=-3.0, hi=-1.0)
    return tr


BATCHED = dict(batched=True, group_batch=True, asymmetric_batch=True)


def test_trainer_step_matches_the_per_tensor_path(dev, tmp_path):
    """Step 1 of the asymmetric batch against the per-tensor path on injected gradients: P.grad of every tensor, ds and db of every
    kernel bit for bit, scales and offsets after the step too; ds of the biases within the bound against the reference."""
    import learned_quantization_amd as lq
    plain = _linear_trainer(dev, tmp_path / "a", 1)
    lq.reset_layer_names()
    batched = _linear_trainer(dev, tmp_path / "b", 1, **BATCHED)
    assert batched.batch.asymmetric and any(e.offset is not None for e in batched.batch.entries)
    before = {}
    for layer, cs in zip(plain.custom_layers, plain.coefficients[0]):
        if len(cs) > 1:
            n = layer.b.numel()
            before[layer.name] = group_reference(layer.b.detach().cpu().numpy().reshape(1, n),
                                                 layer.nested_q_b_layer.scale.detach().cpu().numpy().reshape(1, 1),
                                                 cs[1].cpu().numpy().reshape(1, n), -8, 7, 1, n)
    x = torch.zeros(2, 3, 32, 32, device=dev)
    y = torch.zeros(2, dtype=torch.long, device=dev)
    la, lb = plain.step(x, y), batched.step(x, y)
    assert torch.equal(la, lb)
    for la_, lb_ in zip(plain.custom_layers, batched.custom_layers):
        assert torch.equal(la_.kernel.grad, lb_.kernel.grad), f"{la_.name}: P.grad of the kernel"
        na, nb = la_.nested_q_k_layer, lb_.nested_q_k_layer
        assert torch.equal(na.scale.grad, nb.scale.grad) and bool((nb.scale.grad != 0).all()), f"{la_.name}: ds of the kernel"
        assert torch.equal(na.offset.grad, nb.offset.grad) and bool((nb.offset.grad != 0).any()), f"{la_.name}: db of the kernel"
        assert torch.equal(na.scale.detach(), nb.scale.detach()), f"{la_.name}: the kernel's scales after the step"
        assert torch.equal(na.offset.detach(), nb.offset.detach()), f"{la_.name}: the kernel's offsets after the step"
        if la_.name in before:
            ref = before[la_.name]
            assert torch.equal(la_.b.grad, lb_.b.grad), f"{la_.name}: P.grad of the bias"
            assert bits_equal(lb_.b.grad.cpu().numpy().reshape(1, -1), ref["dP"])
            for tr_layer, who in ((la_, "per-tensor"), (lb_, "batched")):
                assert_within_terms(tr_layer.nested_q_b_layer.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], f"{la_.name}: bias ds, {who}")
    assert len(before) == len(plain.custom_layers)


def test_trainer_eager_and_graphed(dev, tmp_path):
    """The asymmetric batch eager and graph=True from the same state on a fixed linear task: three steps agree bit for bit, every
    parameter, scale and offset included; scales and offsets move."""
    from _linear_task import LinearTaskTrainer, make_coefficients
    from learned_quantization_amd.train import Trainer

    class FixedTask(LinearTaskTrainer):         # one coefficient set: the step can be captured (tests/test_gpu_group_affine.py)
        def __init__(self, *a, **kw):
            Trainer.__init__(self, *a, **kw)
            self.coefficients, self._n = None, 0

    runs = []
    x = torch.zeros(2, 1, 28, 28, device=dev)
    y = torch.zeros(2, dtype=torch.long, device=dev)
    for graph in (False, True):
        import learned_quantization_amd as lq
        lq.reset_layer_names()
        tr = FixedTask(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path / f"g{int(graph)}"), graph=graph, seed=7,
                       bits=4, group_size=64, asymmetric=True, scale_init="minmax", lr=1e-3, **BATCHED)
        tr.coefficients = make_coefficients(tr, 1, seed=7, lo=-3.0, hi=-1.0)
        start = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        step = tr.step_graphed if graph else tr.step
        losses = [step(x, y).detach().clone() for _ in range(3 + (0 if graph else 3))]      # step_graphed: 3 eager warm-up steps first
        torch.cuda.synchronize()
        runs.append((tr, losses[-3:], start))
    (eager, le, start), (graphed, lg, _) = runs
    assert graphed.graph is not None
    assert all(np.isfinite(float(a)) for a in le)
    for a, c in zip(le, lg):
        assert torch.equal(a, c), f"losses differ: {float(a)!r} {float(c)!r}"
    for (n, p), (_, p2) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), n
    names = {id(p): n for n, p in eager.model.named_parameters()}
    for layer in eager.custom_layers:
        nested = layer.nested_q_w_layer
        b0, s0 = start[names[id(nested.offset)]], start[names[id(nested.scale)]]
        assert nested.offset.grad is not None
        assert int((nested.offset.detach() != b0).sum()) > 0 and int((nested.scale.detach() != s0).sum()) > 0, layer.name


def test_one_rank_ddp_mode_a_equals_the_plain_step(dev, tmp_path):
    """Data-parallel mode A on a one-rank gloo group: ds AND db are written into the bucket views the batch found at construction,
    the exchange averages over one rank, and two steps leave every parameter, scale and offset where the plain batched steps do."""
    import socket
    import torch.distributed as dist
    import learned_quantization_amd as lq
    from _linear_task import snapshot

    def run(sub, **kw):
        lq.reset_layer_names()
        tr = _linear_trainer(dev, tmp_path / sub, 2, **BATCHED, **kw)
        for _ in range(2):
            tr.step(None, None)
        torch.cuda.synchronize()
        return tr, snapshot(tr)

    _, plain = run("plain")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        tr, dp = run("dp", ddp_mode="A", force_collectives=True)
        assert tr.dp is not None and tr.batch.asymmetric and tr.batch._external_grads
        views = {v.data_ptr() for v in tr.dp.bucket.views}
        for e in tr.batch.entries:
            assert e.ds.data_ptr() in views and (e.offset is None or e.db.data_ptr() in views), "a gradient outside the bucket"
    finally:
        dist.destroy_process_group()
    for n in plain:
        assert torch.equal(plain[n], dp[n]), n


def test_the_cli_line_runs(dev):
    from learned_quantization_amd import train
    train.main(["--config", "mnist", "--mode", "ste", "--bits", "4", "--group-size", "64", "--asymmetric", "--scale-init", "minmax",
                "--batch", "32", "--batched", "--group-batch", "--asymmetric", "--asymmetric-batch", "--steps", "2", "--warmup", "1"])


# ------------------------------------------------------------------------------------------------------------------ 8 refusals
def test_refusals_on_the_device(dev, tmp_path):
    """What needs a built model or a built batch to be refused: mode B, the clipped batch and the fused Adam step."""
    import learned_quantization_amd as lq
    from learned_quantization_amd.batch import BatchedScaleAdam, FakeQuantBatch
    from learned_quantization_amd.train import Trainer
    model = _asymmetric_model(dev)
    with pytest.raises(ValueError, match="together with clipped=True"):
        FakeQuantBatch(model, clipped=True, asymmetric=True)
    with pytest.raises(ValueError, match="belongs to group_batch=True"):
        FakeQuantBatch(model, asymmetric=True)
    batch = FakeQuantBatch(model, group_batch=True, asymmetric=True, autograd=False)
    with pytest.raises(ValueError, match="fused=False"):
        BatchedScaleAdam(batch, fused=True)
    with pytest.raises(ValueError, match="mode B"):
        batch.scale_grads_from_param_grads()
    batch.defer_scale_grads = True                                 # what DataParallel(mode="B").attach_batch sets
    batch.quantize_all()
    with pytest.raises(ValueError, match="mode B"):
        batch.finish_backward()
    with pytest.raises(ValueError, match="mode 'B'"):
        lq.DataParallel(model, mode="B")
    base = dict(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path), bits=4, group_size=64, asymmetric=True)
    with pytest.raises(ValueError, match="ddp_mode 'B'"):
        Trainer(ddp_mode="B", **BATCHED, **base)
    with pytest.raises(ValueError, match="without clipped_batch"):
        Trainer(clipped_batch=True, **BATCHED, **base)
    with pytest.raises(ValueError, match="asymmetric_batch=True belongs to"):
        Trainer(batched=True, clipped_batch=True, asymmetric_batch=True, **base)
    # a model without an asymmetric layer: the opt-in is allowed and is the plain group batch
    lq.reset_layer_names()
    sym = lq.build_model("mnist", seed=3, mode="ste", value=0.0, bits=4, group_size=64, device=dev)
    plain = FakeQuantBatch(sym, group_batch=True, asymmetric=True)
    assert all(e.offset is None for e in plain.entries)
    plain.quantize_all()
    torch.cuda.synchronize()
