"""GPU tests of microscaling (MX) layers in the group batch (include/lq_hip.h: lq_group_batch_create_mx): tensors on a minifloat
grid under one scale per group, each with its own element format and scale format, in ONE forward and ONE backward launch -- from
the C ABI up to FakeQuantBatch(group_batch=True, mx=True) and Trainer(mx_batch=True).

The reference is tests/_mx_reference.py::mx_reference.  The ten-tensor set (R, C, axis, gs) of tests/test_gpu_group_batch.py:

    0 (37, 5, 0, 8)        scalar columns, ragged last group, one block per group
    1 (256, 260, 0, 32)    float4 columns, 5 column tiles, the last of 4 columns
    2 (96, 130, 0, 96)     scalar columns (C % 4 != 0), gs = len, forward row split over 4 blocks
    3 (7, 27, 1, 8)        scalar rows, ragged last group, team of 2 lanes
    4 (64, 576, 1, 128)    float4 rows, ragged last group (64 elements), team of 8 lanes
    5 (33, 4100, 1, 128)   float4 rows, 35 blocks, a last group of 4 elements
    6 (1, 10, 1, 10)       a bias-shaped line: scalar rows, one group, one block, team of 4 lanes
    7 (1, 512, 1, 512)     a bias-shaped line: float4 rows, team of 32 lanes
    8 (300, 64, 0, 1)      float4 columns, gs = 1: 300 blocks of one row each (15 of 16 row slots idle)
    9 (40, 64, 1, 4)       float4 rows, team of ONE lane

Under rotation ``rot`` tensor i has the element format ``list(FORMATS)[(i + rot) % 5]`` and the scale format
``SCALE_FORMATS[i % 2]``; its inputs are ``_mx_reference.gaussian_case(name, sf, R, C, axis, gs)`` and its grad_scale is
0.37 * (i + 1).  ``test_parity`` runs the five rotations: every format meets every form, both scale formats included, and one
batch always mixes all five formats.

Coverage: k_group_batch_mx has two instantiations, forward and backward; each holds the four forms as block-uniform branches and
every rotation of ``test_parity`` launches both with all four forms (tensors 1, 8: float4 columns; 0, 2: scalar columns; 4, 5, 7,
9: float4 rows; 3, 6: scalar rows).  ``test_alignment`` moves tensor 1 to the scalar column form.

The bar: out, dP and the saturation counts equal the reference bit for bit, the sign of zero included, and ds is held to
tests/_bounds.py::assert_within_terms (1e-5 * sum|terms|) against it; out, dP, the counts AND ds equal lq_fq_forward_mx /
lq_fq_backward_mx on the same buffers bit for bit, the bias-shaped tensors 6 and 7 included (a block runs the same device function
on the same unit of work).  Condition, asserted on the reference before any comparison: every tensor has 0 < saturated < numel, and
its ds is NaN-free and not all zero (tests/test_mx_batch_cpu.py pins it for the 50 (rotation, tensor) pairs without a device)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _mx_reference as X                                                                 # noqa: E402
from _arena import Arena                                                                  # noqa: E402
from _bounds import assert_within_terms                                                   # noqa: E402
from _clip_reference import bits_equal                                                    # noqa: E402

pytestmark = pytest.mark.gpu

SET = [(37, 5, 0, 8), (256, 260, 0, 32), (96, 130, 0, 96), (7, 27, 1, 8), (64, 576, 1, 128), (33, 4100, 1, 128), (1, 10, 1, 10),
       (1, 512, 1, 512), (300, 64, 0, 1), (40, 64, 1, 4)]
NAMES = list(X.FORMATS)
ROTATIONS = range(len(NAMES))
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


def _format(i, rot):
    """(element format, scale format) of tensor i under rotation ``rot``."""
    return NAMES[(i + rot) % len(NAMES)], X.SCALE_FORMATS[i % 2]


_INPUTS, _REFS = {}, {}


def _inputs(i, rot):
    """(P, s, dy) of tensor i under rotation ``rot``."""
    key = (i,) + _format(i, rot)
    if key not in _INPUTS:
        _INPUTS[key] = X.gaussian_case(key[1], key[2], *SET[i])
    return _INPUTS[key]


def _reference(i, rot, s=None):
    P, sn, dy = _inputs(i, rot)
    name, sf = _format(i, rot)
    return X.mx_reference(P, sn if s is None else s, dy, X.FORMATS[name], sf, SET[i][2], SET[i][3], k=_k(i))


def _ref(i, rot):
    """Reference of tensor i, computed once and shared (never modified); the condition is asserted here."""
    key = (i,) + _format(i, rot)
    if key not in _REFS:
        ref = _reference(i, rot)
        saturated, numel = int(ref["clipped"].sum()), _inputs(i, rot)[0].size
        assert 0 < saturated < numel, f"tensor {i} rotation {rot}: {saturated} of {numel} saturated"
        assert not np.isnan(ref["ds"]).any() and bool((ref["ds"] != 0).any()), f"tensor {i} rotation {rot}: ds is NaN or all zero"
        _REFS[key] = ref
    return _REFS[key]


class Buf:
    """Device buffers of one tensor: inputs uploaded, outputs preset to the sentinel word.  ``s``: another scale than the inputs'."""

    def __init__(self, i, rot, dev, s=None, offset=0):
        Pn, sn, dyn = _inputs(i, rot)
        sn = sn if s is None else s
        self.i, self.geom, self.k = i, SET[i], _k(i)
        name, sf = _format(i, rot)
        self.fid, self.sid = X.FORMATS[name].id, X.SCALE_FORMATS.index(sf)
        self.s = _t(sn, dev)
        self.P, self.dy = self._at(Pn, dev, offset), self._at(dyn, dev, offset)
        self.out, self.dp = self._at(None, dev, offset, Pn.shape), self._at(None, dev, offset, Pn.shape)
        self.ds = torch.full(sn.shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)

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
        # qmin / qmax are not read: a range no integer batch would accept
        return _hip.GroupDesc(self.P.data_ptr(), self.s.data_ptr(), self.out.data_ptr(), self.dp.data_ptr(), self.ds.data_ptr(),
                              R, C, gs, axis, 5, -5)

    def untouched(self, *names):
        return all(bool((getattr(self, n).view(torch.int32) == SENTINEL).all()) for n in names)

    def reset(self):
        for t in (self.out, self.dp, self.ds):
            t.view(torch.int32).fill_(SENTINEL)


class Batch:
    def __init__(self, bufs):
        from learned_quantization_amd import _hip
        self._hip, self.lib, self.bufs = _hip, _hip.load(), bufs
        n = len(bufs)
        arr = (_hip.GroupDesc * n)(*[b.desc(_hip) for b in bufs])
        fmts = (_hip.GroupMxFormat * n)(*[_hip.GroupMxFormat(b.fid, b.sid) for b in bufs])
        self.handle = ctypes.c_void_p()
        _hip.check(self.lib.lq_group_batch_create_mx(arr, fmts, n, ctypes.byref(self.handle)), "lq_group_batch_create_mx")
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
        return self.lib.lq_group_batch_backward(self.handle, ptrs, gs, None, 0, self._hip.stream_ptr(self.dev))     # ws = NULL

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


def _single(b):
    """lq_fq_forward_mx / lq_fq_backward_mx on the same buffers: (out, dP, ds, counts) as NumPy arrays."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = b.geom
    st = _hip.stream_ptr(b.P.device)
    out, dP = torch.empty_like(b.P), torch.empty_like(b.P)
    # the single-tensor call takes the batch's form: a misaligned P or dy alone sends both to the scalar form, aligned ones to float4
    assert out.data_ptr() % 16 == 0 and dP.data_ptr() % 16 == 0
    ds, cnt = torch.empty_like(b.s), torch.empty(b.s.shape, dtype=torch.int32, device=b.P.device)
    _hip.check(lib.lq_fq_forward_mx(b.P.data_ptr(), b.s.data_ptr(), out.data_ptr(), None, 0, b.fid, b.sid, R, C, axis, gs, st), "fwd")
    _hip.check(lib.lq_fq_backward_mx(b.P.data_ptr(), b.s.data_ptr(), b.dy.data_ptr(), b.fid, b.sid, b.k, dP.data_ptr(), ds.data_ptr(),
                                     cnt.data_ptr(), R, C, axis, gs, st), "bwd")
    return out.cpu().numpy(), dP.cpu().numpy(), ds.cpu().numpy(), cnt.cpu().numpy().view(np.uint32).astype(np.int64)


def _results(batch):
    """(out, dP, ds, counts) per tensor."""
    torch.cuda.synchronize()
    return [(b.out.cpu().numpy(), b.dp.cpu().numpy(), b.ds.cpu().numpy(), _read_counts(batch, j)) for j, b in enumerate(batch.bufs)]


def _same(a, b, what):
    for name, x, y in zip(("out", "dP", "ds"), a[:3], b[:3]):
        assert bits_equal(x, y), f"{what}: {name}"
    assert np.array_equal(a[3], b[3]), f"{what}: counts"


_BATCH_RESULTS = {}


def _run_set(dev, rot):
    bufs = [Buf(i, rot, dev) for i in range(N)]
    batch = Batch(bufs)
    batch.forward()
    batch.backward()
    return _results(batch), bufs, batch


def _reference_run(dev, rot):
    if rot not in _BATCH_RESULTS:
        _BATCH_RESULTS[rot] = _run_set(dev, rot)[0]
    return _BATCH_RESULTS[rot]


# ------------------------------------------------------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("rot", ROTATIONS)
def test_parity(dev, rot):
    refs = [_ref(i, rot) for i in range(N)]                        # the condition holds for every tensor before any comparison
    got, bufs, batch = _run_set(dev, rot)
    _BATCH_RESULTS.setdefault(rot, got)
    worst = 0.0
    for i, b in enumerate(bufs):
        out, dP, ds, cnt = got[i]
        ref = refs[i]
        what = f"tensor {i} {SET[i]} {_format(i, rot)}"
        assert bits_equal(out, ref["out"]), f"{what}: out against the reference"
        assert bits_equal(dP, ref["dP"]), f"{what}: dP against the reference"
        assert np.array_equal(cnt, ref["clipped"]), f"{what}: counts against the reference"
        _same(got[i], _single(b), f"{what} against the single-tensor ops")
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.max(np.abs(ds.astype(np.float64) - ref["ds"]) / np.maximum(ref["terms"], 1e-300))))
        assert_within_terms(ds, ref["ds"], ref["terms"], f"{what}: ds against the reference")
    print(f"rotation {rot}: worst |ds - ref| / sum|terms| = {worst:.3e}")
    for b in bufs:                                                  # a second run of the same batch: the same bits
        b.reset()
    batch.forward()
    batch.backward()
    for i, r in enumerate(_results(batch)):
        _same(r, got[i], f"tensor {i}: second run of the batch")


def test_mask_only(dev):
    """grad_scale = NULL: dP and the counts as in the full call, and every ds buffer keeps its sentinel word."""
    want = _reference_run(dev, 1)
    bufs = [Buf(i, 1, dev) for i in range(N)]
    batch = Batch(bufs)
    batch.backward(mask_only=True)
    res = _results(batch)
    for i, b in enumerate(bufs):
        assert bits_equal(res[i][1], want[i][1]), f"tensor {i}: dP of the mask-only call"
        assert np.array_equal(res[i][3], want[i][3]), f"tensor {i}: counts of the mask-only call"
        assert b.untouched("ds", "out"), f"tensor {i}: the mask-only call wrote ds (or out)"


# ---------------------------------------------------------------------------------------------------------- 2 memory contract
def test_memory_contract(dev):
    """Every pointer of the batch is a region of one poisoned arena.  A full forward + backward fills every output and leaves the
    guard bands alone; the workspace is 0 bytes and ws = NULL is accepted; mask only writes no ds."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    rot = 2
    want = _reference_run(dev, rot)
    ar = Arena(dev)
    for i, (R, C, axis, gs) in enumerate(SET):
        P, s, dy = _inputs(i, rot)
        row = C * 4
        ar.add(f"P{i}", "in", data=P, row_bytes=row)
        ar.add(f"s{i}", "in", data=s)
        ar.add(f"dy{i}", "in", data=dy, row_bytes=row)
        ar.add(f"out{i}", "out", nbytes=P.nbytes, row_bytes=row)
        ar.add(f"dp{i}", "out", nbytes=P.nbytes, row_bytes=row)
        ar.add(f"ds{i}", "out", nbytes=s.nbytes)
    ar.build()
    arr = (_hip.GroupDesc * N)(*[_hip.GroupDesc(ar.ptr(f"P{i}"), ar.ptr(f"s{i}"), ar.ptr(f"out{i}"), ar.ptr(f"dp{i}"), ar.ptr(f"ds{i}"),
                                                SET[i][0], SET[i][1], SET[i][3], SET[i][2], 0, 0) for i in range(N)])
    fmts = (_hip.GroupMxFormat * N)(*[_hip.GroupMxFormat(X.FORMATS[_format(i, rot)[0]].id, X.SCALE_FORMATS.index(_format(i, rot)[1]))
                                      for i in range(N)])
    outs = [f"{n}{i}" for i in range(N) for n in ("out", "dp", "ds")]
    dys = (ctypes.c_void_p * N)(*[ar.ptr(f"dy{i}") for i in range(N)])
    ks = (ctypes.c_float * N)(*[_k(i) for i in range(N)])
    st = _hip.stream_ptr(dev)

    def run(mask_only=False):
        handle = ctypes.c_void_p()
        _hip.check(lib.lq_group_batch_create_mx(arr, fmts, N, ctypes.byref(handle)), "lq_group_batch_create_mx")
        try:
            assert lib.lq_group_batch_workspace_bytes(handle) == 0
            for name in outs:
                ar.fill(name, 0x7F)
            _hip.check(lib.lq_group_batch_forward(handle, st), "forward")
            _hip.check(lib.lq_group_batch_backward(handle, dys, None if mask_only else ks, None, 0, st), "backward")
            torch.cuda.synchronize(dev)
        finally:
            lib.lq_group_batch_destroy(handle)

    run()
    ar.check("mx group batch")                                     # every out, dp and ds filled; guards and inputs intact
    for i in range(N):
        for name, w in zip(("out", "dp", "ds"), want[i][:3]):
            assert bits_equal(ar.numpy(f"{name}{i}", np.float32).reshape(w.shape), w), f"tensor {i}: {name} of the arena run"
    run(mask_only=True)
    ar.check("mx group batch, mask only", written=[f"{n}{i}" for i in range(N) for n in ("out", "dp")])
    for i in range(N):
        assert bits_equal(ar.numpy(f"dp{i}", np.float32).reshape(want[i][1].shape), want[i][1]), f"tensor {i}: dP of the mask-only call"


# ---------------------------------------------------------------------------------------------------------------- 3 alignment
def test_alignment(dev):
    """Tensor 1 with every dense base 4 bytes off the 16-byte grid: the scalar column form, and the single-tensor ops' bits on the
    same buffers.  A misaligned dy for a tensor whose table entry is a float4 form: LQ_EALIGN before any launch."""
    rot = 3
    want = _reference_run(dev, rot)
    bufs = [Buf(0, rot, dev), Buf(1, rot, dev, offset=1), Buf(7, rot, dev)]
    for t in (bufs[1].P, bufs[1].out, bufs[1].dp, bufs[1].dy):
        assert t.data_ptr() % 16 == 4
    batch = Batch(bufs)
    batch.forward()
    batch.backward()
    res = _results(batch)
    for b, r in zip(bufs, res):
        _same(r, _single(b), f"tensor {b.i} (tensor 1 misaligned) against the single-tensor ops on these buffers")
    assert bits_equal(res[1][0], want[1][0]) and bits_equal(res[1][1], want[1][1]) and np.array_equal(res[1][3], want[1][3])
    ref = _ref(1, rot)
    assert_within_terms(res[1][2], ref["ds"], ref["terms"], "ds of the scalar form")
    bufs = [Buf(0, rot, dev), Buf(1, rot, dev), Buf(7, rot, dev)]
    batch = Batch(bufs)
    off = Buf._at(_inputs(1, rot)[2], dev, 1)
    assert off.data_ptr() % 16 == 4
    assert batch.backward_rc(dys=[bufs[0].dy, off, bufs[2].dy]) == EALIGN and b"tensor 1" in batch.lib.lq_last_error()
    torch.cuda.synchronize()
    assert all(b.untouched("ds", "dp", "out") for b in bufs), "a refused call launched"
    null = (ctypes.c_void_p * 3)(bufs[0].dy.data_ptr(), None, bufs[2].dy.data_ptr())
    ks = (ctypes.c_float * 3)(*[b.k for b in bufs])
    assert batch.lib.lq_group_batch_backward(batch.handle, null, ks, None, 0, batch._hip.stream_ptr(dev)) == EINVAL
    torch.cuda.synchronize()
    assert all(b.untouched("ds", "dp", "out") for b in bufs), "a refused call launched"


# --------------------------------------------------------------------------------------------------------------- 4 bad scales
def test_bad_scale_stays_in_its_group(dev):
    """One group of tensor 4 (E8M0 in every rotation) with a scale of 0, a negative, a subnormal, +Inf and NaN: its out and ds are
    NaN exactly where the reference's are, every other group and every other tensor keeps the clean run's bits."""
    rot = 0
    assert _format(4, rot)[1] == "e8m0"
    want = _reference_run(dev, rot)
    spoiled = np.zeros(_inputs(4, rot)[1].shape, bool)
    spoiled[5, 1] = True                                            # row 5, group 1 of tensor 4 (64, 576, 1, 128)
    elems = np.zeros(SET[4][:2], bool)
    elems[5, 128:256] = True
    for bad in (0.0, -2.0 ** -7, 2.0 ** -130, np.inf, np.nan):
        s4 = _inputs(4, rot)[1].copy()
        s4[5, 1] = np.float32(bad)
        bufs = [Buf(i, rot, dev, s=s4 if i == 4 else None) for i in range(N)]
        batch = Batch(bufs)
        batch.forward()
        batch.backward()
        res = _results(batch)
        for i in range(N):
            if i != 4:
                _same(res[i], want[i], f"tensor {i} next to a scale of {bad!r} in tensor 4")
        ref = _reference(4, rot, s=s4)
        assert np.array_equal(np.isnan(ref["out"]), elems) and np.array_equal(np.isnan(ref["ds"]), spoiled), "the reference itself"
        out, dP, ds, cnt = res[4]
        assert np.array_equal(np.isnan(out), np.isnan(ref["out"])), f"scale {bad!r}: out is NaN elsewhere than the reference's"
        assert np.array_equal(np.isnan(ds), np.isnan(ref["ds"])), f"scale {bad!r}: ds is NaN elsewhere than the reference's"
        assert bits_equal(dP, ref["dP"]) and np.array_equal(cnt, ref["clipped"]), f"scale {bad!r}: dP / counts against the reference"
        assert bits_equal(out[~elems], want[4][0][~elems]), f"scale {bad!r}: out of the other groups"
        assert bits_equal(ds[~spoiled], want[4][2][~spoiled]), f"scale {bad!r}: ds of the other groups"
        _same(res[4], _single(bufs[4]), f"scale {bad!r}: tensor 4 against the single-tensor ops")


# ------------------------------------------------------------------------------------------------------------------ 5 refusals
def test_refusals(dev):
    """Everything lq_group_batch_create_mx refuses returns its code before the first HIP call, and *out stays NULL."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    bufs = [Buf(i, 0, dev) for i in (0, 3, 6)]
    n = len(bufs)

    def call(descs=None, fmts="default", count=n):
        arr = (_hip.GroupDesc * max(count, n))(*((descs or [b.desc(_hip) for b in bufs]) * (max(count, n) // n + 1))[:max(count, n)])
        farr = None
        if fmts is not None:
            f = [(b.fid, b.sid) for b in bufs] if fmts == "default" else fmts
            farr = (_hip.GroupMxFormat * max(count, n))(*([_hip.GroupMxFormat(*x) for x in f] * (max(count, n) // n + 1))[:max(count, n)])
        handle = ctypes.c_void_p(0xDEAD0)                           # the call itself must reset it
        rc = lib.lq_group_batch_create_mx(arr, farr, count, ctypes.byref(handle))
        assert handle.value is None, "*out is not NULL after a refused create"
        return rc

    def desc(j, **kw):
        d = bufs[j].desc(_hip)
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    assert call(fmts=None) == EINVAL and b"fmts" in lib.lq_last_error()
    for bad in ((5, 0), (-1, 0), (0, 2)):
        assert call(fmts=[(bufs[0].fid, bufs[0].sid), bad, (bufs[2].fid, bufs[2].sid)]) == EINVAL and b"tensor 1" in lib.lq_last_error()
    assert call(count=0) == EINVAL
    assert call(count=257) == EINVAL
    for field in ("P", "s", "out", "dp"):
        assert call(descs=[desc(0), desc(1, **{field: None}), desc(2)]) == EINVAL and b"tensor 1" in lib.lq_last_error()
    assert call(descs=[desc(0), desc(1), desc(2, axis=2)]) == EINVAL and b"tensor 2" in lib.lq_last_error()
    assert call(descs=[desc(0), desc(1, gs=0), desc(2)]) == EINVAL and b"tensor 1" in lib.lq_last_error()
    assert lib.lq_group_batch_create_mx((_hip.GroupDesc * n)(*[b.desc(_hip) for b in bufs]),
                                        (_hip.GroupMxFormat * n)(*[_hip.GroupMxFormat(b.fid, b.sid) for b in bufs]), n, None) == EINVAL


# -------------------------------------------------------------------------------------------------------------------- 6 capture
def test_capture_and_replay(dev):
    """Forward + backward recorded on one stream and replayed twice: the eager bits, both times."""
    rot = 4
    eager = _reference_run(dev, rot)
    bufs = [Buf(i, rot, dev) for i in range(N)]
    batch = Batch(bufs)
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


# --------------------------------------------------------------------------------------------------------------------- 7 layers
MIXED = (("fp4_e2m1", "e8m0"), ("fp8_e4m3", "fp32"))               # the formats of the two layers of the MNIST model


def _mixed_model(dev, seed=3):
    """The MNIST model with two element formats: dense_1 fp4_e2m1 under E8M0 scales, dense_2 switched to fp8_e4m3 under fp32 scales
    (make_mx).  Kernel scales from the OCP rule, then shaken down so that elements saturate; a bias runs from 2 / n to twice its
    format's max (in units of its power-of-two scale) with alternating signs: half of it saturates."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    model = lq.build_model("mnist", seed=seed, mode="ste", value=0.0, device=dev, element_format=MIXED[0][0], scale_format=MIXED[0][1])
    layers = lq.custom_layers_of(model)
    assert len(layers) == len(MIXED)
    layers[1].make_mx(*MIXED[1])
    lq.init_scales(model, "mx")
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for layer, (name, _) in zip(layers, MIXED):
            nested = layer.weight_nested()
            nested.scale.mul_(_t(rng.uniform(0.4, 0.8, tuple(nested.scale.shape)).astype(np.float32), dev))
            n = layer.b.numel()
            ramp = (np.arange(n) + 1.0) / n * 2.0 * X.FORMATS[name].max * 2.0 ** -7 * np.where(np.arange(n) % 2, -1.0, 1.0)
            layer.b.copy_(_t(ramp.astype(np.float32).reshape(tuple(layer.b.shape)), dev))
            layer.nested_q_b_layer.scale.fill_(2.0 ** -7)
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
    """FakeQuantBatch(group_batch=True, mx=True) over layers of two formats against the per-tensor layers on injected upstream
    gradients: out, P.grad and scale.grad of kernels AND biases bit for bit.  Then a preset contiguous scale.grad (a bucket view) is
    written in place."""
    import learned_quantization_amd as lq
    from learned_quantization_amd.batch import BatchedScaleAdam, FakeQuantBatch
    model = _mixed_model(dev)
    layers = lq.custom_layers_of(model)
    assert [(l.element_format, l.scale_format) for l in layers] == list(MIXED)
    g = torch.Generator().manual_seed(17)
    cs = [(torch.randn(tuple(l.W.shape), generator=g).to(dev), torch.randn(tuple(l.b.shape), generator=g).to(dev)) for l in layers]

    def tensors():
        out = []
        for l in layers:
            out += [(l.W, l.weight_nested().scale), (l.b, l.nested_q_b_layer.scale)]
        return out

    def clear():
        for p, s in tensors():
            p.grad = s.grad = None

    total, outs = _linear_objective(layers, cs)                    # the per-tensor path
    total.backward()
    want = [(w.detach().clone(), p.grad.detach().clone(), s.grad.detach().clone()) for w, (p, s) in zip(outs, tensors())]
    clear()
    batch = FakeQuantBatch(model, autograd=autograd, group_batch=True, mx=True)
    assert batch.mx and batch.ste and [e.nested.element_format for e in batch.entries] == [MIXED[0][0]] * 2 + [MIXED[1][0]] * 2
    opt = BatchedScaleAdam(batch)
    assert len(opt.param_groups[0]["params"]) == 2 * len(layers)

    def run():
        batch.quantize_all()
        total, outs = _linear_objective(layers, cs)
        total.backward()
        if not autograd:
            batch.finish_backward()
        return outs

    outs = run()
    for j, ((p, s), w, (wo, wp, ws)) in enumerate(zip(tensors(), outs, want)):
        assert torch.equal(w.detach().view(torch.int32), wo.view(torch.int32)), f"tensor {j}: out"
        assert torch.equal(p.grad.view(torch.int32), wp.view(torch.int32)), f"tensor {j}: P.grad"
        assert bool((p.grad == 0).any()) and bool((p.grad != 0).any()), f"tensor {j}: the mask is not at work"
        assert torch.equal(s.grad.view(torch.int32), ws.view(torch.int32)), f"tensor {j}: scale.grad against the per-tensor layer"
        assert not bool(torch.isnan(s.grad).any()) and bool((s.grad != 0).any()), f"tensor {j}: scale.grad is NaN or all zero"
    counts = batch.clip_counts()
    for j, ((p, _), c) in enumerate(zip(tensors(), counts)):
        assert tuple(c.shape) == tuple(tensors()[j][1].shape) and int(c.sum()) == int((p.grad == 0).sum()), f"tensor {j}: saturation counts"
    opt.zero_grad()
    assert all(s.grad is None for _, s in tensors())
    # a bucket view as the scale's gradient: the batch built over it writes ds there
    clear()
    scale = layers[0].weight_nested().scale
    flat = torch.zeros(scale.numel() + 8, device=dev)
    view = flat[4:4 + scale.numel()].view_as(scale)
    scale.grad = view
    batch = FakeQuantBatch(model, autograd=autograd, group_batch=True, mx=True)
    assert batch._external_grads and batch.entries[0].ds is view
    run()
    assert scale.grad is view
    assert torch.equal(flat[4:4 + view.numel()].view_as(view).view(torch.int32), want[0][2].view(torch.int32))
    assert bool((flat[:4] == 0).all()) and bool((flat[-4:] == 0).all())


# -------------------------------------------------------------------------------------------------------------------- 8 trainer
def _linear_trainer(dev, tmp, steps, **kw):
    from _linear_task import LinearTaskTrainer, make_coefficients
    tr = LinearTaskTrainer(config="cifar", mode="ste", value=0.0, device=dev, log_dir=str(tmp), seed=3, element_format="fp4_e2m1",
                           scale_init="mx", lr=1e-3, **kw)
    rng = np.random.default_rng(3)
    with torch.no_grad():                                           # scales off their powers of two: elements saturate
        g = torch.Generator().manual_seed(11)
        for layer in tr.custom_layers:
            for _, nested, param in layer.scale_pairs():
                if param.dim() > 1:
                    nested.scale.mul_(_t(rng.uniform(0.4, 0.8, tuple(nested.scale.shape)).astype(np.float32), dev))
                else:                                               # biases are created at zero: give them something to saturate
                    param.copy_((torch.randn(param.shape, generator=g) * 0.05).to(dev))
                    nested.scale.fill_(0.05 / 6.0)
    tr.coefficients = make_coefficients(tr, steps, lo=-3.0, hi=-1.0)
    return tr


BATCHED = dict(batched=True, group_batch=True, mx_batch=True)


def test_trainer_step_matches_the_per_tensor_path(dev, tmp_path):
    """Step 1 of the MX batch against the per-tensor path on injected gradients: P.grad and ds of every tensor, kernels and biases,
    and the scales after the step, bit for bit."""
    import learned_quantization_amd as lq
    plain = _linear_trainer(dev, tmp_path / "a", 1)
    lq.reset_layer_names()
    batched = _linear_trainer(dev, tmp_path / "b", 1, **BATCHED)
    assert batched.batch.mx and plain.batch is None
    x = torch.zeros(2, 3, 32, 32, device=dev)
    y = torch.zeros(2, dtype=torch.long, device=dev)
    la, lb = plain.step(x, y), batched.step(x, y)
    assert torch.equal(la, lb)
    seen = 0
    for la_, lb_ in zip(plain.custom_layers, batched.custom_layers):
        for (_, na, pa), (_, nb, pb) in zip(la_.scale_pairs(), lb_.scale_pairs()):
            what = f"{la_.name} {tuple(pa.shape)}"
            assert torch.equal(pa.grad.view(torch.int32), pb.grad.view(torch.int32)), f"{what}: P.grad"
            assert torch.equal(na.scale.grad.view(torch.int32), nb.scale.grad.view(torch.int32)), f"{what}: ds"
            assert not bool(torch.isnan(nb.scale.grad).any()) and bool((nb.scale.grad != 0).any()), f"{what}: ds is NaN or all zero"
            assert torch.equal(na.scale.detach().view(torch.int32), nb.scale.detach().view(torch.int32)), f"{what}: the scales after the step"
            seen += 1
    assert seen == len(batched.batch.entries)


def test_trainer_eager_and_graphed(dev, tmp_path):
    """The MX batch eager and graph=True from the same state on a fixed linear task: three steps agree bit for bit, every parameter
    and scale included; the scales move."""
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
                       element_format="fp4_e2m1", scale_init="cover", lr=1e-3, **BATCHED)
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
        scale = layer.weight_nested().scale
        assert scale.grad is not None
        assert int((scale.detach() != start[names[id(scale)]]).sum()) > 0, layer.name


def test_one_rank_ddp_mode_a_equals_the_plain_step(dev, tmp_path):
    """Data-parallel mode A on a one-rank gloo group: ds is written into the bucket views the batch found at construction, the
    exchange averages over one rank, and two steps leave every parameter and scale where the plain batched steps do."""
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
        assert tr.dp is not None and tr.batch.mx and tr.batch._external_grads
        views = {v.data_ptr() for v in tr.dp.bucket.views}
        for e in tr.batch.entries:
            assert e.ds.data_ptr() in views, "a gradient outside the bucket"
    finally:
        dist.destroy_process_group()
    for n in plain:
        assert torch.equal(plain[n], dp[n]), n


def test_the_cli_line_runs(dev):
    from learned_quantization_amd import train
    train.main(["--config", "mnist", "--mode", "ste", "--element-format", "fp4_e2m1", "--scale-init", "cover", "--batch", "32",
                "--batched", "--group-batch", "--mx-batch", "--steps", "2", "--warmup", "1"])


# ------------------------------------------------------------------------------------------------------------------ 9 refusals
def test_refusals_on_the_device(dev, tmp_path):
    """What needs a built model or a built batch to be refused: the fused Adam step and data-parallel mode B over the MX batch."""
    import learned_quantization_amd as lq
    from learned_quantization_amd.batch import BatchedScaleAdam, FakeQuantBatch
    from learned_quantization_amd.train import Trainer
    model = _mixed_model(dev)
    batch = FakeQuantBatch(model, group_batch=True, mx=True, autograd=False)
    with pytest.raises(ValueError, match="fused=False"):
        BatchedScaleAdam(batch, fused=True)
    with pytest.raises(ValueError, match="mode B"):
        batch.scale_grads_from_param_grads()
    batch.defer_scale_grads = True                                 # what DataParallel(mode="B").attach_batch sets
    batch.quantize_all()
    with pytest.raises(ValueError, match="mode B"):
        batch.finish_backward()
    with pytest.raises(ValueError, match="mode B"):
        batch.penalty_values("maxbin")
    with pytest.raises(ValueError, match="mode 'B'|mode B"):
        lq.DataParallel(model, mode="B")
    base = dict(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path), element_format="fp4_e2m1")
    with pytest.raises(ValueError, match="ddp_mode 'B'"):
        Trainer(ddp_mode="B", **BATCHED, **base)
