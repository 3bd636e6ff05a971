"""GPU tests of the group batch (include/lq_hip.h: lq_group_batch_*): group-wise tensors of a model in ONE forward and ONE backward
launch, from the C ABI up to FakeQuantBatch(group_batch=True) and the Trainer.

The reference is tests/_group_reference.py::group_reference.  The ten-tensor set (R, C, axis, gs), inputs from
``make_case(100 + i, ...)``, tensor i with range [(-8, 7), (0, 15), (-3, 5)][i % 3] and grad_scale 0.37 * (i + 1):

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

Coverage: k_group_batch has four instantiations, <RNE, BWD> in {floor, nearest} x {forward, backward}; each holds the four forms
as block-uniform branches.  ``test_parity`` launches all four instantiations (its two roundings, forward and backward), and in each
of them tensors 1, 8 run the float4 column form, 0, 2 the scalar column form, 4, 5, 7, 9 the float4 row form and 3, 6 the scalar
row form.  ``test_alignment`` moves tensor 1 to the scalar column form; ``test_layers`` and the trainer tests run the floor pair
from Python.

The bar: out, dP and the clip counts equal the reference AND the single-tensor ops bit for bit; ds equals the single-tensor op's
bit for bit (the batch runs the same device function on the same unit of work) and is held to tests/_bounds.py::assert_within_terms
(1e-5 * sum|terms|) against the reference.  Condition, asserted on the reference before any comparison: every tensor has
0 < clipped < numel under its range (31-60 % of the elements clip with these seeds).

Biases (``test_layers``, ``test_trainer_step_matches_the_per_tensor_path``): the per-tensor path of a bias is the one-axis clipped
op (lq_fq_backward_clip_r), a different traversal of the same sum -- out and P.grad are compared bit for bit, ds within the bound."""
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
from _group_reference import group_reference, make_case                                   # noqa: E402

pytestmark = pytest.mark.gpu

SET = [(37, 5, 0, 8), (256, 260, 0, 32), (96, 130, 0, 96), (7, 27, 1, 8), (64, 576, 1, 128), (33, 4100, 1, 128), (1, 10, 1, 10),
       (1, 512, 1, 512), (300, 64, 0, 1), (40, 64, 1, 4)]
RANGES = [(-8, 7), (0, 15), (-3, 5)]
ROUNDINGS = ("floor", "nearest")
EINVAL, EALIGN = -1, -4
SENTINEL = 0x7F7F7F7F


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _k(i):
    return float(np.float32(0.37 * (i + 1)))


_INPUTS, _REFS = {}, {}


def _inputs(i):
    if i not in _INPUTS:
        _INPUTS[i] = make_case(100 + i, *SET[i])
    return _INPUTS[i]


def _ref(i, rounding):
    """Reference of tensor i, computed once and shared (never modified); the condition is asserted here."""
    if (i, rounding) not in _REFS:
        P, s, dy = _inputs(i)
        R, C, axis, gs = SET[i]
        ref = group_reference(P, s, dy, *RANGES[i % 3], axis, gs, k=_k(i), rounding=rounding)
        clipped = int(ref["clipped"].sum())
        assert 0 < clipped < P.size, f"tensor {i} {rounding}: {clipped} of {P.size} clipped"
        _REFS[(i, rounding)] = ref
    return _REFS[(i, rounding)]


class Buf:
    """Device buffers of one tensor: inputs uploaded, outputs preset to the sentinel word."""

    def __init__(self, i, dev, P=None, dy=None, offset=0):
        Pn, sn, dyn = _inputs(i)
        Pn, dyn = (Pn if P is None else P), (dyn if dy is None else dy)
        self.i, self.geom, self.range = i, SET[i], RANGES[i % 3]
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

    def desc(self, _hip, ds=True):
        R, C, axis, gs = self.geom
        return _hip.GroupDesc(self.P.data_ptr(), self.s.data_ptr(), self.out.data_ptr(), self.dp.data_ptr(),
                              self.ds.data_ptr() if ds else None, R, C, gs, axis, *self.range)

    def untouched(self, *names):
        return all(bool((getattr(self, n).view(torch.int32) == SENTINEL).all()) for n in names)


class Batch:
    def __init__(self, bufs, rounding="floor", ds=True):
        from learned_quantization_amd import _hip
        self._hip, self.lib, self.bufs = _hip, _hip.load(), bufs
        n = len(bufs)
        arr = (_hip.GroupDesc * n)(*[b.desc(_hip, ds) for b in bufs])
        self.handle = ctypes.c_void_p()
        _hip.check(self.lib.lq_group_batch_create(arr, n, ROUNDINGS.index(rounding), ctypes.byref(self.handle)), "lq_group_batch_create")
        self.need = self.lib.lq_group_batch_workspace_bytes(self.handle)
        self.ws = torch.empty(max(self.need, 16), dtype=torch.uint8, device=bufs[0].P.device)
        self.dev = bufs[0].P.device

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.lq_group_batch_destroy(self.handle)
            self.handle = None

    def forward(self):
        self._hip.check(self.lib.lq_group_batch_forward(self.handle, self._hip.stream_ptr(self.dev)), "lq_group_batch_forward")

    def backward_rc(self, dys=None, mask_only=False, ks=None):
        n = len(self.bufs)
        ptrs = (ctypes.c_void_p * n)(*[(b.dy if dys is None else dys[j]).data_ptr() for j, b in enumerate(self.bufs)])
        gs = None if mask_only else (ctypes.c_float * n)(*[_k(b.i) for b in self.bufs] if ks is None else ks)
        return self.lib.lq_group_batch_backward(self.handle, ptrs, gs, self.ws.data_ptr() if self.need else None, self.need,
                                                self._hip.stream_ptr(self.dev))

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


def _single(b, rounding, dy=None, k=None):
    """The single-tensor ops on the same P, s, dy: (out, dP, ds, counts) as NumPy arrays."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = b.geom
    rnd = ROUNDINGS.index(rounding)
    st = _hip.stream_ptr(b.P.device)
    out, dP = torch.empty_like(b.P), torch.empty_like(b.P)
    ds, cnt = torch.empty_like(b.s), torch.empty(b.s.shape, dtype=torch.int32, device=b.P.device)
    dy = b.dy if dy is None else dy
    _hip.check(lib.lq_fq_forward_group(b.P.data_ptr(), b.s.data_ptr(), out.data_ptr(), None, 0, *b.range, rnd, R, C, axis, gs, st), "fwd")
    _hip.check(lib.lq_fq_backward_group(b.P.data_ptr(), b.s.data_ptr(), dy.data_ptr(), *b.range, rnd, _k(b.i) if k is None else k,
                                        dP.data_ptr(), ds.data_ptr(), cnt.data_ptr(), None, 0, R, C, axis, gs, st), "bwd")
    return out.cpu().numpy(), dP.cpu().numpy(), ds.cpu().numpy(), cnt.cpu().numpy().view(np.uint32).astype(np.int64)


def _results(batch):
    torch.cuda.synchronize()
    return [(b.out.cpu().numpy(), b.dp.cpu().numpy(), b.ds.cpu().numpy(), _read_counts(batch, j)) for j, b in enumerate(batch.bufs)]


def _same(a, b, what):
    for name, x, y in zip(("out", "dP", "ds"), a[:3], b[:3]):
        assert bits_equal(x, y), f"{what}: {name}"
    assert np.array_equal(a[3], b[3]), f"{what}: counts"


_BATCH_RESULTS = {}


def _run_set(dev, rounding, order=None):
    """The ten tensors through the batch in descriptor order ``order``; per-tensor results keyed by tensor index."""
    order = list(range(len(SET))) if order is None else order
    bufs = [Buf(i, dev) for i in order]
    batch = Batch(bufs, rounding)
    assert batch.need == 0
    batch.forward()
    batch.backward()
    return {b.i: r for b, r in zip(bufs, _results(batch))}, bufs


def _reference_run(dev, rounding):
    if rounding not in _BATCH_RESULTS:
        _BATCH_RESULTS[rounding] = _run_set(dev, rounding)[0]
    return _BATCH_RESULTS[rounding]


# ------------------------------------------------------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_parity(dev, rounding):
    refs = [_ref(i, rounding) for i in range(len(SET))]            # the condition holds for every tensor before any comparison
    got, bufs = _run_set(dev, rounding)
    _BATCH_RESULTS.setdefault(rounding, got)
    worst = 0.0
    for i, b in enumerate(bufs):
        out, dP, ds, cnt = got[i]
        ref = refs[i]
        what = f"tensor {i} {SET[i]} {rounding}"
        assert bits_equal(out, ref["out"]), f"{what}: out against the reference"
        assert bits_equal(dP, ref["dP"]), f"{what}: dP against the reference"
        assert np.array_equal(cnt, ref["clipped"]), f"{what}: counts against the reference"
        _same(got[i], _single(b, rounding), f"{what} against the single-tensor ops")
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.max(np.abs(ds.astype(np.float64) - ref["ds"]) / np.maximum(ref["terms"], 1e-300))))
        assert_within_terms(ds, ref["ds"], ref["terms"], f"{what}: ds against the reference")
    print(f"{rounding}: worst |ds - ref| / sum|terms| = {worst:.3e}")


# ------------------------------------------------------------------------------------------------------ 2 order independence
@pytest.mark.parametrize("order", [list(range(9, -1, -1)), [3, 8, 0, 5, 9, 1, 7, 2, 6, 4]], ids=["reversed", "shuffled"])
def test_order_independence(dev, order):
    want = _reference_run(dev, "floor")
    got, _ = _run_set(dev, "floor", order)
    for i in range(len(SET)):
        _same(got[i], want[i], f"tensor {i} in order {order}")


# ------------------------------------------------------------------------------------------------- 3 mask only and ds == NULL
def test_mask_only_and_missing_ds(dev):
    want = _reference_run(dev, "floor")
    bufs = [Buf(i, dev) for i in range(len(SET))]
    batch = Batch(bufs, "floor")
    batch.backward(mask_only=True)
    for j, (b, r) in enumerate(zip(bufs, _results(batch))):
        assert b.untouched("ds", "out"), f"tensor {j}: mask only wrote ds or out"
        assert bits_equal(r[1], want[j][1]) and np.array_equal(r[3], want[j][3]), f"tensor {j}: dP / counts of the mask-only call"
    bufs = [Buf(i, dev) for i in range(len(SET))]
    batch = Batch(bufs, "floor", ds=False)
    assert batch.backward_rc() == EINVAL and b"no ds buffer" in batch.lib.lq_last_error()
    torch.cuda.synchronize()
    assert all(b.untouched("ds", "dp", "out") for b in bufs), "a refused call launched"
    batch.backward(mask_only=True)                                 # the same batch serves the mask alone
    for j, r in enumerate(_results(batch)):
        assert bits_equal(r[1], want[j][1]) and np.array_equal(r[3], want[j][3])


# ---------------------------------------------------------------------------------------------------------------- 4 alignment
def test_alignment(dev):
    """Tensor 1 with every dense base 4 bytes off the 16-byte grid: the scalar column form, and the single-tensor ops' bits on the
    same buffers.  A misaligned dy for a tensor whose table entry is a float4 form: LQ_EALIGN before any launch."""
    want = _reference_run(dev, "floor")
    bufs = [Buf(0, dev), Buf(1, dev, offset=1), Buf(4, dev)]
    assert bufs[1].P.data_ptr() % 16 == 4 and bufs[1].dp.data_ptr() % 16 == 4 and bufs[1].out.data_ptr() % 16 == 4
    batch = Batch(bufs, "floor")
    batch.forward()
    batch.backward()
    res = _results(batch)
    for b, r in zip(bufs, res):
        _same(r, _single(b, "floor"), f"tensor {b.i} (tensor 1 misaligned) against the single-tensor ops on these buffers")
    assert bits_equal(res[1][0], want[1][0]) and bits_equal(res[1][1], want[1][1]) and np.array_equal(res[1][3], want[1][3])
    assert_within_terms(res[1][2], _ref(1, "floor")["ds"], _ref(1, "floor")["terms"], "ds of the scalar form")
    bufs = [Buf(0, dev), Buf(1, dev), Buf(4, dev)]
    batch = Batch(bufs, "floor")
    off = Buf._at(_inputs(1)[2], dev, 1)
    assert off.data_ptr() % 16 == 4
    assert batch.backward_rc(dys=[bufs[0].dy, off, bufs[2].dy]) == EALIGN and b"tensor 1" in batch.lib.lq_last_error()
    torch.cuda.synchronize()
    assert all(b.untouched("ds", "dp", "out") for b in bufs), "a refused call launched"
    n = len(bufs)
    ptrs = (ctypes.c_void_p * n)(bufs[0].dy.data_ptr(), None, bufs[2].dy.data_ptr())
    ks = (ctypes.c_float * n)(1.0, 1.0, 1.0)
    assert batch.lib.lq_group_batch_backward(batch.handle, ptrs, ks, None, 0, None) == EINVAL      # a NULL entry


# ---------------------------------------------------------------------------------------------------------- 5 memory contract
def test_memory_contract(dev):
    from learned_quantization_amd import _hip
    lib = _hip.load()
    want = _reference_run(dev, "floor")
    ar = Arena(dev)
    for i, (R, C, axis, gs) in enumerate(SET):
        P, s, dy = _inputs(i)
        row = C * 4
        ar.add(f"P{i}", "in", data=P, row_bytes=row)
        ar.add(f"s{i}", "in", data=s)
        ar.add(f"dy{i}", "in", data=dy, row_bytes=row)
        ar.add(f"out{i}", "out", nbytes=P.nbytes, row_bytes=row)
        ar.add(f"dp{i}", "out", nbytes=P.nbytes, row_bytes=row)
        ar.add(f"ds{i}", "out", nbytes=s.nbytes)
    n = len(SET)
    # the workspace region is exactly lq_group_batch_workspace_bytes long; a size of 0 leaves nothing the call may touch, so the
    # region that stands in for it (16 bytes, the pointer the call receives) must come back as it was prefilled
    ar.add("ws", "ws", nbytes=16)
    ar.build()
    arr = (_hip.GroupDesc * n)(*[_hip.GroupDesc(ar.ptr(f"P{i}"), ar.ptr(f"s{i}"), ar.ptr(f"out{i}"), ar.ptr(f"dp{i}"), ar.ptr(f"ds{i}"),
                                                SET[i][0], SET[i][1], SET[i][3], SET[i][2], *RANGES[i % 3]) for i in range(n)])
    handle = ctypes.c_void_p()
    _hip.check(lib.lq_group_batch_create(arr, n, 0, ctypes.byref(handle)), "lq_group_batch_create")
    try:
        need = lib.lq_group_batch_workspace_bytes(handle)
        assert need <= 16
        dys = (ctypes.c_void_p * n)(*[ar.ptr(f"dy{i}") for i in range(n)])
        ks = (ctypes.c_float * n)(*[_k(i) for i in range(n)])
        runs = []
        for fill in (0x00, 0xFF):
            ar.fill("ws", fill)
            for i in range(n):
                for name in (f"out{i}", f"dp{i}", f"ds{i}"):
                    ar.fill(name, 0x7F)
            _hip.check(lib.lq_group_batch_forward(handle, _hip.stream_ptr(dev)), "forward")
            _hip.check(lib.lq_group_batch_backward(handle, dys, ks, ar.ptr("ws"), need, _hip.stream_ptr(dev)), "backward")
            torch.cuda.synchronize(dev)
            ar.check(f"group batch, workspace prefill {fill:#x}")
            assert bool((ar.bytes("ws")[need:] == fill).all()), "bytes behind the stated workspace size were written"
            runs.append([(ar.numpy(f"out{i}", np.float32), ar.numpy(f"dp{i}", np.float32), ar.numpy(f"ds{i}", np.float32)) for i in range(n)])
        for i in range(n):
            for a, b, w in zip(runs[0][i], runs[1][i], want[i][:3]):
                assert bits_equal(a, b), f"tensor {i}: the result depends on the workspace prefill"
                assert bits_equal(a.reshape(w.shape), w), f"tensor {i}: the arena run differs from the plain run"
    finally:
        lib.lq_group_batch_destroy(handle)


# ------------------------------------------------------------------------------------------------------------------ 6 NaN / Inf
def test_nan_stays_in_its_group(dev):
    want = _reference_run(dev, "floor")
    P4 = _inputs(4)[0].copy()
    P4[5, 130] = np.nan                                             # row 5, group 1 of tensor 4 (64, 576, 1, 128)
    bufs = [Buf(i, dev, P=P4 if i == 4 else None) for i in range(len(SET))]
    batch = Batch(bufs, "floor")
    batch.forward()
    batch.backward()
    res = _results(batch)
    for i in range(len(SET)):
        if i != 4:
            _same(res[i], want[i], f"tensor {i} next to a NaN in tensor 4")
    ds = res[4][2]
    spoiled = np.zeros(ds.shape, bool)
    spoiled[5, 1] = True
    assert np.array_equal(np.isnan(ds), spoiled)
    assert bits_equal(ds[~spoiled], want[4][2][~spoiled])
    ref = group_reference(P4, _inputs(4)[1], _inputs(4)[2], *RANGES[4 % 3], 1, 128, k=_k(4))
    assert bits_equal(res[4][0], ref["out"]) and bits_equal(res[4][1], ref["dP"]) and np.array_equal(res[4][3], ref["clipped"])


# -------------------------------------------------------------------------------------------------------------------- 7 capture
def test_capture_and_replay(dev):
    """Forward + backward captured into one graph; P and dy rewritten in place; the replay equals the eager batch on the new data."""
    bufs = [Buf(i, dev) for i in range(len(SET))]
    batch = Batch(bufs, "nearest")
    batch.forward()
    batch.backward()                                                # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch.forward()
        batch.backward()
    for b in bufs:
        # new data under the same scales: the old P turned around both axes, dy of another seed
        b.P.copy_(_t(_inputs(b.i)[0][::-1, ::-1].copy(), dev))
        b.dy.copy_(_t(make_case(500 + b.i, *SET[b.i])[2], dev))
        for t in (b.out, b.dp, b.ds):
            t.view(torch.int32).fill_(SENTINEL)
    g.replay()
    replayed = _results(batch)
    for b in bufs:
        for t in (b.out, b.dp, b.ds):
            t.view(torch.int32).fill_(SENTINEL)
    batch.forward()
    batch.backward()
    eager = _results(batch)
    first = _reference_run(dev, "nearest")
    for i, (a, e) in enumerate(zip(replayed, eager)):
        _same(a, e, f"tensor {i}: replay against the eager batch")
        assert not bits_equal(a[0], first[i][0]), f"tensor {i}: the replay did not see the new P"


# --------------------------------------------------------------------------------------------------------------------- 8 layers
def _build_layers(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    kw = dict(orientation="groupwise", device=dev, scale_gradient="ste", grad_scale=0.37, bits=4)
    dense = lq.CustomDenseLayer(units=130, group_size=64, initializer=lq.RandomNormal(seed=5), input_shape=257, **kw)
    conv = lq.CustomConv2DLayer(filters=32, group_size=128, initializer=lq.RandomNormal(seed=6), input_shape=16, **kw)
    nobias = lq.CustomConv2DLayerNoBias(filters=8, kernel_size=(7, 7), group_size=8, initializer=lq.RandomNormal(seed=7), input_shape=3, **kw)
    layers = torch.nn.ModuleList([dense, conv, nobias])
    data = []
    with torch.no_grad():
        P, s, dy = make_case(801, 257, 130, 0, 64)
        dense.W.copy_(_t(P, dev)), dense.nested_q_w_layer.scale.copy_(_t(s, dev))
        data.append((P, s, dy, (257, 130, 0, 64)))
        for seed, layer, (co, ci, kh, gs) in ((802, conv, (32, 16, 3, 128)), (803, nobias, (8, 3, 7, 8))):
            C = ci * kh * kh
            P, s, dy = make_case(seed, co, C, 1, gs)
            layer.kernel.data.permute(3, 2, 0, 1).copy_(_t(P.reshape(co, ci, kh, kh), dev))
            layer.nested_q_k_layer.scale.copy_(_t(s, dev))
            data.append((P, s, dy, (co, C, 1, gs)))
        biases = []
        for seed, layer in ((804, dense), (805, conv)):
            n = layer.b.numel()
            P, s, dy = make_case(seed, 1, n, 1, n)
            layer.b.copy_(_t(P.reshape(n), dev)), layer.nested_q_b_layer.scale.copy_(_t(s.reshape(1), dev))
            biases.append((P, s, dy, (1, n, 1, n)))
    return layers, data, biases


def _upstream(layers, data, biases, dev):
    """Coefficients in the shape of what each layer hands out: (kernel, bias | None) per layer."""
    dense, conv, nobias = layers
    return [(_t(data[0][2], dev), _t(biases[0][2].reshape(-1), dev)),
            (_t(data[1][2].reshape(32, 16, 3, 3), dev), _t(biases[1][2].reshape(-1), dev)),
            (_t(data[2][2].reshape(8, 3, 7, 7), dev), None)]


def _objective(layers, cs):
    total, outs = None, []
    for layer, (ck, cb) in zip(layers, cs):
        w, qb = layer.quantized_parameters()
        t = (w * ck).sum()
        outs.append(w)
        if qb is not None:
            t = t + (qb * cb).sum()
            outs.append(qb)
        total = t if total is None else total + t
    return total, outs


def _tensors_of(layers):
    dense, conv, nobias = layers
    return [(dense.W, dense.nested_q_w_layer.scale, True), (dense.b, dense.nested_q_b_layer.scale, False),
            (conv.kernel, conv.nested_q_k_layer.scale, True), (conv.b, conv.nested_q_b_layer.scale, False),
            (nobias.kernel, nobias.nested_q_k_layer.scale, True)]


@pytest.mark.parametrize("autograd", [True, False], ids=["autograd", "leaves"])
def test_layers(dev, autograd):
    """FakeQuantBatch(group_batch=True) against the per-tensor layers on injected upstream gradients.  Kernels: out, P.grad, ds and
    the counts bit for bit.  Biases: out and P.grad bit for bit, ds within the bound -- their per-tensor path is the one-axis
    clipped op, a different traversal of the same sum."""
    import learned_quantization_amd as lq
    from learned_quantization_amd.batch import FakeQuantBatch
    layers, data, biases = _build_layers(dev)
    cs = _upstream(layers, data, biases, dev)
    total, outs = _objective(layers, cs)                            # the per-tensor path
    total.backward()
    want = [(o.detach().clone(), p.grad.detach().clone(), s.grad.detach().clone()) for o, (p, s, _) in zip(outs, _tensors_of(layers))]
    # the per-tensor layers do not hand out their counts: the per-tensor op on the same parameter, scale and upstream gradient
    # (a conv kernel's arrives OIHW-shaped; the parameter's logical shape is HWIO over the same memory)
    want_counts = [lq.fq_backward_group(p.data, s.data, ck if p.dim() == 2 else ck.permute(2, 3, 1, 0), -8, 7, gs, want_clipped=True)[2]
                   if gs else None
                   for (p, s, _), gs, ck in zip(_tensors_of(layers), (64, None, 128, None, 8), (cs[0][0], None, cs[1][0], None, cs[2][0]))]
    for p, s, _ in _tensors_of(layers):
        p.grad = s.grad = None
    batch = FakeQuantBatch(layers, autograd=autograd, group_batch=True)
    assert [e.desc for e in batch.entries] == [(257, 130, 0, 64), (1, 130, 1, 130), (32, 144, 1, 128), (1, 32, 1, 32), (8, 147, 1, 8)]
    batch.quantize_all()
    total, outs = _objective(layers, cs)
    total.backward()
    if not autograd:
        batch.finish_backward()
    counts = batch.clip_counts()
    refs = [data[0], biases[0], data[1], biases[1], data[2]]
    for j, ((p, s, is_kernel), o, (wo, wp, ws)) in enumerate(zip(_tensors_of(layers), outs, want)):
        assert torch.equal(o.detach(), wo), f"tensor {j}: out"
        assert torch.equal(p.grad, wp), f"tensor {j}: P.grad"
        assert bool((p.grad == 0).any()) and bool((p.grad != 0).any()), f"tensor {j}: the mask is not at work"
        P, sc, dy, (R, C, axis, gs) = refs[j]
        ref = group_reference(P, sc, dy, -8, 7, axis, gs, k=0.37)
        assert 0 < int(ref["clipped"].sum()) < P.size
        assert np.array_equal(counts[j].cpu().numpy().view(np.uint32).astype(np.int64).reshape(ref["clipped"].shape), ref["clipped"])
        if is_kernel:
            assert torch.equal(s.grad, ws), f"tensor {j}: ds against the per-tensor layer"
            assert torch.equal(counts[j], want_counts[j]), f"tensor {j}: counts against the per-tensor op"
        assert_within_terms(s.grad.cpu().numpy(), ref["ds"], ref["terms"], f"tensor {j}: ds against the reference")
        assert_within_terms(ws.cpu().numpy(), ref["ds"], ref["terms"], f"tensor {j}: the per-tensor ds against the reference")


# -------------------------------------------------------------------------------------------------------------------- 9 trainer
def _recipe(model, dev, seed):
    """Scales at which a sizeable share of the weights is inside the range (tests/test_gpu_groupwise.py::_recipe)."""
    import learned_quantization_amd as lq
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for layer in lq.custom_layers_of(model):
            for name in ("nested_q_w_layer", "nested_q_k_layer", "nested_q_b_layer"):
                nested = getattr(layer, name, None)
                if nested is not None:
                    v = np.float32(0.05 / 4) * rng.uniform(0.8, 1.25, tuple(nested.scale.shape)).astype(np.float32)
                    nested.scale.copy_(torch.from_numpy(v).to(dev))


def _linear_trainer(dev, tmp, steps, **kw):
    from _linear_task import LinearTaskTrainer, make_coefficients
    tr = LinearTaskTrainer(config="cifar", mode="ste", value=0.0, device=dev, log_dir=str(tmp), seed=3, bits=4, group_size=128, lr=1e-3, **kw)
    _recipe(tr.model, dev, 3)
    with torch.no_grad():                                           # biases are created at zero: give them something to clip
        g = torch.Generator().manual_seed(11)
        for layer in tr.custom_layers:
            if getattr(layer, "b", None) is not None:
                layer.b.copy_((torch.randn(layer.b.shape, generator=g) * 0.05).to(dev))
    tr.coefficients = make_coefficients(tr, steps, lo=-3.0, hi=-1.0)
    return tr


def test_trainer_step_matches_the_per_tensor_path(dev, tmp_path):
    """Step 1 of batched=True, group_batch=True against the per-tensor path on injected gradients: P.grad of every tensor and ds of
    every kernel bit for bit; ds of the biases (per-tensor: the one-axis clipped op, another traversal) within the bound against
    the reference of the bias geometry."""
    import learned_quantization_amd as lq
    plain = _linear_trainer(dev, tmp_path / "a", 1)
    lq.reset_layer_names()
    batched = _linear_trainer(dev, tmp_path / "b", 1, batched=True, group_batch=True)
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
        sa, sb = la_.nested_q_k_layer.scale, lb_.nested_q_k_layer.scale
        assert torch.equal(sa.grad, sb.grad) and bool((sb.grad != 0).all()), f"{la_.name}: ds of the kernel"
        assert torch.equal(sa.detach(), sb.detach()), f"{la_.name}: the kernel's scales after the step"
        if la_.name in before:
            ref = before[la_.name]
            assert torch.equal(la_.b.grad, lb_.b.grad), f"{la_.name}: P.grad of the bias"
            assert bits_equal(lb_.b.grad.cpu().numpy().reshape(1, -1), ref["dP"])
            for tr_layer, who in ((la_, "per-tensor"), (lb_, "batched")):
                assert_within_terms(tr_layer.nested_q_b_layer.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], f"{la_.name}: bias ds, {who}")
    assert len(before) == len(plain.custom_layers)


def test_two_batched_runs_are_bit_identical(dev, tmp_path):
    import learned_quantization_amd as lq
    runs = []
    x = torch.zeros(2, 3, 32, 32, device=dev)
    y = torch.zeros(2, dtype=torch.long, device=dev)
    for k in range(2):
        lq.reset_layer_names()
        tr = _linear_trainer(dev, tmp_path / str(k), 3, batched=True, group_batch=True)
        start = [l.nested_q_k_layer.scale.detach().clone() for l in tr.custom_layers]
        losses = [float(tr.step(x, y).detach()) for _ in range(3)]
        assert all(np.isfinite(v) for v in losses)
        for l, s0 in zip(tr.custom_layers, start):
            assert bool((l.nested_q_k_layer.scale.detach() != s0).all()), f"{l.name}: a group-wise scale did not move"
        runs.append({n: p.detach().clone() for n, p in tr.model.named_parameters()})
    assert runs[0].keys() == runs[1].keys()
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), n


def test_product_trainer_eager_and_graphed_and_exports(dev, tmp_path):
    """The product Trainer with the group batch, eager and graph=True from the same state (as
    tests/test_gpu_groupwise.py::test_trainer_eager_and_graphed): equal losses and parameters bit for bit, every group-wise scale
    has a gradient in some step and moves.  Both exports of the trained model round-trip."""
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    from learned_quantization_amd.train import Trainer, synthetic_batch
    gen = torch.Generator(device=dev).manual_seed(0)
    y = synthetic_batch("mnist", 32, dev, gen)[1]
    x = torch.randn(32, 1, 28, 28, device=dev, generator=gen)      # zero-mean inputs: see the fixture of test_gpu_groupwise.py
    runs = []
    for graph in (False, True):
        tr = Trainer(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path / f"g{int(graph)}"), graph=graph, seed=7,
                     bits=4, group_size=64, lr=1e-3, batched=True, group_batch=True)
        _recipe(tr.model, dev, 7)
        tr.model.eval()
        scales = [l.nested_q_w_layer.scale for l in tr.custom_layers]
        start = [s.detach().clone() for s in scales]
        step = tr.step_graphed if graph else tr.step
        losses, seen = [], [torch.zeros_like(s, dtype=torch.bool) for s in start]
        for _ in range(3 + (0 if graph else 3)):                    # step_graphed: 3 eager warm-up steps first
            losses.append(step(x, y).detach().clone())
            if not graph:
                seen = [m | (s.grad != 0) for m, s in zip(seen, scales)]
        torch.cuda.synchronize()
        runs.append((tr, losses[-3:], start, seen))
    (eager, le, start, seen), (graphed, lg, _, _) = runs
    assert graphed.graph is not None
    assert all(np.isfinite(float(a)) for a in le)
    for a, b in zip(le, lg):
        assert torch.equal(a, b), f"losses differ: {float(a)!r} {float(b)!r}"
    for (n, p), (_, p2) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), n
    for layer, s0, had in zip(eager.custom_layers, start, seen):
        scale = layer.nested_q_w_layer.scale
        assert bool(had.all()), f"{layer.name}: a group-wise scale without a gradient"
        assert bool((scale.detach() != s0).all()), f"{layer.name}: a group-wise scale did not move"
    model = eager.model
    tensors = export.quantized_tensors(model)
    lq.save_compress_parameters(model, str(tmp_path))
    weights = np.load(os.path.join(str(tmp_path), "weights.npy"), allow_pickle=True).item()
    for name, param, nested in tensors:
        if nested.group_size is not None:
            P, s = param.detach().cpu().numpy(), nested.scale.detach().cpu().numpy()
            assert np.array_equal(weights[name], group_reference(P, s, np.zeros_like(P), -8, 7, 0, 64)["q"].astype(np.int8)), name
    lq.save_packed_parameters(model, str(tmp_path))
    lq.reset_layer_names()
    fresh = lq.build_model("mnist", mode="ste", value=0.0, seed=99, device=dev, bits=4, group_size=64)
    lq.load_packed_parameters(fresh, str(tmp_path))
    for (name, p0, n0), (_, p1, n1) in zip(tensors, export.quantized_tensors(fresh)):
        assert torch.equal(n0.scale.detach(), n1.scale.detach()), name
        assert torch.equal(n0(p0).detach(), n1(p1).detach()), f"{name}: fake-quantised output after the restore"


def test_one_rank_ddp_mode_a_equals_the_plain_step(dev, tmp_path):
    """Data-parallel mode A on a one-rank gloo group: ds is written into the bucket views the batch found at construction, the
    exchange averages over one rank, and two steps leave every parameter and scale where the plain batched steps leave them."""
    import socket
    import torch.distributed as dist
    import learned_quantization_amd as lq
    from _linear_task import snapshot

    def run(sub, **kw):
        lq.reset_layer_names()
        tr = _linear_trainer(dev, tmp_path / sub, 2, batched=True, group_batch=True, **kw)
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
        assert tr.dp is not None and tr.batch.group_batch and tr.batch._external_grads
    finally:
        dist.destroy_process_group()
    for n in plain:
        assert torch.equal(plain[n], dp[n]), n
