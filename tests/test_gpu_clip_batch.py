"""GPU tests of the clipped multi-tensor batch (include/lq_hip.h: lq_batch_set_clip, lq_batch_forward_clip,
lq_batch_backward_clip, lq_batch_clip_counts; ``FakeQuantBatch(clipped=True)``; ``Trainer(batched=True, clipped_batch=True)``).

Yardsticks: tests/_clip_reference.py::clip_reference (floor) and tests/_rne_reference.py::rne_reference (nearest); ``out``, ``dP``
and the clip counts are compared bit for bit, against the reference and against the single-tensor ops; ``ds`` is held to
tests/_bounds.py::assert_within_terms (1e-5 * sum|terms|: its terms have no common quantum, two traversals of one tensor may
differ in the last bit).  Inputs are built so that every tensor has clipped AND inside elements (asserted on the reference
before any comparison): a test in which nothing clips cannot tell a masked dP from dy."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _bounds import assert_within_terms                      # noqa: E402
from _clip_reference import bits_equal, clip_reference       # noqa: E402
from _rne_reference import rne_reference                     # noqa: E402
from oracle import lq_oracle as O                             # noqa: E402
from oracle import lq_oracle_f64 as O64                       # noqa: E402

pytestmark = pytest.mark.gpu
LQ_EINVAL, LQ_EALIGN = -1, -4
REFERENCES = {"floor": clip_reference, "nearest": rne_reference}
RANGES = {"signed4": [(-8, 7)], "unsigned4": [(0, 15)], "per_tensor": [(-8, 7), (0, 15), (-3, 5), (-128, 127), (0, 1)]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pairs(model):
    """(layer, slot, parameter, nested layer) of every quantised tensor, in the batch's order."""
    import learned_quantization_amd as lq
    layers = lq.custom_layers_of(model) if isinstance(model, torch.nn.Module) and not isinstance(model, torch.nn.ModuleList) else list(model)
    out = []
    for l in layers:
        if hasattr(l, "W"):
            out += [(l, 0, l.W, l.nested_q_w_layer), (l, 1, l.b, l.nested_q_b_layer)]
        else:
            out.append((l, 0, l.kernel, l.nested_q_k_layer))
            if l._has_bias:
                out.append((l, 1, l.b, l.nested_q_b_layer))
    return out


def _set_scales(model, dev, seed=5):
    import learned_quantization_amd as lq
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for s in lq.scale_parameters(model):
            s.copy_((torch.rand(s.shape, generator=g) * 9e-3 + 1e-3).to(dev))


def _set_ranges(model, ranges):
    """Range i % len of ``ranges`` for the i-th quantised tensor (a plain attribute of the nested layer)."""
    for i, (_, _, _, nested) in enumerate(_pairs(model)):
        nested.q_range = ranges[i % len(ranges)]


def _fill(model, dev, seed=17):
    """Every parameter, biases included, becomes t * s with t uniform over [qmin - 4, qmax + 4] (fixed CPU generator); element 0
    is (qmax + 3) * s -- outside -- and element 1 is 0.25 * s -- inside (every range here holds 0; every tensor has >= 2 elements)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, _, param, nested in _pairs(model):
            qmin, qmax = nested.q_range
            s = nested.scale.detach().cpu().numpy()
            shape = tuple(param.shape)
            sb = np.broadcast_to(s if s.ndim == len(shape) else s.reshape((1,) * len(shape)), shape)
            t = (torch.rand(shape, generator=g, dtype=torch.float32).numpy() * np.float32(qmax - qmin + 8) + np.float32(qmin - 4)).astype(np.float32)
            P = (t * sb).astype(np.float32)
            flat, sflat = P.reshape(-1), np.ascontiguousarray(sb).reshape(-1)
            assert flat.size >= 2
            flat[0] = np.float32(qmax + 3) * sflat[0]
            flat[1] = np.float32(0.25) * sflat[1]
            param.copy_(torch.from_numpy(P.reshape(shape)).to(dev))


def _reference(rounding, param, nested, dy, k):
    ref = REFERENCES[rounding](param.detach().cpu().numpy(), nested.scale.detach().cpu().numpy(), dy.cpu().numpy(), *nested.q_range, k)
    n_out = int((~ref["inside"]).sum())
    assert 0 < n_out < ref["inside"].size, "the inputs must clip somewhere and pass somewhere"
    return ref


def _mixed_layers(dev, **kw):
    """The shapes of tests/test_gpu_ste_scale.py::_mixed_layers: row-stream, column-small, one long row, conv planes stored OIHW."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    kw = dict(initializer=lq.RandomNormal(seed=9), device=dev, **kw)
    layers = [lq.CustomDenseLayer(units=130, orientation="rowwise", input_shape=257, **kw),
              lq.CustomDenseLayer(units=10, orientation="columnwise", input_shape=133, **kw),
              lq.CustomDenseLayer(units=33, orientation="scalar", input_shape=401, **kw),
              lq.CustomConv2DLayer(filters=32, kernel_size=(3, 3), orientation="channelwise", input_shape=16, **kw),
              lq.CustomConv2DLayerNoBias(filters=8, kernel_size=(7, 7), orientation="channelwise", input_shape=3, **kw)]
    assert not layers[3].kernel.is_contiguous()                                            # stored OIHW (the default)
    return torch.nn.ModuleList(layers)


def _build(dev, which, rounding, ranges, scale_gradient="ste"):
    import learned_quantization_amd as lq
    if which == "mixed":
        m = _mixed_layers(dev, scale_gradient=scale_gradient, grad_scale=0.37, q_range=RANGES[ranges][0], rounding=rounding)
    else:
        lq.reset_layer_names()
        m = lq.build_model("cifar", mode="ste", value=0.0, seed=3, orientation="rowwise" if "rowwise" in which else "channelwise",
                           device=dev, grad_scale="rsqrt_group" if "rsqrt" in which else None, q_range=RANGES[ranges][0], rounding=rounding)
    _set_ranges(m, RANGES[ranges])
    _set_scales(m, dev)
    _fill(m, dev)
    return m


def _upstream(outs, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(o.shape, device=dev, generator=g) * torch.pow(10.0, torch.rand(o.shape, device=dev, generator=g) * 10.0 - 12.0)
            for o in outs]


def _run(batch, dys=None, dev=None):
    """quantize_all, backward with the upstream gradients ``dys`` (made here when None), finish_backward for the leaf form."""
    for e in batch.entries:
        e.param.grad = e.nested.scale.grad = None
    outs = batch.quantize_all()
    if dys is None:
        dys = _upstream(outs, dev)
    torch.autograd.backward(outs, dys)
    if not batch.autograd:
        batch.finish_backward()
    return outs, dys


# ------------------------------------------------------------------------------------------ 1: batch, reference, single-tensor ops
@pytest.mark.parametrize("which", ["cifar", "cifar_rsqrt_rowwise", "mixed"])
@pytest.mark.parametrize("ranges", list(RANGES))
@pytest.mark.parametrize("rounding", ["floor", "nearest"])
def test_batch_against_reference_and_single_tensor_ops(dev, rounding, ranges, which):
    import learned_quantization_amd as lq
    from learned_quantization_amd import ops
    m = _build(dev, which, rounding, ranges)
    refs = dys = None
    for autograd in (True, False):
        batch = lq.FakeQuantBatch(m, autograd=autograd, clipped=True)
        assert batch.clipped and batch.ste and batch.rounding == rounding and len(batch.entries) == (12 if which != "mixed" else 9)
        if ranges == "per_tensor":
            assert len({e.nested.q_range for e in batch.entries}) == len(RANGES[ranges])
        outs, dys = _run(batch, dys, dev)
        if refs is None:           # computed once: both forms see the same parameters, scales and upstream gradients
            refs = [_reference(rounding, e.param, e.nested, d, e.nested.grad_scale_value(e.param.numel())) for e, d in zip(batch.entries, dys)]
        counts = batch.clip_counts()
        first = []
        for e, o, d, ref, cnt in zip(batch.entries, outs, dys, refs, counts):
            what = f"{which} {ranges} {rounding} autograd={autograd} {e.layer.name} slot {e.slot} {e.nested.q_range}"
            qmin, qmax = e.nested.q_range
            k = e.nested.grad_scale_value(e.param.numel())
            dP = e.param.grad
            assert bits_equal(o.detach().cpu().numpy(), ref["out"]), what + ": out vs reference"
            assert torch.equal(o.detach(), ops.fq_forward_clip(e.param.data, e.nested.scale.data, qmin, qmax, rounding=rounding)), what + ": out vs single op"
            assert bits_equal(dP.cpu().numpy(), ref["dP"]), what + ": dP vs reference"
            assert not torch.equal(dP, d), what + ": dP must be a MASKED copy of dy"
            sdP, sds, scl = ops.fq_backward_clip(e.param.data, e.nested.scale.data, d, qmin, qmax, k, want_clipped=True, rounding=rounding)
            assert bits_equal(dP.cpu().numpy(), sdP.cpu().numpy()), what + ": dP vs single op"
            assert cnt.dtype == torch.int32 and cnt.shape == e.nested.scale.shape
            assert np.array_equal(cnt.cpu().numpy().astype(np.int64), ref["clipped"]), what + ": clip counts vs reference"
            assert torch.equal(cnt, scl), what + ": clip counts vs single op"
            got = e.nested.scale.grad.cpu().numpy()
            assert_within_terms(got, ref["ds"], ref["terms"], what + ": ds vs reference")
            assert_within_terms(sds.cpu().numpy(), ref["ds"], ref["terms"], what + ": single-op ds vs reference")
            assert_within_terms(got, sds.cpu().numpy(), ref["terms"], what + ": ds vs single op")
            first.append((dP.clone(), e.nested.scale.grad.clone(), cnt))
        # a second backward: the same bits
        _run(batch, dys, dev)
        for e, (dP, ds, cnt), cnt2 in zip(batch.entries, first, batch.clip_counts()):
            assert torch.equal(e.param.grad, dP) and torch.equal(e.nested.scale.grad, ds) and torch.equal(cnt, cnt2)


# ------------------------------------------------------------------------------------------ 2: mask only
@pytest.mark.parametrize("rounding", ["floor", "nearest"])
@pytest.mark.parametrize("autograd", [True, False])
def test_mask_only_leaves_the_scale_gradients_alone(dev, autograd, rounding):
    import learned_quantization_amd as lq
    m = _build(dev, "mixed", rounding, "per_tensor", scale_gradient=None)
    batch = lq.FakeQuantBatch(m, autograd=autograd, clipped=True)
    assert batch.clipped and not batch.ste
    for e in batch.entries:
        e.ds.fill_(123.0)
    outs, dys = _run(batch, None, dev)
    for e, o, d, cnt in zip(batch.entries, outs, dys, batch.clip_counts()):
        ref = _reference(rounding, e.param, e.nested, d, 1.0)
        what = f"{rounding} {e.layer.name} slot {e.slot}"
        assert bits_equal(o.detach().cpu().numpy(), ref["out"]), what
        assert bits_equal(e.param.grad.cpu().numpy(), ref["dP"]) and not torch.equal(e.param.grad, d), what
        assert np.array_equal(cnt.cpu().numpy().astype(np.int64), ref["clipped"]), what
        assert e.nested.scale.grad is None, what
        assert bool((e.ds == 123.0).all()), what + ": ds must not be written at all"


# ------------------------------------------------------------------------------------------ 3: stecl
@pytest.mark.parametrize("kind", ["maxbin", "difference", "inverse"])
def test_stecl_is_clipped_ste_part_plus_penalty_part(dev, kind):
    """backward (lq_batch_backward_clip writes ds), then inject_penalty_grads(..., accumulate_ds=True) adds the term's."""
    import learned_quantization_amd as lq
    gamma = 0.37
    lq.reset_layer_names()
    m = lq.build_model("cifar", mode="stecl", value=gamma, seed=3, orientation="channelwise", device=dev, bits=4)
    _set_scales(m, dev)
    _fill(m, dev)
    layers = lq.custom_layers_of(m)
    batch = lq.FakeQuantBatch(m, clipped=True)
    outs, dys = _run(batch, None, dev)
    batch.inject_penalty_grads(kind, gamma, accumulate_ds=True)
    l64 = []
    for l in layers:
        k, ks = l.kernel.detach().cpu().numpy(), l.nested_q_k_layer.scale.detach().cpu().numpy()
        b, bs = l.b.detach().cpu().numpy(), l.nested_q_b_layer.scale.detach().cpu().numpy()
        l64.append((k, ks, O.group_descriptor(k.shape, ks.shape), b, bs, O.group_descriptor(b.shape, bs.shape)))
    g64 = O64.penalty_grads(kind, l64, gamma)
    by_param = {id(e.param): d for e, d in zip(batch.entries, dys)}
    for l, e64 in zip(layers, g64):
        for param, nested, key in ((l.kernel, l.nested_q_k_layer, "dsK"), (l.b, l.nested_q_b_layer, "dsb")):
            ref = _reference("floor", param, nested, by_param[id(param)], nested.grad_scale_value(param.numel()))
            pen = np.asarray(e64[key], np.float64).reshape(ref["ds"].shape)
            pen_terms = np.asarray(e64[key + "_abs"], np.float64).reshape(ref["ds"].shape)
            assert np.any(pen != 0.0)
            assert_within_terms(nested.scale.grad.cpu().numpy(), ref["ds"] + pen, ref["terms"] + pen_terms, f"{kind} {l.name} {key}")


# ------------------------------------------------------------------------------------------ 4: the C ABI's refusals
class _AbiBatch:
    """Two tensors through ``_hip`` directly: (1, 5, 4100) -- a float4 row stream -- and (133, 10, 1) -- a scalar column form."""
    DESCS = [(1, 5, 4100), (133, 10, 1)]

    def __init__(self, dev, dp_offset=0, no_dp=False, p_offset=0):
        from learned_quantization_amd import _hip
        self.lib = _hip.load()
        g = torch.Generator().manual_seed(3)
        n = len(self.DESCS)
        self.keep, self.P, self.s, self.out, self.ds, self.dp, self.dy = [], [], [], [], [], [], []
        arr = (_hip.TensorDesc * n)()
        for i, (outer, G, inner) in enumerate(self.DESCS):
            numel = outer * G * inner
            s = (torch.rand(G, generator=g) * 9e-3 + 1e-3).to(dev)
            t = torch.rand(numel, generator=g) * 24.0 - 12.0
            P = self._at(dev, numel, p_offset if i == 0 else 0)
            P.copy_((t.view(outer, G, inner) * s.cpu().view(1, G, 1)).reshape(-1).to(dev))
            dy = self._at(dev, numel, p_offset if i == 0 else 0)
            dy.copy_(torch.randn(numel, generator=g).to(dev))
            out = self._at(dev, numel, p_offset if i == 0 else 0).fill_(-7.0)
            dp = self._at(dev, numel, (dp_offset or p_offset) if i == 0 else 0).fill_(-7.0)
            ds = torch.full((G,), -7.0, device=dev)
            for lst, v in ((self.P, P), (self.s, s), (self.out, out), (self.ds, ds), (self.dp, dp), (self.dy, dy)):
                lst.append(v)
            arr[i] = _hip.TensorDesc(P.data_ptr(), s.data_ptr(), None, out.data_ptr(), ds.data_ptr(), None, None, outer, G, inner,
                                     float("nan"), float("-inf"), None, None if (no_dp and i == 1) else dp.data_ptr(), 0, 0, 0)
        self.handle = ctypes.c_void_p()
        _hip.check(self.lib.lq_batch_create(arr, n, ctypes.byref(self.handle)), "lq_batch_create")
        self.n = n

    def _at(self, dev, numel, offset_floats):
        buf = torch.zeros(numel + 4, device=dev)
        assert buf.data_ptr() % 16 == 0
        self.keep.append(buf)
        return buf[offset_floats:offset_floats + numel]

    def set_clip(self, qmin=(-8, 0), qmax=(7, 15), n=None, rounding=0):
        a, b = (ctypes.c_int32 * len(qmin))(*qmin), (ctypes.c_int32 * len(qmax))(*qmax)
        return self.lib.lq_batch_set_clip(self.handle, a, b, self.n if n is None else n, rounding)

    def workspace(self, dev):
        return torch.empty(self.lib.lq_batch_workspace_bytes(self.handle), dtype=torch.uint8, device=dev)

    def backward(self, dev, dys=None, grad_scale=(1.0, 1.0)):
        ws = self.workspace(dev)
        ptrs = (ctypes.c_void_p * self.n)(*[d.data_ptr() for d in (dys or self.dy)])
        gs = None if grad_scale is None else (ctypes.c_float * self.n)(*grad_scale)
        return self.lib.lq_batch_backward_clip(self.handle, ptrs, gs, ws.data_ptr(), ws.numel(), None)

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == -7.0).all()) for t in self.out + self.dp + self.ds)

    def err(self):
        return self.lib.lq_last_error().decode()

    def close(self):
        self.lib.lq_batch_destroy(self.handle)


def test_abi_refusals_launch_nothing(dev):
    """Forward / backward before lq_batch_set_clip, a bad range, a bad rounding, a wrong n: an error code, and no output written."""
    b = _AbiBatch(dev)
    assert b.lib.lq_batch_forward_clip(b.handle, None) == LQ_EINVAL and "lq_batch_set_clip" in b.err()
    assert b.backward(dev) == LQ_EINVAL and "lq_batch_set_clip" in b.err()
    dv, groups = ctypes.c_void_p(), ctypes.c_int64()
    assert b.lib.lq_batch_clip_counts(b.handle, 0, ctypes.byref(dv), ctypes.byref(groups)) == LQ_EINVAL
    assert b.set_clip(qmin=(8, 0), qmax=(7, 15)) == LQ_EINVAL and "qmin" in b.err()
    assert b.set_clip(qmax=(7, (1 << 24) + 1)) == LQ_EINVAL
    assert b.set_clip(rounding=7) == LQ_EINVAL and "rounding" in b.err()
    assert b.set_clip(n=1) == LQ_EINVAL and b.set_clip(qmin=(-8, 0, 0), qmax=(7, 15, 15), n=3) == LQ_EINVAL
    assert b.lib.lq_batch_forward_clip(b.handle, None) == LQ_EINVAL          # a refused set_clip leaves the batch without ranges
    assert b.untouched()
    b.close()


def test_abi_refuses_bad_dy_and_bad_dp(dev):
    """A refused call returns its code before any launch: outputs keep their sentinel.  ``dp`` 4 bytes off a 16-byte base under a
    float4 task is REFUSED with LQ_EALIGN by lq_batch_set_clip (the scalar form is taken only where P itself is misaligned)."""
    b = _AbiBatch(dev)
    assert b.set_clip() == 0
    null_dy = (ctypes.c_void_p * b.n)(b.dy[0].data_ptr(), None)
    ws = b.workspace(dev)
    assert b.lib.lq_batch_backward_clip(b.handle, null_dy, None, ws.data_ptr(), ws.numel(), None) == LQ_EINVAL and "upstream" in b.err()
    shifted = torch.zeros(b.dy[0].numel() + 4, device=dev)
    assert shifted.data_ptr() % 16 == 0
    assert b.backward(dev, [shifted[1:1 + b.dy[0].numel()], b.dy[1]]) == LQ_EALIGN and "16-byte" in b.err()
    assert b.lib.lq_batch_backward_clip(b.handle, None, None, None, 0, None) == -3                          # LQ_EWORKSPACE
    assert b.untouched()
    b.close()
    b = _AbiBatch(dev, no_dp=True)
    assert b.set_clip() == LQ_EINVAL and "dp" in b.err()
    assert b.lib.lq_batch_forward_clip(b.handle, None) == LQ_EINVAL
    assert b.untouched()
    b.close()
    b = _AbiBatch(dev, dp_offset=1)
    assert b.dp[0].data_ptr() % 16 == 4
    assert b.set_clip() == LQ_EALIGN and "dp" in b.err()
    assert b.lib.lq_batch_forward_clip(b.handle, None) == LQ_EINVAL and b.backward(dev) == LQ_EINVAL
    assert b.untouched()
    b.close()


@pytest.mark.parametrize("rounding", [0, 1])
@pytest.mark.parametrize("p_offset", [0, 1])
def test_abi_calls_equal_the_single_tensor_ops(dev, rounding, p_offset):
    """Through the C ABI alone.  ``p_offset=1``: P, dy, out and dp of the row tensor one float off a 16-byte base -- the scalar forms
    serve it, bit-correct.  Then a repeated lq_batch_set_clip replaces the ranges."""
    from learned_quantization_amd import ops
    b = _AbiBatch(dev, p_offset=p_offset)
    name = ("floor", "nearest")[rounding]
    for ranges in (((-8, 0), (7, 15)), ((-3, -2), (5, 2))):
        assert b.set_clip(qmin=ranges[0], qmax=ranges[1], rounding=rounding) == 0
        assert b.lib.lq_batch_forward_clip(b.handle, None) == 0
        assert b.backward(dev, grad_scale=(0.37, 2.0)) == 0
        for i, (outer, G, inner) in enumerate(b.DESCS):
            qmin, qmax = ranges[0][i], ranges[1][i]
            P, s, dy = b.P[i].view(outer, G, inner), b.s[i].view(1, G, 1), b.dy[i].view(outer, G, inner)
            assert torch.equal(b.out[i].view(outer, G, inner), ops.fq_forward_clip(P, s, qmin, qmax, rounding=name))
            dP, ds, cl = ops.fq_backward_clip(P, s, dy, qmin, qmax, (0.37, 2.0)[i], want_clipped=True, rounding=name)
            assert torch.equal(b.dp[i].view(outer, G, inner), dP) and bool((dP == 0).any()) and bool((dP != 0).any())
            ref = REFERENCES[name](P.cpu().numpy(), s.cpu().numpy(), dy.cpu().numpy(), qmin, qmax, (0.37, 2.0)[i])
            assert_within_terms(b.ds[i].cpu().numpy(), ref["ds"], ref["terms"], f"tensor {i} {ranges}")
            dv, groups = ctypes.c_void_p(), ctypes.c_int64()
            assert b.lib.lq_batch_clip_counts(b.handle, i, ctypes.byref(dv), ctypes.byref(groups)) == 0 and groups.value == G and dv.value
    b.close()


# ------------------------------------------------------------------------------------------ 5: the trainer, per tensor against batched
def _linear_pair(dev, tmp_path, mode, loss, value, **kw):
    from _linear_task import LinearTaskTrainer, make_coefficients
    out = []
    for batched in (False, True):
        tr = LinearTaskTrainer("cifar", mode, value, "channelwise", loss, device=dev, log_dir=str(tmp_path), batched=batched,
                               clipped_batch=batched, seed=11, bits=4, **kw)
        _set_scales(tr.model, dev)
        _fill(tr.model, dev)
        tr.coefficients = make_coefficients(tr, 1)
        out.append(tr)
    assert out[1].batch is not None and out[1].batch.clipped and out[0].batch is None
    return out


@pytest.mark.parametrize("case", ["ste", "ste_nearest", "stecl_difference"])
def test_trainer_per_tensor_against_clipped_batch_after_one_step(dev, tmp_path, case):
    """Same state, same injected upstream gradients (tests/_linear_task.py), ONE step: every parameter gradient bit-equal between
    the two forms, every scale.grad within the bound of the reference and of the other form."""
    gamma = 0.37
    rounding = "nearest" if "nearest" in case else "floor"
    if case.startswith("stecl"):
        per_tensor, batched = _linear_pair(dev, tmp_path, "stecl", "difference", gamma, rounding=rounding)
        k = 1.0
    else:
        per_tensor, batched = _linear_pair(dev, tmp_path, "ste", None, 0.0, grad_scale=0.37, rounding=rounding)
        k = 0.37
    layers = per_tensor.custom_layers
    l64 = []
    for l in layers:
        kk, ks = l.kernel.detach().cpu().numpy().copy(), l.nested_q_k_layer.scale.detach().cpu().numpy().copy()
        b, bs = l.b.detach().cpu().numpy().copy(), l.nested_q_b_layer.scale.detach().cpu().numpy().copy()
        l64.append((kk, ks, O.group_descriptor(kk.shape, ks.shape), b, bs, O.group_descriptor(b.shape, bs.shape)))
    g64 = O64.penalty_grads("difference", l64, gamma) if case.startswith("stecl") else None
    for tr in (per_tensor, batched):
        tr.step(None, None)
    coeffs = per_tensor.coefficients[0]
    for li, (la, lb) in enumerate(zip(layers, batched.custom_layers)):
        for slot, (pa, pb, na, nb, key) in enumerate(((la.kernel, lb.kernel, la.nested_q_k_layer, lb.nested_q_k_layer, "dsK"),
                                                      (la.b, lb.b, la.nested_q_b_layer, lb.nested_q_b_layer, "dsb"))):
            what = f"{case} {la.name} slot {slot}"
            P, s = l64[li][0 + 3 * slot], l64[li][1 + 3 * slot]
            dy = coeffs[li][slot].cpu().numpy()
            ref = REFERENCES[rounding](P, s, dy, -8, 7, k)
            assert 0 < int((~ref["inside"]).sum()) < ref["inside"].size
            rds, rterms = ref["ds"], ref["terms"]
            if g64 is not None:
                rds = rds + np.asarray(g64[li][key], np.float64).reshape(rds.shape)
                rterms = rterms + np.asarray(g64[li][key + "_abs"], np.float64).reshape(rds.shape)
            else:
                assert bits_equal(pb.grad.cpu().numpy(), ref["dP"]) and not bits_equal(pb.grad.cpu().numpy(), dy), what
            ga, gb = na.scale.grad.cpu().numpy(), nb.scale.grad.cpu().numpy()
            assert_within_terms(ga, rds, rterms, what + ": per-tensor")
            assert_within_terms(gb, rds, rterms, what + ": clipped batch")
            assert_within_terms(ga, gb, rterms, what + ": per-tensor vs clipped batch")
            assert bits_equal(pa.grad.cpu().numpy(), pb.grad.cpu().numpy()), what + ": parameter gradients"


# ------------------------------------------------------------------------------------------ 6: graphed step
def test_trainer_graphed_clipped_batch_step_equals_eager_step(dev, tmp_path):
    """mnist, bits=4, mode "ste": the whole clipped-batch step from a hipGraph == the eager one, parameter for parameter, 3 steps."""
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    res, start = [], None
    for graph in (False, True):
        tr = Trainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path), graph=graph, batched=True, clipped_batch=True,
                     seed=7, bits=4)
        _set_scales(tr.model, dev)
        _fill(tr.model, dev)
        start = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
        tr.model.eval()
        step = tr.step_graphed if graph else tr.step
        for _ in range(3 + (0 if graph else 3)):          # step_graphed runs 3 eager warm-up steps before it captures
            step(x, y)
        torch.cuda.synchronize()
        res.append({n: p.detach().clone() for n, p in tr.model.named_parameters()})
    moved = False
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), n
        moved = moved or ("scale" in n and not torch.equal(res[0][n], start[n]))
    assert moved, "no scale moved"


# ------------------------------------------------------------------------------------------ 7: one-rank data parallel, mode A
def test_one_rank_ddp_mode_a_clipped_batch_step_equals_the_plain_step(dev, tmp_path):
    import socket
    import torch.distributed as dist
    from _linear_task import LinearTaskTrainer, make_coefficients, snapshot

    def run(**kw):
        tr = LinearTaskTrainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path), batched=True, clipped_batch=True,
                               bits=4, seed=5, **kw)
        _set_scales(tr.model, dev)
        _fill(tr.model, dev)
        tr.coefficients = make_coefficients(tr, 2)
        for _ in range(2):
            tr.step(None, None)
        torch.cuda.synchronize()
        return tr, snapshot(tr)

    _, plain = run()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        tr, dp = run(ddp_mode="A", force_collectives=True)
        assert tr.dp is not None and tr.batch.clipped
    finally:
        dist.destroy_process_group()
    for n in plain:
        assert torch.equal(plain[n], dp[n]), n


# ------------------------------------------------------------------------------------------ 8: export
def test_export_after_clipped_batch_steps(dev, tmp_path):
    import learned_quantization_amd as lq
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    tr = Trainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path), batched=True, clipped_batch=True, seed=7, bits=4,
                 lr=1e-3)
    _set_scales(tr.model, dev)
    _fill(tr.model, dev)
    before = tr.model.dense_1.W.detach().clone()
    for _ in range(3):
        assert np.isfinite(float(tr.step(x, y).detach()))
    assert not torch.equal(before, tr.model.dense_1.W.detach())
    lq.save_compress_parameters(tr.model, str(tmp_path))
    weights = np.load(os.path.join(str(tmp_path), "weights.npy"), allow_pickle=True).item()
    assert weights
    for name, w in weights.items():
        assert w.dtype == np.int8 and w.min() >= -8 and w.max() <= 7, name
    info = lq.save_packed_parameters(tr.model, str(tmp_path))
    assert info["bits_per_weight"] <= 4.0


# ------------------------------------------------------------------------------------------ refusals that need a built batch
def test_clipped_batch_refuses_mode_b_and_the_fused_update(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    m = lq.build_model("mnist", mode="ste", value=0.0, seed=3, orientation="rowwise", device=dev, bits=4)
    batch = lq.FakeQuantBatch(m, autograd=False, clipped=True)
    with pytest.raises(ValueError, match="fused=False"):
        lq.BatchedScaleAdam(batch, fused=True)
    lq.BatchedScaleAdam(batch, fused=False)
    with pytest.raises(ValueError, match="masked copy"):
        batch.scale_grads_from_param_grads()
    batch.defer_scale_grads = True
    batch.quantize_all()
    with pytest.raises(ValueError, match="masked copy"):
        batch.finish_backward()
