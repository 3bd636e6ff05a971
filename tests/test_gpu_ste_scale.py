"""GPU tests of the straight-through scale gradient (include/lq_hip.h: lq_fq_scale_grad_ste, lq_batch_scale_grad_ste).

The yardstick is tests/_bounds.py::assert_within_terms, |got - ref| <= 1e-5 * sum|terms| (floor 2^-136), against the NumPy
restatement of the definition below.  Any admissible implementation is off by about 2^-23 * sum|terms| (one product rounding,
one final rounding, an f64 sum); a float64 QUOTIENT instead of K1's float32 one is off by ~3e-4 * sum|terms| at the initial
scale and fails.  Results of different traversals of one tensor (single-tensor call, batch, per-tensor against batched
trainer) are NOT bit-identical -- the terms have no common quantum -- and are compared under the same bound; every single
traversal is run-to-run bit-stable, which is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _bounds import assert_within_terms, stable_seed      # noqa: E402
from oracle import lq_oracle as O                          # noqa: E402
from oracle import lq_oracle_f64 as O64                    # noqa: E402

pytestmark = pytest.mark.gpu
SCALE_INIT = 1.1920929e-05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def ste_reference(P, s, dy, k=1.0):
    """(k * S, k * sum|terms|) per scale element, in the shape of ``s``: t = P / s as the float32 quotient, r = floor(t) - t as
    ONE float32 subtraction, products and sums in float64.  ``s`` broadcasts against ``P`` (one non-unit axis, or one element)."""
    P, dy, s = np.asarray(P, np.float32), np.asarray(dy, np.float32), np.asarray(s, np.float32)
    sb = s if s.ndim == P.ndim else s.reshape((1,) * P.ndim)
    with np.errstate(all="ignore"):
        t = P / sb
        r = np.floor(t) - t
        assert t.dtype == np.float32 and r.dtype == np.float32
        terms = dy.astype(np.float64) * r.astype(np.float64)
        axes = tuple(a for a in range(P.ndim) if sb.shape[a] == 1)
        k64 = float(np.float32(k))                     # the factor travels as a C float
        return terms.sum(axis=axes).reshape(s.shape) * k64, np.abs(terms).sum(axis=axes).reshape(s.shape) * k64


DESCRIPTORS = [
    (1, 1, 12289),                                                     # scalar: one long row, scalar head/tail
    (1, 1, 10),                                                        # bias
    (1, 5, 4100),                                                      # row stream with a folded tail
    (2, 3, 1027),                                                      # rows off the 16-byte grid
    (1, 37, 100), (1, 64, 17), (3, 7, 196), (1, 9, 1000),              # row small / teams
    (133, 10, 1), (300, 3, 1), (64, 130, 4), (129, 257, 1), (40, 1001, 1),      # column forms
    (256, 16, 49),                                                     # 7 x 7 planes
    (1, 2, 300001),                                                    # 293 partials per group: the 256-thread finalize
    (1024, 2048, 1),                                                   # 64 row blocks x 2048 columns: the column form of the finalize
    (1, 3, 1 << 21), (1 << 20, 6, 1),                                  # streaming size: the generic bodies still serve them
]
SCALE_KINDS = ["init", "random", "one", "pow2"]


def _inputs(desc, scale_kind):
    """P, s and the three dy of one case as device tensors of shape (outer, G, inner) / (1, G, 1)."""
    outer, G, inner = desc
    rng = np.random.default_rng(stable_seed(desc, scale_kind))
    n = outer * G * inner
    P = rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)
    if scale_kind == "init":
        s = np.full(G, SCALE_INIT, np.float32)                         # |q| ~ 1e4
    elif scale_kind == "random":
        s = rng.uniform(1e-3, 1e-2, G).astype(np.float32)
    elif scale_kind == "one":
        s = np.ones(G, np.float32)
        P *= np.float32(1e-2)                                          # |P| << 1: q in {-1, 0}
    else:
        s = np.full(G, 2.0 ** -7, np.float32)
    signed = (rng.standard_normal(n, dtype=np.float32) * np.power(10.0, rng.uniform(-12.0, -2.0, n))).astype(np.float32)
    dys = {"signed": signed, "positive": np.abs(signed) + np.float32(1e-30), "zero": np.zeros(n, np.float32)}
    return P.reshape(desc), s.reshape(1, G, 1), {k: v.reshape(desc) for k, v in dys.items()}


def _dev(a, dev, misaligned=False):
    """Device copy; ``misaligned``: one float off a 16-byte base."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if not misaligned:
        return t
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _check_case(dev, desc, scale_kind, misaligned=False):
    import learned_quantization_amd as lq
    P, s, dys = _inputs(desc, scale_kind)
    Pt, st = _dev(P, dev, misaligned), _dev(s, dev)
    for name, dy in dys.items():
        dt = _dev(dy, dev, misaligned)
        ds = lq.fq_scale_grad_ste(Pt, st, dt)
        again = lq.fq_scale_grad_ste(Pt, st, dt)
        assert ds.shape == st.shape
        assert torch.equal(ds, again), f"{desc} {scale_kind} {name}: two calls differ"
        got = ds.cpu().numpy()
        ref, terms = ste_reference(P, s, dy)
        print(f"{desc} {scale_kind} {name}: max err / sum|terms| = "
              f"{float(np.max(np.abs(got - ref) / np.maximum(terms, 1e-300))) if name != 'zero' else 0.0:.3e}")
        if name == "zero":
            assert np.all(got == 0.0), f"{desc} {scale_kind}: dy == 0 must give ds == 0"
            continue
        if name == "positive":             # every term <= 0: the yardstick IS |ds|, the bound is a relative one
            np.testing.assert_allclose(terms, np.abs(ref), rtol=1e-12)
            assert np.all(got <= 0.0)
        assert_within_terms(got, ref, terms, f"{desc} {scale_kind} dy {name}")


@pytest.mark.parametrize("scale_kind", SCALE_KINDS)
@pytest.mark.parametrize("desc", DESCRIPTORS, ids=lambda d: "x".join(map(str, d)))
def test_single_tensor_against_the_reference(dev, desc, scale_kind):
    _check_case(dev, desc, scale_kind)


@pytest.mark.parametrize("scale_kind", SCALE_KINDS)
@pytest.mark.parametrize("desc", [(1, 1, 12289), (1, 5, 4100), (1, 37, 100), (64, 130, 4), (129, 257, 1), (300, 3, 1)],
                         ids=lambda d: "x".join(map(str, d)))
def test_misaligned_base(dev, desc, scale_kind):
    """P and dy one float off a 16-byte base: the scalar forms of every traversal."""
    _check_case(dev, desc, scale_kind, misaligned=True)


@pytest.mark.parametrize("desc", [(1, 1, 12289), (1, 1, 10), (1, 5, 4100), (1, 37, 100), (133, 10, 1), (64, 130, 4)],
                         ids=lambda d: "x".join(map(str, d)))
def test_grad_scale_factor(dev, desc):
    """k = 0.37: applied once per group in f64, by the finalize forms and by the direct emit alike."""
    import learned_quantization_amd as lq
    P, s, dys = _inputs(desc, "random")
    ds = lq.fq_scale_grad_ste(_dev(P, dev), _dev(s, dev), _dev(dys["signed"], dev), grad_scale=0.37)
    ref, terms = ste_reference(P, s, dys["signed"], 0.37)
    assert_within_terms(ds.cpu().numpy(), ref, terms, f"{desc} k=0.37")
    ref1, _ = ste_reference(P, s, dys["signed"])
    assert np.max(np.abs(ref - ref1)) > 0.0


@pytest.mark.parametrize("orientation", ["rowwise", "columnwise", "channelwise", "scalar"])
@pytest.mark.parametrize("scale_kind", SCALE_KINDS)
def test_oihw_stored_conv_kernel_through_ops(dev, orientation, scale_kind):
    """A (3, 3, 16, 32) kernel shaped HWIO and stored OIHW (layers.py kernel_storage): described in memory order, not copied;
    dy arrives in the logical order and in the parameter's own order."""
    import learned_quantization_amd as lq
    shape = (3, 3, 16, 32)
    sshape = lq.scale_shape(shape, orientation)
    G = int(np.prod(sshape))
    P, s, dys = _inputs((1, G, int(np.prod(shape)) // G), scale_kind)
    P, s = P.reshape(shape), s.reshape(sshape)
    Pt = _dev(P, dev).permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)
    assert not Pt.is_contiguous() and tuple(Pt.shape) == shape
    st = _dev(s, dev)
    for name in ("signed", "positive"):
        dy = dys[name].reshape(shape)
        ref, terms = ste_reference(P, s, dy)
        d_logical = _dev(dy, dev)
        d_stored = d_logical.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)
        for dt in (d_logical, d_stored):
            ds = lq.fq_scale_grad_ste(Pt, st, dt)
            assert ds.shape == st.shape
            assert_within_terms(ds.cpu().numpy(), ref, terms, f"OIHW-stored {orientation} {scale_kind} {name}")
    assert torch.equal(lq.fq_scale_grad_ste(Pt, st, _dev(dys["zero"].reshape(shape), dev)), torch.zeros_like(st))


def test_special_values(dev):
    """NaN / Inf as float32 arithmetic gives them: a NaN quotient poisons its own group only; |t| >= 2^23 contributes exactly 0."""
    import learned_quantization_amd as lq
    for desc in ((1, 5, 4100), (1, 37, 100), (133, 10, 1), (64, 130, 4)):
        P, s, dys = _inputs(desc, "random")
        G = desc[1]
        P = P.copy()
        P[:, 2, :] = (np.round(P[:, 2, :] * 1e6) + 1.0) * np.float32(2.0 ** 24) * s[0, 2, 0]      # group 2: every |t| >= 2^23
        P[0, 1, 0] = np.nan                                                                       # group 1: one NaN
        if G > 4:
            P[-1, 4, -1] = np.inf                                                                 # group 4: one +Inf quotient
        dy = dys["signed"]
        got = lq.fq_scale_grad_ste(_dev(P, dev), _dev(s, dev), _dev(dy, dev)).cpu().numpy().reshape(-1)
        ref, terms = (a.reshape(-1) for a in ste_reference(P, s, dy))
        assert np.isnan(got[1]) and np.isnan(ref[1])
        assert got[2] == 0.0 and ref[2] == 0.0 and terms[2] == 0.0
        if G > 4:
            assert np.isnan(got[4]) and np.isnan(ref[4])
        ok = np.array([g not in (1, 2, 4) for g in range(G)])
        assert np.all(np.isfinite(got[ok]))
        assert_within_terms(got[ok], ref[ok], terms[ok], f"{desc} groups without special values")


def test_autograd(dev):
    import learned_quantization_amd as lq
    P, s, dys = _inputs((1, 37, 100), "random")
    for gs in (1.0, 0.37):
        Pt = _dev(P, dev).requires_grad_(True)
        st = _dev(s, dev).requires_grad_(True)
        dy = _dev(dys["signed"], dev)
        out = lq.my_custom_gradient(Pt, st, scale_gradient="ste", grad_scale=gs)
        assert torch.equal(out, lq.fq_forward(Pt.detach(), st.detach()))
        out.backward(dy)
        assert torch.equal(Pt.grad, dy)                                                    # dP is dy, bit for bit
        assert torch.equal(st.grad, lq.fq_scale_grad_ste(Pt.detach(), st.detach(), dy, gs))
    # the default is today's behaviour: the two-argument op hands back zeros for the scale
    Pt = _dev(P, dev).requires_grad_(True)
    st = _dev(s, dev).requires_grad_(True)
    lq.my_custom_gradient(Pt, st, scale_gradient=None).backward(dy)
    assert torch.equal(st.grad, torch.zeros_like(st)) and torch.equal(Pt.grad, dy)
    Pt.grad = st.grad = None
    lq.my_custom_gradient(Pt, st).backward(dy)
    assert torch.equal(st.grad, torch.zeros_like(st)) and torch.equal(Pt.grad, dy)


@pytest.mark.parametrize("storage", ["oihw", "hwio"])
def test_conv_layer_per_tensor_path_takes_either_storage(dev, storage):
    """``kernel_storage="hwio"``: the plain op and the permuted view (no OIHW companion op exists for this rule)."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomConv2DLayer(filters=32, kernel_size=(3, 3), orientation="channelwise", initializer=lq.RandomNormal(seed=4),
                                 input_shape=16, device=dev, scale_gradient="ste", grad_scale="rsqrt_group", kernel_storage=storage)
    _set_scales(layer, dev)
    assert layer.kernel.is_contiguous() == (storage == "hwio")
    w, qb = layer.quantized_parameters()
    assert tuple(w.shape) == (32, 16, 3, 3)
    g = torch.Generator(device=dev).manual_seed(2)
    c = torch.randn(w.shape, device=dev, generator=g) * 1e-3
    cb = torch.randn(qb.shape, device=dev, generator=g) * 1e-3
    ((w * c).sum() + (qb * cb).sum()).backward()
    assert torch.equal(layer.kernel.grad, c.permute(2, 3, 1, 0)) and torch.equal(layer.b.grad, cb)
    for param, nested, dy in ((layer.kernel, layer.nested_q_k_layer, c.permute(2, 3, 1, 0)), (layer.b, layer.nested_q_b_layer, cb)):
        k = nested.grad_scale_value(param.numel())
        assert k == pytest.approx((param.numel() / nested.scale.numel()) ** -0.5)
        ref, terms = ste_reference(param.detach().cpu().numpy(), nested.scale.detach().cpu().numpy(), dy.cpu().numpy(), k)
        assert_within_terms(nested.scale.grad.cpu().numpy(), ref, terms, f"{storage} {tuple(param.shape)}")


# ------------------------------------------------------------------------------------------ the multi-tensor batch
def _set_scales(model, dev, seed=5):
    import learned_quantization_amd as lq
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for s in lq.scale_parameters(model):
            s.copy_((torch.rand(s.shape, generator=g) * 9e-3 + 1e-3).to(dev))


def _mixed_layers(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=9)
    kw = dict(initializer=init, device=dev, scale_gradient="ste", grad_scale=0.37)
    layers = [lq.CustomDenseLayer(units=130, orientation="rowwise", input_shape=257, **kw),
              lq.CustomDenseLayer(units=10, orientation="columnwise", input_shape=133, **kw),
              lq.CustomDenseLayer(units=33, orientation="scalar", input_shape=401, **kw),
              lq.CustomConv2DLayer(filters=32, kernel_size=(3, 3), orientation="channelwise", input_shape=16, **kw),
              lq.CustomConv2DLayerNoBias(filters=8, kernel_size=(7, 7), orientation="channelwise", input_shape=3, **kw)]
    assert not layers[3].kernel.is_contiguous()                                            # stored OIHW (the default)
    return torch.nn.ModuleList(layers)


def _batch_backward(batch, dev, seed=1):
    outs = batch.quantize_all()
    g = torch.Generator(device=dev).manual_seed(seed)
    dys = [torch.randn(o.shape, device=dev, generator=g) * torch.pow(10.0, torch.rand(o.shape, device=dev, generator=g) * 10.0 - 12.0)
           for o in outs]
    torch.autograd.backward(outs, dys)
    return outs, dys


@pytest.mark.parametrize("which", ["cifar", "cifar_rsqrt_rowwise", "mixed"])
def test_batch_against_reference_and_single_tensor_op(dev, which):
    import learned_quantization_amd as lq
    if which == "mixed":
        m = _mixed_layers(dev)
    else:
        lq.reset_layer_names()
        m = lq.build_model("cifar", mode="ste", value=0.0, seed=3, orientation="rowwise" if "rowwise" in which else "channelwise",
                           device=dev, grad_scale="rsqrt_group" if "rsqrt" in which else None)
    _set_scales(m, dev)
    batch = lq.FakeQuantBatch(m)
    assert batch.ste and len(batch.entries) == (12 if which != "mixed" else 9)
    outs, dys = _batch_backward(batch, dev)
    for e, o, d in zip(batch.entries, outs, dys):
        what = f"{which} {e.layer.name} slot {e.slot}"
        k = e.nested.grad_scale_value(e.param.numel())
        assert torch.equal(o, lq.fq_forward(e.param.data, e.nested.scale.data)), what
        assert torch.equal(e.param.grad, d), "dP must be dy"
        ref, terms = ste_reference(e.param.detach().cpu().numpy(), e.nested.scale.detach().cpu().numpy(), d.cpu().numpy(), k)
        got = e.nested.scale.grad.cpu().numpy()
        assert_within_terms(got, ref, terms, what + ": batch vs reference")
        single = lq.fq_scale_grad_ste(e.param.data, e.nested.scale.data, d, k).cpu().numpy()
        assert_within_terms(single, ref, terms, what + ": single-tensor op vs reference")
        assert_within_terms(got, single, terms, what + ": batch vs single-tensor op")
    # run-to-run bit-stable
    first = [e.nested.scale.grad.clone() for e in batch.entries]
    for e in batch.entries:
        e.param.grad = e.nested.scale.grad = None
    outs = batch.quantize_all()
    torch.autograd.backward(outs, dys)
    for e, f in zip(batch.entries, first):
        assert torch.equal(e.nested.scale.grad, f)


def test_batch_refuses_what_it_cannot_do(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    m = lq.build_model("cifar", mode="ste", value=0.0, seed=3, orientation="channelwise", device=dev, kernel_storage="hwio")
    with pytest.raises(ValueError, match='kernel_storage="oihw"'):
        lq.FakeQuantBatch(m)
    lq.reset_layer_names()
    m = lq.build_model("mnist", mode="ste", value=0.0, seed=3, orientation="rowwise", device=dev)
    batch = lq.FakeQuantBatch(m)
    with pytest.raises(ValueError, match="fused=False"):
        lq.BatchedScaleAdam(batch, fused=True)
    lq.BatchedScaleAdam(batch, fused=False)


@pytest.mark.parametrize("kind", ["maxbin", "difference", "inverse"])
def test_batch_stecl_is_ste_part_plus_penalty_part(dev, kind):
    """``stecl``: lq_batch_scale_grad_ste writes ds, lq_batch_penalty_grads(LQ_PENALTY_ACCUMULATE_DS) adds the term's."""
    import learned_quantization_amd as lq
    gamma = 0.37
    lq.reset_layer_names()
    m = lq.build_model("cifar", mode="stecl", value=gamma, seed=3, orientation="channelwise", device=dev)
    _set_scales(m, dev)
    layers = lq.custom_layers_of(m)
    batch = lq.FakeQuantBatch(m)
    outs, dys = _batch_backward(batch, dev)
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
            ref, terms = ste_reference(param.detach().cpu().numpy(), nested.scale.detach().cpu().numpy(), by_param[id(param)].cpu().numpy())
            pen = np.asarray(e64[key], np.float64).reshape(ref.shape)
            pen_terms = np.asarray(e64[key + "_abs"], np.float64).reshape(ref.shape)
            assert np.any(pen != 0.0)
            assert_within_terms(nested.scale.grad.cpu().numpy(), ref + pen, terms + pen_terms, f"{kind} {l.name} {key}")


# ------------------------------------------------------------------------------------------ the trainer
def test_trainer_ste_moves_every_weight_scale(dev, tmp_path):
    """mode="ste" on mnist, 3 steps: every W scale tensor leaves SCALE_INIT (in "cl" without a term none can: the op hands back
    zeros).  Tensor by tensor: an ELEMENT whose gradient is positive is pushed down by Adam and held at SCALE_INIT by the
    MinValueConstraint (min_value == SCALE_INIT, custom_layers.py:158), so not every element can move."""
    from learned_quantization_amd.train import Trainer, synthetic_batch
    for batched in (False, True):
        tr = Trainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path), batched=batched)
        x, y = synthetic_batch("mnist", 16, dev, torch.Generator(device=dev).manual_seed(0))
        losses = [float(tr.step(x, y).detach()) for _ in range(3)]
        assert all(np.isfinite(l) for l in losses)
        for layer in tr.custom_layers:
            sc = layer.nested_q_w_layer.scale.detach()
            moved = int((sc != np.float32(SCALE_INIT)).sum())
            print(f"batched={batched} {layer.name}: {moved} of {sc.numel()} W scale elements left SCALE_INIT")
            assert moved > 0, layer.name
            assert float(sc.min()) >= O.SCALE_MIN


def test_trainer_ste_graphed_step_equals_eager_step(dev, tmp_path):
    """Batched form: the whole step from a hipGraph == the eager step, parameter for parameter, over 3 steps."""
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    res = []
    for graph in (False, True):
        tr = Trainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path), graph=graph, batched=True, seed=7)
        tr.model.eval()
        step = tr.step_graphed if graph else tr.step
        for _ in range(3 + (0 if graph else 3)):          # step_graphed runs 3 eager warm-up steps before it captures
            step(x, y)
        torch.cuda.synchronize()
        res.append({n: p.detach().clone() for n, p in tr.model.named_parameters()})
    moved = False
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), n
        moved = moved or ("scale" in n and bool((res[0][n] != np.float32(SCALE_INIT)).any()))
    assert moved


def _linear_pair(dev, tmp_path, mode, loss, value, **kw):
    from _linear_task import LinearTaskTrainer, make_coefficients
    out = []
    for batched in (False, True):
        tr = LinearTaskTrainer("cifar", mode, value, "channelwise", loss, device=dev, log_dir=str(tmp_path), batched=batched, seed=11, **kw)
        _set_scales(tr.model, dev)
        tr.coefficients = make_coefficients(tr, 1)
        out.append(tr)
    return out


def test_trainer_per_tensor_against_batched_after_one_step(dev, tmp_path):
    """Same state, same injected upstream gradients (tests/_linear_task.py: no convolution library in between), ONE step: every
    scale.grad of both forms within the bound of the reference -- not bitwise, the two forms traverse differently."""
    per_tensor, batched = _linear_pair(dev, tmp_path, "ste", None, 0.0, grad_scale=0.37)
    state = [[(p.detach().cpu().numpy().copy(), n.scale.detach().cpu().numpy().copy())
              for p, n in ((l.kernel, l.nested_q_k_layer), (l.b, l.nested_q_b_layer))] for l in per_tensor.custom_layers]
    for tr in (per_tensor, batched):
        tr.step(None, None)
    coeffs = per_tensor.coefficients[0]
    for li, (la, lb) in enumerate(zip(per_tensor.custom_layers, batched.custom_layers)):
        for slot, (na, nb) in enumerate(((la.nested_q_k_layer, lb.nested_q_k_layer), (la.nested_q_b_layer, lb.nested_q_b_layer))):
            P, s = state[li][slot]
            ref, terms = ste_reference(P, s, coeffs[li][slot].cpu().numpy(), 0.37)
            ga, gb = na.scale.grad.cpu().numpy(), nb.scale.grad.cpu().numpy()
            assert_within_terms(ga, ref, terms, f"{la.name} slot {slot}: per-tensor")
            assert_within_terms(gb, ref, terms, f"{la.name} slot {slot}: batched")
            assert_within_terms(ga, gb, terms, f"{la.name} slot {slot}: per-tensor vs batched")


def test_trainer_stecl_per_tensor_against_batched_after_one_step(dev, tmp_path):
    """``stecl``: per-tensor the term goes through autograd, batched it is injected with LQ_PENALTY_ACCUMULATE_DS."""
    gamma = 0.37
    per_tensor, batched = _linear_pair(dev, tmp_path, "stecl", "difference", gamma)
    layers = per_tensor.custom_layers
    l64 = []
    for l in layers:
        k, ks = l.kernel.detach().cpu().numpy().copy(), l.nested_q_k_layer.scale.detach().cpu().numpy().copy()
        b, bs = l.b.detach().cpu().numpy().copy(), l.nested_q_b_layer.scale.detach().cpu().numpy().copy()
        l64.append((k, ks, O.group_descriptor(k.shape, ks.shape), b, bs, O.group_descriptor(b.shape, bs.shape)))
    g64 = O64.penalty_grads("difference", l64, gamma)
    for tr in (per_tensor, batched):
        tr.step(None, None)
    coeffs = per_tensor.coefficients[0]
    for li, (la, lb, e64) in enumerate(zip(layers, batched.custom_layers, g64)):
        for slot, (na, nb, key) in enumerate(((la.nested_q_k_layer, lb.nested_q_k_layer, "dsK"), (la.nested_q_b_layer, lb.nested_q_b_layer, "dsb"))):
            P, s = l64[li][0 + 3 * slot], l64[li][1 + 3 * slot]
            ref, terms = ste_reference(P, s, coeffs[li][slot].cpu().numpy())
            ref = ref + np.asarray(e64[key], np.float64).reshape(ref.shape)
            terms = terms + np.asarray(e64[key + "_abs"], np.float64).reshape(ref.shape)
            assert_within_terms(na.scale.grad.cpu().numpy(), ref, terms, f"{la.name} slot {slot}: per-tensor")
            assert_within_terms(nb.scale.grad.cpu().numpy(), ref, terms, f"{la.name} slot {slot}: batched")


def test_trainer_refuses_ddp_mode_b(dev, tmp_path):
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="linear in dy"):
        Trainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path), ddp_mode="B")
    with pytest.raises(ValueError, match="linear in dy"):
        Trainer("mnist", "stecl", 1e-7, "rowwise", "inverse", device=dev, log_dir=str(tmp_path), ddp_mode="B", batched=True)


@pytest.mark.parametrize("batched", [False, True])
def test_one_rank_ddp_mode_a_step_equals_the_plain_step(dev, tmp_path, batched):
    """The rule is linear in dy: averaging ds over the ranks is the global-batch gradient.  One rank: the bucket, its exchange
    and the gradient views change nothing, bit for bit."""
    import socket
    import torch.distributed as dist
    from _linear_task import LinearTaskTrainer, make_coefficients, snapshot

    def run(**kw):
        tr = LinearTaskTrainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path), batched=batched, seed=5, **kw)
        _set_scales(tr.model, dev)
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
        assert tr.dp is not None
    finally:
        dist.destroy_process_group()
    for n in plain:
        assert torch.equal(plain[n], dp[n]), n
