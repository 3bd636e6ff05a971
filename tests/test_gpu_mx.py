"""GPU tests of the OCP microscaling quantizer (csrc/lq_mx.hpp on the traversal bodies of csrc/lq_group.hpp; include/lq_hip.h:
lq_fq_forward_mx / lq_fq_backward_mx / lq_scale_init_mx) against tests/_mx_reference.py.

The bar: out, the code view, dP and the saturation counts equal the reference BIT FOR BIT (NaN positional, the sign of zero kept);
ds is held to tests/_bounds.py::assert_within_terms, |got - ref| <= 1e-5 * sum|dy_i r_i|, and is NaN exactly where the reference is;
two calls give the same bits.  The data sets and their conditions are tests/_mx_reference.py's, asserted without a device by
tests/test_mx_cpu.py; the references are computed once per case and shared.

Which case launches which kernel (k_group_mx_cols<BWD, V, TX> / k_group_mx_rows<BWD, V>, forward and backward alike; k_init_cols /
k_init_rows<M = 4 (mx) | 5 (cover)>): cols4 (200, 64, 0, 64), cols1 (96, 130, 0, 96), rows4 (9, 200, 1, 64), rows1 (11, 203, 1, 30)
-- the four window shapes every section below runs on; the rows of FORMS add every team width, the second trip of the column
forms' group loop and the forward's row split."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _mx_reference as X                                                                     # noqa: E402
from _arena import Arena                                                                      # noqa: E402
from _bounds import assert_within_terms, stable_seed                                          # noqa: E402
from _clip_reference import bits_equal                                                        # noqa: E402
from _group_forms import FORM_CASES, LARGE, WINDOW_SHAPES, window_group_case                  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(X.FORMATS)
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _counts(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _mx_pair(dev, P, s, dy, geom, name, sf, k=1.0):
    """Forward (float32 and int32 code views) and backward through the C ABI, where the axis is an argument, each called twice:
    the same bits."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = geom
    fid, sid, st = X.FORMATS[name].id, X.SCALE_FORMATS.index(sf), _hip.stream_ptr(dev)
    Pt, st_, dt = _t(P, dev), _t(s, dev), _t(dy, dev)
    runs = []
    for q_dtype, code in ((torch.float32, _hip.LQ_Q_F32), (torch.int32, _hip.LQ_Q_I32)):
        out, q = torch.empty_like(Pt), torch.empty(Pt.shape, dtype=q_dtype, device=dev)
        dP, ds, cnt = torch.empty_like(Pt), torch.empty_like(st_), torch.empty(st_.shape, dtype=torch.int32, device=dev)
        _hip.check(lib.lq_fq_forward_mx(Pt.data_ptr(), st_.data_ptr(), out.data_ptr(), q.data_ptr(), code, fid, sid, R, C, axis, gs, st),
                   "lq_fq_forward_mx")
        _hip.check(lib.lq_fq_backward_mx(Pt.data_ptr(), st_.data_ptr(), dt.data_ptr(), fid, sid, float(k), dP.data_ptr(), ds.data_ptr(),
                                         cnt.data_ptr(), R, C, axis, gs, st), "lq_fq_backward_mx")
        runs.append((out, q, dP, ds, cnt))
    (out, q, dP, ds, cnt), second = runs
    for what, x, y in zip(("out", "dP", "ds", "clipped"), (out, dP, ds, cnt), (second[0],) + second[2:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"two calls differ in {what}"
    return dict(out=out.cpu().numpy(), code=q.cpu().numpy(), codei=second[1].cpu().numpy(), dP=dP.cpu().numpy(), ds=ds.cpu().numpy(),
                clipped=_counts(cnt))


def _compare(got, ref, what, special=False):
    assert bits_equal(got["out"], ref["out"]), f"{what}: out"
    assert np.array_equal(got["codei"].astype(np.int64), ref["code"]), f"{what}: code (int32 view)"
    assert np.array_equal(got["code"].astype(np.int64), ref["code"]), f"{what}: code (float32 view)"
    assert bits_equal(got["dP"], ref["dP"]), f"{what}: dP"
    assert np.array_equal(got["clipped"].reshape(ref["clipped"].shape), ref["clipped"]), f"{what}: clipped"
    ds, nan = got["ds"].reshape(ref["ds"].shape), np.isnan(ref["ds"])
    assert special or not nan.any()
    assert np.array_equal(np.isnan(ds), nan), f"{what}: ds is NaN in other groups than the reference's"
    assert_within_terms(ds[~nan], ref["ds"][~nan], ref["terms"][~nan], f"{what}: ds")


_REFS = {}


def _case(kind, name, sf, geom):
    """(P, s, dy, ref) of one data set, computed once and shared (never modified)."""
    key = (kind, name, sf, geom)
    if key not in _REFS:
        P, s, dy = (X.gaussian_case if kind == "gauss" else X.loguniform_case)(name, sf, *geom)
        _REFS[key] = (P, s, dy, X.mx_reference(P, s, dy, X.FORMATS[name], sf, geom[2], geom[3], k=0.75))
    return _REFS[key]


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("geom", [c for c in FORM_CASES if c != LARGE], ids=_ids)
def test_parity_every_form(dev, geom):
    """Every launch form of the group-wise rule (team widths, second trip, row split) in fp4_e2m1 / e8m0, Gaussian data."""
    P, s, dy, ref = _case("gauss", "fp4_e2m1", "e8m0", geom)
    _compare(_mx_pair(dev, P, s, dy, geom, "fp4_e2m1", "e8m0", k=0.75), ref, f"{geom}")


@pytest.mark.parametrize("sf", X.SCALE_FORMATS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", WINDOW_SHAPES, ids=_ids)
def test_parity_every_format(dev, geom, name, sf):
    """cols4, cols1, rows4, rows1 in every format and both scale formats, on the Gaussian and the log-uniform set."""
    for kind in ("gauss", "loguniform"):
        P, s, dy, ref = _case(kind, name, sf, geom)
        _compare(_mx_pair(dev, P, s, dy, geom, name, sf, k=0.75), ref, f"{kind} {name} {sf} {geom}")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", X.RAGGED_SHAPES, ids=_ids)
def test_parity_ragged_last_group(dev, geom, name):
    """A last group of 5 rows on the column form, of one float4 on the row form: Gaussian data in every format, the log-uniform
    set where the tensor can hold the format's codes (_mx_reference.loguniform_shapes)."""
    kinds = ("gauss",) + (("loguniform",) if geom in X.loguniform_shapes(name) else ())
    for kind in kinds:
        P, s, dy, ref = _case(kind, name, "e8m0", geom)
        _compare(_mx_pair(dev, P, s, dy, geom, name, "e8m0", k=0.75), ref, f"{kind} {name} {geom}")


def test_int8_code_view_wraps(dev):
    """The int8 view (what weights.npy holds): the two's-complement wrap of the code, fp8 codes of negative values included."""
    import learned_quantization_amd as lq
    geom = WINDOW_SHAPES[2]
    P, s, dy, ref = _case("loguniform", "fp8_e4m3", "e8m0", geom)
    code = lq.fq_forward_mx(_t(P, dev), _t(s, dev), "fp8_e4m3", geom[3], q_dtype=torch.int8)[1].cpu().numpy()
    assert (ref["code"] >= 128).any() and np.array_equal(code, ref["code"].astype(np.uint8).view(np.int8))


# -------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", WINDOW_SHAPES, ids=_ids)
def test_ties(dev, geom, name):
    """Every midpoint of the grid and the first beyond the max, both signs, and the floats next to each, under E8M0 scales: the
    codes and `inside` (dP of dy == 1) bit for bit."""
    P, s, dy, _ = X.ties_case(name, *geom)
    ref = X.mx_reference(P, s, dy, X.FORMATS[name], "e8m0", geom[2], geom[3])
    got = _mx_pair(dev, P, s, dy, geom, name, "e8m0")
    assert np.array_equal(got["codei"].astype(np.int64), ref["code"]), "codes"
    assert np.array_equal(got["dP"] == 1.0, ref["inside"]) and bits_equal(got["dP"], ref["dP"]), "inside"
    _compare(got, ref, f"ties {name} {geom}")


# --------------------------------------------------------------------------------------------------------------- bad inputs
@pytest.mark.parametrize("sf", X.SCALE_FORMATS)
@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e5m2"])
@pytest.mark.parametrize("geom", WINDOW_SHAPES, ids=_ids)
def test_bad_scales_and_special_values(dev, geom, name, sf):
    """Scales that are zero, negative, subnormal, huge, Inf, NaN or outside the fast-division window interleaved with ordinary ones,
    special values planted in P: a bad group equals the reference, and its neighbours are untouched (they equal it too, and are finite)."""
    P, s, dy, bad = window_group_case(stable_seed("mx-window", geom), *geom)
    ref = X.mx_reference(P, s, dy, X.FORMATS[name], sf, geom[2], geom[3])
    got = _mx_pair(dev, P, s, dy, geom, name, sf)
    _compare(got, ref, f"bad {name} {sf} {geom}", special=True)
    assert np.isnan(ref["ds"]).any() and np.isfinite(ref["ds"][~bad]).mean() > 0.5
    good = np.isfinite(ref["ds"])
    assert np.isfinite(got["ds"].reshape(ref["ds"].shape)[good]).all()


# --------------------------------------------------------------------------------------------------------------------- init
def _init_data(R, C, axis, gs, fmt, seed):
    """N(0, 0.05) weights with, in turn over the groups of the first lines: a group of zeros, one with a NaN, one with an Inf, one
    whose largest element is mm * 2^-3 exactly, one of subnormals."""
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((R, C)) * 0.05).astype(np.float32)
    length = R if axis == 0 else C
    gs = min(gs, length)
    nb = -(-length // gs)
    plans = ["zeros", "nan", "inf", "mm", "tiny"]
    if nb * (C if axis == 0 else R) < len(plans):      # a bias: one group, left as it is
        return P
    for j, plan in enumerate(plans):
        g, line = j % nb, j // nb
        sl = slice(g * gs, min((g + 1) * gs, length))
        block = P[sl, line] if axis == 0 else P[line, sl]
        if plan == "zeros":
            block[:] = 0.0
        elif plan == "nan":
            block[0] = np.nan
        elif plan == "inf":
            block[-1] = -np.inf
        elif plan == "mm":
            block[:] = np.clip(block, -0.1, 0.1)
            block[0] = -np.float32(fmt.mm * 2.0 ** -3)
        else:
            block[:] = np.float32(1e-41) * np.sign(block)
    return P


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("geom", WINDOW_SHAPES + [(1, 70, 1, 70)], ids=_ids)
def test_scale_init(dev, geom, name):
    """"mx" and "cover" bit for bit; after "cover" the backward reports no saturated element (groups holding NaN / Inf aside)."""
    from learned_quantization_amd import _hip, ops
    lib = _hip.load()
    fmt = X.FORMATS[name]
    R, C, axis, gs = geom
    P = _init_data(R, C, axis, gs, fmt, stable_seed("mx-init", geom))
    Pt = _t(P, dev)
    for mid, method in enumerate(("mx", "cover")):
        for mv in (ops.SCALE_INIT, float(np.float32(2.0 ** -126))):
            want = X.init_reference(P, fmt, method, axis, gs, mv)
            s = torch.full(want.shape, -1.0, dtype=torch.float32, device=dev)
            _hip.check(lib.lq_scale_init_mx(Pt.data_ptr(), s.data_ptr(), fmt.id, mid, mv, R, C, axis, gs, _hip.stream_ptr(dev)),
                       "lq_scale_init_mx")
            assert bits_equal(s.cpu().numpy(), want), f"{method} {name} {geom} min_value {mv}"
        assert want.size == 1 or (np.isnan(want).sum() == 2 and (want == np.float32(mv)).any())
    fin = np.isfinite(want)
    got = _mx_pair(dev, np.where(np.isfinite(P), P, 0).astype(np.float32), np.where(fin, want, 1.0).astype(np.float32), np.ones_like(P), geom, name, "e8m0")
    assert got["clipped"].reshape(want.shape)[fin].sum() == 0


def test_scale_init_of_a_bias_through_the_ops(dev):
    import learned_quantization_amd as lq
    b = _t(np.linspace(-0.3, 0.2, 70).astype(np.float32), dev)
    s = torch.zeros(1, device=dev)
    for method in ("mx", "cover"):
        lq.scale_init_mx(b, s, "fp4_e2m1", None, method)
        want = X.init_reference(b.cpu().numpy().reshape(1, -1), X.FORMATS["fp4_e2m1"], method, 1, 70, lq.SCALE_INIT)
        assert bits_equal(s.cpu().numpy(), want.reshape(1))


# ---------------------------------------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize("residue", [0, 4])
@pytest.mark.parametrize("geom", [(69, 128, 0, 32), (9, 200, 1, 64)], ids=_ids)
def test_memory_contract(dev, geom, residue):
    """Guard bands around every output of the three calls; residue 4 moves every dense base off the 16-byte grid (scalar forms)."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    name, sf = "fp6_e3m2", "e8m0"
    fmt = X.FORMATS[name]
    R, C, axis, gs = geom
    P, s, dy, ref = _case("gauss", name, sf, geom)
    row = C * 4
    a = Arena(dev)
    a.add("P", "in", data=P, residue=residue, row_bytes=row)
    a.add("s", "in", data=s, row_bytes=s.shape[1] * 4)
    a.add("dy", "in", data=dy, residue=residue, row_bytes=row)
    a.add("out", "out", nbytes=P.nbytes, residue=residue, row_bytes=row)
    a.add("code", "out", nbytes=P.size, residue=residue, row_bytes=C)
    a.add("dP", "out", nbytes=P.nbytes, residue=residue, row_bytes=row)
    a.add("ds", "out", nbytes=s.nbytes, residue=4, row_bytes=s.shape[1] * 4)
    a.add("clipped", "out", nbytes=s.nbytes, residue=8, row_bytes=s.shape[1] * 4)
    a.add("s_init", "out", nbytes=s.nbytes, residue=12, row_bytes=s.shape[1] * 4)
    a.build()
    st = _hip.stream_ptr(dev)
    _hip.check(lib.lq_fq_forward_mx(a.ptr("P"), a.ptr("s"), a.ptr("out"), a.ptr("code"), _hip.LQ_Q_I8, fmt.id, 0, R, C, axis, gs, st), "forward")
    torch.cuda.synchronize(dev)
    a.check("forward", written=["out", "code"])
    _hip.check(lib.lq_fq_backward_mx(a.ptr("P"), a.ptr("s"), a.ptr("dy"), fmt.id, 0, 0.75, a.ptr("dP"), a.ptr("ds"), a.ptr("clipped"),
                                     R, C, axis, gs, st), "backward")
    torch.cuda.synchronize(dev)
    a.check("backward", written=["out", "code", "dP", "ds", "clipped"])
    _hip.check(lib.lq_scale_init_mx(a.ptr("P"), a.ptr("s_init"), fmt.id, 1, 2.0 ** -20, R, C, axis, gs, st), "init")
    torch.cuda.synchronize(dev)
    a.check("init")
    got = dict(out=a.numpy("out", np.float32).reshape(R, C), dP=a.numpy("dP", np.float32).reshape(R, C),
               ds=a.numpy("ds", np.float32), clipped=a.numpy("clipped", np.uint32).astype(np.int64))
    got["code"] = got["codei"] = a.numpy("code", np.uint8).reshape(R, C)
    _compare(got, ref, f"arena {geom} residue {residue}")
    assert bits_equal(a.numpy("s_init", np.float32).reshape(s.shape), X.init_reference(P, fmt, "cover", axis, gs, np.float32(2.0 ** -20)))
    # mask only: ds and clipped NULL, nothing but dP is written
    a.fill("dP", 0x7F), a.fill("ds", 0x7F), a.fill("clipped", 0x7F), a.fill("out", 0x7F), a.fill("code", 0x7F), a.fill("s_init", 0x7F)
    _hip.check(lib.lq_fq_backward_mx(a.ptr("P"), a.ptr("s"), a.ptr("dy"), fmt.id, 0, 0.75, a.ptr("dP"), None, None, R, C, axis, gs, st),
               "mask only")
    torch.cuda.synchronize(dev)
    a.check("mask only", written=["dP"])
    assert bits_equal(a.numpy("dP", np.float32).reshape(R, C), ref["dP"])


# ------------------------------------------------------------------------------------------------------------------- layers
def _load(param_view, nested, P, s, dev):
    with torch.no_grad():
        param_view.copy_(_t(P, dev))
        nested.scale.copy_(_t(s, dev))


@pytest.mark.parametrize("name,sf", [("fp4_e2m1", "e8m0"), ("fp8_e4m3", "fp32")])
def test_dense_layer(dev, name, sf):
    """Dense (70, 40), gs = 32 (axis 0, scale (3, 40)): the autograd output and gradients are the ops'; the bias runs as one group."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomDenseLayer(units=40, orientation="groupwise", element_format=name, scale_format=sf, initializer=lq.RandomNormal(seed=5),
                                input_shape=70, device=dev, grad_scale=0.75)
    nested, nb = layer.nested_q_w_layer, layer.nested_q_b_layer
    assert tuple(nested.scale.shape) == (3, 40) and tuple(nb.scale.shape) == (1,) and layer.group_size == 32
    geom = (70, 40, 0, 32)
    P, s, dy, ref = _case("gauss", name, sf, geom)
    _load(layer.W, nested, P, s, dev)
    rng = np.random.default_rng(2)
    sb = np.float32([2.0 ** -6 * 1.3])
    b = (rng.standard_normal(40) * X.FORMATS[name].max * 2.0 ** -6).astype(np.float32)
    db = rng.standard_normal(40).astype(np.float32)
    _load(layer.b, nb, b, sb, dev)
    bref = X.mx_reference(b.reshape(1, 40), sb.reshape(1, 1), db.reshape(1, 40), X.FORMATS[name], sf, 1, 40, k=0.75)
    qw, qb = layer.quantized_parameters()
    assert bits_equal(qw.detach().cpu().numpy(), ref["out"]) and bits_equal(qb.detach().cpu().numpy().reshape(1, 40), bref["out"])
    ((qw * _t(dy, dev)).sum() + (qb * _t(db, dev)).sum()).backward()
    assert bits_equal(layer.W.grad.cpu().numpy(), ref["dP"]) and bits_equal(layer.b.grad.cpu().numpy().reshape(1, 40), bref["dP"])
    assert_within_terms(nested.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], "dense ds")
    assert_within_terms(nb.scale.grad.cpu().numpy(), bref["ds"], bref["terms"], "bias ds")
    dP, ds, _ = lq.fq_backward_mx(layer.W.data, nested.scale.data, _t(dy, dev), name, 32, sf, grad_scale=0.75)
    assert torch.equal(dP, layer.W.grad) and torch.equal(ds, nested.scale.grad)
    assert np.array_equal(nested.quantized_integers(layer.W.data, torch.int32).cpu().numpy(), ref["code"])
    assert np.array_equal(nb.quantized_integers(layer.b.data, torch.int32).cpu().numpy().reshape(1, 40), bref["code"])
    assert bref["clipped"].sum() > 0 and bref["inside"].sum() > 0
    x = torch.ones(3, 70, device=dev)
    assert torch.equal(layer(x), torch.matmul(x, nested(layer.W)) + nb(layer.b))
    with pytest.raises(ValueError, match="quant_stats on a layer with an element format"):
        nested.quant_stats(layer.W.data)
    assert lq.quant_stats(layer) == {}
    layer.init_scales("cover")
    want = X.init_reference(P, X.FORMATS[name], "cover", 0, 32, lq.SCALE_INIT)
    assert bits_equal(nested.scale.detach().cpu().numpy(), want)
    assert bits_equal(nb.scale.detach().cpu().numpy(), X.init_reference(b.reshape(1, 40), X.FORMATS[name], "cover", 1, 40, lq.SCALE_INIT).reshape(1))


def test_conv_layer(dev):
    """Conv 3 x 3 x 5 x 8 stored OIHW, gs = 32 (axis 1, C = 45: a last group of 13, rows1; scale (8, 2))."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    name, sf = "fp6_e2m3", "e8m0"
    layer = lq.CustomConv2DLayer(filters=8, orientation="groupwise", element_format=name, initializer=lq.RandomNormal(seed=6), input_shape=5,
                                 device=dev)
    nested = layer.nested_q_k_layer
    assert tuple(layer.kernel.shape) == (3, 3, 5, 8) and tuple(nested.scale.shape) == (8, 2)
    geom = (8, 45, 1, 32)
    P, s, dy, ref = _case("gauss", name, sf, geom)
    oihw = lambda a: a.reshape(8, 5, 3, 3)                                        # noqa: E731  the memory-order matrix as OIHW
    _load(layer.kernel.data.permute(3, 2, 0, 1), nested, oihw(P), s, dev)
    w = layer.quantized_parameters()[0]
    assert tuple(w.shape) == (8, 5, 3, 3) and w.is_contiguous()
    assert bits_equal(w.detach().cpu().numpy().reshape(8, 45), ref["out"])
    (w * _t(oihw(dy), dev)).sum().backward()
    assert bits_equal(layer.kernel.grad.permute(3, 2, 0, 1).contiguous().cpu().numpy().reshape(8, 45), ref["dP"])
    ref1 = X.mx_reference(P, s, dy, X.FORMATS[name], sf, 1, 32, k=1.0)
    assert_within_terms(nested.scale.grad.cpu().numpy(), ref1["ds"], ref1["terms"], "conv ds")
    code = nested.quantized_integers(layer.kernel.data, torch.int32).permute(3, 2, 0, 1).contiguous().cpu().numpy().reshape(8, 45)
    assert np.array_equal(code, ref["code"])
    y = layer(torch.ones(2, 5, 8, 8, device=dev))
    assert tuple(y.shape) == (2, 8, 8, 8) and bool(torch.isfinite(y).all())


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """Trainer(config="mnist", mode="ste", element_format="fp4_e2m1", scale_init="cover"), eager and graphed, three steps each from
    the same state (after the three eager warm-up steps of step_graphed)."""
    from learned_quantization_amd.train import Trainer, synthetic_batch
    gen = torch.Generator(device=dev).manual_seed(0)
    y = synthetic_batch("mnist", 32, dev, gen)[1]
    x = torch.randn(32, 1, 28, 28, device=dev, generator=gen)
    runs = []
    for graph in (False, True):
        tr = Trainer(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path_factory.mktemp("mx")), graph=graph,
                     seed=7, element_format="fp4_e2m1", scale_init="cover", lr=1e-3)
        tr.model.eval()
        start = [l.nested_q_w_layer.scale.detach().clone() for l in tr.custom_layers]
        step = tr.step_graphed if graph else tr.step
        losses = [step(x, y).detach().clone() for _ in range(3 + (0 if graph else 3))]
        torch.cuda.synchronize()
        runs.append((tr, losses[-3:], start))
    return runs


def test_trainer_eager_and_graphed(dev, trained):
    """Finite losses, every layer's scales have gradients and some move; graphed losses and parameters equal the eager ones bit
    for bit."""
    (eager, le, start), (graphed, lg, _) = trained
    assert all(np.isfinite(float(a)) for a in le)
    for a, b in zip(le, lg):
        assert torch.equal(a, b), f"losses differ: {float(a)!r} {float(b)!r}"
    for (n, p), (_, p2) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), n
    for layer, s0 in zip(eager.custom_layers, start):
        scale = layer.nested_q_w_layer.scale
        assert layer.element_format == "fp4_e2m1" and layer.group_size == 32
        assert tuple(scale.shape) == ((25, 128) if layer.W.shape[0] == 784 else (4, 10))
        assert scale.grad is not None and bool((scale.grad != 0).any()) and bool((scale.detach() != s0).any()), layer.name
        assert bool((s0 == torch.exp2(torch.round(torch.log2(s0)))).all()), "cover writes powers of two"


# ------------------------------------------------------------------------------------------------------------------- export
@pytest.mark.parametrize("name,sf", [("fp4_e2m1", "e8m0"), ("fp8_e4m3", "e8m0"), ("fp8_e4m3", "fp32")])
def test_export_round_trip(dev, tmp_path, name, sf):
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    fmt = X.FORMATS[name]
    lq.reset_layer_names()
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format=name, scale_format=sf, scale_init="mx")
    with torch.no_grad():      # off the powers of two: what training leaves behind
        for _, _, nested in export.quantized_tensors(model):
            nested.scale.mul_(torch.empty_like(nested.scale).uniform_(0.8, 1.3))
    tensors = export.quantized_tensors(model)
    d = str(tmp_path)
    # the reference-format file: the codes cast to int8
    lq.save_compress_parameters(model, d)
    weights = np.load(os.path.join(d, "weights.npy"), allow_pickle=True).item()
    for tname, param, nested in tensors:
        code = nested.quantized_integers(param.data, torch.int32).cpu().numpy()
        assert weights[tname].dtype == np.int8 and np.array_equal(weights[tname], code.astype(np.uint8).view(np.int8)), tname
    info = lq.save_packed_parameters(model, d)
    assert info["bits_per_weight"] == fmt.bits
    with np.load(os.path.join(d, "weights_packed.npz")) as z:
        manifest = export.read_packed_manifest(z)
        for e, (tname, param, nested) in zip(manifest["tensors"], tensors):
            assert e["element_format"] == name and e["scale_format"] == sf and e.get("group_size") == nested.group_size
            assert e["bits"] == fmt.bits and e["qmin"] == 0
            sc, codes = z[tname + ".scale"], z[tname + ".codes"]
            assert sc.shape == tuple(nested.scale.shape) and sc.dtype == (np.uint8 if sf == "e8m0" else np.float32)
            # the size is the bit count: bits * numel (to the 32-bit word) + 8 (or 32) bits per group
            assert codes.nbytes == 4 * -(-fmt.bits * param.numel() // 32) and sc.nbytes == nested.scale.numel() * (1 if sf == "e8m0" else 4)
            if sf == "e8m0":
                want = X.e8m0_round(nested.scale.detach().cpu().numpy())
                assert np.array_equal((sc.astype(np.uint32) << 23).view(np.float32), want)
    lq.reset_layer_names()
    fresh = lq.build_model("mnist", mode="ste", value=0.0, seed=99, device=dev, element_format=name, scale_format=sf)
    lq.load_packed_parameters(fresh, d)
    for (tname, p0, n0), (_, p1, n1) in zip(tensors, export.quantized_tensors(fresh)):
        assert torch.equal(n0(p0).detach().view(torch.int32), n1(p1).detach().view(torch.int32)), f"{tname}: out after the restore"
        assert torch.equal(n0.quantized_integers(p0.data, torch.int32), n1.quantized_integers(p1.data, torch.int32)), f"{tname}: codes"
        want = X.effective_scale(n0.scale.detach().cpu().numpy(), sf)
        assert bits_equal(n1.scale.detach().cpu().numpy(), want), f"{tname}: s = s_eff"
    x = torch.rand(4, 1, 28, 28, device=dev) * 255.0
    model.eval(), fresh.eval()
    with torch.no_grad():
        assert torch.equal(model(x), fresh(x))
    # another format, scale format or group size, or an integer model: refused, the model left untouched
    others = [dict(element_format="fp6_e2m3" if name != "fp6_e2m3" else "fp6_e3m2", scale_format=sf),
              dict(element_format=name, scale_format="fp32" if sf == "e8m0" else "e8m0"),
              dict(element_format=name, scale_format=sf, group_size=16), dict(bits=4, group_size=32)]
    for kw, needle in zip(others, ("element_format", "scale_format", "group_size", "element_format")):
        lq.reset_layer_names()
        other = lq.build_model("mnist", mode="ste", value=0.0, seed=99, device=dev, **kw)
        before = other.dense_1.W.detach().clone()
        with pytest.raises(ValueError, match=needle):
            lq.load_packed_parameters(other, d)
        assert torch.equal(before, other.dense_1.W.detach())


def test_export_refuses_what_it_cannot_store(dev, tmp_path):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="cover")
    with torch.no_grad():
        model.dense_2.W[3, 1] = float("nan")
    with pytest.raises(ValueError, match="custom_dense_layer_1/W.*no finite value"):
        lq.save_packed_parameters(model, str(tmp_path))
    with torch.no_grad():
        model.dense_2.W[3, 1] = 0.0
        model.dense_1.nested_q_w_layer.scale[2, 5] = 1e-40
    with pytest.raises(ValueError, match="custom_dense_layer/W.*no valid e8m0 scale"):
        lq.save_packed_parameters(model, str(tmp_path))
    assert not os.path.exists(os.path.join(str(tmp_path), "weights_packed.npz"))


def test_export_without_element_formats_is_unchanged(dev, tmp_path):
    """A model without element formats: both files hold exactly what they held before the formats existed -- rebuilt entry by entry
    with the ops that path uses (npz members carry a time stamp: the members are compared, in order, not the zip's bytes)."""
    import io
    import json
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    lq.reset_layer_names()
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, bits=4, group_size=32, scale_init="absmax")
    tensors = export.quantized_tensors(model)
    lq.save_compress_parameters(model, str(tmp_path))
    want = {name: np.ascontiguousarray(n.quantized_integers(p.data, torch.int8).cpu().numpy()) for name, p, n in tensors}
    buf = io.BytesIO()
    np.save(buf, want)
    assert open(os.path.join(str(tmp_path), "weights.npy"), "rb").read() == buf.getvalue()
    lq.save_packed_parameters(model, str(tmp_path))
    entries, arrays = [], {}
    unit = torch.ones(1, device=dev)
    for name, p, n in tensors:
        q = n.quantized_integers(p.data, torch.float32)
        u = unit if n.group_size is not None else torch.ones_like(n.scale.data)
        lo, hi = (int(v) for v in lq.q_minmax(q, u).tolist())
        entries.append({"name": name, "shape": list(p.shape), "scale_shape": list(n.scale.shape), "orientation": n.orientation,
                        "qmin": lo, "bits": (hi - lo).bit_length(), "numel": int(p.numel())})
        if n.group_size is not None:
            entries[-1]["group_size"] = n.group_size
        arrays[name + ".codes"] = lq.q_pack(q, u, qmin=lo, bits=entries[-1]["bits"])[0].cpu().numpy().view(np.uint32)
        arrays[name + ".scale"] = n.scale.detach().cpu().numpy()
    manifest = {"format": "lq-packed", "version": 1, "tensors": entries, "state": []}
    with np.load(os.path.join(str(tmp_path), "weights_packed.npz")) as z:
        assert z.files == ["manifest"] + list(arrays)
        assert bytes(z["manifest"]) == json.dumps(manifest).encode("utf-8")
        for key, a in arrays.items():
            assert z[key].dtype == a.dtype and z[key].shape == a.shape and z[key].tobytes() == a.tobytes(), key
