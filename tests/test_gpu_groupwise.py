"""GPU tests of the group-wise (block) scales of the clipped b-bit quantizer (include/lq_hip.h: lq_fq_forward_group,
lq_fq_backward_group) from the C ABI up to the layers, the training harness and the export.

The reference is the NumPy restatement tests/_group_reference.py (pinned by tests/test_groupwise_cpu.py).  The bar is the same in
every case: out, q, dP and clipped equal it BIT FOR BIT; ds is held to tests/_bounds.py::assert_within_terms,
|got - ref| <= 1e-5 * sum|dy_i r_i| (floor 2^-136).  Inputs (``make_case``): per-group s = 2^U(-9, -5), P = N(0, 1) * 8 s,
seeds from ``stable_seed``; at 4 bits about a third of the elements clip.

The condition on the inputs is checked on the reference before any kernel runs: at least 90 % of the groups OF AT LEAST 8
ELEMENTS hold both clipped and inside elements, and overall at least a tenth of the elements is clipped and a tenth inside.
(A group of one element -- the gs = 1 cases -- can never hold both; a group of 4 does in 78 % of the draws.  The per-group form
of the condition is therefore asked of the groups that can meet it.)

Special values: a NaN in P makes exactly its own group's ds NaN.  A +Inf in P saturates (q0 = +Inf is clamped to qmax by the
comparisons, r = qmax): by the definition, and in the reference, its group's ds stays finite; the test plants both and holds
every group, the two included, to the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _arena import Arena                                                                  # noqa: E402
from _bounds import assert_within_terms, stable_seed                                      # noqa: E402
from _clip_reference import bits_equal, edge_table                                        # noqa: E402
from _group_reference import check_condition as _check_condition                          # noqa: E402
from _group_reference import expand_scale, group_reference, make_case, scale_shape        # noqa: E402

pytestmark = pytest.mark.gpu
LIM = 1 << 24
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731

AXIS0 = [(37, 5, 8), (256, 260, 32), (130, 1028, 128), (300, 64, 1), (96, 130, 96), (50, 12, 64), (784, 128, 64), (4608, 512, 128)]
AXIS1 = [(7, 27, 8), (64, 576, 128), (33, 4100, 128), (40, 64, 4), (16, 100, 1), (20, 96, 96), (512, 4608, 128), (512, 4608, 100)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_CASES = {}


def _case(R, C, axis, gs, qmin=-8, qmax=7, rounding="floor", k=1.0):
    """Inputs and reference of one case, computed once and shared (never modified)."""
    key = (R, C, axis, gs, qmin, qmax, rounding, k)
    if key not in _CASES:
        P, s, dy = make_case(stable_seed("groupwise", R, C, axis, gs), R, C, axis, gs)
        ref = group_reference(P, s, dy, qmin, qmax, axis, gs, k=k, rounding=rounding)
        _check_condition(ref, R, C, axis, gs, f"{key}")
        _CASES[key] = (P, s, dy, ref)
    return _CASES[key]


def _ratio(got, ref, terms):
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(got, np.float64) - ref) / np.maximum(terms, 1e-300)
    return float(np.nanmax(r)) if r.size else 0.0


def _counts(clipped):
    return clipped.cpu().numpy().view(np.uint32).astype(np.int64)


def _check_case(dev, R, C, axis, gs, qmin=-8, qmax=7, rounding="floor", k=1.0):
    import learned_quantization_amd as lq
    what = f"({R}, {C}) axis {axis} gs {gs} [{qmin}, {qmax}] {rounding}"
    P, s, dy, ref = _case(R, C, axis, gs, qmin, qmax, rounding, k)
    Pt, st, dt = _t(P, dev), _t(s, dev), _t(dy, dev)
    out, q = lq.fq_forward_group(Pt, st, qmin, qmax, gs, q_dtype=torch.int32, rounding=rounding)
    assert torch.equal(out, lq.fq_forward_group(Pt, st, qmin, qmax, gs, rounding=rounding)), f"{what}: two forward calls differ"
    assert bits_equal(out.cpu().numpy(), ref["out"]), f"{what}: out"
    assert np.array_equal(q.cpu().numpy(), ref["q"].astype(np.int32)), f"{what}: q"
    dP, ds, clipped = lq.fq_backward_group(Pt, st, dt, qmin, qmax, gs, grad_scale=k, want_clipped=True, rounding=rounding)
    dP2, ds2, clipped2 = lq.fq_backward_group(Pt, st, dt, qmin, qmax, gs, grad_scale=k, want_clipped=True, rounding=rounding)
    assert torch.equal(dP, dP2) and torch.equal(ds, ds2) and torch.equal(clipped, clipped2), f"{what}: two backward calls differ"
    assert ds.shape == st.shape and clipped.shape == st.shape and dP.shape == Pt.shape
    assert bits_equal(dP.cpu().numpy(), ref["dP"]), f"{what}: dP"
    assert np.array_equal(_counts(clipped), ref["clipped"]), f"{what}: clipped"
    print(f"{what}: max err / sum|terms| = {_ratio(ds.cpu().numpy(), ref['ds'], ref['terms']):.3e}")
    assert_within_terms(ds.cpu().numpy(), ref["ds"], ref["terms"], f"{what}: ds")
    return Pt, st, dt, ref, (dP, ds, clipped)


# ------------------------------------------------------------------------------------------------------------ the two axes
@pytest.mark.parametrize("shape", AXIS0, ids=_ids)
def test_axis0_signed_floor(dev, shape):
    _check_case(dev, shape[0], shape[1], 0, shape[2])


@pytest.mark.parametrize("variant", [((-8, 7), "nearest"), ((0, 15), "floor")], ids=["nearest", "unsigned"])
@pytest.mark.parametrize("shape", AXIS0[:4], ids=_ids)
def test_axis0_nearest_and_unsigned(dev, shape, variant):
    (qmin, qmax), rounding = variant
    _check_case(dev, shape[0], shape[1], 0, shape[2], qmin, qmax, rounding)


@pytest.mark.parametrize("shape", AXIS1, ids=_ids)
def test_axis1_signed_floor(dev, shape):
    _check_case(dev, shape[0], shape[1], 1, shape[2])


@pytest.mark.parametrize("shape", [(7, 27, 8), (64, 576, 128), (40, 64, 4)], ids=_ids)
def test_axis1_nearest(dev, shape):
    _check_case(dev, shape[0], shape[1], 1, shape[2], rounding="nearest")


# --------------------------------------------------------------------- raw C-ABI calls inside a poisoned arena (misaligned bases, guards)
def _raw_case(dev, R, C, axis, gs, residue, want_ds=True, want_clipped=True):
    """Forward and backward through the C ABI with every dense tensor at ``residue`` bytes off the 16-byte grid, each region
    between guard bands: the results equal the reference, every output is fully written, no guard byte is touched."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    P, s, dy, ref = _case(R, C, axis, gs)
    nbytes, row = P.nbytes, C * 4
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=residue, row_bytes=row)
    ar.add("s", "in", data=s)
    ar.add("dy", "in", data=dy, residue=residue, row_bytes=row)
    ar.add("out", "out", nbytes=nbytes, residue=residue, row_bytes=row)
    ar.add("q", "out", nbytes=nbytes)
    ar.add("dP", "out", nbytes=nbytes, residue=residue, row_bytes=row)
    ar.add("ds", "out", nbytes=s.nbytes)
    ar.add("clipped", "out", nbytes=s.nbytes)
    need = lib.lq_group_workspace_bytes(R, C, axis, gs)
    if need:
        ar.add("ws", "ws", nbytes=need)
    ar.build()
    assert ar.ptr("P") % 16 == residue and ar.ptr("dP") % 16 == residue
    st = _hip.stream_ptr(dev)
    _hip.check(lib.lq_fq_forward_group(ar.ptr("P"), ar.ptr("s"), ar.ptr("out"), ar.ptr("q"), _hip.LQ_Q_I32, -8, 7, 0, R, C, axis, gs, st),
               "lq_fq_forward_group")
    _hip.check(lib.lq_fq_backward_group(ar.ptr("P"), ar.ptr("s"), ar.ptr("dy"), -8, 7, 0, 1.0, ar.ptr("dP"),
                                        ar.ptr("ds") if want_ds else None, ar.ptr("clipped") if want_clipped else None,
                                        ar.ptr("ws") if need else None, need, R, C, axis, gs, st), "lq_fq_backward_group")
    torch.cuda.synchronize(dev)
    written = ["out", "q", "dP"] + (["ds"] if want_ds else []) + (["clipped"] if want_clipped else [])
    ar.check(f"({R}, {C}) axis {axis} gs {gs} residue {residue}", written=written)
    assert bits_equal(ar.numpy("out", np.float32).reshape(R, C), ref["out"])
    assert np.array_equal(ar.numpy("q", np.int32).reshape(R, C), ref["q"].astype(np.int32))
    assert bits_equal(ar.numpy("dP", np.float32).reshape(R, C), ref["dP"])
    if want_ds:
        assert_within_terms(ar.numpy("ds", np.float32), ref["ds"], ref["terms"], "ds")
    if want_clipped:
        assert np.array_equal(ar.numpy("clipped", np.uint32).astype(np.int64).reshape(s.shape), ref["clipped"])
    return ar


@pytest.mark.parametrize("case", [(256, 260, 0, 32), (33, 4100, 1, 128)], ids=_ids)
def test_misaligned_base(dev, case):
    """P, dy, out and dP one float off the 16-byte grid: the scalar forms, same results."""
    _raw_case(dev, *case, residue=4)


@pytest.mark.parametrize("case", [(37, 5, 0, 8), (256, 260, 0, 32), (96, 130, 0, 96), (7, 27, 1, 8), (64, 576, 1, 128), (33, 4100, 1, 128)], ids=_ids)
def test_guard_bands_and_optional_outputs(dev, case):
    """Aligned bases between guard bands; ds == NULL (mask only) and clipped == NULL leave their regions untouched."""
    _raw_case(dev, *case, residue=0)
    _raw_case(dev, *case, residue=0, want_ds=False)
    _raw_case(dev, *case, residue=0, want_clipped=False)
    _raw_case(dev, *case, residue=0, want_ds=False, want_clipped=False)


def test_workspace_contract(dev):
    """Every tested shape: the workspace size is what the backward is allowed to touch; with a size of 0 the call takes NULL (the
    raw cases above pass NULL then).  A nonzero size is exercised by the raw cases with a poisoned workspace region."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    sizes = {(R, C, axis, gs): lib.lq_group_workspace_bytes(R, C, axis, gs)
             for axis, shapes in ((0, AXIS0), (1, AXIS1)) for R, C, gs in shapes}
    print(sizes)
    for (R, C, axis, gs), need in sizes.items():
        if need and R * C <= 1 << 20:
            _raw_case(dev, R, C, axis, gs, residue=0)


# ------------------------------------------------------------------------------------------ cross-checks against the shipped ops
def _cross(dev, R, C, axis, gs, one_axis_view):
    import learned_quantization_amd as lq
    Pt, st, dt, ref, (dP, ds, clipped) = _check_case(dev, R, C, axis, gs)
    out = lq.fq_forward_group(Pt, st, -8, 7, gs)
    shape_p, shape_s = one_axis_view
    P1, s1, d1 = Pt.reshape(shape_p), st.reshape(shape_s), dt.reshape(shape_p)
    out1 = lq.fq_forward_clip(P1, s1, -8, 7)
    dP1, ds1, clipped1 = lq.fq_backward_clip(P1, s1, d1, -8, 7, want_clipped=True)
    assert torch.equal(out.reshape(shape_p), out1) and bits_equal(out.cpu().numpy().reshape(shape_p), out1.cpu().numpy())
    assert bits_equal(dP.cpu().numpy().reshape(shape_p), dP1.cpu().numpy())
    assert torch.equal(clipped.reshape(shape_s), clipped1)
    assert_within_terms(ds1.cpu().numpy(), ref["ds"], ref["terms"], "the shipped op's ds")
    assert_within_terms(ds.cpu().numpy(), ref["ds"], ref["terms"], "the group-wise ds")


def test_axis0_whole_columns_is_columnwise(dev):
    _cross(dev, 96, 130, 0, 96, ((96, 130), (1, 130)))


def test_axis1_whole_rows_is_rowwise(dev):
    _cross(dev, 20, 96, 1, 96, ((20, 96), (20, 1)))


def test_axis1_dividing_groups_is_reshaped_rowwise(dev):
    _cross(dev, 40, 64, 1, 4, ((40 * 16, 4), (40 * 16, 1)))
    _cross(dev, 64, 576, 1, 64, ((64 * 9, 64), (64 * 9, 1)))


# ---------------------------------------------------------------------------------------------------- edges and special values
@pytest.mark.parametrize("rng_", [(-8, 7), (0, 15), (-2, 1)], ids=_ids)
@pytest.mark.parametrize("axis", [0, 1])
def test_range_edges_at_power_of_two_scales(dev, axis, rng_):
    import learned_quantization_amd as lq
    qmin, qmax = rng_
    t, q_want, inside_want = edge_table(qmin, qmax, 1.0)               # 11 quotients around both edges
    n = t.size
    R, C, gs = (n, 6, 4) if axis == 0 else (6, n, 4)
    along = lambda v: np.broadcast_to(v.reshape((n, 1) if axis == 0 else (1, n)), (R, C)).copy()      # noqa: E731  the table along the groups' axis
    tm, qm, im = along(t), along(q_want), along(inside_want)
    rng = np.random.default_rng(stable_seed("edges", axis, rng_))
    s = np.exp2(rng.integers(-9, -4, size=scale_shape(R, C, axis, gs))).astype(np.float32)
    sb = expand_scale(s, R, C, axis, gs)
    P = tm * sb
    assert np.array_equal(P / sb, tm)                                   # the quotients are exact
    dy = rng.standard_normal((R, C)).astype(np.float32)
    ref = group_reference(P, s, dy, qmin, qmax, axis, gs)
    assert np.array_equal(ref["q"], qm) and np.array_equal(ref["inside"], im)
    out, q = lq.fq_forward_group(_t(P, dev), _t(s, dev), qmin, qmax, gs, q_dtype=torch.float32)
    dP, ds, clipped = lq.fq_backward_group(_t(P, dev), _t(s, dev), _t(dy, dev), qmin, qmax, gs, want_clipped=True)
    assert np.array_equal(q.cpu().numpy(), qm) and bits_equal(out.cpu().numpy(), qm * sb)
    assert bits_equal(dP.cpu().numpy(), np.where(im, dy, np.float32(0.0))) and not np.any(np.signbit(dP.cpu().numpy()[~im]))
    assert np.array_equal(_counts(clipped), ref["clipped"])
    assert_within_terms(ds.cpu().numpy(), ref["ds"], ref["terms"], "ds on the edge table")


@pytest.mark.parametrize("case", [(37, 5, 0, 8), (256, 260, 0, 32), (7, 27, 1, 8), (64, 576, 1, 128)], ids=_ids)
def test_nan_and_inf_stay_in_their_groups(dev, case):
    import learned_quantization_amd as lq
    R, C, axis, gs = case
    P, s, dy, clean = _case(R, C, axis, gs)
    P = P.copy()
    nan_at, inf_at = ((1, 2), (R - 1, C - 1))                           # first group of a line and the (ragged) last one
    P[nan_at], P[inf_at] = np.nan, np.inf
    ref = group_reference(P, s, dy, -8, 7, axis, gs)
    g_nan = (nan_at[0] // gs, nan_at[1]) if axis == 0 else (nan_at[0], nan_at[1] // gs)
    g_inf = (inf_at[0] // gs, inf_at[1]) if axis == 0 else (inf_at[0], inf_at[1] // gs)
    assert g_nan != g_inf
    want_nan = np.zeros(s.shape, bool)
    want_nan[g_nan] = True
    assert np.array_equal(np.isnan(ref["ds"]), want_nan)               # the reference: NaN poisons its group, +Inf saturates
    assert ref["q"][inf_at] == 7 and not ref["inside"][inf_at] and np.isfinite(ref["ds"][g_inf])
    out, q = lq.fq_forward_group(_t(P, dev), _t(s, dev), -8, 7, gs, q_dtype=torch.float32)
    dP, ds, clipped = lq.fq_backward_group(_t(P, dev), _t(s, dev), _t(dy, dev), -8, 7, gs, want_clipped=True)
    assert bits_equal(out.cpu().numpy(), ref["out"]) and bits_equal(q.cpu().numpy(), ref["q"])
    assert bits_equal(dP.cpu().numpy(), ref["dP"]) and np.array_equal(_counts(clipped), ref["clipped"])
    got = ds.cpu().numpy()
    assert np.array_equal(np.isnan(got), want_nan)
    keep = ~want_nan
    assert_within_terms(got[keep], ref["ds"][keep], ref["terms"][keep], "ds of the other groups")
    untouched = keep.copy()
    untouched[g_inf] = False
    assert np.array_equal(ref["ds"][untouched], clean["ds"][untouched])  # every other group is the clean case's


@pytest.mark.parametrize("case", [(37, 5, 0, 8), (7, 27, 1, 8), (64, 576, 1, 128)], ids=_ids)
def test_degenerate_and_widest_range(dev, case):
    import learned_quantization_amd as lq
    R, C, axis, gs = case
    P, s, dy, _ = _case(R, C, axis, gs)
    Pt, st, dt = _t(P, dev), _t(s, dev), _t(dy, dev)
    ref = group_reference(P, s, dy, 3, 3, axis, gs)                     # qmin == qmax
    out = lq.fq_forward_group(Pt, st, 3, 3, gs)
    dP, ds, clipped = lq.fq_backward_group(Pt, st, dt, 3, 3, gs, want_clipped=True)
    assert bits_equal(out.cpu().numpy(), ref["out"]) and np.array_equal(out.cpu().numpy(), np.float32(3.0) * expand_scale(s, R, C, axis, gs))
    assert bits_equal(dP.cpu().numpy(), ref["dP"]) and np.array_equal(_counts(clipped), ref["clipped"])
    assert_within_terms(ds.cpu().numpy(), ref["ds"], ref["terms"], "ds of the degenerate range")
    ref = group_reference(P, s, dy, -LIM, LIM, axis, gs)                # the widest range: nothing clips
    out = lq.fq_forward_group(Pt, st, -LIM, LIM, gs)
    dP, ds, clipped = lq.fq_backward_group(Pt, st, dt, -LIM, LIM, gs, want_clipped=True)
    assert torch.equal(dP, dt) and int(clipped.sum()) == 0 and bits_equal(out.cpu().numpy(), ref["out"])
    assert_within_terms(ds.cpu().numpy(), ref["ds"], ref["terms"], "ds of the widest range")
    # out == fq_forward of the expanded problem: every group a tensor of its own under a one-axis scale
    length = R if axis == 0 else C
    for g in range(scale_shape(R, C, axis, gs)[axis]):
        sl = slice(g * gs, min((g + 1) * gs, length))
        if axis == 0:
            want = lq.fq_forward(Pt[sl, :].contiguous(), st[g:g + 1, :].contiguous())
            assert torch.equal(out[sl, :], want)
        else:
            want = lq.fq_forward(Pt[:, sl].contiguous(), st[:, g:g + 1].contiguous())
            assert torch.equal(out[:, sl], want)


@pytest.mark.parametrize("case", [(256, 260, 0, 32), (33, 4100, 1, 128)], ids=_ids)
def test_grad_scale_factor_and_mask_only(dev, case):
    import learned_quantization_amd as lq
    R, C, axis, gs = case
    Pt, st, dt, ref, _ = _check_case(dev, R, C, axis, gs, k=0.37)
    dP, ds, clipped = lq.fq_backward_group(Pt, st, dt, -8, 7, gs, want_ds=False)
    assert ds is None and clipped is None and bits_equal(dP.cpu().numpy(), ref["dP"])
    dP, ds, clipped = lq.fq_backward_group(Pt, st, dt, -8, 7, gs, want_ds=False, want_clipped=True)
    assert ds is None and np.array_equal(_counts(clipped), ref["clipped"]) and bits_equal(dP.cpu().numpy(), ref["dP"])


# ------------------------------------------------------------------------------------------------------- autograd and layers
def _load_case(param_view, nested, P, s, dev):
    with torch.no_grad():
        param_view.copy_(_t(P, dev))
        nested.scale.copy_(_t(s, dev))


@pytest.mark.parametrize("grad_scale", [1.0, "rsqrt_group"])
def test_dense_layer(dev, grad_scale):
    """Dense 784 x 128, gs = 64 (axis 0, scale (13, 128)): forward and backward against the reference, P.grad is the masked dy."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomDenseLayer(units=128, orientation="groupwise", group_size=64, initializer=lq.RandomNormal(seed=5), input_shape=784,
                                device=dev, scale_gradient="ste", grad_scale=grad_scale, bits=4)
    nested = layer.nested_q_w_layer
    assert tuple(nested.scale.shape) == (13, 128) and tuple(layer.nested_q_b_layer.scale.shape) == (1,)
    k = 1.0 if grad_scale == 1.0 else 1.0 / np.sqrt(784 * 128 / (13 * 128))
    assert nested.grad_scale_value(layer.W.numel()) == k
    P, s, dy, ref = _case(784, 128, 0, 64, k=k)
    _load_case(layer.W, nested, P, s, dev)
    qw = layer.quantized_parameters()[0]
    assert bits_equal(qw.detach().cpu().numpy(), ref["out"])
    (qw * _t(dy, dev)).sum().backward()
    assert bits_equal(layer.W.grad.cpu().numpy(), ref["dP"])
    assert_within_terms(nested.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], f"dense ds, grad_scale {grad_scale}")
    assert np.array_equal(nested.quantized_integers(layer.W.data, torch.int32).cpu().numpy(), ref["q"].astype(np.int32))
    x = torch.ones(3, 784, device=dev)
    y = layer(x)
    assert torch.equal(y, torch.matmul(x, nested(layer.W)) + layer.nested_q_b_layer(layer.b))


def test_conv_layer(dev):
    """Conv 3 x 3 x 16 x 32 stored OIHW, gs = 32 (axis 1, C = 144 = 4.5 groups, scale (32, 5)); "hwio" raises."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=6)
    with pytest.raises(ValueError, match="memory order"):
        lq.CustomConv2DLayer(filters=32, orientation="groupwise", group_size=32, initializer=init, input_shape=16, device=dev,
                             kernel_storage="hwio", scale_gradient="ste", bits=4)
    layer = lq.CustomConv2DLayer(filters=32, orientation="groupwise", group_size=32, initializer=init, input_shape=16, device=dev,
                                 scale_gradient="ste", bits=4)
    nested = layer.nested_q_k_layer
    assert tuple(layer.kernel.shape) == (3, 3, 16, 32) and tuple(nested.scale.shape) == (32, 5)
    P, s, dy, ref = _case(32, 144, 1, 32)
    oihw = lambda a: a.reshape(32, 16, 3, 3)                                      # noqa: E731  the memory-order matrix as OIHW
    _load_case(layer.kernel.data.permute(3, 2, 0, 1), nested, oihw(P), s, dev)
    w = layer.quantized_parameters()[0]                                           # what the convolution consumes: OIHW-shaped
    assert tuple(w.shape) == (32, 16, 3, 3) and w.is_contiguous()
    assert bits_equal(w.detach().cpu().numpy().reshape(32, 144), ref["out"])
    (w * _t(oihw(dy), dev)).sum().backward()
    g = layer.kernel.grad
    assert tuple(g.shape) == (3, 3, 16, 32)
    assert bits_equal(g.permute(3, 2, 0, 1).contiguous().cpu().numpy().reshape(32, 144), ref["dP"])
    assert_within_terms(nested.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], "conv ds")
    q = nested.quantized_integers(layer.kernel.data, torch.int32).permute(3, 2, 0, 1).contiguous().cpu().numpy().reshape(32, 144)
    assert np.array_equal(q, ref["q"].astype(np.int32))
    y = layer(torch.ones(2, 16, 8, 8, device=dev))
    assert tuple(y.shape) == (2, 32, 8, 8) and bool(torch.isfinite(y).all())


def test_forward_and_backward_from_a_graph(dev):
    """Forward and backward of a group-wise Dense layer and conv kernel recorded on one stream and replayed == the eager results."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    dense = lq.CustomDenseLayer(units=24, orientation="groupwise", group_size=16, initializer=lq.RandomNormal(seed=8), input_shape=50,
                                device=dev, scale_gradient="ste", bits=4)
    conv = lq.CustomConv2DLayerNoBias(filters=8, orientation="groupwise", group_size=32, initializer=lq.RandomNormal(seed=9),
                                      input_shape=5, device=dev, scale_gradient="ste", bits=4)
    P, s, _, _ = _case(50, 24, 0, 16)
    _load_case(dense.W, dense.nested_q_w_layer, P, s, dev)
    P, s, _, _ = _case(8, 45, 1, 32)
    _load_case(conv.kernel.data.permute(3, 2, 0, 1), conv.nested_q_k_layer, P.reshape(8, 5, 3, 3), s, dev)
    with torch.no_grad():
        dense.nested_q_b_layer.scale.fill_(2.0 ** -6)
    rng = np.random.default_rng(8)
    x = _t(rng.standard_normal((16, 50), dtype=np.float32), dev)
    cw = _t(rng.standard_normal((16, 24), dtype=np.float32), dev)
    ck = _t(rng.standard_normal((8, 5, 3, 3), dtype=np.float32), dev)
    params = [dense.W, dense.b, dense.nested_q_w_layer.scale, dense.nested_q_b_layer.scale, conv.kernel, conv.nested_q_k_layer.scale]

    def run():
        y = dense(x)
        w = conv.quantized_parameters()[0]
        return (y, w) + torch.autograd.grad((y * cw).sum() + (w * ck).sum(), params)

    eager = [t.detach().clone() for t in run()]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        for i, (a, b) in enumerate(zip(eager, captured)):
            assert torch.equal(a, b.detach()), f"result {i}: replay differs from the eager result"
    assert bool((eager[2] == 0).any()) and bool((eager[2] != 0).any())            # the mask is at work
    assert bool((eager[4] != 0).all()) and bool((eager[7] != 0).all())            # every group-wise scale has a gradient


# ----------------------------------------------------------------------------------------------------------------- harness
def _recipe(model, dev, seed):
    """Scales where a sizeable share of the weights is inside the range (at SCALE_INIT every weight clips and none moves):
    N(0, 0.05) weights over s = 0.05 / 4 * U[0.8, 1.25]."""
    import learned_quantization_amd as lq
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for layer in lq.custom_layers_of(model):
            for name in ("nested_q_w_layer", "nested_q_k_layer", "nested_q_b_layer"):
                nested = getattr(layer, name, None)
                if nested is not None:
                    v = np.float32(0.05 / 4) * rng.uniform(0.8, 1.25, tuple(nested.scale.shape)).astype(np.float32)
                    nested.scale.copy_(torch.from_numpy(v).to(dev))


def _group_scales(tr):
    return [l.nested_q_w_layer.scale for l in tr.custom_layers]


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """The product Trainer(config="mnist", mode="ste", bits=4, group_size=64), eager and graphed, three steps each from the same
    state (after the three eager warm-up steps of step_graphed); the eager run records which groups had a gradient in some step."""
    from learned_quantization_amd.train import Trainer, synthetic_batch
    gen = torch.Generator(device=dev).manual_seed(0)
    y = synthetic_batch("mnist", 32, dev, gen)[1]
    # zero-mean inputs: under raw 0..255 pixels the floor quantizer's mean error of -s/2 per weight, times the sum of a
    # sample's pixels, switches all but one hidden unit off at these scales (measured: 13 of 1664 groups of the first layer had a
    # gradient in step 1, none afterwards), and a switched-off unit passes no gradient to its column of W
    x = torch.randn(32, 1, 28, 28, device=dev, generator=gen)
    runs = []
    for graph in (False, True):
        tr = Trainer(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path_factory.mktemp("groupwise")), graph=graph,
                     seed=7, bits=4, group_size=64, lr=1e-3)
        _recipe(tr.model, dev, 7)
        tr.model.eval()
        start = [s.detach().clone() for s in _group_scales(tr)]
        step = tr.step_graphed if graph else tr.step
        losses, seen = [], [torch.zeros_like(s, dtype=torch.bool) for s in start]
        for _ in range(3 + (0 if graph else 3)):                                             # step_graphed: 3 eager warm-up steps first
            losses.append(step(x, y).detach().clone())
            if not graph:
                seen = [m | (s.grad != 0) for m, s in zip(seen, _group_scales(tr))]          # groups that had a gradient in some step
                print("groups with a gradient:", [int((s.grad != 0).sum()) for s in _group_scales(tr)], "loss", float(losses[-1]))
        torch.cuda.synchronize()
        runs.append((tr, losses[-3:], start, seen))
    return runs


def test_trainer_eager_and_graphed(dev, trained):
    """The product Trainer (tests/_linear_task.py's trainer runs eager steps only; it is used in the next test): finite losses,
    every group-wise scale, group by group, has a nonzero gradient and moves, graphed losses and parameters equal the eager ones
    bit for bit.  The batch is zero-mean noise (see the fixture): every hidden unit is then on for some sample of the batch."""
    (eager, le, start, seen), (graphed, lg, _, _) = trained
    assert all(np.isfinite(float(a)) for a in le)
    for a, b in zip(le, lg):
        assert torch.equal(a, b), f"losses differ: {float(a)!r} {float(b)!r}"
    for (n, p), (_, p2) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), n
    for layer, s0, had in zip(eager.custom_layers, start, seen):
        scale = layer.nested_q_w_layer.scale
        assert tuple(scale.shape) == ((13, 128) if layer.W.shape[0] == 784 else (2, 10))
        moved = scale.detach() != s0
        print(f"{layer.name}: {int(had.sum())} of {scale.numel()} groups had a gradient, {int(moved.sum())} moved")
        assert scale.grad is not None and bool(had.all()), f"{layer.name}: a group-wise scale without a gradient"
        assert bool(moved.all()), f"{layer.name}: a group-wise scale did not move"


def test_linear_task_trainer(dev, tmp_path):
    """tests/_linear_task.py's trainer accepts the keyword (eager steps only: it refuses graph=True): three steps on injected
    gradients give finite objectives, every group-wise scale has a nonzero gradient and moves.  CIFAR config: conv kernels, axis 1."""
    from _linear_task import LinearTaskTrainer, make_coefficients
    tr = LinearTaskTrainer(config="cifar", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path), seed=3, bits=4, group_size=128,
                           lr=1e-3)
    _recipe(tr.model, dev, 3)
    tr.coefficients = make_coefficients(tr, 3, lo=-3.0, hi=-1.0)
    scales = [l.nested_q_k_layer.scale for l in tr.custom_layers]
    assert [tuple(s.shape) for s in scales] == [(32, 1), (32, 3), (64, 3), (64, 5), (128, 5), (128, 9)]
    start = [s.detach().clone() for s in scales]
    x = torch.zeros(2, 3, 32, 32, device=dev)
    y = torch.zeros(2, dtype=torch.long, device=dev)
    losses = [float(tr.step(x, y)) for _ in range(3)]
    assert all(np.isfinite(v) for v in losses)
    for s, s0 in zip(scales, start):
        assert s.grad is not None and bool((s.grad != 0).all()) and bool((s.detach() != s0).all())


# ------------------------------------------------------------------------------------------------------------------ export
def test_export_of_a_group_wise_model(dev, trained, tmp_path):
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    model = trained[0][0].model
    tensors = export.quantized_tensors(model)
    # the reference-format int8 file: the clamped integers of the reference
    lq.save_compress_parameters(model, str(tmp_path))
    weights = np.load(os.path.join(str(tmp_path), "weights.npy"), allow_pickle=True).item()
    for name, param, nested in tensors:
        if nested.group_size is None:
            continue
        P, s = param.detach().cpu().numpy(), nested.scale.detach().cpu().numpy()
        ref = group_reference(P, s, np.zeros_like(P), -8, 7, 0, 64)
        assert weights[name].dtype == np.int8 and np.array_equal(weights[name], ref["q"].astype(np.int8)), name
    assert sum(n.group_size is not None for _, _, n in tensors) == 2
    # the packed container: group_size and the scale shape in the manifest, an exact restore into a fresh model
    info = lq.save_packed_parameters(model, str(tmp_path))
    assert info["bits_per_weight"] <= 4.0
    with np.load(os.path.join(str(tmp_path), "weights_packed.npz")) as z:
        manifest = export.read_packed_manifest(z)
    for e, (_, _, nested) in zip(manifest["tensors"], tensors):
        assert e.get("group_size") == nested.group_size and e["scale_shape"] == list(nested.scale.shape) and e["bits"] <= 4
    lq.reset_layer_names()
    fresh = lq.build_model("mnist", mode="ste", value=0.0, seed=99, device=dev, bits=4, group_size=64)
    lq.load_packed_parameters(fresh, str(tmp_path))
    for (name, p0, n0), (_, p1, n1) in zip(tensors, export.quantized_tensors(fresh)):
        assert torch.equal(n0.scale.detach(), n1.scale.detach()), name
        assert torch.equal(n0(p0).detach(), n1(p1).detach()), f"{name}: fake-quantised output after the restore"
    x = torch.rand(4, 1, 28, 28, device=dev) * 255.0
    model.eval(), fresh.eval()
    with torch.no_grad():
        assert torch.equal(model(x), fresh(x))
    # another group size, or none: refused, the model left untouched
    for kw in (dict(group_size=32), dict(orientation="rowwise")):
        lq.reset_layer_names()
        other = lq.build_model("mnist", mode="ste", value=0.0, seed=99, device=dev, bits=4, **kw)
        before = other.dense_1.W.detach().clone()
        with pytest.raises(ValueError, match="group_size"):
            lq.load_packed_parameters(other, str(tmp_path))
        assert torch.equal(before, other.dense_1.W.detach())


def test_export_of_a_conv_model_round_trips(dev, tmp_path):
    """Conv kernels (axis 1, OIHW memory behind the HWIO shape), floor and nearest: pack, restore, same fake-quantised tensors."""
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    for rounding in ("floor", "nearest"):
        lq.reset_layer_names()
        model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=dev, bits=4, group_size=128, rounding=rounding)
        _recipe(model, dev, 3)
        d = os.path.join(str(tmp_path), rounding)
        lq.save_packed_parameters(model, d)
        lq.reset_layer_names()
        fresh = lq.build_model("cifar", mode="ste", value=0.0, seed=4, device=dev, bits=4, group_size=128, rounding=rounding)
        lq.load_packed_parameters(fresh, d)
        for (name, p0, n0), (_, p1, n1) in zip(export.quantized_tensors(model), export.quantized_tensors(fresh)):
            assert torch.equal(n0(p0).detach(), n1(p1).detach()), f"{name} {rounding}"


def test_export_without_group_wise_layers_is_unchanged(dev, tmp_path):
    """A model without group-wise layers: both files hold exactly what the per-axis path writes -- rebuilt here entry by entry with
    the ops that path uses (npz members carry a time stamp, so the members are compared, in order, not the zip's bytes)."""
    import io
    import json
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    lq.reset_layer_names()
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, orientation="rowwise", device=dev, bits=4)
    _recipe(model, dev, 3)
    tensors = export.quantized_tensors(model)
    lq.save_compress_parameters(model, str(tmp_path))
    want = {name: np.ascontiguousarray(lq.fq_forward_clip(p.data, n.scale.data, -8, 7, q_dtype=torch.int8)[1].cpu().numpy())
            for name, p, n in tensors}
    buf = io.BytesIO()
    np.save(buf, want)
    assert open(os.path.join(str(tmp_path), "weights.npy"), "rb").read() == buf.getvalue()
    lq.save_packed_parameters(model, str(tmp_path))
    entries, arrays = [], {}
    for name, p, n in tensors:
        q = lq.fq_forward_clip(p.data, n.scale.data, -8, 7, q_dtype=torch.float32)[1]
        unit = torch.ones_like(n.scale.data)
        lo, hi = (int(v) for v in lq.q_minmax(q, unit).tolist())
        entries.append({"name": name, "shape": list(p.shape), "scale_shape": list(n.scale.shape), "orientation": n.orientation,
                        "qmin": lo, "bits": (hi - lo).bit_length(), "numel": int(p.numel())})
        arrays[name + ".codes"] = lq.q_pack(q, unit, qmin=lo, bits=entries[-1]["bits"])[0].cpu().numpy().view(np.uint32)
        arrays[name + ".scale"] = n.scale.detach().cpu().numpy()
    manifest = {"format": "lq-packed", "version": 1, "tensors": entries, "state": []}
    with np.load(os.path.join(str(tmp_path), "weights_packed.npz")) as z:
        assert z.files == ["manifest"] + list(arrays)
        assert bytes(z["manifest"]) == json.dumps(manifest).encode("utf-8")
        for key, a in arrays.items():
            assert z[key].dtype == a.dtype and z[key].shape == a.shape and z[key].tobytes() == a.tobytes(), key
