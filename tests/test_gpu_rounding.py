"""GPU tests of round-to-nearest for the clipped b-bit fake-quant (include/lq_hip.h: lq_fq_forward_clip_r,
lq_fq_backward_clip_r with LQ_ROUND_NEAREST_EVEN; Python: ``rounding="nearest"``).

The reference is the NumPy restatement tests/_rne_reference.py (pinned on hand-written tables by tests/test_rounding_cpu.py).
out, q, dP and clipped must equal it BIT FOR BIT (out and dP including the sign of zero); ds is held to
tests/_bounds.py::assert_within_terms, |got - ref| <= 1e-5 * sum|dy_i r_i| (floor 2^-136) with the clipped terms included in the
sum.  Two calls must be ``torch.equal``.  Before any kernel runs, the reference itself must clip on both sides, stay mostly
inside, and differ from the floor pair's integers on at least 30 % of the elements: a floor kernel cannot pass.  Every case
prints its worst err / sum|terms|; run with ``-s`` to see them (the overall worst is recorded in DESIGN.md)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _bounds import assert_within_terms, stable_seed                                                   # noqa: E402
from _rne_reference import bits_equal, floor_integers, rne_reference, tie_table, with_other_dy      # noqa: E402

pytestmark = pytest.mark.gpu
LIM = 1 << 24
NEAREST = dict(rounding="nearest")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


ROW = [(1, 1, 12289), (1, 1, 10), (1, 5, 4100), (2, 3, 1027), (1, 37, 100), (1, 64, 17), (3, 7, 196)]
COL = [(133, 10, 1), (300, 3, 1), (64, 130, 4), (129, 257, 1), (40, 1001, 1), (256, 16, 49)]
FIN = [(1, 2, 300001), (1024, 2048, 1)]
STREAM = [(1, 3, 1 << 21), (1 << 20, 6, 1)]                 # both sides of the 4 M-element planner switch with the rest
DESCRIPTORS = ROW + COL + FIN + STREAM
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


def _range(bits, signed=True):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)


def _inputs(desc, bits, signed=True):
    """The clipped suite's recipe (tests/test_gpu_clip.py::_inputs), restated: P ~ N(0, 0.05), s[g] = 0.05 / 2^(b-2) *
    U[0.8, 1.25], dy ~ N(0, 1) plus an all-positive and an all-zero dy; unsigned ranges: P shifted by 2^(b-1) * s[g]."""
    outer, G, inner = desc
    rng = np.random.default_rng(stable_seed(desc, bits, signed))
    n = outer * G * inner
    P = (rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)).reshape(desc)
    s = (np.float32(0.05 / 2 ** (bits - 2)) * rng.uniform(0.8, 1.25, G).astype(np.float32)).reshape(1, G, 1)
    if not signed:
        P = P + np.float32(2 ** (bits - 1)) * s
    signed_dy = rng.standard_normal(n, dtype=np.float32).reshape(desc)
    dys = {"signed": signed_dy, "positive": np.abs(signed_dy) + np.float32(1e-30), "zero": np.zeros(desc, np.float32)}
    return P, s, dys


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


def _ratio(got, ref, terms):
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(got, np.float64) - ref) / np.maximum(terms, 1e-300)
    return float(np.nanmax(r)) if r.size else 0.0


def _check_condition(ref, P, s, qmin, qmax, what):
    """Asserted on the REFERENCE before any kernel runs: the case clips on both sides, mostly does not, and its integers are not
    the floor pair's."""
    n = ref["inside"].size
    low, high = int((ref["q0"] < qmin).sum()), int((ref["q0"] > qmax).sum())
    inside = int(ref["inside"].sum())
    differ = int((floor_integers(P, s, qmin, qmax) != ref["q"]).sum())
    assert low >= 2 and low >= 0.002 * n, f"{what}: {low} of {n} clipped low"
    assert high >= 2 and high >= 0.002 * n, f"{what}: {high} of {n} clipped high"
    assert inside >= 0.8 * n, f"{what}: only {inside} of {n} inside"
    assert differ >= 0.3 * n, f"{what}: only {differ} of {n} integers differ from the floor pair's"
    assert low + high + inside == n
    return low, high, differ


def _check_case(dev, desc, qmin, qmax, P, s, dys, misaligned=False, k=1.0, condition=True):
    import learned_quantization_amd as lq
    what = f"{desc} [{qmin}, {qmax}] nearest{' misaligned' if misaligned else ''}"
    ref = rne_reference(P, s, dys["signed"], qmin, qmax, k)
    if condition and P.size >= 900:
        low, high, differ = _check_condition(ref, P, s, qmin, qmax, what)
        print(f"{what}: {low} low, {high} high, {differ} unlike floor of {P.size}")
    Pt, st = _dev(P, dev, misaligned), _dev(s, dev)
    out, q = lq.fq_forward_clip(Pt, st, qmin, qmax, q_dtype=torch.int32, **NEAREST)
    assert torch.equal(out, lq.fq_forward_clip(Pt, st, qmin, qmax, **NEAREST)), f"{what}: two forward calls differ"
    assert bits_equal(out.cpu().numpy(), ref["out"]), f"{what}: out"
    assert np.array_equal(q.cpu().numpy(), ref["q"].astype(np.int32)), f"{what}: q"
    worst = 0.0
    for name, dy in dys.items():
        dP_ref, ds_ref, terms = (ref["dP"], ref["ds"], ref["terms"]) if name == "signed" else with_other_dy(ref, s, dy, k)
        dt = _dev(dy, dev, misaligned)
        dP, ds, clipped = lq.fq_backward_clip(Pt, st, dt, qmin, qmax, grad_scale=k, want_clipped=True, **NEAREST)
        dP2, ds2, clipped2 = lq.fq_backward_clip(Pt, st, dt, qmin, qmax, grad_scale=k, want_clipped=True, **NEAREST)
        assert torch.equal(dP, dP2) and torch.equal(ds, ds2) and torch.equal(clipped, clipped2), f"{what} {name}: two calls differ"
        assert ds.shape == st.shape and clipped.shape == st.shape and dP.shape == Pt.shape
        assert bits_equal(dP.cpu().numpy(), dP_ref), f"{what} dy {name}: dP"
        assert np.array_equal(clipped.cpu().numpy().view(np.uint32).astype(np.int64), ref["clipped"]), f"{what} dy {name}: clipped"
        got = ds.cpu().numpy()
        ratio = _ratio(got, ds_ref, terms) if name != "zero" else 0.0
        worst = max(worst, ratio)
        print(f"{what} dy {name}: max err / sum|terms| = {ratio:.3e}")
        if name == "zero":
            assert np.all(got == 0.0) and not np.any(np.signbit(dP.cpu().numpy())), f"{what}: dy == 0 must give ds == 0, dP == +0"
            continue
        assert_within_terms(got, ds_ref, terms, f"{what} dy {name}")
    # mask only (the loss-term-only rule): no ds, the same dP
    dP3, ds3, c3 = lq.fq_backward_clip(Pt, st, _dev(dys["signed"], dev, misaligned), qmin, qmax, want_ds=False, **NEAREST)
    assert ds3 is None and c3 is None and bits_equal(dP3.cpu().numpy(), ref["dP"]), f"{what}: mask-only dP"
    return worst


# ------------------------------------------------------------------------------------------------ 1 + 2: descriptors
@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("desc", DESCRIPTORS, ids=_ids)
def test_descriptors_signed(dev, desc, bits):
    P, s, dys = _inputs(desc, bits)
    _check_case(dev, desc, *_range(bits), P, s, dys)


@pytest.mark.parametrize("desc", [(1, 5, 4100), (64, 130, 4), (1, 3, 1 << 21)], ids=_ids)
def test_descriptors_unsigned_4_bit(dev, desc):
    P, s, dys = _inputs(desc, 4, signed=False)
    _check_case(dev, desc, 0, 15, P, s, dys)


@pytest.mark.parametrize("desc", [(1, 5, 4100), (64, 130, 4)], ids=_ids)
def test_misaligned_base(dev, desc):
    """P and dy one float off a 16-byte base: the scalar forms of the row stream and of the column tile."""
    P, s, dys = _inputs(desc, 4)
    _check_case(dev, desc, -8, 7, P, s, dys, misaligned=True)


@pytest.mark.parametrize("desc", [(1, 1, 12289), (1, 37, 100), (133, 10, 1), (1, 2, 300001)], ids=_ids)
def test_grad_scale_factor(dev, desc):
    """k = 0.37: applied once per group in f64, by the finalize forms and by the direct emit alike."""
    P, s, dys = _inputs(desc, 4)
    _check_case(dev, desc, -8, 7, P, s, {"signed": dys["signed"]}, k=0.37)
    assert np.max(np.abs(rne_reference(P, s, dys["signed"], -8, 7, 0.37)["ds"] - rne_reference(P, s, dys["signed"], -8, 7)["ds"])) > 0


def test_q_dtypes(dev):
    import learned_quantization_amd as lq
    P, s, dys = _inputs((1, 5, 4100), 8)
    ref = rne_reference(P, s, dys["signed"], -128, 127)
    for dt, npdt in ((torch.int8, np.int8), (torch.int32, np.int32), (torch.float32, np.float32)):
        out, q = lq.fq_forward_clip(_dev(P, dev), _dev(s, dev), -128, 127, q_dtype=dt, **NEAREST)
        assert q.dtype == dt and np.array_equal(q.cpu().numpy(), ref["q"].astype(npdt))
        assert bits_equal(out.cpu().numpy(), ref["out"])
    assert ref["q"].min() == -128 and ref["q"].max() == 127              # the int8 view holds both bounds without a wrap


# ------------------------------------------------------------------------------------------------ 3: ties and edges
@pytest.mark.parametrize("scalar", [False, True], ids=["rowwise", "scalar"])
@pytest.mark.parametrize("sv", [2.0 ** -7, 1.0])
@pytest.mark.parametrize("qmin,qmax", [(-8, 7), (0, 15)])
def test_tie_and_edge_table_on_the_device(dev, qmin, qmax, sv, scalar):
    """Every half-integer from qmin - 1.5 to qmax + 1.5, the neighbours of both edges' ties and +-0 at a power-of-two scale
    (exact quotients), tiled to 8 rows; rows rotated so that every table entry meets every lane position.  The expected q0 is
    written out by the tie rule in tie_table, not computed by rint."""
    import learned_quantization_amd as lq
    t, q0_want = tie_table(qmin, qmax)
    Pt = t * np.float32(sv)
    assert np.array_equal(Pt / np.float32(sv), t)                                         # the quotients are exact
    q_want = np.clip(q0_want, qmin, qmax)
    inside_want = (q0_want >= qmin) & (q0_want <= qmax)
    rows, reps = 8, 23
    L = reps * Pt.size
    tile = lambda a: np.stack([np.roll(np.tile(a, reps), r) for r in range(rows)])      # noqa: E731
    P, q_full, in_full, t_full = tile(Pt).astype(np.float32), tile(q_want), tile(inside_want), tile(t)
    rng = np.random.default_rng(stable_seed("ties", qmin, qmax, sv, scalar))
    dy = rng.standard_normal(P.shape, dtype=np.float32)
    if scalar:
        desc, s = (1, 1, rows * L), np.full((1, 1, 1), sv, np.float32)
    else:
        desc, s = (1, rows, L), np.full((1, rows, 1), sv, np.float32)
    P, dy = P.reshape(desc), dy.reshape(desc)
    ref = rne_reference(P, s, dy, qmin, qmax)
    assert np.array_equal(ref["q"].reshape(rows, L), q_full) and np.array_equal(ref["inside"].reshape(rows, L), in_full)
    _check_case(dev, desc, qmin, qmax, P, s, {"signed": dy, "positive": np.abs(dy), "zero": np.zeros_like(dy)}, condition=False)
    # q, inside and the sign of out, against the hand-written expectations themselves
    ones = torch.ones(desc, device=dev)
    out, q = lq.fq_forward_clip(_dev(P, dev), _dev(s, dev), qmin, qmax, q_dtype=torch.int32, **NEAREST)
    dP = lq.fq_backward_clip(_dev(P, dev), _dev(s, dev), ones, qmin, qmax, want_ds=False, **NEAREST)[0]
    assert np.array_equal(q.cpu().numpy().reshape(rows, L), q_full.astype(np.int32))
    assert np.array_equal(dP.cpu().numpy().reshape(rows, L) == 1.0, in_full)
    o = out.cpu().numpy().reshape(rows, L)
    neg_zero = (t_full >= -0.5) & (t_full <= 0) & np.signbit(t_full)                      # t in [-1/2, -0]: q0 = -0, out = -0 * s
    assert neg_zero.sum() >= 2 * rows * reps
    assert np.all(o[neg_zero] == 0.0) and np.all(np.signbit(o[neg_zero]))
    pos_zero = (t_full >= 0) & (t_full <= 0.5) & ~np.signbit(t_full)
    assert np.all(o[pos_zero] == 0.0) and not np.any(np.signbit(o[pos_zero]))


# ------------------------------------------------------------------------------------------------ 4: special values
@pytest.mark.parametrize("desc", [(1, 5, 4100), (1, 37, 100), (133, 10, 1), (64, 130, 4), (1, 1, 3000)], ids=_ids)
def test_special_values_stay_in_their_group(dev, desc):
    """NaN, +-Inf, |t| >= 2^23, +-0 and denormals in group 1 (or in the only group), clean data in the others."""
    import learned_quantization_amd as lq
    P, s, dys = _inputs(desc, 4)
    G = desc[1]
    g = 1 if G > 1 else 0
    sg = float(s.reshape(-1)[g])
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38, sg * 2.0 ** 23, -sg * (2.0 ** 23 + 2), sg * 2.0 ** 25],
                       np.float32)
    P = P.copy()
    view = P[:, g, :].reshape(-1)
    assert view.size >= special.size
    pos = np.linspace(0, view.size - 1, special.size).astype(int)
    view[pos] = special
    P[:, g, :] = view.reshape(P[:, g, :].shape)
    dy = dys["signed"]
    ref = rne_reference(P, s, dy, -8, 7)
    with np.errstate(all="ignore"):
        assert int((np.abs(ref["t"]) >= 2.0 ** 23).sum()) >= 5
    Pt, st = _dev(P, dev), _dev(s, dev)
    out, q = lq.fq_forward_clip(Pt, st, -8, 7, q_dtype=torch.float32, **NEAREST)
    dP, ds, clipped = lq.fq_backward_clip(Pt, st, _dev(dy, dev), -8, 7, want_clipped=True, **NEAREST)
    assert bits_equal(out.cpu().numpy(), ref["out"])
    assert bits_equal(q.cpu().numpy(), ref["q"])                                                 # the float view keeps -0 and NaN
    dPn = dP.cpu().numpy()
    assert bits_equal(dPn, ref["dP"])
    bad = ~np.isfinite(P)
    assert bad.sum() == 3 and np.all(dPn[bad] == 0.0) and not np.any(np.signbit(dPn[bad]))       # exactly +0 at NaN and Inf
    assert np.array_equal(clipped.cpu().numpy().view(np.uint32).astype(np.int64), ref["clipped"])
    got = ds.cpu().numpy().reshape(-1)
    assert np.isnan(got[g]) and np.isnan(ref["ds"].reshape(-1)[g])                               # NaN confined to that group
    ok = np.arange(G) != g
    assert np.all(np.isfinite(got[ok]))
    assert_within_terms(got[ok], ref["ds"].reshape(-1)[ok], ref["terms"].reshape(-1)[ok], f"{desc}: groups without special values")
    # the same tensor without the NaN: that group's ds is finite again and within the bound (Inf saturates, it does not poison)
    P2 = P.copy()
    P2[np.isnan(P2)] = np.float32(0.01)
    ref2 = rne_reference(P2, s, dy, -8, 7)
    _, ds2, c2 = lq.fq_backward_clip(_dev(P2, dev), st, _dev(dy, dev), -8, 7, want_clipped=True, **NEAREST)
    assert_within_terms(ds2.cpu().numpy(), ref2["ds"], ref2["terms"], f"{desc}: Inf, zeros, denormals, large quotients")
    assert np.array_equal(c2.cpu().numpy().view(np.uint32).astype(np.int64), ref2["clipped"])
    # in the widest range a quotient of 2^23 and more is inside, comes back unchanged and has r == 0
    wide = rne_reference(P2, s, dy, -LIM, LIM)
    outw = lq.fq_forward_clip(_dev(P2, dev), st, -LIM, LIM, **NEAREST)
    assert bits_equal(outw.cpu().numpy(), wide["out"])


# ------------------------------------------------------------------------------------------------ 5: floor through the new entry points
@pytest.mark.parametrize("desc", [(1, 5, 4100), (64, 130, 4), (1, 2, 300001)], ids=_ids)
def test_floor_through_the_new_entry_points(dev, desc):
    """rounding="floor" goes through lq_fq_forward_clip_r / lq_fq_backward_clip_r; the old entry points, called through the
    binding table directly, give the same bits."""
    import learned_quantization_amd as lq
    from learned_quantization_amd import _hip
    lib = _hip.load()
    P, s, dys = _inputs(desc, 4)
    Pt, st, dt = _dev(P, dev), _dev(s, dev), _dev(dys["signed"], dev)
    outer, G, inner = desc
    out, q = lq.fq_forward_clip(Pt, st, -8, 7, q_dtype=torch.int32, rounding="floor")
    dP, ds, clipped = lq.fq_backward_clip(Pt, st, dt, -8, 7, grad_scale=0.37, want_clipped=True, rounding="floor")
    out0, q0 = torch.empty_like(Pt), torch.empty_like(Pt, dtype=torch.int32)
    _hip.check(lib.lq_fq_forward_clip(_hip.ptr(Pt), _hip.ptr(st), _hip.ptr(out0), _hip.ptr(q0), _hip.LQ_Q_I32, -8, 7, outer, G, inner,
                                      _hip.stream_ptr(dev)), "lq_fq_forward_clip")
    dP0, ds0, c0 = torch.empty_like(Pt), torch.empty_like(st), torch.empty_like(st, dtype=torch.int32)
    ws = _hip.workspace_for(dev, outer, G, inner)
    _hip.check(lib.lq_fq_backward_clip(_hip.ptr(Pt), _hip.ptr(st), _hip.ptr(dt), -8, 7, 0.37, _hip.ptr(dP0), _hip.ptr(ds0), _hip.ptr(c0),
                                       _hip.ptr(ws), ws.numel(), outer, G, inner, _hip.stream_ptr(dev)), "lq_fq_backward_clip")
    torch.cuda.synchronize(dev)
    for name, a, b in (("out", out, out0), ("q", q, q0), ("dP", dP, dP0), ("ds", ds, ds0), ("clipped", clipped, c0)):
        assert torch.equal(a, b), f"{desc}: {name} of rounding='floor' differs from the existing call"
    # and the default of the Python wrappers is floor
    assert torch.equal(out, lq.fq_forward_clip(Pt, st, -8, 7))
    dP1, ds1, c1 = lq.fq_backward_clip(Pt, st, dt, -8, 7, grad_scale=0.37, want_clipped=True)
    assert torch.equal(dP, dP1) and torch.equal(ds, ds1) and torch.equal(clipped, c1)
    assert not torch.equal(out, lq.fq_forward_clip(Pt, st, -8, 7, **NEAREST))


# ------------------------------------------------------------------------------------------------ 6: widest range
@pytest.mark.parametrize("desc", [(1, 5, 4100), (64, 130, 4)], ids=_ids)
def test_widest_range_is_the_unbounded_nearest_quantizer(dev, desc):
    """(-2^24, 2^24): out == rint(P/s) * s bit for bit, dP == dy, nothing clipped."""
    import learned_quantization_amd as lq
    P, s, dys = _inputs(desc, 4)
    Pt, st, dt = _dev(P, dev), _dev(s, dev), _dev(dys["signed"], dev)
    want = np.rint(P / s) * s
    assert want.dtype == np.float32 and float(np.abs(P / s).max()) < LIM
    out = lq.fq_forward_clip(Pt, st, -LIM, LIM, **NEAREST)
    assert bits_equal(out.cpu().numpy(), want)
    dP, ds, clipped = lq.fq_backward_clip(Pt, st, dt, -LIM, LIM, want_clipped=True, **NEAREST)
    assert torch.equal(dP, dt) and int(clipped.sum()) == 0
    ref = rne_reference(P, s, dys["signed"], -LIM, LIM)
    assert_within_terms(ds.cpu().numpy(), ref["ds"], ref["terms"], f"{desc}: widest range")


# ------------------------------------------------------------------------------------------------ 7: autograd and layers
@pytest.mark.parametrize("rule,gs", [(None, 1.0), ("ste", 1.0), ("ste", 0.37)])
def test_autograd(dev, rule, gs):
    import learned_quantization_amd as lq
    desc = (1, 37, 100)
    P, s, dys = _inputs(desc, 4)
    dy = dys["signed"]
    ref = rne_reference(P, s, dy, -8, 7, gs)
    assert float((floor_integers(P, s, -8, 7) != ref["q"]).mean()) >= 0.3
    Pt, st = _dev(P, dev).requires_grad_(True), _dev(s, dev).requires_grad_(True)
    out = lq.my_custom_gradient(Pt, st, None, scale_gradient=rule, grad_scale=gs, q_range=(-8, 7), **NEAREST)
    (out * _dev(dy, dev)).sum().backward()
    assert bits_equal(out.detach().cpu().numpy(), ref["out"])
    assert bits_equal(Pt.grad.cpu().numpy(), ref["dP"])
    if rule is None:
        assert torch.equal(st.grad, torch.zeros_like(st))              # the reference's `cl` rule: zeros for the scale
    else:
        assert_within_terms(st.grad.cpu().numpy(), ref["ds"], ref["terms"], f"autograd {rule} k={gs}")
    # only one of the two inputs wants a gradient
    Pt2 = _dev(P, dev).requires_grad_(True)
    out2 = lq.my_custom_gradient(Pt2, _dev(s, dev), scale_gradient=rule, q_range=(-8, 7), **NEAREST)
    (out2 * _dev(dy, dev)).sum().backward()
    assert bits_equal(Pt2.grad.cpu().numpy(), ref["dP"])


def _layer_case(layer, param, nested, get_q, dy_logical_of, dev, what, k_of):
    """Forward and both gradients of one quantised tensor of a layer, through the route the layer itself takes."""
    qmin, qmax = nested.q_range
    assert nested.rounding == "nearest"
    P = param.detach().cpu().numpy()                 # logical order whatever the memory order
    s = nested.scale.detach().cpu().numpy()
    w = get_q()
    rng = np.random.default_rng(stable_seed(what))
    dy_w = torch.from_numpy(rng.standard_normal(tuple(w.shape), dtype=np.float32)).to(dev)
    (w * dy_w).sum().backward()
    dy = dy_logical_of(dy_w).cpu().numpy()
    ref = rne_reference(P, s, dy, qmin, qmax, k_of(param))
    assert bits_equal(dy_logical_of(w.detach()).cpu().numpy(), ref["out"]), f"{what}: forward"
    assert param.grad.stride() == param.stride(), f"{what}: dP must have the parameter's strides"
    assert bits_equal(param.grad.cpu().numpy(), ref["dP"]), f"{what}: dP"
    assert P.size < 900 or 0 < int(ref["clipped"].sum()) < P.size      # a 24-element bias may clip nothing
    assert P.size < 900 or float((floor_integers(P, s, qmin, qmax) != ref["q"]).mean()) >= 0.3
    assert np.array_equal(nested.quantized_integers(param.data, torch.int32).cpu().numpy(), ref["q"].astype(np.int32)), f"{what}: integer view"
    if nested.scale_gradient == "ste":
        assert_within_terms(nested.scale.grad.cpu().numpy(), ref["ds"], ref["terms"], f"{what}: ds")
        print(f"{what}: max err / sum|terms| = {_ratio(nested.scale.grad.cpu().numpy(), ref['ds'], ref['terms']):.3e}")
    else:
        assert torch.equal(nested.scale.grad, torch.zeros_like(nested.scale))


def _set_scale(nested, rng, dev, bits=4):
    with torch.no_grad():
        v = np.float32(0.05 / 2 ** (bits - 2)) * rng.uniform(0.8, 1.25, tuple(nested.scale.shape)).astype(np.float32)
        nested.scale.copy_(torch.from_numpy(v).to(dev))


@pytest.mark.parametrize("grad_scale", [1.0, "rsqrt_group"])
@pytest.mark.parametrize("orientation", ["rowwise", "columnwise", "scalar"])
def test_dense_layer(dev, orientation, grad_scale):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomDenseLayer(units=24, orientation=orientation, initializer=lq.RandomNormal(seed=5), input_shape=50, device=dev,
                                scale_gradient="ste", grad_scale=grad_scale, bits=4, **NEAREST)
    rng = np.random.default_rng(stable_seed("dense", orientation))
    _set_scale(layer.nested_q_w_layer, rng, dev)
    _set_scale(layer.nested_q_b_layer, rng, dev)
    k_of = lambda nested: (lambda p: nested.grad_scale_value(p.numel()))      # noqa: E731
    _layer_case(layer, layer.W, layer.nested_q_w_layer, lambda: layer.quantized_parameters()[0], lambda t: t, dev,
                f"dense W {orientation} {grad_scale}", k_of(layer.nested_q_w_layer))
    layer.zero_grad()
    _layer_case(layer, layer.b, layer.nested_q_b_layer, lambda: layer.quantized_parameters()[1], lambda t: t, dev,
                f"dense b {orientation} {grad_scale}", k_of(layer.nested_q_b_layer))
    y = layer(torch.ones(3, 50, device=dev))                                  # the layer's own call runs on the rounded weights
    want = torch.matmul(torch.ones(3, 50, device=dev), layer.nested_q_w_layer(layer.W)) + layer.nested_q_b_layer(layer.b)
    assert torch.equal(y, want)


@pytest.mark.parametrize("orientation", ["rowwise", "columnwise", "channelwise", "scalar"])
@pytest.mark.parametrize("storage", ["oihw", "hwio"])
def test_conv_layer(dev, storage, orientation):
    """A 3 x 3 conv kernel, 16 -> 32 channels, shaped HWIO in both memory orders, against the reference on the logical tensor."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomConv2DLayer(filters=32, orientation=orientation, initializer=lq.RandomNormal(seed=6), input_shape=16, device=dev,
                                 kernel_storage=storage, scale_gradient="ste", bits=4, **NEAREST)
    assert layer.kernel.is_contiguous() == (storage == "hwio") and tuple(layer.kernel.shape) == (3, 3, 16, 32)
    rng = np.random.default_rng(stable_seed("conv", storage, orientation))
    _set_scale(layer.nested_q_k_layer, rng, dev)
    _layer_case(layer, layer.kernel, layer.nested_q_k_layer, lambda: layer.quantized_parameters()[0],
                lambda t: t.permute(2, 3, 1, 0), dev, f"conv {storage} {orientation}", lambda p: 1.0)
    y = layer(torch.ones(2, 16, 8, 8, device=dev))
    assert tuple(y.shape) == (2, 32, 8, 8) and bool(torch.isfinite(y).all())


def test_dense_layer_forward_and_backward_from_a_graph(dev):
    """Forward and backward of one nearest Dense layer recorded on a single stream and replayed twice == the eager results."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    layer = lq.CustomDenseLayer(units=24, orientation="rowwise", initializer=lq.RandomNormal(seed=8), input_shape=50, device=dev,
                                scale_gradient="ste", bits=4, **NEAREST)
    rng = np.random.default_rng(8)
    _set_scale(layer.nested_q_w_layer, rng, dev)
    _set_scale(layer.nested_q_b_layer, rng, dev)
    x = torch.from_numpy(rng.standard_normal((16, 50), dtype=np.float32)).to(dev)
    w = torch.from_numpy(rng.standard_normal((16, 24), dtype=np.float32)).to(dev)
    params = [layer.W, layer.b, layer.nested_q_w_layer.scale, layer.nested_q_b_layer.scale]

    def run():
        y = layer(x)
        return (y,) + torch.autograd.grad((y * w).sum(), params)

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
        for name, a, b in zip(("y", "dW", "db", "dsW", "dsb"), eager, captured):
            assert torch.equal(a, b.detach()), f"{name}: replay differs from the eager result"
    assert bool((eager[1] == 0).any()) and bool((eager[1] != 0).any())            # the mask is at work
    # the floor layer of the same weights gives another output: the graph really ran the nearest pair
    P, s = layer.W.detach().cpu().numpy(), layer.nested_q_w_layer.scale.detach().cpu().numpy()
    assert bits_equal(layer.nested_q_w_layer(layer.W).detach().cpu().numpy(), rne_reference(P, s, np.zeros_like(P), -8, 7)["out"])


# ------------------------------------------------------------------------------------------------ 8: trainer
def _recipe_scales(model, dev, seed):
    rng = np.random.default_rng(seed)
    import learned_quantization_amd as lq
    for layer in lq.custom_layers_of(model):
        _set_scale(layer.nested_q_w_layer if hasattr(layer, "nested_q_w_layer") else layer.nested_q_k_layer, rng, dev)
        _set_scale(layer.nested_q_b_layer, rng, dev)


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """Trainer(config="mnist", mode="ste", bits=4, rounding="nearest"), eager and graphed, three steps each from the same state.
    The scales start at the recipe's value instead of SCALE_INIT (where every element would be clipped and no weight would move)."""
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    runs = []
    for graph in (False, True):
        tr = Trainer("mnist", "ste", 0.0, "rowwise", None, device=dev, log_dir=str(tmp_path_factory.mktemp("rne")), graph=graph,
                     seed=7, bits=4, lr=1e-3, **NEAREST)
        _recipe_scales(tr.model, dev, 7)
        tr.model.eval()
        step = tr.step_graphed if graph else tr.step
        losses = [step(x, y).detach().clone() for _ in range(3 + (0 if graph else 3))]      # step_graphed: 3 eager warm-up steps first
        torch.cuda.synchronize()
        runs.append((tr, losses[-3:]))
    return runs


def test_trainer_graphed_losses_equal_eager_losses(dev, trained):
    """Losses and parameters bit for bit between the eager and the graphed trainer.  Afterwards every weight's integer as the layer
    computes it lies in [-8, 7], equals clamp(rint(P/s)) from NumPy and differs from the floor view on some weights."""
    import learned_quantization_amd as lq
    (eager, le), (graphed, lg) = trained
    assert eager.rounding == graphed.rounding == "nearest"
    for a, b in zip(le, lg):
        assert torch.equal(a, b), f"losses differ: {float(a)!r} {float(b)!r}"
    assert all(np.isfinite(float(a)) for a in le)
    for (n, p), (_, p2) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(p.detach(), p2.detach()), n
    init = lq.build_model("mnist", mode="ste", value=0.0, seed=7, orientation="rowwise", device=dev, bits=4, **NEAREST)
    assert not torch.equal(init.dense_1.W.detach(), eager.model.dense_1.W.detach())              # the weights moved
    unlike = 0
    for tr in (eager, graphed):
        for layer in tr.custom_layers:
            for param, nested in ((layer.W, layer.nested_q_w_layer), (layer.b, layer.nested_q_b_layer)):
                assert nested.q_range == (-8, 7) and nested.rounding == "nearest"
                q = nested.quantized_integers(param.data, torch.int32)
                assert int(q.min()) >= -8 and int(q.max()) <= 7
                P, s = param.detach().cpu().numpy(), nested.scale.detach().cpu().numpy()
                want = np.clip(np.rint(P / s), -8, 7).astype(np.int32)
                assert np.array_equal(q.cpu().numpy(), want), layer.name
                floor_view = lq.quantized_integers(param.data, nested.scale.data, torch.int32).clamp(-8, 7)
                unlike += int((q != floor_view).sum())
    assert unlike > 0


# ------------------------------------------------------------------------------------------------ 9: export
def test_export_of_a_nearest_4_bit_model(dev, trained, tmp_path):
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    model = trained[0][0].model
    tensors = export.quantized_tensors(model)
    info = lq.save_packed_parameters(model, str(tmp_path))
    assert info["bits_per_weight"] <= 4.0
    with np.load(os.path.join(str(tmp_path), "weights_packed.npz")) as z:
        manifest = export.read_packed_manifest(z)
    assert manifest["version"] == 1
    for e in manifest["tensors"]:
        assert e["rounding"] == "nearest" and e["bits"] <= 4 and e["qmin"] >= -8, e
    lq.reset_layer_names()                       # the container names its tensors by the layers' auto-names
    fresh = lq.build_model("mnist", mode="ste", value=0.0, seed=99, orientation="rowwise", device=dev, bits=4, **NEAREST)
    lq.load_packed_parameters(fresh, str(tmp_path))
    for (name, p0, n0), (_, p1, n1) in zip(tensors, export.quantized_tensors(fresh)):
        assert torch.equal(n0.scale.detach(), n1.scale.detach()), name
        assert torch.equal(n0(p0).detach(), n1(p1).detach()), f"{name}: fake-quantised output after the restore"      # value equality
        assert torch.equal(n0.quantized_integers(p0.data, torch.int32), n1.quantized_integers(p1.data, torch.int32)), name
    x = torch.rand(4, 1, 28, 28, device=dev) * 255.0
    model.eval(), fresh.eval()
    with torch.no_grad():
        assert torch.equal(model(x), fresh(x))
    # a floor model refuses the container and stays as it was
    lq.reset_layer_names()
    floor_model = lq.build_model("mnist", mode="ste", value=0.0, seed=5, orientation="rowwise", device=dev, bits=4)
    before = {k: v.detach().clone() for k, v in floor_model.state_dict().items()}
    with pytest.raises(ValueError, match="rounding"):
        lq.load_packed_parameters(floor_model, str(tmp_path))
    for k, v in floor_model.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed although the load was refused"
    # a nearest model with a narrower range refuses it too, for that reason and not as a rounding miss
    lq.reset_layer_names()
    narrow = lq.build_model("mnist", mode="ste", value=0.0, seed=5, orientation="rowwise", device=dev, bits=2, **NEAREST)
    before = {k: v.detach().clone() for k, v in narrow.state_dict().items()}
    with pytest.raises(ValueError, match="outside the integer range of their layer"):
        lq.load_packed_parameters(narrow, str(tmp_path))
    for k, v in narrow.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed although the load was refused"
    # the reference-format int8 file: clamp(rint(P/s))
    lq.save_compress_parameters(model, str(tmp_path))
    weights = np.load(os.path.join(str(tmp_path), "weights.npy"), allow_pickle=True).item()
    for name, param, nested in tensors:
        P, s = param.detach().cpu().numpy(), nested.scale.detach().cpu().numpy()
        assert weights[name].dtype == np.int8 and np.array_equal(weights[name], np.clip(np.rint(P / s), -8, 7).astype(np.int8)), name


def test_a_floor_model_gets_no_rounding_key_and_refuses_nothing(dev, tmp_path):
    import learned_quantization_amd as lq
    from learned_quantization_amd import export
    lq.reset_layer_names()
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, orientation="rowwise", device=dev, bits=4)
    _recipe_scales(model, dev, 3)
    lq.save_packed_parameters(model, str(tmp_path))
    with np.load(os.path.join(str(tmp_path), "weights_packed.npz")) as z:
        manifest = export.read_packed_manifest(z)
    assert manifest["tensors"] and all("rounding" not in e for e in manifest["tensors"])
    # a nearest model refuses a floor container (a missing key means floor) and stays as it was
    lq.reset_layer_names()
    nearest = lq.build_model("mnist", mode="ste", value=0.0, seed=4, orientation="rowwise", device=dev, bits=4, **NEAREST)
    before = {k: v.detach().clone() for k, v in nearest.state_dict().items()}
    with pytest.raises(ValueError, match="rounding"):
        lq.load_packed_parameters(nearest, str(tmp_path))
    for k, v in nearest.state_dict().items():
        assert torch.equal(v, before[k]), k
    lq.reset_layer_names()
    again = lq.build_model("mnist", mode="ste", value=0.0, seed=6, orientation="rowwise", device=dev, bits=4)
    lq.load_packed_parameters(again, str(tmp_path))                        # floor into floor still loads
    for (name, p0, n0), (_, p1, n1) in zip(export.quantized_tensors(model), export.quantized_tensors(again)):
        assert torch.equal(n0(p0).detach(), n1(p1).detach()), name
