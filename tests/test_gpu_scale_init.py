"""GPU tests of scale initialisation (include/lq_hip.h: lq_scale_init_group; ops.scale_init_group, layers.init_scales, the
``scale_init`` option of build_model / Trainer / the drivers) against tests/_scale_init_reference.py.

Inputs: P = N(0, 1) * 0.05 as float32, one array per geometry (_scale_init_reference.make_input); ranges [-8, 7], [0, 15], [-2, 1].
tests/test_scale_init_cpu.py asserts on the reference alone what these tests rely on (nothing clipped after absmax, no group of a
case with an mse gap in (0, 1e-9] beyond 1 %).  Bounds:

  absmax  bit for bit: two exact maxima, two IEEE quotients, one product.
  lsq     within 1 ulp of the reference's math.fsum value: with n <= 2^20 the kernel's f64 sum is within 2^-33 relative of the exact
          one, so only the final rounding to fp32 can differ.
  mse     bit-equal to the reference's choice wherever the relative gap between its best and second-best E_k is 0 (an exact tie:
          the same terms under both candidates, decided by the rule) or above 1e-9 (2000 x the f64 summation bound n * 2^-53 of the
          largest group here); elsewhere bit-equal to the best or the runner-up.

Which case launches which instantiation (every method and, for mse, both roundings run on every geometry; the vector forms need
C % 4 == 0 -- and gs % 4 == 0 on axis 1 -- and a 16-byte aligned P):
  k_init_cols V = 4   (256, 260, 32) (130, 1028, 128) (300, 64, 1) (50, 12, 64) (33000, 4, 1: second trip of the group loop)
  k_init_cols V = 1   (37, 5, 8) (96, 130, 96), and (256, 260, 32) one float off the 16-byte grid
  k_init_rows V = 4   (64, 576, 128) (33, 4100, 128) (40, 64, 4) (20, 96, 96) (1, 70000, 70000)
  k_init_rows V = 1   (7, 27, 8) (16, 100, 1) (1, 130, 130), and (33, 4100, 128) one float off the 16-byte grid"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _scale_init_reference as S                                                     # noqa: E402
from _arena import Arena                                                              # noqa: E402
from _clip_reference import bits_equal                                                # noqa: E402
from _group_reference import scale_shape                                              # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731
MV = S.MIN_VALUE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: the shared inputs are read-only


def _init(dev, P, axis, gs, qmin, qmax, method, rounding="floor", min_value=MV):
    """lq_scale_init_group through the C ABI on a fresh device copy of P; s starts as NaN (an unwritten scale shows)."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C = P.shape
    p = _t(P, dev)
    s = torch.full(scale_shape(R, C, axis, min(gs, R if axis == 0 else C)), float("nan"), dtype=torch.float32, device=dev)
    _hip.check(lib.lq_scale_init_group(_hip.ptr(p), _hip.ptr(s), qmin, qmax, S.ROUNDINGS.index(rounding), S.METHODS.index(method),
                                       min_value, R, C, axis, gs, _hip.stream_ptr(dev)), "lq_scale_init_group")
    return s


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=_ids)
def test_absmax_is_the_reference_bit_for_bit(dev, geo):
    R, C, axis, gs = geo
    P = S.make_input(*geo)
    for qmin, qmax in S.RANGES:
        got = _init(dev, P, axis, gs, qmin, qmax, "absmax").cpu().numpy()
        assert bits_equal(got, S.case_reference(*geo, qmin, qmax, "absmax")["s"]), (geo, qmin, qmax)


@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=_ids)
def test_lsq_is_within_one_ulp(dev, geo):
    R, C, axis, gs = geo
    P = S.make_input(*geo)
    for qmin, qmax in S.RANGES:
        got = _init(dev, P, axis, gs, qmin, qmax, "lsq").cpu().numpy()
        ref = S.case_reference(*geo, qmin, qmax, "lsq")["s"]
        assert np.isfinite(got).all()
        d = _ulps(got, ref)
        print(geo, (qmin, qmax), "lsq: max ulps", int(d.max()), "groups off", int((d > 0).sum()), "of", d.size)
        assert int(d.max()) <= 1


@pytest.mark.parametrize("rounding", S.ROUNDINGS)
@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=_ids)
def test_mse_is_the_reference_choice(dev, geo, rounding):
    R, C, axis, gs = geo
    P = S.make_input(*geo)
    for qmin, qmax in S.RANGES:
        got = _init(dev, P, axis, gs, qmin, qmax, "mse", rounding).cpu().numpy()
        ref = S.case_reference(*geo, qmin, qmax, "mse", rounding)
        same = got.view(np.int32) == ref["s"].view(np.int32)
        strict = (ref["gap"] == 0) | (ref["gap"] > S.GAP)
        runner = got.view(np.int32) == ref["runner"].view(np.int32)
        print(geo, (qmin, qmax), rounding, "mse: equal", int(same.sum()), "of", same.size, "strict", int(strict.sum()),
              "exact ties", int((ref["gap"] == 0).sum()))
        assert same[strict].all(), f"{int((~same[strict]).sum())} groups differ from the reference's choice"
        assert (same | runner)[~strict].all()


# ------------------------------------------------------------------------------------------- the invariants, by the project's own ops
def _backward_counts(dev, P, s, axis, gs, qmin, qmax, rounding):
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C = P.shape
    p = _t(P, dev)
    dy = torch.ones_like(p)
    dP = torch.empty_like(p)
    clipped = torch.full(s.shape, -1, dtype=torch.int32, device=dev)
    _hip.check(lib.lq_fq_backward_group(_hip.ptr(p), _hip.ptr(s), _hip.ptr(dy), qmin, qmax, S.ROUNDINGS.index(rounding), 1.0,
                                        _hip.ptr(dP), None, _hip.ptr(clipped), None, 0, R, C, axis, gs, _hip.stream_ptr(dev)),
               "lq_fq_backward_group")
    return clipped, dP


@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=_ids)
def test_nothing_is_clipped_after_absmax(dev, geo):
    """The project's own backward on the same data: every clip count is 0 for the signed ranges, both roundings, and dP == dy."""
    R, C, axis, gs = geo
    P = S.make_input(*geo)
    for qmin, qmax in ((-8, 7), (-2, 1)):
        s = _init(dev, P, axis, gs, qmin, qmax, "absmax")
        for rounding in S.ROUNDINGS:
            clipped, dP = _backward_counts(dev, P, s, axis, gs, qmin, qmax, rounding)
            assert int(clipped.abs().sum()) == 0, (geo, qmin, qmax, rounding, int((clipped != 0).sum()))
            assert bool((dP == 1).all())


@pytest.mark.parametrize("orientation", ["rowwise", "columnwise", "scalar"])
def test_nothing_is_clipped_after_absmax_one_axis(dev, orientation):
    """A one-axis scale through ops.scale_init_group(group_size=None) and the one-axis clipped backward's counts."""
    import learned_quantization_amd as lq
    P = S.make_input(96, 130, 0, 96)
    p = _t(P, dev)
    for qmin, qmax in ((-8, 7), (-2, 1)):
        for rounding in S.ROUNDINGS:
            s = torch.full(lq.scale_shape(P.shape, orientation), float("nan"), device=dev)
            assert lq.scale_init_group(p, s, qmin, qmax, None, "absmax", rounding=rounding) is s
            geo = {"rowwise": (96, 130, 1, 130), "columnwise": (96, 130, 0, 96), "scalar": (1, 96 * 130, 1, 96 * 130)}[orientation]
            assert lq.init_geometry(p.shape, p.stride(), s.shape) == geo
            ref = S.scale_init_reference(P.reshape(geo[0], geo[1]), qmin, qmax, geo[2], geo[3], "absmax")["s"]
            assert bits_equal(s.cpu().numpy().reshape(ref.shape), ref)
            _, _, clipped = lq.fq_backward_clip(p, s, torch.ones_like(p), qmin, qmax, want_ds=False, want_clipped=True, rounding=rounding)
            assert int(clipped.abs().sum()) == 0, (orientation, qmin, qmax, rounding)


@pytest.mark.parametrize("rounding", S.ROUNDINGS)
@pytest.mark.parametrize("geo", S.GEOMETRIES, ids=_ids)
def test_mse_error_is_not_above_absmax(dev, geo, rounding):
    """sum (P - out)^2 per group, recomputed from lq_fq_forward_group's out, under the mse scales and under the absmax scales."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = geo
    P = S.make_input(*geo)
    p = _t(P, dev)
    for qmin, qmax in S.RANGES:
        errs = []
        for method in ("mse", "absmax"):
            s = _init(dev, P, axis, gs, qmin, qmax, method, rounding)
            out = torch.empty_like(p)
            _hip.check(lib.lq_fq_forward_group(_hip.ptr(p), _hip.ptr(s), _hip.ptr(out), None, 0, qmin, qmax, S.ROUNDINGS.index(rounding),
                                               R, C, axis, gs, _hip.stream_ptr(dev)), "lq_fq_forward_group")
            errs.append(S.squared_error(P, out.cpu().numpy(), axis, gs))
        print(geo, (qmin, qmax), rounding, "summed error mse / absmax:", float(errs[0].sum() / max(errs[1].sum(), 1e-300)))
        assert (errs[0] <= errs[1]).all(), f"{int((errs[0] > errs[1]).sum())} groups worse than absmax"


# ------------------------------------------------------------------------------------------------------ memory and alignment
@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("case", [(256, 260, 0, 32, 4), (33, 4100, 1, 128, 4), (256, 260, 0, 32, 0), (33, 4100, 1, 128, 0),
                                  (37, 5, 0, 8, 8), (7, 27, 1, 8, 12)], ids=_ids)
def test_arena_alignment_and_determinism(dev, case, method):
    """Every pointer carved out of a poisoned arena, P at ``residue`` bytes off the 16-byte grid: s is the reference's, fully
    written, no guard byte is touched, P is unchanged, and a second run gives the same bits."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs, residue = case
    geo = (R, C, axis, gs)
    P = S.make_input(*geo)
    shape = scale_shape(R, C, axis, gs)
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=residue, row_bytes=C * 4)
    ar.add("s", "out", nbytes=int(np.prod(shape)) * 4, residue=(residue + 4) % 16, row_bytes=shape[1] * 4)
    ar.build()
    assert ar.ptr("P") % 16 == residue
    runs = []
    for _ in range(2):
        ar.fill("s", 0x7F)
        _hip.check(lib.lq_scale_init_group(ar.ptr("P"), ar.ptr("s"), -8, 7, 1, S.METHODS.index(method), MV, R, C, axis, gs,
                                           _hip.stream_ptr(dev)), "lq_scale_init_group")
        torch.cuda.synchronize(dev)
        ar.check(f"{case} {method}")
        runs.append(ar.numpy("s", np.float32).reshape(shape).copy())
    assert bits_equal(runs[0], runs[1])
    ref = S.case_reference(*geo, -8, 7, method, "nearest")
    if method == "lsq":
        assert int(_ulps(runs[0], ref["s"]).max()) <= 1
    else:
        assert bits_equal(runs[0], ref["s"])          # mse: these cases have no gap in (0, 1e-9] (test_scale_init_cpu.py)


# ------------------------------------------------------------------------------------------------------------ special groups
@pytest.mark.parametrize("method", S.METHODS)
@pytest.mark.parametrize("geo", [(256, 260, 0, 32), (37, 5, 0, 8), (64, 576, 1, 128), (7, 27, 1, 8)], ids=_ids)
def test_zero_nan_and_inf_groups(dev, geo, method):
    R, C, axis, gs = geo
    P = np.array(S.make_input(*geo))
    # group 0 of line 1: zeros; group 1 of line 2: one NaN; the last (short) group of line 3: one +Inf
    nb = -(-(R if axis == 0 else C) // gs)
    lines = P.T if axis == 0 else P          # a view: a line is a column (axis 0) or a row (axis 1)
    lines[1, 0:gs] = 0.0
    lines[2, gs + 1] = np.nan
    lines[3, -1] = np.inf
    clean = _init(dev, S.make_input(*geo), axis, gs, -8, 7, method).cpu().numpy()
    got = _init(dev, P, axis, gs, -8, 7, method).cpu().numpy()
    at = (lambda line, g: (g, line)) if axis == 0 else (lambda line, g: (line, g))
    assert got[at(1, 0)] == np.float32(MV)
    assert np.isnan(got[at(2, 1)]) and np.isnan(got[at(3, nb - 1)])
    other = np.ones(got.shape, bool)
    for k in (at(1, 0), at(2, 1), at(3, nb - 1)):
        other[k] = False
    assert bits_equal(got[other], clean[other]) and np.isfinite(got[other]).all()
    ref = S.scale_init_reference(P, -8, 7, axis, gs, method)
    assert np.array_equal(np.isnan(got), ref["bad"])
    if method == "absmax":
        assert bits_equal(got, ref["s"])


# --------------------------------------------------------------------------------------------------------------------- layers
def _memory_matrix(param, geometry):
    """The parameter's elements in memory order as the [R][C] matrix of ``geometry``."""
    from learned_quantization_amd.descriptor import memory_order
    order = memory_order(param.shape, param.stride())
    return param.detach().permute(*order).contiguous().cpu().numpy().reshape(geometry[0], geometry[1])


def _check_nested(nested, param, method):
    import learned_quantization_amd as lq
    geo = lq.init_geometry(param.shape, param.stride(), nested.scale.shape, nested.group_size)
    ref = S.scale_init_reference(_memory_matrix(param, geo), *nested.q_range, geo[2], geo[3], method, rounding=nested.rounding)
    got = nested.scale.detach().cpu().numpy().reshape(ref["s"].shape)
    if method == "lsq":
        assert int(_ulps(got, ref["s"]).max()) <= 1
    else:
        ok = got.view(np.int32) == ref["s"].view(np.int32)
        if method == "mse":
            ok |= (got.view(np.int32) == ref["runner"].view(np.int32)) & (ref["gap"] > 0) & (ref["gap"] <= S.GAP)
        assert ok.all()
    return geo


@pytest.mark.parametrize("method", S.METHODS)
def test_every_geometry_branch_through_the_layers(dev, method):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    init = lq.RandomNormal(seed=11)
    seen = set()
    for orientation, kw in (("rowwise", {}), ("columnwise", {}), ("scalar", {}), ("groupwise", {"group_size": 8})):
        d = lq.CustomDenseLayer(units=6, orientation=orientation, initializer=init, input_shape=20, device=dev, scale_gradient="ste",
                                bits=4, rounding="nearest", **kw)
        d.init_scales(method)
        seen.add(("dense", orientation) + _check_nested(d.nested_q_w_layer, d.W, method)[2:3])
        assert _check_nested(d.nested_q_b_layer, d.b, method) == (1, 6, 1, 6)
    for storage, orientation, kw in (("oihw", "scalar", {}), ("oihw", "columnwise", {}), ("oihw", "groupwise", {"group_size": 16}),
                                     ("hwio", "scalar", {}), ("hwio", "rowwise", {})):
        c = lq.CustomConv2DLayer(filters=8, orientation=orientation, initializer=init, input_shape=4, device=dev, scale_gradient="ste",
                                 q_range=(-2, 1), kernel_storage=storage, **kw)
        c.init_scales(method)
        seen.add((storage, orientation) + _check_nested(c.nested_q_k_layer, c.kernel, method)[2:3])
        _check_nested(c.nested_q_b_layer, c.b, method)
    assert {k[2] for k in seen} == {0, 1}
    for storage, orientation in (("oihw", "rowwise"), ("oihw", "channelwise"), ("hwio", "columnwise"), ("hwio", "channelwise")):
        c = lq.CustomConv2DLayer(filters=8, orientation=orientation, initializer=init, input_shape=4, device=dev, scale_gradient="ste",
                                 bits=4, kernel_storage=storage)
        with pytest.raises(ValueError, match="not lines of a matrix"):
            c.init_scales(method)


def test_init_scales_names_the_layer_of_a_nan(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    model = lq.build_model("mnist", seed=3, mode="ste", value=0.0, bits=4, group_size=64, device=dev, scale_init="absmax")
    layers = lq.custom_layers_of(model)
    for layer in layers:
        for _, nested, _ in layer.scale_pairs():
            assert bool(torch.isfinite(nested.scale).all()) and bool((nested.scale > lq.SCALE_INIT).any())
    before = [n.scale.data_ptr() for l in layers for _, n, _ in l.scale_pairs()]
    with torch.no_grad():
        layers[1].W[3, 2] = float("nan")
    for method in S.METHODS:
        with pytest.raises(ValueError, match=repr(layers[1].name)) as e:
            lq.init_scales(model, method)
        assert "'W'" in str(e.value) and repr(layers[0].name) not in str(e.value)
    assert before == [n.scale.data_ptr() for l in layers for _, n, _ in l.scale_pairs()]      # written in place


# -------------------------------------------------------------------------------------------------------------------- harness
def _batch(dev):
    """The zero-mean batch of tests/test_gpu_groupwise.py's fixture (under raw 0..255 pixels most hidden units are switched off)."""
    from learned_quantization_amd.train import synthetic_batch
    gen = torch.Generator(device=dev).manual_seed(0)
    y = synthetic_batch("mnist", 32, dev, gen)[1]
    return torch.randn(32, 1, 28, 28, device=dev, generator=gen), y


def _weights(tr):
    return [l.W for l in tr.custom_layers]


def _nonzero_share(tr):
    return [float((w.grad != 0).float().mean()) for w in _weights(tr)]


@pytest.mark.parametrize("method", S.METHODS)
def test_trainer_trains_from_initialised_scales(dev, tmp_path, method):
    """Trainer(config="mnist", mode="ste", bits=4, group_size=64, scale_init=m), three steps: finite losses, eager and graphed equal
    bit for bit, after the first backward at least half of every W.grad is nonzero, every group-wise scale has a gradient in
    some step."""
    from learned_quantization_amd.train import Trainer
    x, y = _batch(dev)
    runs = []
    for graph in (False, True):
        tr = Trainer(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path / f"g{int(graph)}"), graph=graph, seed=7,
                     bits=4, group_size=64, lr=1e-3, scale_init=method)
        scales = [l.nested_q_w_layer.scale for l in tr.custom_layers]
        assert all(bool((s > 1e-4).all()) for s in scales)                                   # far from SCALE_INIT = 1.19e-5
        step = tr.step_graphed if graph else tr.step
        losses, seen = [], [torch.zeros_like(s, dtype=torch.bool) for s in scales]
        for i in range(3 + (0 if graph else 3)):                                             # step_graphed: 3 eager warm-up steps first
            losses.append(step(x, y).detach().clone())
            if not graph:
                seen = [m | (s.grad != 0) for m, s in zip(seen, scales)]
                if i == 0:
                    share = _nonzero_share(tr)
                    print(method, "nonzero share of W.grad after the first backward:", share)
                    assert min(share) >= 0.5
        torch.cuda.synchronize()
        runs.append((tr, losses[-3:], seen))
    (eager, le, seen), (graphed, lg, _) = runs
    assert all(np.isfinite(float(a)) for a in le)
    for a, b in zip(le, lg):
        assert torch.equal(a, b), f"losses differ: {float(a)!r} {float(b)!r}"
    for layer, had in zip(eager.custom_layers, seen):
        assert bool(had.all()), f"{layer.name}: {int((~had).sum())} group-wise scales never had a gradient"


def test_without_scale_init_nothing_trains(dev, tmp_path):
    """The contrast: at SCALE_INIT every weight is clipped (|W| < 8 s is about 0.15 % of N(0, 0.05)) and under 1 % of W.grad is
    nonzero; the same trainer with scale_init="absmax" passes a gradient to more than half of every W."""
    from learned_quantization_amd.train import Trainer
    x, y = _batch(dev)
    shares = {}
    for method in (None, "absmax"):
        tr = Trainer(config="mnist", mode="ste", value=0.0, device=dev, log_dir=str(tmp_path / str(method)), seed=7, bits=4,
                     group_size=64, lr=1e-3, scale_init=method)
        assert np.isfinite(float(tr.step(x, y).detach()))
        shares[method] = _nonzero_share(tr)
    print("nonzero share of W.grad:", shares)
    assert max(shares[None]) < 0.01
    assert min(shares["absmax"]) >= 0.5


def test_train_cli_with_scale_init(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "learned_quantization_amd.train", "--config", "mnist", "--mode", "ste", "--bits", "4",
                        "--group-size", "64", "--scale-init", "mse", "--steps", "3", "--warmup", "0"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["scale_init"] == "mse" and line["group_size"] == 64 and np.isfinite(line["final_loss"])
