"""GPU tests of the per-group quantization statistics (include/lq_hip.h: lq_group_stats; ops.group_stats / summarize_stats,
CustomQuantizedScaleLayer.quant_stats, layers.quant_stats, tracking.GroupQuantTrackingCallback, the drivers) against
tests/_group_stats_reference.py.

Inputs: _group_reference.make_case / _group_affine_reference.make_affine_case on _group_stats_reference.GEOMETRIES, the smallest
that reach every launch form; tests/test_group_stats_cpu.py asserts on the reference alone what these tests rely on (both sides
clip a sizeable share, no bin is empty).  Bounds:

  below, above, hist   equal to the reference exactly, and to the shipped kernels: below + above == clipped of the group-wise
                       backward on the same buffers, hist == bincount(q - qmin) of the forward's int32 view.
  err2, sig2           within 2^-30 relative of the float64 reference.  Derived, not measured: every term is non-negative and no
                       group has more than 2^20 elements, so any order of f64 additions plus the rounding of each product stays
                       within 2 n 2^-53 <= 2^-32 of the exact sum; the same holds for NumPy's own sum; 2^-30 covers both.
  two runs             the same bits.

Which case launches which instantiation (the vector forms need C % 4 == 0 -- and gs % 4 == 0 on axis 1 -- and a 16-byte aligned P):
  k_stats_cols V = 4   (200, 64, 64: ragged last group) (33000, 4, 1: second trip of the group loop)
  k_stats_cols V = 1   (50, 7, 20) (96, 130, 96), and (200, 64, 64) one float off the 16-byte grid
  k_stats_rows V = 4   (9, 200, 64: team 4) (5, 1100, 256: team 16) (3, 2600, 1024: team 64)
  k_stats_rows V = 1   (70, 12, 3: team 1) (7, 333, 50: team 16) (3, 1001, 333: team 64, last group 2) (1, 130, 130: a bias), and
                       (5, 1100, 256) one float off the 16-byte grid"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _group_stats_reference as G                                                    # noqa: E402
import _scale_init_reference as S                                                     # noqa: E402
from _arena import Arena                                                              # noqa: E402
from _group_affine_reference import make_affine_case                                  # noqa: E402
from _group_reference import make_case, scale_shape                                   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731
SEED = 20                                                                       # tests/test_group_stats_cpu.py checks this seed
ROUNDINGS = ("floor", "nearest")
CONFIGS = [(qmin, qmax, rounding, False) for qmin, qmax, rounding in G.RANGES] + [(-8, 7, "floor", True), (-8, 7, "nearest", True)]
_CASES, _REFS = {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(geo, affine):
    """(P, s, b or None) of a geometry, made once per process and never modified."""
    key = (geo, affine)
    if key not in _CASES:
        if affine:
            P, s, b, _ = make_affine_case(SEED, *geo)
        else:
            (P, s, _), b = make_case(SEED, *geo), None
        for a in (P, s, b):
            if a is not None:
                a.setflags(write=False)
        _CASES[key] = (P, s, b)
    return _CASES[key]


def _ref(geo, qmin, qmax, rounding, affine):
    """The reference of one case, computed once per process and shared."""
    key = (geo, qmin, qmax, rounding, affine)
    if key not in _REFS:
        P, s, b = _case(geo, affine)
        _REFS[key] = G.group_stats_reference(P, s, qmin, qmax, geo[2], geo[3], b=b, rounding=rounding)
    return _REFS[key]


def _t(a, dev, off=0):
    """A device copy of ``a`` (the shared inputs are read-only); ``off`` floats off the allocation's 16-byte grid."""
    a = np.array(a, order="C")
    if not off:
        return torch.from_numpy(a).to(dev)
    buf = torch.empty(a.size + off, dtype=torch.float32, device=dev)
    view = buf[off:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * off
    return view


def _stats(dev, P, s, b, qmin, qmax, rounding, axis, gs, hist=True, prefill=0):
    """lq_group_stats through the C ABI on device tensors; the four group outputs start as the byte 0x7F (an unwritten group
    shows), the bins as ``prefill``.  Returns host arrays: below, above, hist as int64, err2, sig2 as float64."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C = P.shape
    shape = tuple(s.shape)
    below = torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev)
    above = torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev)
    err2 = torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    sig2 = torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    h = torch.full((qmax - qmin + 1,), prefill, dtype=torch.int32, device=dev) if hist else None
    _hip.check(lib.lq_group_stats(_hip.ptr(P), _hip.ptr(s), _hip.ptr(b), qmin, qmax, ROUNDINGS.index(rounding), _hip.ptr(below),
                                  _hip.ptr(above), _hip.ptr(err2), _hip.ptr(sig2), _hip.ptr(h), R, C, axis, gs, _hip.stream_ptr(dev)),
               "lq_group_stats")
    u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)      # noqa: E731
    return dict(below=u32(below), above=u32(above), err2=err2.cpu().numpy(), sig2=sig2.cpu().numpy(), hist=None if h is None else u32(h))


def _check(got, ref, what):
    assert np.array_equal(got["below"], ref["below"]), what
    assert np.array_equal(got["above"], ref["above"]), what
    if got["hist"] is not None:
        assert np.array_equal(got["hist"], ref["hist"]), (what, got["hist"], ref["hist"])
    for k in ("err2", "sig2"):
        with np.errstate(all="ignore"):
            rel = np.nanmax(np.abs(got[k] - ref[k]) / np.abs(ref[k]))
        print(f"{what} {k}: largest relative difference {rel:.3e} (bound {G.REL:.3e})")
        assert G.close(got[k], ref[k]), (what, k, rel)


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("geo", G.GEOMETRIES, ids=_ids)
def test_every_form_against_the_reference_and_the_shipped_kernels(dev, geo):
    import learned_quantization_amd as lq
    R, C, axis, gs = geo
    for affine in (False, True):
        P, s, b = _case(geo, affine)
        p, sd, bd = _t(P, dev), _t(s, dev), (_t(b, dev) if affine else None)
        dy = torch.ones_like(p)
        for qmin, qmax, rounding, aff in CONFIGS:
            if aff != affine:
                continue
            what = f"{geo} [{qmin}, {qmax}] {rounding}{' affine' if affine else ''}"
            got = _stats(dev, p, sd, bd, qmin, qmax, rounding, axis, gs)
            _check(got, _ref(geo, qmin, qmax, rounding, affine), what)
            assert _same_bits(got, _stats(dev, p, sd, bd, qmin, qmax, rounding, axis, gs)), what      # two runs, the same bits
            # the shipped kernels on the same buffers
            if affine:
                clipped = lq.fq_backward_group_affine(p, sd, bd, dy, qmin, qmax, gs, want_ds=False, want_db=False, want_clipped=True,
                                                      rounding=rounding)[3]
                q = lq.fq_forward_group_affine(p, sd, bd, qmin, qmax, gs, q_dtype=torch.int32, rounding=rounding)[1]
            else:
                clipped = lq.fq_backward_group(p, sd, dy, qmin, qmax, gs, want_ds=False, want_clipped=True, rounding=rounding)[2]
                q = lq.fq_forward_group(p, sd, qmin, qmax, gs, q_dtype=torch.int32, rounding=rounding)[1]
            assert np.array_equal(got["below"] + got["above"], clipped.cpu().numpy().view(np.uint32).astype(np.int64)), what
            assert np.array_equal(got["hist"], np.bincount(q.cpu().numpy().reshape(-1).astype(np.int64) - qmin, minlength=qmax - qmin + 1)), what


@pytest.mark.parametrize("geo", [(200, 64, 0, 64), (5, 1100, 1, 256)], ids=_ids)
def test_scalar_forms_one_float_off_the_16_byte_grid(dev, geo):
    R, C, axis, gs = geo
    for affine in (False, True):
        P, s, b = _case(geo, affine)
        p, sd, bd = _t(P, dev, off=1), _t(s, dev), (_t(b, dev) if affine else None)
        for qmin, qmax, rounding, aff in CONFIGS:
            if aff == affine:
                got = _stats(dev, p, sd, bd, qmin, qmax, rounding, axis, gs)
                _check(got, _ref(geo, qmin, qmax, rounding, affine), f"{geo} off the grid [{qmin}, {qmax}] {rounding} affine={affine}")


# ------------------------------------------------------------------------------------------------------------- range limits
@pytest.mark.parametrize("geo", [(200, 64, 0, 64), (7, 333, 1, 50)], ids=_ids)
def test_4096_bins_and_no_histogram(dev, geo):
    R, C, axis, gs = geo
    P, s, _ = _case(geo, False)
    s = (s / np.float32(64.0)).astype(np.float32)          # |t| up to ~ 8 * 64 * 4: the codes spread over hundreds of bins, some clip
    p, sd = _t(P, dev), _t(s, dev)
    ref = G.group_stats_reference(P, s, -2048, 2047, axis, gs)
    assert ref["hist"].size == 4096 and np.count_nonzero(ref["hist"]) > 500
    got = _stats(dev, p, sd, None, -2048, 2047, "floor", axis, gs)
    _check(got, ref, f"{geo} 4096 bins")
    bare = _stats(dev, p, sd, None, -2048, 2047, "floor", axis, gs, hist=False)
    assert bare["hist"] is None and all(np.array_equal(bare[k].view(np.int64), got[k].view(np.int64)) for k in ("below", "above", "err2", "sig2"))
    # a wider range has no histogram; the other four are served
    wide = _stats(dev, p, sd, None, -4096, 4095, "floor", axis, gs, hist=False)
    _check(wide, G.group_stats_reference(P, s, -4096, 4095, axis, gs), f"{geo} 8192 codes, no histogram")
    from learned_quantization_amd import ops
    with pytest.raises(ValueError, match="4096"):
        ops.group_stats(p, sd, -4096, 4095, gs)


# ---------------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("affine", [False, True], ids=["symmetric", "affine"])
def test_nan_and_inf_spoil_their_own_group_only(dev, affine):
    geo = (7, 333, 1, 50)
    R, C, axis, gs = geo
    P, s, b = _case(geo, affine)
    clean = _stats(dev, _t(P, dev), _t(s, dev), _t(b, dev) if affine else None, -8, 7, "floor", axis, gs)
    bad = np.array(P)
    bad[2, 3 * gs + 7] = np.nan          # row 2, group 3
    bad[5, 1 * gs + 49] = np.inf         # row 5, group 1
    got = _stats(dev, _t(bad, dev), _t(s, dev), _t(b, dev) if affine else None, -8, 7, "floor", axis, gs)
    ref = G.group_stats_reference(bad, s, -8, 7, axis, gs, b=b)
    _check(got, ref, f"{geo} non-finite affine={affine}")
    assert np.isnan(got["err2"][2, 3]) and np.isnan(got["sig2"][2, 3]) and got["hist"].sum() == R * C - 1
    was_above = G.group_stats_reference(P, s, -8, 7, axis, gs, b=b)["q0"][5, gs + 49] > 7
    assert got["above"][5, 1] == clean["above"][5, 1] + (0 if was_above else 1) and np.isinf(got["err2"][5, 1])
    keep = np.ones(got["err2"].shape, bool)
    keep[2, 3] = keep[5, 1] = False
    for k in ("below", "above", "err2", "sig2"):
        assert np.array_equal(got[k][keep].view(np.int64), clean[k][keep].view(np.int64)), k      # every other group keeps its bits


# ----------------------------------------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize("geo,residue", [((200, 64, 0, 64), 0), ((200, 64, 0, 64), 4), ((50, 7, 0, 20), 0), ((5, 1100, 1, 256), 0),
                                         ((5, 1100, 1, 256), 12), ((3, 1001, 1, 333), 8), ((1, 130, 1, 130), 0)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else f"r{v}")
def test_memory_contract(dev, geo, residue):
    """Guard bands around P, s, b and all five outputs: nothing outside the stated extents changes, the inputs stay as they
    were, every group output is written, and the bins are ADDED to."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = geo
    for affine in (False, True):
        P, s, b = _case(geo, affine)
        ref = _ref(geo, -8, 7, "nearest", affine)
        a = Arena(dev)
        a.add("P", "in", data=P, residue=residue, row_bytes=C * 4)
        a.add("s", "in", data=s, residue=4)
        if affine:
            a.add("b", "in", data=b, residue=8)
        for name, width, res in (("below", 4, 4), ("above", 4, 12), ("err2", 8, 8), ("sig2", 8, 0)):
            a.add(name, "out", nbytes=s.size * width, residue=res)
        a.add("hist", "inout", data=np.full(16, 7, np.uint32), residue=4)
        a.build()
        _hip.check(lib.lq_group_stats(a.ptr("P"), a.ptr("s"), a.ptr("b") if affine else None, -8, 7, 1, a.ptr("below"), a.ptr("above"),
                                      a.ptr("err2"), a.ptr("sig2"), a.ptr("hist"), R, C, axis, gs, _hip.stream_ptr(dev)), "lq_group_stats")
        torch.cuda.synchronize(dev)
        a.check(f"{geo} residue {residue} affine={affine}")
        got = dict(below=a.numpy("below", np.uint32).astype(np.int64).reshape(s.shape),
                   above=a.numpy("above", np.uint32).astype(np.int64).reshape(s.shape),
                   err2=a.numpy("err2", np.float64).reshape(s.shape), sig2=a.numpy("sig2", np.float64).reshape(s.shape),
                   hist=a.numpy("hist", np.uint32).astype(np.int64) - 7)
        _check(got, ref, f"{geo} in the arena, residue {residue}, affine={affine}")


# ---------------------------------------------------------------------------------------- consistency with scale initialisation
@pytest.mark.parametrize("geo", [(256, 260, 0, 32), (64, 576, 1, 128)], ids=_ids)
def test_consistency_with_scale_initialisation(dev, geo):
    import learned_quantization_amd as lq
    R, C, axis, gs = geo
    p = _t(S.make_input(*geo), dev)
    for qmin, qmax in S.RANGES:
        for rounding in ROUNDINGS:
            s_abs = lq.scale_init_group(p, torch.empty(scale_shape(*geo), device=dev), qmin, qmax, gs, "absmax", rounding=rounding)
            s_mse = lq.scale_init_group(p, torch.empty(scale_shape(*geo), device=dev), qmin, qmax, gs, "mse", rounding=rounding)
            e_abs = _stats(dev, p, s_abs, None, qmin, qmax, rounding, axis, gs)
            e_mse = _stats(dev, p, s_mse, None, qmin, qmax, rounding, axis, gs)
            # absmax covers every side whose bound is not zero (the header's statement): nothing is clipped there
            assert e_abs["above"].sum() == 0 and (qmin == 0 or e_abs["below"].sum() == 0), (geo, qmin, qmax, rounding)
            assert np.all(e_mse["err2"] <= e_abs["err2"] * (1 + G.REL)), (geo, qmin, qmax, rounding)
    P, s, b = _case((200, 64, 0, 64) if axis == 0 else (5, 1100, 1, 256), True)
    g2 = (200, 64, 0, 64) if axis == 0 else (5, 1100, 1, 256)
    pd = _t(P, dev)
    for rounding in ROUNDINGS:
        sd, bd = torch.empty(s.shape, device=dev), torch.empty(s.shape, device=dev)
        lq.scale_init_group_minmax(pd, sd, bd, -8, 7, g2[3], rounding=rounding)
        got = _stats(dev, pd, sd, bd, -8, 7, rounding, g2[2], g2[3])
        assert got["below"].sum() == 0 and got["above"].sum() == 0 and got["hist"].sum() == P.size, (g2, rounding)


# ---------------------------------------------------------------------------------------------------------- layers and drivers
def _model(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    return lq.build_model("mnist", mode="ste", value=0.0, seed=3, bits=4, group_size=32, asymmetric=True, scale_init="minmax", device=dev)


def test_layers_quant_stats_equals_the_op_by_hand(dev):
    import learned_quantization_amd as lq
    from learned_quantization_amd import export, ops
    model = _model(dev)
    with torch.no_grad():                                    # move the weights off their initial grid: something clips
        for _, param, _ in export.quantized_tensors(model):
            param.mul_(1.0 + 0.5 * torch.rand_like(param)).add_(0.001 * torch.randn_like(param))      # the biases start as zeros
    stats = lq.quant_stats(model)
    tensors = export.quantized_tensors(model)
    assert list(stats) == [name for name, _, _ in tensors] and len(stats) == 4
    some_clipped = False
    for name, param, nested in tensors:
        rec = ops.group_stats(param.data, nested.scale.data, *nested.q_range, nested.group_size,
                              offset=nested.offset.data if nested.asymmetric else None, rounding=nested.rounding)
        assert rec.below.dtype == rec.above.dtype == rec.hist.dtype == torch.int32 and rec.err2.dtype == rec.sig2.dtype == torch.float64
        assert rec.below.shape == rec.err2.shape == nested.scale.shape and rec.hist.numel() == 16
        by_hand = ops.summarize_stats(rec, param.numel())
        assert by_hand == stats[name] == ops.summarize_stats(nested.quant_stats(param), param.numel()), name
        assert set(by_hand) == {"clip_low", "clip_high", "sqnr_db", "worst_group_sqnr_db", "used_levels", "entropy_bits"}
        assert 0 <= by_hand["clip_low"] < 1 and 0 <= by_hand["clip_high"] < 1 and np.isfinite(by_hand["sqnr_db"])
        assert by_hand["worst_group_sqnr_db"] <= by_hand["sqnr_db"] and 1 <= by_hand["used_levels"] <= 16
        assert 0 <= by_hand["entropy_bits"] <= 4.0
        assert nested.quant_stats(param, want_hist=False).hist is None
        some_clipped |= by_hand["clip_low"] + by_hand["clip_high"] > 0
    assert some_clipped


def test_a_layer_without_a_range_raises(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev)
    layer = lq.custom_layers_of(model)[0]
    with pytest.raises(ValueError, match="needs bits or q_range"):
        layer.nested_q_w_layer.quant_stats(layer.W)
    with pytest.raises(ValueError, match="has no range"):
        lq.quant_stats(model)


def _blocks(path):
    lines = open(path).read().splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith("Epoch ")]
    return [lines[a + 1:b] for a, b in zip(heads, heads[1:] + [len(lines)])], [lines[i] for i in heads]


def test_tracking_callback_files(dev, tmp_path):
    import learned_quantization_amd as lq
    model = _model(dev)
    layer = lq.custom_layers_of(model)[0]
    cb = lq.GroupQuantTrackingCallback(layer, str(tmp_path))
    cb.on_train_begin()
    first = cb.on_epoch_end(0)
    cb.on_epoch_end(1)
    cb.on_train_end()
    groups = layer.nested_q_w_layer.scale.numel()
    files = cb.epoch_files()
    assert len(files) == 8 + 7 and len(set(files)) == len(files)          # kernel: with offsets; bias: without
    for f in files:
        blocks, heads = _blocks(f)
        assert heads == ["Epoch 0", "Epoch 1"], f
        base = os.path.basename(f)
        per_group = base.startswith(("Clip_low_", "Clip_high_", "Weights_", "Bias_")) or (base.startswith("SQNR_dB_") and "tensor" not in base)
        want = (groups if "Weights" in base else 1) if per_group else 1
        assert [len(b) for b in blocks] == [want, want], (f, [len(b) for b in blocks], want)
        # the bias starts as zeros: no error and no signal, its SQNR is written as inf
        assert all(not np.isnan(float(v)) and ("Bias" in base or np.isfinite(float(v))) for b in blocks for v in b), f
    for d, prefix in (("on_train_begin", "Unique_initial_quantized_"), ("on_train_end", "Unique_quantized_")):
        names = sorted(os.listdir(os.path.join(str(tmp_path), d)))
        assert len(names) == 2 and all(n.startswith(prefix) for n in names), names
        for n, numel in zip(names, (layer.b.numel(), layer.W.numel())):      # "Bias..." sorts before "Weights..."
            rows = [l.split(", ") for l in open(os.path.join(str(tmp_path), d, n)).read().splitlines()]
            assert 1 <= len(rows) <= 16 and sum(int(c) for _, c in rows) == numel and all(-8 <= float(v) <= 7 for v, _ in rows)
    assert cb.stats() == first and set(first) == {"kernel", "bias"}
    assert first["kernel"] == lq.quant_stats(model)[layer.name + "/W"]


def test_experiment_driver_logs_groupwise_layers(dev, tmp_path):
    res = subprocess.run([sys.executable, "-m", "learned_quantization_amd.experiment", "--seed", "42", "--epochs", "2", "--steps-per-epoch", "3",
                          "--batch", "16", "--log-root", str(tmp_path), "--config", "mnist", "--orientation", "rowwise", "--training",
                          "from_scratch", "--bits", "4", "--group-size", "32", "--scale-gradient", "ste"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["group_size"] == 32 and "first_layer_unique_integers" not in out
    for key in ("first_layer_sqnr_db", "first_layer_clip_low", "first_layer_clip_high"):
        assert isinstance(out[key], float), key
    assert 0 <= out["first_layer_clip_low"] <= 1 and 0 <= out["first_layer_clip_high"] <= 1
    d = out["log_dir"]
    epoch = os.listdir(os.path.join(d, "on_epoch_end"))
    for prefix in ("Clip_low_Weights", "Clip_high_Weights", "SQNR_dB_Weights", "SQNR_dB_tensor_Weights", "Used_levels_Weights",
                   "Code_entropy_bits_Weights", "Weights_", "Clip_low_Bias", "SQNR_dB_Bias", "Bias_"):
        assert any(n.startswith(prefix) for n in epoch), (prefix, epoch)
    blocks, heads = _blocks(os.path.join(d, "on_epoch_end", next(n for n in epoch if n.startswith("SQNR_dB_tensor_Weights"))))
    assert heads == ["Epoch 0", "Epoch 1"] and [len(b) for b in blocks] == [1, 1]
    assert len(os.listdir(os.path.join(d, "on_train_begin"))) == 4 and len(os.listdir(os.path.join(d, "on_train_end"))) == 4      # two layers, kernel and bias


def test_train_driver_quant_stats_flag(dev, capsys):
    from learned_quantization_amd import train
    train.main(["--config", "mnist", "--mode", "ste", "--bits", "4", "--group-size", "64", "--scale-init", "mse", "--batch", "32",
                "--steps", "2", "--warmup", "1", "--quant-stats"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(line["quant_stats"]) == 4 and all(np.isfinite(v["sqnr_db"]) and v["used_levels"] >= 1 for v in line["quant_stats"].values())
    train.main(["--config", "mnist", "--mode", "ste", "--bits", "4", "--group-size", "64", "--batch", "32", "--steps", "1", "--warmup", "0"])
    assert "quant_stats" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
