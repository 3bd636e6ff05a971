"""GPU tests of the per-group statistics of the microscaling quantizer (include/lq_hip.h: lq_mx_stats; ops.mx_stats /
summarize_mx_stats, CustomQuantizedScaleLayer.mx_stats, layers.mx_quant_stats, tracking.MxQuantTrackingCallback, the drivers)
against tests/_mx_stats_reference.py.

Inputs: _mx_reference.loguniform_case on _group_stats_reference.GEOMETRIES, the smallest that reach every launch form;
tests/test_mx_stats_cpu.py asserts on the reference alone what these tests rely on (elements saturate on both sides, are flushed
and land on subnormal codes).  Bounds:

  below, above, flushed, hist   equal to the reference exactly, and to the shipped kernels: below + above == clipped of the
                                microscaling backward on the same buffers, hist == bincount of the forward's int32 code view.
  err2, sig2                    within 2^-30 relative of the float64 reference.  Derived, not measured: every term is non-negative
                                and no group has more than 2^20 elements, so any order of f64 additions plus the rounding of each
                                product stays within 2 n 2^-53 <= 2^-32 of the exact sum; the same holds for NumPy's own sum;
                                2^-30 covers both (the head of tests/test_gpu_group_stats.py).
  two runs                      the same bits.

Which case launches which instantiation (the vector forms need C % 4 == 0 -- and gs % 4 == 0 on axis 1 -- and a 16-byte aligned P):
  k_mx_stats_cols V = 4   (200, 64, 64: ragged last group) (33000, 4, 1: second trip of the group loop)
  k_mx_stats_cols V = 1   (50, 7, 20) (96, 130, 96), and (200, 64, 64) one float off the 16-byte grid
  k_mx_stats_rows V = 4   (9, 200, 64: team 4) (5, 1100, 256: team 16) (3, 2600, 1024: team 64)
  k_mx_stats_rows V = 1   (70, 12, 3: team 1) (7, 333, 50: team 16) (3, 1001, 333: team 64, last group 2) (1, 130, 130: a bias), and
                          (5, 1100, 256) one float off the 16-byte grid"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _mx_stats_reference as M                                                       # noqa: E402
from _arena import Arena                                                              # noqa: E402
from _mx_reference import FORMATS                                                     # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731
SCALE_FORMATS = ("e8m0", "fp32")
COUNTS = ("below", "above", "flushed")
GROUP_OUTPUTS = COUNTS + ("err2", "sig2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


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


def _u32(t):
    return t.cpu().numpy().view(np.uint32).astype(np.int64)


def _buffers(dev, shape, bits, hist=True, prefill=0):
    """The six outputs on the device: the group outputs start as the byte 0x7F / -7.0 (an unwritten group shows), the bins as
    ``prefill``."""
    out = {k: torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device=dev) for k in COUNTS}
    out.update({k: torch.full(shape, -7.0, dtype=torch.float64, device=dev) for k in ("err2", "sig2")})
    out["hist"] = torch.full((1 << bits,), prefill, dtype=torch.int32, device=dev) if hist else None
    return out


def _launch(dev, P, s, name, sf, axis, gs, o):
    from learned_quantization_amd import _hip
    R, C = P.shape
    _hip.check(_hip.load().lq_mx_stats(_hip.ptr(P), _hip.ptr(s), FORMATS[name].id, SCALE_FORMATS.index(sf), _hip.ptr(o["below"]),
                                       _hip.ptr(o["above"]), _hip.ptr(o["flushed"]), _hip.ptr(o["err2"]), _hip.ptr(o["sig2"]),
                                       _hip.ptr(o["hist"]), R, C, axis, gs, _hip.stream_ptr(dev)), "lq_mx_stats")


def _host(o):
    got = {k: _u32(o[k]) for k in COUNTS}
    got.update(err2=o["err2"].cpu().numpy(), sig2=o["sig2"].cpu().numpy(), hist=None if o["hist"] is None else _u32(o["hist"]))
    return got


def _stats(dev, P, s, name, sf, axis, gs, hist=True, prefill=0):
    """lq_mx_stats through the C ABI on device tensors.  Returns host arrays: the counts and hist as int64, err2, sig2 as float64."""
    o = _buffers(dev, tuple(s.shape), FORMATS[name].bits, hist, prefill)
    _launch(dev, P, s, name, sf, axis, gs, o)
    return _host(o)


def _check(got, ref, what):
    for k in COUNTS:
        assert np.array_equal(got[k], ref[k]), (what, k)
    if got["hist"] is not None:
        assert np.array_equal(got["hist"], ref["hist"]), (what, got["hist"], ref["hist"])
    for k in ("err2", "sig2"):
        with np.errstate(all="ignore"):
            rel = np.nanmax(np.abs(got[k] - ref[k]) / np.abs(ref[k]))
        print(f"{what} {k}: largest relative difference {rel:.3e} (bound {M.REL:.3e})")
        assert M.close(got[k], ref[k]), (what, k, rel)


def _same_bits(a, b, keys=None):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in (keys or a))


# ------------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("geo", M.GEOMETRIES, ids=_ids)
def test_every_form_against_the_reference_and_the_shipped_kernels(dev, geo):
    import learned_quantization_amd as lq
    R, C, axis, gs = geo
    for name, sf, g in M.gpu_cases():
        if g != geo:
            continue
        what = f"{name} {sf} {geo}"
        P, s = M.case(name, sf, geo)
        ref = M.reference(name, sf, geo)
        p, sd = _t(P, dev), _t(s, dev)
        got = _stats(dev, p, sd, name, sf, axis, gs)
        _check(got, ref, what)
        assert _same_bits(got, _stats(dev, p, sd, name, sf, axis, gs)), what                      # two runs, the same bits
        bare = _stats(dev, p, sd, name, sf, axis, gs, hist=False)                                 # hist = NULL: the five group outputs the same
        assert bare["hist"] is None and _same_bits(bare, got, GROUP_OUTPUTS), what
        # the shipped kernels on the same buffers
        clipped = lq.fq_backward_mx(p, sd, torch.ones_like(p), name, gs, sf, want_ds=False, want_clipped=True)[2]
        assert np.array_equal(got["below"] + got["above"], _u32(clipped)), what
        out, code = lq.fq_forward_mx(p, sd, name, gs, sf, q_dtype=torch.int32)
        out, code = out.cpu().numpy(), code.cpu().numpy()
        number = ~np.isnan(out)
        assert np.array_equal(got["hist"], np.bincount(code[number].astype(np.int64), minlength=1 << FORMATS[name].bits)), what
        e = P.astype(np.float64) - out.astype(np.float64)
        assert M.close(got["err2"], M._sums(e * e, R, C, axis, min(gs, R if axis == 0 else C))), what


@pytest.mark.parametrize("geo", [(200, 64, 0, 64), (5, 1100, 1, 256)], ids=_ids)
def test_scalar_forms_one_float_off_the_16_byte_grid(dev, geo):
    R, C, axis, gs = geo
    for name, sf in (("fp4_e2m1", "e8m0"), ("fp8_e4m3", "fp32")):
        P, s = M.case(name, sf, geo)
        got = _stats(dev, _t(P, dev, off=1), _t(s, dev), name, sf, axis, gs)
        _check(got, M.reference(name, sf, geo), f"{name} {sf} {geo} off the grid")


# ------------------------------------------------------------------------------------------------------------- bins are added
@pytest.mark.parametrize("geo", [(200, 64, 0, 64), (7, 333, 1, 50)], ids=_ids)
def test_bins_are_added(dev, geo):
    R, C, axis, gs = geo
    name, sf = "fp6_e2m3", "e8m0"
    P, s = M.case(name, sf, geo)
    got = _stats(dev, _t(P, dev), _t(s, dev), name, sf, axis, gs, prefill=7)
    got["hist"] = got["hist"] - 7
    _check(got, M.reference(name, sf, geo), f"{name} {sf} {geo} prefilled bins")


# ---------------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("geo", [(9, 200, 1, 64), (200, 64, 0, 64)], ids=_ids)
def test_non_finite_values_spoil_their_own_group_only(dev, geo):
    R, C, axis, gs = geo
    name, sf = "fp4_e2m1", "e8m0"
    fmt = FORMATS[name]
    P, s = M.case(name, sf, geo)
    clean = _stats(dev, _t(P, dev), _t(s, dev), name, sf, axis, gs)
    # (element, group) of the NaN, of the +Inf and an element of the group under the zero scale, each group apart
    if axis == 1:
        (nan_at, nan_g), (inf_at, inf_g), zero_g = ((2, 3 * gs + 7), (2, 3)), ((5, 1 * gs + 49), (5, 1)), (7, 0)
        members = lambda g: (slice(g[0], g[0] + 1), slice(g[1] * gs, min((g[1] + 1) * gs, C)))      # noqa: E731
    else:
        (nan_at, nan_g), (inf_at, inf_g), zero_g = ((3 * gs + 7, 2), (3, 2)), ((1 * gs + 49, 5), (1, 5)), (0, 7)
        members = lambda g: (slice(g[0] * gs, min((g[0] + 1) * gs, R)), slice(g[1], g[1] + 1))      # noqa: E731
    bad, bad_s = np.array(P), np.array(s)
    bad[nan_at] = np.nan
    bad[inf_at] = np.inf
    bad_s[zero_g] = 0.0                              # an invalid E8M0 scale: s_eff is NaN
    got = _stats(dev, _t(bad, dev), _t(bad_s, dev), name, sf, axis, gs)
    ref = M.mx_stats_reference(bad, bad_s, fmt, sf, axis, gs)
    _check(got, ref, f"{geo} non-finite")
    n_zero = bad[members(zero_g)].size
    assert got["hist"].sum() == R * C - 1 - n_zero
    assert np.isnan(got["err2"][nan_g]) and np.isnan(got["sig2"][nan_g])
    assert all(got[k][nan_g] <= clean[k][nan_g] for k in COUNTS)
    was_above = M.reference(name, sf, geo)["q0"][inf_at] > fmt.max
    assert got["above"][inf_g] == clean["above"][inf_g] + (0 if was_above else 1) and np.isinf(got["err2"][inf_g]) and np.isinf(got["sig2"][inf_g])
    assert all(got[k][zero_g] == 0 for k in COUNTS) and np.isnan(got["err2"][zero_g])
    assert got["sig2"][zero_g] == clean["sig2"][zero_g] and n_zero == min(gs, R if axis == 0 else C)
    keep = np.ones(got["err2"].shape, bool)
    keep[nan_g] = keep[inf_g] = keep[zero_g] = False
    for k in GROUP_OUTPUTS:
        assert np.array_equal(got[k][keep].view(np.int64), clean[k][keep].view(np.int64)), k      # every other group keeps its bits


# ----------------------------------------------------------------------------------------------------------- memory contract
@pytest.mark.parametrize("geo,residue", [((200, 64, 0, 64), 0), ((5, 1100, 1, 256), 0)], ids=lambda v: _ids(v) if isinstance(v, tuple) else f"r{v}")
def test_memory_contract(dev, geo, residue):
    """Guard bands around P, s and all six outputs: nothing outside the stated extents changes, the inputs stay as they were,
    every group output is written, and the bins are ADDED to."""
    from learned_quantization_amd import _hip
    lib = _hip.load()
    R, C, axis, gs = geo
    name, sf = "fp4_e2m1", "e8m0"
    P, s = M.case(name, sf, geo)
    a = Arena(dev)
    a.add("P", "in", data=P, residue=residue, row_bytes=C * 4)
    a.add("s", "in", data=s, residue=4)
    for out, width, res in (("below", 4, 4), ("above", 4, 12), ("flushed", 4, 8), ("err2", 8, 8), ("sig2", 8, 0)):
        a.add(out, "out", nbytes=s.size * width, residue=res)
    a.add("hist", "inout", data=np.full(16, 7, np.uint32), residue=4)
    a.build()
    _hip.check(lib.lq_mx_stats(a.ptr("P"), a.ptr("s"), FORMATS[name].id, 0, a.ptr("below"), a.ptr("above"), a.ptr("flushed"), a.ptr("err2"),
                               a.ptr("sig2"), a.ptr("hist"), R, C, axis, gs, _hip.stream_ptr(dev)), "lq_mx_stats")
    torch.cuda.synchronize(dev)
    a.check(f"{geo} residue {residue}")
    got = {k: a.numpy(k, np.uint32).astype(np.int64).reshape(s.shape) for k in COUNTS}
    got.update(err2=a.numpy("err2", np.float64).reshape(s.shape), sig2=a.numpy("sig2", np.float64).reshape(s.shape),
               hist=a.numpy("hist", np.uint32).astype(np.int64) - 7)
    _check(got, M.reference(name, sf, geo), f"{geo} in the arena, residue {residue}")


# ---------------------------------------------------------------------------------------------------------------- capturable
def test_capture_and_replay(dev):
    geo = (200, 64, 0, 64)
    R, C, axis, gs = geo
    name, sf = "fp6_e3m2", "fp32"
    P, s = M.case(name, sf, geo)
    p, sd = _t(P, dev), _t(s, dev)
    eager = _stats(dev, p, sd, name, sf, axis, gs)
    o = _buffers(dev, tuple(s.shape), FORMATS[name].bits)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(dev, p, sd, name, sf, axis, gs, o)
    for _ in range(2):
        for k in COUNTS:
            o[k].fill_(0x7F7F7F7F)
        o["err2"].fill_(-7.0)
        o["sig2"].fill_(-7.0)
        o["hist"].zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        assert _same_bits(_host(o), eager)
    _check(eager, M.reference(name, sf, geo), f"{name} {sf} {geo} eager")


# ---------------------------------------------------------------------------------------------------------- layers and drivers
def _model(dev):
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    return lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format="fp4_e2m1", scale_init="mx")


def _perturb(model):
    from learned_quantization_amd import export
    with torch.no_grad():                                    # off the initial state: the biases start as zeros
        for _, param, _ in export.quantized_tensors(model):
            param.mul_(1.0 + 0.5 * torch.rand_like(param)).add_(0.001 * torch.randn_like(param))


def test_mx_quant_stats_equals_the_op_by_hand(dev):
    import learned_quantization_amd as lq
    from learned_quantization_amd import export, ops
    model = _model(dev)
    _perturb(model)
    stats = lq.mx_quant_stats(model)
    tensors = export.quantized_tensors(model)
    assert list(stats) == [name for name, _, _ in tensors] and len(stats) == 4 and lq.quant_stats(model) == {}
    lossy = False
    for name, param, nested in tensors:
        rec = ops.mx_stats(param.data, nested.scale.data, "fp4_e2m1", nested.group_size, "e8m0")
        assert isinstance(rec, ops.MxStats) and rec.hist.numel() == 16 and rec.hist.dtype == rec.flushed.dtype == torch.int32
        assert rec.below.shape == rec.flushed.shape == rec.err2.shape == nested.scale.shape and rec.err2.dtype == torch.float64
        by_hand = ops.summarize_mx_stats(rec, param.numel(), element_format="fp4_e2m1")
        assert by_hand == stats[name] == ops.summarize_mx_stats(nested.mx_stats(param), param.numel(), element_format="fp4_e2m1"), name
        assert int(rec.hist.sum()) == param.numel()
        for k in ("sat_low", "sat_high", "flushed", "zero", "subnormal"):
            assert 0 <= by_hand[k] <= 1, (name, k)
        assert by_hand["flushed"] <= by_hand["zero"] and np.isfinite(by_hand["sqnr_db"]) and by_hand["worst_group_sqnr_db"] <= by_hand["sqnr_db"]
        assert 1 <= by_hand["used_codes"] <= 16 and 0 <= by_hand["entropy_bits"] <= 4.0
        assert nested.mx_stats(param, want_hist=False).hist is None
        lossy |= by_hand["flushed"] > 0
    assert lossy
    assert lq.mx_quant_stats(lq.build_model("mnist", mode="ste", value=0.0, seed=3, bits=4, group_size=32, device=dev)) == {}


def _blocks(path):
    lines = open(path).read().splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith("Epoch ")]
    return [lines[a + 1:b] for a, b in zip(heads, heads[1:] + [len(lines)])], [lines[i] for i in heads]


def test_tracking_callback_files(dev, tmp_path):
    import learned_quantization_amd as lq
    from learned_quantization_amd import ops
    model = _model(dev)
    _perturb(model)
    layer = lq.custom_layers_of(model)[0]
    cb = lq.MxQuantTrackingCallback(layer, str(tmp_path))
    cb.on_train_begin()
    first = cb.on_epoch_end(0)
    cb.on_epoch_end(1)
    cb.on_train_end()
    groups = layer.nested_q_w_layer.scale.numel()
    files = cb.epoch_files()
    assert len(files) == 18 and len(set(files)) == 18
    for f in files:
        blocks, heads = _blocks(f)
        assert heads == ["Epoch 0", "Epoch 1"], f
        base = os.path.basename(f)
        per_tensor = base.startswith(("SQNR_dB_tensor_", "Used_codes_", "Code_entropy_bits_"))
        want = 1 if per_tensor or "Bias" in base else groups
        assert [len(b) for b in blocks] == [want, want], (f, [len(b) for b in blocks], want)
        assert all(np.isfinite(float(v)) for b in blocks for v in b), f
        if base.startswith("Scale_exponent_"):
            assert all(float(v) == round(float(v)) for b in blocks for v in b), f          # E8M0: whole exponents
        if base.startswith(("Sat_low_", "Sat_high_", "Flushed_")):
            assert all(0 <= float(v) <= 1 for b in blocks for v in b), f
    table = ops.mx_decode_table("fp4_e2m1")
    for d, prefix in (("on_train_begin", "Unique_initial_quantized_"), ("on_train_end", "Unique_quantized_")):
        names = sorted(os.listdir(os.path.join(str(tmp_path), d)))
        assert len(names) == 2 and all(n.startswith(prefix) for n in names), names
        for n, numel in zip(names, (layer.b.numel(), layer.W.numel())):      # "Bias..." sorts before "Weights..."
            rows = [l.split(", ") for l in open(os.path.join(str(tmp_path), d, n)).read().splitlines()]
            assert 1 <= len(rows) <= 16 and sum(int(c) for _, c in rows) == numel
            values = [v for v, _ in rows]
            codes = [next(c for c in range(16) if str(table[c]) == v) for v in values]      # "-0.0" is code 8, "0.0" code 0
            assert codes == sorted(codes) and len(set(codes)) == len(codes), values          # code order
    assert cb.stats() == first and set(first) == {"kernel", "bias"}
    assert first["kernel"] == lq.mx_quant_stats(model)[layer.name + "/W"]


def test_experiment_driver_logs_mx_layers(dev, tmp_path):
    res = subprocess.run([sys.executable, "-m", "learned_quantization_amd.experiment", "--seed", "42", "--epochs", "2", "--steps-per-epoch", "3",
                          "--batch", "16", "--log-root", str(tmp_path), "--config", "mnist", "--orientation", "scalar", "--training",
                          "from_scratch", "--scale-gradient", "ste", "--element-format", "fp4_e2m1", "--scale-init", "cover"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["element_format"] == "fp4_e2m1" and out["group_size"] == 32 and "first_layer_unique_integers" not in out
    assert "first_layer_clip_low" not in out
    for key in ("first_layer_sqnr_db", "first_layer_sat_low", "first_layer_sat_high", "first_layer_flushed"):
        assert isinstance(out[key], float), key
    assert all(0 <= out[k] <= 1 for k in ("first_layer_sat_low", "first_layer_sat_high", "first_layer_flushed"))
    d = out["log_dir"]
    epoch = os.listdir(os.path.join(d, "on_epoch_end"))
    for prefix in ("Scale_exponent_Weights", "Sat_low_Weights", "Sat_high_Weights", "Flushed_Weights", "SQNR_dB_Weights",
                   "SQNR_dB_tensor_Weights", "Used_codes_Weights", "Code_entropy_bits_Weights", "Weights_", "Flushed_Bias", "SQNR_dB_Bias", "Bias_"):
        assert any(n.startswith(prefix) for n in epoch), (prefix, epoch)
    blocks, heads = _blocks(os.path.join(d, "on_epoch_end", next(n for n in epoch if n.startswith("SQNR_dB_tensor_Weights"))))
    assert heads == ["Epoch 0", "Epoch 1"] and [len(b) for b in blocks] == [1, 1]
    assert len(os.listdir(os.path.join(d, "on_train_begin"))) == 4 and len(os.listdir(os.path.join(d, "on_train_end"))) == 4      # two layers, kernel and bias


def test_train_driver_mx_stats_flag(dev, capsys):
    from learned_quantization_amd import train
    train.main(["--config", "mnist", "--mode", "ste", "--element-format", "fp4_e2m1", "--scale-init", "cover", "--batch", "32",
                "--steps", "2", "--warmup", "1", "--mx-stats"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(line["mx_stats"]) == 4 and all(np.isfinite(v["sqnr_db"]) and v["used_codes"] >= 1 for v in line["mx_stats"].values())
    train.main(["--config", "mnist", "--mode", "ste", "--element-format", "fp4_e2m1", "--scale-init", "cover", "--batch", "32",
                "--steps", "1", "--warmup", "0"])
    assert "mx_stats" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
