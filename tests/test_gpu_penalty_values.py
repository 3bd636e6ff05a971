"""GPU tests of the penalty VALUES of the multi-tensor batch (lq_batch_penalty_values, lq_batch_penalty_grads_values), the
device-side loss log (lq_loss_log_append, LossLog) and ``Trainer(loss_values=True)``."""
import glob
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import lq_oracle as O
from oracle import lq_oracle_f64 as O64

from _bounds import assert_within_terms

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RTOL = 1e-5              # the project's float32 tolerance (BASELINE.json north_star)
KINDS = ["maxbin", "difference", "inverse"]
ORIENTS = ["rowwise", "columnwise", "channelwise", "scalar"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, config, orient, storage, scales, mode="cl", value=0.37):
    """Layers built by the project's layer classes (bias scale "scalar"); ``scales``: "init" leaves SCALE_INIT, "random" draws
    every scale from [1e-3, 1]."""
    import learned_quantization_amd as lq
    lq.reset_layer_names()
    m = lq.build_model(config, mode=mode, value=value, seed=3, orientation=orient, device=dev, kernel_storage=storage)
    if scales == "random":
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for s in lq.scale_parameters(m):
                s.copy_((torch.rand(s.shape, generator=g) * (1.0 - 1e-3) + 1e-3).to(dev))
    return m


def _np_layers(layers):
    from learned_quantization_amd.losses import _kernel_and_scales       # dense layers name their kernel W (MNIST CL-F variant)
    return [tuple(t.detach().cpu().numpy() for t in _kernel_and_scales(l)) for l in layers]


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def _check_values(dev, config, orient, storage, scales, kind, tmp_path):
    import learned_quantization_amd as lq
    m = _model(dev, config, orient, storage, scales)
    layers = lq.custom_layers_of(m)
    batch = lq.FakeQuantBatch(m)
    terms, pen = batch.penalty_values(kind)
    terms, pen = terms.cpu().numpy().copy(), float(pen)
    # --- the float64 oracle, 1e-5 * sum|terms| (every term is >= 0: the yardstick is the value itself)
    npl = _np_layers(layers)
    l64 = [(k, ks, O.group_descriptor(k.shape, ks.shape), b, bs, O.group_descriptor(b.shape, bs.shape)) for k, ks, b, bs in npl]
    val64 = O64.penalty(kind, l64)
    t64 = []
    for k, ks, dk, b, bs, db in l64:
        if kind == "maxbin":
            t64 += [O64.maxbin_term(k, ks, *dk), O64.maxbin_term(b, bs, *db)]
        elif kind == "difference":
            t64 += [O64.difference_term(k, ks, *dk), O64.difference_term(b, bs, *db)]
        else:
            t64 += [O64.inverse_term(ks), O64.inverse_term(bs)]
    assert len(t64) == len(batch.entries) == terms.size
    what = f"{kind} {config} {orient} {storage} {scales}"
    assert_within_terms(pen, val64, abs(val64), f"{what}: penalty vs float64 oracle")
    assert_within_terms(terms, np.array(t64), None, f"{what}: terms vs float64 oracle")
    # --- the float32 restatement of the reference
    f32 = float({"maxbin": O.maxbin_penalty, "difference": O.difference_penalty, "inverse": O.inverse_penalty}[kind](npl))
    assert pen == pytest.approx(f32, rel=RTOL), f"{what}: penalty {pen!r} vs float32 oracle {f32!r} (rel {_rel(pen, f32):.3e})"
    # --- the reference's ORDER and pairing (CL-F:102-116), replayed in numpy float32 on the device's own terms: per layer
    # t_k * dim_k + t_b * dim_b, running sum over the layers, / normalizer -- every operation rounded on its own.  Exact:
    # a flat sum, a fused multiply-add or a lost kernel/bias pairing differs in the last bits
    f = np.float32
    total, normalizer = None, 0.0
    for li in range(len(layers)):
        tk, tb = f(terms[2 * li]), f(terms[2 * li + 1])
        nk, nb = float(npl[li][0].size), float(npl[li][2].size)
        layer_penalty = f(f(tk * f(nk)) + f(tb * f(nb)))
        total = layer_penalty if total is None else f(total + layer_penalty)
        normalizer += nk + nb
    replay = f(total / f(normalizer))
    assert np.float32(pen) == replay, f"{what}: penalty {pen!r} is not the float32 replay {float(replay)!r} of the reference's order"
    # --- MaxBin / Inverse terms are the single-tensor entry points' bits (one summation code)
    if kind != "difference":
        with torch.no_grad():
            for i, e in enumerate(batch.entries):
                single = lq.ops.maxbin_term(e.param, e.nested.scale) if kind == "maxbin" else lq.ops.inverse_term(e.nested.scale)
                assert float(single) == float(terms[i]), f"{what}: term {i} {terms[i]!r} != single-tensor op {float(single)!r}"
    # --- the per-tensor path (same partials merged in different block shapes: 1e-6)
    cls = {"maxbin": lq.SCCEMaxBin, "difference": lq.SCCEDifference, "inverse": lq.SCCEInverse}[kind]
    with torch.no_grad():
        per_tensor = float(getattr(cls(layers, 0.37, str(tmp_path)), f"compute_{kind}_penalty")())
    d_pt = _rel(pen, per_tensor)
    # --- gradients untouched, and the value of the gradient entry point
    g = torch.Generator(device=dev).manual_seed(3)
    seeds = [(torch.randn(e.param.shape, device=dev, generator=g) * 1e-3, torch.randn(e.ds.shape, device=dev, generator=g) * 1e-3)
             for e in batch.entries]
    d_gv = 0.0
    for accumulate in (False, True):
        got = []
        for values in (False, True):
            for e, (sp, sd) in zip(batch.entries, seeds):
                e.param.grad = torch.empty_like(e.param.data).copy_(sp)
                e.ds.copy_(sd)
            ret = batch.inject_penalty_grads(kind, 0.37, accumulate_ds=accumulate, values=values)
            assert (ret is None) == (not values)
            got.append(([e.param.grad.clone() for e in batch.entries], [e.nested.scale.grad.clone() for e in batch.entries],
                        None if ret is None else float(ret)))
        for i, e in enumerate(batch.entries):
            assert torch.equal(got[0][0][i], got[1][0][i]), f"{what} accumulate={accumulate}: P.grad of tensor {i} changed"
            assert torch.equal(got[0][1][i], got[1][1][i]), f"{what} accumulate={accumulate}: ds of tensor {i} changed"
        d_gv = max(d_gv, _rel(got[1][2], pen))
    assert d_pt <= 1e-6 and d_gv <= 1e-6, (f"{what}: penalty_values {pen!r}, per-tensor path {per_tensor!r} (rel {d_pt:.3e}), "
                                           f"grads_values vs values rel {d_gv:.3e}")


@pytest.mark.parametrize("scales", ["init", "random"])
@pytest.mark.parametrize("storage", ["oihw", "hwio"])
@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("config", ["mnist", "cifar"])
def test_penalty_values_small_models(dev, config, kind, orient, storage, scales, tmp_path):
    _check_values(dev, config, orient, storage, scales, kind, tmp_path)


@pytest.mark.parametrize("orient", ["rowwise", "channelwise"])
@pytest.mark.parametrize("kind", KINDS)
def test_penalty_values_resnet18_like(dev, kind, orient, tmp_path):
    """The ResNet-18-like model: its tensors reach every traversal form of the batch."""
    _check_values(dev, "imagenette", orient, "oihw", "random", kind, tmp_path)


def test_penalty_values_are_run_to_run_bit_stable(dev):
    import learned_quantization_amd as lq
    m = _model(dev, "cifar", "channelwise", "oihw", "random")
    batch = lq.FakeQuantBatch(m)
    for kind in KINDS:
        first = None
        for _ in range(3):
            terms, pen = batch.penalty_values(kind)
            cur = (terms.clone(), pen.clone())
            if first is None:
                first = cur
            assert torch.equal(first[0], cur[0]) and torch.equal(first[1], cur[1]), kind


# ------------------------------------------------------------------ the device-side log
def test_loss_log_append_rows_cursor_and_capacity(dev, tmp_path):
    import learned_quantization_amd as lq
    from learned_quantization_amd import _hip
    lib = _hip.load()
    cap, guard = 2, 6
    buf = torch.full((3 * cap + guard,), -7.0, device=dev)           # guard words after the rows
    cursor = torch.zeros(2, dtype=torch.int64, device=dev)
    last = torch.zeros(3, device=dev)
    rate = 0.3
    want = []
    for i in range(5):
        scce = torch.tensor(1.5 + i, device=dev)
        pen = torch.tensor(0.7 * (i + 1), device=dev)
        _hip.check(lib.lq_loss_log_append(scce.data_ptr(), pen.data_ptr(), rate, buf.data_ptr(), cap, cursor.data_ptr(), last.data_ptr(),
                                          _hip.stream_ptr(dev)), "lq_loss_log_append")
        rp = np.float32(rate) * np.float32(0.7 * (i + 1))
        want.append([np.float32(np.float32(1.5 + i) + rp), np.float32(1.5 + i), rp])
        assert last.cpu().numpy().tolist() == [float(v) for v in want[-1]]       # the latest row, logged or dropped
    assert cursor.tolist() == [2, 3]
    got = buf.cpu().numpy()
    assert got[:6].tolist() == [float(v) for r in want[:2] for v in r]
    assert (got[6:] == -7.0).all(), "written past the end of rows_dev"
    # LossLog: the same through the class, flush writes the files and resets the cursor
    obj = lq.SCCEMaxBin([], rate, str(tmp_path))
    log = lq.LossLog(obj, capacity=2, device=dev)
    for i in range(5):
        log.append(torch.tensor(1.5 + i, device=dev), torch.tensor(0.7 * (i + 1), device=dev))
    with pytest.warns(RuntimeWarning, match="3 rows were dropped"):
        assert log.flush() == (2, 3)
    assert log.cursor.tolist() == [0, 0]
    d = os.path.join(str(tmp_path), "custom_losses")
    for col, name in enumerate(("total_loss.log", "scce_loss.log", "maxbin_loss.log")):
        assert open(os.path.join(d, name)).read() == "".join(f"{float(r[col])}\n" for r in want[:2])


# ------------------------------------------------------------------ the trainer
def _bound(total, rp):
    """Two independent float32 evaluations of the penalty, each within 1e-5 of the float64 value, plus mean(SCCE_i + c)
    against mean(SCCE_i) + c."""
    return 2e-5 * abs(rp) + 4 * 2.0 ** -23 * abs(total)


def _run(dev, tmp_path, mode, tag, steps=3, **kw):
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    value = (2e-4, 0.05) if mode == "nqcl" else 0.05
    tr = Trainer("mnist", mode, value, "rowwise", "maxbin", device=dev, log_dir=os.path.join(str(tmp_path), tag), **kw)
    tr.model.eval()
    losses, terms = [], []
    for _ in range(steps):
        losses.append(tr.step(x, y).detach().clone())
        terms.append(None if tr.loss_terms is None else tr.loss_terms.clone())
    params = [p.detach().clone() for p in tr.model.parameters()]
    return tr, losses, terms, params


@pytest.mark.parametrize("mode", ["cl", "nqcl"])
def test_trainer_loss_values(dev, tmp_path, mode):
    tr0, l0, t0, p0 = _run(dev, tmp_path, mode, "plain", batched=True)
    tr1, l1, t1, p1 = _run(dev, tmp_path, mode, "values", batched=True, loss_values=True)
    # (a) evaluating the penalty changes nothing that is trained
    assert len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
    # (c) the default: no value buffers, no log, the loss is mean(SCCE) as before -- the scce entry of the other run
    assert tr0.loss_terms is None and tr0.loss_log is None and getattr(tr0.batch, "_values", None) is None
    for a, t in zip(l0, t1):
        assert torch.equal(a, t[1])
    for l, t in zip(l1, t1):
        assert torch.equal(l, t[0]) and float(t[0]) == float(np.float32(float(t[1])) + np.float32(float(t[2])))
        assert float(t[2]) > 0.0
    # (b) against the per-tensor path, which differentiates mean(SCCE_i + rate * penalty)
    tr2, l2, t2, _ = _run(dev, tmp_path, mode, "per_tensor", batched=False, loss_values=True)
    tr3, l3, _, p3 = _run(dev, tmp_path, mode, "per_tensor_plain", batched=False)
    for a, b in zip(l2, l3):
        assert torch.equal(a, b)                     # logging does not change the per-tensor objective
    for i, (a, b, t) in enumerate(zip(l1, l2, t1)):
        diff, bound = abs(float(a) - float(b)), _bound(float(a), float(t[2]))
        print(f"{mode} step {i}: batched {float(a)!r} per-tensor {float(b)!r} diff {diff:.3e} bound {bound:.3e}")
    for i, (a, b, t) in enumerate(zip(l1, l2, t1)):
        diff, bound = abs(float(a) - float(b)), _bound(float(a), float(t[2]))
        assert diff <= bound, (mode, i, float(a), float(b), diff, bound)
    # both forms write the same three files, one line per step, without a per-step synchronisation
    assert tr1.flush_loss_log() == (3, 0) and tr2.flush_loss_log() == (3, 0)
    for tag in ("values", "per_tensor"):
        d = os.path.join(str(tmp_path), tag, "custom_losses")
        for name in ("total_loss.log", "scce_loss.log", "maxbin_loss.log"):
            assert len(open(os.path.join(d, name)).read().splitlines()) == 3, (tag, name)
    # evaluate(with_penalty=True) adds rate * penalty of the current parameters
    from learned_quantization_amd.train import synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(1))
    v0, acc0 = tr1.evaluate(x, y)
    v1, acc1 = tr1.evaluate(x, y, with_penalty=True)
    rp = 0.05 * float(tr1.batch.penalty_values("maxbin")[1])
    assert acc0 == acc1 and abs((v1 - v0) - rp) <= _bound(v1, rp) and rp > 0.0


def test_regularisers_are_in_the_returned_total_and_not_in_the_log(dev, tmp_path):
    """Keras adds the regulariser losses outside compute_total_loss (custom_layers.py:327; CL-F:47-71): the log's row is
    {scce + rate * penalty, scce, rate * penalty}, the returned loss has the regularisers on top."""
    import learned_quantization_amd as lq
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    tr = Trainer("mnist", "cl", 0.05, "rowwise", "maxbin", device=dev, log_dir=str(tmp_path), batched=True, loss_values=True)
    for layer in tr.custom_layers:
        layer.regularizer = lq.l2(0.01)
    tr.regularized = list(tr.custom_layers)
    with torch.no_grad():                            # the regularisers of the parameters the step starts from, summed in float64
        reg = sum(float(l.regularizer(w)) for l in tr.custom_layers for w in l._regularized())
    loss = tr.step(x, y)
    t = tr.loss_terms.clone()
    row = tr.loss_log.rows[0].clone()
    assert torch.equal(loss.detach(), t[0])
    assert float(row[0]) == float(np.float32(float(row[1])) + np.float32(float(row[2])))       # no regulariser in the log
    assert torch.equal(row[1:], t[1:])
    extra = float(t[0]) - float(row[0])
    # t[0] = ((scce + r_1) + r_2) + rate * penalty in float32 against row[0] = scce + rate * penalty: four float32 additions
    assert reg > 0.0 and abs(extra - reg) <= 4 * 2.0 ** -23 * abs(float(t[0])), (extra, reg)


def test_trainer_loss_values_needs_a_loss_term(dev, tmp_path):
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="loss term"):
        Trainer("mnist", "nq", 1e-3, "rowwise", None, device=dev, log_dir=str(tmp_path), loss_values=True)


def test_graphed_step_logs_on_the_device(dev, tmp_path):
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    rows = {}
    for tag, graph in (("eager", False), ("graph", True)):
        tr = Trainer("mnist", "cl", 0.05, "rowwise", "maxbin", device=dev, log_dir=os.path.join(str(tmp_path), tag), batched=True,
                     graph=graph, loss_values=True)
        tr.model.eval()
        if graph:
            for _ in range(4):                       # 3 eager warm-up steps inside the first call, then 4 replays
                loss = tr.step_graphed(x, y)
        else:
            for _ in range(7):
                loss = tr.step(x, y)
        torch.cuda.synchronize()
        r = tr.loss_log.rows[:7].clone()
        assert tr.loss_log.cursor.tolist() == [7, 0]
        assert torch.equal(r[-1][0], loss.detach()), "the last row's total is the returned loss (mnist has no regulariser)"
        assert torch.equal(r[:, 0], r[:, 1] + r[:, 2])
        assert tr.flush_loss_log() == (7, 0)
        rows[tag] = r
    assert torch.equal(rows["eager"], rows["graph"]), (rows["eager"], rows["graph"])
    # a log that is too small: rows are counted as dropped, nothing is written past the buffer
    tr = Trainer("mnist", "cl", 0.05, "rowwise", "maxbin", device=dev, log_dir=os.path.join(str(tmp_path), "small"), batched=True,
                 graph=True, loss_values=True, loss_log_capacity=2)
    log = tr.loss_log
    backing = torch.full((3 * 2 + 8,), -7.0, device=dev)
    log.rows = backing[:6].view(2, 3)
    for _ in range(2):                               # 3 warm-up steps + 2 replays = 5 steps
        tr.step_graphed(x, y)
    torch.cuda.synchronize()
    assert (backing[6:] == -7.0).all().item(), "written past the end of the rows"
    assert torch.equal(backing[:6].view(2, 3), rows["graph"][:2])
    with pytest.warns(RuntimeWarning, match="3 rows were dropped"):
        assert tr.flush_loss_log() == (2, 3)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("ddp_mode", ["A", "B"])
def test_data_parallel_returns_the_same_total(dev, tmp_path, ddp_mode):
    """One-rank gloo group on the GPU with force_collectives=True: the exchange really runs."""
    import torch.distributed as dist
    _, ref, ref_terms, ref_params = _run(dev, tmp_path, "nqcl", "single", batched=True, loss_values=True)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        tr, got, terms, params = _run(dev, tmp_path, "nqcl", "dp" + ddp_mode, batched=True, loss_values=True, ddp_mode=ddp_mode,
                                      force_collectives=True)
        assert tr.dp is not None
        for a, b in zip(ref, got):
            assert torch.equal(a, b), (ddp_mode, float(a), float(b))
        for a, b in zip(ref_terms, terms):
            assert torch.equal(a, b)
        assert tr.flush_loss_log() == (3, 0)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ddp_mode", ["A", "B"])
def test_data_parallel_graphed_step_logs_the_eager_rows(dev, tmp_path, ddp_mode):
    """graph(backward) -> eager all-reduce -> graph(update) on the one-rank gloo group: mode A appends the row in the first
    graph, mode B (penalty after the exchange) in the second; either way the rows are the eager single-process ones."""
    import torch.distributed as dist
    from learned_quantization_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch("mnist", 32, dev, torch.Generator(device=dev).manual_seed(0))
    ref = Trainer("mnist", "nqcl", (2e-4, 0.05), "rowwise", "maxbin", device=dev, log_dir=os.path.join(str(tmp_path), "ref"),
                  batched=True, loss_values=True)
    for _ in range(5):
        ref_loss = ref.step(x, y).detach().clone()
    torch.cuda.synchronize()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        tr = Trainer("mnist", "nqcl", (2e-4, 0.05), "rowwise", "maxbin", device=dev, log_dir=os.path.join(str(tmp_path), "dp"),
                     batched=True, loss_values=True, ddp_mode=ddp_mode, force_collectives=True, graph=True)
        for _ in range(2):                           # 3 eager warm-up steps inside the first call, then 2 replays
            loss = tr.step_graphed(x, y)
        torch.cuda.synchronize()
        assert tr.graph is not None and tr.graph_update is not None
        assert tr.loss_log.cursor.tolist() == [5, 0]
        assert torch.equal(tr.loss_log.rows[:5], ref.loss_log.rows[:5]), (tr.loss_log.rows[:5], ref.loss_log.rows[:5])
        assert torch.equal(loss.detach(), ref_loss)
        assert tr.flush_loss_log() == (5, 0)
    finally:
        dist.destroy_process_group()


def test_experiment_loss_values(dev, tmp_path):
    """experiment.py --loss-values: one line per step in the three custom_losses files, val_loss includes rate * penalty."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = {}
    for tag, extra in (("plain", []), ("values", ["--loss-values"])):
        res = subprocess.run([sys.executable, "-m", "learned_quantization_amd.experiment", "--config", "mnist", "--seed", "42",
                              "--orientation", "rowwise", "--training", "from_scratch", "--custom_loss", "maxbin", "--value", "0.05",
                              "--batched", "--epochs", "2", "--steps-per-epoch", "5", "--batch", "32",
                              "--log-root", os.path.join(str(tmp_path), tag)] + extra,
                             capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
        out[tag] = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    d = out["values"]["log_dir"]
    for name in ("total_loss.log", "scce_loss.log", "maxbin_loss.log"):
        lines = open(os.path.join(d, "custom_losses", name)).read().splitlines()
        assert len(lines) == 2 * 5, (name, len(lines))
        assert all(np.isfinite(float(v)) for v in lines)
    total, scce, pen = (np.array([float(v) for v in open(os.path.join(d, "custom_losses", n)).read().splitlines()], np.float32)
                        for n in ("total_loss.log", "scce_loss.log", "maxbin_loss.log"))
    assert np.array_equal(total, scce + pen)
    # the same seeds and the same trained parameters: loss/val_loss.log differs by rate * penalty of the final parameters
    def last_val_loss(tag):
        path = glob.glob(os.path.join(out[tag]["log_dir"], "loss", "val_*loss*.log"))
        assert len(path) == 1, path
        return float(open(path[0]).read().splitlines()[-1])
    v0, v1 = last_val_loss("plain"), last_val_loss("values")
    assert out["plain"]["final"]["val_accuracy"] == out["values"]["final"]["val_accuracy"]
    rp = out["values"]["rate_penalty"]
    diff = v1 - v0
    print(f"val_loss plain {v0!r} values {v1!r} diff {diff!r} rate*penalty of the final parameters {rp!r} bound {_bound(v1, rp):.3e}")
    assert rp > 0.0 and abs(diff - rp) <= _bound(v1, rp), (v0, v1, diff, rp, _bound(v1, rp))
