"""GPU tests of the lossless packed export (lq_q_pack / lq_q_unpack, export.save_packed_parameters / load_packed_parameters).

The pack words are compared bit for bit with a NumPy packer applied to K1's own integers (quantized_integers - qmin);
unpack must give back those integers exactly, K1's `out` bit for bit and a float that floors back to q.  Then whole
models go through save -> fresh model -> load, in both kernel storages, and the experiment driver writes the container."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import export, ops
from learned_quantization_amd.train import Trainer, synthetic_batch

from test_pack_cpu import np_pack

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BENCH_SHAPE = (256, 3, 224, 224)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def np_pack_fast(codes: np.ndarray, bits: int) -> np.ndarray:
    """The same stream as test_pack_cpu.np_pack, by word arithmetic (the bit-matrix form does not fit 38 M elements): code i
    adds its low part to word (i*bits)//32 and, when it crosses the boundary, its high part to the next word -- the parts
    of different codes never share a bit, so OR is a sum (exact in float64 below 2^53)."""
    c = np.asarray(codes, dtype=np.uint64).reshape(-1)
    n = c.size
    nw = (n * bits + 31) // 32
    if bits == 0:
        return np.zeros(0, dtype=np.uint32)
    b = np.arange(n, dtype=np.uint64) * np.uint64(bits)
    w = (b >> np.uint64(5)).astype(np.int64)
    sh = b & np.uint64(31)
    lo = (c << sh) & np.uint64(0xFFFFFFFF)
    hi = c >> (np.uint64(32) - sh)                       # sh = 0: shift by 32 of a < 2^32 value is 0
    hi[sh == 0] = 0
    words = np.bincount(w, weights=lo.astype(np.float64), minlength=nw + 1)
    words += np.bincount(w + 1, weights=hi.astype(np.float64), minlength=nw + 1)
    return words[:nw].astype(np.uint64).astype(np.uint32)


def _bitwise_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_round_trip(P: torch.Tensor, s: torch.Tensor, expect_bits=None):
    """Pack against the NumPy packer, then unpack: q exact, out = K1's out bit for bit (P != -0), p_restore floors to q."""
    q = ops.quantized_integers(P, s, torch.int32)
    qn = q.cpu().numpy().astype(np.int64)
    words, qmin, bits = ops.q_pack(P, s)
    assert qmin == int(qn.min()) and bits == int(qn.max() - qn.min()).bit_length()
    if expect_bits is not None:
        assert bits == expect_bits
    ref = (np_pack if P.numel() <= 1 << 20 else np_pack_fast)((qn - qmin).reshape(-1), bits)
    got = words.cpu().numpy().view(np.uint32)
    assert got.shape == ref.shape and np.array_equal(got, ref), "pack words differ from the NumPy packer"
    out, qu, pr = ops.q_unpack(words, qmin, bits, s, P.shape)
    assert torch.equal(qu, q.contiguous()), "unpacked q differs from quantized_integers"
    out_k1 = ops.fq_forward(P, s).contiguous()
    keep = ~((P == 0) & torch.signbit(P)).contiguous()
    assert _bitwise_equal(out[keep], out_k1[keep]), "unpacked out differs from fq_forward's out"
    assert torch.equal(out[~keep], torch.zeros_like(out[~keep])) and not torch.signbit(out[~keep]).any()
    assert torch.equal(ops.quantized_integers(pr, s, torch.int32), q.contiguous()), "p_restore does not floor back to q"
    return words, qmin, bits


# ------------------------------------------------------------------ kernels
def _width_case(bits: int, dev, n: int = 12289):
    rng = np.random.default_rng(100 + bits)
    if bits <= 20:
        qmin = -(1 << (bits - 1))
        qmax = qmin + (1 << bits) - 1
        q = rng.integers(qmin, qmax + 1, size=n).astype(np.float64)
        q[5], q[n - 7] = qmin, qmax
        u = rng.uniform(0.05, 0.95, size=n)
        s = np.float32(0.0123)
        P = ((q + u) * np.float64(s)).astype(np.float32)
    else:                                                    # float-representable integers inside int32, s a power of two
        qmin = -(1 << min(bits - 1, 30))
        qmax = (1 << (bits - 1)) - (1 << max(bits - 25, 0)) if bits < 32 else 2147483392
        q = np.floor(rng.uniform(qmin, qmax, size=n).astype(np.float32)).astype(np.float64)
        q[5], q[n - 7] = qmin, qmax
        s = np.float32(0.5)
        P = (q.astype(np.float32) * s).astype(np.float32)    # exact: P/s = q
    return torch.tensor(P, device=dev), torch.tensor([s], device=dev)


@pytest.mark.parametrize("bits", list(range(1, 33)))
def test_pack_matches_numpy_packer_every_width(dev, bits):
    P, s = _width_case(bits, dev)
    check_round_trip(P, s, expect_bits=bits)


def test_pack_zero_width_writes_no_words(dev):
    P = torch.full((1000,), 3.3, device=dev)
    s = torch.tensor([1.0], device=dev)
    words, qmin, bits = check_round_trip(P, s, expect_bits=0)
    assert words.numel() == 0 and qmin == 3


@pytest.mark.parametrize("kind,orientation", [(k, o) for k in ("dense", "conv_hwio", "conv_oihw")
                                              for o in ("rowwise", "columnwise", "channelwise", "scalar")
                                              if not (k == "dense" and o == "channelwise")])   # axis 2: conv kernels only
def test_pack_every_orientation_and_storage(dev, orientation, kind):
    g = torch.Generator(device="cpu").manual_seed(7)
    shape = (784, 128) if kind == "dense" else (3, 3, 64, 128)
    P = (torch.randn(shape, generator=g) * 0.05).to(dev)
    sshape = lq.scale_shape(shape, orientation)
    s = (torch.rand(sshape, generator=g) * 9e-3 + 1e-3).to(dev)
    if kind == "conv_oihw":
        P = P.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)      # layers.py kernel_storage="oihw"
        assert not P.is_contiguous()
    words, _, _ = check_round_trip(P, s)
    if kind == "conv_oihw":                                              # the stream speaks about the logical order
        assert torch.equal(words, ops.q_pack(P.contiguous(), s)[0])


@pytest.mark.parametrize("n", [10, 1, 33, 2049])
def test_pack_bias_and_odd_sizes(dev, n):
    g = torch.Generator(device="cpu").manual_seed(n)
    P = (torch.randn(n, generator=g) * 0.05).to(dev)
    check_round_trip(P, torch.tensor([3e-3], device=dev))


def test_pack_bench_tensor_per_channel_and_per_tensor(dev):
    g = torch.Generator(device=dev).manual_seed(42)
    x = torch.rand(BENCH_SHAPE, device=dev, generator=g) * 255.0
    check_round_trip(x, torch.tensor([0.5, 1.0, 2.0], device=dev).view(1, 3, 1, 1), expect_bits=9)
    check_round_trip(x, torch.tensor([1.0], device=dev), expect_bits=8)


def test_pack_bench_weight_like_tensor(dev):
    g = torch.Generator(device=dev).manual_seed(43)
    x = torch.randn(BENCH_SHAPE, device=dev, generator=g) * 0.05
    _, _, bits = check_round_trip(x, torch.tensor([1.1920929e-05], device=dev))
    assert 15 <= bits <= 17


def test_restore_is_exact_up_to_2_pow_22(dev):
    rng = np.random.default_rng(5)
    lim = (1 << 22) - 1
    q = rng.integers(-lim, lim + 1, size=(37, 129)).astype(np.float64)
    q[0, 0], q[-1, -1] = -lim, lim
    s = rng.uniform(1e-4, 3.0, size=(37, 1)).astype(np.float32)
    P = ((q + 0.5) * s.astype(np.float64)).astype(np.float32)
    Pt, st = torch.tensor(P, device=dev), torch.tensor(s, device=dev)
    check_round_trip(Pt, st)
    words, qmin, bits = ops.q_pack(Pt, st)
    _, qu, pr = ops.q_unpack(words, qmin, bits, st, Pt.shape, want_out=False)
    assert int(qu.abs().max()) == lim
    assert torch.equal(ops.quantized_integers(pr, st, torch.int32), qu)


def test_thesis_shaped_range_takes_five_bits(dev):
    """MNIST's trained range [-12, 11] (thesis chapter4.tex:123-127) is 5 bits: ceil(n*5/32) words."""
    n = 784 * 128
    q = np.tile(np.arange(-12, 12, dtype=np.float64), n // 24 + 1)[:n]
    P = torch.tensor(((q + 0.5) * 0.01).astype(np.float32).reshape(784, 128), device=dev)
    words, qmin, bits = check_round_trip(P, torch.tensor([0.01], device=dev), expect_bits=5)
    assert qmin == -12 and words.numel() * 4 == (n * 5 + 31) // 32 * 4


# ------------------------------------------------------------------ refusal
def _mnist(dev):
    lq.reset_layer_names()
    return lq.build_model("mnist", mode="nq", value=1e-10, seed=42, orientation="rowwise", device=dev)


@pytest.mark.parametrize("poison", ["nan", "inf", "huge", "all_nan"])
def test_save_refuses_integers_it_cannot_store(dev, tmp_path, poison):
    m = _mnist(dev)
    with torch.no_grad():
        W = m.dense_2.W
        s = float(m.dense_2.nested_q_w_layer.scale.max())
        if poison == "nan":
            W[3, 4] = float("nan")
        elif poison == "inf":
            W[3, 4] = float("-inf")
        elif poison == "huge":
            W[3, 4] = 3.0e9 * s                                 # |q| >= 2^31
        else:
            W.fill_(float("nan"))
    with pytest.raises(ValueError, match=m.dense_2.name + "/W"):
        lq.save_packed_parameters(m, str(tmp_path))
    assert not [f for f in os.listdir(tmp_path) if "weights_packed" in f or f == "packed_sizes.log"], os.listdir(tmp_path)


# ------------------------------------------------------------------ whole models
def _container_arrays(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _same_containers(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _fresh(config, mode, value, orientation, storage, dev):
    lq.reset_layer_names()
    return lq.build_model(config, kernel_storage=storage, mode=mode, value=value, seed=7, orientation=orientation, device=dev)


@pytest.mark.parametrize("storage", ["oihw", "hwio"])
@pytest.mark.parametrize("config,mode,loss,value,orientation,batch", [
    ("mnist", "nq", None, 1e-10, "rowwise", 32),
    ("cifar", "nq", None, 1e-11, "channelwise", 16),
    ("cifar", "cl", "maxbin", 1e-7, "rowwise", 16),
    ("imagenette", "nq", None, 1e-11, "channelwise", 4),
])
def test_model_round_trip(dev, tmp_path, config, mode, loss, value, orientation, batch, storage):
    tr = Trainer(config, mode, value, orientation, loss, seed=42, device=dev, log_dir=str(tmp_path / "logs"),
                 kernel_storage=storage)
    g = torch.Generator(device=dev).manual_seed(3)
    for _ in range(3):
        x, y = synthetic_batch(config, batch, dev, g)
        tr.step(x, y)
    torch.cuda.synchronize()
    model = tr.model
    info = lq.save_packed_parameters(model, str(tmp_path / "a"))
    assert info["packed_mb"] > 0 and info["zip_mb"] > 0 and 0 < info["bits_per_weight"] <= 32
    for f in export.PACKED_FILES:
        assert os.path.exists(tmp_path / "a" / f), f
    log = open(tmp_path / "a" / "packed_sizes.log").read().splitlines()
    assert log[0].startswith("Packed weights size: ") and log[0].endswith(" MB")
    assert log[1].startswith("Compressed packed weights size: ") and log[2].startswith("Bits per quantised weight: ")

    fresh = _fresh(config, mode, value, orientation, storage, dev)
    manifest = lq.load_packed_parameters(fresh, str(tmp_path / "a"))
    assert manifest["format"] == "lq-packed" and manifest["version"] == 1
    for (name, p0, n0), (_, p1, n1) in zip(export.quantized_tensors(model), export.quantized_tensors(fresh)):
        assert p1.stride() == p0.stride(), name                          # restored into the parameter's own storage
        assert torch.equal(n1.scale, n0.scale), name
        assert torch.equal(ops.fq_forward(p1.data, n1.scale.data), ops.fq_forward(p0.data, n0.scale.data)), name
    sd0, sd1 = model.state_dict(), fresh.state_dict()
    for key in manifest["state"]:
        a, b = sd0[key], sd1[key]
        assert a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), key
    model.eval()
    fresh.eval()
    with torch.no_grad():
        x, _ = synthetic_batch(config, 4, dev, torch.Generator(device=dev).manual_seed(11))
        torch.testing.assert_close(fresh(x), model(x), rtol=1e-5, atol=1e-6)
    lq.save_packed_parameters(fresh, str(tmp_path / "b"))
    a, b = _container_arrays(tmp_path / "a" / "weights_packed.npz"), _container_arrays(tmp_path / "b" / "weights_packed.npz")
    _same_containers(a, b)


def test_container_does_not_depend_on_kernel_storage(dev, tmp_path):
    paths, contiguous = [], []
    for storage in ("oihw", "hwio"):
        m = _fresh("cifar", "nq", 1e-11, "columnwise", storage, dev)
        with torch.no_grad():
            for _, p, nested in export.quantized_tensors(m):
                nested.scale.mul_(37.0)                                   # a few hundred levels, not the initial 100 eps
        contiguous.append(all(p.is_contiguous() for _, p, _ in export.quantized_tensors(m)))
        lq.save_packed_parameters(m, str(tmp_path / storage))
        paths.append(tmp_path / storage / "weights_packed.npz")
    assert contiguous == [False, True]
    _same_containers(_container_arrays(paths[0]), _container_arrays(paths[1]))


def test_lossless_where_the_int8_file_wraps(dev, tmp_path):
    """At the initial scale (1.19e-5) |q| ~ 10^4: weights.npy wraps, the packed container does not."""
    m = _mnist(dev)
    lq.save_compress_parameters(m, str(tmp_path))
    lq.save_packed_parameters(m, str(tmp_path))
    int8 = np.load(tmp_path / "weights.npy", allow_pickle=True).item()
    fresh = _mnist(dev)
    lq.load_packed_parameters(fresh, str(tmp_path))
    for (name, p0, n0), (_, p1, n1) in zip(export.quantized_tensors(m), export.quantized_tensors(fresh)):
        q0 = ops.quantized_integers(p0.data, n0.scale.data, torch.int32).cpu().numpy()
        q1 = ops.quantized_integers(p1.data, n1.scale.data, torch.int32).cpu().numpy()
        assert np.array_equal(q1, q0), name
        assert np.array_equal(int8[name], q0.astype(np.int8))                       # the reference file: the wrap of q
        if name.endswith("/W"):
            assert not np.array_equal(int8[name].astype(np.int32), q0) and np.abs(q0).max() > 127


def test_experiment_driver_writes_the_packed_export(dev, tmp_path):
    base = [sys.executable, "-m", "learned_quantization_amd.experiment", "--seed", "42", "--epochs", "1",
            "--steps-per-epoch", "2", "--batch", "16", "--config", "mnist", "--orientation", "rowwise",
            "--training", "post_training", "--value", "1e-10",
            "--baseline-weights", os.path.join(ROOT, "tests", "golden", "mnist_baseline_weights.npz")]
    outs = {}
    for flag in (True, False):
        cmd = base + ["--log-root", str(tmp_path / str(flag))] + (["--export-packed"] if flag else [])
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        outs[flag] = json.loads(res.stdout.strip().splitlines()[-1])
    d = outs[True]["log_dir"]
    for f in export.PACKED_FILES + ("weights.npy", "weights.zip", "file_sizes.log", "scales.npz"):
        assert os.path.exists(os.path.join(d, f)), f
    assert set(outs[True]["packed"]) == {"packed_mb", "zip_mb", "bits_per_weight"}
    assert "packed" not in outs[False]
    assert not any(os.path.exists(os.path.join(outs[False]["log_dir"], f)) for f in export.PACKED_FILES)
    fresh = _mnist(dev)
    lq.load_packed_parameters(fresh, d)
    int8 = np.load(os.path.join(d, "weights.npy"), allow_pickle=True).item()
    for name, p, nested in export.quantized_tensors(fresh):                          # the run's q, through its int8 wrap
        assert np.array_equal(ops.quantized_integers(p.data, nested.scale.data, torch.int8).cpu().numpy(), int8[name]), name
