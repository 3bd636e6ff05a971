"""CPU tests of the lossless packed export: the stream format (a NumPy packer written from the format's definition), the
argument validation of lq_q_pack / lq_q_unpack, and the container checks of export.load_packed_parameters -- everything
that must hold without a device.  The kernels themselves are checked against this packer in test_gpu_pack.py."""
import ctypes
import json

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, export
from learned_quantization_amd.ops import packed_words


# ------------------------------------------------------------------ reference packer (the format, restated in NumPy)
def np_pack(codes: np.ndarray, bits: int) -> np.ndarray:
    """Codes LSB-first: element i at stream bits [i*bits, i*bits + bits), stream bit j = bit (j % 32) of word j // 32,
    ceil(n*bits/32) little-endian uint32 words, pad bits 0."""
    codes = np.asarray(codes, dtype=np.uint64).reshape(-1)
    n = codes.size
    nwords = (n * bits + 31) // 32
    if bits == 0:
        return np.zeros(0, dtype=np.uint32)
    stream = ((codes[:, None] >> np.arange(bits, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    stream = np.concatenate([stream, np.zeros(nwords * 32 - stream.size, dtype=np.uint8)])
    return np.packbits(stream, bitorder="little").view("<u4").astype(np.uint32)


def np_unpack(words: np.ndarray, n: int, bits: int) -> np.ndarray:
    if bits == 0:
        return np.zeros(n, dtype=np.uint64)
    stream = np.unpackbits(np.asarray(words, dtype="<u4").view(np.uint8), bitorder="little")[: n * bits].reshape(n, bits)
    return (stream.astype(np.uint64) << np.arange(bits, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def test_reference_packer_matches_the_format_by_hand():
    # bits 5: codes 1, 2, 3 -> word 0 = 1 | 2 << 5 | 3 << 10
    assert np_pack(np.array([1, 2, 3]), 5).tolist() == [1 | 2 << 5 | 3 << 10]
    # bits 12: the third code straddles the word boundary (stream bits 24..35)
    w = np_pack(np.array([0xABC, 0x123, 0xFED]), 12)
    assert w.tolist() == [0xABC | 0x123 << 12 | (0xFED & 0xFF) << 24, 0xFED >> 8]
    assert np_pack(np.array([0xFFFFFFFF, 7]), 32).tolist() == [0xFFFFFFFF, 7]


@pytest.mark.parametrize("bits", list(range(33)))
def test_reference_packer_round_trips_every_width(bits):
    rng = np.random.default_rng(bits)
    for n in (1, 31, 32, 33, 2047, 2048, 2049, 10 ** 5):
        hi = (1 << bits) - 1
        codes = rng.integers(0, hi + 1, size=n, dtype=np.uint64) if bits else np.zeros(n, dtype=np.uint64)
        codes[0] = hi                                    # the width is really needed
        words = np_pack(codes, bits)
        assert words.dtype == np.uint32 and words.size == (n * bits + 31) // 32 == packed_words(n, bits)
        assert np.array_equal(np_unpack(words, n, bits), codes)
        if bits and (n * bits) % 32:                     # pad bits are zero
            assert int(words[-1]) >> ((n * bits) % 32) == 0


# ------------------------------------------------------------------ C ABI argument validation (no launch)
def _aligned_buffer():
    buf = (ctypes.c_float * 256)()
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_pack_argument_validation_without_gpu():
    """lq_q_pack / lq_q_unpack validate before any launch: NULL, bits > 32, non-positive extents, misalignment, size."""
    lib = _hip.load()
    buf, p = _aligned_buffer()
    assert p % 16 == 0
    assert lib.lq_q_pack(None, p, 0, 8, p, p, 1, 1, 16, None) == -1
    assert b"NULL" in lib.lq_last_error()
    assert lib.lq_q_pack(p, None, 0, 8, p, p, 1, 1, 16, None) == -1
    assert lib.lq_q_pack(p, p, 0, 33, p, p, 1, 1, 16, None) == -1
    assert b"0..32" in lib.lq_last_error()
    assert lib.lq_q_pack(p, p, 0, -1, p, p, 1, 1, 16, None) == -1
    assert lib.lq_q_pack(p, p, 0, 8, p, p, 0, 1, 16, None) == -1
    assert b"positive" in lib.lq_last_error()
    assert lib.lq_q_pack(p, p, 0, 8, p, p, 1, -3, 16, None) == -1
    assert lib.lq_q_pack(p, p, 0, 8, p, p, 1, 1, (1 << 31) + 1, None) == -1     # 32-bit element indices
    assert lib.lq_q_pack(p + 4, p, 0, 8, p, p, 1, 1, 16, None) == -4            # float4 loads
    assert lib.lq_q_pack(p, p + 2, 0, 8, p, p, 1, 1, 16, None) == -4
    assert lib.lq_q_pack(p, p, 0, 8, None, p, 1, 1, 16, None) == -1             # words needed when bits > 0
    assert lib.lq_q_pack(p, p, 0, 8, p + 2, p, 1, 1, 16, None) == -4
    assert lib.lq_q_pack(p, p, 0, 8, p, None, 1, 1, 16, None) == -1             # the rejection counter is required
    assert lib.lq_q_pack(p, p, 0, 8, p, p + 4, 1, 1, 16, None) == -4
    u = lib.lq_q_unpack
    assert u(None, 0, 8, p, p, p, p, p, 1, 1, 16, None) == -1
    assert u(p, 0, 33, p, p, p, p, p, 1, 1, 16, None) == -1
    assert u(p, 0, 8, None, p, p, p, p, 1, 1, 16, None) == -1
    assert u(p, 0, 8, p, None, None, None, p, 1, 1, 16, None) == -1            # nothing to compute
    assert u(p, 0, 8, p, p, p, p, None, 1, 1, 16, None) == -1                  # p_restore is always checked
    assert u(p, 0, 8, p, p + 4, None, None, None, 1, 1, 16, None) == -4        # 16-byte stores
    assert u(p, 0, 8, p, None, p + 8, None, None, 1, 1, 16, None) == -4
    assert u(p, 0, 8, p, None, None, p + 4, p, 1, 1, 16, None) == -4
    assert u(p, 0, 8, p, None, None, p, p + 4, 1, 1, 16, None) == -4
    assert u(p + 2, 0, 8, p, p, None, None, None, 1, 1, 16, None) == -4
    assert u(p, 0, 8, p, p, None, None, None, 1, 0, 16, None) == -1
    assert u(p, 0, 8, p, p, None, None, None, 1, 1, (1 << 31) + 1, None) == -1
    del buf


# ------------------------------------------------------------------ container checks of load_packed_parameters
def _model():
    lq.reset_layer_names()
    return lq.build_model("cifar", mode="nq", value=1e-11, seed=42, orientation="channelwise")


def _container(model, path, edit=None):
    """A well-formed container of ``model`` (every code 0, bits 0), written by hand; ``edit(manifest, arrays)`` corrupts it."""
    tensors = export.quantized_tensors(model)
    sd = model.state_dict()
    state = export._plain_state_keys(model, tensors)
    manifest = {"format": "lq-packed", "version": 1,
                "tensors": [{"name": n, "shape": list(p.shape), "scale_shape": list(nq.scale.shape), "orientation": nq.orientation,
                             "qmin": 0, "bits": 0, "numel": p.numel()} for n, p, nq in tensors],
                "state": state}
    arrays = {}
    for n, p, nq in tensors:
        arrays[n + ".codes"] = np.zeros(0, dtype=np.uint32)
        arrays[n + ".scale"] = nq.scale.detach().numpy().copy()
    for k in state:
        arrays["state/" + k] = sd[k].numpy().copy()
    if edit is not None:
        edit(manifest, arrays)
    arrays["manifest"] = np.frombuffer(json.dumps(manifest).encode("utf-8"), dtype=np.uint8)
    with open(path, "wb") as fh:
        np.savez(fh, **arrays)
    return path


def _snapshot(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def _unchanged(model, snap):
    sd = model.state_dict()
    return sd.keys() == snap.keys() and all(torch.equal(sd[k], snap[k]) for k in snap)


def test_container_lists_every_state_entry_but_the_quantized_ones():
    m = _model()
    tensors = export.quantized_tensors(m)
    assert len(tensors) == 12                                               # 6 custom convs, kernel + bias each
    assert [n for n, _, _ in tensors][:2] == ["custom_conv2d_layer/W", "custom_conv2d_layer/b"]
    state = export._plain_state_keys(m, tensors)
    assert any("running_mean" in k for k in state) and any("num_batches_tracked" in k for k in state)
    assert not any(k.endswith(".kernel") or k.endswith(".scale") for k in state)
    assert any(k.startswith("dense") for k in state)                         # plain layers are state entries


def test_well_formed_container_passes_the_checks(tmp_path):
    """A consistent container gets past every check; only the device restore remains (there is no CPU fallback)."""
    m = _model()
    snap = _snapshot(m)
    path = _container(m, str(tmp_path / "weights_packed.npz"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lq.load_packed_parameters(m, str(tmp_path))
    assert _unchanged(m, snap)


def _set(key, value):
    def edit(manifest, arrays):
        manifest[key] = value
    return edit


def _drop_tensor(manifest, arrays):
    gone = manifest["tensors"].pop(3)
    del arrays[gone["name"] + ".codes"], arrays[gone["name"] + ".scale"]


def _shape(manifest, arrays):
    manifest["tensors"][2]["shape"][-1] += 1


def _orientation(manifest, arrays):
    manifest["tensors"][0]["orientation"] = "rowwise"


def _drop_state(manifest, arrays):
    k = manifest["state"].pop(0)
    del arrays["state/" + k]


@pytest.mark.parametrize("edit,match", [(_set("format", "weights-npy"), "lq-packed"), (_set("version", 2), "version"),
                                        (_drop_tensor, "missing from the container"), (_shape, "shape"),
                                        (_orientation, "orientation"), (_drop_state, "state entries")])
def test_load_rejects_a_mismatched_container_and_leaves_the_model_untouched(tmp_path, edit, match):
    m = _model()
    snap = _snapshot(m)
    path = _container(m, str(tmp_path / "weights_packed.npz"), edit)
    with pytest.raises(ValueError, match=match):
        lq.load_packed_parameters(m, path)
    assert _unchanged(m, snap)


def test_load_rejects_a_model_of_another_storage_order_only_by_content(tmp_path):
    """The manifest speaks about the reference layout: a container of an "hwio" model passes the checks of an "oihw" one."""
    lq.reset_layer_names()
    hwio = lq.build_model("cifar", kernel_storage="hwio", mode="nq", value=1e-11, seed=42, orientation="channelwise")
    path = _container(hwio, str(tmp_path / "weights_packed.npz"))
    m = _model()
    snap = _snapshot(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lq.load_packed_parameters(m, path)
    assert _unchanged(m, snap)
