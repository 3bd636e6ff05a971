"""CPU tests of the group batch (include/lq_hip.h: lq_group_batch_*; FakeQuantBatch(group_batch=True)) -- no GPU.

``lq_group_batch_create`` validates every descriptor before its first HIP call, so each LQ_EINVAL / LQ_EALIGN is reached on a
machine without a device; the Python refusals are raised before anything touches the device either.  The last test pins the
geometry the batch gives a bias -- one line, one group: (R, C, axis, gs) = (1, n, 1, n) -- to the one-axis clipped reference."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from _clip_reference import bits_equal, clip_reference            # noqa: E402
from _group_reference import group_reference                      # noqa: E402

import learned_quantization_amd as lq                              # noqa: E402
from learned_quantization_amd import _hip                          # noqa: E402
from learned_quantization_amd.batch import BatchedScaleAdam, FakeQuantBatch      # noqa: E402

CPU = torch.device("cpu")
EINVAL, EALIGN = -1, -4
A = 0x10000          # a made-up, 16-byte aligned device address: create() must refuse before it would ever be dereferenced


def _desc(**kw):
    d = dict(P=A, s=A, out=A, dp=A, ds=A, R=8, C=8, gs=4, axis=0, qmin=-8, qmax=7)
    d.update(kw)
    return _hip.GroupDesc(d["P"], d["s"], d["out"], d["dp"], d["ds"], d["R"], d["C"], d["gs"], d["axis"], d["qmin"], d["qmax"])


def _create(descs, rounding=0, n=None):
    lib = _hip.load()
    arr = (_hip.GroupDesc * max(1, len(descs)))(*descs)
    handle = ctypes.c_void_p()
    rc = lib.lq_group_batch_create(arr, len(descs) if n is None else n, rounding, ctypes.byref(handle))
    assert handle.value is None or rc == 0
    return rc, lib.lq_last_error().decode()


def test_symbols_and_version():
    lib = _hip.load()
    assert lib.lq_version() == 3
    for name in ("lq_group_batch_create", "lq_group_batch_destroy", "lq_group_batch_workspace_bytes", "lq_group_batch_forward",
                 "lq_group_batch_backward", "lq_group_batch_clip_counts"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert ctypes.sizeof(_hip.GroupDesc) == 5 * 8 + 3 * 8 + 3 * 4 + 4      # five pointers, three int64, three int32, tail padding


@pytest.mark.parametrize("what,kw,code", [
    ("P", dict(P=None), EINVAL), ("s", dict(s=None), EINVAL), ("out", dict(out=None), EINVAL), ("dp", dict(dp=None), EINVAL),
    ("axis", dict(axis=2), EINVAL), ("axis", dict(axis=-1), EINVAL), ("group size", dict(gs=0), EINVAL),
    ("positive", dict(R=0), EINVAL), ("positive", dict(C=-3), EINVAL), ("2^31", dict(R=1 << 16, C=1 << 15), EINVAL),
    ("qmin", dict(qmin=3, qmax=2), EINVAL), ("2^24", dict(qmax=(1 << 24) + 1), EINVAL), ("2^24", dict(qmin=-(1 << 24) - 1), EINVAL),
    ("aligned", dict(P=A + 2), EALIGN), ("aligned", dict(s=A + 1), EALIGN), ("aligned", dict(out=A + 2), EALIGN),
    ("aligned", dict(dp=A + 3), EALIGN), ("aligned", dict(ds=A + 2), EALIGN)])
def test_create_refuses_before_any_hip_call(what, kw, code):
    rc, msg = _create([_desc(), _desc(**kw)])
    assert rc == code, msg
    assert "tensor 1" in msg and what in msg, msg


def test_create_refuses_counts_and_rounding():
    assert _create([_desc()], n=0)[0] == EINVAL
    assert _create([_desc()], n=-1)[0] == EINVAL
    assert _create([_desc()], n=257)[0] == EINVAL
    rc, msg = _create([_desc()], rounding=2)
    assert rc == EINVAL and "rounding" in msg
    lib = _hip.load()
    assert lib.lq_group_batch_create(None, 1, 0, ctypes.byref(ctypes.c_void_p())) == EINVAL
    assert lib.lq_group_batch_create((_hip.GroupDesc * 1)(_desc()), 1, 0, None) == EINVAL


def test_null_batch_is_refused_by_the_other_five_calls():
    lib = _hip.load()
    dev, groups = ctypes.c_void_p(), ctypes.c_int64()
    assert lib.lq_group_batch_destroy(None) == EINVAL and b"NULL batch" in lib.lq_last_error()
    assert lib.lq_group_batch_forward(None, None) == EINVAL and b"NULL batch" in lib.lq_last_error()
    assert lib.lq_group_batch_backward(None, None, None, None, 0, None) == EINVAL and b"NULL batch" in lib.lq_last_error()
    assert lib.lq_group_batch_clip_counts(None, 0, ctypes.byref(dev), ctypes.byref(groups)) == EINVAL
    assert lib.lq_group_batch_workspace_bytes(None) == 0      # a size, not a status: 0 for every shipped form


# ---------------------------------------------------------------------------------------------------------- Python refusals
def _dense(**kw):
    kw.setdefault("scale_gradient", "ste")
    kw.setdefault("bits", 4)
    return lq.CustomDenseLayer(units=3, initializer=lq.RandomNormal(seed=2), input_shape=8, **kw)


def _gdense(**kw):
    return _dense(orientation="groupwise", group_size=4, **kw)


def test_a_batch_over_a_group_wise_layer_names_the_opt_in():
    lq.reset_layer_names()
    for kw in (dict(), dict(clipped=True)):
        with pytest.raises(ValueError, match="group_batch=True"):
            FakeQuantBatch([_gdense()], **kw)


def test_group_batch_refusals():
    lq.reset_layer_names()
    with pytest.raises(ValueError, match="together with clipped=True"):
        FakeQuantBatch([_gdense()], group_batch=True, clipped=True)
    with pytest.raises(ValueError, match="clipped batch"):              # any other one-axis orientation
        FakeQuantBatch([_gdense(), _dense(orientation="rowwise")], group_batch=True)
    with pytest.raises(ValueError, match="without a range"):
        FakeQuantBatch([_gdense(), _dense(bits=None)], group_batch=True)
    with pytest.raises(ValueError, match="one rounding"):
        FakeQuantBatch([_gdense(), _gdense(rounding="nearest")], group_batch=True)
    with pytest.raises(ValueError, match="one scale-gradient rule"):
        FakeQuantBatch([_gdense(), _gdense(scale_gradient=None)], group_batch=True)
    with pytest.raises(ValueError, match="loss term"):
        FakeQuantBatch([_gdense(), _dense(bits=4, penalty_rate=1e-7)], group_batch=True)
    conv = lq.CustomConv2DLayer(filters=4, initializer=lq.RandomNormal(seed=3), input_shape=2, bits=4, kernel_storage="hwio",
                                scale_gradient="ste")
    with pytest.raises(ValueError, match='kernel_storage="oihw"'):
        FakeQuantBatch([_gdense(), conv], group_batch=True)


def test_what_a_built_group_batch_refuses():
    """The refusals of an existing batch, on an object that skipped the device-side construction."""
    b = FakeQuantBatch.__new__(FakeQuantBatch)
    b._set_kind(clipped=False, group_batch=True, asymmetric=False)
    b.ste, b.defer_scale_grads, b.entries = True, True, []
    with pytest.raises(ValueError, match="group_batch=True"):
        b.scale_grads_from_param_grads()
    with pytest.raises(ValueError, match="group_batch=True"):
        b._backward_core([])                                            # defer_scale_grads is set
    with pytest.raises(ValueError, match="group_batch=True"):
        b.inject_penalty_grads("maxbin", 1e-7)
    with pytest.raises(ValueError, match="group_batch=True"):
        b.penalty_values("maxbin")
    with pytest.raises(ValueError, match="fused=False"):
        BatchedScaleAdam(b, fused=True)


def test_trainer_refusals():
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="belongs to batched=True"):
        Trainer("mnist", "ste", 0.0, device=CPU, bits=4, group_size=64, group_batch=True)
    with pytest.raises(ValueError, match="needs group_size"):
        Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, bits=4, batched=True, group_batch=True)
    with pytest.raises(ValueError, match="without clipped_batch"):
        Trainer("mnist", "ste", 0.0, device=CPU, bits=4, group_size=64, batched=True, group_batch=True, clipped_batch=True)
    # the two existing refusals still fire without the keyword, and now name it
    with pytest.raises(ValueError, match="multi-tensor batch") as e:
        Trainer("mnist", "ste", 0.0, device=CPU, bits=4, group_size=64, batched=True)
    assert "group_batch=True" in str(e.value)
    with pytest.raises(ValueError, match="multi-tensor batch"):
        Trainer("mnist", "ste", 0.0, device=CPU, bits=4, group_size=64, batched=True, clipped_batch=True)
    # what group-wise scales refuse stays refused with the opt-in
    with pytest.raises(ValueError, match="ddp_mode 'B'"):
        Trainer("mnist", "ste", 0.0, device=CPU, bits=4, group_size=64, batched=True, group_batch=True, ddp_mode="B")
    with pytest.raises(ValueError, match="group_size with mode 'nq'"):
        Trainer("mnist", "nq", 1e-11, device=CPU, bits=4, group_size=64, batched=True, group_batch=True)


@pytest.mark.parametrize("module", ["train", "experiment"])
def test_argument_parsers_accept_the_flag(module):
    import importlib
    ap = importlib.import_module(f"learned_quantization_amd.{module}").build_parser()
    base = ["--seed", "1", "--orientation", "rowwise", "--training", "from_scratch"] if module == "experiment" else []
    assert ap.parse_args(base + ["--batched", "--group-batch", "--bits", "4", "--group-size", "128"]).group_batch is True
    assert ap.parse_args(base + ["--batched"]).group_batch is False


# ------------------------------------------------------------------------------------------------------- the bias geometry
@pytest.mark.parametrize("n", [1, 10, 512])
@pytest.mark.parametrize("rng_", [(-8, 7), (0, 15), (-3, 5)])
def test_bias_geometry_is_the_scalar_scale_clipped_reference(n, rng_):
    """(R, C, axis, gs) = (1, n, 1, n) of group_reference == clip_reference with a scalar scale: out, dP and the count bit for bit."""
    rng = np.random.default_rng(1000 + n)
    s = np.exp2(rng.uniform(-9.0, -5.0, size=(1,))).astype(np.float32)
    P = (rng.standard_normal(n).astype(np.float32) * np.float32(8.0) * s[0]).astype(np.float32)
    dy = rng.standard_normal(n).astype(np.float32)
    g = group_reference(P.reshape(1, n), s.reshape(1, 1), dy.reshape(1, n), *rng_, 1, n, k=0.37)
    c = clip_reference(P, s, dy, *rng_, k=0.37)
    assert bits_equal(g["out"].reshape(n), c["out"]) and bits_equal(g["dP"].reshape(n), c["dP"])
    assert int(g["clipped"].reshape(())) == int(np.asarray(c["clipped"]).reshape(()))
    assert np.array_equal(g["q"].reshape(n), c["q"])
