"""CPU tests of asymmetric layers in the group batch (include/lq_hip.h: lq_group_batch_create_affine;
FakeQuantBatch(group_batch=True, asymmetric=True); Trainer(asymmetric_batch=True)) -- no GPU.

``lq_group_batch_create_affine`` validates the descriptors and the offsets before its first HIP call, so each LQ_EINVAL / LQ_EALIGN
is reached on a machine without a device, with made-up addresses that are never dereferenced; the Python refusals are raised before
anything touches the device either."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip
from learned_quantization_amd.batch import BatchedScaleAdam, FakeQuantBatch

CPU = torch.device("cpu")
EINVAL, EALIGN = -1, -4
A = 0x10000          # a made-up, 16-byte aligned device address: create() must refuse before it would ever be dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
    d = dict(P=A, s=A, out=A, dp=A, ds=A, R=8, C=8, gs=4, axis=0, qmin=-8, qmax=7)
    d.update(kw)
    return _hip.GroupDesc(d["P"], d["s"], d["out"], d["dp"], d["ds"], d["R"], d["C"], d["gs"], d["axis"], d["qmin"], d["qmax"])


def _off(b=A, db=A, kb=0.5):
    return _hip.GroupOffset(b, db, kb)


def _create(descs, offs, rounding=0, n=None):
    lib = _hip.load()
    arr = (_hip.GroupDesc * max(1, len(descs)))(*descs)
    oarr = None if offs is None else (_hip.GroupOffset * max(1, len(offs)))(*offs)
    handle = ctypes.c_void_p()
    rc = lib.lq_group_batch_create_affine(arr, oarr, len(descs) if n is None else n, rounding, ctypes.byref(handle))
    assert handle.value is None or rc == 0
    return rc, lib.lq_last_error().decode()


def test_symbol_struct_and_version():
    lib = _hip.load()
    assert lib.lq_version() == 3
    assert "lq_group_batch_create_affine" in _hip.SIGNATURES and hasattr(lib, "lq_group_batch_create_affine")
    assert ctypes.sizeof(_hip.GroupDesc) == 5 * 8 + 3 * 8 + 3 * 4 + 4      # unchanged: five pointers, three int64, three int32, padding
    assert ctypes.sizeof(_hip.GroupOffset) == 24                            # two pointers, a float, tail padding
    assert [f[0] for f in _hip.GroupOffset._fields_] == ["b", "db", "offset_grad_scale"]
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    assert re.search(r"int\s+lq_group_batch_create_affine\s*\(\s*const lq_group_desc\*\s*descs,\s*const lq_group_offset\*\s*offs", header)
    body = re.search(r"typedef struct lq_group_offset \{(.*?)\} lq_group_offset;", header, re.S).group(1)
    assert [m for m in re.findall(r"(\w+);\s*/\*", body)] == ["b", "db", "offset_grad_scale"]
    assert re.search(r"typedef struct lq_group_desc \{.*?int32_t axis, qmin, qmax;\s*\} lq_group_desc;", header, re.S)


@pytest.mark.parametrize("what,off,code", [
    ("db", dict(b=None, db=A), EINVAL),
    ("offset_grad_scale", dict(kb=float("nan")), EINVAL), ("offset_grad_scale", dict(kb=float("inf")), EINVAL),
    ("offset_grad_scale", dict(kb=float("-inf")), EINVAL),
    ("aligned", dict(b=A + 2), EALIGN), ("aligned", dict(db=A + 1), EALIGN), ("aligned", dict(b=A + 3, db=None), EALIGN)])
def test_create_affine_refuses_offsets_before_any_hip_call(what, off, code):
    rc, msg = _create([_desc(), _desc()], [_off(), _off(**off)])
    assert rc == code, msg
    assert "lq_group_batch_create_affine" in msg and "tensor 1" in msg and what in msg, msg


def test_a_symmetric_tensor_ignores_its_factor():
    """b == NULL and db == NULL: the tensor is symmetric and its offset_grad_scale is not looked at.  Nothing here is refused, so
    the call goes on to its first HIP call: without a device that fails with LQ_EHIP, which is no refusal of the arguments."""
    lib = _hip.load()
    arr = (_hip.GroupDesc * 1)(_desc())
    oarr = (_hip.GroupOffset * 1)(_off(b=None, db=None, kb=float("nan")))
    handle = ctypes.c_void_p()
    rc = lib.lq_group_batch_create_affine(arr, oarr, 1, 0, ctypes.byref(handle))
    assert rc not in (EINVAL, EALIGN), lib.lq_last_error().decode()
    if rc == 0:
        lib.lq_group_batch_destroy(handle)


@pytest.mark.parametrize("what,kw,code", [
    ("P", dict(P=None), EINVAL), ("s", dict(s=None), EINVAL), ("out", dict(out=None), EINVAL), ("dp", dict(dp=None), EINVAL),
    ("axis", dict(axis=2), EINVAL), ("group size", dict(gs=0), EINVAL), ("positive", dict(R=0), EINVAL),
    ("2^31", dict(R=1 << 16, C=1 << 15), EINVAL), ("qmin", dict(qmin=3, qmax=2), EINVAL), ("2^24", dict(qmax=(1 << 24) + 1), EINVAL),
    ("aligned", dict(P=A + 2), EALIGN), ("aligned", dict(ds=A + 2), EALIGN)])
@pytest.mark.parametrize("with_offsets", [False, True], ids=["offs=NULL", "offs"])
def test_create_affine_keeps_every_refusal_of_create(what, kw, code, with_offsets):
    """offs = NULL is accepted exactly where lq_group_batch_create accepts: the same code and the same tensor for every bad
    descriptor, with and without offsets, and the same verdict from lq_group_batch_create itself."""
    descs = [_desc(), _desc(**kw)]
    rc, msg = _create(descs, [_off(), _off()] if with_offsets else None)
    assert rc == code, msg
    assert "lq_group_batch_create_affine" in msg and "tensor 1" in msg and what in msg, msg
    lib = _hip.load()
    arr = (_hip.GroupDesc * 2)(*descs)
    assert lib.lq_group_batch_create(arr, 2, 0, ctypes.byref(ctypes.c_void_p())) == code
    assert b"lq_group_batch_create:" in lib.lq_last_error()


def test_create_affine_refuses_counts_rounding_and_null_arguments():
    for n in (0, -1, 257):
        assert _create([_desc()], None, n=n)[0] == EINVAL
    rc, msg = _create([_desc()], [_off()], rounding=2)
    assert rc == EINVAL and "rounding" in msg
    lib = _hip.load()
    assert lib.lq_group_batch_create_affine(None, None, 1, 0, ctypes.byref(ctypes.c_void_p())) == EINVAL
    assert lib.lq_group_batch_create_affine((_hip.GroupDesc * 1)(_desc()), None, 1, 0, None) == EINVAL


# ---------------------------------------------------------------------------------------------------------- Python refusals
def _dense(**kw):
    kw.setdefault("scale_gradient", "ste")
    kw.setdefault("bits", 4)
    return lq.CustomDenseLayer(units=3, initializer=lq.RandomNormal(seed=2), input_shape=8, **kw)


def _gdense(**kw):
    return _dense(orientation="groupwise", group_size=4, **kw)


def _adense(**kw):
    return _gdense(asymmetric=True, **kw)


def test_without_the_opt_in_the_refusal_stays_and_names_it():
    lq.reset_layer_names()
    for kw in (dict(), dict(clipped=True), dict(group_batch=True)):
        with pytest.raises(ValueError, match="asymmetric") as e:
            FakeQuantBatch([_adense()], **kw)
        assert "asymmetric=True" in str(e.value) and "group_batch=True" in str(e.value)


def test_batch_refusals_with_the_opt_in():
    lq.reset_layer_names()
    with pytest.raises(ValueError, match="belongs to group_batch=True"):
        FakeQuantBatch([_adense()], asymmetric=True)
    with pytest.raises(ValueError, match="asymmetric=True together with clipped=True"):
        FakeQuantBatch([_adense()], asymmetric=True, clipped=True)
    with pytest.raises(ValueError, match="asymmetric=True together with clipped=True"):
        FakeQuantBatch([_adense()], asymmetric=True, clipped=True, group_batch=True)
    with pytest.raises(ValueError, match="loss term"):
        FakeQuantBatch([_adense(), _dense(bits=4, penalty_rate=1e-7)], group_batch=True, asymmetric=True)
    conv = lq.CustomConv2DLayer(filters=4, initializer=lq.RandomNormal(seed=3), input_shape=2, bits=4, kernel_storage="hwio",
                                scale_gradient="ste")
    with pytest.raises(ValueError, match='kernel_storage="oihw"'):
        FakeQuantBatch([_adense(), conv], group_batch=True, asymmetric=True)
    with pytest.raises(ValueError, match="one rounding"):
        FakeQuantBatch([_adense(), _gdense(rounding="nearest")], group_batch=True, asymmetric=True)


def test_what_a_built_asymmetric_batch_refuses():
    """Mode B, the loss term and the fused Adam step on an object that skipped the device-side construction."""
    b = FakeQuantBatch.__new__(FakeQuantBatch)
    b._set_kind(clipped=False, group_batch=True, asymmetric=True)
    b.ste, b.defer_scale_grads, b.entries = True, True, []
    with pytest.raises(ValueError, match="mode B"):
        b._backward_core([])                                            # defer_scale_grads is set
    with pytest.raises(ValueError, match="mode B"):
        b.scale_grads_from_param_grads()
    with pytest.raises(ValueError, match="loss term"):
        b.inject_penalty_grads("maxbin", 1e-7)
    with pytest.raises(ValueError, match="fused=False") as e:
        BatchedScaleAdam(b, fused=True)
    assert "asymmetric=True" in str(e.value)


def test_the_adam_set_limit_is_stated():
    assert FakeQuantBatch.ADAM_SET_MAX == 256
    assert "256" in FakeQuantBatch.__init__.__doc__ and "scales + offsets" in FakeQuantBatch.__init__.__doc__


def test_trainer_refusals_and_defaults():
    from learned_quantization_amd.train import Trainer
    assert inspect.signature(Trainer.__init__).parameters["asymmetric_batch"].default is False
    assert inspect.signature(FakeQuantBatch.__init__).parameters["asymmetric"].default is False
    base = dict(device=CPU, bits=4, group_size=64)
    for kw in (dict(), dict(asymmetric=True), dict(asymmetric=True, batched=True), dict(batched=True, group_batch=True),
               dict(asymmetric=True, group_batch=True)):
        with pytest.raises(ValueError, match="asymmetric_batch=True belongs to"):
            Trainer("mnist", "ste", 0.0, asymmetric_batch=True, **base, **kw)
    # the refusal without the opt-in stays, and names it
    with pytest.raises(ValueError, match="asymmetric") as e:
        Trainer("mnist", "ste", 0.0, asymmetric=True, batched=True, group_batch=True, **base)
    assert "asymmetric_batch=True" in str(e.value) and "--asymmetric-batch" in str(e.value)
    # what asymmetric layers refuse stays refused with the opt-in
    with pytest.raises(ValueError, match="ddp_mode 'B'"):
        Trainer("mnist", "ste", 0.0, asymmetric=True, batched=True, group_batch=True, asymmetric_batch=True, ddp_mode="B", **base)
    with pytest.raises(ValueError, match="without clipped_batch"):
        Trainer("mnist", "ste", 0.0, asymmetric=True, batched=True, group_batch=True, asymmetric_batch=True, clipped_batch=True, **base)
    with pytest.raises(ValueError, match="kernel_storage"):
        Trainer("cifar", "ste", 0.0, asymmetric=True, batched=True, group_batch=True, asymmetric_batch=True, kernel_storage="hwio",
                device=CPU, bits=4, group_size=128)


@pytest.mark.parametrize("module", ["train", "experiment"])
def test_argument_parsers(module, capsys):
    import importlib
    ap = importlib.import_module(f"learned_quantization_amd.{module}").build_parser()
    base = ["--seed", "1", "--orientation", "rowwise", "--training", "from_scratch"] if module == "experiment" else []
    full = base + ["--bits", "4", "--group-size", "128", "--asymmetric", "--batched", "--group-batch", "--asymmetric-batch"]
    assert ap.parse_args(full).asymmetric_batch is True
    assert ap.parse_args(full + ["--scale-init", "minmax"]).scale_init == "minmax"
    assert ap.parse_args(base + ["--bits", "4", "--group-size", "128", "--asymmetric"]).asymmetric_batch is False
    for drop in ("--asymmetric", "--batched", "--group-batch"):
        with pytest.raises(SystemExit):
            ap.parse_args([a for a in full if a != drop])
        assert "--asymmetric-batch needs" in capsys.readouterr().err
