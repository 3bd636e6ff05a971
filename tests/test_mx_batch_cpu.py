"""CPU tests of microscaling (MX) layers in the group batch (include/lq_hip.h: lq_group_batch_create_mx;
FakeQuantBatch(group_batch=True, mx=True); Trainer(mx_batch=True)) -- no GPU.

``lq_group_batch_create_mx`` validates the descriptors and the formats before its first HIP call, so each LQ_EINVAL / LQ_EALIGN is
reached on a machine without a device, with made-up addresses that are never dereferenced; the Python refusals are raised before
anything touches the device either.  The condition on the inputs of tests/test_gpu_mx_batch.py -- every one of the 50 (rotation,
tensor) pairs saturates somewhere but not everywhere, with a ds that is NaN-free and not all zero -- is pinned here on the reference."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip
from learned_quantization_amd.batch import BatchedScaleAdam, FakeQuantBatch

sys.path.insert(0, os.path.dirname(__file__))
import _mx_reference as X                                                                 # noqa: E402

CPU = torch.device("cpu")
EINVAL, EALIGN = -1, -4
A = 0x10000          # a made-up, 16-byte aligned device address: create() must refuse before it would ever be dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET = [(37, 5, 0, 8), (256, 260, 0, 32), (96, 130, 0, 96), (7, 27, 1, 8), (64, 576, 1, 128), (33, 4100, 1, 128), (1, 10, 1, 10),
       (1, 512, 1, 512), (300, 64, 0, 1), (40, 64, 1, 4)]      # tests/test_gpu_mx_batch.py


# ------------------------------------------------------------------------------------------------- the GPU file's data condition
@pytest.mark.parametrize("i", range(len(SET)))
def test_every_rotation_of_the_gpu_set_saturates_somewhere_but_not_everywhere(i):
    names = list(X.FORMATS)
    assert len(names) == 5 and X.SCALE_FORMATS == ("e8m0", "fp32")
    sf = X.SCALE_FORMATS[i % 2]
    R, C, axis, gs = SET[i]
    for rot in range(5):
        name = names[(i + rot) % 5]
        P, s, dy = X.gaussian_case(name, sf, R, C, axis, gs)
        ref = X.mx_reference(P, s, dy, X.FORMATS[name], sf, axis, gs, k=float(np.float32(0.37 * (i + 1))))
        saturated = int(ref["clipped"].sum())
        assert 0 < saturated < P.size, f"tensor {i} {name} {sf}: {saturated} of {P.size} saturated"
        assert not np.isnan(ref["ds"]).any() and bool((ref["ds"] != 0).any()), f"tensor {i} {name} {sf}: ds is NaN or all zero"
    # tensor 4 carries the bad scales of test_bad_scale_stays_in_its_group: under E8M0 in every rotation
    assert X.SCALE_FORMATS[4 % 2] == "e8m0"


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _desc(**kw):
    d = dict(P=A, s=A, out=A, dp=A, ds=A, R=8, C=8, gs=4, axis=0, qmin=0, qmax=0)
    d.update(kw)
    return _hip.GroupDesc(d["P"], d["s"], d["out"], d["dp"], d["ds"], d["R"], d["C"], d["gs"], d["axis"], d["qmin"], d["qmax"])


def _create(descs, fmts, n=None):
    lib = _hip.load()
    arr = (_hip.GroupDesc * max(1, len(descs)))(*descs)
    farr = None if fmts is None else (_hip.GroupMxFormat * max(1, len(fmts)))(*[_hip.GroupMxFormat(*f) for f in fmts])
    handle = ctypes.c_void_p(0xDEAD0)                               # the call itself must reset it
    rc = lib.lq_group_batch_create_mx(arr, farr, len(descs) if n is None else n, ctypes.byref(handle))
    assert handle.value is None or rc == 0, "*out is not NULL after a refused create"
    return rc, lib.lq_last_error().decode()


def test_symbol_struct_and_version():
    lib = _hip.load()
    assert lib.lq_version() == 3                                    # additions only
    assert "lq_group_batch_create_mx" in _hip.SIGNATURES and hasattr(lib, "lq_group_batch_create_mx")
    assert ctypes.sizeof(_hip.GroupDesc) == 5 * 8 + 3 * 8 + 3 * 4 + 4      # unchanged: five pointers, three int64, three int32, padding
    assert ctypes.sizeof(_hip.GroupMxFormat) == 8                   # two int32
    assert [(f[0], getattr(_hip.GroupMxFormat, f[0]).offset, getattr(_hip.GroupMxFormat, f[0]).size) for f in _hip.GroupMxFormat._fields_] \
        == [("format", 0, 4), ("scale_format", 4, 4)]
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    assert re.search(r"int\s+lq_group_batch_create_mx\s*\(\s*const lq_group_desc\*\s*descs,\s*const lq_group_mx_format\*\s*fmts[^,]*,"
                     r"\s*int n,\s*lq_group_batch\*\*\s*out\)", header)
    body = re.search(r"typedef struct lq_group_mx_format \{(.*?)\} lq_group_mx_format;", header, re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+);\s*/\*", body) == [("int32_t", "format"), ("int32_t", "scale_format")]
    doc = header[header.index("microscaling (MX) tensors in the batch"):header.index("typedef struct lq_group_mx_format")]
    for needle in ("lq_fq_forward_mx / lq_fq_backward_mx", "qmin / qmax of a descriptor are not read", "no rounding argument", "ONE launch",
                   "saturation counts", "bit-identical", "LQ_EINVAL", "LQ_EALIGN", "mask only", "never inside a capture", "can be captured"):
        assert needle in doc, needle


def test_create_mx_refuses_formats_before_any_hip_call():
    rc, msg = _create([_desc(), _desc()], None)
    assert rc == EINVAL and "lq_group_batch_create_mx" in msg and "fmts" in msg, msg
    for bad, what in (((5, 0), "element format"), ((-1, 0), "element format"), ((0, 2), "scale format"), ((0, -1), "scale format")):
        rc, msg = _create([_desc(), _desc()], [(0, 0), bad])
        assert rc == EINVAL, msg
        assert "lq_group_batch_create_mx" in msg and "tensor 1" in msg and what in msg, msg


@pytest.mark.parametrize("what,kw,code", [
    ("P", dict(P=None), EINVAL), ("s", dict(s=None), EINVAL), ("out", dict(out=None), EINVAL), ("dp", dict(dp=None), EINVAL),
    ("axis", dict(axis=2), EINVAL), ("group size", dict(gs=0), EINVAL), ("positive", dict(R=0), EINVAL),
    ("2^31", dict(R=1 << 16, C=1 << 15), EINVAL), ("aligned", dict(P=A + 2), EALIGN), ("aligned", dict(ds=A + 2), EALIGN)])
def test_create_mx_keeps_the_refusals_of_create(what, kw, code):
    rc, msg = _create([_desc(), _desc(**kw)], [(0, 0), (3, 1)])
    assert rc == code, msg
    assert "lq_group_batch_create_mx" in msg and "tensor 1" in msg and what in msg, msg


def test_create_mx_does_not_read_the_range():
    """qmin > qmax and a bound outside +-2^24, which lq_group_batch_create refuses, pass the validation: the call goes on to its
    first HIP call, which without a device fails with LQ_EHIP -- no refusal of the arguments."""
    lib = _hip.load()
    for kw in (dict(qmin=3, qmax=2), dict(qmax=(1 << 24) + 1)):
        arr = (_hip.GroupDesc * 1)(_desc(**kw))
        assert lib.lq_group_batch_create(arr, 1, 0, ctypes.byref(ctypes.c_void_p())) == EINVAL
        handle = ctypes.c_void_p()
        rc = lib.lq_group_batch_create_mx(arr, (_hip.GroupMxFormat * 1)(_hip.GroupMxFormat(0, 0)), 1, ctypes.byref(handle))
        assert rc not in (EINVAL, EALIGN), lib.lq_last_error().decode()
        if rc == 0:
            lib.lq_group_batch_destroy(handle)


def test_create_mx_refuses_counts_and_null_arguments():
    for n in (0, -1, 257):
        assert _create([_desc()], [(0, 0)], n=n)[0] == EINVAL
    lib = _hip.load()
    fmts = (_hip.GroupMxFormat * 1)(_hip.GroupMxFormat(0, 0))
    assert lib.lq_group_batch_create_mx(None, fmts, 1, ctypes.byref(ctypes.c_void_p())) == EINVAL
    assert lib.lq_group_batch_create_mx((_hip.GroupDesc * 1)(_desc()), fmts, 1, None) == EINVAL


# ---------------------------------------------------------------------------------------------------------- Python refusals
def _mdense(element_format="fp4_e2m1", **kw):
    return lq.CustomDenseLayer(units=3, initializer=lq.RandomNormal(seed=2), input_shape=64, orientation="groupwise",
                               element_format=element_format, **kw)


def _gdense(**kw):
    return lq.CustomDenseLayer(units=3, initializer=lq.RandomNormal(seed=2), input_shape=64, orientation="groupwise", group_size=32,
                               scale_gradient="ste", bits=4, **kw)


def test_without_the_opt_in_the_refusal_stands_word_for_word():
    lq.reset_layer_names()
    for kw in (dict(), dict(clipped=True), dict(group_batch=True), dict(group_batch=True, asymmetric=True)):
        with pytest.raises(ValueError) as e:
            FakeQuantBatch([_mdense()], **kw)
        assert str(e.value) == ("FakeQuantBatch over a layer with an element format ('fp4_e2m1'): none of the multi-tensor batches "
                                "(default, clipped, group) carries a minifloat grid; run such a model on the per-tensor path "
                                "(batched=False)")


def test_batch_refusals_with_the_opt_in():
    lq.reset_layer_names()
    assert inspect.signature(FakeQuantBatch.__init__).parameters["mx"].default is False
    with pytest.raises(ValueError, match="mx=True belongs to group_batch=True"):
        FakeQuantBatch([_mdense()], mx=True)
    with pytest.raises(ValueError, match="mx=True together with clipped=True"):
        FakeQuantBatch([_mdense()], mx=True, group_batch=True, clipped=True)
    with pytest.raises(ValueError, match="mx=True together with asymmetric=True"):
        FakeQuantBatch([_mdense()], mx=True, group_batch=True, asymmetric=True)
    with pytest.raises(ValueError, match="without an element format"):
        FakeQuantBatch([_mdense(), _gdense()], mx=True, group_batch=True)
    with pytest.raises(ValueError, match="without an element format"):
        FakeQuantBatch([_gdense()], mx=True, group_batch=True)
    # a loss term and HWIO storage cannot be built into a layer with an element format: the layer itself refuses them, and the
    # batch's own check stands behind it
    with pytest.raises(ValueError, match="loss term"):
        _mdense(penalty_rate=1e-7)
    conv = lq.CustomConv2DLayer(filters=4, initializer=lq.RandomNormal(seed=3), input_shape=32, element_format="fp6_e2m3",
                                orientation="groupwise", kernel_storage="oihw")
    conv.kernel_storage = "hwio"
    with pytest.raises(ValueError, match='kernel_storage="oihw"'):
        FakeQuantBatch([_mdense(), conv], mx=True, group_batch=True)
    layer = _mdense()
    layer.nested_q_b_layer.penalty_rate = 1e-7
    with pytest.raises(ValueError, match="loss term"):
        FakeQuantBatch([layer], mx=True, group_batch=True)


def test_formats_may_differ_between_layers():
    """Two layers of different element and scale formats pass every check: the construction goes on to the device, which this
    machine does not have -- the refusal is the device's, not the batch's."""
    lq.reset_layer_names()
    a, b = _mdense("fp4_e2m1"), _mdense("fp8_e5m2", scale_format="fp32")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FakeQuantBatch([a, b], mx=True, group_batch=True)


def test_what_a_built_mx_batch_refuses():
    """Mode B, the loss term and the fused Adam step on an object that skipped the device-side construction."""
    b = FakeQuantBatch.__new__(FakeQuantBatch)
    b._set_kind(clipped=False, group_batch=True, asymmetric=False, mx=True)
    assert b.mx and b.group_batch and b._kind.mx and b._kind.owns_dp
    b.ste, b.defer_scale_grads, b.entries = True, True, []
    with pytest.raises(ValueError, match="mode B"):
        b._backward_core([])                                            # defer_scale_grads is set
    with pytest.raises(ValueError, match="mode B"):
        b.scale_grads_from_param_grads()
    with pytest.raises(ValueError, match="loss term"):
        b.inject_penalty_grads("maxbin", 1e-7)
    with pytest.raises(ValueError, match="loss term"):
        b.penalty_values("maxbin")
    with pytest.raises(ValueError, match="fused=False") as e:
        BatchedScaleAdam(b, fused=True)
    assert "mx=True" in str(e.value)
    # the plain group batch is not an MX batch
    b._set_kind(clipped=False, group_batch=True, asymmetric=False)
    assert not b.mx and not b._kind.mx


def test_trainer_refusals_and_defaults():
    from learned_quantization_amd.train import Trainer
    assert inspect.signature(Trainer.__init__).parameters["mx_batch"].default is False
    mx = dict(device=CPU, element_format="fp4_e2m1")
    # without the opt-in every current refusal stays
    for kw in (dict(batched=True), dict(batched=True, group_batch=True), dict(batched=True, clipped_batch=True), dict(group_batch=True)):
        with pytest.raises(ValueError, match="element_format with batched=True") as e:
            Trainer("mnist", "ste", 0.0, **mx, **kw)
        assert "per-tensor path" in str(e.value)
    # the opt-in belongs to element_format, group_batch and batched
    for kw in (dict(), dict(batched=True), dict(group_batch=True)):
        with pytest.raises(ValueError, match="mx_batch=True belongs to"):
            Trainer("mnist", "ste", 0.0, mx_batch=True, **mx, **kw)
    with pytest.raises(ValueError, match="mx_batch=True belongs to"):
        Trainer("mnist", "ste", 0.0, mx_batch=True, batched=True, group_batch=True, device=CPU, bits=4, group_size=64)
    with pytest.raises(ValueError, match="mx_batch=True with clipped_batch"):
        Trainer("mnist", "ste", 0.0, mx_batch=True, batched=True, group_batch=True, clipped_batch=True, **mx)
    # mode B stays refused, and what a model with an element format refuses stays refused with the opt-in
    with pytest.raises(ValueError, match="ddp_mode 'B'"):
        Trainer("mnist", "ste", 0.0, mx_batch=True, batched=True, group_batch=True, ddp_mode="B", **mx)
    with pytest.raises(ValueError, match="hwio"):
        Trainer("cifar", "ste", 0.0, mx_batch=True, batched=True, group_batch=True, kernel_storage="hwio", **mx)
    with pytest.raises(ValueError):
        Trainer("mnist", "ste", 0.0, mx_batch=True, batched=True, group_batch=True, bits=4, **mx)
    # the full line passes every check (group_size left at the MX default) and stops at the device
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X|HIP"):
        Trainer("mnist", "ste", 0.0, mx_batch=True, batched=True, group_batch=True, **mx)


@pytest.mark.parametrize("module", ["train", "experiment"])
def test_argument_parsers(module, capsys):
    import importlib
    ap = importlib.import_module(f"learned_quantization_amd.{module}").build_parser()
    if module == "experiment":
        base = ["--seed", "1", "--orientation", "rowwise", "--training", "from_scratch", "--scale-gradient", "ste"]
    else:
        base = ["--mode", "ste"]
    mx = base + ["--element-format", "fp4_e2m1"]
    full = mx + ["--batched", "--group-batch", "--mx-batch"]
    args = ap.parse_args(full + ["--scale-init", "cover", "--scale-format", "fp32"])
    assert args.mx_batch is True and args.batched and args.group_batch and args.group_size is None and args.scale_format == "fp32"
    assert ap.parse_args(mx).mx_batch is False
    for drop in ("--batched", "--group-batch"):
        with pytest.raises(SystemExit):
            ap.parse_args([a for a in full if a != drop])
        assert "--mx-batch needs" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--bits", "4", "--group-size", "32", "--batched", "--group-batch", "--mx-batch"])
    assert "--mx-batch needs" in capsys.readouterr().err
    # without the opt-in --element-format ... --batched is refused as before
    for extra in (["--batched"], ["--batched", "--group-batch"]):
        with pytest.raises(SystemExit):
            ap.parse_args(mx + extra)
        assert "--element-format with --batched" in capsys.readouterr().err
    for extra in (["--clipped-batch"], ["--bits", "4"], ["--rounding", "nearest"]):
        with pytest.raises(SystemExit):
            ap.parse_args(full + extra)
        capsys.readouterr()
