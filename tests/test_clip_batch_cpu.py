"""CPU tests of the clipped multi-tensor batch's opt-in (no GPU): every refusal is raised before anything touches the device.

The default call forms keep refusing a layer with a range ("masked copy": tests/test_clip_cpu.py::test_the_batch_is_refused pins
that) and now name the opt-in; ``clipped=True`` / ``clipped_batch=True`` refuse what a clipped batch cannot do."""
import ctypes

import pytest
import torch

import learned_quantization_amd as lq
from learned_quantization_amd import _hip
from learned_quantization_amd.batch import FakeQuantBatch

CPU = torch.device("cpu")


def _dense(**kw):
    return lq.CustomDenseLayer(units=3, initializer=lq.RandomNormal(seed=2), input_shape=5, **kw)


def test_the_default_forms_still_refuse_and_name_the_opt_in():
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="masked copy") as e:
        Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, batched=True, bits=4)
    assert "clipped_batch=True" in str(e.value) and "--clipped-batch" in str(e.value)
    lq.reset_layer_names()
    with pytest.raises(ValueError, match="masked copy") as e:
        FakeQuantBatch([_dense(scale_gradient="ste", bits=4)])
    assert "clipped=True" in str(e.value)
    with pytest.raises(ValueError, match="masked copy"):
        FakeQuantBatch([_dense(scale_gradient="ste", bits=4)], clipped=False)


def test_trainer_opt_in_needs_the_batch_and_a_range():
    from learned_quantization_amd.train import Trainer
    with pytest.raises(ValueError, match="batched=True"):
        Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, batched=False, clipped_batch=True, bits=4)
    with pytest.raises(ValueError, match="bits / q_range"):
        Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, batched=True, clipped_batch=True)
    # what a range refuses stays refused with the opt-in: mode B and the nested-quantization modes
    with pytest.raises(ValueError, match="clipped elements"):
        Trainer("mnist", "cl", 1e-7, "rowwise", "maxbin", device=CPU, ddp_mode="B", batched=True, clipped_batch=True, bits=4)
    with pytest.raises(ValueError, match="linear in dy"):
        Trainer("mnist", "ste", 0.0, "rowwise", device=CPU, ddp_mode="B", batched=True, clipped_batch=True, bits=4)
    with pytest.raises(ValueError):
        Trainer("mnist", "nq", 1e-11, "rowwise", device=CPU, batched=True, clipped_batch=True, bits=4)


def test_clipped_batch_refuses_a_layer_without_a_range():
    lq.reset_layer_names()
    with pytest.raises(ValueError, match="without a range"):
        FakeQuantBatch([_dense(scale_gradient="ste")], clipped=True)
    with pytest.raises(ValueError, match="without a range"):
        FakeQuantBatch([_dense(scale_gradient="ste", bits=4), _dense(scale_gradient="ste")], clipped=True)
    with pytest.raises(ValueError, match="without a range"):
        FakeQuantBatch(lq.build_model("mnist", mode="ste", value=0.0), clipped=True)


def test_clipped_batch_holds_one_rounding_and_one_rule():
    lq.reset_layer_names()
    with pytest.raises(ValueError, match="one rounding"):
        FakeQuantBatch([_dense(scale_gradient="ste", bits=4), _dense(scale_gradient="ste", bits=4, rounding="nearest")], clipped=True)
    with pytest.raises(ValueError, match="one scale-gradient rule"):
        FakeQuantBatch([_dense(scale_gradient="ste", bits=4), _dense(bits=4)], clipped=True)


def test_hwio_stored_conv_kernel_is_refused_with_the_ste_batch_s_message():
    lq.reset_layer_names()
    conv = lq.CustomConv2DLayer(filters=4, initializer=lq.RandomNormal(seed=3), input_shape=2, bits=4, kernel_storage="hwio")
    with pytest.raises(ValueError, match='kernel_storage="oihw"'):
        FakeQuantBatch([conv], clipped=True)


@pytest.mark.parametrize("module", ["train", "experiment"])
def test_argument_parsers_accept_the_flag(module):
    import importlib
    ap = importlib.import_module(f"learned_quantization_amd.{module}").build_parser()
    base = ["--seed", "1", "--orientation", "rowwise", "--training", "from_scratch"] if module == "experiment" else []
    assert ap.parse_args(base + ["--batched", "--clipped-batch", "--bits", "4"]).clipped_batch is True
    assert ap.parse_args(base + ["--batched"]).clipped_batch is False


def test_abi_refusals_that_need_no_device():
    """NULL batch: every new entry point returns LQ_EINVAL with a message (the device-side refusals are in tests/test_gpu_clip_batch.py)."""
    lib = _hip.load()
    one = (ctypes.c_int32 * 1)(0)
    dev, groups = ctypes.c_void_p(), ctypes.c_int64()
    assert lib.lq_batch_set_clip(None, one, one, 1, 0) == -1 and b"NULL batch" in lib.lq_last_error()
    assert lib.lq_batch_forward_clip(None, None) == -1 and b"NULL batch" in lib.lq_last_error()
    assert lib.lq_batch_backward_clip(None, None, None, None, 0, None) == -1 and b"NULL batch" in lib.lq_last_error()
    assert lib.lq_batch_clip_counts(None, 0, ctypes.byref(dev), ctypes.byref(groups)) == -1
