"""CPU tests of the penalty-value entry points and the device-side loss log: C-ABI surface, argument validation without a
launch, and the host side of ``LossLog`` (no GPU here)."""
import ctypes
import os
import re
import warnings

import pytest

import learned_quantization_amd as lq
from learned_quantization_amd import _hip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("lq_batch_penalty_values", "lq_batch_penalty_grads_values", "lq_loss_log_append")


def test_new_entry_points_are_declared_exported_and_bound():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/lq_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.SIGNATURES, f"{name} is not in the binding table"
    assert lib.lq_version() == 3            # additions only: the ABI version stays


def _err():
    return _hip.load().lq_last_error().decode()


def test_penalty_value_entry_points_validate_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)                # never dereferenced: every call below fails in validation
    dims = (ctypes.c_float * 2)(4.0, 2.0)
    start = (ctypes.c_uint8 * 2)(1, 0)
    coeff = (ctypes.c_float * 2)(0.5, 0.5)
    grads = (ctypes.c_void_p * 2)(p, p)
    # bad kind
    assert lib.lq_batch_penalty_values(None, 3, dims, start, p, p, p, 1024, None) == -1 and "bad kind 3" in _err()
    assert lib.lq_batch_penalty_values(None, -1, dims, start, p, p, p, 1024, None) == -1 and "bad kind" in _err()
    assert lib.lq_batch_penalty_grads_values(None, 7, coeff, grads, dims, start, p, p, p, 1024, None) == -1 and "bad kind 7" in _err()
    # the accumulate flag is not a kind of its own
    assert lib.lq_batch_penalty_grads_values(None, _hip.LQ_PENALTY_ACCUMULATE_DS | 5, coeff, grads, dims, start, p, p, p, 1024, None) == -1
    assert "bad kind 5" in _err()
    # NULL outputs / host tables
    assert lib.lq_batch_penalty_values(None, 0, dims, start, None, p, p, 1024, None) == -1 and "terms_dev is NULL" in _err()
    assert lib.lq_batch_penalty_values(None, 0, dims, start, p, None, p, 1024, None) == -1 and "penalty_dev is NULL" in _err()
    assert lib.lq_batch_penalty_values(None, 1, None, start, p, p, p, 1024, None) == -1 and "dims is NULL" in _err()
    assert lib.lq_batch_penalty_values(None, 1, dims, None, p, p, p, 1024, None) == -1 and "layer_start is NULL" in _err()
    assert lib.lq_batch_penalty_grads_values(None, 2, coeff, grads, dims, start, None, p, p, 1024, None) == -1 and "terms_dev is NULL" in _err()
    assert lib.lq_batch_penalty_grads_values(None, 2, coeff, grads, dims, start, p, None, p, 1024, None) == -1 and "penalty_dev is NULL" in _err()
    assert lib.lq_batch_penalty_values(None, 0, dims, start, p + 2, p, p, 1024, None) == -4       # LQ_EALIGN
    # NULL batch (everything else in order)
    for kind in (0, 1, 2):
        assert lib.lq_batch_penalty_values(None, kind, dims, start, p, p, p, 1024, None) == -1 and "NULL batch" in _err()
        assert lib.lq_batch_penalty_grads_values(None, kind, coeff, grads, dims, start, p, p, p, 1024, None) == -1 and "NULL batch" in _err()
    assert _err().startswith("lq_batch_penalty_grads_values:")
    # the entry point without values keeps its name in its messages
    assert lib.lq_batch_penalty_grads(None, 0, coeff, grads, p, 1024, None) == -1 and _err().startswith("lq_batch_penalty_grads: NULL batch")


def test_loss_log_append_validates_before_any_launch():
    lib = _hip.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.addressof(buf)
    assert p % 8 == 0
    assert lib.lq_loss_log_append(None, p, 0.1, p, 4, p, None, None) == -1 and "NULL" in _err()
    assert lib.lq_loss_log_append(p, None, 0.1, p, 4, p, None, None) == -1 and "NULL" in _err()
    assert lib.lq_loss_log_append(p, p, 0.1, None, 4, p, None, None) == -1 and "rows_dev is NULL" in _err()
    assert lib.lq_loss_log_append(p, p, 0.1, p, 4, None, None, None) == -1 and "cursor_dev is NULL" in _err()
    assert lib.lq_loss_log_append(p, p, 0.1, p, 0, p, None, None) == -1 and "capacity" in _err()
    assert lib.lq_loss_log_append(p, p, 0.1, p, -3, p, None, None) == -1 and "capacity" in _err()
    assert lib.lq_loss_log_append(p, p, 0.1, p, 4, p + 4, None, None) == -4 and "cursor_dev must be 8-byte aligned" in _err()
    assert lib.lq_loss_log_append(p + 2, p, 0.1, p, 4, p, None, None) == -4
    assert lib.lq_loss_log_append(p, p, 0.1, p, 4, p, p + 1, None) == -4


class _Obj:
    penalty_rate = 0.25
    _penalty_log = "maxbin_loss.log"

    def __init__(self, d):
        self.custom_loss_dir = str(d)


def test_loss_log_flush_formatting(tmp_path):
    d = tmp_path / "custom_losses"
    d.mkdir()
    log = lq.LossLog(_Obj(d), capacity=8)
    assert log.flush() == (0, 0)                                  # nothing appended yet: no device buffer, no file touched
    rows = [[2.5, 2.25, 0.25], [2.3025851249694824, 2.0, 0.30258512496948242]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                            # no dropped rows: no warning
        assert log._write(rows, 0) == (2, 0)
    names = ("total_loss.log", "scce_loss.log", "maxbin_loss.log")
    for col, name in enumerate(names):
        assert (d / name).read_text() == "".join(f"{r[col]}\n" for r in rows)      # _SCCEBase._append's format, one value per line
    assert (d / "total_loss.log").read_text().splitlines()[0] == "2.5"
    with pytest.warns(RuntimeWarning, match="3 rows were dropped"):
        assert log._write([[1.0, 0.5, 0.5]], 3) == (1, 3)
    for col, name in enumerate(names):                            # the second flush appends
        lines = (d / name).read_text().splitlines()
        assert len(lines) == 3 and float(lines[2]) == [1.0, 0.5, 0.5][col]
    with pytest.raises(ValueError):
        lq.LossLog(_Obj(d), capacity=0)


def test_loss_object_creates_the_same_files_the_log_appends_to(tmp_path):
    lq.reset_layer_names()
    obj = lq.SCCEDifference([], 1e-3, str(tmp_path))
    log = lq.LossLog(obj, capacity=4)
    assert log._write([[3.0, 2.0, 1.0]], 0) == (1, 0)
    d = tmp_path / "custom_losses"
    assert sorted(os.listdir(d)) == ["difference_loss.log", "scce_loss.log", "total_loss.log"]
    assert (d / "difference_loss.log").read_text() == "1.0\n"
