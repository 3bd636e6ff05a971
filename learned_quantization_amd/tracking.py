"""Scale / quantisation tracking statistics (SURVEY f-2) in the reference's log format.

Mirrors /root/reference/CIFAR-10/nested_quantization_layer/custom_components/custom_callbacks.py:
``NestedScaleTrackingCallback`` (:9-208) and ``AccuracyLossTrackingCallBack`` (:211-237).  File names,
directory layout (``on_epoch_end`` / ``on_train_end`` / ``on_train_begin``) and the
``Epoch N`` + one-value-per-line format are kept so the reference's plot_scripts.py parsers
(process_file_logged_per_epoch, plot_scripts.py:13-38) keep working.

The statistics that define the Pareto axes are computed on the GPU -- ``floor(P/s)`` by the HIP kernel K1,
``max|q|`` over axis 1 by ``lq_q_absmax_over_axis``, unique values/counts by ``lq_q_minmax`` + ``lq_q_histogram``
(LDS-privatised integer histogram) -- and only the
results cross PCIe.  The reference's per-epoch dump of every raw kernel value (:52-66) is opt-in
(``dump_values=True``): it is tens of MB of text per epoch and not needed by the Pareto plots.

``GroupQuantTrackingCallback`` (not in the reference) logs the clipped b-bit quantizer in the same format: per group the
clipped shares on either side and the SQNR, per tensor the SQNR, the codes in use and their entropy, from one
``lq_group_stats`` launch per tensor.  ``MxQuantTrackingCallback`` does the same for a layer with an element format (the OCP
microscaling quantizer): saturated and flushed shares, SQNR, the encodings in use, from one ``lq_mx_stats`` launch per tensor.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops
from .descriptor import init_geometry


def _shape(t) -> str:
    return "(" + ", ".join(str(int(d)) for d in t.shape) + ("," if t.dim() == 1 else "") + ")"


class NestedScaleTrackingCallback:
    def __init__(self, layer, log_dir, dump_values: bool = False):
        self.layer = layer
        self.dump_values = dump_values
        if hasattr(layer, "kernel"):
            self.param, self.qk_layer, kernel_name = layer.kernel, layer.nested_q_k_layer, f"Kernel_{layer.name}"
        else:
            self.param, self.qk_layer, kernel_name = layer.W, layer.nested_q_w_layer, "Weights"
        self.qb_layer = layer.nested_q_b_layer
        self.k_scale, self.b_scale = self.qk_layer.scale, self.qb_layer.scale
        bias_name = f"Bias_{layer.name}" if hasattr(layer, "kernel") else "Bias"
        ks_name, bs_name = self.qk_layer.scale_name, self.qb_layer.scale_name
        ksh, bsh = _shape(self.param), _shape(layer.b)
        kss, bss = _shape(self.k_scale), _shape(self.b_scale)
        e, t, b0 = (os.path.join(log_dir, d) for d in ("on_epoch_end", "on_train_end", "on_train_begin"))
        for d in (e, t, b0):
            os.makedirs(d, exist_ok=True)
        self.log_file_path_kernel = f"{e}/{kernel_name}_{ksh}.log"
        self.log_file_path_biases = f"{e}/{bias_name}_{bsh}.log"
        self.log_file_path_k_scale = f"{e}/{kernel_name}_{ksh}_{ks_name}_{kss}.log"
        self.log_file_path_b_scale = f"{e}/{bias_name}_{bsh}_{bs_name}_{bss}.log"
        self.log_file_path_qk_epoch = f"{e}/Number_of_unique_{kernel_name}_{ksh}.log"
        self.log_file_path_qb_epoch = f"{e}/Number_of_unique_{bias_name}_{bsh}.log"
        self.log_file_path_qk_epoch_max = f"{e}/Max_{kernel_name}_{ksh}.log"
        self.log_file_path_qb_epoch_max = f"{e}/Max_{bias_name}_{bsh}.log"
        self.log_file_path_qk = f"{t}/Quantized_{kernel_name}_{ksh}_{ks_name}_{kss}.log"
        self.log_file_path_qb = f"{t}/Quantized_{bias_name}_{bsh}_{bs_name}_{bss}.log"
        self.log_file_path_qk_unique = f"{t}/Unique_quantized_{kernel_name}_{ksh}_{ks_name}_{kss}.log"
        self.log_file_path_qb_unique = f"{t}/Unique_quantized_{bias_name}_{bsh}_{bs_name}_{bss}.log"
        self.log_file_path_qk_initial = f"{b0}/Initial_Quantized_{kernel_name}_{ksh}__{ks_name}__{kss}.log"
        self.log_file_path_qb_initial = f"{b0}/Initial_Quantized_{bias_name}_{bsh}_{bs_name}_{bss}.log"
        self.log_file_path_qk_initial_unique = f"{b0}/Unique_initial_quantized_{kernel_name}_{ksh}_{ks_name}_{kss}.log"
        self.log_file_path_qb_initial_unique = f"{b0}/Unique_initial_quantized_{bias_name}_{bsh}_{bs_name}_{bss}.log"

    # ---- statistics (device side)
    def stats(self):
        """{'unique_k', 'unique_b', 'max_k' (max|q| over axis 1), 'max_b'} -- custom_callbacks.py:84-129."""
        axis = 1 if self.param.dim() > 1 else 0
        b = self.layer.b.data
        return {
            "unique_k": int(ops.q_unique(self.param.data, self.k_scale.data)[0].numel()),
            "unique_b": int(ops.q_unique(b, self.b_scale.data)[0].numel()),
            "max_k": ops.q_absmax_over_axis(self.param.data, self.k_scale.data, axis).flatten().cpu(),
            # global max|q| of the bias (custom_callbacks.py:123): the same kernel, the bias viewed as (1, n, 1)
            "max_b": float(ops.q_absmax_over_axis(b.reshape(1, -1), self.b_scale.data.reshape(1, 1), 1)),
        }

    @staticmethod
    def _append(path, header, values):
        with open(path, "a") as f:
            if header is not None:
                f.write(header)
            for v in values:
                f.write(f"{v}\n")

    def on_epoch_end(self, epoch, logs=None):
        hdr = f"Epoch {epoch}\n"
        if self.dump_values:
            self._append(self.log_file_path_kernel, hdr, self.param.detach().flatten().cpu().numpy())
            self._append(self.log_file_path_biases, hdr, self.layer.b.detach().flatten().cpu().numpy())
        self._append(self.log_file_path_k_scale, hdr, self.k_scale.detach().flatten().cpu().numpy())
        self._append(self.log_file_path_b_scale, hdr, self.b_scale.detach().flatten().cpu().numpy())
        st = self.stats()
        self._append(self.log_file_path_qk_epoch, hdr, [st["unique_k"]])
        self._append(self.log_file_path_qk_epoch_max, hdr, st["max_k"].numpy())
        self._append(self.log_file_path_qb_epoch, hdr, [st["unique_b"]])
        self._append(self.log_file_path_qb_epoch_max, hdr, [st["max_b"]])
        return st

    def _dump_quantized(self, path_k, path_b, path_ku, path_bu):
        for param, scale, p_all, p_unique in ((self.param, self.k_scale, path_k, path_ku),
                                              (self.layer.b, self.b_scale, path_b, path_bu)):
            q = ops.quantized_integers(param.data, scale.data, torch.float32).flatten()
            self._append(p_all, None, q.cpu().numpy())
            u, c = ops.q_unique(param.data, scale.data)                 # HIP histogram, not a device sort
            with open(p_unique, "a") as f:
                for value, count in zip(u.cpu().numpy().astype("float32"), c.cpu().numpy()):
                    f.write(f"{value}, {count}\n")

    def on_train_end(self, logs=None):
        self._dump_quantized(self.log_file_path_qk, self.log_file_path_qb, self.log_file_path_qk_unique,
                             self.log_file_path_qb_unique)

    def on_train_begin(self, logs=None):
        self._dump_quantized(self.log_file_path_qk_initial, self.log_file_path_qb_initial,
                             self.log_file_path_qk_initial_unique, self.log_file_path_qb_initial_unique)


def group_sizes(param, scale, group_size) -> np.ndarray:
    """Elements per group of ``scale`` on ``param`` (int64, the scale's shape): the last group of a line may be short."""
    R, C, axis, gs = init_geometry(tuple(param.shape), param.stride(), tuple(scale.shape), group_size)
    length, lines = (R, C) if axis == 0 else (C, R)
    gs = min(gs, length)
    per_line = np.minimum(gs, length - gs * np.arange(-(-length // gs), dtype=np.int64))
    n = np.repeat(per_line[:, None], lines, axis=1) if axis == 0 else np.repeat(per_line[None, :], lines, axis=0)
    return n.reshape(tuple(scale.shape))


class _StatsTrackingCallback:
    """What the two statistics callbacks share: the layer's quantized tensors, the directories, the file table, one statistics
    launch per tensor with one device->host copy per call, the ``Epoch N`` + one-value-per-line appends and the histogram dump.
    A subclass supplies

      _STEMS                    (key, file name stem) of its per-epoch files after the scales and offsets, in the order written
      _refuse(name, q)          raises ValueError for a quantizer it does not log; called before any directory is made
      _device_stats(p, q)       the statistics record of one tensor, on the device
      _summary(rec, p, q)       the summary of a host record
      _rows(rec, st, n, q)      [(key, values)] that ``on_epoch_end`` appends; ``n``: float64 elements per group, flat
      _code_value(q)            code -> what the histogram dump prints for it"""

    def __init__(self, layer, log_dir):
        self.layer = layer
        if hasattr(layer, "kernel"):
            param, nested, kernel_name = layer.kernel, layer.nested_q_k_layer, f"Kernel_{layer.name}"
        else:
            param, nested, kernel_name = layer.W, layer.nested_q_w_layer, "Weights"
        bias_name = f"Bias_{layer.name}" if hasattr(layer, "kernel") else "Bias"
        self.tensors = [("kernel", kernel_name, param, nested)]
        if getattr(layer, "b", None) is not None and getattr(layer, "nested_q_b_layer", None) is not None:
            self.tensors.append(("bias", bias_name, layer.b, layer.nested_q_b_layer))
        for _, name, _, q in self.tensors:
            self._refuse(name, q)
        e, t, b0 = (os.path.join(log_dir, d) for d in ("on_epoch_end", "on_train_end", "on_train_begin"))
        for d in (e, t, b0):
            os.makedirs(d, exist_ok=True)
        self.paths, self.sizes = {}, {}
        for what, name, p, q in self.tensors:
            self.sizes[what] = group_sizes(p, q.scale, q.group_size)      # ValueError where the groups are not lines of a matrix
            psh, ssh = _shape(p), _shape(q.scale)
            self.paths[what] = {
                "scale": f"{e}/{name}_{psh}_{q.scale_name}_{ssh}.log",
                "offset": f"{e}/{name}_{psh}_Offset_{ssh}.log" if getattr(q, "asymmetric", False) else None,
                **{key: f"{e}/{stem}_{name}_{psh}.log" for key, stem in self._STEMS},
                "hist_begin": f"{b0}/Unique_initial_quantized_{name}_{psh}_{q.scale_name}_{ssh}.log",
                "hist_end": f"{t}/Unique_quantized_{name}_{psh}_{q.scale_name}_{ssh}.log",
            }

    def epoch_files(self):
        """Every file ``on_epoch_end`` appends to."""
        return [path for what, *_ in self.tensors for key, path in self.paths[what].items()
                if path is not None and not key.startswith("hist_")]

    def _records(self):
        """The host copies of every tensor's statistics, taken together."""
        return ops._stats_to_host([self._device_stats(p.data, q) for _, _, p, q in self.tensors])

    def stats(self):
        """{"kernel": summary, "bias": summary} of the tensors as they are now."""
        return {what: self._summary(rec, p, q) for (what, _, p, q), rec in zip(self.tensors, self._records())}

    _append = staticmethod(NestedScaleTrackingCallback._append)

    @staticmethod
    def _sqnr_rows(rec, st):
        return [("sqnr", [ops._sqnr_db(float(a), float(b)) for a, b in zip(rec.sig2.reshape(-1), rec.err2.reshape(-1))]),
                ("sqnr_tensor", [st["sqnr_db"]])]

    def on_epoch_end(self, epoch, logs=None):
        hdr = f"Epoch {epoch}\n"
        out = {}
        for (what, _, p, q), rec in zip(self.tensors, self._records()):
            st = out[what] = self._summary(rec, p, q)
            for key, values in self._rows(rec, st, self.sizes[what].reshape(-1).astype(np.float64), q):
                self._append(self.paths[what][key], hdr, values)
        return out

    def _dump_hist(self, key):
        for (what, _, _, q), rec in zip(self.tensors, self._records()):
            if rec.hist is None:
                continue
            value = self._code_value(q)
            with open(self.paths[what][key], "a") as f:
                for code, count in enumerate(rec.hist):
                    if count:
                        f.write(f"{value(code)}, {int(count)}\n")

    def on_train_end(self, logs=None):
        self._dump_hist("hist_end")

    def on_train_begin(self, logs=None):
        self._dump_hist("hist_begin")


class GroupQuantTrackingCallback(_StatsTrackingCallback):
    """Per-epoch logs of a layer whose quantizer has a range (``bits`` / ``q_range``), with any scale ops.group_stats takes:
    group-wise (symmetric or with offsets), scalar, a Dense orientation, channel-wise on OIHW storage.  Same directory layout
    and ``Epoch N`` + one-value-per-line format as ``NestedScaleTrackingCallback``.  For the kernel and the bias, per epoch end
    (group values in the scale's memory order):

      <name>_<shape>_<scale name>_<scale shape>.log    the scales          <name>_<shape>_Offset_<scale shape>.log   the offsets
      Clip_low_<name>_<shape>.log / Clip_high_...      share of each group's elements clipped below / above the range
      SQNR_dB_<name>_<shape>.log                       10 log10(sig2 / err2) of each group
      SQNR_dB_tensor_<name>_<shape>.log                the same of the whole tensor (one value per epoch)
      Used_levels_<name>_<shape>.log                   codes of the range that occur
      Code_entropy_bits_<name>_<shape>.log             Shannon entropy of the code distribution

    and on train begin / train end the code histogram as ``value, count`` lines (``Unique_initial_quantized_...`` /
    ``Unique_quantized_...``).  One lq_group_stats launch per tensor and one device->host copy per call.  ``stats()`` holds
    ops.summarize_stats of each tensor."""

    _STEMS = (("clip_low", "Clip_low"), ("clip_high", "Clip_high"), ("sqnr", "SQNR_dB"), ("sqnr_tensor", "SQNR_dB_tensor"),
              ("used", "Used_levels"), ("entropy", "Code_entropy_bits"))

    def _refuse(self, name, q):
        if q.q_range is None:
            raise ValueError(f"GroupQuantTrackingCallback: the quantizer of {name} has no range; use NestedScaleTrackingCallback")

    def _device_stats(self, p, q):
        return q.quant_stats(p, want_hist=q.q_range[1] - q.q_range[0] < ops.STATS_MAX_BINS)

    def _summary(self, rec, p, q):
        return ops._summarize_host(rec, p.numel())

    def _rows(self, rec, st, n, q):
        rows = [("scale", q.scale.detach().flatten().cpu().numpy())]
        if q.asymmetric:
            rows.append(("offset", q.offset.detach().flatten().cpu().numpy()))
        rows += [("clip_low", rec.below.reshape(-1) / n), ("clip_high", rec.above.reshape(-1) / n)] + self._sqnr_rows(rec, st)
        if rec.hist is not None:      # a range of more than ops.STATS_MAX_BINS codes has no histogram
            rows += [("used", [st["used_levels"]]), ("entropy", [st["entropy_bits"]])]
        return rows

    def _code_value(self, q):
        return lambda code: np.float32(q.q_range[0] + code)


class MxQuantTrackingCallback(_StatsTrackingCallback):
    """Per-epoch logs of a layer with an element format (the OCP microscaling quantizer), the counterpart of
    ``GroupQuantTrackingCallback``: same directory layout and ``Epoch N`` + one-value-per-line format.  For the kernel and the
    bias, per epoch end (group values in the scale's memory order):

      <name>_<shape>_<scale name>_<scale shape>.log    the stored scales
      Scale_exponent_<name>_<shape>.log                log2 of each group's effective scale (ops.mx_effective_scale; NaN: invalid)
      Sat_low_<name>_<shape>.log / Sat_high_...        share of each group's elements saturated below -max / above +max
      Flushed_<name>_<shape>.log                       share of each group's elements that are not zero and become zero
      SQNR_dB_<name>_<shape>.log                       10 log10(sig2 / err2) of each group
      SQNR_dB_tensor_<name>_<shape>.log                the same of the whole tensor (one value per epoch)
      Used_codes_<name>_<shape>.log                    encodings of the format that occur
      Code_entropy_bits_<name>_<shape>.log             Shannon entropy of the code distribution

    and on train begin / train end the code histogram as ``value, count`` lines in code order, the value from
    ops.mx_decode_table (``Unique_initial_quantized_...`` / ``Unique_quantized_...``).  One lq_mx_stats launch per tensor and one
    device->host copy per call.  ``stats()`` holds ops.summarize_mx_stats of each tensor."""

    _STEMS = (("exponent", "Scale_exponent"), ("sat_low", "Sat_low"), ("sat_high", "Sat_high"), ("flushed", "Flushed"),
              ("sqnr", "SQNR_dB"), ("sqnr_tensor", "SQNR_dB_tensor"), ("used", "Used_codes"), ("entropy", "Code_entropy_bits"))

    def _refuse(self, name, q):
        if getattr(q, "element_format", None) is None:
            raise ValueError(f"MxQuantTrackingCallback: the quantizer of {name} has no element format; use "
                             "GroupQuantTrackingCallback (a range) or NestedScaleTrackingCallback")

    def _device_stats(self, p, q):
        return q.mx_stats(p)

    def _summary(self, rec, p, q):
        return ops._summarize_mx_host(rec, p.numel(), q.element_format)

    def _rows(self, rec, st, n, q):
        stored = q.scale.detach().flatten().cpu().numpy()
        with np.errstate(all="ignore"):
            exponent = np.log2(ops.mx_effective_scale(stored, q.scale_format).astype(np.float64))
        return [("scale", stored), ("exponent", exponent), ("sat_low", rec.below.reshape(-1) / n), ("sat_high", rec.above.reshape(-1) / n),
                ("flushed", rec.flushed.reshape(-1) / n)] + self._sqnr_rows(rec, st) + [("used", [st["used_codes"]]),
                                                                                       ("entropy", [st["entropy_bits"]])]

    def _code_value(self, q):
        return ops.mx_decode_table(q.element_format).__getitem__      # -0.0 prints as such


class AccuracyLossTrackingCallBack:
    """custom_callbacks.py:211-237: train/val accuracy and loss, one value per epoch."""

    def __init__(self, log_dir, accuracy_file="accuracy.log", loss_file="loss.log"):
        os.makedirs(f"{log_dir}/accuracy", exist_ok=True)
        os.makedirs(f"{log_dir}/loss", exist_ok=True)
        self.accuracy_log_file_path = f"{log_dir}/accuracy/train_{accuracy_file}"
        self.val_accuracy_log_file_path = f"{log_dir}/accuracy/val_{accuracy_file}"
        self.loss_log_file_path = f"{log_dir}/loss/train_{loss_file}"
        self.val_loss_log_file_path = f"{log_dir}/loss/val_{loss_file}"

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        for path, key in ((self.val_accuracy_log_file_path, "val_accuracy"), (self.val_loss_log_file_path, "val_loss"),
                          (self.accuracy_log_file_path, "accuracy"), (self.loss_log_file_path, "loss")):
            with open(path, "a") as f:
                f.write(f"Epoch {epoch}\n")
                f.write(f"{logs.get(key)}\n")
