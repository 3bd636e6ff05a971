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


class GroupQuantTrackingCallback:
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
    ``Unique_quantized_...``).  One lq_group_stats launch per tensor and one device->host copy per call."""

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
        e, t, b0 = (os.path.join(log_dir, d) for d in ("on_epoch_end", "on_train_end", "on_train_begin"))
        for d in (e, t, b0):
            os.makedirs(d, exist_ok=True)
        self.paths, self.sizes = {}, {}
        for what, name, p, q in self.tensors:
            if q.q_range is None:
                raise ValueError(f"GroupQuantTrackingCallback: the quantizer of {name} has no range; use NestedScaleTrackingCallback")
            self.sizes[what] = group_sizes(p, q.scale, q.group_size)      # ValueError where the groups are not lines of a matrix
            psh, ssh = _shape(p), _shape(q.scale)
            self.paths[what] = {
                "scale": f"{e}/{name}_{psh}_{q.scale_name}_{ssh}.log",
                "offset": f"{e}/{name}_{psh}_Offset_{ssh}.log" if q.asymmetric else None,
                "clip_low": f"{e}/Clip_low_{name}_{psh}.log",
                "clip_high": f"{e}/Clip_high_{name}_{psh}.log",
                "sqnr": f"{e}/SQNR_dB_{name}_{psh}.log",
                "sqnr_tensor": f"{e}/SQNR_dB_tensor_{name}_{psh}.log",
                "used": f"{e}/Used_levels_{name}_{psh}.log",
                "entropy": f"{e}/Code_entropy_bits_{name}_{psh}.log",
                "hist_begin": f"{b0}/Unique_initial_quantized_{name}_{psh}_{q.scale_name}_{ssh}.log",
                "hist_end": f"{t}/Unique_quantized_{name}_{psh}_{q.scale_name}_{ssh}.log",
            }

    def epoch_files(self):
        """Every file ``on_epoch_end`` appends to."""
        keys = ("scale", "offset", "clip_low", "clip_high", "sqnr", "sqnr_tensor", "used", "entropy")
        return [self.paths[what][k] for what, *_ in self.tensors for k in keys if self.paths[what][k] is not None]

    def _records(self):
        """The host copies of every tensor's statistics, taken together."""
        return ops._stats_to_host([q.quant_stats(p.data, want_hist=q.q_range[1] - q.q_range[0] < ops.STATS_MAX_BINS)
                                   for _, _, p, q in self.tensors])

    def stats(self):
        """{"kernel": summary, "bias": summary}: ops.summarize_stats of the tensors as they are now."""
        return {what: ops._summarize_host(rec, p.numel()) for (what, _, p, _), rec in zip(self.tensors, self._records())}

    _append = staticmethod(NestedScaleTrackingCallback._append)

    def on_epoch_end(self, epoch, logs=None):
        hdr = f"Epoch {epoch}\n"
        out = {}
        for (what, _, p, q), rec in zip(self.tensors, self._records()):
            paths, n = self.paths[what], self.sizes[what].reshape(-1).astype(np.float64)
            st = ops._summarize_host(rec, p.numel())
            self._append(paths["scale"], hdr, q.scale.detach().flatten().cpu().numpy())
            if paths["offset"] is not None:
                self._append(paths["offset"], hdr, q.offset.detach().flatten().cpu().numpy())
            self._append(paths["clip_low"], hdr, rec.below.reshape(-1) / n)
            self._append(paths["clip_high"], hdr, rec.above.reshape(-1) / n)
            self._append(paths["sqnr"], hdr, [ops._sqnr_db(float(a), float(b)) for a, b in zip(rec.sig2.reshape(-1), rec.err2.reshape(-1))])
            self._append(paths["sqnr_tensor"], hdr, [st["sqnr_db"]])
            if rec.hist is not None:      # a range of more than ops.STATS_MAX_BINS codes has no histogram
                self._append(paths["used"], hdr, [st["used_levels"]])
                self._append(paths["entropy"], hdr, [st["entropy_bits"]])
            out[what] = st
        return out

    def _dump_hist(self, key):
        for (what, _, _, q), rec in zip(self.tensors, self._records()):
            if rec.hist is None:
                continue
            with open(self.paths[what][key], "a") as f:
                for code, count in enumerate(rec.hist):
                    if count:
                        f.write(f"{np.float32(q.q_range[0] + code)}, {int(count)}\n")

    def on_train_end(self, logs=None):
        self._dump_hist("hist_end")

    def on_train_begin(self, logs=None):
        self._dump_hist("hist_begin")


class MxQuantTrackingCallback:
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
    device->host copy per call."""

    _KEYS = ("scale", "exponent", "sat_low", "sat_high", "flushed", "sqnr", "sqnr_tensor", "used", "entropy")

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
        for _, name, _, q in self.tensors:      # before any directory is made
            if getattr(q, "element_format", None) is None:
                raise ValueError(f"MxQuantTrackingCallback: the quantizer of {name} has no element format; use "
                                 "GroupQuantTrackingCallback (a range) or NestedScaleTrackingCallback")
        e, t, b0 = (os.path.join(log_dir, d) for d in ("on_epoch_end", "on_train_end", "on_train_begin"))
        for d in (e, t, b0):
            os.makedirs(d, exist_ok=True)
        self.paths, self.sizes = {}, {}
        for what, name, p, q in self.tensors:
            self.sizes[what] = group_sizes(p, q.scale, q.group_size)
            psh, ssh = _shape(p), _shape(q.scale)
            self.paths[what] = {
                "scale": f"{e}/{name}_{psh}_{q.scale_name}_{ssh}.log",
                "exponent": f"{e}/Scale_exponent_{name}_{psh}.log",
                "sat_low": f"{e}/Sat_low_{name}_{psh}.log",
                "sat_high": f"{e}/Sat_high_{name}_{psh}.log",
                "flushed": f"{e}/Flushed_{name}_{psh}.log",
                "sqnr": f"{e}/SQNR_dB_{name}_{psh}.log",
                "sqnr_tensor": f"{e}/SQNR_dB_tensor_{name}_{psh}.log",
                "used": f"{e}/Used_codes_{name}_{psh}.log",
                "entropy": f"{e}/Code_entropy_bits_{name}_{psh}.log",
                "hist_begin": f"{b0}/Unique_initial_quantized_{name}_{psh}_{q.scale_name}_{ssh}.log",
                "hist_end": f"{t}/Unique_quantized_{name}_{psh}_{q.scale_name}_{ssh}.log",
            }

    def epoch_files(self):
        """Every file ``on_epoch_end`` appends to."""
        return [self.paths[what][k] for what, *_ in self.tensors for k in self._KEYS]

    def _records(self):
        """The host copies of every tensor's statistics, taken together."""
        return ops._stats_to_host([q.mx_stats(p.data) for _, _, p, q in self.tensors])

    def stats(self):
        """{"kernel": summary, "bias": summary}: ops.summarize_mx_stats of the tensors as they are now."""
        return {what: ops._summarize_mx_host(rec, p.numel(), q.element_format)
                for (what, _, p, q), rec in zip(self.tensors, self._records())}

    _append = staticmethod(NestedScaleTrackingCallback._append)

    def on_epoch_end(self, epoch, logs=None):
        hdr = f"Epoch {epoch}\n"
        out = {}
        for (what, _, p, q), rec in zip(self.tensors, self._records()):
            paths, n = self.paths[what], self.sizes[what].reshape(-1).astype(np.float64)
            st = ops._summarize_mx_host(rec, p.numel(), q.element_format)
            stored = q.scale.detach().flatten().cpu().numpy()
            with np.errstate(all="ignore"):
                exponent = np.log2(ops.mx_effective_scale(stored, q.scale_format).astype(np.float64))
            self._append(paths["scale"], hdr, stored)
            self._append(paths["exponent"], hdr, exponent)
            self._append(paths["sat_low"], hdr, rec.below.reshape(-1) / n)
            self._append(paths["sat_high"], hdr, rec.above.reshape(-1) / n)
            self._append(paths["flushed"], hdr, rec.flushed.reshape(-1) / n)
            self._append(paths["sqnr"], hdr, [ops._sqnr_db(float(a), float(b)) for a, b in zip(rec.sig2.reshape(-1), rec.err2.reshape(-1))])
            self._append(paths["sqnr_tensor"], hdr, [st["sqnr_db"]])
            self._append(paths["used"], hdr, [st["used_codes"]])
            self._append(paths["entropy"], hdr, [st["entropy_bits"]])
            out[what] = st
        return out

    def _dump_hist(self, key):
        for (what, _, _, q), rec in zip(self.tensors, self._records()):
            table = ops.mx_decode_table(q.element_format)
            with open(self.paths[what][key], "a") as f:
                for code, count in enumerate(rec.hist):
                    if count:
                        f.write(f"{table[code]}, {int(count)}\n")      # -0.0 prints as such

    def on_train_end(self, logs=None):
        self._dump_hist("hist_end")

    def on_train_begin(self, logs=None):
        self._dump_hist("hist_begin")


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
