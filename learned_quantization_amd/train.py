"""End-to-end training harness for the BASELINE configs (SURVEY f-3): the thin PyTorch counterpart of the
reference's ``experiment.py`` drivers, on synthetic data (no dataset is reachable offline).

  python -m learned_quantization_amd.train --config cifar --mode nq --value 1e-11 --orientation channelwise \
        --batch 256 --steps 50 --warmup 10 [--loss maxbin] [--ddp-mode A|B] [--seed 42]
  (N GPUs: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... -m learned_quantization_amd.train ...)

Mirrors (reference file:line under /root/reference):
  seeds, lr 1e-4 Adam, batch sizes       CIFAR-10/nested_quantization_layer/experiment.py:435-443, 550-572
  CL mode ``loss=obj.compute_total_loss``  CIFAR-10/custom_loss_terms/experiment.py:436-465
  regulariser terms added to the loss     custom_layers.py:327 (Keras ``add_weight(regularizer=...)``)
  constraint after the optimizer step     custom_layers.py:158

Per step: forward (custom layers -> K1), loss, backward (-> K2+K3 / K5 backward), one bucketed all-reduce
(DataParallel, RCCL) when world_size > 1, torch Adam on the ordinary parameters, ScaleAdam (K6: Adam +
MinValueConstraint in one launch) on the learned scales.  Prints one JSON line with images/s.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from typing import Optional

import torch
import torch.distributed as dist

from . import layers as L
from . import _hip
from .ddp import CaptureRefused, DataParallel, capture_with_agreement, control_group
from .losses import LossLog, SCCEDifference, SCCEInverse, SCCEMaxBin, sparse_categorical_crossentropy
from .models import INPUT_SHAPES, build_model, check_asymmetric_model, check_clip_mode, check_group_mode, check_mx_model
from .ops import (ELEMENT_FORMATS, LAYER_SCALE_INITS, MX_OPERAND_FORMATS, MX_SCALE_INITS, ROUNDINGS, SCALE_FORMATS, check_element_format, check_minmax_range,
                  check_rounding, check_scale_format, q_range_of)
from .optim import KerasAdam, ScaleAdam, non_scale_parameters, scale_parameters

LOSSES = {"maxbin": SCCEMaxBin, "difference": SCCEDifference, "inverse": SCCEInverse}


def synthetic_batch(config: str, batch: int, device, generator: Optional[torch.Generator] = None):
    """Images are raw 0..255 floats like the reference feeds them (experiment.py:512-513); uniform labels."""
    c, h, w = INPUT_SHAPES[config]
    x = torch.rand(batch, c, h, w, device=device, generator=generator) * 255.0
    y = torch.randint(0, 10, (batch,), device=device, generator=generator)
    return x, y


class Trainer:
    """One training configuration: model, loss, optimizers, optional multi-tensor batch, hipGraph and data-parallel wrapper.

    ``mode``: "nq" (nested quantization: ``value`` = penalty_threshold), "cl" (custom loss terms: ``value`` =
    penalty_rate, ``loss`` names the term), "nqcl" (BASELINE.json configs[3], "nested quantization + custom_loss_terms
    penalty": ``value`` = (penalty_threshold, penalty_rate); the scale gradient is the hand-written NQ gradient PLUS the
    penalty's -- an extension without a reference call site, the reference never combines the two: CL-L:61-62),
    "ste" (the straight-through scale gradient of ops.fq_scale_grad_ste, no loss term, ``value`` ignored) and "stecl" (the
    same plus a loss term: ``value`` = penalty_rate, ``loss`` names the term); ``grad_scale`` is their factor k, a float
    or "rsqrt_group".  ``bits`` (with ``signed``) or ``q_range`` (modes "cl", "ste", "stecl"; eager and graphed, per-tensor
    path, data-parallel mode "A") gives every quantised tensor the clipped quantizer with that integer range; with
    ``rounding="nearest"`` that quantizer rounds P/s to the nearest integer, ties to even, instead of down.  Both rules are linear
    in dy: data-parallel mode "A" (average ds over the ranks) already is the global-batch gradient, mode "B" is refused.

    A step is two phases: ``_backward_phase`` (zero the gradients, fake-quantise, forward, loss, backward, penalty
    injection) and ``_update_phase`` (exact-mode scale gradients, both optimizers); between them the data-parallel
    exchange.  ``graph=True`` records the phases into hipGraphs: one graph for the whole step on one GPU; with
    ``world_size > 1`` ONE graph that contains the RCCL all-reduce as well (RCCL kernels are capturable; the default on
    backend "nccl": 118.7 k against 109.6 k images/s for the CIFAR step on a one-rank communicator, profiles/r02_e2e.jsonl),
    or graph(backward) -> eager bucketed all-reduce -> graph(update) (``graph_collectives=False``, other backends, and the
    fallback when the capture of the collective fails).
    """

    def __init__(self, config="cifar", mode="nq", value=1e-11, orientation="channelwise", loss: Optional[str] = None,
                 lr=1e-4, seed=42, device=None, ddp_mode="A", log_dir="logs", graph=False, batched=False,
                 bucket_mb: float = 25.0, overlap: bool = True, graph_collectives: Optional[bool] = None,
                 force_collectives: bool = False, kernel_storage: str = "oihw", loss_values: bool = False,
                 loss_log_capacity: int = 4096, grad_scale=None, bits=None, signed=True, q_range=None, rounding="floor",
                 clipped_batch: bool = False, group_size=None, group_batch: bool = False, scale_init=None, asymmetric: bool = False,
                 asymmetric_batch: bool = False, element_format=None, scale_format="e8m0", mx_batch: bool = False):
        """``element_format`` (one of ops.ELEMENT_FORMATS; mode "ste"; eager, graphed and data-parallel mode "A"; per-tensor path
        unless ``mx_batch``) with ``scale_format`` ("e8m0", the default, or "fp32"): the OCP microscaling quantizer for every quantised tensor
        (models.build_model): kernels in blocks of ``group_size`` (32 by default), biases as one group.  It takes no range,
        rounding or offsets, and no batch but the one ``mx_batch`` asks for; ``scale_init`` is "mx" (the OCP rule) or "cover" (nothing saturates).
        ``mx_batch`` (opt-in, with ``element_format``, ``group_batch`` and ``batched``; eager, graphed, data-parallel mode "A"):
        the microscaling kernels and their biases run in the group batch (``FakeQuantBatch(group_batch=True, mx=True)``): one
        forward and one backward launch for the whole model, results those of the per-tensor path bit for bit, and one launch
        steps every scale.  ``group_size`` may be left at the microscaling default of 32.
        ``asymmetric`` (with ``group_size``, a range and mode "ste"; eager, graphed and data-parallel mode "A"; per-tensor path
        unless ``asymmetric_batch``): every group-wise kernel also learns an offset per group (models.build_model); the offsets
        are stepped by the scales' optimizer, without a lower bound.  ``scale_init="minmax"`` exists for such models only.
        ``asymmetric_batch`` (opt-in, with ``asymmetric``, ``group_batch`` and ``batched``; eager, graphed, data-parallel mode
        "A"): the group batch also carries the offsets (``FakeQuantBatch(group_batch=True, asymmetric=True)``): still one forward
        and one backward launch for the whole model, the backward writes every offset's gradient too (into the data-parallel
        bucket's views where there is one), and scales and offsets are stepped by one launch.
        ``scale_init`` ("absmax" / "lsq" / "mse"; with ``bits`` / ``q_range``): every scale starts from its layer's weights
        (layers.init_scales) instead of the library's initial value, at which a range clips every weight.  It runs once, on the
        device, after the weights are in place and before the optimizers, the batch, the graph and the data-parallel wrapper are
        built: the scales are written in place, and the wrapper's initial broadcast carries them to every rank.
        ``group_size`` (with ``bits`` / ``q_range`` and mode "ste"; eager, graphed and data-parallel mode "A"): group-wise scales
        for every quantised kernel (models.build_model); it replaces ``orientation``.
        ``group_batch`` (opt-in, with ``batched=True`` and ``group_size``; mode "ste", eager, graphed, data-parallel mode "A"): the
        group-wise kernels and their biases run in the group batch (``FakeQuantBatch(group_batch=True)``: one forward launch and
        one backward launch for the whole model, results those of the per-tensor path bit for bit for the kernels).
        ``clipped_batch`` (opt-in, with ``batched=True`` and a range): the clipped layers run in the multi-tensor batch
        (``FakeQuantBatch(clipped=True)``: one forward launch, two backward launches; the batch owns one dP buffer per tensor
        and its backward moves 12 bytes per element instead of 8).  Everything else about a range stays: modes "cl", "ste",
        "stecl", data-parallel mode "A".
        ``loss_values`` (modes with a loss term): the step also EVALUATES the penalty -- batched: as a by-product of the
        gradient injection (lq_batch_penalty_grads_values); per-tensor path: the loss object's own device scalar -- appends the
        reference's three per-step numbers (CL-F:58-71) to a device-side ``LossLog`` (no synchronisation, capturable) and
        ``step()`` / ``step_graphed()`` return ``mean(SCCE) (+ regularisers) + rate * penalty``.  ``loss_terms`` is a
        persistent device tensor of the trainer, ``[total, scce, rate * penalty]`` of the latest step with the regularisers
        in ``total`` in both forms (the log's rows never hold them: Keras adds them outside ``compute_total_loss``).  Batched,
        the returned loss IS ``loss_terms[0]``: one buffer, rewritten by every step -- ``clone()`` it to keep the losses of
        several steps (the per-tensor path returns the differentiated scalar, a fresh tensor every step).
        ``flush_loss_log()`` writes the files."""
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        torch.manual_seed(seed)
        L.reset_layer_names()
        self.config = config
        self.mode = mode
        ste = mode in ("ste", "stecl")
        self.group_size = group_size
        self.asymmetric = bool(asymmetric)
        self.element_format, self.scale_format = element_format, (scale_format if element_format is not None else None)
        if element_format is not None:
            check_element_format(element_format)
            check_scale_format(scale_format)
            check_mx_model(mode, bits, signed, q_range, rounding, asymmetric, kernel_storage, scale_init)
            if mx_batch and not (group_batch and batched):
                raise ValueError("mx_batch=True belongs to element_format, group_batch=True and batched=True: it lets the group batch "
                                 "carry the element formats of a microscaling model")
            if mx_batch and (clipped_batch or asymmetric_batch):
                raise ValueError("mx_batch=True with clipped_batch / asymmetric_batch: a microscaling model runs in the group batch "
                                 "alone (batched=True, group_batch=True, mx_batch=True)")
            if (batched or clipped_batch or group_batch or asymmetric_batch) and not mx_batch:
                raise ValueError("element_format with batched=True: none of the multi-tensor batches (default, clipped, group) carries "
                                 "a minifloat grid; a model with an element format runs on the per-tensor path")
            if ddp_mode == "B":
                raise ValueError("element_format with ddp_mode 'B': it recomputes ds from the all-reduced dP, which no longer holds "
                                 "the dy of the saturated elements; use ddp_mode 'A'")
        elif mx_batch:
            raise ValueError("mx_batch=True belongs to element_format, group_batch=True and batched=True: a model without an element "
                             "format has no microscaling layer to batch")
        elif scale_init in MX_SCALE_INITS:
            raise ValueError(f"scale_init {scale_init!r} on a model without an element format: it writes the power-of-two scale of a "
                             "microscaling block")
        if asymmetric:
            check_asymmetric_model(mode, bits is not None or q_range is not None, group_size, kernel_storage)
            if batched and not asymmetric_batch:
                raise ValueError("asymmetric=True with batched=True: the multi-tensor batches carry no offset per group unless asked "
                                 "to; asymmetric layers run on the per-tensor path, or opt in to offsets in the group batch "
                                 "(group_batch=True, asymmetric_batch=True / --group-batch --asymmetric-batch)")
            if ddp_mode == "B":
                raise ValueError("asymmetric=True with ddp_mode 'B': it recomputes ds from the all-reduced dP, which no longer holds "
                                 "the dy of the clipped elements -- the very elements the offset's gradient sums; use ddp_mode 'A'")
        if asymmetric_batch and not (asymmetric and group_batch and batched):
            raise ValueError("asymmetric_batch=True belongs to asymmetric=True, group_batch=True and batched=True: it lets the group "
                             "batch carry the offsets of an asymmetric model")
        self.asymmetric_batch = bool(asymmetric_batch)
        self.mx_batch = bool(mx_batch)
        if scale_init == "minmax":
            if not asymmetric:
                raise ValueError('scale_init "minmax" on a symmetric model: it places each group\'s range over [min, max] through an '
                                 "offset, which only asymmetric=True layers have")
            check_minmax_range(*q_range_of(bits, signed, q_range))
        if group_size is not None and element_format is None:
            check_group_mode(mode, bits is not None or q_range is not None)
            if batched and (not group_batch or clipped_batch):
                raise ValueError("group_size with batched=True: the multi-tensor batch describes every tensor by one-axis "
                                 "(outer, G, inner) scales; group-wise scales run on the per-tensor path, or opt in to the group "
                                 "batch (group_batch=True / --group-batch, without clipped_batch)")
            if ddp_mode == "B":
                raise ValueError("group_size with ddp_mode 'B': it recomputes ds from the all-reduced dP, which no longer holds the "
                                 "dy of the clipped elements; use ddp_mode 'A'")
        if ste and ddp_mode == "B":
            raise ValueError(f"mode {mode!r} with ddp_mode 'B': the straight-through scale gradient is linear in dy, so averaging ds "
                             "over the ranks (ddp_mode 'A') already is the global-batch gradient; there is nothing to recompute")
        if grad_scale is not None and not ste:
            raise ValueError("grad_scale belongs to the modes 'ste' and 'stecl'")
        # ``bits`` / ``signed`` or ``q_range``: the clipped quantizer for every quantised tensor (layers.py), per-tensor path
        self.q_range = q_range_of(bits, signed, q_range)
        check_rounding(rounding, self.q_range is not None)
        self.rounding = rounding
        if self.q_range is not None:
            check_clip_mode(mode)
            if ddp_mode == "B":
                raise ValueError("bits / q_range with ddp_mode 'B': it recomputes ds from the all-reduced dP, which no longer holds "
                                 "the dy of the clipped elements; use ddp_mode 'A'")
            if batched and not clipped_batch and not group_batch:
                raise ValueError("bits / q_range with batched=True: the multi-tensor backward hands dy on as dP, but a clipped "
                                 "layer's dP is a masked copy of dy; use the per-tensor path, or opt in to the clipped batch "
                                 "(clipped_batch=True / --clipped-batch), which owns a dP buffer per tensor")
        if clipped_batch and not batched:
            raise ValueError("clipped_batch=True belongs to batched=True")
        if clipped_batch and self.q_range is None:
            raise ValueError("clipped_batch=True needs bits / q_range: an unclipped model runs the default batch")
        if group_batch and not batched:
            raise ValueError("group_batch=True belongs to batched=True")
        if group_batch and group_size is None and not mx_batch:      # a microscaling model has its own default group size
            raise ValueError("group_batch=True needs group_size: a model of one-axis scales runs the default or the clipped batch")
        self.clipped_batch = bool(clipped_batch)
        self.group_batch = bool(group_batch)
        # conv kernels shaped HWIO like the reference's, stored in the order MIOpen consumes (layers.py kernel_storage): the
        # fake-quantised kernel goes to the convolution as written and its weight gradient is dP
        self.model = build_model(config, mode=mode, value=value, seed=seed, orientation=orientation, device=self.device,
                                 kernel_storage=kernel_storage, grad_scale=grad_scale, q_range=self.q_range, rounding=rounding,
                                 group_size=group_size, asymmetric=self.asymmetric, element_format=element_format,
                                 scale_format=scale_format)
        self.model.to(self.device)
        self.scale_init = scale_init
        if scale_init is not None:
            if self.q_range is None and element_format is None:
                raise ValueError("scale_init needs bits / q_range: the unbounded quantizer clips nothing, there is no range to cover")
            L.init_scales(self.model, scale_init)
        self.custom_layers = L.custom_layers_of(self.model)
        self.loss_obj = None
        self.loss_kind = loss
        self.penalty_rate = value[1] if mode == "nqcl" else value
        if mode in ("cl", "nqcl", "stecl"):
            if loss not in LOSSES:
                raise ValueError(f"mode {mode!r} needs --loss maxbin|difference|inverse")
            self.loss_obj = LOSSES[loss](self.custom_layers, self.penalty_rate, log_dir)   # custom_loss_terms/experiment.py:436-455
        elif loss is not None:
            raise ValueError("a loss term needs mode 'cl', 'nqcl' or 'stecl'")
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        use_dp = self.world > 1 or (force_collectives and dist.is_initialized())
        # Exact mode B reads the all-reduced P.grad as the global-batch dy (custom_layers.py:118): everything else that has a
        # gradient with respect to P or s -- the loss term of "nqcl", weight regularisers -- is applied AFTER the scale
        # gradients were recomputed (it is a function of the parameters only, identical on every rank: no exchange needed).
        self._after_exchange = use_dp and ddp_mode == "B"
        if self._after_exchange and mode == "nqcl" and not batched:
            raise ValueError("mode 'nqcl' with ddp_mode 'B' needs batched=True: the loss term's gradients are injected after the "
                             "exact scale gradients were recomputed, which the per-tensor autograd path cannot order")
        # graphed steps exchange after backward (hooks cannot launch collectives from inside a capture that is replayed
        # without them): overlap is a property of the eager step
        self.dp = DataParallel(self.model, mode=ddp_mode, bucket_mb=bucket_mb, overlap=overlap and not graph,
                               force_collectives=force_collectives) if use_dp else None
        # Keras 2.11 Adam (lr 1e-4, eps 1e-7 outside the bias correction) for every ordinary parameter in one launch
        self.opt = KerasAdam(non_scale_parameters(self.model), lr=lr, eps=1e-7, capturable=graph)
        self.batch = None
        if batched:
            # one launch for every fake-quant forward, two for every scale gradient, one for every scale update
            from .batch import BatchedScaleAdam, FakeQuantBatch
            if self.dp is not None:
                self.dp.zero_grad()          # makes scale.grad the bucket views the batch will write into
            # the convolutions consume the OIHW companions only; autograd=False: the fake-quantised tensors are leaves and
            # _backward_phase calls finish_backward() itself (0.4-0.6 ms less autograd-engine work per eager step for 40 tensors)
            self.batch = FakeQuantBatch(self.model, lr=lr, hwio_out=False, autograd=False, clipped=self.clipped_batch,
                                        group_batch=self.group_batch, asymmetric=self.asymmetric_batch, mx=self.mx_batch)
            # nothing touches ds between its computation and the scales' update when there is no loss term and ds is not
            # exchanged (one process, or exact mode B): the finalize then applies the Adam step itself (one launch fewer)
            # (the fused finalize + Adam is the nested-quantization pass's: not for the straight-through modes, nor for a kind of
            # batch that cannot fuse)
            fused = self.loss_obj is None and (self.dp is None or ddp_mode == "B") and not ste and self.batch._kind.fuses
            self.scale_opt = BatchedScaleAdam(self.batch, capturable=graph, fused=fused)
            if self.dp is not None:
                self.dp.attach_batch(self.batch)
        else:
            self.scale_opt = ScaleAdam(scale_parameters(self.model), lr=lr, capturable=graph)
        self.regularized = [l for l in self.custom_layers if l.regularizer is not None]
        self.loss_values = bool(loss_values)
        if self.loss_values and self.loss_obj is None:
            raise ValueError("loss_values=True needs a loss term (mode 'cl' or 'nqcl')")
        self.loss_log = LossLog(self.loss_obj, loss_log_capacity, self.device) if self.loss_values else None
        # [total, scce, rate * penalty] of the latest step, regularisers in the total (persistent: a captured graph rewrites it)
        self.loss_terms = torch.zeros(3, dtype=torch.float32, device=self.device) if self.loss_values else None
        self._scce = self._task = None       # this step's mean(SCCE) and mean(SCCE) + regularisers (batched form)
        self.graph = None
        self.graph_update = None
        if graph_collectives is None:          # default: capture the collective where the backend can be captured
            graph_collectives = bool(use_dp and dist.get_backend() == "nccl")
        self.graph_collectives = graph_collectives
        # host-side agreement on capture outcomes (collective creation: every rank builds its Trainer at the same point)
        self._control = control_group() if (use_dp and graph and graph_collectives) else None
        self.graph_note = None
        self._want_graph = graph

    def loss(self, y, p):
        if self.loss_obj is not None and self.batch is None:
            if self.loss_values:
                # compute_total_loss (CL-F:47-58) with its two ingredients kept: they are the log's row
                cross_entropy_loss = sparse_categorical_crossentropy(y, p)
                penalty = self.loss_obj._penalty()
                per_sample = cross_entropy_loss + self.loss_obj.penalty_rate * penalty
                self._row = self.loss_log.append(cross_entropy_loss.detach().mean(), penalty.detach())
            else:
                per_sample = self.loss_obj.compute_total_loss(y, p)
        else:
            per_sample = sparse_categorical_crossentropy(y, p)
        total = per_sample.mean()
        if self.loss_values and self.batch is not None:
            self._scce = total.detach()
        total = self._with_regularizers(total)
        if self.loss_values and self.batch is not None:
            self._task = total.detach()
        elif self.loss_values:
            self.loss_terms.copy_(self._row)
            self.loss_terms[0].copy_(total.detach())      # the differentiated scalar: regularisers included
        return total

    def _with_regularizers(self, total):
        """Keras adds the regulariser losses to the objective (custom_layers.py:327).  Exact mode B: their VALUE is added here,
        their gradients follow in ``_update_phase``, after the scale gradients were recomputed from the pure task-loss P.grad."""
        for layer in self.regularized:
            r = layer.regularization_loss()
            total = total + (r.detach() if self._after_exchange else r)
        return total

    def _objective(self, x, y):
        """The scalar that is differentiated: task loss of the model's output (+ loss term, + regularisers)."""
        return self.loss(y, self.model(x))

    # ---------------------------------------------------------------- the two phases of a step
    def _backward_phase(self, x, y):
        self.model.train()
        if self.dp is not None:
            self.dp.zero_grad()
        else:
            self.opt.zero_grad(set_to_none=True)
            self.scale_opt.zero_grad(set_to_none=True)
        if self.batch is not None:
            self.batch.quantize_all()
        loss = self._objective(x, y)
        loss.backward()
        if self.batch is not None:
            self.batch.finish_backward()         # scale-gradient launches; dP = dy to every quantised parameter
        if self.batch is not None and self.loss_obj is not None and not self._after_exchange:
            self._inject_penalty()
        return loss

    def _inject_penalty(self):
        # batched custom-loss-terms mode: the task loss went through autograd, the penalty gradients are injected
        # by the batch kernels (identical on every rank, so adding them before the all-reduce changes nothing);
        # "nqcl" / "stecl": the penalty's ds is ADDED to the op's own ds the batch has just written
        penalty = self.batch.inject_penalty_grads(self.loss_kind, self.penalty_rate, accumulate_ds=(self.mode in ("nqcl", "stecl")),
                                                  values=self.loss_values)
        if self.loss_values:
            # the log's row is the reference's three numbers (CL-F:58-71); Keras adds the regularisers outside
            # compute_total_loss: they are in the returned total, not in the log
            self.loss_terms.copy_(self.loss_log.append(self._scce, penalty))
            if self.regularized:
                self.loss_terms[0].copy_(self._task + self.loss_terms[2])

    def _returned_loss(self, loss):
        """What ``step()`` hands back: the differentiated scalar, or -- batched with ``loss_values`` -- the total read from
        ``loss_terms`` (the penalty never went through autograd there)."""
        if self.loss_values and self.batch is not None:
            return self.loss_terms[0]
        return loss

    def flush_loss_log(self):
        """Writes the rows collected since the last flush to ``custom_losses/*.log``; ``(rows_written, rows_dropped)``."""
        if self.loss_log is None:
            raise RuntimeError("flush_loss_log() needs Trainer(loss_values=True)")
        return self.loss_log.flush()

    def _update_phase(self):
        if self.dp is not None:
            self.dp.recompute_scale_grads()          # mode B only: ds from the pure task-loss P.grad
        if self._after_exchange:
            if self.batch is not None and self.loss_obj is not None:
                self._inject_penalty()
            if self.regularized:
                with self.dp.no_sync():              # a second backward into the exchanged bucket, on purpose
                    reg = self.regularized[0].regularization_loss()
                    for layer in self.regularized[1:]:
                        reg = reg + layer.regularization_loss()
                    reg.backward()
        self.opt.step()
        self.scale_opt.step()

    def step(self, x, y):
        """One training step; returns the loss as a 0-dim device tensor.  With ``loss_values=True`` and ``batched=True`` that is
        ``loss_terms[0]``, a view of one persistent buffer that the next step overwrites (``clone()`` to keep it)."""
        loss = self._backward_phase(x, y)
        if self.dp is not None:
            self.dp.exchange()
        self._update_phase()
        return self._returned_loss(loss)

    def _capture(self, fn):
        g = torch.cuda.CUDAGraph()
        # with a process group alive its watchdog THREAD polls events while this thread captures: "thread_local" keeps
        # that legal (the default "global" mode makes every other thread's HIP call an error during the capture)
        mode = "thread_local" if self.dp is not None else "global"
        with torch.cuda.graph(g, capture_error_mode=mode):
            out = fn()
        return g, out

    def _capture_whole_step(self) -> bool:
        """ONE graph: backward phase, RCCL all-reduce (synchronous collectives on the capturing stream), update phase.
        The outcome is AGREED ON by all ranks (ddp.capture_with_agreement, over the gloo control group): True when every rank
        captured; False -- on every rank, with the trainer left ready for the split form -- when the stack refused to record the
        collective on at least one of them (an error raised while the exchange was being recorded, or when the capture was
        closed) and the communicator still answers an eager all-reduce afterwards.  Errors of the step itself (argument
        validation, shapes: anything raised in the backward or update phase, any ``LQError``) are re-raised, on every rank."""
        phase = ["backward"]

        def whole():
            loss = self._backward_phase(self._x, self._y)
            phase[0] = "exchange"
            self.dp.exchange(capture_safe=True)
            phase[0] = "update"
            self._update_phase()
            phase[0] = "end"                 # what is raised from here on comes from closing the capture
            return self._returned_loss(loss)

        def attempt():
            try:
                self.graph, self._loss = self._capture(whole)
            except _hip.LQError:
                raise
            except RuntimeError as e:
                if phase[0] in ("exchange", "end"):
                    raise CaptureRefused(f"{e!r}"[:300]) from e
                raise

        try:
            ok = capture_with_agreement(attempt, self._control, health_check=self.dp.health_check)
        except BaseException:
            self.graph = None
            raise
        if ok:
            return True
        self.graph = None
        self.graph_collectives = False
        self.graph_note = "the collective could not be captured on every rank: graph / eager all-reduce / graph"
        torch.cuda.synchronize(self.device)
        self.dp.begin_step()                 # arrival counters of the hooks that ran during the abandoned capture
        if hasattr(self.scale_opt, "_applied"):
            self.scale_opt._applied = False  # the fused scale update was recorded, not executed
        return False

    def step_graphed(self, x, y):
        """The training step as hipGraph launches.  These steps are launch-bound (hundreds of small kernels); capture
        removes the host from the loop.  First call: 3 eager warm-up steps on a side stream, then capture.
        One GPU: ONE graph (forward, loss, backward, both optimizers).  Data parallel: graph(backward phase) -> eager
        bucketed RCCL all-reduce -> graph(update phase); or, with ``graph_collectives``, one graph including the
        all-reduce (synchronous collectives on the capturing stream)."""
        if self.graph is None:
            self._x = torch.empty_like(x)
            self._y = torch.empty_like(y)
            self._x.copy_(x)
            self._y.copy_(y)
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                for _ in range(3):
                    self.step(self._x, self._y)
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            if self.dp is None:
                self.opt.zero_grad(set_to_none=True)
                self.scale_opt.zero_grad(set_to_none=True)
                self.graph, self._loss = self._capture(lambda: self.step(self._x, self._y))
            elif self.graph_collectives and self._capture_whole_step():
                pass
            else:
                self.graph, self._loss = self._capture(lambda: self._backward_phase(self._x, self._y))
                self.dp.exchange()
                self.graph_update, _ = self._capture(self._update_phase)
                self._loss = self._returned_loss(self._loss)      # mode B evaluates the penalty in the update phase
        self._x.copy_(x)
        self._y.copy_(y)
        if self.dp is not None:
            self.dp.begin_step()
        self.graph.replay()
        if self.graph_update is not None:
            self.dp.exchange()
            self.graph_update.replay()
        return self._loss

    @torch.no_grad()
    def evaluate(self, x, y, with_penalty: bool = False):
        """``with_penalty``: add ``rate * penalty`` to the validation loss, as Keras' ``val_loss`` of a model compiled with
        ``loss=obj.compute_total_loss`` does (CL-F:47-58)."""
        self.model.eval()
        p = self.model(x)
        loss = sparse_categorical_crossentropy(y, p).mean()
        if with_penalty:
            if self.loss_obj is None:
                raise ValueError("evaluate(with_penalty=True) needs a loss term (mode 'cl' or 'nqcl')")
            penalty = self.batch.penalty_values(self.loss_kind)[1] if self.batch is not None else self.loss_obj._penalty()
            loss = loss + self.penalty_rate * penalty
        return float(loss), float((p.argmax(1) == y).float().mean())


class DriverParser(argparse.ArgumentParser):
    """Argument parser of both drivers: what the flags refuse in combination is refused here, as a usage error, before any device
    is touched -- ``--scale-init minmax`` belongs to ``--asymmetric``, which belongs to ``--group-size``; ``--asymmetric-batch``
    belongs to ``--asymmetric``, ``--group-batch`` and ``--batched``; ``--mx-batch`` belongs to ``--element-format``,
    ``--group-batch`` and ``--batched``, and is the only way an element format meets ``--batched``."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if getattr(ns, "asymmetric", False) and getattr(ns, "group_size", None) is None:
            self.error("--asymmetric needs --group-size: offsets exist per group (a group size of the line length or more gives "
                       "per-channel offsets)")
        if getattr(ns, "asymmetric_batch", False) and not (getattr(ns, "asymmetric", False) and getattr(ns, "group_batch", False)
                                                           and getattr(ns, "batched", False)):
            self.error("--asymmetric-batch needs --asymmetric, --group-batch and --batched: it lets the group batch carry the "
                       "offsets of an asymmetric model")
        mx_batch = getattr(ns, "mx_batch", False)
        if mx_batch and not (getattr(ns, "element_format", None) is not None and getattr(ns, "group_batch", False)
                             and getattr(ns, "batched", False)):
            self.error("--mx-batch needs --element-format, --group-batch and --batched: it lets the group batch carry the element "
                       "formats of a microscaling model")
        if mx_batch and (getattr(ns, "clipped_batch", False) or getattr(ns, "asymmetric_batch", False)):
            self.error("--mx-batch with --clipped-batch / --asymmetric-batch: a microscaling model runs in the group batch alone")
        if getattr(ns, "element_format", None) is None:
            if getattr(ns, "scale_init", None) in MX_SCALE_INITS:
                self.error("--scale-init mx / cover needs --element-format: it writes the power-of-two scale of a microscaling block")
            if getattr(ns, "scale_format", None) is not None:
                self.error("--scale-format needs --element-format")
        else:
            for flag, bad in (("--bits", getattr(ns, "bits", None) is not None), ("--unsigned", getattr(ns, "unsigned", False)),
                              ("--rounding", getattr(ns, "rounding", "floor") != "floor"), ("--asymmetric", getattr(ns, "asymmetric", False)),
                              ("--batched", getattr(ns, "batched", False) and not mx_batch)):
                if bad:
                    self.error(f"--element-format with {flag}: an element format brings its own grid, range and rounding, has no "
                               "offsets and runs on the per-tensor path")
            if getattr(ns, "scale_init", None) not in (None,) + MX_SCALE_INITS:
                self.error("--element-format takes --scale-init mx or cover: a microscaling scale is a power of two")
        if getattr(ns, "scale_init", None) == "minmax" and not getattr(ns, "asymmetric", False):
            self.error("--scale-init minmax needs --asymmetric: it places each group's range over [min, max] through an offset, "
                       "which a symmetric layer does not have")
        return ns


def build_parser():
    ap = DriverParser()
    ap.add_argument("--config", choices=list(INPUT_SHAPES), default="cifar")
    ap.add_argument("--mode", choices=["nq", "cl", "nqcl", "ste", "stecl"], default="nq")
    ap.add_argument("--value", type=float, default=1e-11, help="penalty_threshold (nq, nqcl) or penalty_rate (cl, stecl); ignored by ste")
    ap.add_argument("--grad-scale", default=None,
                    help="modes ste / stecl: factor of the straight-through scale gradient, a float or 'rsqrt_group' (default 1)")
    ap.add_argument("--bits", type=int, default=None,
                    help="modes cl / ste / stecl: clipped b-bit quantizer, integers in [-2^(b-1), 2^(b-1) - 1] (1 <= b <= 24)")
    ap.add_argument("--unsigned", action="store_true", help="with --bits: integers in [0, 2^b - 1]")
    ap.add_argument("--rounding", default="floor", choices=list(ROUNDINGS),
                    help="with --bits: round P/s down (the reference's floor) or to nearest, ties to even")
    ap.add_argument("--group-size", type=int, default=None,
                    help="with --bits and mode ste: group-wise scales, one per N consecutive inputs of each output unit (replaces "
                         "--orientation; biases keep a scalar scale)")
    ap.add_argument("--asymmetric", action="store_true",
                    help="with --bits, --group-size and mode ste: every group-wise kernel also learns an offset per group (per-tensor "
                         "path unless --asymmetric-batch; biases stay symmetric)")
    ap.add_argument("--element-format", default=None, choices=list(ELEMENT_FORMATS),
                    help="mode ste: OCP microscaling quantizer, elements on this minifloat grid under one scale per block of "
                         "--group-size elements (default 32); replaces --orientation, --bits and --rounding; biases are one block")
    ap.add_argument("--scale-format", default=None, choices=list(SCALE_FORMATS),
                    help="with --element-format: e8m0 (default; the scale is rounded to a power of two) or fp32")
    ap.add_argument("--scale-init", default=None, choices=list(LAYER_SCALE_INITS + MX_SCALE_INITS),
                    help="with --bits: start every scale from its weights (absmax: nothing clipped; lsq: 2 mean|w| / sqrt(Qp); mse: "
                         "least squared error below absmax; minmax, with --asymmetric only: scale and offset from each group's "
                         "minimum and maximum) instead of the library's initial value, which clips every weight")
    ap.add_argument("--rate", type=float, default=1e-7, help="penalty_rate of the loss term in mode nqcl")
    ap.add_argument("--value-coarse", type=float, default=None,
                    help="resnet50 only: threshold of the 3x3 kernels ('mixed' quantisation intensity); --value is the rest")
    ap.add_argument("--orientation", default="channelwise")
    ap.add_argument("--loss", choices=list(LOSSES), default=None)
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--ddp-mode", choices=["A", "B"], default="A")
    ap.add_argument("--export-dir", default=None, help="write the reference's integer export here at the end")
    ap.add_argument("--graph", action="store_true", help="replay the step from hipGraphs (N > 1: graph / all-reduce / graph)")
    ap.add_argument("--graph-collectives", dest="graph_collectives", action="store_true", default=None,
                    help="N > 1: capture the RCCL all-reduce inside ONE graph (the default on backend nccl)")
    ap.add_argument("--no-graph-collectives", dest="graph_collectives", action="store_false",
                    help="N > 1: graph(backward) -> eager bucketed all-reduce -> graph(update)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed and run the collectives even with one rank (RCCL rehearsal on one GPU)")
    ap.add_argument("--bucket-mb", type=float, default=25.0)
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL over xGMI (default); gloo + --share-gpu rehearses N>1 on one GPU")
    ap.add_argument("--share-gpu", action="store_true", help="rehearsal only: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--batched", action="store_true", help="multi-tensor launches for all fake-quant ops of a step (lq_batch_*)")
    ap.add_argument("--clipped-batch", action="store_true",
                    help="with --batched and --bits: run the clipped layers in the multi-tensor batch (opt-in: it owns a dP buffer per "
                         "tensor and its backward moves 12 bytes per element instead of 8)")
    ap.add_argument("--group-batch", action="store_true",
                    help="with --batched, --bits and --group-size: run the group-wise layers and their biases in the group batch "
                         "(opt-in: one forward and one backward launch for the whole model)")
    ap.add_argument("--asymmetric-batch", action="store_true",
                    help="with --asymmetric, --batched and --group-batch: the group batch also carries the offsets (opt-in: still one "
                         "forward and one backward launch, which writes the offsets' gradients too)")
    ap.add_argument("--mx-batch", action="store_true",
                    help="with --element-format, --batched and --group-batch: run the microscaling layers and their biases in the "
                         "group batch (opt-in: one forward and one backward launch for the whole model, formats per tensor)")
    ap.add_argument("--loss-values", action="store_true",
                    help="modes cl / nqcl: evaluate the penalty with its gradients, report mean(SCCE) + rate * penalty and keep the "
                         "reference's per-step loss logs in a device buffer (written at the end)")
    ap.add_argument("--kernel-storage", choices=["oihw", "hwio"], default="oihw",
                    help="memory order of the conv kernels behind their HWIO shape (layers.py)")
    ap.add_argument("--channels-last", action="store_true",
                    help="feed NHWC-strided batches (torch.channels_last): MIOpen's fp32 igemm kernels are NHWC; measured "
                         "+17 %% on the ResNet-18-like config, -17 %% on the small CIFAR CNN")
    ap.add_argument("--quant-stats", action="store_true",
                    help="with --bits: add layers.quant_stats of the final parameters to the result line (per tensor: clipped "
                         "shares, SQNR in dB, codes in use, code entropy); taken after the timed steps")
    ap.add_argument("--mx-stats", action="store_true",
                    help="with --element-format: add layers.mx_quant_stats of the final parameters to the result line (per tensor: "
                         "saturated and flushed shares, SQNR in dB, encodings in use, code entropy); taken after the timed steps")
    ap.add_argument("--mx-eval", nargs="?", const="fp8_e4m3", default=None, choices=list(MX_OPERAND_FORMATS), metavar="ACT_FORMAT",
                    help="with --element-format: evaluate the final model once more under layers.mx_hardware (Dense layers on the "
                         "block-scaled matrix instruction, activations quantised per block to ACT_FORMAT, default fp8_e4m3) and add "
                         "mx_eval_accuracy, mx_eval_accuracy_fake (the same quantised activations times the fake-quantised weights "
                         "with torch.matmul) and mx_eval_max_logit_diff to the result line")
    ap.add_argument("--mx-eval-fused", action="store_true",
                    help="with --mx-eval: evaluate once more under layers.mx_hardware(fused=True) (the Dense tail through "
                         "layers.mx_dense_chain: relu and the next operand's quantisation in the GEMM's epilogue) and add "
                         "mx_eval_fused_layers, mx_eval_fused_accuracy and mx_eval_fused_max_logit_diff (against the unfused "
                         "hardware path; 0.0 is expected) to the result line")
    ap.add_argument("--mx-eval-convs", action="store_true",
                    help="with --mx-eval: evaluate once more under layers.mx_hardware(convs=True) (conv layers too on the block-scaled "
                         "matrix instruction, their im2col operand gathered by ops.mx_operand_im2col) and add mx_eval_conv_layers, "
                         "mx_eval_conv_accuracy and mx_eval_conv_max_logit_diff (the model's outputs against the emulated path with "
                         "convs=True) to the result line")
    ap.add_argument("--i8-eval", action="store_true",
                    help="with --bits (a signed range of at most 8 bits): evaluate the final model once more under layers.i8_hardware "
                         "(Dense layers on the int8 matrix instruction, activations quantised per row to 8-bit integers) and add "
                         "i8_eval_accuracy, i8_eval_accuracy_emulated, i8_eval_accuracy_fake, i8_eval_max_logit_diff (against "
                         "emulate=True: the same quantised activations times the fake-quantised weights with torch.matmul) and "
                         "i8_eval_max_logit_diff_fake (against the fake-quantised model) to the result line")
    ap.add_argument("--i8-eval-act-block", type=int, default=0, metavar="B",
                    help="with --i8-eval: one activation scale per row and B consecutive inputs (a multiple of 64) instead of one per row")
    ap.add_argument("--i8-eval-convs", action="store_true",
                    help="with --i8-eval: evaluate once more under layers.i8_hardware(convs=True) (conv layers too on the int8 matrix "
                         "instruction, their im2col operand gathered by ops.i8_operand_im2col) and add i8_eval_conv_layers, "
                         "i8_eval_conv_accuracy and i8_eval_conv_max_logit_diff (the model's outputs against the emulated path with "
                         "convs=True) to the result line")
    ap.add_argument("--i8-eval-fused", action="store_true",
                    help="with --i8-eval --i8-eval-act-block 64: evaluate once more under layers.i8_hardware(fused=True) (the Dense "
                         "tail through layers.i8_dense_chain: relu and the next operand's quantisation, per row and block of 64, in "
                         "the GEMM's epilogue) and add i8_eval_fused_layers, i8_eval_fused_accuracy and "
                         "i8_eval_fused_max_logit_diff (against the unfused hardware path; 0.0 is expected) to the result line")
    ap.add_argument("--i8-eval-offsets", action="store_true",
                    help="with --i8-eval: asymmetric layers (--asymmetric) take the hardware path too (layers.i8_hardware(offsets=True): "
                         "their operand carries the offsets and the product adds the offset's row-sum term, at the price of more "
                         "matrix instructions per step); without it --i8-eval --asymmetric is refused")
    return ap


@torch.no_grad()
def i8_eval(model, x, y, act_block=0, convs=False, fused=False, offsets=False):
    """One evaluation of ``model`` on (x, y) under layers.i8_hardware, one under its ``emulate=True`` yardstick and one of the
    fake-quantised model as it stands: a dict of the three accuracies and the largest |difference| of the outputs of the last Dense
    layer that took the path (the logits of the MNIST model) between the hardware path and each of the other two.  ValueError for
    a model without a Dense layer that can take the path.  ``convs=True`` adds an evaluation under ``i8_hardware(convs=True)`` and one
    under its emulation: the number of conv layers that took the path, the accuracy, and the largest |difference| of the model's
    outputs between the two; a model without such a Dense layer is then accepted, and its Dense fields are those of the model's
    own output with no layer switched.  ``fused=True`` (``act_block`` must be 64) adds an evaluation under
    ``i8_hardware(fused=True)``: the number of layers that fused, its accuracy and the largest |difference| of the model's ``logits``
    from the unfused hardware path's (the same bits are expected: 0.0)."""
    was_training = model.training
    model.eval()
    acc, logits = [], []
    fields = {}
    try:
        probe = L.i8_hardware(model, act_block)
        last = ([m for m in L.custom_layers_of(model) if L.i8_hardware_eligible(m, offsets)] or [model if convs else None])[-1]
        if last is None:
            raise ValueError("i8_eval: the model has no Dense layer that can run on the int8 matrix instruction (a signed range of at "
                             "most 8 bits, symmetric, scalar / columnwise scales or groups of a multiple of 64 inputs)")
        for how in ("hardware", "emulate", "fake"):
            seen = []
            hook = last.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
            try:
                if how == "fake":
                    p = model(x)
                else:
                    with L.i8_hardware(model, probe.act_block, emulate=how == "emulate", offsets=offsets) as hw:
                        n_layers = len(hw.layers)
                        p = model(x)
            finally:
                hook.remove()
            acc.append(float((p.argmax(1) == y).float().mean()))
            logits.append(seen[-1])
        if fused:
            with L.i8_hardware(model, probe.act_block, fused=True, offsets=offsets) as hwf:
                if not hwf.fused_layers or not callable(getattr(model, "logits", None)):
                    raise ValueError("i8_eval: fused=True needs a model whose Dense tail fuses (i8_chain() and logits(), as "
                                     "models.MNISTDense has): nothing but relu between eligible Dense layers")
                fused_logits, p = model.logits(x), model(x)
                fields = {"i8_eval_fused_layers": len(hwf.fused_layers), "i8_eval_fused_accuracy": float((p.argmax(1) == y).float().mean()),
                          "i8_eval_fused_max_logit_diff": float((fused_logits - logits[0]).abs().max())}
        if convs:
            outs = []
            for emulate in (False, True):
                with L.i8_hardware(model, probe.act_block, emulate=emulate, convs=True, offsets=offsets) as hwc:
                    n_convs = sum(L.i8_conv_eligible(m, offsets) for m in hwc.layers)
                    if not n_convs:
                        raise ValueError("i8_eval: convs=True needs a model with a conv layer that can run on the int8 matrix "
                                         "instruction (a signed range of at most 8 bits, symmetric, a scalar scale or groups of a "
                                         "multiple of 64 along (ci, kh, kw), kernel stored oihw)")
                    outs.append(model(x))
            fields.update({"i8_eval_conv_layers": n_convs, "i8_eval_conv_accuracy": float((outs[0].argmax(1) == y).float().mean()),
                           "i8_eval_conv_max_logit_diff": float((outs[0] - outs[1]).abs().max())})
    finally:
        model.train(was_training)
    return {"i8_eval_act_block": probe.act_block, "i8_eval_layers": n_layers, "i8_eval_accuracy": acc[0],
            "i8_eval_accuracy_emulated": acc[1], "i8_eval_accuracy_fake": acc[2],
            "i8_eval_max_logit_diff": float((logits[0] - logits[1]).abs().max()),
            "i8_eval_max_logit_diff_fake": float((logits[0] - logits[2]).abs().max()), **fields}


@torch.no_grad()
def mx_eval(model, x, y, act_format="fp8_e4m3", act_scale="mx", fused=False, convs=False):
    """One evaluation of ``model`` on (x, y) under layers.mx_hardware and one under its ``emulate=True`` yardstick: a dict of both
    accuracies and the largest |difference| of the outputs of the last Dense layer that took the path (the logits of the MNIST
    model).  ``fused=True`` adds a third evaluation under ``mx_hardware(fused=True)``: its accuracy and the largest |difference| of
    the model's ``logits`` from the unfused hardware path's (the same bits are expected: 0.0).  ``convs=True`` adds an evaluation under
    ``mx_hardware(convs=True)`` and one under its emulation: the number of conv layers that took the path, the accuracy, and the
    largest |difference| of the model's outputs between the two; a model without Dense layers is then accepted."""
    was_training = model.training
    model.eval()
    acc, logits = [], []
    try:
        for emulate in (False, True):
            with L.mx_hardware(model, act_format, act_scale, emulate=emulate) as hw:
                if not hw.layers and not convs:
                    raise ValueError("mx_eval: the model has no Dense layer that can run on the block-scaled matrix instruction "
                                     "(fp4 / fp8 element format, E8M0 scales, blocks of 32)")
                seen = []
                # with convs=True a model without such a Dense layer is accepted: its Dense fields are those of the model's own output
                hook = (hw.layers[-1] if hw.layers else model).register_forward_hook(lambda m, i, o: seen.append(o.detach()))
                try:
                    p = model(x)
                finally:
                    hook.remove()
                acc.append(float((p.argmax(1) == y).float().mean()))
                logits.append(seen[-1])
        fields = {}
        if fused:
            with L.mx_hardware(model, act_format, act_scale, fused=True) as hwf:
                if not hwf.fused_layers or not callable(getattr(model, "logits", None)):
                    raise ValueError("mx_eval: fused=True needs a model whose Dense tail fuses (mx_chain() and logits(), as "
                                     "models.MNISTDense has): nothing but relu between eligible Dense layers")
                fused_logits, p = model.logits(x), model(x)
                fields = {"mx_eval_fused_layers": len(hwf.fused_layers), "mx_eval_fused_accuracy": float((p.argmax(1) == y).float().mean()),
                          "mx_eval_fused_max_logit_diff": float((fused_logits - logits[0]).abs().max())}
        if convs:
            outs = []
            for emulate in (False, True):
                with L.mx_hardware(model, act_format, act_scale, emulate=emulate, convs=True) as hwc:
                    n_convs = sum(L.mx_conv_eligible(m) for m in hwc.layers)
                    if not n_convs:
                        raise ValueError("mx_eval: convs=True needs a model with a conv layer that can run on the block-scaled matrix "
                                         "instruction (fp4 / fp8 element format, E8M0 scales, blocks of 32, kernel stored oihw)")
                    outs.append(model(x))
            fields.update({"mx_eval_conv_layers": n_convs, "mx_eval_conv_accuracy": float((outs[0].argmax(1) == y).float().mean()),
                           "mx_eval_conv_max_logit_diff": float((outs[0] - outs[1]).abs().max())})
    finally:
        model.train(was_training)
    return {"mx_eval_act_format": act_format, "mx_eval_layers": len(hw.layers), "mx_eval_accuracy": acc[0],
            "mx_eval_accuracy_fake": acc[1], "mx_eval_max_logit_diff": float((logits[0] - logits[1]).abs().max()), **fields}


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.mx_eval is not None and args.element_format is None:
        ap.error("--mx-eval needs --element-format: it runs the layers of a microscaling model on the block-scaled matrix instruction")
    if args.mx_eval_fused and args.mx_eval is None:
        ap.error("--mx-eval-fused needs --mx-eval: it compares the fused Dense tail with the unfused hardware path")
    if args.mx_eval_convs and args.mx_eval is None:
        ap.error("--mx-eval-convs needs --mx-eval: it adds the conv layers to the hardware path that --mx-eval evaluates")
    if args.i8_eval_offsets and not args.i8_eval:
        ap.error("--i8-eval-offsets needs --i8-eval: it lets the asymmetric layers take the hardware path that --i8-eval evaluates")
    if args.i8_eval and (args.bits is None or args.bits > 8 or args.unsigned or (args.asymmetric and not args.i8_eval_offsets)
                         or args.element_format is not None):
        ap.error("--i8-eval needs --bits of at most 8, signed and symmetric (or --asymmetric with --i8-eval-offsets, which adds the "
                 "offset's row-sum term to the product), and no --element-format: it runs the Dense layers of an integer model on "
                 "the int8 matrix instruction")
    if args.i8_eval_act_block and not args.i8_eval:
        ap.error("--i8-eval-act-block needs --i8-eval")
    if args.i8_eval_convs and not args.i8_eval:
        ap.error("--i8-eval-convs needs --i8-eval: it adds the conv layers to the hardware path that --i8-eval evaluates")
    if args.i8_eval_fused and not args.i8_eval:
        ap.error("--i8-eval-fused needs --i8-eval: it compares the fused Dense tail with the unfused hardware path")
    if args.i8_eval_fused and args.i8_eval_act_block != 64:
        ap.error("--i8-eval-fused needs --i8-eval-act-block 64: the epilogue writes scale blocks of 64, so under any other "
                 "activation block the fused model would not be the unfused one")
    if args.quant_stats and args.bits is None:
        ap.error("--quant-stats needs --bits: the statistics are those of a quantizer with a range")
    if args.mx_stats and args.element_format is None:
        ap.error("--mx-stats needs --element-format: the statistics are those of the microscaling quantizer")

    # read by the HSA runtime when it initialises (the first torch.cuda call below): the host driver only supports dmabuf IPC
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("the training harness needs an MI355X (no CPU fallback)")
    if args.share_gpu:
        if args.backend == "nccl":
            raise SystemExit("--share-gpu needs --backend gloo (RCCL cannot put two ranks on one GPU)")
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        if world == 1:
            for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29531"), ("RANK", "0"), ("WORLD_SIZE", "1")):
                os.environ.setdefault(k, v)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
    rank = dist.get_rank() if use_dist else 0

    value = args.value
    if args.mode == "nqcl":
        value = (args.value, args.rate)
    elif args.config == "resnet50" and args.value_coarse is not None:
        value = (args.value_coarse, args.value)
    tr = Trainer(args.config, args.mode, value, args.orientation, args.loss, seed=args.seed, device=dev,
                 ddp_mode=args.ddp_mode, graph=args.graph, batched=args.batched, bucket_mb=args.bucket_mb,
                 graph_collectives=args.graph_collectives, force_collectives=args.force_dist, kernel_storage=args.kernel_storage,
                 loss_values=args.loss_values, loss_log_capacity=max(4096, args.steps + args.warmup + 8),
                 grad_scale=(None if args.grad_scale is None else
                             (args.grad_scale if args.grad_scale == "rsqrt_group" else float(args.grad_scale))),
                 bits=args.bits, signed=not args.unsigned, rounding=args.rounding, clipped_batch=args.clipped_batch,
                 group_size=args.group_size, group_batch=args.group_batch, scale_init=args.scale_init,
                 asymmetric=args.asymmetric, asymmetric_batch=args.asymmetric_batch, element_format=args.element_format,
                 scale_format=args.scale_format or "e8m0", mx_batch=args.mx_batch)
    do_step = tr.step_graphed if args.graph else tr.step
    g = torch.Generator(device=dev).manual_seed(args.seed + rank)
    batches = [synthetic_batch(args.config, args.batch, dev, g) for _ in range(4)]
    if args.channels_last and args.config != "mnist":
        batches = [(x.contiguous(memory_format=torch.channels_last), y) for x, y in batches]
    for i in range(args.warmup):
        do_step(*batches[i % 4])
    torch.cuda.synchronize(dev)
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = do_step(*batches[i % 4])
    torch.cuda.synchronize(dev)
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    log_rows = tr.flush_loss_log() if args.loss_values and rank == 0 else None     # every rank holds the same rows: one writes
    quant_stats = L.quant_stats(tr.model) if args.quant_stats and rank == 0 else None      # after the clock has stopped
    mx_stats = L.mx_quant_stats(tr.model) if args.mx_stats and rank == 0 else None
    mx_eval_fields = mx_eval(tr.model, *batches[0], act_format=args.mx_eval, fused=args.mx_eval_fused, convs=args.mx_eval_convs) if args.mx_eval is not None and rank == 0 else None
    i8_eval_fields = i8_eval(tr.model, *batches[0], act_block=args.i8_eval_act_block, convs=args.i8_eval_convs, fused=args.i8_eval_fused, offsets=args.i8_eval_offsets) if args.i8_eval and rank == 0 else None
    if rank == 0:
        n_q = sum(p.numel() for l in tr.custom_layers for p in l._regularized())
        print(json.dumps({
            "metric": "images/sec end-to-end training step (synthetic data)", "config": args.config, "mode": args.mode,
            "value": world * args.batch * args.steps / dt, "unit": "images/s", "n_gpus": world,
            "ms_per_step": dt / args.steps * 1e3, "per_gpu_batch": args.batch,
            "orientation": ("groupwise" if args.group_size is not None or tr.element_format is not None else args.orientation),
            **({"element_format": tr.element_format, "scale_format": tr.scale_format} if tr.element_format is not None else {}),
            "loss_term": args.loss, "quantized_elements": n_q, "final_loss": float(loss.detach()), "ddp_mode": args.ddp_mode,
            "hipgraph": bool(args.graph), "graph_collectives": bool(tr.graph_collectives and args.graph and use_dist),
            **({"graph_note": tr.graph_note} if tr.graph_note else {}), "batched": bool(args.batched),
            **({"clipped_batch": True} if args.clipped_batch else {}),
            **({"group_batch": True} if args.group_batch else {}),
            **({"asymmetric_batch": True} if args.asymmetric_batch else {}),
            **({"mx_batch": True} if args.mx_batch else {}),
            "backend": (args.backend if use_dist else None),
            "channels_last": bool(args.channels_last), "kernel_storage": args.kernel_storage,
            **({"q_range": list(tr.q_range)} if tr.q_range else {}),
            **({"rounding": tr.rounding} if tr.rounding != "floor" else {}),
            **({"group_size": tr.custom_layers[0].group_size if tr.element_format is not None else tr.group_size}
               if tr.group_size is not None or tr.element_format is not None else {}),
            **({"asymmetric": True} if tr.asymmetric else {}),
            **({"scale_init": tr.scale_init} if tr.scale_init is not None else {}),
            **({"loss_values": True, "loss_log_rows": log_rows[0], "loss_log_dropped": log_rows[1]} if log_rows else {}),
            **({"quant_stats": quant_stats} if quant_stats is not None else {}),
            **({"mx_stats": mx_stats} if mx_stats is not None else {}),
            **(mx_eval_fields or {}), **(i8_eval_fields or {})}))
        if args.export_dir:
            from .export import save_compress_parameters
            print(json.dumps(save_compress_parameters(tr.model, args.export_dir)))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
