"""Multi-tensor batching of the per-step fake-quant work (SURVEY f-4) on top of ``lq_batch_*``.

A training step of the reference quantises every custom layer's kernel AND bias through its own
``my_custom_gradient`` call (custom_layers.py:263-268, 338-350): 4 / 12 / 40 tiny ops forward and as many
backward for the MNIST / CIFAR-10 / Imagenette models.  None of them depends on an activation, so

  * ``FakeQuantBatch.quantize_all()`` runs ALL forwards in one launch before the model forward and hands each
    layer its quantised tensors;
  * its autograd node receives ALL upstream gradients at the end of the backward pass and computes every scale
    gradient in two launches (traversal + finalize), writing ``scale.grad`` directly (no per-scale
    accumulate kernels) and passing ``dy`` through unchanged as ``∂P`` (STE, custom_layers.py:118) -- the
    nested-quantization vote (``lq_batch_scale_grad``), or, for a model whose layers all have ``scale_gradient="ste"``,
    the straight-through scale gradient (``lq_batch_scale_grad_ste``); one batch holds one rule;
  * ``BatchedScaleAdam.step()`` updates every scale (Adam + MinValueConstraint, custom_layers.py:158) in one launch.

Semantics per tensor are those of the single-tensor ops (same device code; results bit-identical).
Gradient accumulation across several backward passes is not supported in this mode (``scale.grad`` is
overwritten each backward), which matches the reference's one-backward-per-step training loop.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import torch

from . import _hip
from .descriptor import group_geometry, memory_descriptor
from .layers import _ConvBase, _HostLayer, custom_layers_of
from .ops import ROUNDINGS, check_element_format, check_scale_format


class _Entry:
    __slots__ = ("layer", "slot", "param", "nested", "scale", "out", "ds", "m", "v", "desc", "out_oihw", "dp", "conv", "nq",
                 "offset", "db", "mb", "vb")      # asymmetric group batch: the layer's offset, its gradient and its Adam moments


class _DeviceInts:
    """A window onto int32 device memory the library owns, for ``torch.as_tensor`` (no copy, no ownership)."""

    def __init__(self, address: int, count: int):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<i4", "data": (int(address), False), "version": 2}


class _Kind:
    """What one kind of batch owns: its refusals (``check``, ``describe``: before any device call), what an entry holds beyond the
    common buffers (``own``), the library handle or handles with their workspace (``create`` / ``destroy``), the four per-step
    calls (``forward``, ``backward``, ``clip_counts``, ``adam_step``: bound once by ``FakeQuantBatch.__init__``) and the
    capabilities below.  A kind never refers to its batch: it keeps the arrays its calls pass on (``_bind``)."""
    owns_dp = False        # the backward writes a masked dP of every tensor into a buffer of the batch (else dP is dy itself)
    loss_terms = True      # penalty_values() / inject_penalty_grads()
    defers = True          # defer_scale_grads / scale_grads_from_param_grads(): exact data-parallel mode B
    fuses = True           # BatchedScaleAdam(fused=True); where False, ``name`` says what to build fused=False for
    handle = None          # the lq_batch handle (FakeQuantBatch._handle): penalty calls, bench.py and the tools pass it on
    fused_opt = None       # BatchedScaleAdam(fused=True): the scale-gradient finalize applies the Adam step itself

    @staticmethod
    def _destroy(handle, destroy: str):
        """Destroys a library handle, if there is one.  Never raises: it runs from ``FakeQuantBatch.__del__``."""
        if handle:
            try:
                getattr(_hip.load(), destroy)(handle)
            except Exception:
                pass

    def _bind(self, batch):
        self.entries, self.device, self.hyper = batch.entries, batch.device, batch.hyper
        self.ptrs, self.grad_scales = batch._ptrs, batch._grad_scales

    def _counts(self, fn, handle, what: str):
        out = []
        for i, e in enumerate(self.entries):
            dev, groups = ctypes.c_void_p(), ctypes.c_int64()
            _hip.check(fn(handle, i, ctypes.byref(dev), ctypes.byref(groups)), what)
            view = torch.as_tensor(_DeviceInts(dev.value, groups.value), device=self.device)
            out.append(view.clone().reshape(e.scale.shape))
        return out


class _DefaultKind(_Kind):
    """The default batch on ``lq_batch_*``: the vote, ``"ste"`` or STE-only scale rule; ``dP`` is ``dy`` itself."""

    def check(self, layers, nested_layers):
        if any(getattr(n, "q_range", None) is not None for n in nested_layers):
            raise ValueError("FakeQuantBatch over a clipped layer (bits / q_range): the multi-tensor backward hands dy on as dP, "
                             "but a clipped layer's dP is a masked copy of dy; run such a model on the per-tensor path (batched=False), "
                             "or opt in to the clipped batch, which owns a dP buffer per tensor: FakeQuantBatch(..., clipped=True)")
        self._one_rule(nested_layers)
        self.rounding = "floor"

    def _one_rule(self, nested_layers):
        rules = {n.scale_gradient for n in nested_layers}
        if "ste" in rules and len(rules) > 1:
            raise ValueError('one FakeQuantBatch holds one scale-gradient rule: every layer needs scale_gradient="ste", or none')
        self.ste = "ste" in rules

    def describe(self, layer, param, nested):
        # a dense permutation of the logical axes (conv kernels stored OIHW, layers.py kernel_storage) is described in
        # memory order; outputs and gradients carry the parameter's strides
        desc = memory_descriptor(tuple(param.shape), param.data.stride(), tuple(nested.scale.shape))
        if desc is None:
            raise ValueError("parameters must be dense (contiguous, or a permutation of a contiguous array)")
        if self.ste and isinstance(layer, _ConvBase) and layer.kernel_storage == "hwio":
            raise ValueError('a batched scale_gradient="ste" model takes conv kernels in the memory order the convolution '
                             'consumes: build it with kernel_storage="oihw"')
        return desc

    def own(self, batch, e, oihw: bool, hwio_out: bool):
        # conv kernels of nested-quantization layers: the forward launch also emits the OIHW tensor MIOpen consumes and
        # the scale-gradient launch reads MIOpen's OIHW weight gradient, writing dP back in HWIO order (lq_hip.h:
        # lq_fq_forward_oihw) -- no transposition launches around the convolutions
        param = e.param
        if (oihw and e.slot == 0 and isinstance(e.layer, _ConvBase) and e.nested.penalty_threshold is not None
                and param.data.is_contiguous()):          # HWIO-stored kernels only: an OIHW-stored one needs no companion
            kh, kw, ci, co = (int(d) for d in param.shape)
            e.conv = (kh * kw, ci, co)
            e.out_oihw = torch.empty((co, ci, kh, kw), dtype=torch.float32, device=param.device)
            e.dp = torch.empty_like(param.data)
            if (not hwio_out and param.data_ptr() % 16 == 0
                    and _hip.load().lq_conv_tile_supported(kh * kw, ci, co, *e.desc) == 1):
                e.out = None               # the companion is the only forward output of this tensor

    def create(self, batch):
        self._bind(batch)
        lib = _hip.load()
        n = len(self.entries)
        arr = (_hip.TensorDesc * n)()
        for i, e in enumerate(self.entries):
            lam = e.nested.penalty_threshold
            c = getattr(e.nested.scale, "lq_constraint", None)
            arr[i] = _hip.TensorDesc(e.param.data_ptr(), e.nested.scale.data_ptr(), None, _hip.ptr(e.out), e.ds.data_ptr(),
                                     e.m.data_ptr(), e.v.data_ptr(), e.desc[0], e.desc[1], e.desc[2],
                                     float("nan") if lam is None else float(lam),
                                     float(c.min_value) if c is not None else float("-inf"),
                                     _hip.ptr(e.out_oihw), _hip.ptr(e.dp), *(e.conv or (0, 0, 0)))
        handle = ctypes.c_void_p()
        _hip.check(lib.lq_batch_create(arr, n, ctypes.byref(handle)), "lq_batch_create")
        self.handle = handle
        self._set_up(lib, n)
        self.ws = torch.empty(lib.lq_batch_workspace_bytes(handle), dtype=torch.uint8, device=self.device)

    def _set_up(self, lib, n: int):
        pass

    def destroy(self):
        self._destroy(self.handle, "lq_batch_destroy")
        self.handle = None

    def forward(self):
        _hip.check(_hip.load().lq_batch_forward(self.handle, _hip.stream_ptr(self.device)), "lq_batch_forward")

    def backward(self, oihw: bool):
        """lq_batch_scale_grad(_oihw), or -- a fused optimizer attached -- lq_batch_scale_grad_step: same launches, the finalize
        also applies the scales' Adam step."""
        lib = _hip.load()
        opt = self.fused_opt
        sp = _hip.stream_ptr(self.device)
        if self.ste:
            _hip.check(lib.lq_batch_scale_grad_ste(self.handle, self.ptrs, self.grad_scales, _hip.ptr(self.ws), self.ws.numel(), sp),
                       "lq_batch_scale_grad_ste")
            return
        if opt is None:
            fn = lib.lq_batch_scale_grad_oihw if oihw else lib.lq_batch_scale_grad
            _hip.check(fn(self.handle, self.ptrs, _hip.ptr(self.ws), self.ws.numel(), sp), "lq_batch_scale_grad")
            return
        if opt._applied:
            # the finalize of a scale-gradient pass applies Adam: a second pass before step() (gradient accumulation, a retried
            # backward) would update the scales twice and the weights once
            raise RuntimeError("FakeQuantBatch: the fused scale update of this step has already been applied; call the optimizer's "
                               "step() first, or build BatchedScaleAdam(fused=False) (fused=True excludes gradient accumulation)")
        step, step_dev = opt._advance()
        h = self.hyper
        _hip.check(lib.lq_batch_scale_grad_step(self.handle, self.ptrs, 1 if oihw else 0, _hip.ptr(self.ws), self.ws.numel(),
                                                h["lr"], h["betas"][0], h["betas"][1], h["eps"], int(step or 0), _hip.ptr(step_dev),
                                                _hip.adam_mode(h["mode"]), sp), "lq_batch_scale_grad_step")
        opt._applied = True

    def clip_counts(self):
        raise RuntimeError("clip_counts() belongs to FakeQuantBatch(clipped=True) and FakeQuantBatch(group_batch=True)")

    def adam_step(self, step: Optional[int] = None, step_dev: Optional[torch.Tensor] = None):
        h = self.hyper
        _hip.check(_hip.load().lq_batch_scale_adam(self.handle, h["lr"], h["betas"][0], h["betas"][1], h["eps"],
                                                   int(step or 0), _hip.ptr(step_dev), _hip.adam_mode(h["mode"]), _hip.stream_ptr(self.device)),
                   "lq_batch_scale_adam")


class _ClippedKind(_DefaultKind):
    """The clipped batch: ``lq_batch_*`` plus ``lq_batch_set_clip``; the backward writes the masked ``dP`` of every tensor."""
    owns_dp = True
    defers = False
    fuses = False
    name = "a clipped batch"
    _REFUSALS = {
        "defer_scale_grads": "a clipped FakeQuantBatch cannot defer its scale gradients (data-parallel mode B): the exchanged dP is a "
                             "masked copy of dy and no longer holds the dy of the clipped elements; use mode A",
        "scale_grads_from_param_grads()": "scale_grads_from_param_grads() reads P.grad as dy; a clipped batch's dP is a masked copy of "
                                          "dy, which no longer holds the dy of the clipped elements: average ds over the ranks "
                                          "(data-parallel mode A)"}

    def refuse(self, what: str):
        raise ValueError(self._REFUSALS[what])

    def check(self, layers, nested_layers):
        self._one_rule(nested_layers)
        if any(getattr(n, "q_range", None) is None for n in nested_layers):
            raise ValueError("FakeQuantBatch(clipped=True) over a layer without a range: every quantised tensor of a clipped batch "
                             "needs bits / q_range (an unclipped model runs the default batch)")
        roundings = {n.rounding for n in nested_layers}
        if len(roundings) > 1:
            raise ValueError(f"one clipped FakeQuantBatch holds one rounding, got {sorted(roundings)}")
        self.rounding = next(iter(roundings), "floor")
        if any(isinstance(layer, _ConvBase) and layer.kernel_storage == "hwio" for layer in layers):
            raise ValueError('a clipped batch takes conv kernels in the memory order the convolution '
                             'consumes: build it with kernel_storage="oihw"')

    def own(self, batch, e, oihw: bool, hwio_out: bool):
        super().own(batch, e, oihw, hwio_out)
        e.dp = torch.empty_like(e.param.data)            # the masked dP (lq_batch_backward_clip), in the parameter's element order

    def _set_up(self, lib, n: int):
        qmin = (ctypes.c_int32 * n)(*[int(e.nested.q_range[0]) for e in self.entries])
        qmax = (ctypes.c_int32 * n)(*[int(e.nested.q_range[1]) for e in self.entries])
        _hip.check(lib.lq_batch_set_clip(self.handle, qmin, qmax, n, ROUNDINGS.index(self.rounding)), "lq_batch_set_clip")

    def forward(self):
        _hip.check(_hip.load().lq_batch_forward_clip(self.handle, _hip.stream_ptr(self.device)), "lq_batch_forward_clip")

    def backward(self, oihw: bool):
        # dP of every tensor into the batch's buffers, the clip counts, and -- rule "ste" -- ds; mask only: no grad_scale, ds untouched
        _hip.check(_hip.load().lq_batch_backward_clip(self.handle, self.ptrs, self.grad_scales, _hip.ptr(self.ws), self.ws.numel(),
                                                      _hip.stream_ptr(self.device)), "lq_batch_backward_clip")

    def clip_counts(self):
        return self._counts(_hip.load().lq_batch_clip_counts, self.handle, "lq_batch_clip_counts")


class _GroupKind(_Kind):
    """The group batch on ``lq_group_batch_*``, with the offsets of asymmetric layers where there are any: entries, buffers and
    the ``lq_group_batch`` handle (one descriptor per kernel and bias), and an Adam set of its own."""
    owns_dp = True
    loss_terms = False
    defers = False
    fuses = False
    name = "a group batch (with or without asymmetric=True: the offsets step with the scales in the Adam set's one launch)"
    group = None           # the lq_group_batch handle
    adam_set = None
    mx = False             # the microscaling batch (_MxGroupKind): lq_group_batch_create_mx, a format per tensor

    def refuse(self, what: str):
        raise ValueError(f"{what} is not available on FakeQuantBatch(group_batch=True): group-wise scales have no loss term and "
                         "their dP is a masked copy of dy (no exact data-parallel mode B)")

    def check(self, layers, nested_layers):
        if any(getattr(n, "q_range", None) is None for n in nested_layers):
            raise ValueError("FakeQuantBatch(group_batch=True) over a layer without a range: group-wise scales exist for the clipped "
                             "quantizer only, every quantised tensor needs bits / q_range")
        rules = {n.scale_gradient for n in nested_layers}
        if len(rules) > 1:
            raise ValueError(f"one FakeQuantBatch holds one scale-gradient rule, got {sorted(map(str, rules))}")
        self.ste = "ste" in rules
        roundings = {n.rounding for n in nested_layers}
        if len(roundings) > 1:
            raise ValueError(f"one group FakeQuantBatch holds one rounding, got {sorted(roundings)}")
        self.rounding = next(iter(roundings), "floor")
        if any(n.penalty_threshold is not None or n.penalty_rate is not None for n in nested_layers):
            raise ValueError("FakeQuantBatch(group_batch=True) with a loss term / penalty_threshold: the penalty kernels broadcast "
                             "one-axis scales; group-wise scales have no loss term")
        if any(isinstance(layer, _ConvBase) and layer.kernel_storage == "hwio" for layer in layers):
            raise ValueError('FakeQuantBatch(group_batch=True) with kernel_storage="hwio": the groups are defined in the memory order '
                             'the convolution consumes; build the model with kernel_storage="oihw"')

    def describe(self, layer, param, nested):
        if nested.group_size is not None:
            R, C, axis = group_geometry(tuple(param.shape), param.data.stride(), tuple(nested.scale.shape), nested.group_size)
            return R, C, axis, int(nested.group_size)
        if param.dim() == 1 and param.data.is_contiguous() and nested.scale.numel() == 1:
            return 1, param.numel(), 1, param.numel()        # a bias with its scalar scale: one line, one group
        raise ValueError(f"FakeQuantBatch(group_batch=True): a parameter of shape {tuple(param.shape)} with a one-axis scale "
                         f"of shape {tuple(nested.scale.shape)} is neither group-wise nor a 1-D parameter with a scalar "
                         "scale; one-axis orientations belong to the clipped batch (clipped=True)")

    def own(self, batch, e, oihw: bool, hwio_out: bool):
        e.dp = torch.empty_like(e.param.data)                    # the masked dP, in the parameter's element order
        if getattr(e.nested, "asymmetric", False):               # only where the batch was asked to carry offsets (__init__)
            e.offset = e.nested.offset
            _hip.require_device_f32(e.offset.data, "offset")
            e.db = batch._grad_buffer(e.offset)
            e.mb = torch.zeros_like(e.offset.data)
            e.vb = torch.zeros_like(e.offset.data)

    def create(self, batch):
        self._bind(batch)
        affine = [e for e in self.entries if e.offset is not None]
        if len(self.entries) + len(affine) > batch.ADAM_SET_MAX:
            raise ValueError(f"FakeQuantBatch(group_batch=True): {len(self.entries)} scales + {len(affine)} offsets are more than the "
                             f"{batch.ADAM_SET_MAX} tensors one lq_adam_set steps in its single launch")
        lib = _hip.load()
        n = len(self.entries)
        arr = (_hip.GroupDesc * n)()
        for i, e in enumerate(self.entries):
            R, C, axis, gs = e.desc
            qmin, qmax = (0, 0) if self.mx else e.nested.q_range      # an element format brings its own range
            arr[i] = _hip.GroupDesc(e.param.data_ptr(), e.scale.data_ptr(), e.out.data_ptr(), e.dp.data_ptr(), e.ds.data_ptr(),
                                    R, C, gs, axis, int(qmin), int(qmax))
        handle = ctypes.c_void_p()
        if self.mx:
            fmts = (_hip.GroupMxFormat * n)(*[_hip.GroupMxFormat(check_element_format(e.nested.element_format).id,
                                                                 check_scale_format(e.nested.scale_format)) for e in self.entries])
            _hip.check(lib.lq_group_batch_create_mx(arr, fmts, n, ctypes.byref(handle)), "lq_group_batch_create_mx")
        elif affine:
            # kb is the layer's factor (ops.fq_backward_group_affine: the offset's defaults to the scale's), fixed for the batch's life
            offs = (_hip.GroupOffset * n)()
            for i, e in enumerate(self.entries):
                if e.offset is not None:
                    offs[i] = _hip.GroupOffset(e.offset.data_ptr(), e.db.data_ptr(), float(e.nested.grad_scale_value(e.param.numel())))
            _hip.check(lib.lq_group_batch_create_affine(arr, offs, n, ROUNDINGS.index(self.rounding), ctypes.byref(handle)),
                       "lq_group_batch_create_affine")
        else:
            _hip.check(lib.lq_group_batch_create(arr, n, ROUNDINGS.index(self.rounding), ctypes.byref(handle)), "lq_group_batch_create")
        self.group = handle
        self.ws_bytes = lib.lq_group_batch_workspace_bytes(handle)
        self.ws = torch.empty(max(1, self.ws_bytes), dtype=torch.uint8, device=self.device)
        # the Adam step of the scales, then of the offsets (no lower bound): one launch over all of them (lq_adam_set_step; the
        # gradients are the batch's ds and db buffers)
        stepped = [(e.scale, e.m, e.v, e.ds) for e in self.entries] + [(e.offset, e.mb, e.vb, e.db) for e in affine]
        na = len(stepped)
        cnt = (ctypes.c_int64 * na)(*[w.numel() for w, _, _, _ in stepped])
        mv = (ctypes.c_float * na)(*[float(c.min_value) if (c := getattr(w, "lq_constraint", None)) is not None else float("-inf")
                                     for w, _, _, _ in stepped])
        w = (ctypes.c_void_p * na)(*[t[0].data_ptr() for t in stepped])
        m = (ctypes.c_void_p * na)(*[t[1].data_ptr() for t in stepped])
        v = (ctypes.c_void_p * na)(*[t[2].data_ptr() for t in stepped])
        adam = ctypes.c_void_p()
        _hip.check(lib.lq_adam_set_create(w, m, v, cnt, mv, na, ctypes.byref(adam)), "lq_adam_set_create")
        self.adam_set = adam
        self.adam_grads = (ctypes.c_void_p * na)(*[t[3].data_ptr() for t in stepped])

    def destroy(self):
        self._destroy(self.group, "lq_group_batch_destroy")
        self._destroy(self.adam_set, "lq_adam_set_destroy")
        self.group = self.adam_set = None

    def forward(self):
        _hip.check(_hip.load().lq_group_batch_forward(self.group, _hip.stream_ptr(self.device)), "lq_group_batch_forward")

    def backward(self, oihw: bool):
        # ONE launch: dP of every tensor into the batch's buffers, the clip counts, and -- rule "ste" -- ds; mask only otherwise
        _hip.check(_hip.load().lq_group_batch_backward(self.group, self.ptrs, self.grad_scales,
                                                       _hip.ptr(self.ws) if self.ws_bytes else None, self.ws_bytes,
                                                       _hip.stream_ptr(self.device)), "lq_group_batch_backward")

    def clip_counts(self):
        return self._counts(_hip.load().lq_group_batch_clip_counts, self.group, "lq_group_batch_clip_counts")

    def adam_step(self, step: Optional[int] = None, step_dev: Optional[torch.Tensor] = None):
        h = self.hyper
        _hip.check(_hip.load().lq_adam_set_step(self.adam_set, self.adam_grads, h["lr"], h["betas"][0], h["betas"][1], h["eps"],
                                                int(step or 0), _hip.ptr(step_dev), _hip.adam_mode(h["mode"]), _hip.stream_ptr(self.device)),
                   "lq_adam_set_step")


class _MxGroupKind(_GroupKind):
    """The group batch over layers with an element format (``lq_group_batch_create_mx``): every tensor its own element format
    and scale format, the straight-through rule and the one rounding of a minifloat grid for all."""
    name = "a microscaling group batch (mx=True)"
    mx = True

    def check(self, layers, nested_layers):
        plain = [n for n in nested_layers if getattr(n, "element_format", None) is None]
        if plain:
            raise ValueError("FakeQuantBatch(group_batch=True, mx=True) over a layer without an element format: every quantised "
                             "tensor of a microscaling batch needs an element_format (formats and scale formats may differ between "
                             "layers; an integer model runs the plain group batch)")
        if any(n.penalty_threshold is not None or n.penalty_rate is not None for n in nested_layers):
            raise ValueError("FakeQuantBatch(group_batch=True, mx=True) with a loss term / penalty_threshold: the penalty kernels "
                             "know the integer grid only; a microscaling layer has no loss term")
        if any(isinstance(layer, _ConvBase) and layer.kernel_storage == "hwio" for layer in layers):
            raise ValueError('FakeQuantBatch(group_batch=True, mx=True) with kernel_storage="hwio": the blocks are defined in the '
                             'memory order the convolution consumes; build the model with kernel_storage="oihw"')
        self.ste = True                # a layer with an element format has the straight-through scale gradient
        self.rounding = "nearest"      # a minifloat grid has one rounding: ties to even


class FakeQuantBatch:
    def __init__(self, model_or_layers, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-7, mode: str = "keras",
                 oihw: bool = True, hwio_out: bool = True, autograd: bool = True, clipped: bool = False,
                 group_batch: bool = False, asymmetric: bool = False, mx: bool = False):
        """``autograd=True``: ``quantize_all()`` is ONE autograd node (2 x tensors inputs, one output per tensor) and everything happens
        inside ``loss.backward()``.  Convenient -- and, for 40 tensors, 0.4-0.6 ms of autograd-engine work per step (an 80-input node,
        40 output wrappers, an AccumulateGrad per parameter that adds into the data-parallel bucket with a launch of its own).
        ``autograd=False`` (the trainer's form): the fake-quantised tensors are persistent LEAVES -- autograd only delivers their
        gradients (``leaf.grad``, stolen from the producer: no launch) -- and ``finish_backward()`` after ``loss.backward()`` runs
        the scale-gradient launches and hands ``dP = dy`` (custom_layers.py:118) to the parameters: by reference where a parameter
        has no gradient yet, with one fused add over all others (bucket views, regularised kernels).
        ``oihw``: conv kernels of nested-quantization layers get an OIHW companion output (what MIOpen consumes).
        ``hwio_out=False``: where the LDS-tile kernel writes that companion, the HWIO output is not materialised at all -- in a
        training step the convolution is the kernel's only consumer (custom_layers.py:340-348), so the forward moves 8 bytes
        per element instead of 12; ``quantize_all()`` then returns the HWIO tensor as a permuted VIEW of the companion.
        ``clipped=True`` (opt-in): a batch of clipped b-bit layers (``bits`` / ``q_range``, each tensor its own range, one
        ``rounding`` and one rule -- ``scale_gradient`` ``None`` or ``"ste"`` -- for all).  ``quantize_all()`` is
        ``lq_batch_forward_clip``; the backward is ``lq_batch_backward_clip``, which writes the masked ``dP`` of every tensor into a
        buffer the batch owns (one per tensor, handed to the parameters) and reads 12 bytes per element (P, dy, dP) where the
        unclipped batch reads 8.  Not combined with ``defer_scale_grads`` / ``scale_grads_from_param_grads`` (a masked dP no
        longer holds the dy of the clipped elements) nor with ``BatchedScaleAdam(fused=True)``.
        ``group_batch=True`` (opt-in, not together with ``clipped``): a batch of group-wise layers (``orientation="groupwise"``) and
        their scalar-scale biases on ``lq_group_batch_*``: ``quantize_all()`` is ONE launch and the whole backward -- the masked
        ``dP`` of every tensor into a buffer the batch owns, ds, the clip counts -- ONE more.  Per tensor the results are the
        per-tensor group-wise ops' bit for bit, ds included.  A bias is the one-group line ``R = 1, C = numel, axis = 1``; any
        other one-axis scale belongs to the clipped batch.  One rounding and one rule for all; no loss term, no HWIO storage, no
        ``defer_scale_grads`` / ``scale_grads_from_param_grads``, no ``BatchedScaleAdam(fused=True)``.
        ``asymmetric=True`` (opt-in, with ``group_batch=True`` only): the group batch also carries the offsets of asymmetric layers
        (``lq_group_batch_create_affine``): still ONE launch per pass, which also writes every offset's gradient; ``out``, ``dP``,
        ds and db are the per-tensor asymmetric ops' bit for bit, and the biases (symmetric, scalar) keep the symmetric batch's
        bits.  An offset's gradient factor is its layer's ``grad_scale_value`` (what the per-tensor path passes), fixed when the
        batch is built.  The offsets join the scales' Adam set without a lower bound: scales and offsets are stepped by ONE
        launch.  That set holds 256 tensors at most (scales + offsets; the ResNet-50-like model has 108 + 54 = 162): a larger model is
        refused at construction, never split silently.  Over a model without an asymmetric layer this is the plain group batch.
        Everything the group batch refuses stays refused (``clipped``, a loss term, HWIO storage, ``defer_scale_grads``,
        ``BatchedScaleAdam(fused=True)``).
        ``mx=True`` (opt-in, with ``group_batch=True`` only, not together with ``clipped`` or ``asymmetric``): a group batch over
        layers with an ``element_format`` (``lq_group_batch_create_mx``): still ONE launch per pass.  Every quantised tensor of
        the model must carry an element format; the format and the scale format live per tensor in the batch's task table, so
        layers of different formats (``layer.make_mx(...)``) share one batch.  ``out``, ``dP``, ds and the saturation counts
        (``clip_counts()``) are the per-tensor microscaling ops' bit for bit, kernels and biases alike (a bias is the one-group
        line, as on the per-tensor path).  Each tensor's gradient factor is its layer's ``grad_scale_value``; the scales join
        the Adam set with their constraint's lower bound.  Everything the group batch refuses stays refused (a loss term, HWIO
        storage, ``defer_scale_grads``, ``BatchedScaleAdam(fused=True)``)."""
        layers = custom_layers_of(model_or_layers) if isinstance(model_or_layers, torch.nn.Module) else list(model_or_layers)
        self.layers = layers
        self.autograd = bool(autograd)
        self._external_grads = False
        self.defer_scale_grads = False       # exact data-parallel mode: backward skips ds, scale_grads_from_param_grads() follows
        self.entries: List[_Entry] = []
        nested_layers = [getattr(layer, a) for layer in layers for a in ("nested_q_w_layer", "nested_q_k_layer", "nested_q_b_layer")
                         if hasattr(layer, a)]
        fmt = [n for n in nested_layers if getattr(n, "element_format", None) is not None]
        if fmt and not mx:        # the microscaling batch is an opt-in of its own: FakeQuantBatch(..., group_batch=True, mx=True)
            raise ValueError(f"FakeQuantBatch over a layer with an element format ({fmt[0].element_format!r}): none of the multi-tensor "
                             "batches (default, clipped, group) carries a minifloat grid; run such a model on the per-tensor path "
                             "(batched=False)")
        kind = self._set_kind(clipped, group_batch, asymmetric, mx)
        if not asymmetric and any(getattr(n, "asymmetric", False) for n in nested_layers):
            raise ValueError("FakeQuantBatch over an asymmetric layer: the offsets and their gradients travel only in the group "
                             "batch that was asked to carry them; opt in with FakeQuantBatch(..., group_batch=True, asymmetric=True), "
                             "or run such a model on the per-tensor path (batched=False)")
        if not group_batch and any(getattr(n, "group_size", None) is not None for n in nested_layers):
            raise ValueError("FakeQuantBatch over a group-wise layer (group_size): its scale has two non-unit axes, which the "
                             "(outer, G, inner) descriptor of the default and the clipped batch cannot express; run such a model on "
                             "the per-tensor path, or opt in to the group batch: FakeQuantBatch(..., group_batch=True)")
        kind.check(layers, nested_layers)
        self.ste = kind.ste                  # every scale gradient of the batch is the straight-through one
        self.rounding = kind.rounding
        self._build_entries(layers, oihw, hwio_out)
        self.device = self.entries[0].param.device
        n = len(self.entries)
        self._ptrs = (ctypes.c_void_p * n)()
        self._grad_scales = (ctypes.c_float * n)(*[e.nested.grad_scale_value(e.param.numel()) for e in self.entries]) if self.ste else None
        self.hyper = dict(lr=lr, betas=betas, eps=eps, mode=mode)
        # what the backward publishes and the optimizer steps, as (parameter, gradient buffer, the op gives it a gradient): the
        # scales, then the offsets of asymmetric entries
        self._stepped = ([(e.scale, e.ds, e.nq) for e in self.entries]
                         + [(e.offset, e.db, e.nq) for e in self.entries if e.offset is not None])
        kind.create(self)
        self._handle = kind.handle
        self.ws = kind.ws
        self._forward_call = kind.forward
        self._scale_grad_call = kind.backward
        self.scale_adam_step = kind.adam_step
        self._data_ptrs = [(e.param.data_ptr(), e.nested.scale.data_ptr()) for e in self.entries]
        self._offset_ptrs = [(e, e.offset.data_ptr()) for e in self.entries if e.offset is not None]
        # per-step host work is kept to list lookups: the flat (param, scale, ...) argument list of the autograd node and,
        # per layer, which outputs are its kernel and its bias
        self._flat = [t for e in self.entries for t in (e.param, e.nested.scale)]
        slots = {}
        for i, e in enumerate(self.entries):
            slots.setdefault(id(e.layer), [e.layer, None, None])[1 + e.slot] = i
        self._layer_slots = list(slots.values())
        self._oihw_idx = [i for i, e in enumerate(self.entries) if e.out_oihw is not None]     # extra autograd outputs, in this order
        self._oihw_pos = {i: len(self.entries) + k for k, i in enumerate(self._oihw_idx)}
        if not self.autograd:
            # persistent leaves over the static output buffers (the forward launch rewrites the memory under them; autograd never
            # looks at their values, only routes gradients to them)
            self._leaf = [None if e.out is None else e.out.detach().requires_grad_(True) for e in self.entries]
            self._leaf_o = [None if e.out_oihw is None else e.out_oihw.detach().requires_grad_(True) for e in self.entries]
            self._all_leaves = [t for t in self._leaf + self._leaf_o if t is not None]
            # no companions at all (kernels stored OIHW, dense models): what quantize_all() hands to the layers never changes
            self._static_pre = self._static_outs = None
            if not self._oihw_idx and all(lf is not None for lf in self._leaf):
                self._static_outs = list(self._leaf)
                self._static_pre = [(layer.__dict__, (None if ik is None else self._leaf[ik], None if ib is None else self._leaf[ib], None))
                                    for layer, ik, ib in self._layer_slots]

    def _set_kind(self, clipped: bool, group_batch: bool, asymmetric: bool, mx: bool = False):
        """The four opt-ins as read-only facts and the kind they resolve to -- the only place that reads them.  No device call."""
        self.clipped = bool(clipped)
        self.group_batch = bool(group_batch)
        self.asymmetric = bool(asymmetric)
        self.mx = bool(mx)
        if mx and not group_batch:
            raise ValueError("mx=True belongs to group_batch=True: only the group batch carries an element format per tensor "
                             "(FakeQuantBatch(..., group_batch=True, mx=True))")
        if mx and (clipped or asymmetric):
            raise ValueError(f"mx=True together with {'clipped' if clipped else 'asymmetric'}=True: the microscaling formats are "
                             "symmetric and bring their own range; a microscaling batch is group_batch=True, mx=True alone")
        if asymmetric and clipped:
            raise ValueError("asymmetric=True together with clipped=True: the clipped one-axis batch carries no offset per group; "
                             "offsets travel in the group batch only (group_batch=True, asymmetric=True)")
        if asymmetric and not group_batch:
            raise ValueError("asymmetric=True belongs to group_batch=True: only the group batch carries an offset per group and its "
                             "gradient")
        if group_batch and clipped:
            raise ValueError("group_batch=True together with clipped=True: a batch is either the group batch (group-wise layers and "
                             "their biases) or the clipped batch (one-axis scales), not both")
        self._kind = _MxGroupKind() if mx else _GroupKind() if group_batch else _ClippedKind() if clipped else _DefaultKind()
        return self._kind

    def _grad_buffer(self, t):
        """The gradient buffer of a learned tensor (scale or offset): an existing contiguous ``.grad`` (e.g. a DataParallel bucket
        view) is written straight into; otherwise zeros of the batch's own."""
        g = t.grad
        if g is not None and g.is_contiguous():
            self._external_grads = True          # external buffer (bucket view): zeroed by its owner, never set to None
            return g
        return torch.zeros_like(t.data)

    def _build_entries(self, layers, oihw: bool, hwio_out: bool):
        """One entry per kernel / ``W`` (slot 0) and bias (slot 1) of every layer, for every kind."""
        kind = self._kind
        found = []
        for layer in layers:
            if not isinstance(layer, _HostLayer):
                raise TypeError(f"not a custom layer: {type(layer).__name__}")
            for slot, (_, nested, param) in enumerate(layer.scale_pairs()):
                # geometry first: a tensor the kind cannot describe is refused before anything touches the device
                found.append((layer, slot, param, nested, kind.describe(layer, param, nested)))
        for layer, slot, param, nested, desc in found:
            e = _Entry()
            e.layer, e.slot, e.param, e.nested, e.desc = layer, slot, param, nested, desc
            e.scale = nested.scale             # the Parameter itself: nn.Module attribute lookup is the dearest step of a per-step loop
            _hip.require_device_f32(param.data, "parameter")
            _hip.require_device_f32(nested.scale.data, "scale")
            e.out = torch.empty_like(param.data)
            e.nq = nested.penalty_threshold is not None or self.ste      # the op itself gives this scale a gradient
            e.ds = self._grad_buffer(nested.scale)
            e.m = torch.zeros_like(nested.scale.data)
            e.v = torch.zeros_like(nested.scale.data)
            e.out_oihw = e.dp = e.conv = None
            e.offset = e.db = e.mb = e.vb = None
            kind.own(self, e, oihw, hwio_out)
            self.entries.append(e)
        if not self.entries:
            raise ValueError("no custom layers")

    #: tensors one lq_adam_set steps in its single launch (scales + offsets of a group batch)
    ADAM_SET_MAX = 256

    def __del__(self):
        kind = getattr(self, "_kind", None)      # absent where the constructor raised before the kind was resolved
        if kind is not None:
            kind.destroy()
            self._handle = None

    def _check_pointers(self):
        for e, (pp, sp) in zip(self.entries, self._data_ptrs):
            if e.param.data_ptr() != pp or e.nested.scale.data_ptr() != sp:      # the module's scale: a replaced Parameter is caught too
                raise RuntimeError("a parameter or scale was re-allocated after the batch was built "
                                   "(e.g. model.to(device)); rebuild the FakeQuantBatch")
        for e, bp in self._offset_ptrs:
            if e.nested.offset.data_ptr() != bp:
                raise RuntimeError("an offset was re-allocated after the batch was built (e.g. model.to(device)); rebuild the "
                                   "FakeQuantBatch")

    # ------------------------------------------------------------------ forward
    def quantize_all(self):
        """One launch: fake-quantise every kernel/bias; layers pick the results up in their next call."""
        self._check_pointers()
        if not self.autograd:
            return self._quantize_all_leaves()
        outs = _BatchFn.apply(self, *self._flat)
        n = len(self.entries)
        for layer, ik, ib in self._layer_slots:
            # plain instance attribute (not a Parameter/Module): written through __dict__, nn.Module.__setattr__ costs ~3 us
            layer.__dict__["_q_pre"] = (None if ik is None else outs[ik], None if ib is None else outs[ib],
                                        outs[self._oihw_pos[ik]] if ik in self._oihw_pos else None)
        return outs[:n]

    def _quantize_all_leaves(self):
        self._forward_call()
        self._awaiting_finish = True
        for lf in self._all_leaves:
            lf.grad = None
        if self._static_pre is not None:                   # every tensor has its own HWIO-shaped leaf: the hand-outs never change
            for d, pre in self._static_pre:
                d["_q_pre"] = pre
            return self._static_outs
        outs = [lf if lf is not None else lo.permute(2, 3, 1, 0)      # the HWIO-shaped view of a companion-only kernel
                for lf, lo in zip(self._leaf, self._leaf_o)]
        for layer, ik, ib in self._layer_slots:
            layer.__dict__["_q_pre"] = (None if ik is None else outs[ik], None if ib is None else outs[ib],
                                        self._leaf_o[ik] if ik is not None else None)
        return outs

    def finish_backward(self):
        """``autograd=False``: call after ``loss.backward()``.  Reads the gradients autograd left on the fake-quantised leaves, runs
        the scale-gradient launches (unless ``defer_scale_grads``: exact data-parallel mode computes them after the exchange) and
        gives every parameter its ``dP = dy`` (custom_layers.py:118)."""
        if self.autograd:
            raise RuntimeError("finish_backward() belongs to FakeQuantBatch(autograd=False)")
        if not getattr(self, "_awaiting_finish", False):
            # a second call would add dP to the parameters' gradients (bucket views) once more
            raise RuntimeError("finish_backward() without a quantize_all() since the last call: one backward pass per forward")
        self._awaiting_finish = False
        dps = self._backward_core([None if lf is None else lf.grad for lf in self._leaf]
                                  + [self._leaf_o[i].grad for i in self._oihw_idx])
        add_to, add_from = [], []
        for e, dp in zip(self.entries, dps):
            p = e.param
            if p.grad is None:
                p.grad = dp                                # by reference: no launch (what AccumulateGrad does with a fresh gradient)
            elif p.grad.data_ptr() == dp.data_ptr():
                pass                                       # clipped batch: the parameter still holds the batch's dP buffer, just rewritten
            else:
                add_to.append(p.grad)                      # a data-parallel bucket view, or the gradient a regulariser left there
                add_from.append(dp)
        if add_to:
            torch._foreach_add_(add_to, add_from)          # one fused launch for all of them

    # ------------------------------------------------------------------ backward of every tensor (both modes)
    def _point_at(self, grads, name: str = "dy", as_it_stands=(), zeros: bool = True):
        """The one writer of the pointer table the scale-gradient launches read ``dy`` from.  ``grads[i]`` is the upstream
        gradient of tensor i: ``None`` (nothing consumed the tensor) stands for zeros like the parameter -- or, ``zeros=False``, for
        a NULL entry where the op reads no dy (a tensor without a vote; the caller has refused every other); an index in
        ``as_it_stands`` holds the OIHW gradient of a companion, which the launch gathers itself; every other gradient is brought
        into the parameter's element order (this loop runs every eager step for every tensor: ``_hip.require_like``).  Returns the
        tensors the table now points at, one per entry: the caller keeps them alive until the launch is enqueued."""
        ptrs = self._ptrs
        keep = []
        for i, e in enumerate(self.entries):
            d = grads[i]
            if d is None and not (zeros or e.nq):
                keep.append(None)
                ptrs[i] = None
                continue
            if d is None:
                d = torch.zeros_like(e.param.data)
            elif i in as_it_stands:
                d = _hip.require_device_f32(d, name)
            else:
                d = _hip.require_like(d, name, e.param)
            keep.append(d)
            ptrs[i] = d.data_ptr()
        return keep

    def _launch_and_publish(self, keep, oihw: bool = False, gathered=(), refuse_accumulation: bool = True):
        """The scale-gradient launches on the table ``_point_at`` has just written, then ``scale.grad`` of every scale the op gives
        a gradient.  Returns ``dP`` per tensor: the batch's own buffers where the launch writes one (a clipped batch: the masked
        copies of dy; ``gathered`` companions: dy in HWIO order), the kept dy itself otherwise (custom_layers.py:118)."""
        if refuse_accumulation and not self._external_grads:
            for p, _, nq in self._stepped:
                if nq and p.grad is not None:
                    # the kernel OVERWRITES its gradient buffer: a second backward without zero_grad(set_to_none=True)
                    # would silently drop the first gradient -- refuse instead (before anything is launched)
                    raise RuntimeError("FakeQuantBatch: scale (and offset) gradients must be None before backward "
                                       "(gradient accumulation over several backward passes is not supported in batched mode)")
        self._scale_grad_call(oihw)
        for p, g, nq in self._stepped:
            if nq:
                p.grad = g                                 # written in place by the kernel: no accumulate launch (an offset's by the same launch)
            # STE-only: zeros_like(scale) (CL custom_layers.py:62) -- no scale gradient from the op
        if self._kind.owns_dp:
            return [e.dp for e in self.entries]
        if gathered:
            return [e.dp if i in gathered else d for i, (e, d) in enumerate(zip(self.entries, keep))]
        return keep

    def _backward_core(self, dys):
        """``dys``: upstream gradient of every HWIO-shaped output, then of every OIHW companion (``None`` where nothing consumed
        it).  Launches the scale-gradient pass (unless deferred), sets ``scale.grad`` and returns ``dP`` per tensor."""
        if self.defer_scale_grads and not self._kind.defers:
            self._kind.refuse("defer_scale_grads")
        dys = list(dys)
        # a conv kernel with an OIHW companion: its consumer (the convolution) used the companion, so the gradient arrives there,
        # in OIHW order; a consumer that used the HWIO output instead is served like every other tensor
        gathered = set()
        for i in self._oihw_idx:
            d_o = dys[self._oihw_pos[i]]
            if d_o is not None:
                if dys[i] is not None:
                    raise RuntimeError("FakeQuantBatch: both the HWIO and the OIHW output of one conv kernel received a gradient")
                gathered.add(i)
        if self.defer_scale_grads:           # dP == dy (custom_layers.py:118); ds follows after the all-reduce
            dps = []
            for i, e in enumerate(self.entries):
                d = dys[self._oihw_pos[i]].permute(2, 3, 1, 0) if i in gathered else dys[i]
                dps.append(d if d is not None else torch.zeros_like(e.param.data))
            return dps
        for i in gathered:
            dys[i] = dys[self._oihw_pos[i]]
        if gathered and any(dys[i] is not None for i in self._oihw_idx if i not in gathered):
            raise RuntimeError("FakeQuantBatch: conv kernels must all be consumed through the same layout in one step")
        return self._launch_and_publish(self._point_at(dys, as_it_stands=gathered), bool(gathered), gathered)

    def clip_counts(self):
        """Clipped batch: per entry, the number of elements the latest backward found outside the range, per group (int32, in
        the shape of the entry's scale; exact).  Copies of the library's device buffers: no synchronisation."""
        return self._kind.clip_counts()

    # ------------------------------------------------------------------ exact data-parallel mode (ddp.py, mode B)
    def scale_grads_from_param_grads(self):
        """ds of every nested-quantization tensor from its parameter's CURRENT gradient, in two launches.  After the
        data-parallel all-reduce ``P.grad`` is the global-batch dy (dP == dy, custom_layers.py:118), so this yields the
        single-device large-batch scale gradient, identical on every rank."""
        if not self._kind.defers:
            self._kind.refuse("scale_grads_from_param_grads()")
        if self.ste:
            raise RuntimeError("scale_grads_from_param_grads() is the exact mode of the nested-quantization vote; the straight-through "
                               "scale gradient is linear in dy: average ds over the ranks (data-parallel mode A)")
        grads = [e.param.grad for e in self.entries]
        if any(g is None and e.nq for g, e in zip(grads, self.entries)):
            raise RuntimeError("scale_grads_from_param_grads: a quantised parameter has no gradient")
        # no refusal here: ds is recomputed from whatever P.grad holds now, as often as the caller asks
        self._launch_and_publish(self._point_at(grads, "parameter gradient", zeros=False), refuse_accumulation=False)

    # ------------------------------------------------------------------ custom loss terms
    _KINDS = {"maxbin": 0, "difference": 1, "inverse": 2}

    def _value_buffers(self):
        """Host constants and persistent device outputs of the penalty value (built once: a captured graph keeps pointing at
        ``terms`` / ``penalty``): element counts and, per tensor, whether it opens a new layer (CL-F:102-116 pairs a layer's
        kernel with its bias)."""
        vb = getattr(self, "_values", None)
        if vb is None:
            n = len(self.entries)
            dims = (ctypes.c_float * n)(*[float(e.param.numel()) for e in self.entries])
            start = (ctypes.c_uint8 * n)(*[1 if e.slot == 0 else 0 for e in self.entries])
            terms = torch.zeros(n, dtype=torch.float32, device=self.device)
            penalty = torch.zeros((), dtype=torch.float32, device=self.device)
            vb = self._values = (dims, start, terms, penalty)
        return vb

    def penalty_values(self, kind: str):
        """``(terms, penalty)``: the per-tensor terms (one float per entry) and the model penalty of the reference's
        ``compute_{maxbin,difference,inverse}_penalty`` (custom_loss_functions.py:75-116, 161-195, 240-275) for the current
        parameters and scales, without a backward pass (lq_batch_penalty_values).  Both are persistent device tensors that
        the next call rewrites in place."""
        if not self._kind.loss_terms:
            self._kind.refuse("penalty_values()")
        self._check_pointers()
        dims, start, terms, penalty = self._value_buffers()
        _hip.check(_hip.load().lq_batch_penalty_values(self._handle, self._KINDS[kind], dims, start, terms.data_ptr(), penalty.data_ptr(),
                                                       _hip.ptr(self.ws), self.ws.numel(), _hip.stream_ptr(self.device)),
                   "lq_batch_penalty_values")
        return terms, penalty

    def inject_penalty_grads(self, kind: str, penalty_rate: float, accumulate_ds: bool = False, values: bool = False):
        """Adds d(penalty_rate * penalty)/dP to every ``P.grad`` and writes d(...)/ds to every ``scale.grad`` in 2-4
        launches.  Call after ``loss.backward()`` of the task loss alone: the reference's objective is
        ``mean(SCCE) + penalty_rate * penalty`` (custom_loss_functions.py:58), so the coefficient of tensor i's term
        ``mean(...)_i`` is the constant ``penalty_rate * numel_i / sum(numel)`` (:110-116) and no autograd node per tensor
        is needed.  Equivalent to differentiating ``SCCE*.compute_total_loss`` (tests/test_gpu_batch.py).
        ``accumulate_ds``: add the penalty's scale gradient to what the ds buffers already hold (nested-quantization layers
        trained with a loss term: LQ_PENALTY_ACCUMULATE_DS).
        ``values``: also evaluate the penalty (lq_batch_penalty_grads_values: the same gradient launches, then the value
        launches) and return it as a 0-dim device tensor -- a persistent buffer, rewritten in place by every call; the
        per-tensor terms are in ``self._values[2]``.  Default: returns ``None`` and issues the gradient launches only."""
        if not self._kind.loss_terms:
            self._kind.refuse("inject_penalty_grads()")
        lib = _hip.load()
        n = len(self.entries)
        normalizer = float(sum(e.param.numel() for e in self.entries))
        coeff = (ctypes.c_float * n)(*[float(penalty_rate) * e.param.numel() / normalizer for e in self.entries])
        grads = (ctypes.c_void_p * n)()
        for i, e in enumerate(self.entries):
            if kind != "inverse":
                g = e.param.grad
                if g is None:
                    g = e.param.grad = torch.zeros_like(e.param.data)
                if not _hip.same_layout(g, e.param.data):       # a hand-assigned gradient: bring it into the parameter's element order
                    g = e.param.grad = torch.empty_like(e.param.data).copy_(g)
                grads[i] = g.data_ptr()
        kind_flag = self._KINDS[kind] | (_hip.LQ_PENALTY_ACCUMULATE_DS if accumulate_ds else 0)
        penalty = None
        if values:
            dims, start, terms, penalty = self._value_buffers()
            _hip.check(lib.lq_batch_penalty_grads_values(self._handle, kind_flag, coeff, grads, dims, start, terms.data_ptr(),
                                                         penalty.data_ptr(), _hip.ptr(self.ws), self.ws.numel(),
                                                         _hip.stream_ptr(self.device)), "lq_batch_penalty_grads_values")
        else:
            _hip.check(lib.lq_batch_penalty_grads(self._handle, kind_flag, coeff, grads, _hip.ptr(self.ws), self.ws.numel(),
                                                  _hip.stream_ptr(self.device)), "lq_batch_penalty_grads")
        for e in self.entries:
            e.scale.grad = e.ds
        return penalty


class _BatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, batch: FakeQuantBatch, *tensors):
        batch._forward_call()
        ctx.batch = batch
        ctx.set_materialize_grads(False)        # an output nobody consumed arrives as None in backward, not as a zero tensor
        # fresh tensor objects over the static buffers: every HWIO output, then the OIHW companions of the conv kernels
        # (a tensor without a materialised HWIO output hands out the HWIO-shaped permuted view of its companion)
        return tuple(e.out.detach() if e.out is not None else e.out_oihw.detach().permute(2, 3, 1, 0) for e in batch.entries) \
            + tuple(batch.entries[i].out_oihw.detach() for i in batch._oihw_idx)

    @staticmethod
    def backward(ctx, *dys):
        batch: FakeQuantBatch = ctx.batch
        dps = batch._backward_core(dys)
        grads = [None]
        for dp in dps:
            grads.extend((dp, None))       # (dP, d scale): the scale gradient is written in place by the kernel, never through autograd
        return tuple(grads)


class BatchedScaleAdam:
    """Optimizer facade over ``FakeQuantBatch.scale_adam_step`` (K6 for every scale in one launch)."""

    def __init__(self, batch: FakeQuantBatch, capturable: bool = False, fused: bool = False):
        """``fused``: the batch's scale-gradient finalize applies this optimizer's step in the same launch
        (lq_batch_scale_grad_step) and ``step()`` only acknowledges it.  For training steps in which nothing reads or changes the
        scale gradients between backward and ``step()`` -- no loss term, no exchange of ds (single process, or exact data-parallel
        mode B where ds is computed after the exchange); every tensor must be a nested-quantization one.  Exactly ONE
        scale-gradient pass per ``step()``: a second one raises (it would apply Adam to the scales twice) -- no gradient accumulation."""
        self.batch = batch
        self.capturable = capturable
        self._applied = False
        if fused:
            if not batch._kind.fuses:
                raise ValueError("the fused finalize + Adam launch exists for the nested-quantization vote only: "
                                 f"build BatchedScaleAdam(fused=False) for {batch._kind.name}")
            if batch.ste:
                raise ValueError("the fused finalize + Adam launch exists for the nested-quantization vote only: "
                                 'build BatchedScaleAdam(fused=False) for a scale_gradient="ste" model')
            if any(e.nested.penalty_threshold is None for e in batch.entries):
                raise ValueError("a fused scale update needs nested-quantization layers throughout (every scale gets its gradient "
                                 "from the batch's own scale-gradient pass)")
            if batch._external_grads:
                raise ValueError("a fused scale update cannot be combined with gradient buffers that are exchanged (bucket views)")
            batch._kind.fused_opt = self
        self._step = 0
        self._step_t = torch.zeros(1, dtype=torch.int64, device=batch.device) if capturable else None
        self.param_groups = [{"params": [p for p, _, _ in batch._stepped]}]

    def zero_grad(self, set_to_none: bool = True):
        for p, _, _ in self.batch._stepped:
            p.grad = None

    def _advance(self):
        """(host step, device step tensor) of the update that is about to be applied."""
        if self.capturable:
            self._step_t += 1
            return None, self._step_t
        self._step += 1
        return self._step, None

    @torch.no_grad()
    def step(self):
        if self.batch._kind.fused_opt is self:
            if not self._applied:
                raise RuntimeError("BatchedScaleAdam(fused=True).step() without a backward pass of the batch since the last step")
            self._applied = False            # the finalize of this step's scale-gradient pass has already updated the scales
            return
        # only scales that actually received a gradient this step are updated by Adam in the reference too; with the
        # nested-quantization op every scale does.  STE-only scales are updated from the loss-term gradients.
        for p, buf, _ in self.batch._stepped:                      # an asymmetric group batch: the offsets step in the same launch
            g = p.grad
            if g is None:
                buf.zero_()
            elif g.data_ptr() != buf.data_ptr():
                buf.copy_(g)                                       # loss-term gradients arrive in autograd-owned tensors
        step, step_dev = self._advance()
        self.batch.scale_adam_step(step=step, step_dev=step_dev)
