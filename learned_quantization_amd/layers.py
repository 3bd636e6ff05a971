"""Host layers: the reference's constructor / attribute / call surface on PyTorch-ROCm.

Mirrors /root/reference/MNIST/nested_quantization_layer/custom_components/custom_layers.py
(NQ-L) and /root/reference/CIFAR-10/custom_loss_terms/custom_components/custom_layers.py (CL-L):

  MinValueConstraint(min_value); __call__(w); get_config()                       NQ-L:35-46
  CustomQuantizedScaleLayer(penalty_threshold|penalty_rate, initializer, orientation)
      .build(input_shape) .call(inputs) .scale .orientation                      NQ-L:123-200, CL-L:67-144
  CustomDenseLayer(seed, units, penalty_threshold, orientation, initializer, name,
                   regularizer, trained_weights=None, **kw)
      .W .b .nested_q_w_layer .nested_q_b_layer .units                           NQ-L:203-268
  CustomConv2DLayer(seed, penalty_threshold, orientation, initializer, filters, kernel_size,
                    strides, padding, name, regularizer, trained_weights=None, **kw)
      .kernel .b .nested_q_k_layer .nested_q_b_layer                             NQ-L:271-350
  CustomConv2DLayerNoBias(...)  .kernel .nested_q_k_layer
      /root/reference/CIFAR-10/paper_implementation/custom_components/custom_layers.py:299-365

Parameters have the REFERENCE's shapes -- Dense ``W`` = (in, out), conv ``kernel`` =
HWIO (kh, kw, ci, co) -- so ``orientation`` means the same axes as in the reference
(rowwise = axis 0, columnwise = axis 1, channelwise = axis 2 = input channels), the loss terms
and callbacks see the same shapes, and the integer export is byte-compatible.  The matmul /
convolution themselves are stock (rocBLAS / MIOpen through torch) and out of scope; only
the fake-quant of W/kernel/b runs in this package's HIP kernels.

``kernel_storage`` (conv layers; not in the reference) chooses the MEMORY order behind the HWIO shape:
  "oihw" (default)  the kernel's elements lie in the order MIOpen consumes.  ``kernel.permute(3, 2, 0, 1)`` is a contiguous
                    OIHW tensor, so the fake-quantised kernel goes to the convolution as it is written, MIOpen's weight
                    gradient IS dP (custom_layers.py:118, 0 bytes), and the fake-quant kernels stream both (8 B per element
                    forward, 8 B backward -- SURVEY 8d's figures) with the groups described in memory order
                    (descriptor.memory_descriptor).  Index by index every tensor equals the HWIO-stored one.
  "hwio"            contiguous HWIO like a TensorFlow variable (zero-copy hand-over of the raw buffer to code that expects
                    that); the kernels then transpose through LDS tiles (lq_fq_forward_oihw / lq_fq_scale_grad_oihw).

Like Keras layers, these build lazily on first call (``build(input_shape)``); pass
``input_shape=`` (Dense: last dim, Conv: channels) to build eagerly so an optimizer can be
created before the first forward.

Conscious deviations (documented in DESIGN.md): activations are NCHW by default
(``data_format="NHWC"`` accepts the reference's layout); the ``setup_logger`` side effects
at construction (NQ-L:133-145) are dropped.
"""
from __future__ import annotations

import math
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .descriptor import groupwise_scale_shape, scale_shape

eps_float32 = float(np.finfo(np.float32).eps)            # NQ-L:11
SCALE_INIT = float(np.float32(eps_float32 * 100))        # NQ-L:156
_NAME_COUNTERS = {}


def _auto_name(prefix: str) -> str:
    """Keras auto-naming: custom_dense_layer, custom_dense_layer_1, ... (the reference's
    name-substring selection relies on these because `name` is not forwarded, NQ-L:219,290)."""
    n = _NAME_COUNTERS.get(prefix, 0)
    _NAME_COUNTERS[prefix] = n + 1
    return prefix if n == 0 else f"{prefix}_{n}"


def reset_layer_names() -> None:
    """Counterpart of tf.keras.backend.clear_session() for the auto-name counters."""
    _NAME_COUNTERS.clear()


class RandomNormal:
    """tf.keras.initializers.RandomNormal(mean=0.0, stddev=0.05, seed=None) counterpart: callable(shape)."""

    def __init__(self, mean: float = 0.0, stddev: float = 0.05, seed: Optional[int] = None):
        self.mean, self.stddev, self.seed = mean, stddev, seed
        self._calls = 0

    def __call__(self, shape, dtype=torch.float32, device=None):
        gen = None
        if self.seed is not None:
            gen = torch.Generator(device="cpu")
            gen.manual_seed(int(self.seed) + self._calls)   # distinct tensors per call, reproducible per seed
            self._calls += 1
        t = torch.empty(tuple(shape), dtype=dtype).normal_(self.mean, self.stddev, generator=gen)
        return t.to(device) if device is not None else t


class L2:
    """tf.keras.regularizers.l2(l2): l2 * sum(w^2)."""

    def __init__(self, l2: float = 0.01):
        self.l2 = float(l2)

    def __call__(self, w: torch.Tensor) -> torch.Tensor:
        return self.l2 * torch.sum(torch.square(w))


def l2(value: float = 0.01) -> L2:
    return L2(value)


class MinValueConstraint:
    """Ensures the scale factor values stay above a defined minimum value (NQ-L:35-46)."""

    def __init__(self, min_value):
        self.min_value = min_value

    def __call__(self, w):
        """Returns max(w, min_value) (NQ-L:42-43).  Out of place, like tf.maximum."""
        out = w.detach().clone()
        return ops.min_value_project_(out, self.min_value)

    def project_(self, w: torch.Tensor) -> torch.Tensor:
        """In-place form used after an optimizer step (Keras applies constraints by assignment)."""
        with torch.no_grad():
            return ops.min_value_project_(w, self.min_value)

    def get_config(self):
        return {"min_value": self.min_value}


class CustomQuantizedScaleLayer(nn.Module):
    """Nested layer that owns the trainable scale and applies the fake-quant op (NQ-L:123-200).

    ``penalty_threshold`` given  -> nested-quantization op (hand-written scale gradient).
    ``penalty_rate`` given instead (CL-L:71) -> STE-only op; the scale learns through a loss term.
    ``scale_gradient="ste"`` (not in the reference; only without ``penalty_threshold``) -> the scale also receives the
    straight-through gradient ``grad_scale * sum dy * (floor(P/s) - P/s)`` (ops.fq_scale_grad_ste); ``grad_scale`` is a
    float or ``"rsqrt_group"`` = 1 / sqrt(elements per group).
    ``bits`` / ``signed`` or ``q_range=(qmin, qmax)`` (not in the reference; only without ``penalty_threshold``) -> the clipped
    quantizer (ops.fq_forward_clip / fq_backward_clip): integers saturate at [-2^(b-1), 2^(b-1) - 1] (signed) or [0, 2^b - 1],
    clipped elements pass no gradient to the parameter and, with ``scale_gradient="ste"``, pull the scale towards covering them.
    ``rounding="nearest"`` (not in the reference; only with a range) -> the integers are rint(P/s), round half to even, instead of
    floor(P/s); the LSQ residual is then centred on zero.
    ``orientation="groupwise", group_size=gs`` (not in the reference; only with a range and without a loss term) -> one scale per
    ``gs`` consecutive inputs of each output unit (descriptor.groupwise_scale_shape; ops.fq_forward_group / fq_backward_group).
    The groups are defined in the parameter's memory order: a Dense kernel ``(in, out)`` gets scales ``(nb, out)``, a conv kernel
    stored OIHW gets ``(co, nb)`` over the (ci, kh, kw) run of each output channel.
    ``asymmetric=True`` (not in the reference; only with ``orientation="groupwise"``, a range and ``scale_gradient="ste"``) -> the
    layer also owns ``offset``, a Parameter of the scale's shape (zeros), and quantises ``clamp(rnd((P - b) / s)) * s + b``
    (ops.fq_forward_group_affine / fq_backward_group_affine): a group's grid need not be centred on zero.  The offset is stepped
    like a scale (``lq_is_scale``) but has no lower bound (no ``lq_constraint``); ``lq_is_offset`` tells it apart.
    ``element_format="fp4_e2m1" | ...`` (one of ops.ELEMENT_FORMATS; not in the reference) -> the OCP microscaling quantizer
    (ops.fq_forward_mx / fq_backward_mx): the elements lie on that minifloat grid under one scale per group, with
    ``scale_format="e8m0"`` (the default) the stored scale rounded to a power of two, with "fp32" the scale as it is.  It needs
    ``orientation="groupwise"`` (``group_size`` defaults to 32, the MX block) -- or "scalar", the one-group form the host layers
    give their biases -- and takes neither a range, a rounding, an offset nor a loss term; the gradients are the straight-through
    ones (``scale_gradient`` is "ste").  ``init_scale`` takes "mx" / "cover" (ops.scale_init_mx), ``quantized_integers`` returns
    the elements' encodings, the statistics are ``mx_stats`` (``quant_stats`` is the integer range's and raises).
    """

    _SCALE_NAMES = {"rowwise": "Rowwise-scaler", "columnwise": "Columnwise-scaler",
                    "channelwise": "Columnwise-scaler",      # sic, NQ-L:178
                    "scalar": "Scalar-scaler", "groupwise": "Groupwise-scaler"}

    def __init__(self, penalty_threshold=None, initializer=None, orientation="scalar", *, penalty_rate=None,
                 scale_gradient=None, grad_scale=1.0, bits=None, signed=True, q_range=None, rounding="floor", group_size=None,
                 asymmetric=False, element_format=None, scale_format="e8m0"):
        super().__init__()
        self.element_format = self.scale_format = None
        if element_format is not None:
            group_size = check_element_layer(element_format, scale_format, orientation, group_size, bits, signed, q_range, rounding,
                                             asymmetric, penalty_threshold, penalty_rate, scale_gradient, bias=orientation == "scalar")
            self.element_format, self.scale_format, scale_gradient = element_format, scale_format, "ste"
        self.q_range = ops.q_range_of(bits, signed, q_range)
        ops.check_rounding(rounding, self.q_range is not None)
        self.rounding = rounding
        self.asymmetric = check_asymmetric(asymmetric, orientation, self.q_range, penalty_threshold, penalty_rate, scale_gradient)
        self.group_size = group_size if element_format is not None else \
            check_groupwise(orientation, group_size, self.q_range, penalty_threshold, penalty_rate)
        if self.q_range is not None and penalty_threshold is not None:
            raise ValueError("a clipped layer (bits / q_range) needs penalty_threshold=None: the nested-quantization vote is "
                             "defined on the unclipped quantizer")
        if scale_gradient not in ops.SCALE_GRADIENTS:
            raise ValueError(f"scale_gradient must be one of {ops.SCALE_GRADIENTS}, got {scale_gradient!r}")
        if scale_gradient == "ste" and penalty_threshold is not None:
            raise ValueError('scale_gradient="ste" replaces the nested-quantization vote: it needs penalty_threshold=None')
        if grad_scale != "rsqrt_group":
            grad_scale = float(grad_scale)
        self.scale_gradient = scale_gradient
        self.grad_scale = grad_scale
        self.initializer = initializer
        self.orientation = orientation
        self.penalty_threshold = penalty_threshold
        self.penalty_rate = penalty_rate
        self.constraint = MinValueConstraint(SCALE_INIT)          # NQ-L:158
        self.scale: Optional[nn.Parameter] = None
        self.offset: Optional[nn.Parameter] = None      # asymmetric layers only
        self.scale_name: Optional[str] = None
        self.built = False
        self.defer_scale_grad = False          # set by DataParallel(mode="B"): ds is recomputed after the all-reduce

    def build(self, input_shape, device=None):
        if self.group_size is not None:
            shape = groupwise_scale_shape(tuple(input_shape), self.group_size)
        else:
            shape = scale_shape(tuple(input_shape), self.orientation)  # raises ValueError like NQ-L:194-197
        self.scale = nn.Parameter(torch.full(shape, SCALE_INIT, dtype=torch.float32, device=device))  # NQ-L:156
        self.scale.lq_constraint = self.constraint                 # found by optim.apply_constraints
        self.scale.lq_is_scale = True
        if self.asymmetric:
            self.offset = nn.Parameter(torch.zeros(shape, dtype=torch.float32, device=device))
            self.offset.lq_is_scale = True       # stepped by ScaleAdam; no lq_constraint: an offset has no lower bound
            self.offset.lq_is_offset = True
        if self.penalty_rate is not None and not hasattr(self, "penalty_rate_weight"):
            # the MNIST loss-term variant keeps the rate as a NON-trainable weight of the nested layer
            # (MNIST/custom_loss_terms/custom_components/custom_layers.py:97-102): a buffer here, saved with the model
            self.register_buffer("penalty_rate_weight", torch.tensor(float(self.penalty_rate), dtype=torch.float32, device=device))
        self.scale_name = self._SCALE_NAMES[self.orientation]
        self.built = True

    def grad_scale_value(self, parameter_numel: int) -> float:
        """The factor k of the straight-through scale gradient for a parameter of that many elements."""
        if self.grad_scale == "rsqrt_group":
            return 1.0 / math.sqrt(parameter_numel / self.scale.numel())
        return self.grad_scale

    def call(self, inputs):
        if not self.built:
            self.build(tuple(inputs.shape), device=inputs.device)
        if self.element_format is not None:
            if self.defer_scale_grad:
                raise ValueError("a layer with an element format with defer_scale_grad (data-parallel mode B): the all-reduced dP no "
                                 "longer holds the dy of its saturated elements, so ds cannot be recomputed from it")
            return ops.my_custom_gradient(inputs, self.scale, grad_scale=self.grad_scale_value(inputs.numel()),
                                          group_size=self.group_size, element_format=self.element_format, scale_format=self.scale_format)
        if self.asymmetric:
            if self.defer_scale_grad:
                raise ValueError("an asymmetric layer with defer_scale_grad (data-parallel mode B): the all-reduced dP of a clipped "
                                 "layer no longer holds the dy of its clipped elements, so neither ds nor db can be recomputed from it")
            return ops.my_custom_gradient(inputs, self.scale, scale_gradient="ste", grad_scale=self.grad_scale_value(inputs.numel()),
                                          q_range=self.q_range, rounding=self.rounding, group_size=self.group_size, offset=self.offset)
        if self.q_range is not None:
            return ops.my_custom_gradient(inputs, self.scale, self.penalty_threshold, scale_gradient=self.scale_gradient,
                                          grad_scale=self.grad_scale_value(inputs.numel()) if self.scale_gradient == "ste" else 1.0,
                                          defer_scale_grad=self.defer_scale_grad, q_range=self.q_range, rounding=self.rounding,
                                          group_size=self.group_size)
        if self.scale_gradient == "ste":
            return ops.my_custom_gradient(inputs, self.scale, scale_gradient="ste", grad_scale=self.grad_scale_value(inputs.numel()),
                                          defer_scale_grad=self.defer_scale_grad)
        if self.penalty_threshold is None:
            return ops.my_custom_gradient(inputs, self.scale)                        # CL-L:143-144
        return ops.my_custom_gradient(inputs, self.scale, self.penalty_threshold,   # NQ-L:199-200
                                      defer_scale_grad=self.defer_scale_grad)

    forward = call

    def extra_repr(self):
        r = f"orientation={self.orientation!r}, penalty_threshold={self.penalty_threshold}, penalty_rate={self.penalty_rate}"
        if self.scale_gradient is not None:
            r += f", scale_gradient={self.scale_gradient!r}, grad_scale={self.grad_scale!r}"
        if self.q_range is not None:
            r += f", q_range={self.q_range!r}"
        if self.rounding != "floor":
            r += f", rounding={self.rounding!r}"
        if self.group_size is not None:
            r += f", group_size={self.group_size}"
        if self.asymmetric:
            r += ", asymmetric=True"
        if self.element_format is not None:
            r += f", element_format={self.element_format!r}, scale_format={self.scale_format!r}"
        return r

    def init_scale(self, parameter, method):
        """Writes this layer's scale IN PLACE from ``parameter`` (ops.scale_init_group; ``method`` one of ops.SCALE_INITS) with
        the layer's range, rounding and group size and the ``min_value`` of its constraint.  The unbounded quantizer has nothing
        to cover: ValueError without a range.  One launch, no synchronisation.
        An asymmetric layer also takes "minmax" (ops.scale_init_group_minmax: scale and offset from each group's minimum and
        maximum); under the other methods its scale is written as a symmetric layer's and its offset is set to zero.
        A layer with an element format takes "mx" (the OCP rule) and "cover" (nothing saturates) instead: ops.scale_init_mx."""
        if self.element_format is not None:
            ops.check_mx_scale_init(method)
            if not self.built:
                self.build(tuple(parameter.shape), device=parameter.device)
            with torch.no_grad():
                ops.scale_init_mx(parameter.detach(), self.scale.data, self.element_format, self.group_size, method,
                                  min_value=self.constraint.min_value)
            return self.scale
        if method in ops.MX_SCALE_INITS:
            raise ValueError(f"scale_init {method!r} on a layer without an element format: it writes the power-of-two scale of a "
                             f"microscaling block; an integer layer takes one of {ops.LAYER_SCALE_INITS}")
        ops.check_layer_scale_init(method)
        if method == "minmax":
            if not self.asymmetric:
                raise ValueError('scale_init "minmax" on a symmetric layer: it places each group\'s range over [min, max] through an '
                                 "offset, which only an asymmetric=True layer has")
            ops.check_minmax_range(*self.q_range)
            if not self.built:
                self.build(tuple(parameter.shape), device=parameter.device)
            with torch.no_grad():
                ops.scale_init_group_minmax(parameter.detach(), self.scale.data, self.offset.data, *self.q_range, self.group_size,
                                            rounding=self.rounding, min_value=self.constraint.min_value)
            return self.scale
        if self.q_range is None:
            raise ValueError("scale initialisation needs bits or q_range: the unbounded quantizer clips nothing, there is no range "
                             "for the scale to cover")
        if not self.built:
            self.build(tuple(parameter.shape), device=parameter.device)
        with torch.no_grad():
            ops.scale_init_group(parameter.detach(), self.scale.data, *self.q_range, self.group_size, method,
                                 rounding=self.rounding, min_value=self.constraint.min_value)
            if self.asymmetric:
                self.offset.data.zero_()
        return self.scale

    def quant_stats(self, parameter, want_hist=True):
        """Statistics of this layer's quantizer on ``parameter`` as the scale (and offset) stand now (ops.group_stats, with the
        layer's own range, rounding, group size and offset): an ops.GroupStats record of device tensors, to be read with
        ops.summarize_stats.  One launch, no synchronisation.  A layer without a range clips nothing and has no fixed set of
        codes: ValueError; its statistics are ops.q_minmax, ops.q_unique and ops.q_absmax_over_axis
        (tracking.NestedScaleTrackingCallback)."""
        if self.element_format is not None:
            raise ValueError("quant_stats on a layer with an element format: the statistics kernel bins the codes of an integer range; "
                             "a microscaling layer has none (its statistics are `mx_stats`)")
        if self.q_range is None:
            raise ValueError("quant_stats needs bits or q_range: the unbounded quantizer clips nothing and has no fixed set of codes; "
                             "its statistics are ops.q_minmax / ops.q_unique / ops.q_absmax_over_axis "
                             "(tracking.NestedScaleTrackingCallback)")
        if not self.built:
            raise ValueError("quant_stats before the layer is built: there is no scale yet")
        with torch.no_grad():
            return ops.group_stats(parameter.detach(), self.scale.data, *self.q_range, self.group_size,
                                   offset=self.offset.data if self.asymmetric else None, rounding=self.rounding, want_hist=want_hist)

    def mx_stats(self, parameter, want_hist=True):
        """Statistics of this layer's microscaling quantizer on ``parameter`` as the scale stands now (ops.mx_stats, with the
        layer's own element format, scale format and group size): an ops.MxStats record of device tensors, to be read with
        ops.summarize_mx_stats.  One launch, no synchronisation.  A layer without an element format: ValueError; its statistics
        are ``quant_stats``."""
        if self.element_format is None:
            raise ValueError("mx_stats on a layer without an element format: the statistics of an integer range are quant_stats")
        if not self.built:
            raise ValueError("mx_stats before the layer is built: there is no scale yet")
        with torch.no_grad():
            return ops.mx_stats(parameter.detach(), self.scale.data, self.element_format, self.group_size, self.scale_format,
                                want_hist=want_hist)

    def quantized_integers(self, parameter, dtype=torch.float32):
        """The integer view of ``parameter`` under this layer's quantizer: floor(P/s), clamped when the layer has a range (then
        rint(P/s) for ``rounding="nearest"``).  With an element format: the elements' encodings (the code view)."""
        if self.element_format is not None:
            return ops.fq_forward_mx(parameter, self.scale.data, self.element_format, self.group_size, self.scale_format,
                                     q_dtype=dtype)[1]
        if self.q_range is None:
            return ops.quantized_integers(parameter, self.scale.data, dtype)
        if self.asymmetric:
            return ops.fq_forward_group_affine(parameter, self.scale.data, self.offset.data, *self.q_range, self.group_size,
                                               q_dtype=dtype, rounding=self.rounding)[1]
        if self.group_size is not None:
            return ops.fq_forward_group(parameter, self.scale.data, *self.q_range, self.group_size, q_dtype=dtype,
                                        rounding=self.rounding)[1]
        return ops.fq_forward_clip(parameter, self.scale.data, *self.q_range, q_dtype=dtype, rounding=self.rounding)[1]


def check_asymmetric(asymmetric, orientation, q_range, penalty_threshold=None, penalty_rate=None, scale_gradient="ste") -> bool:
    """``asymmetric`` as a bool, or ValueError naming the reason it cannot be had."""
    if not asymmetric:
        return False
    if orientation != "groupwise":
        raise ValueError(f'asymmetric=True needs orientation="groupwise", got orientation={orientation!r}: offsets exist per group; a '
                         "group_size of the line length or more gives per-channel offsets")
    if q_range is None:
        raise ValueError("asymmetric=True needs bits or q_range: the offset places a chosen integer range over each group")
    if penalty_threshold is not None:
        raise ValueError("asymmetric=True with a penalty_threshold: the nested-quantization vote is defined on the unclipped "
                         "symmetric quantizer")
    if penalty_rate is not None:
        raise ValueError("asymmetric=True with a loss term (penalty_rate): the penalty kernels know scales only, an offset would "
                         "get no gradient from them")
    if scale_gradient != "ste":
        raise ValueError('asymmetric=True needs scale_gradient="ste": the loss-term-only rule has no gradient for an offset')
    return True


def check_element_layer(element_format, scale_format, orientation, group_size, bits=None, signed=True, q_range=None, rounding="floor",
                        asymmetric=False, penalty_threshold=None, penalty_rate=None, scale_gradient="ste", bias=False):
    """The group size of a layer with an ``element_format`` (None for ``bias``, the scalar one-group form), or ValueError naming
    what does not go with a microscaling format."""
    ops.check_element_format(element_format)
    ops.check_scale_format(scale_format)
    if bits is not None or q_range is not None or not signed:
        raise ValueError(f"element_format={element_format!r} with bits / q_range / signed: an element format brings its own grid, "
                         "range and sign")
    if rounding != "floor":
        raise ValueError(f"element_format={element_format!r} with rounding={rounding!r}: a minifloat grid rounds to nearest, ties to "
                         "even, and nothing else; leave rounding at its default")
    if asymmetric:
        raise ValueError(f"element_format={element_format!r} with asymmetric=True: the microscaling formats are symmetric, a block "
                         "has a scale and no offset")
    if penalty_threshold is not None:
        raise ValueError(f"element_format={element_format!r} with a penalty_threshold: the nested-quantization vote is defined on "
                         "the unclipped integer quantizer")
    if penalty_rate is not None:
        raise ValueError(f"element_format={element_format!r} with a loss term (penalty_rate): the penalty kernels know the integer "
                         "quantizer with one-axis scales only")
    if scale_gradient not in (None, "ste"):
        raise ValueError(f'element_format={element_format!r} needs scale_gradient="ste", got {scale_gradient!r}')
    if bias:
        if orientation != "scalar" or group_size is not None:
            raise ValueError("the bias of a layer with an element format is one group under a scalar scale")
        return None
    if orientation != "groupwise":
        raise ValueError(f'element_format={element_format!r} needs orientation="groupwise", got orientation={orientation!r}: a '
                         "microscaling scale belongs to a block of consecutive elements")
    if group_size is None:
        return ops.MX_GROUP_SIZE
    if isinstance(group_size, bool) or int(group_size) != group_size or int(group_size) < 1:
        raise ValueError(f"group_size must be an integer >= 1, got {group_size!r}")
    return int(group_size)


def check_groupwise(orientation, group_size, q_range, penalty_threshold=None, penalty_rate=None):
    """The ``group_size`` of a layer as an int (None for the reference's orientations), or ValueError naming the reason."""
    if orientation != "groupwise":
        if group_size is not None:
            raise ValueError(f'group_size needs orientation="groupwise", got orientation={orientation!r}')
        return None
    if group_size is None:
        raise ValueError('orientation="groupwise" needs group_size (elements per scale)')
    if isinstance(group_size, bool) or int(group_size) != group_size or int(group_size) < 1:
        raise ValueError(f"group_size must be an integer >= 1, got {group_size!r}")
    if q_range is None:
        raise ValueError('orientation="groupwise" needs bits or q_range: group-wise scales exist for the clipped quantizer only')
    if penalty_threshold is not None:
        raise ValueError('orientation="groupwise" with a penalty_threshold: the nested-quantization vote is defined on the '
                         "unclipped quantizer with one-axis scales")
    if penalty_rate is not None:
        raise ValueError('orientation="groupwise" with a loss term (penalty_rate): the penalty kernels broadcast one-axis scales')
    return int(group_size)


def _nested(penalty_threshold, penalty_rate, orientation, scale_gradient=None, grad_scale=1.0, q_range=None, rounding="floor",
            group_size=None, asymmetric=False, element_format=None, scale_format="e8m0"):
    return CustomQuantizedScaleLayer(penalty_threshold=penalty_threshold, initializer=None,
                                     orientation=orientation, penalty_rate=penalty_rate,
                                     scale_gradient=scale_gradient, grad_scale=grad_scale, q_range=q_range,
                                     rounding=rounding, group_size=group_size, asymmetric=asymmetric,
                                     element_format=element_format, scale_format=scale_format)


def _as_tensor(a, shape, device):
    t = torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a, dtype=torch.float32)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"trained weight has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.to(device).contiguous()


class _HostLayer(nn.Module):
    q_range = None
    rounding = "floor"
    group_size = None
    asymmetric = False
    element_format = None
    scale_format = None

    def _element_args(self, element_format, scale_format, orientation, group_size, bits, signed, q_range, rounding, asymmetric,
                      penalty_threshold, penalty_rate, scale_gradient):
        """Constructor half of ``element_format``: checks it against everything else and returns the group size (unchanged without
        a format)."""
        if element_format is None:
            return group_size
        gs = check_element_layer(element_format, scale_format, orientation, group_size, bits, signed, q_range, rounding, asymmetric,
                                 penalty_threshold, penalty_rate, scale_gradient)
        self.element_format, self.scale_format = element_format, scale_format
        return gs

    def _nested_quantizers(self):
        return [getattr(self, n) for n in ("nested_q_k_layer", "nested_q_w_layer", "nested_q_b_layer") if hasattr(self, n)]

    def make_mx(self, element_format, scale_format="e8m0", group_size=None):
        """Switches both quantizers of a constructed layer to the microscaling ``element_format``: the kernel / ``W`` group-wise
        with ``group_size`` (32 by default), the bias as one group under its scalar scale; rebuilds the weight's scale
        (models.build_model applies it after construction)."""
        conv = hasattr(self, "nested_q_k_layer")
        nested = self.weight_nested()
        gs = check_element_layer(element_format, scale_format, "groupwise", group_size, None, True, self.q_range, self.rounding,
                                 self.asymmetric, nested.penalty_threshold, nested.penalty_rate, nested.scale_gradient)
        if conv and self.kernel_storage != "oihw":
            raise ValueError(f'element_format={element_format!r} with kernel_storage="hwio": the blocks are defined in the '
                             'convolution\'s memory order (the contiguous (ci, kh, kw) run of an output channel); store the kernel "oihw"')
        self.element_format, self.scale_format, self.group_size = element_format, scale_format, gs
        for n in self._nested_quantizers():
            n.element_format, n.scale_format, n.scale_gradient = element_format, scale_format, "ste"
        nested.group_size, nested.orientation = gs, "groupwise"
        if nested.built:
            param = self.kernel if conv else self.W
            nested.build(tuple(param.shape), device=param.device)

    def extra_repr(self):
        r = f"q_range={self.q_range!r}" if self.q_range is not None else ""
        if self.element_format is not None:
            r += f"element_format={self.element_format!r}, scale_format={self.scale_format!r}"
        if self.rounding != "floor":
            r += f", rounding={self.rounding!r}"
        if self.group_size is not None:
            r += f", group_size={self.group_size}"
        if self.asymmetric:
            r += ", asymmetric=True"
        return r

    def weight_nested(self):
        """The nested layer of the kernel / ``W`` (the one that may be group-wise and asymmetric; the bias never is)."""
        return self.nested_q_k_layer if hasattr(self, "nested_q_k_layer") else self.nested_q_w_layer

    def make_asymmetric(self):
        """Gives the weight quantizer of a constructed group-wise layer an offset per group (models.build_model applies it after
        ``make_groupwise``); the bias stays symmetric and scalar."""
        nested = self.weight_nested()
        check_asymmetric(True, nested.orientation, self.q_range, nested.penalty_threshold, nested.penalty_rate, nested.scale_gradient)
        self.asymmetric = nested.asymmetric = True
        if nested.built:
            param = self.kernel if hasattr(self, "nested_q_k_layer") else self.W
            nested.build(tuple(param.shape), device=param.device)

    def make_groupwise(self, group_size):
        """Switches the weight quantizer of a constructed layer to ``orientation="groupwise"`` with this ``group_size`` and
        rebuilds its scale (models.build_model applies ranges and group sizes after construction); the bias stays scalar."""
        conv = hasattr(self, "nested_q_k_layer")
        nested = self.nested_q_k_layer if conv else self.nested_q_w_layer
        gs = check_groupwise("groupwise", group_size, self.q_range, nested.penalty_threshold, nested.penalty_rate)
        if conv and self.kernel_storage != "oihw":
            raise ValueError('orientation="groupwise" with kernel_storage="hwio": the groups are defined in the convolution\'s memory '
                             'order (the contiguous (ci, kh, kw) run of an output channel); store the kernel "oihw"')
        self.group_size = nested.group_size = gs
        nested.orientation = "groupwise"
        if nested.built:
            param = self.kernel if conv else self.W
            nested.build(tuple(param.shape), device=param.device)

    def scale_pairs(self):
        """[(what, nested layer, parameter)] of this layer's quantised tensors."""
        conv = hasattr(self, "nested_q_k_layer")
        pairs = [("kernel", self.nested_q_k_layer, self.kernel)] if conv else [("W", self.nested_q_w_layer, self.W)]
        if hasattr(self, "nested_q_b_layer"):
            pairs.append(("b", self.nested_q_b_layer, self.b))
        return pairs

    def init_scales(self, method):
        """``CustomQuantizedScaleLayer.init_scale`` for the kernel / ``W`` and the bias of a built layer."""
        if self.element_format is not None:
            ops.check_mx_scale_init(method)
            if not self.built:
                raise ValueError(f"{self.name}: scale initialisation reads the weights; build the layer first")
            for _, nested, param in self.scale_pairs():
                nested.init_scale(param, method)
            return
        if method in ops.MX_SCALE_INITS:
            raise ValueError(f"{self.name}: scale_init {method!r} on a layer without an element format: it writes the power-of-two "
                             f"scale of a microscaling block; an integer layer takes one of {ops.LAYER_SCALE_INITS}")
        ops.check_layer_scale_init(method)
        if method == "minmax" and not self.asymmetric:
            raise ValueError(f'{self.name}: scale_init "minmax" on a symmetric layer: it places each group\'s range over [min, max] '
                             "through an offset, which only an asymmetric=True layer has")
        if method == "minmax":
            ops.check_minmax_range(*self.q_range)
        if not self.built:
            raise ValueError(f"{self.name}: scale initialisation reads the weights; build the layer first")
        for _, nested, param in self.scale_pairs():
            # the bias of an asymmetric layer is symmetric and scalar: "absmax" covers it under "minmax"
            nested.init_scale(param, "absmax" if method == "minmax" and not nested.asymmetric else method)

    def _init_value(self, initializer, shape, device):
        if initializer is None:
            raise ValueError("initializer is required when trained_weights is not given")
        v = initializer(shape)
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(np.asarray(v), dtype=torch.float32)
        return v.to(dtype=torch.float32, device=device).contiguous()

    def regularization_loss(self) -> Optional[torch.Tensor]:
        """Keras adds regularizer(variable) of every regularised weight to the loss (NQ-L:251,259)."""
        if self.regularizer is None or not self.built:
            return None
        total = None
        for w in self._regularized():
            r = self.regularizer(w)
            total = r if total is None else total + r
        return total


class _MatrixFamily(NamedTuple):
    """One hardware matrix path as the layers use it.  ``act`` below is the family's activation arguments: (act_format, act_scale)
    of the block-scaled path, (act_block,) of the int8 path."""
    hw: str                   # the layer attribute under which a context manager parks (operand, bias, *act)
    operand: str              # the layer method that packs the kernel
    quantize: Callable        # (matrix, *act) -> operand
    im2col: Callable          # (x, kernel_size, strides, padding, *act) -> operand
    decode: Callable          # operand -> fp32 matrix
    gemm: Callable            # (a, b, bias, out) -> fp32 matrix
    operand_type: type        # what ``quantize`` and the epilogue return: a layer multiplies an input of this type as it is
    gemm_quantize: Callable   # (a, b, bias, activation, out, act) -> the next layer's operand: the operand-out epilogue
    out_name: str             # the argument of call_mx / call_i8 that asks for the epilogue
    chain: str                # the module method that states a Dense tail for the family's fused path
    fused: str                # the module attribute under which a context manager parks ``(act, keywords)`` for that tail

    def product(self, a, operand, qb, out=None):
        """``a`` times the layer's ``operand`` plus ``qb`` on the matrix instruction -- or, where ``operand`` is a tensor (the
        fake-quantised kernel as a (K, out) matrix: ``emulate=True``), the decoded ``a`` times it by ``torch.matmul``."""
        if not isinstance(operand, torch.Tensor):
            return self.gemm(a, operand, qb, out=out)
        y = torch.matmul(self.decode(a), operand, out=out)
        return y if qb is None else y.add_(qb)


_MX = _MatrixFamily("_mx_hw", "mx_operand", ops.mx_operand_quantize, ops.mx_operand_im2col, ops.mx_operand_decode, ops.mx_gemm,
                    ops.MxOperand, lambda a, b, bias, activation, out, act: ops.mx_gemm_quantize(a, b, bias, activation, out, act[1]),
                    "out_format", "mx_chain", "_mx_fused")
_I8 = _MatrixFamily("_i8_hw", "i8_operand", ops.i8_operand_quantize, ops.i8_operand_im2col, ops.i8_operand_decode, ops.i8_gemm,
                    ops.I8Operand, lambda a, b, bias, activation, out, act: ops.i8_gemm_quantize(a, b, bias, activation, out),
                    "out_block", "i8_chain", "_i8_fused")


def _check_max_lines(max_lines) -> None:
    if max_lines is not None and (not isinstance(max_lines, int) or isinstance(max_lines, bool) or max_lines < 1):
        raise ValueError(f"max_lines must be a positive integer or None, got {max_lines!r}")


class CustomDenseLayer(_HostLayer):
    """Standard dense layer with nested quantization layers for weights and bias (NQ-L:203-268)."""

    def __init__(self, seed=None, units=None, penalty_threshold=None, orientation="scalar", initializer=None,
                 name=None, regularizer=None, trained_weights=None, *, penalty_rate=None, input_shape=None,
                 device=None, scale_gradient=None, grad_scale=1.0, bits=None, signed=True, q_range=None, rounding="floor",
                 group_size=None, asymmetric=False, element_format=None, scale_format="e8m0", **kwargs):
        super().__init__()
        self.seed = seed
        group_size = self._element_args(element_format, scale_format, orientation, group_size, bits, signed, q_range, rounding,
                                        asymmetric, penalty_threshold, penalty_rate, scale_gradient)
        self.q_range = ops.q_range_of(bits, signed, q_range)      # None: the reference's unbounded quantizer
        ops.check_rounding(rounding, self.q_range is not None)
        self.rounding = rounding
        self.asymmetric = check_asymmetric(asymmetric, orientation, self.q_range, penalty_threshold, penalty_rate, scale_gradient)
        # groupwise: groups along `in` for every output column, scale (nb, out); the bias keeps its scalar scale
        self.group_size = group_size if element_format is not None else \
            check_groupwise(orientation, group_size, self.q_range, penalty_threshold, penalty_rate)
        self.nested_q_w_layer = _nested(penalty_threshold, penalty_rate, orientation, scale_gradient, grad_scale, self.q_range, rounding,
                                        self.group_size, self.asymmetric, element_format, scale_format)   # NQ-L:222-224
        self.nested_q_b_layer = _nested(penalty_threshold, penalty_rate, "scalar", scale_gradient, grad_scale, self.q_range, rounding,
                                        element_format=element_format, scale_format=scale_format)      # NQ-L:225-227
        self.units = units
        self.initializer = initializer
        self.regularizer = regularizer
        self.trained_weights = trained_weights
        self.name = _auto_name("custom_dense_layer")     # `name` is not forwarded in the reference (NQ-L:219)
        self.requested_name = name
        self.built = False
        if input_shape is not None:
            shape = (input_shape,) if isinstance(input_shape, int) else tuple(input_shape)
            self.build(shape, device=device)

    def build(self, input_shape, device=None):
        in_features = int(input_shape[-1])
        w_shape, b_shape = (in_features, self.units), (self.units,)                         # NQ-L:249,257
        if self.trained_weights:                                                            # NQ-L:240-245
            w = _as_tensor(self.trained_weights[0], w_shape, device)
            b = _as_tensor(self.trained_weights[1], b_shape, device)
        else:
            w = self._init_value(self.initializer, w_shape, device)
            b = self._init_value(self.initializer, b_shape, device)
        self.W = nn.Parameter(w)
        self.b = nn.Parameter(b)
        self.nested_q_w_layer.build(w_shape, device=device)
        self.nested_q_b_layer.build(b_shape, device=device)
        self.built = True

    def _regularized(self):
        return (self.W, self.b)

    def quantized_parameters(self):
        """(qW, qb) of this call: what FakeQuantBatch.quantize_all() left for the layer (one launch for all tensors, consumed
        once), else the nested layers' own ops (NQ-L:265-266)."""
        pre, self._q_pre = getattr(self, "_q_pre", None), None
        if pre is not None:
            return pre[0], pre[1]
        return self.nested_q_w_layer(self.W), self.nested_q_b_layer(self.b)

    def call(self, inputs):
        if not self.built:
            self.build(tuple(inputs.shape), device=inputs.device)
        for family in (_MX, _I8):
            hw = getattr(self, family.hw, None)
            if hw is not None and not self.training:              # inside layers.mx_hardware(...) / i8_hardware(...), eval mode
                self._q_pre = None                                # a batch's fake-quantised pair is not what this path multiplies
                return self._matrix_product(inputs, hw[0], hw[1], family, hw[2:])
        qw, qb = self.quantized_parameters()
        return torch.add(torch.matmul(inputs, qw), qb)           # NQ-L:268

    forward = call

    def _check_i8(self, offsets=False):
        """(qmin, qmax) of a layer that can run on the int8 matrix instruction, or ValueError naming the reason.  ``offsets=True``
        lets an asymmetric layer pass (ops.check_i8_operand_layer)."""
        q_range = ops.check_i8_operand_layer(self.q_range, self.nested_q_w_layer.orientation, self.group_size, self.asymmetric,
                                             self.element_format, self.W.shape[0] if self.built else None, offsets=offsets)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return q_range

    def i8_operand(self, offsets=False) -> "ops.I8Operand":
        """The kernel under its current scales as an operand of the int8 matrix instruction (ops.i8_operand_pack): ``units`` lines
        over K = in.  A "groupwise" layer passes its scale as it is; a "scalar" or "columnwise" layer its scale broadcast to
        ``(1, out)``, one group per output unit.  ValueError naming the reason for a layer without a range, with a range outside
        [-128, 127], with an offset, with "rowwise" scales, with an element format, or not built.
        ``offsets=True``: an asymmetric layer is packed with its ``(nb, out)`` scale and offset into an ops.I8AffineOperand, whose
        product adds the offset's row-sum term; a symmetric layer takes the path it always took."""
        qmin, qmax = self._check_i8(offsets)
        fan_in, units = self.W.shape
        scale = self.nested_q_w_layer.scale.data
        if self.nested_q_w_layer.orientation == "groupwise":
            gs = self.group_size
        else:
            scale, gs = scale.reshape(1, -1).expand(1, units).contiguous(), fan_in
        offset = self.nested_q_w_layer.offset.data if self.asymmetric else None
        return ops.i8_operand_pack(self.W.detach(), scale, qmin, qmax, gs, self.rounding, offset)

    def call_i8(self, inputs, act_block=0, out_block=None, activation=None, offsets=False):
        """The layer on the int8 matrix instruction, under ``no_grad``: the inputs quantised per row and ``act_block`` consecutive
        inputs (0: per row) to symmetric 8-bit integers (ops.i8_operand_quantize), multiplied with ``i8_operand()`` by ops.i8_gemm,
        plus the fake-quantised bias.  Inference only: there is no backward through this path.
        ``inputs`` may be an ops.I8Operand (``lines`` rows over ``K`` = in), which is multiplied as it is; ``act_block`` is then not
        read.  With ``out_block`` (64) the result is not the fp32 matrix but the NEXT layer's operand, ``activation`` (None or
        "relu") applied and quantised per row and block of 64 by the product's own epilogue (ops.i8_gemm_quantize): one launch, no
        fp32 activation in memory.  ``offsets=True`` lets an asymmetric layer run (``i8_operand(offsets=True)``)."""
        given = isinstance(inputs, ops.I8Operand)
        if not given:
            ops.check_i8_block(act_block)
        if not self.built:
            if given:
                raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
            self.build(tuple(inputs.shape), device=inputs.device)
        if given:
            self._check_operand_input(inputs)
        if out_block is not None:
            ops.check_i8_out_block(out_block)
        ops.check_activation(activation)
        with torch.no_grad():
            return self._matrix_product(inputs, self.i8_operand(offsets), self.nested_q_b_layer(self.b), _I8, (act_block,), out_block,
                                        activation)

    def mx_operand(self) -> "ops.MxOperand":
        """The kernel under its current scales as an operand of the block-scaled matrix instruction (ops.mx_operand_pack): ``units``
        lines over K = in.  ValueError naming the reason for a layer without an element format, with ``scale_format="fp32"``, with
        an fp6 format or with a group size other than 32."""
        ops.check_mx_operand_layer(self.element_format, self.scale_format, self.group_size)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return ops.mx_operand_pack(self.W.detach(), self.nested_q_w_layer.scale.data, self.element_format, self.group_size,
                                   self.scale_format)

    def _check_operand_input(self, operand):
        if operand.K != self.W.shape[0]:
            raise ValueError(f"{self.name}: the input operand reduces over K = {operand.K}, the layer over in = {self.W.shape[0]}")

    def _matrix_product(self, inputs, operand, qb, family, act, out=None, activation=None):
        """``out`` (the family's out_format / out_block) and ``activation``: the operand-out epilogue.  An input of the family's
        operand type is multiplied as it is."""
        with torch.no_grad():
            if isinstance(inputs, family.operand_type):      # a previous layer's epilogue wrote it: used as it is
                self._check_operand_input(inputs)
                a, lead = inputs, (inputs.lines,)
            else:
                a, lead = family.quantize(inputs.reshape(-1, inputs.shape[-1]), *act), tuple(inputs.shape[:-1])
            if out is None:
                if activation is not None:
                    raise ValueError(f"{self.name}: activation={activation!r} is fused into the operand-out epilogue: give "
                                     f"{family.out_name}")
                y = family.product(a, operand, qb)
                return y.reshape(*lead, y.shape[-1])
            if isinstance(operand, torch.Tensor):
                raise ValueError(f"{self.name}: the emulated path has no operand-out epilogue ({family.out_name}={out!r})")
            return family.gemm_quantize(a, operand, qb, activation, out, act)

    def call_mx(self, inputs, act_format="fp8_e4m3", act_scale="mx", out_format=None, activation=None):
        """The layer on the block-scaled matrix instruction, under ``no_grad``: the inputs quantised per block of 32 along their last
        axis (``act_format`` elements under the ``act_scale`` rule, ops.mx_operand_quantize), multiplied with ``mx_operand()`` by
        ops.mx_gemm, plus the fake-quantised bias.  Inference only: there is no backward through this path.
        ``inputs`` may be an ops.MxOperand (``lines`` rows over ``K`` = in), which is multiplied as it is.  With ``out_format`` the
        result is not the fp32 matrix but the NEXT layer's operand, ``activation`` (None or "relu") applied and quantised under
        ``act_scale`` by the product's own epilogue (ops.mx_gemm_quantize): one launch, no fp32 activation in memory."""
        if not self.built:
            if isinstance(inputs, ops.MxOperand):
                raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
            self.build(tuple(inputs.shape), device=inputs.device)
        if isinstance(inputs, ops.MxOperand):
            self._check_operand_input(inputs)
        if out_format is not None:
            ops.check_mx_operand_format(out_format)
        ops.check_mx_activation(activation)
        with torch.no_grad():
            return self._matrix_product(inputs, self.mx_operand(), self.nested_q_b_layer(self.b), _MX, (act_format, act_scale),
                                        out_format, activation)


_KERNEL_STORAGE = ["oihw"]


class default_kernel_storage:
    """``with default_kernel_storage("hwio"): model = build_model(...)`` -- the memory order of conv kernels built inside."""

    def __init__(self, storage: str):
        if storage not in ("oihw", "hwio"):
            raise ValueError("kernel_storage must be 'oihw' or 'hwio'")
        self.storage = storage

    def __enter__(self):
        _KERNEL_STORAGE.append(self.storage)
        return self

    def __exit__(self, *exc):
        _KERNEL_STORAGE.pop()
        return False


def _pair(v) -> Tuple[int, int]:
    if isinstance(v, int):
        return (v, v)
    v = tuple(int(x) for x in v)
    return v if len(v) == 2 else (v[0], v[0])


def _same_padding(size: int, k: int, s: int) -> Tuple[int, int]:
    """TensorFlow 'SAME': total = max((ceil(n/s)-1)*s + k - n, 0), extra pixel goes after."""
    out = math.ceil(size / s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


class _ConvBase(_HostLayer):
    _prefix = "custom_conv2d_layer"
    _has_bias = True

    def __init__(self, seed=None, penalty_threshold=None, orientation="scalar", initializer=None, filters=None,
                 kernel_size=(3, 3), strides=(1, 1), padding="same", name=None, regularizer=None,
                 trained_weights=None, *, penalty_rate=None, input_shape=None, data_format="NCHW", device=None,
                 kernel_storage=None, scale_gradient=None, grad_scale=1.0, bits=None, signed=True, q_range=None, rounding="floor",
                 group_size=None, asymmetric=False, element_format=None, scale_format="e8m0", **kwargs):
        super().__init__()
        self.seed = seed
        group_size = self._element_args(element_format, scale_format, orientation, group_size, bits, signed, q_range, rounding,
                                        asymmetric, penalty_threshold, penalty_rate, scale_gradient)
        self.q_range = ops.q_range_of(bits, signed, q_range)      # None: the reference's unbounded quantizer
        ops.check_rounding(rounding, self.q_range is not None)
        self.rounding = rounding
        self.asymmetric = check_asymmetric(asymmetric, orientation, self.q_range, penalty_threshold, penalty_rate, scale_gradient)
        if kernel_storage is None:
            kernel_storage = _KERNEL_STORAGE[-1]
        if kernel_storage not in ("oihw", "hwio"):
            raise ValueError("kernel_storage must be 'oihw' or 'hwio'")
        self.kernel_storage = kernel_storage
        # groupwise: groups along the (ci, kh, kw) memory run of every output channel, scale (co, nb); the bias stays scalar
        self.group_size = group_size if element_format is not None else \
            check_groupwise(orientation, group_size, self.q_range, penalty_threshold, penalty_rate)
        if self.group_size is not None and kernel_storage != "oihw":
            raise ValueError('orientation="groupwise" with kernel_storage="hwio": the groups are defined in the convolution\'s memory '
                             'order (the contiguous (ci, kh, kw) run of an output channel); store the kernel "oihw"')
        self.nested_q_k_layer = _nested(penalty_threshold, penalty_rate, orientation, scale_gradient, grad_scale, self.q_range, rounding,
                                        self.group_size, self.asymmetric, element_format, scale_format)      # NQ-L:293-295
        if self._has_bias:
            self.nested_q_b_layer = _nested(penalty_threshold, penalty_rate, "scalar", scale_gradient, grad_scale, self.q_range, rounding,
                                            element_format=element_format, scale_format=scale_format)     # NQ-L:296-298
        self.initializer = initializer
        self.filters = filters
        self.kernel_size = _pair(kernel_size)
        self.strides = _pair(strides)
        self.padding = str(padding).upper()                                                # NQ-L:305
        if self.padding not in ("SAME", "VALID"):
            raise ValueError(f"padding must be 'same' or 'valid', got {padding!r}")
        self.regularizer = regularizer
        self.trained_weights = trained_weights
        self.name = _auto_name(self._prefix)      # conv forwards **kwargs but not `name` (NQ-L:290)
        self.requested_name = name
        if data_format not in ("NCHW", "NHWC"):
            raise ValueError("data_format must be 'NCHW' or 'NHWC'")
        self.data_format = data_format
        self.built = False
        if input_shape is not None:
            ci = input_shape if isinstance(input_shape, int) else (
                input_shape[-1] if data_format == "NHWC" else input_shape[-3])
            self._build_channels(int(ci), device)

    def build(self, input_shape, device=None):
        ci = input_shape[-1] if self.data_format == "NHWC" else input_shape[-3]
        self._build_channels(int(ci), device)

    def _build_channels(self, ci: int, device):
        kernel_shape = (*self.kernel_size, ci, self.filters)                               # NQ-L:321  HWIO
        if self.trained_weights:                                                           # NQ-L:314-319
            k = _as_tensor(self.trained_weights[0], kernel_shape, device)
            b = _as_tensor(self.trained_weights[1], (self.filters,), device) if self._has_bias else None
        else:
            k = self._init_value(self.initializer, kernel_shape, device)
            b = self._init_value(self.initializer, (self.filters,), device) if self._has_bias else None
        if self.kernel_storage == "oihw":          # same shape and values, elements in (co, ci, kh, kw) order
            k = k.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)
        self.kernel = nn.Parameter(k)
        self.nested_q_k_layer.build(kernel_shape, device=device)
        if self._has_bias:
            self.b = nn.Parameter(b)
            self.nested_q_b_layer.build((self.filters,), device=device)
        self.built = True

    def _regularized(self):
        return (self.kernel, self.b) if self._has_bias else (self.kernel,)

    def quantized_parameters(self):
        """(w, qb) of this call: ``w`` is the fake-quantised kernel as the OIHW-shaped tensor the convolution consumes (NQ-L:340),
        ``qb`` the fake-quantised bias (NQ-L:341; None without one) -- from FakeQuantBatch.quantize_all() when it ran (one launch
        for all tensors, consumed once), else from the nested layers' own ops."""
        pre, self._q_pre = getattr(self, "_q_pre", None), None
        nested = self.nested_q_k_layer
        if pre is not None and len(pre) > 2 and pre[2] is not None:
            w = pre[2]                                   # the batch emitted the OIHW companion with the same launch
        elif pre is not None:
            w = pre[0].permute(3, 2, 0, 1)                                                 # HWIO -> OIHW view
        elif (self.kernel_storage == "hwio" and nested.built and nested.penalty_threshold is not None
              and self.kernel.is_cuda and self.kernel.is_contiguous()):
            # NQ-L:340 with K1 writing the OIHW tensor MIOpen consumes (and K2 reading its OIHW weight gradient): same
            # values as nested(kernel).permute(3, 2, 0, 1), without the two transposition launches
            w = ops.my_custom_gradient_oihw(self.kernel, nested.scale, nested.penalty_threshold,
                                            defer_scale_grad=nested.defer_scale_grad)
        else:
            # NQ-L:340; HWIO -> OIHW view -- contiguous when the kernel is stored "oihw": MIOpen takes it as it is and its
            # weight gradient comes back with the parameter's own strides
            w = nested(self.kernel).permute(3, 2, 0, 1)
        if not self._has_bias:
            return w, None
        return w, (pre[1] if pre is not None else self.nested_q_b_layer(self.b))

    def call(self, inputs):
        if not self.built:
            self.build(tuple(inputs.shape), device=inputs.device)
        for family in (_MX, _I8):
            hw = getattr(self, family.hw, None)
            if hw is not None and not self.training:              # inside layers.mx_hardware / i8_hardware(..., convs=True), eval mode
                self._q_pre = None                                # a batch's fake-quantised pair is not what this path multiplies
                return self._matrix_conv(inputs, hw[0], hw[1], family, hw[2:])
        x = inputs.permute(0, 3, 1, 2) if self.data_format == "NHWC" else inputs
        w, qb = self.quantized_parameters()
        if self.padding == "SAME":
            ph = _same_padding(x.shape[-2], self.kernel_size[0], self.strides[0])
            pw = _same_padding(x.shape[-1], self.kernel_size[1], self.strides[1])
            if ph[0] == ph[1] and pw[0] == pw[1]:
                y = F.conv2d(x, w, None, self.strides, (ph[0], pw[0]))
            else:
                y = F.conv2d(F.pad(x, (pw[0], pw[1], ph[0], ph[1])), w, None, self.strides, 0)
        else:
            y = F.conv2d(x, w, None, self.strides, 0)                                      # NQ-L:343-348
        if qb is not None:
            y = torch.add(y, qb.view(1, -1, 1, 1))                                         # NQ-L:350
        return y.permute(0, 2, 3, 1) if self.data_format == "NHWC" else y

    forward = call

    def mx_operand(self) -> "ops.MxOperand":
        """The kernel under its current scales as an operand of the block-scaled matrix instruction (ops.mx_operand_pack, blocks
        along the contiguous axis): ``filters`` lines over K = ci kh kw, the reduction order of ops.mx_operand_im2col.  ValueError
        naming the reason for ``kernel_storage="hwio"``, for a layer without an element format, with ``scale_format="fp32"``, with an
        fp6 format or with a group size other than 32, and for a layer that is not built."""
        if self.kernel_storage != "oihw":
            raise ValueError(f'{self.name}: kernel_storage="hwio": the block-scaled GEMM reduces over the (ci, kh, kw) memory run of a '
                             'kernel stored "oihw"')
        ops.check_mx_operand_layer(self.element_format, self.scale_format, self.group_size)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return ops.mx_operand_pack(self.kernel.detach(), self.nested_q_k_layer.scale.data, self.element_format, self.group_size,
                                   self.scale_format)

    def _mx_padding(self, h: int, w: int) -> Tuple[int, int, int, int]:
        """(top, bottom, left, right) of this layer on an h x w input: TensorFlow 'SAME' (asymmetric where it is) or none.  Both
        matrix paths pad by it."""
        if self.padding != "SAME":
            return (0, 0, 0, 0)
        return (*_same_padding(h, self.kernel_size[0], self.strides[0]), *_same_padding(w, self.kernel_size[1], self.strides[1]))

    def _matrix_conv(self, inputs, operand, qb, family, act, max_lines=None):
        """The layer on ``family``'s matrix instruction: per run of whole images (ops.im2col_runs) the im2col operand of the
        inputs, times ``operand``, plus ``qb``, into its rows of the one result."""
        with torch.no_grad():
            if inputs.dim() != 4:
                raise ValueError(f"{self.name}: the input must have four axes, got shape {tuple(inputs.shape)}")
            x = inputs.permute(0, 3, 1, 2) if self.data_format == "NHWC" else inputs       # a view: the operand reads its strides
            padding = self._mx_padding(x.shape[2], x.shape[3])
            M, K, OH, OW = ops.mx_im2col_dims(x.shape, self.kernel_size, self.strides, padding)
            B, per = x.shape[0], OH * OW
            y = torch.empty((M, self.filters), dtype=torch.float32, device=x.device)
            for b0, b1 in ops.im2col_runs(B, per, K, max_lines):
                a = family.im2col(x[b0:b1], self.kernel_size, self.strides, padding, *act)
                family.product(a, operand, qb, out=y[b0 * per:b1 * per])
            y = y.view(B, OH, OW, self.filters)                   # the GEMM's [M][co] is NHWC: no transposition launch
            return y if self.data_format == "NHWC" else y.permute(0, 3, 1, 2)

    def _call_matrix(self, inputs, family, act, max_lines, **operand_kwargs):
        if not self.built:
            self.build(tuple(inputs.shape), device=inputs.device)
        with torch.no_grad():
            operand = getattr(self, family.operand)(**operand_kwargs)
            qb = self.nested_q_b_layer(self.b) if self._has_bias else None
            return self._matrix_conv(inputs, operand, qb, family, act, max_lines)

    def call_mx(self, inputs, act_format="fp8_e4m3", act_scale="mx", max_lines=None):
        """The layer on the block-scaled matrix instruction, under ``no_grad``: the im2col matrix of the inputs quantised per block
        of 32 along (ci, kh, kw) (``act_format`` elements under the ``act_scale`` rule) by ops.mx_operand_im2col -- TensorFlow 'SAME'
        padding as ``call`` pads, or 'VALID' -- multiplied with ``mx_operand()`` by ops.mx_gemm, plus the fake-quantised bias where
        the layer has one.  Inference only: there is no backward through this path.  The result is a view of the GEMM's (M, co)
        matrix: ``(B, co, OH, OW)`` with channels-last strides for ``data_format="NCHW"``, ``(B, OH, OW, co)`` for "NHWC".  A batch
        whose im2col matrix has 2^31 elements or more, more than 65535 * 64 lines or more than ``max_lines`` lines is cut into runs
        of whole images that write their rows of the one result; the result does not depend on the cut."""
        _check_max_lines(max_lines)
        ops.check_mx_operand_format(act_format)
        ops.check_mx_scale_init(act_scale)
        return self._call_matrix(inputs, _MX, (act_format, act_scale), max_lines)

    def _check_i8(self, offsets=False):
        """(qmin, qmax) of a conv layer that can run on the int8 matrix instruction, or ValueError naming the reason.
        ``offsets=True`` lets an asymmetric layer pass (ops.check_i8_conv_operand_layer)."""
        fan_in = self.kernel.shape[0] * self.kernel.shape[1] * self.kernel.shape[2] if self.built else None
        q_range = ops.check_i8_conv_operand_layer(self.q_range, self.nested_q_k_layer.orientation, self.group_size, self.asymmetric,
                                                  self.element_format, fan_in, self.kernel_storage, offsets=offsets)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return q_range

    def i8_operand(self, offsets=False) -> "ops.I8Operand":
        """The kernel under its current scales as an operand of the int8 matrix instruction (ops.i8_operand_pack, groups along the
        contiguous axis): ``filters`` lines over K = ci kh kw, the reduction order of ops.i8_operand_im2col.  A "groupwise" layer
        passes its scale as it is; a "scalar" layer its scale broadcast to ``(filters, 1)``, one group per output channel.
        ValueError naming the reason for a one-axis orientation, ``kernel_storage="hwio"``, a layer without a range, with a range
        outside [-128, 127], with an offset, with an element format, or not built.
        ``offsets=True``: an asymmetric layer is packed with its ``(co, nb)`` scale and offset into an ops.I8AffineOperand, whose
        product adds the offset's row-sum term (padded taps hold code 0 and add no offset); a symmetric layer takes the path it
        always took."""
        qmin, qmax = self._check_i8(offsets)
        K = self.kernel.numel() // self.filters
        scale = self.nested_q_k_layer.scale.data
        if self.nested_q_k_layer.orientation == "groupwise":
            gs = self.group_size
        else:
            scale, gs = scale.reshape(1, 1).expand(self.filters, 1).contiguous(), K
        offset = self.nested_q_k_layer.offset.data if self.asymmetric else None
        return ops.i8_operand_pack(self.kernel.detach(), scale, qmin, qmax, gs, self.rounding, offset)

    def call_i8(self, inputs, act_block=0, max_lines=None, offsets=False):
        """The layer on the int8 matrix instruction, under ``no_grad``: the im2col matrix of the inputs quantised per line and
        ``act_block`` consecutive k of (ci, kh, kw) (0: per line) to symmetric 8-bit integers by ops.i8_operand_im2col -- TensorFlow
        'SAME' padding as ``call`` pads, or 'VALID' -- multiplied with ``i8_operand()`` by ops.i8_gemm, plus the fake-quantised bias
        where the layer has one.  Inference only: there is no backward through this path.  The result is a view of the GEMM's
        (M, co) matrix: ``(B, co, OH, OW)`` with channels-last strides for ``data_format="NCHW"``, ``(B, OH, OW, co)`` for "NHWC".  A
        batch whose im2col matrix has 2^31 elements or more, more than 65535 * 64 lines or more than ``max_lines`` lines is cut into
        runs of whole images that write their rows of the one result; the result does not depend on the cut.  ``offsets=True``
        lets an asymmetric layer run (``i8_operand(offsets=True)``)."""
        _check_max_lines(max_lines)
        ops.check_i8_block(act_block)
        return self._call_matrix(inputs, _I8, (act_block,), max_lines, offsets=offsets)


class CustomConv2DLayer(_ConvBase):
    """Standard convolutional layer with nested quantization layers for kernel and bias (NQ-L:271-350)."""


class CustomConv2DLayerNoBias(_ConvBase):
    """Bias-free variant (paper_implementation custom_layers.py:299-365)."""
    _has_bias = False


def custom_layers_of(model: nn.Module):
    """The reference selects layers by name substring (experiment.py:73, custom_loss_terms/experiment.py:446)."""
    return [m for m in model.modules()
            if isinstance(m, (CustomDenseLayer, _ConvBase))]


def mx_hardware_eligible(layer: nn.Module) -> bool:
    """Whether ``layer`` takes the block-scaled GEMM under ``mx_hardware``: a built Dense layer with an fp4 / fp8 element format,
    E8M0 scales and blocks of 32.  Conv layers keep the fake-quantised path (no implicit GEMM is built)."""
    return (isinstance(layer, CustomDenseLayer) and layer.built and layer.element_format in ops.MX_OPERAND_FORMATS
            and layer.scale_format == "e8m0" and layer.group_size == ops.MX_GROUP_SIZE)


def mx_conv_eligible(layer: nn.Module) -> bool:
    """Whether ``layer`` takes the block-scaled GEMM under ``mx_hardware(convs=True)``: a built conv layer with an fp4 / fp8 element
    format, E8M0 scales, blocks of 32 and the kernel stored "oihw" (the blocks then run along the im2col operand's K)."""
    return (isinstance(layer, _ConvBase) and layer.built and layer.element_format in ops.MX_OPERAND_FORMATS
            and layer.scale_format == "e8m0" and layer.group_size == ops.MX_GROUP_SIZE and layer.kernel_storage == "oihw")


class _matrix_hardware:
    """Entry and exit of ``mx_hardware`` and ``i8_hardware``: the eligible Dense layers, then (``convs``) the eligible conv layers,
    get ``(operand, bias, *act)`` under the family's attribute -- built once, on entry -- and lose it on exit."""
    _family = _dense_eligible = _conv_eligible = None
    _opt_in = {}              # keywords of the eligibility tests and of the layers' operand method (i8_hardware: offsets)

    def __enter__(self):
        family, custom, opt_in = self._family, custom_layers_of(self.model), self._opt_in
        switching = [m for m in custom if self._dense_eligible(m, **opt_in)]
        switching += [m for m in custom if self._conv_eligible(m, **opt_in)] if self.convs else []
        self.layers = []
        with torch.no_grad():
            for m in switching:
                if not self.emulate:
                    weight = getattr(m, family.operand)(**opt_in)
                elif isinstance(m, _ConvBase):      # the fake-quantised kernel as the (K, co) matrix the decoded operand multiplies
                    weight = m.nested_q_k_layer(m.kernel).detach().permute(3, 2, 0, 1).reshape(m.filters, -1).t()
                else:
                    weight = m.nested_q_w_layer(m.W).detach()
                bias = m.nested_q_b_layer(m.b).detach() if getattr(m, "_has_bias", True) else None
                setattr(m, family.hw, (weight, bias, *self._act))
                self.layers.append(m)
        # fused: a module that states its Dense tail (the family's chain method) evaluates it through the family's dense chain
        self.fused_layers, self._fused_modules = [], []
        if self.fused:
            for mod in self.model.modules():
                chain = getattr(mod, family.chain)() if callable(getattr(mod, family.chain, None)) else []
                if len(chain) > 1 and all(self._dense_eligible(layer, **opt_in) and act in ops.MX_ACTIVATIONS
                                          for layer, act in chain):
                    setattr(mod, family.fused, (self._act, dict(opt_in)))      # the dense chain's arguments after the chain, and its keywords
                    self._fused_modules.append(mod)
                    self.fused_layers += [layer for layer, _ in chain]
        return self

    def __exit__(self, *exc):
        for mod in self._fused_modules:
            setattr(mod, self._family.fused, None)
        for m in self.layers:
            setattr(m, self._family.hw, None)
        return False


class mx_hardware(_matrix_hardware):
    """Context manager: inside it every eligible Dense layer of ``model`` (``mx_hardware_eligible``) computes its eval-mode ``call``
    as ``call_mx`` does -- activations quantised per block (``act_format``, ``act_scale``), the product on the block-scaled matrix
    instruction.  The operands and the fake-quantised biases are built ONCE, on entry, from the scales the layers have then;
    training-mode calls and every other layer keep the fake-quantised path.  ``layers`` lists the layers that switched.
    ``emulate=True`` is the yardstick of that path in stock arithmetic: the same quantised activations, decoded, times the
    fake-quantised kernel with ``torch.matmul`` -- what the block-scaled product is compared against.
    ``fused=True``: a module of ``model`` that states its Dense tail as ``mx_chain()`` -- [(layer, activation), ...] with nothing but
    relu between the layers, as models.MNISTDense does -- evaluates it in eval mode through ``mx_dense_chain``: every layer but the
    last writes the next layer's operand from its own epilogue, and no fp32 hidden activation exists.  Same bits as ``fused=False``.
    ``fused_layers`` lists the layers that fused; a model without such a tail (BatchNorm between its Dense layers) keeps the
    per-layer path and lists none.  ``emulate=True`` with ``fused=True`` is refused: the yardstick is the unfused path.
    ``convs=True``: every conv layer that can (``mx_conv_eligible``) switches its eval-mode ``call`` too, to what its ``call_mx``
    does -- the im2col operand of its input gathered and quantised in one launch (ops.mx_operand_im2col), times the kernel's
    operand, plus the fake-quantised bias; the result is a channels-last view for ``data_format="NCHW"``.  Operand and bias are
    built once, on entry, and the layer is listed in ``layers`` after the Dense layers.  Under ``emulate=True`` such a layer
    multiplies the decoded im2col operand with the fake-quantised kernel by ``torch.matmul`` instead.  Without ``convs`` (the
    default) conv layers keep the fake-quantised path."""

    _family, _dense_eligible, _conv_eligible = _MX, staticmethod(mx_hardware_eligible), staticmethod(mx_conv_eligible)

    def __init__(self, model: nn.Module, act_format="fp8_e4m3", act_scale="mx", emulate=False, fused=False, convs=False):
        ops.check_mx_operand_format(act_format)
        ops.check_mx_scale_init(act_scale)
        if emulate and fused:
            raise ValueError("mx_hardware: emulate=True with fused=True: the emulated path is the yardstick of the unfused path and "
                             "has no operand-out epilogue")
        self.model, self.act_format, self.act_scale, self.emulate, self.fused = model, act_format, act_scale, bool(emulate), bool(fused)
        self.convs, self._act = bool(convs), (act_format, act_scale)
        self.layers, self.fused_layers, self._fused_modules = [], [], []


def _passes_check_i8(layer: nn.Module, cls, offsets=False) -> bool:
    if not isinstance(layer, cls):
        return False
    try:
        layer._check_i8(offsets)
    except ValueError:
        return False
    return True


def i8_hardware_eligible(layer: nn.Module, offsets=False) -> bool:
    """Whether ``layer`` takes the int8 GEMM under ``i8_hardware``: a built Dense layer with a range inside [-128, 127], symmetric,
    with scalar, columnwise or groupwise scales (group size a multiple of 64, or the whole input) and no element format.  Conv
    layers are judged by ``i8_conv_eligible``.  ``offsets=True``: an asymmetric layer is eligible too."""
    return _passes_check_i8(layer, CustomDenseLayer, offsets)


def i8_conv_eligible(layer: nn.Module, offsets=False) -> bool:
    """Whether ``layer`` takes the int8 GEMM under ``i8_hardware(convs=True)``: a built conv layer with a range inside
    [-128, 127], symmetric, with a scalar scale or groupwise scales (group size a multiple of 64, or at least ci kh kw), no
    element format and the kernel stored "oihw" (the groups then run along the im2col operand's K).  ``offsets=True``: an
    asymmetric layer is eligible too."""
    return _passes_check_i8(layer, _ConvBase, offsets)


class i8_hardware(_matrix_hardware):
    """Context manager beside ``mx_hardware``: inside it every eligible Dense layer of ``model`` (``i8_hardware_eligible``) computes
    its eval-mode ``call`` as ``call_i8`` does -- activations quantised per row and ``act_block`` inputs to symmetric 8-bit
    integers, the product on the int8 matrix instruction.  The operands and the fake-quantised biases are built ONCE, on entry,
    from the scales the layers have then; training-mode calls and every other layer keep the fake-quantised path.  ``layers`` lists
    the layers that switched.  ``emulate=True`` is the yardstick of that path in stock arithmetic: the same quantised activations,
    decoded, times the fake-quantised kernel with ``torch.matmul`` in fp32.
    ``convs=True``: every conv layer that can (``i8_conv_eligible``) switches its eval-mode ``call`` too, to what its ``call_i8``
    does -- the im2col operand of its input gathered and quantised in one launch (ops.i8_operand_im2col), times the kernel's
    operand, plus the fake-quantised bias; the result is a channels-last view for ``data_format="NCHW"``.  Operand and bias are
    built once, on entry, and the layer is listed in ``layers`` after the Dense layers.  Under ``emulate=True`` such a layer
    multiplies the decoded im2col operand with the fake-quantised kernel as a (K, co) matrix by ``torch.matmul`` instead.  Without
    ``convs`` (the default) conv layers keep the fake-quantised path.
    ``fused=True``: a module of ``model`` that states its Dense tail as ``i8_chain()`` -- [(layer, activation), ...] with nothing but
    relu between the layers, as models.MNISTDense does -- evaluates it in eval mode through ``i8_dense_chain``: every layer but the
    last writes the next layer's operand from its own epilogue, and no fp32 hidden activation exists.  The epilogue writes scale
    blocks of 64, so ``fused=True`` needs ``act_block=64`` -- then the bits are those of ``fused=False`` -- and is refused with any
    other.  ``fused_layers`` lists the layers that fused.  ``emulate=True`` with ``fused=True`` is refused, as on ``mx_hardware``.
    ``offsets=True``: asymmetric layers (a learned offset per group) switch too, and ``layers`` lists them: their operand carries
    the offsets and their product adds the offset's row-sum term, which costs matrix instructions that a symmetric product does
    not pay -- hence the opt-in.  It combines with ``convs``, ``fused`` and ``emulate`` (which needs nothing new: it multiplies the
    decoded activation with the fake-quantised kernel); a symmetric model is bit-identical with or without it."""

    _family, _dense_eligible, _conv_eligible = _I8, staticmethod(i8_hardware_eligible), staticmethod(i8_conv_eligible)

    def __init__(self, model: nn.Module, act_block=0, emulate=False, convs=False, fused=False, offsets=False):
        self.offsets = bool(offsets)
        self._opt_in = {"offsets": True} if self.offsets else {}
        self.model, self.act_block, self.emulate, self.fused = model, ops.check_i8_block(act_block), bool(emulate), bool(fused)
        if self.fused and self.emulate:
            raise ValueError("i8_hardware: emulate=True with fused=True: the emulated path is the yardstick of the unfused path and "
                             "has no operand-out epilogue")
        if self.fused and self.act_block != ops.I8_OUT_BLOCK:
            raise ValueError(f"i8_hardware: fused=True with act_block={self.act_block}: the epilogue writes scale blocks of "
                             f"{ops.I8_OUT_BLOCK}, so the fused model would not be the unfused one; give act_block={ops.I8_OUT_BLOCK}")
        self.convs, self._act = bool(convs), (self.act_block,)
        self.layers, self.fused_layers, self._fused_modules = [], [], []


def _dense_chain(fn, family, gemm_name, check_layer, check_act, x, chain, act, out, **operand_kwargs):
    """The body of ``mx_dense_chain`` and ``i8_dense_chain``: the chain checked before any launch, ``x`` quantised once, every layer
    but the last through the family's operand-out epilogue (``out``), the last to fp32."""
    chain = list(chain)
    if not chain:
        raise ValueError(f"{fn}: the chain is empty")
    for k, (layer, activation) in enumerate(chain):
        if not isinstance(layer, CustomDenseLayer):
            raise ValueError(f"{fn}: layer {k} is a {type(layer).__name__}: only Dense layers run on the {gemm_name} GEMM")
        if not layer.built:
            raise ValueError(f"{fn}: {layer.name}: the layer is not built yet (no kernel to pack)")
        try:
            check_layer(layer)
            ops.check_activation(activation)
        except ValueError as e:
            raise ValueError(f"{fn}: {layer.name}: {e}") from None
        if k == len(chain) - 1 and activation is not None:
            raise ValueError(f"{fn}: {layer.name}: the last layer writes fp32 and takes no activation (got {activation!r}): "
                             "apply it to the result")
    check_act()
    with torch.no_grad():
        lead = tuple(x.shape[:-1])
        a = family.quantize(x.reshape(-1, x.shape[-1]), *act)
        for k, (layer, activation) in enumerate(chain):
            hw = getattr(layer, family.hw, None)
            if hw is not None and not isinstance(hw[0], torch.Tensor):
                operand, qb = hw[0], hw[1]
            else:
                operand, qb = getattr(layer, family.operand)(**operand_kwargs), layer.nested_q_b_layer(layer.b)
            last = k == len(chain) - 1
            a = layer._matrix_product(a, operand, qb, family, act, None if last else out, activation)
        return a.reshape(*lead, a.shape[-1])


def mx_dense_chain(x, chain, act_format="fp8_e4m3", act_scale="mx"):
    """``chain`` = [(layer, activation), ...]: Dense layers applied one after the other on the block-scaled matrix instruction, under
    ``no_grad``.  ``x`` is quantised once (ops.mx_operand_quantize); every layer but the last goes through ops.mx_gemm_quantize, which
    applies its activation (None or "relu") and writes the next layer's operand (``act_format`` under ``act_scale``) in the product's
    epilogue; the last goes through ops.mx_gemm to fp32 and takes no activation.  Bit for bit ``call_mx`` -> activation -> ``call_mx``
    ..., without the fp32 activations and their launches.  Inside ``mx_hardware`` the operands and biases built on its entry are
    used, otherwise they are built here.  ValueError naming the reason for a layer that cannot take the path
    (``mx_hardware_eligible``) or an activation other than None / "relu"."""
    def check_act():
        ops.check_mx_operand_format(act_format)
        ops.check_mx_scale_init(act_scale)
    return _dense_chain("mx_dense_chain", _MX, "block-scaled",
                        lambda layer: ops.check_mx_operand_layer(layer.element_format, layer.scale_format, layer.group_size), check_act,
                        x, chain, (act_format, act_scale), act_format)


def i8_dense_chain(x, chain, act_block=64, offsets=False):
    """``chain`` = [(layer, activation), ...]: Dense layers applied one after the other on the int8 matrix instruction, under
    ``no_grad``.  ``x`` is quantised once per row and ``act_block`` inputs (ops.i8_operand_quantize); every layer but the last goes
    through ops.i8_gemm_quantize, which applies its activation (None or "relu") and writes the next layer's operand, per row and
    block of 64, in the product's epilogue; the last goes through ops.i8_gemm to fp32 and takes no activation.  Bit for bit
    ``call_i8(act_block)`` -> activation -> ``call_i8(act_block=64)`` ..., without the fp32 activations and their launches.  Inside
    ``i8_hardware`` the operands and biases built on its entry are used, otherwise they are built here.  ValueError naming the
    reason for a layer that cannot take the path (``i8_hardware_eligible``) or an activation other than None / "relu".
    ``offsets=True`` lets asymmetric layers take the path (``i8_operand(offsets=True)``): the epilogue's product adds the offset
    term too, so the bits stay those of the unfused path."""
    opt_in = {"offsets": True} if offsets else {}
    return _dense_chain("i8_dense_chain", _I8, "int8", lambda layer: layer._check_i8(**opt_in),
                        lambda: ops.check_i8_block(act_block), x, chain, (act_block,), ops.I8_OUT_BLOCK, **opt_in)


def quantized_tensors(model: nn.Module):
    """(reference name, parameter, nested scale layer) of every quantized tensor -- kernel/W and bias of every custom layer,
    in module order.  The one walk the int8 file (log_scripts.py:74-79), the packed container (export.py) and ``quant_stats``
    use."""
    out = []
    for layer in model.modules():
        if isinstance(layer, _ConvBase):
            out.append((layer.name + "/W", layer.kernel, layer.nested_q_k_layer))
            if layer._has_bias:
                out.append((layer.name + "/b", layer.b, layer.nested_q_b_layer))
        elif isinstance(layer, CustomDenseLayer):
            out.append((layer.name + "/W", layer.W, layer.nested_q_w_layer))
            out.append((layer.name + "/b", layer.b, layer.nested_q_b_layer))
    return out


def _model_stats(model: nn.Module, want_hist, mx: bool) -> dict:
    """The walk of ``quant_stats`` (``mx=False``: the tensors without an element format) and ``mx_quant_stats`` (those with one):
    one launch per tensor, then every record to the host in one copy."""
    tensors = [t for t in quantized_tensors(model) if (t[2].element_format is not None) == mx]
    numels = [param.numel() for _, param, _ in tensors]
    if mx:
        records = [nested.mx_stats(param.data, want_hist) for _, param, nested in tensors]
        summaries = ops.summarize_mx_stats_many(records, numels, [nested.element_format for _, _, nested in tensors])
    else:
        for name, _, nested in tensors:      # before any launch
            if nested.q_range is None:
                raise ValueError(f"quant_stats: the quantizer of {name!r} has no range (bits / q_range); the unbounded quantizer's "
                                 "statistics are tracking.NestedScaleTrackingCallback's")
        # a range of more than ops.STATS_MAX_BINS codes has no histogram: its summary holds None for the two code statistics
        records = [nested.quant_stats(param.data, want_hist and nested.q_range[1] - nested.q_range[0] < ops.STATS_MAX_BINS)
                   for _, param, nested in tensors]
        summaries = ops.summarize_stats_many(records, numels)
    return {name: summary for (name, _, _), summary in zip(tensors, summaries)}


def quant_stats(model: nn.Module, want_hist=True) -> dict:
    """{reference name: summary} of every quantized tensor of ``model`` (``quantized_tensors``' walk): the
    ops.summarize_stats dict of the tensor's ``CustomQuantizedScaleLayer.quant_stats``.  One launch per tensor, then all records
    go to the host together in one copy (one synchronisation: call it between steps, never inside a capture).  Every layer
    needs a range: ValueError otherwise.  Tensors of layers with an element format are skipped: the statistics kernel bins the
    codes of an integer range; theirs is ``mx_quant_stats``."""
    return _model_stats(model, want_hist, mx=False)


def mx_quant_stats(model: nn.Module, want_hist=True) -> dict:
    """{reference name: summary} of every tensor of ``model`` whose layer has an element format (``quantized_tensors``' walk;
    the others are skipped: theirs is ``quant_stats``): the ops.summarize_mx_stats dict of the tensor's
    ``CustomQuantizedScaleLayer.mx_stats``.  One launch per tensor, then all records go to the host together in one copy (one
    synchronisation: call it between steps, never inside a capture).  ``{}`` for a model without such layers."""
    return _model_stats(model, want_hist, mx=True)


def init_scales(model: nn.Module, method) -> nn.Module:
    """Initialises every scale of every custom layer of ``model`` from its weights (``_HostLayer.init_scales``; ``method`` one of
    ops.SCALE_INITS), then checks all scales with ONE ``isfinite`` reduction -- one synchronisation: this is a host call made
    once, before the optimizer and any graph exist, never inside a capture.  A NaN scale (a weight tensor that holds a NaN or
    an Inf) raises ValueError with the layer's name.  The scales are written in place: pointers taken before stay valid.
    A model of layers with an element format takes "mx" / "cover" (ops.MX_SCALE_INITS) and none of the others; a model without
    them takes none of these two."""
    layers = custom_layers_of(model)
    mx = [layer for layer in layers if layer.element_format is not None]
    if mx:
        if method not in ops.MX_SCALE_INITS:
            raise ValueError(f"scale_init {method!r} on a model with element formats ({mx[0].name!r}: {mx[0].element_format!r}): a "
                             f"microscaling scale is a power of two, written by one of {ops.MX_SCALE_INITS}")
    elif method in ops.MX_SCALE_INITS:
        raise ValueError(f"scale_init {method!r} on a model without element formats: it writes the power-of-two scale of a "
                         f"microscaling block; an integer model takes one of {ops.LAYER_SCALE_INITS}")
    else:
        ops.check_layer_scale_init(method)
    if method == "minmax":      # before any launch: every layer must be able to take it
        for layer in layers:
            if not layer.asymmetric:
                raise ValueError(f'scale_init "minmax" on a symmetric layer ({layer.name!r}): it places each group\'s range over '
                                 "[min, max] through an offset, which only an asymmetric=True layer has")
            ops.check_minmax_range(*layer.q_range)
    entries = []
    for layer in layers:
        layer.init_scales(method)
        entries += [(layer, what, nested) for what, nested, _ in layer.scale_pairs()]
    if entries:
        ok = torch.stack([torch.isfinite(nested.scale.detach()).all() if nested.offset is None else
                          torch.isfinite(nested.scale.detach()).all() & torch.isfinite(nested.offset.detach()).all()
                          for _, _, nested in entries]).cpu().numpy()
        for (layer, what, nested), fine in zip(entries, ok):
            if not fine:
                raise ValueError(f"scale initialisation ({method}) of layer {layer.name!r}: the scale of {what!r} is not finite -- "
                                 "the weights hold a NaN or an Inf")
    return model
