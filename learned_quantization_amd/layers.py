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

    def _check_i8(self, offsets=False, int4=False):
        """(qmin, qmax) of a layer that can run on the int8 matrix instruction, or ValueError naming the reason.  ``offsets=True``
        lets an asymmetric layer pass (ops.check_i8_operand_layer); ``int4=True`` asks for a range that fits the packed 4-bit
        operand as well (ops.check_i4_operand_layer)."""
        check = ops.check_i4_operand_layer if int4 else ops.check_i8_operand_layer
        q_range = check(self.q_range, self.nested_q_w_layer.orientation, self.group_size, self.asymmetric,
                        self.element_format, self.W.shape[0] if self.built else None, offsets=offsets)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return q_range

    def i8_operand(self, offsets=False, int4=False) -> "ops.I8Operand":
        """The kernel under its current scales as an operand of the int8 matrix instruction (ops.i8_operand_pack): ``units`` lines
        over K = in.  A "groupwise" layer passes its scale as it is; a "scalar" or "columnwise" layer its scale broadcast to
        ``(1, out)``, one group per output unit.  ValueError naming the reason for a layer without a range, with a range outside
        [-128, 127], with an offset, with "rowwise" scales, with an element format, or not built.
        ``offsets=True``: an asymmetric layer is packed with its ``(nb, out)`` scale and offset into an ops.I8AffineOperand, whose
        product adds the offset's row-sum term; a symmetric layer takes the path it always took.
        ``int4=True``: the same codes two to a byte, an ops.I4Operand (ops.i4_operand_pack), for a layer whose range lies inside
        [-8, 7]; its products are bit for bit those of the byte operand."""
        qmin, qmax = self._check_i8(offsets, int4)
        fan_in, units = self.W.shape
        scale = self.nested_q_w_layer.scale.data
        if self.nested_q_w_layer.orientation == "groupwise":
            gs = self.group_size
        else:
            scale, gs = scale.reshape(1, -1).expand(1, units).contiguous(), fan_in
        offset = self.nested_q_w_layer.offset.data if self.asymmetric else None
        pack = ops.i4_operand_pack if int4 else ops.i8_operand_pack
        return pack(self.W.detach(), scale, qmin, qmax, gs, self.rounding, offset)

    def call_i8(self, inputs, act_block=0, out_block=None, activation=None, offsets=False, int4=False):
        """The layer on the int8 matrix instruction, under ``no_grad``: the inputs quantised per row and ``act_block`` consecutive
        inputs (0: per row) to symmetric 8-bit integers (ops.i8_operand_quantize), multiplied with ``i8_operand()`` by ops.i8_gemm,
        plus the fake-quantised bias.  Inference only: there is no backward through this path.
        ``inputs`` may be an ops.I8Operand (``lines`` rows over ``K`` = in), which is multiplied as it is; ``act_block`` is then not
        read.  With ``out_block`` (64) the result is not the fp32 matrix but the NEXT layer's operand, ``activation`` (None or
        "relu") applied and quantised per row and block of 64 by the product's own epilogue (ops.i8_gemm_quantize): one launch, no
        fp32 activation in memory.  ``offsets=True`` lets an asymmetric layer run (``i8_operand(offsets=True)``); ``int4=True``
        multiplies with the packed 4-bit operand (``i8_operand(int4=True)``), the same bits from half the weight bytes."""
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
            return self._matrix_product(inputs, self.i8_operand(offsets, int4), self.nested_q_b_layer(self.b), _I8, (act_block,),
                                        out_block, activation)

    def mx_operand(self, fp6=False) -> "ops.MxOperand":
        """The kernel under its current scales as an operand of the block-scaled matrix instruction (ops.mx_operand_pack): ``units``
        lines over K = in.  ValueError naming the reason for a layer without an element format, with ``scale_format="fp32"``, with
        an fp6 format or with a group size other than 32.
        ``fp6=True``: a layer with an fp6 element format is packed into an ops.Mx6Operand (ops.mx6_operand_pack) instead of being
        refused; every other layer gets what it gets without it."""
        ops.check_mx_operand_layer(self.element_format, self.scale_format, self.group_size, fp6=fp6)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return ops.mx_layer_pack(self.W.detach(), self.nested_q_w_layer.scale.data, self.element_format, self.group_size,
                                 self.scale_format, fp6)

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

    def call_mx(self, inputs, act_format="fp8_e4m3", act_scale="mx", out_format=None, activation=None, fp6=False):
        """The layer on the block-scaled matrix instruction, under ``no_grad``: the inputs quantised per block of 32 along their last
        axis (``act_format`` elements under the ``act_scale`` rule, ops.mx_operand_quantize), multiplied with ``mx_operand()`` by
        ops.mx_gemm, plus the fake-quantised bias.  Inference only: there is no backward through this path.
        ``inputs`` may be an ops.MxOperand (``lines`` rows over ``K`` = in), which is multiplied as it is.  With ``out_format`` the
        result is not the fp32 matrix but the NEXT layer's operand, ``activation`` (None or "relu") applied and quantised under
        ``act_scale`` by the product's own epilogue (ops.mx_gemm_quantize): one launch, no fp32 activation in memory.
        ``fp6=True`` lets a layer with an fp6 element format run (``mx_operand(fp6=True)``): the activations stay ``act_format``
        (fp8 or fp4), so the layer runs as W6A8 or W6A4."""
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
            return self._matrix_product(inputs, self.mx_operand(fp6), self.nested_q_b_layer(self.b), _MX, (act_format, act_scale),
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
    _i8_direct_hw = None      # (operand, bias) parked by i8_hardware(convs=True, direct=True)
    _i8_chain_hw = None       # (operand, bias) parked by i8_hardware(fused_convs=True) on the layers of a conv chain
    _i8_stem_hw = None        # (stem operand, bias) parked by i8_hardware(stem_convs=True) on a first conv of at most 4 channels

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
        direct = self._i8_direct_hw
        if direct is not None and not self.training:              # inside layers.i8_hardware(..., convs=True, direct=True), eval mode
            self._q_pre = None
            return self._direct_conv(inputs, direct[0], direct[1])
        stem = self._i8_stem_hw
        if stem is not None and not self.training:                # inside layers.i8_hardware(..., stem_convs=True), eval mode
            self._q_pre = None
            with torch.no_grad():
                return self._direct_step(inputs, stem[0], stem[1])
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

    def mx_operand(self, fp6=False) -> "ops.MxOperand":
        """The kernel under its current scales as an operand of the block-scaled matrix instruction (ops.mx_operand_pack, blocks
        along the contiguous axis): ``filters`` lines over K = ci kh kw, the reduction order of ops.mx_operand_im2col.  ValueError
        naming the reason for ``kernel_storage="hwio"``, for a layer without an element format, with ``scale_format="fp32"``, with an
        fp6 format or with a group size other than 32, and for a layer that is not built.
        ``fp6=True``: a layer with an fp6 element format is packed into an ops.Mx6Operand instead of being refused."""
        if self.kernel_storage != "oihw":
            raise ValueError(f'{self.name}: kernel_storage="hwio": the block-scaled GEMM reduces over the (ci, kh, kw) memory run of a '
                             'kernel stored "oihw"')
        ops.check_mx_operand_layer(self.element_format, self.scale_format, self.group_size, fp6=fp6)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return ops.mx_layer_pack(self.kernel.detach(), self.nested_q_k_layer.scale.data, self.element_format, self.group_size,
                                 self.scale_format, fp6)

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

    def call_mx(self, inputs, act_format="fp8_e4m3", act_scale="mx", max_lines=None, fp6=False):
        """The layer on the block-scaled matrix instruction, under ``no_grad``: the im2col matrix of the inputs quantised per block
        of 32 along (ci, kh, kw) (``act_format`` elements under the ``act_scale`` rule) by ops.mx_operand_im2col -- TensorFlow 'SAME'
        padding as ``call`` pads, or 'VALID' -- multiplied with ``mx_operand()`` by ops.mx_gemm, plus the fake-quantised bias where
        the layer has one.  Inference only: there is no backward through this path.  The result is a view of the GEMM's (M, co)
        matrix: ``(B, co, OH, OW)`` with channels-last strides for ``data_format="NCHW"``, ``(B, OH, OW, co)`` for "NHWC".  A batch
        whose im2col matrix has 2^31 elements or more, more than 65535 * 64 lines or more than ``max_lines`` lines is cut into runs
        of whole images that write their rows of the one result; the result does not depend on the cut.
        ``fp6=True`` lets a layer with an fp6 element format run (``mx_operand(fp6=True)``); the im2col operand stays ``act_format``."""
        _check_max_lines(max_lines)
        ops.check_mx_operand_format(act_format)
        ops.check_mx_scale_init(act_scale)
        return self._call_matrix(inputs, _MX, (act_format, act_scale), max_lines, fp6=fp6)

    def _check_i8(self, offsets=False, int4=False):
        """(qmin, qmax) of a conv layer that can run on the int8 matrix instruction, or ValueError naming the reason.
        ``offsets=True`` lets an asymmetric layer pass (ops.check_i8_conv_operand_layer); ``int4=True`` asks for a range that fits
        the packed 4-bit operand as well (ops.check_i4_operand_layer)."""
        fan_in = self.kernel.shape[0] * self.kernel.shape[1] * self.kernel.shape[2] if self.built else None
        if int4:
            q_range = ops.check_i4_operand_layer(self.q_range, self.nested_q_k_layer.orientation, self.group_size, self.asymmetric,
                                                 self.element_format, fan_in, offsets=offsets, conv=True,
                                                 kernel_storage=self.kernel_storage)
        else:
            q_range = ops.check_i8_conv_operand_layer(self.q_range, self.nested_q_k_layer.orientation, self.group_size,
                                                      self.asymmetric, self.element_format, fan_in, self.kernel_storage,
                                                      offsets=offsets)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return q_range

    def i8_operand(self, offsets=False, int4=False) -> "ops.I8Operand":
        """The kernel under its current scales as an operand of the int8 matrix instruction (ops.i8_operand_pack, groups along the
        contiguous axis): ``filters`` lines over K = ci kh kw, the reduction order of ops.i8_operand_im2col.  A "groupwise" layer
        passes its scale as it is; a "scalar" layer its scale broadcast to ``(filters, 1)``, one group per output channel.
        ValueError naming the reason for a one-axis orientation, ``kernel_storage="hwio"``, a layer without a range, with a range
        outside [-128, 127], with an offset, with an element format, or not built.
        ``offsets=True``: an asymmetric layer is packed with its ``(co, nb)`` scale and offset into an ops.I8AffineOperand, whose
        product adds the offset's row-sum term (padded taps hold code 0 and add no offset); a symmetric layer takes the path it
        always took.  ``int4=True``: the same ``(co, ci kh kw)`` codes two to a byte, an ops.I4Operand of the im2col path, for a
        layer whose range lies inside [-8, 7]."""
        qmin, qmax = self._check_i8(offsets, int4)
        K = self.kernel.numel() // self.filters
        scale = self.nested_q_k_layer.scale.data
        if self.nested_q_k_layer.orientation == "groupwise":
            gs = self.group_size
        else:
            scale, gs = scale.reshape(1, 1).expand(self.filters, 1).contiguous(), K
        offset = self.nested_q_k_layer.offset.data if self.asymmetric else None
        pack = ops.i4_operand_pack if int4 else ops.i8_operand_pack
        return pack(self.kernel.detach(), scale, qmin, qmax, gs, self.rounding, offset)

    def call_i8(self, inputs, act_block=0, max_lines=None, offsets=False, int4=False):
        """The layer on the int8 matrix instruction, under ``no_grad``: the im2col matrix of the inputs quantised per line and
        ``act_block`` consecutive k of (ci, kh, kw) (0: per line) to symmetric 8-bit integers by ops.i8_operand_im2col -- TensorFlow
        'SAME' padding as ``call`` pads, or 'VALID' -- multiplied with ``i8_operand()`` by ops.i8_gemm, plus the fake-quantised bias
        where the layer has one.  Inference only: there is no backward through this path.  The result is a view of the GEMM's
        (M, co) matrix: ``(B, co, OH, OW)`` with channels-last strides for ``data_format="NCHW"``, ``(B, OH, OW, co)`` for "NHWC".  A
        batch whose im2col matrix has 2^31 elements or more, more than 65535 * 64 lines or more than ``max_lines`` lines is cut into
        runs of whole images that write their rows of the one result; the result does not depend on the cut.  ``offsets=True``
        lets an asymmetric layer run (``i8_operand(offsets=True)``); ``int4=True`` multiplies with the packed 4-bit operand
        (``i8_operand(int4=True)``), the same bits from half the weight bytes."""
        _check_max_lines(max_lines)
        ops.check_i8_block(act_block)
        return self._call_matrix(inputs, _I8, (act_block,), max_lines, offsets=offsets, int4=int4)

    def _check_i8_direct(self):
        """(qmin, qmax) of a conv layer that can run as a direct int8 convolution, or ValueError naming the reason
        (ops.check_i8_direct_layer): what ``_check_i8`` asks, symmetric, and one scale per filter."""
        fan_in = self.kernel.shape[0] * self.kernel.shape[1] * self.kernel.shape[2] if self.built else None
        q_range = ops.check_i8_direct_layer(self.q_range, self.nested_q_k_layer.orientation, self.group_size, self.asymmetric,
                                            self.element_format, fan_in, self.kernel_storage)
        if not self.built:
            raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
        return q_range

    def i8_direct_operand(self) -> "ops.I8ConvKernel":
        """The kernel under its current scales as the per-tap operand of the direct int8 convolution (ops.i8_conv_kernel_pack): the
        codes of ``i8_operand()``, in the order ops.i8_conv2d reads them, under one scale per filter.  ValueError naming the reason
        for everything ``i8_operand()`` refuses, for an asymmetric layer and for group-wise scales that vary along (ci, kh, kw)."""
        qmin, qmax = self._check_i8_direct()
        scale = self.nested_q_k_layer.scale.data.reshape(-1)      # one element ("scalar"), or one per filter ("groupwise", (co, 1))
        return ops.i8_conv_kernel_pack(self.kernel.detach().permute(3, 2, 0, 1), scale, qmin, qmax, self.rounding)

    def _check_i8_stem(self):
        """(qmin, qmax) of a conv layer that can run as a stem convolution, or ValueError naming the reason: what
        ``_check_i8_direct`` asks, at most 4 input channels and a kernel of at most 16 x 8 (ops.check_i8_stem_shape)."""
        q_range = self._check_i8_direct()
        ops.check_i8_stem_shape(self.kernel.shape[2], self.kernel_size)
        return q_range

    def i8_stem_operand(self) -> "ops.I8StemKernel":
        """The kernel under its current scales as the per-row operand of the stem convolution (ops.i8_stem_kernel_pack): the codes
        of ``i8_direct_operand()``, a kernel row per step.  ValueError naming the reason for everything ``i8_direct_operand()``
        refuses, for more than 4 input channels and for a kernel wider than 8 or higher than 16."""
        qmin, qmax = self._check_i8_stem()
        scale = self.nested_q_k_layer.scale.data.reshape(-1)
        return ops.i8_stem_kernel_pack(self.kernel.detach().permute(3, 2, 0, 1), scale, qmin, qmax, self.rounding)

    def call_i8_stem(self, inputs, max_lines=None, out_pixels=False, activation=None, affine=None, affine_first=False, pool=None):
        """The layer as a stem convolution, under ``no_grad``: the inputs (a tensor of at most 4 channels) quantised ONCE per image
        row to symmetric 8-bit integers (ops.i8_rows_quantize: an int8 NHWC4 copy, one scale per row), convolved with
        ``i8_stem_operand()`` by ops.i8_stem_conv2d -- a kernel row per step of the int8 matrix instruction, no padded channels, no
        im2col matrix -- padded as ``call`` pads, plus the fake-quantised bias where the layer has one.  Inference only.  The result
        is the kind of view ``call_i8_direct`` returns, and the batch is cut into runs of whole images as it cuts it.  The
        activation scale is per image ROW here: the result is not bit-identical to ``call_i8`` or ``call_i8_direct``.
        ``out_pixels=True``: the result is the NEXT conv's ops.I8Pixels from the product's own epilogue
        (ops.i8_stem_conv2d_quantize) after ``activation`` and ``affine`` in the order ``affine_first`` says; at most 128 filters.
        Without it an epilogue is refused.
        ``pool=3`` (with ``out_pixels=True``): the epilogue takes the 3 x 3 maximum of stride 2 after the activation and the affine,
        padded as TensorFlow pads a "same" pool of the conv's output extents ((0, 1) for an even extent, (1, 1) for an odd one), and
        writes the pixel operand of the pooled image (ops.i8_stem_conv2d_quantize, ``pool``); refused without ``out_pixels``."""
        _check_max_lines(max_lines)
        if pool is not None and not out_pixels:
            raise ValueError(f"{self.name}: pool={pool!r} without out_pixels=True: the fp32 result has no epilogue to pool in; apply "
                             "F.max_pool2d to the result")
        if not out_pixels and (activation is not None or affine is not None or affine_first):
            raise ValueError(f"{self.name}: the fp32 result takes no epilogue (activation={activation!r}, affine, affine_first): "
                             "apply it to the result, or ask for out_pixels=True")
        if not isinstance(inputs, torch.Tensor):
            raise ValueError(f"{self.name}: the stem convolution quantises a tensor itself, got {type(inputs).__name__}")
        if not self.built:
            self.build(tuple(inputs.shape), device=inputs.device)
        with torch.no_grad():
            operand = self.i8_stem_operand()
            qb = self.nested_q_b_layer(self.b) if self._has_bias else None
            return self._direct_step(inputs, operand, qb, max_lines, out_pixels, activation, affine, affine_first, pool=pool)

    def _direct_conv(self, inputs, operand, qb, max_lines=None):
        """The layer as a direct int8 convolution: per run of whole images (by lines) the pixel operand of the inputs, convolved
        with ``operand``, plus ``qb``, into its rows of the one result.  Where ``operand`` is a tensor (the fake-quantised OIHW
        kernel: ``emulate=True``) the decoded pixel operand is convolved with it by ``F.conv2d`` instead."""
        with torch.no_grad():
            if inputs.dim() != 4:
                raise ValueError(f"{self.name}: the input must have four axes, got shape {tuple(inputs.shape)}")
            x = inputs.permute(0, 3, 1, 2) if self.data_format == "NHWC" else inputs       # a view: the quantizer reads its strides
            top, bottom, left, right = padding = self._mx_padding(x.shape[2], x.shape[3])
            M, _, OH, OW = ops.mx_im2col_dims(x.shape, self.kernel_size, self.strides, padding)
            B, C, per = x.shape[0], x.shape[1], OH * OW
            y = torch.empty((M, self.filters), dtype=torch.float32, device=x.device)
            fit = 65535 * 64 if max_lines is None else min(65535 * 64, max_lines)
            images = max(1, min(B, fit // per))
            for b0 in range(0, B, images):
                b1 = min(B, b0 + images)
                pixels = ops.i8_pixels_quantize(x[b0:b1])
                if not isinstance(operand, torch.Tensor):
                    ops.i8_conv2d(pixels, operand, qb, self.strides, padding, out=y[b0 * per:b1 * per])
                    continue
                decoded = pixels.codes[..., :C].view(torch.int8).float().mul_(pixels.scales.unsqueeze(-1)).permute(0, 3, 1, 2)
                out = F.conv2d(F.pad(decoded, (left, right, top, bottom)), operand, qb, self.strides)
                y[b0 * per:b1 * per].copy_(out.permute(0, 2, 3, 1).reshape(-1, self.filters))
            y = y.view(B, OH, OW, self.filters)                   # [M][co] is NHWC: no transposition launch
            return y if self.data_format == "NHWC" else y.permute(0, 3, 1, 2)

    def _direct_step(self, x, operand, qb, max_lines=None, out_pixels=False, activation=None, affine=None, affine_first=False,
                     residual=None, wide=False, pool=None):
        """One layer of a direct-conv chain: ``x`` a tensor in the layer's data format (quantised here, per run) or an ops.I8Pixels;
        the result the fp32 view ``_direct_conv`` returns, or (``out_pixels``) the next conv's ops.I8Pixels from the product's own
        epilogue (ops.i8_conv2d_quantize).  The batch is cut into runs of whole images by lines, as ``_direct_conv`` cuts it; a
        ``residual`` (an ops.I8Pixels of the result's shape) is cut by the same images.  ``wide`` and ``pool``:
        ops.i8_conv2d_quantize's (a pool works inside an image, so the cut does not change it).  Where ``operand`` is an
        ops.I8StemKernel the step is the stem convolution: ``x`` a tensor, quantised per image row (ops.i8_rows_quantize), the
        product ops.i8_stem_conv2d or its epilogue, which takes no residual or wide row, and of the pools only 3: the 3 x 3 / 2
        maximum under TensorFlow's "same" pool paddings of the conv's output extents (ops.i8_stem_conv2d_quantize, ``pool``)."""
        stem = isinstance(operand, ops.I8StemKernel)
        if stem and (isinstance(x, ops.I8Pixels) or residual is not None or wide or not (pool is None or (pool == 3 and not isinstance(pool, bool)))):
            raise ValueError(f"{self.name}: the stem convolution quantises a tensor itself and its epilogue takes no residual, wide "
                             "row or pool other than 3")

        def images_of(px):        # a cut: the codes of whole images stay on the 16-byte grid (CP % 32 == 0); the scales may not
            def cut(b0, b1):
                scales = px.scales[b0:b1]
                return ops.I8Pixels(px.codes[b0:b1], scales.clone() if scales.data_ptr() % 16 else scales, (b1 - b0, *px.shape[1:]))
            return cut
        if isinstance(x, ops.I8Pixels):
            B, C, H, W = x.shape
            run = images_of(x)
        else:
            if x.dim() != 4:
                raise ValueError(f"{self.name}: the input must have four axes, got shape {tuple(x.shape)}")
            xt = x.permute(0, 3, 1, 2) if self.data_format == "NHWC" else x
            B, C, H, W = xt.shape
            run = lambda b0, b1: (ops.i8_rows_quantize if stem else ops.i8_pixels_quantize)(xt[b0:b1])  # noqa: E731
        padding = self._mx_padding(H, W)
        M, _, OH, OW = ops.mx_im2col_dims((B, C, H, W), self.kernel_size, self.strides, padding)
        per = OH * OW
        fit = 65535 * 64 if max_lines is None else min(65535 * 64, max_lines)
        images = max(1, min(B, fit // per))
        runs = [(b0, min(B, b0 + images)) for b0 in range(0, B, images)]
        if out_pixels:
            if residual is not None and (not isinstance(residual, ops.I8Pixels) or tuple(residual.shape) != (B, self.filters, OH, OW)):
                raise ValueError(f"{self.name}: the residual must be an ops.I8Pixels of the result's shape {(B, self.filters, OH, OW)}, got "
                                 f"{tuple(residual.shape) if isinstance(residual, ops.I8Pixels) else type(residual).__name__}")
            res = images_of(residual) if residual is not None else (lambda b0, b1: None)
            if stem:
                same = lambda n: (n % 2, 1)       # noqa: E731  a "same" 3 / 2 pool pads 1 in all (even) or 2 (odd), the lesser half first
                pool_padding = (*same(OH), *same(OW)) if pool is not None else (0, 0, 0, 0)
                outs = [ops.i8_stem_conv2d_quantize(run(b0, b1), operand, qb, self.strides, padding, activation, affine, affine_first,
                                                    pool, pool_padding) for b0, b1 in runs]
            else:
                outs = [ops.i8_conv2d_quantize(run(b0, b1), operand, qb, self.strides, padding, activation, affine, affine_first,
                                               res(b0, b1), wide, pool) for b0, b1 in runs]
            if len(outs) == 1:
                return outs[0]
            return ops.I8Pixels(torch.cat([o.codes for o in outs]), torch.cat([o.scales for o in outs]), (B, *outs[0].shape[1:]))
        y = torch.empty((M, self.filters), dtype=torch.float32, device=operand.codes.device)
        for b0, b1 in runs:
            (ops.i8_stem_conv2d if stem else ops.i8_conv2d)(run(b0, b1), operand, qb, self.strides, padding, out=y[b0 * per:b1 * per])
        y = y.view(B, OH, OW, self.filters)
        return y if self.data_format == "NHWC" else y.permute(0, 3, 1, 2)

    def call_i8_direct(self, inputs, max_lines=None, out_pixels=False, activation=None, affine=None, affine_first=False,
                       residual=None, wide=False, pool=None):
        """The layer as a direct int8 convolution, under ``no_grad``: the inputs quantised ONCE per pixel to symmetric 8-bit integers
        (ops.i8_pixels_quantize: an int8 NHWC copy, one scale per pixel), convolved with ``i8_direct_operand()`` on the int8 matrix
        instruction by ops.i8_conv2d -- TensorFlow 'SAME' padding as ``call`` pads, or 'VALID' -- plus the fake-quantised bias where
        the layer has one.  No im2col matrix is written.  Inference only.  The result is the kind of view ``call_i8`` returns.  A
        batch of more than 65535 * 64 lines or more than ``max_lines`` lines is cut into runs of whole images; the result does not
        depend on the cut.  The activation scale is per PIXEL here and per im2col LINE in ``call_i8``: the two paths round the
        activations differently and are not bit-identical.
        ``inputs`` may be an ops.I8Pixels (the pixel operand another conv's epilogue wrote): it is multiplied as it is.
        ``out_pixels=True``: the result is the NEXT conv's ops.I8Pixels, written by the product's own epilogue
        (ops.i8_conv2d_quantize) after ``activation`` (None or "relu") and ``affine = (g, h)`` (``bn_affine``), in the order
        ``affine_first`` says; byte for byte ``ops.i8_pixels_quantize`` of that result.  Without it an epilogue is refused.
        ``residual`` (with ``out_pixels=True``): an ops.I8Pixels of the result's shape, decoded and added directly before the
        activation by the same epilogue (the basic ResNet block).
        ``wide=True`` (with ``out_pixels=True``): a layer of more than 512 filters, up to 2048, goes through the epilogue that parks
        its output row in LDS (ops.i8_conv2d_quantize, ``wide``); a layer of at most 512 goes where it goes without it.
        ``pool=2`` (with ``out_pixels=True``): the epilogue takes the 2 x 2 maximum after the activation and the affine and writes
        the pixel operand of the pooled image (ops.i8_conv2d_quantize, ``pool``); refused without ``out_pixels``."""
        _check_max_lines(max_lines)
        if pool is not None and not out_pixels:
            raise ValueError(f"{self.name}: pool={pool!r} without out_pixels=True: the fp32 result has no epilogue to pool in; apply "
                             "F.max_pool2d to the result")
        if pool == 3 and not isinstance(pool, bool):
            raise ValueError(f"{self.name}: pool=3: the 3 x 3 / 2 maximum is built in the stem convolution's epilogue only (call_i8_stem)")
        if not out_pixels and (activation is not None or affine is not None or affine_first or residual is not None):
            raise ValueError(f"{self.name}: the fp32 result takes no epilogue (activation={activation!r}, affine, affine_first, "
                             "residual): apply it to the result, or ask for out_pixels=True")
        direct = isinstance(inputs, ops.I8Pixels) or out_pixels
        if not self.built:
            if isinstance(inputs, ops.I8Pixels):
                raise ValueError(f"{self.name}: the layer is not built yet (no kernel to pack)")
            self.build(tuple(inputs.shape), device=inputs.device)
        with torch.no_grad():
            operand = self.i8_direct_operand()
            qb = self.nested_q_b_layer(self.b) if self._has_bias else None
            if not direct:
                return self._direct_conv(inputs, operand, qb, max_lines)
            return self._direct_step(inputs, operand, qb, max_lines, out_pixels, activation, affine, affine_first, residual, wide, pool)


class CustomConv2DLayer(_ConvBase):
    """Standard convolutional layer with nested quantization layers for kernel and bias (NQ-L:271-350)."""


class CustomConv2DLayerNoBias(_ConvBase):
    """Bias-free variant (paper_implementation custom_layers.py:299-365)."""
    _has_bias = False


def custom_layers_of(model: nn.Module):
    """The reference selects layers by name substring (experiment.py:73, custom_loss_terms/experiment.py:446)."""
    return [m for m in model.modules()
            if isinstance(m, (CustomDenseLayer, _ConvBase))]


def _mx_layer_formats(fp6) -> Tuple[str, ...]:
    return ops.MX_OPERAND_FORMATS + (ops.MX6_OPERAND_FORMATS if fp6 else ())


def mx_hardware_eligible(layer: nn.Module, fp6=False) -> bool:
    """Whether ``layer`` takes the block-scaled GEMM under ``mx_hardware``: a built Dense layer with an fp4 / fp8 element format,
    E8M0 scales and blocks of 32.  Conv layers keep the fake-quantised path (no implicit GEMM is built).  ``fp6=True``: a layer
    with an fp6 element format is eligible too."""
    return (isinstance(layer, CustomDenseLayer) and layer.built and layer.element_format in _mx_layer_formats(fp6)
            and layer.scale_format == "e8m0" and layer.group_size == ops.MX_GROUP_SIZE)


def mx_conv_eligible(layer: nn.Module, fp6=False) -> bool:
    """Whether ``layer`` takes the block-scaled GEMM under ``mx_hardware(convs=True)``: a built conv layer with an fp4 / fp8 element
    format, E8M0 scales, blocks of 32 and the kernel stored "oihw" (the blocks then run along the im2col operand's K).  ``fp6=True``:
    a layer with an fp6 element format is eligible too."""
    return (isinstance(layer, _ConvBase) and layer.built and layer.element_format in _mx_layer_formats(fp6)
            and layer.scale_format == "e8m0" and layer.group_size == ops.MX_GROUP_SIZE and layer.kernel_storage == "oihw")


class _matrix_hardware:
    """Entry and exit of ``mx_hardware`` and ``i8_hardware``: the eligible Dense layers, then (``convs``) the eligible conv layers,
    get ``(operand, bias, *act)`` under the family's attribute -- built once, on entry -- and lose it on exit."""
    _family = _dense_eligible = _conv_eligible = None
    _opt_in = {}              # keywords of the eligibility tests and of the layers' operand method (i8_hardware: offsets)

    def _operand_kwargs(self, layer):
        """The keywords of ``layer``'s operand method: the opt-ins, and what a subclass decides per layer."""
        return self._opt_in

    def __enter__(self):
        family, custom, opt_in = self._family, custom_layers_of(self.model), self._opt_in
        switching = [m for m in custom if self._dense_eligible(m, **opt_in)]
        switching += [m for m in custom if self._conv_eligible(m, **opt_in)] if self.convs else []
        self.layers = []
        with torch.no_grad():
            for m in switching:
                if not self.emulate:
                    weight = getattr(m, family.operand)(**self._operand_kwargs(m))
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
    default) conv layers keep the fake-quantised path.
    ``fp6=True``: layers with an fp6 element format switch too -- their kernels packed into ops.Mx6Operand, the activations still
    ``act_format`` (W6A8 / W6A4; an fp6 ``act_format`` stays refused) -- and are listed in ``layers``.  It combines with ``convs``,
    ``fused`` and ``emulate``; fp4 / fp8 layers behave as they do without it, so a model without fp6 layers is bit-identical.
    Without it (the default) fp6 layers keep the fake-quantised path."""

    _family, _dense_eligible, _conv_eligible = _MX, staticmethod(mx_hardware_eligible), staticmethod(mx_conv_eligible)

    def __init__(self, model: nn.Module, act_format="fp8_e4m3", act_scale="mx", emulate=False, fused=False, convs=False, fp6=False):
        self.fp6 = bool(fp6)
        self._opt_in = {"fp6": True} if self.fp6 else {}
        ops.check_mx_operand_format(act_format)
        ops.check_mx_scale_init(act_scale)
        if emulate and fused:
            raise ValueError("mx_hardware: emulate=True with fused=True: the emulated path is the yardstick of the unfused path and "
                             "has no operand-out epilogue")
        self.model, self.act_format, self.act_scale, self.emulate, self.fused = model, act_format, act_scale, bool(emulate), bool(fused)
        self.convs, self._act = bool(convs), (act_format, act_scale)
        self.layers, self.fused_layers, self._fused_modules = [], [], []


def _passes_check_i8(layer: nn.Module, cls, offsets=False, int4=False) -> bool:
    if not isinstance(layer, cls):
        return False
    try:
        layer._check_i8(offsets, int4)
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


def i8_int4_eligible(layer: nn.Module, offsets=False) -> bool:
    """Whether ``layer`` can take the packed 4-bit operand (``i8_operand(int4=True)``): a Dense layer that passes
    ``i8_hardware_eligible`` or a conv layer that passes ``i8_conv_eligible``, with a range inside [-8, 7] (``bits`` of at most 4,
    signed)."""
    return _passes_check_i8(layer, (CustomDenseLayer, _ConvBase), offsets, True)


def i8_direct_eligible(layer: nn.Module) -> bool:
    """Whether ``layer`` can run as a direct int8 convolution (``call_i8_direct``): it passes ``i8_conv_eligible``, is symmetric, and
    has one scale per filter ("scalar", or "groupwise" with ``group_size >= ci kh kw``)."""
    if not isinstance(layer, _ConvBase):
        return False
    try:
        layer._check_i8_direct()
    except ValueError:
        return False
    return True


def _takes_direct(layer: nn.Module) -> bool:
    """What ``i8_hardware(direct=True)`` sends down the direct path: an eligible conv whose input channels fill whole steps of 32
    (a first layer of 3 channels would multiply 29 padded zeros per tap: it stays on the im2col path)."""
    return i8_direct_eligible(layer) and layer.kernel.shape[2] % 32 == 0


def i8_stem_eligible(layer: nn.Module) -> bool:
    """Whether ``layer`` can run as a stem convolution (``call_i8_stem``): it passes ``i8_direct_eligible``, reads at most 4 input
    channels and has a kernel of at most 16 x 8."""
    if not isinstance(layer, _ConvBase):
        return False
    try:
        layer._check_i8_stem()
    except ValueError:
        return False
    return True


def _takes_stem(layer: nn.Module) -> bool:
    """What ``i8_hardware(stem_convs=True)`` sends down the stem path: a stem-eligible conv that ``_takes_direct`` rejects."""
    return i8_stem_eligible(layer) and not _takes_direct(layer)


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
    decoded activation with the fake-quantised kernel); a symmetric model is bit-identical with or without it.
    ``direct=True`` (with ``convs=True``): an eligible conv layer with one scale per filter, symmetric, whose input channels are a
    multiple of 32 (``i8_direct_eligible``) computes what its ``call_i8_direct`` does instead -- its input quantised once per pixel
    (ops.i8_pixels_quantize), the windows gathered inside the product (ops.i8_conv2d), no im2col matrix -- and is listed in
    ``direct_layers`` as well as in ``layers``; ``act_block`` does not apply to it (the scale is per pixel).  Every other layer goes
    where it goes without ``direct``.  Under ``emulate=True`` such a layer convolves the decoded pixel operand with the
    fake-quantised kernel by ``F.conv2d``.  Without ``direct`` (the default) nothing changes.
    ``int4=True``: a layer that switches and whose range lies inside [-8, 7] (``i8_int4_eligible``) gets the packed 4-bit operand
    (``i8_operand(int4=True)``: half the weight bytes, the same bits) and is listed in ``int4_layers``; every other layer that
    switches keeps its byte operand.  It combines with ``convs``, ``fused``, ``offsets`` and ``emulate`` (which multiplies no
    operand and lists none); with ``direct`` the direct convs keep their own per-tap byte operand (a 4-bit one is not built).
    Without ``int4`` (the default) nothing changes.
    ``fused_convs=True`` (with ``convs=True, direct=True``; the model in eval mode on entry): a module of ``model`` that states conv
    chains as ``i8_conv_chains()`` -- lists of (conv, activation, BatchNorm2d or None, affine_first), as models.CIFARCNN states its
    three conv -> relu -> BN -> conv pairs -- evaluates each chain whose layers pass ``i8_direct_eligible`` through
    ``i8_conv_chain`` in eval mode: every conv but the last writes the next conv's pixel operand from its own epilogue
    (ops.i8_conv2d_quantize), the BatchNorm folded to ``bn_affine``'s ``(g, h)`` on entry, and no fp32 activation exists between
    them.  ``fused_conv_layers`` lists the convs with such an epilogue.  A module whose class sets ``i8_chains_out_pixels = True``
    (models._ResidualBlock) runs its chains with ``out_pixels=True`` -- every conv through the epilogue, conv2 with the shortcut as
    its residual, a chain of one conv allowed -- takes them all or none, and has every conv of them listed: models.ResNet18Like
    then runs its eight basic blocks conv to conv in int8 (19 convs listed; the last block's conv2 reads conv1's pixel operand
    but writes fp32 for the mean).  A model that states no chains, or reaches more than 512 filters (models.ResNet50Like), keeps
    running unfused.  The outputs differ from ``fused_convs=False`` by
    roundings: ``aff`` is not torch's BatchNorm kernel bit for bit, and an ulp can move a code.  Refused without ``direct`` or with
    ``emulate``.  Without it (the default) nothing changes.
    ``wide_convs=True`` (with ``fused_convs=True``): a module that states ``i8_wide_chains()`` (models._BottleneckBlock: conv1 ->
    conv2 -> conv3 with the shortcut as conv3's residual, and the one-conv chain of a projection shortcut) gets them parked as
    above, all or none, with up to 2048 filters on a conv: its chains run through ``i8_conv_chain(..., out_pixels=True,
    wide=True)``, where a conv of more than 512 filters goes through the epilogue that parks its row in LDS
    (ops.i8_conv2d_quantize, ``wide``).  models.ResNet50Like then runs its 16 bottleneck blocks from pixel operand to pixel
    operand (52 convs listed; the last block's conv3 writes fp32 for the mean).  Without it (the default) ``i8_wide_chains`` is not
    read and nothing changes.
    ``pooled_convs=True`` (with ``fused_convs=True``): a module that states ``i8_pooled_chain()`` -- ``(chain, pools)``, as
    models.CIFARCNN states its six convs with the MaxPool(2) of blocks 1 and 2 -- and whose layers all pass ``i8_direct_eligible``
    evaluates its conv stack in eval mode through ``i8_conv_chain(..., pools=pools)`` instead of its ``i8_conv_chains()``: a conv
    before a pool takes the 2 x 2 maximum in its own epilogue (ops.i8_conv2d_quantize, ``pool``), so the model runs from its
    first conv to its last from pixel operand to pixel operand, and ``fused_conv_layers`` lists five layers for it.  The pool is
    exact, but the BatchNorm before it is now ``bn_affine``'s ``(g, h)`` in the epilogue where ``fused_convs`` alone runs torch's
    kernel on the fp32 result, so the outputs differ from ``fused_convs`` alone by those roundings (an ulp can move a code); bit
    for bit they are ``call_i8_direct`` -> relu -> ``.mul(g)`` -> ``.add(h)`` -> ``F.max_pool2d`` written out.  Without it (the default) ``i8_pooled_chain`` is not read and nothing changes.
    ``stem_convs=True`` (with ``convs=True, direct=True``): a conv that can run as a stem convolution (``i8_stem_eligible``: at most
    4 input channels, a kernel of at most 16 x 8) and that ``direct`` leaves on the im2col path -- the first conv of every model
    here -- computes what its ``call_i8_stem`` does instead: its input quantised once per image ROW (ops.i8_rows_quantize), a kernel
    row per step of the matrix instruction (ops.i8_stem_conv2d), no im2col matrix and no padded channels.  It is listed in
    ``stem_layers`` as well as in ``layers``.  With ``fused_convs`` / ``pooled_convs`` a stated chain that BEGINS with such a conv
    (of at most 128 filters) runs it through the stem entry and its pixel-operand epilogue (``i8_conv_chain(..., stem=True)``):
    models.CIFARCNN then runs conv 1 to conv 6 with no padded-channel product.  Without ``stem_pool`` the ResNets' stems write
    fp32 and their 3 x 3 / 2 max-pool is torch's.  The activation scale is per row there, so the outputs differ from
    ``stem_convs=False``; refused with ``emulate``.  Without it (the default) nothing changes.
    ``stem_pool=True`` (with ``stem_convs=True`` and ``fused_convs=True``; ``wide_convs=True`` too for models.ResNet50Like): a model
    that states ``i8_stem_chain()`` -- ``(chain, pools)``: its stem conv with activation and BatchNorm, and the 3 x 3 / 2 pool behind
    it -- whose stem conv took the stem path (at most 128 filters) gets the chain parked with its affine as ``(g, h)``; where all its
    blocks fuse, its eval forward runs ``i8_rows_quantize`` -> the pooled stem epilogue (ops.i8_stem_conv2d_quantize, ``pool=3``) ->
    the blocks, int8 from the image rows to the last block, and the stem is listed in ``fused_conv_layers``.  The BatchNorm is then
    ``bn_affine``'s product and sum, so the outputs differ from ``stem_pool=False`` in the last bits; bit for bit they are
    ``call_i8_stem`` -> ``.mul(g)`` -> ``.add(h)`` -> relu -> ``F.pad(-inf)`` -> ``F.max_pool2d(3, 2)`` -> ``i8_pixels_quantize``
    written out.  Refused without ``stem_convs`` and ``fused_convs``, or with ``emulate``.  Without it (the default)
    ``i8_stem_chain`` is not read and nothing changes."""

    _family, _dense_eligible = _I8, staticmethod(i8_hardware_eligible)

    def __init__(self, model: nn.Module, act_block=0, emulate=False, convs=False, fused=False, offsets=False, direct=False,
                 int4=False, fused_convs=False, wide_convs=False, pooled_convs=False, stem_convs=False, stem_pool=False):
        self.stem_convs, self.stem_layers, self._stem_modules = bool(stem_convs), [], []
        self.stem_pool, self._stem_pool_modules = bool(stem_pool), []
        if self.stem_pool and emulate:
            raise ValueError("i8_hardware: emulate=True with stem_pool=True: the emulated path has no row-scaled operand and no "
                             "pixel-operand epilogue")
        if self.stem_pool and not (stem_convs and fused_convs):
            raise ValueError("i8_hardware: stem_pool=True needs stem_convs=True and fused_convs=True: it takes the max-pool behind a "
                             "stem convolution into its pixel-operand epilogue, which feeds the fused conv chains")
        if self.stem_convs and not (convs and direct):
            raise ValueError("i8_hardware: stem_convs=True needs convs=True and direct=True: it takes the first conv off the im2col "
                             "path that direct=True leaves it on")
        if self.stem_convs and emulate:
            raise ValueError("i8_hardware: emulate=True with stem_convs=True: the emulated path has no row-scaled operand")
        self.direct, self.direct_layers = bool(direct), []
        self.fused_convs, self.fused_conv_layers, self._fused_conv_modules = bool(fused_convs), [], []
        self.wide_convs = bool(wide_convs)
        if self.wide_convs and not self.fused_convs:
            raise ValueError("i8_hardware: wide_convs=True needs fused_convs=True: it widens the pixel-operand epilogue of the fused "
                             "conv chains to 2048 filters")
        self.pooled_convs, self._pooled_conv_modules = bool(pooled_convs), []
        if self.pooled_convs and not self.fused_convs:
            raise ValueError("i8_hardware: pooled_convs=True needs fused_convs=True: it takes the max-pool between fused conv chains "
                             "into the pixel-operand epilogue")
        if self.fused_convs and not (convs and direct):
            raise ValueError("i8_hardware: fused_convs=True needs convs=True and direct=True: the epilogue writes the pixel operand of "
                             "the direct int8 convolution")
        if self.fused_convs and emulate:
            raise ValueError("i8_hardware: emulate=True with fused_convs=True: the emulated path is the yardstick of the unfused path "
                             "and has no pixel-operand epilogue")
        self.int4, self.int4_layers = bool(int4), []
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

    def _conv_eligible(self, layer, **opt_in):
        """The convs of the im2col path: with ``direct`` those that the direct path does not take."""
        return i8_conv_eligible(layer, **opt_in) and not (self.direct and _takes_direct(layer)) \
            and not (self.stem_convs and _takes_stem(layer))

    def _operand_kwargs(self, layer):
        return {**self._opt_in, "int4": True} if self.int4 and i8_int4_eligible(layer, **self._opt_in) else self._opt_in

    def __enter__(self):
        direct = [m for m in custom_layers_of(self.model) if _takes_direct(m)] if self.direct and self.convs else []
        stem = [m for m in custom_layers_of(self.model) if _takes_stem(m)] if self.stem_convs else []
        self.int4_layers = []
        with torch.no_grad():     # every operand before any layer switches: an exception here leaves the model as it was
            parked = [(m.nested_q_k_layer(m.kernel).detach().permute(3, 2, 0, 1) if self.emulate else m.i8_direct_operand(),
                       m.nested_q_b_layer(m.b).detach() if m._has_bias else None) for m in direct]
            parked_stem = [(m.i8_stem_operand(), m.nested_q_b_layer(m.b).detach() if m._has_bias else None) for m in stem]
        super().__enter__()
        self.int4_layers = [m for m in self.layers if isinstance(getattr(m, _I8.hw)[0], ops.I4Operand)]
        for m, hw in zip(direct, parked):
            m._i8_direct_hw = hw
        for m, hw in zip(stem, parked_stem):
            m._i8_stem_hw = hw
        self.direct_layers, self.stem_layers = direct, stem
        if direct or stem:        # ``layers``: the Dense layers, then the conv layers of every path in module order
            order = {id(m): k for k, m in enumerate(custom_layers_of(self.model))}
            dense = [m for m in self.layers if isinstance(m, CustomDenseLayer)]
            convs = [m for m in self.layers if not isinstance(m, CustomDenseLayer)] + direct + stem
            self.layers = dense + sorted(convs, key=lambda m: order[id(m)])
        if self.fused_convs:
            self._enter_fused_convs()
        if self.stem_pool:
            self._enter_stem_pool()
        return self

    def _enter_stem_pool(self):
        """A module that states ``i8_stem_chain()`` -- (chain, pools): one step, its stem conv -- whose conv ``stem_convs`` took
        (at most 128 filters) and whose blocks ALL fused (its forward takes the pooled stem only then) gets the chain with its
        affine as ``(g, h)`` and the pools; the conv is a fused layer then."""
        for mod in self.model.modules():
            if not callable(getattr(mod, "i8_stem_chain", None)):
                continue
            blocks = [b for b in mod.modules() if callable(getattr(b, "i8_fused", None))]
            if not blocks or any(getattr(b, "_i8_fused_convs", None) is None or None in b._i8_fused_convs for b in blocks):
                continue
            chain, pools = mod.i8_stem_chain()
            (c, act, aff, first), = chain
            if c._i8_stem_hw is None or c.filters > ops.I8_STEM_QUANT_MAX_FILTERS or act not in ops.MX_ACTIVATIONS:
                continue
            c._i8_chain_hw = c._i8_stem_hw
            mod._i8_stem_pool = ([(c, act, bn_affine(aff) if isinstance(aff, nn.BatchNorm2d) else aff, first)], list(pools))
            self.fused_conv_layers.insert(0, c)
            self._stem_pool_modules.append(mod)

    def _stated_chains(self, mod):
        """(chains, every, most) of a module: what it states as ``i8_conv_chains()``, whether it runs them with ``out_pixels=True``
        (``i8_chains_out_pixels``), and the filters an epilogue of them takes.  Under ``wide_convs`` a module may state
        ``i8_wide_chains()`` instead (models._BottleneckBlock): run with ``out_pixels=True, wide=True``, up to 2048 filters."""
        if callable(getattr(mod, "i8_conv_chains", None)):
            return mod.i8_conv_chains(), bool(getattr(mod, "i8_chains_out_pixels", False)), ops.I8_CONV_QUANT_MAX_FILTERS
        if self.wide_convs and callable(getattr(mod, "i8_wide_chains", None)):
            return mod.i8_wide_chains(), True, ops.I8_CONV_QUANT_WIDE_MAX_FILTERS
        return [], False, 0

    def _enter_fused_convs(self):
        """A module that states conv chains (``i8_conv_chains()``: lists of (conv, activation, BatchNorm2d or (g, h) or None,
        affine_first)) gets, per chain whose layers all pass ``i8_direct_eligible``, the chain with its affines as ``(g, h)`` --
        None for a chain that cannot fuse -- and the chain's layers their operands."""
        self.fused_conv_layers, self._fused_conv_modules = [], []
        with torch.no_grad():
            for mod in self.model.modules():
                if self.pooled_convs and self._enter_pooled_convs(mod):
                    continue
                stated, every, most = self._stated_chains(mod)
                parked = []
                for chain in stated:
                    ok = (len(chain) > 1 or every) and all(i8_direct_eligible(c) and act in ops.MX_ACTIVATIONS for c, act, _, _ in chain) \
                        and all(c.filters <= most for c, _, _, _ in (chain if every else chain[:-1]))
                    parked.append([(c, act, bn_affine(aff) if isinstance(aff, nn.BatchNorm2d) else aff, first)
                                   for c, act, aff, first in chain] if ok else None)
                if every and any(chain is None for chain in parked):          # such a module's chains feed each other: all or none
                    continue
                if any(chain is not None for chain in parked):
                    for chain in filter(None, parked):
                        for k, (c, _, _, _) in enumerate(chain):
                            c._i8_chain_hw = self._chain_hw(mod, c, k == 0)
                        self.fused_conv_layers += [c for c, _, _, _ in (chain if every else chain[:-1])]
                    mod._i8_fused_convs = parked
                    self._fused_conv_modules.append(mod)

    def _chain_hw(self, mod, c, first):
        """(operand, bias) of a conv of a parked chain: what ``direct`` parked on it, or packed here.  The FIRST conv of a chain
        keeps the stem operand ``stem_convs`` parked on it where the stem epilogue takes its filters; ``mod`` is then marked
        (``_i8_stem_chain``) so that its forward asks ``i8_conv_chain`` for ``stem=True``."""
        if first and c._i8_stem_hw is not None and c.filters <= ops.I8_STEM_QUANT_MAX_FILTERS:
            mod._i8_stem_chain = True
            self._stem_modules.append(mod)
            return c._i8_stem_hw
        return c._i8_direct_hw or (c.i8_direct_operand(), c.nested_q_b_layer(c.b).detach() if c._has_bias else None)

    def _enter_pooled_convs(self, mod):
        """A module that states ``i8_pooled_chain()`` -- (chain, pools) -- whose layers all pass ``i8_direct_eligible`` gets the
        chain with its affines as ``(g, h)`` and the pools, and the layers their operands; True then.  Otherwise nothing changes
        and its ``i8_conv_chains()`` are read as ever."""
        if not callable(getattr(mod, "i8_pooled_chain", None)):
            return False
        chain, pools = mod.i8_pooled_chain()
        if not (all(i8_direct_eligible(c) and act in ops.MX_ACTIVATIONS for c, act, _, _ in chain)
                and all(c.filters <= ops.I8_CONV_QUANT_MAX_FILTERS for c, _, _, _ in chain[:-1])):
            return False
        for k, (c, _, _, _) in enumerate(chain):
            c._i8_chain_hw = self._chain_hw(mod, c, k == 0)
        self.fused_conv_layers += [c for c, _, _, _ in chain[:-1]]
        mod._i8_pooled_convs = ([(c, act, bn_affine(aff) if isinstance(aff, nn.BatchNorm2d) else aff, first)
                                 for c, act, aff, first in chain], list(pools))
        self._pooled_conv_modules.append(mod)
        return True

    def __exit__(self, *exc):
        for mod in self._stem_pool_modules:
            mod._i8_stem_pool[0][0][0]._i8_chain_hw = None
            mod._i8_stem_pool = None
        self._stem_pool_modules = []
        for mod in self._pooled_conv_modules:
            for c, _, _, _ in mod._i8_pooled_convs[0]:
                c._i8_chain_hw = None
            mod._i8_pooled_convs = None
        self._pooled_conv_modules = []
        for mod in self._fused_conv_modules:
            mod._i8_fused_convs = None
            for chain in filter(None, self._stated_chains(mod)[0]):
                for c, _, _, _ in chain:
                    c._i8_chain_hw = None
        self._fused_conv_modules = []
        for m in self.direct_layers:
            m._i8_direct_hw = None
        for m in self.stem_layers:
            m._i8_stem_hw = None
        for mod in self._stem_modules:
            mod._i8_stem_chain = False
        self._stem_modules = []
        return super().__exit__(*exc)


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


def mx_dense_chain(x, chain, act_format="fp8_e4m3", act_scale="mx", fp6=False):
    """``chain`` = [(layer, activation), ...]: Dense layers applied one after the other on the block-scaled matrix instruction, under
    ``no_grad``.  ``x`` is quantised once (ops.mx_operand_quantize); every layer but the last goes through ops.mx_gemm_quantize, which
    applies its activation (None or "relu") and writes the next layer's operand (``act_format`` under ``act_scale``) in the product's
    epilogue; the last goes through ops.mx_gemm to fp32 and takes no activation.  Bit for bit ``call_mx`` -> activation -> ``call_mx``
    ..., without the fp32 activations and their launches.  Inside ``mx_hardware`` the operands and biases built on its entry are
    used, otherwise they are built here.  ValueError naming the reason for a layer that cannot take the path
    (``mx_hardware_eligible``) or an activation other than None / "relu".  ``fp6=True`` lets layers with an fp6 element format take
    the path (``mx_operand(fp6=True)``); the operands between the layers stay ``act_format``."""
    def check_act():
        ops.check_mx_operand_format(act_format)
        ops.check_mx_scale_init(act_scale)
    opt_in = {"fp6": True} if fp6 else {}
    return _dense_chain("mx_dense_chain", _MX, "block-scaled",
                        lambda layer: ops.check_mx_operand_layer(layer.element_format, layer.scale_format, layer.group_size, **opt_in),
                        check_act, x, chain, (act_format, act_scale), act_format, **opt_in)


def i8_dense_chain(x, chain, act_block=64, offsets=False, int4=False):
    """``chain`` = [(layer, activation), ...]: Dense layers applied one after the other on the int8 matrix instruction, under
    ``no_grad``.  ``x`` is quantised once per row and ``act_block`` inputs (ops.i8_operand_quantize); every layer but the last goes
    through ops.i8_gemm_quantize, which applies its activation (None or "relu") and writes the next layer's operand, per row and
    block of 64, in the product's epilogue; the last goes through ops.i8_gemm to fp32 and takes no activation.  Bit for bit
    ``call_i8(act_block)`` -> activation -> ``call_i8(act_block=64)`` ..., without the fp32 activations and their launches.  Inside
    ``i8_hardware`` the operands and biases built on its entry are used, otherwise they are built here.  ValueError naming the
    reason for a layer that cannot take the path (``i8_hardware_eligible``) or an activation other than None / "relu".
    ``offsets=True`` lets asymmetric layers take the path (``i8_operand(offsets=True)``): the epilogue's product adds the offset
    term too, so the bits stay those of the unfused path.  ``int4=True``: every layer multiplies with its packed 4-bit operand
    (``i8_operand(int4=True)``; a layer whose range does not fit [-8, 7] is refused) -- the same bits again.  Inside ``i8_hardware``
    the operands parked on its entry are used whatever ``int4`` says here, packed or not: the bits are the same."""
    opt_in = {"offsets": True} if offsets else {}
    if int4:
        opt_in["int4"] = True
    return _dense_chain("i8_dense_chain", _I8, "int8", lambda layer: layer._check_i8(**opt_in),
                        lambda: ops.check_i8_block(act_block), x, chain, (act_block,), ops.I8_OUT_BLOCK, **opt_in)


def bn_affine(bn: nn.BatchNorm2d):
    """``(g, h)``, float32 ``(C,)`` each, of an eval-mode ``BatchNorm2d``: ``bn(v) = v g + h`` with ``g = gamma / sqrt(var + eps)`` and
    ``h = beta - mean g``, computed in float64 and rounded once -- the affine of ops.i8_conv2d_quantize's epilogue.  (torch's own
    eval-mode kernel rounds differently: the two agree to an ulp or so, not bit for bit.)"""
    if not isinstance(bn, nn.BatchNorm2d) or bn.training or bn.running_mean is None or bn.running_var is None:
        raise ValueError("bn_affine: needs a BatchNorm2d in eval mode with running statistics")
    with torch.no_grad():
        one = torch.ones_like(bn.running_var, dtype=torch.float64)
        gamma = bn.weight.double() if bn.weight is not None else one
        beta = bn.bias.double() if bn.bias is not None else 0.0 * one
        g = gamma / torch.sqrt(bn.running_var.double() + bn.eps)
        return g.float(), (beta - bn.running_mean.double() * g).float()


def i8_conv_chain(x, chain, max_lines=None, out_pixels=False, wide=False, pools=None, stem=False):
    """``chain`` = [(conv, activation, affine, affine_first), ...]: conv layers applied one after the other as direct int8
    convolutions, under ``no_grad``.  ``x`` is quantised once per pixel; every layer but the last goes through
    ops.i8_conv2d_quantize, whose epilogue applies ``activation`` (None or "relu") and ``affine`` (None or ``(g, h)``, ``bn_affine``)
    -- ``affine_first`` False: relu then affine, True: affine then relu -- and writes the next conv's pixel operand; the last goes
    through ops.i8_conv2d to fp32 and takes no epilogue.  Bit for bit ``call_i8_direct`` -> relu -> ``.mul(g)`` -> ``.add(h)`` ->
    ``call_i8_direct`` ..., without the fp32 activations and their launches.  A batch whose lines exceed the launch limit (or
    ``max_lines``) is cut into runs of whole images; the result does not depend on the cut.  Inside ``i8_hardware(fused_convs=True)``
    the operands parked on its entry are used, otherwise they are built here.  ValueError naming the reason for a layer that cannot
    take the path (``i8_direct_eligible``), more than 512 filters on a layer with an epilogue, or an epilogue on the last layer.
    A step may carry a fifth entry, the RESIDUAL of its epilogue: an ops.I8Pixels of the step's output shape (or None), decoded and
    added directly before the activation (ops.i8_conv2d_quantize, ``residual``).  ``out_pixels=True``: the LAST layer goes through
    the epilogue too, with its activation, affine and residual, and the chain returns an ops.I8Pixels; ``x`` may itself be one.
    So a basic ResNet block is ``[(conv1, "relu", bn1, True), (conv2, "relu", bn2, True, shortcut)]`` with ``out_pixels=True``.
    A residual on a last layer that writes fp32 is refused: the fp32 result has no epilogue to add it in.
    ``wide=True``: a layer with an epilogue may have up to 2048 filters (ops.I8_CONV_QUANT_WIDE_MAX_FILTERS); one of more than 512
    goes through ops.i8_conv2d_quantize(..., wide=True), every other where it goes without the flag, so a chain can mix widths.
    So a bottleneck block is ``[(conv1, "relu", bn1, True), (conv2, "relu", bn2, True), (conv3, "relu", bn3, True, shortcut)]``.
    ``pools``: a sequence with one entry per step, None or 2.  A step with 2 takes the non-overlapping 2 x 2 maximum after its
    activation and affine, in the same epilogue (ops.i8_conv2d_quantize, ``pool``), and writes the pixel operand of the pooled
    image: conv -> relu -> BN -> MaxPool(2) -> conv without an fp32 activation.  It is refused on a step that writes fp32, has
    a residual or has more than 512 filters.  So models.CIFARCNN's six convs are one chain (``i8_pooled_chain()``).
    ``stem=True``: the FIRST conv runs as a stem convolution (``call_i8_stem``): ``x``, a tensor of at most 4 channels, is quantised
    per image row and multiplied a kernel row per step, with no padded channels; where the step has an epilogue it is
    ops.i8_stem_conv2d_quantize's (at most 128 filters, no residual).  The rest of the chain is unchanged.  Bit for bit
    ``call_i8_stem`` -> relu -> ``.mul(g)`` -> ``.add(h)`` -> ``call_i8_direct`` ....  ValueError naming the reason for a first
    conv that cannot take it (``i8_stem_eligible``).  Without it (the default) nothing changes.
    The stem step, and no other, takes 3 in ``pools``: the 3 x 3 maximum of stride 2 under TensorFlow's "same" pool paddings in the
    stem epilogue (``call_i8_stem``, ``pool``), so a ResNet's stem is ``[(stem, "relu", bn0, True)]`` with ``pools=[3]``,
    ``stem=True`` and ``out_pixels=True``: image rows in, the first block's pixel operand out."""
    fn = "i8_conv_chain"
    chain = [tuple(step) for step in chain]
    _check_max_lines(max_lines)
    if not chain:
        raise ValueError(f"{fn}: the chain is empty")
    if stem:
        first = chain[0][0]
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{fn}: stem=True: the stem convolution quantises a tensor itself, got {type(x).__name__}")
        try:
            if isinstance(first, _ConvBase):
                first._check_i8_stem()
        except ValueError as e:
            raise ValueError(f"{fn}: stem=True: {first.name}: {e}") from None
        epilogue = out_pixels or len(chain) > 1
        if epilogue and getattr(first, "filters", 0) > ops.I8_STEM_QUANT_MAX_FILTERS:
            raise ValueError(f"{fn}: stem=True: {first.name}: {first.filters} filters: the stem epilogue holds a whole output row in one "
                             f"wave, at most {ops.I8_STEM_QUANT_MAX_FILTERS}")
        if (pools is not None and list(pools)[:1] not in ([], [None], [3])) or (len(chain[0]) == 5 and chain[0][4] is not None):
            raise ValueError(f"{fn}: stem=True: the stem epilogue takes no pool but 3 (the 3 x 3 / 2 maximum) and no residual")
    pools = [None] * len(chain) if pools is None else list(pools)
    if len(pools) != len(chain):
        raise ValueError(f"{fn}: pools has {len(pools)} entries for {len(chain)} steps: one per step, None or 2")
    for k, pool in enumerate(pools):
        if pool is None:
            continue
        on_stem = stem and k == 0 and pool == 3 and not isinstance(pool, bool)
        if not on_stem and (isinstance(pool, bool) or pool != 2):
            raise ValueError(f"{fn}: step {k}: pool={pool!r}: only the non-overlapping 2 x 2 maximum (2) is built, or None; the 3 x 3 "
                             "/ 2 maximum (3) on the step of a stem convolution (stem=True, step 0) only")
        if k == len(chain) - 1 and not out_pixels:
            raise ValueError(f"{fn}: step {k}: a pool on the last layer, which writes fp32: apply F.max_pool2d to the result, or ask "
                             "for out_pixels=True")
        if len(chain[k]) == 5 and chain[k][4] is not None:
            raise ValueError(f"{fn}: step {k}: a pool on a step with a residual is not built")
        if len(chain[k]) in (4, 5) and getattr(chain[k][0], "filters", 0) > ops.I8_CONV_QUANT_MAX_FILTERS:
            raise ValueError(f"{fn}: step {k}: a pool on a step with {chain[k][0].filters} filters: the pooled epilogue holds its row "
                             f"in registers, at most {ops.I8_CONV_QUANT_MAX_FILTERS}")
    for k, step in enumerate(chain):
        if len(step) not in (4, 5):
            raise ValueError(f"{fn}: step {k} must be (conv, activation, affine, affine_first) or the same and a residual, got "
                             f"{len(step)} entries")
        layer, activation, affine, affine_first = step[:4]
        residual = step[4] if len(step) == 5 else None
        if residual is not None and not isinstance(residual, ops.I8Pixels):
            raise ValueError(f"{fn}: step {k}: the residual must be an ops.I8Pixels or None, got {type(residual).__name__}")
        if not isinstance(layer, _ConvBase):
            raise ValueError(f"{fn}: layer {k} is a {type(layer).__name__}: only conv layers run as direct int8 convolutions")
        try:
            layer._check_i8_direct()
            ops.check_mx_activation(activation)
        except ValueError as e:
            raise ValueError(f"{fn}: {layer.name}: {e}") from None
        if k == len(chain) - 1 and not out_pixels:
            if activation is not None or affine is not None or affine_first:
                raise ValueError(f"{fn}: {layer.name}: the last layer writes fp32 and takes no epilogue (got activation={activation!r}, "
                                 f"affine {'given' if affine is not None else 'None'}): apply it to the result")
            if residual is not None:
                raise ValueError(f"{fn}: {layer.name}: the last layer writes fp32 and has no epilogue to add a residual in: add it to "
                                 "the result, or ask for out_pixels=True")
        elif wide and layer.filters > ops.I8_CONV_QUANT_WIDE_MAX_FILTERS:
            raise ValueError(f"{fn}: {layer.name}: {layer.filters} filters: the wide epilogue parks a whole output row in LDS, at most "
                             f"{ops.I8_CONV_QUANT_WIDE_MAX_FILTERS}")
        elif not wide and layer.filters > ops.I8_CONV_QUANT_MAX_FILTERS:
            raise ValueError(f"{fn}: {layer.name}: {layer.filters} filters: the epilogue holds a whole output row in one thread block, "
                             f"at most {ops.I8_CONV_QUANT_MAX_FILTERS}")
    with torch.no_grad():
        a = x
        for k, step in enumerate(chain):
            layer, activation, affine, affine_first = step[:4]
            hw = layer._i8_chain_hw
            operand, qb = hw if hw is not None else (layer.i8_direct_operand(), layer.nested_q_b_layer(layer.b) if layer._has_bias else None)
            by_row = stem and k == 0
            if by_row != isinstance(operand, ops.I8StemKernel):       # the parked operand is the other path's: pack this path's here
                operand = layer.i8_stem_operand() if by_row else layer.i8_direct_operand()
            a = layer._direct_step(a, operand, qb, max_lines, out_pixels or k < len(chain) - 1, activation, affine, affine_first,
                                   step[4] if len(step) == 5 else None, wide and pools[k] is None and not by_row, pools[k])
        return a


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
