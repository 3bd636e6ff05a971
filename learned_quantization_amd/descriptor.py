"""Scale shapes and the (outer, G, inner) group descriptor of the C ABI.

``scale_shape`` restates CustomQuantizedScaleLayer.build
(/root/reference/MNIST/nested_quantization_layer/custom_components/custom_layers.py:147-197):
rowwise keeps axis 0, columnwise axis 1, channelwise axis 2, scalar is ``(1,)``;
any other string raises ``ValueError`` with the reference's message (:194-197).

``group_descriptor`` maps (parameter shape, scale shape) to the descriptor of
include/lq_hip.h: element ``i`` of the contiguous parameter uses scale element
``(i // inner) % G``.

``memory_order`` / ``memory_descriptor`` do the same for a parameter whose MEMORY is a permutation of its logical axes
(a conv kernel presented HWIO like the reference's, custom_layers.py:321, but stored in the OIHW order the convolution
library consumes): the descriptor then speaks about the element order in memory, which is all the kernels see.

``groupwise_scale_shape`` / ``group_geometry`` are the second descriptor, for group-wise (block) scales (include/lq_hip.h,
lq_fq_forward_group): the parameter's memory seen as a matrix [R][C] with groups of ``group_size`` along one of the two axes,
which the flat rule above cannot express (groups along the strided axis, ragged lines).

``init_geometry`` maps ANY scale of a clipped layer -- group-wise, one-axis or scalar -- to that matrix form for scale
initialisation (lq_scale_init_group), or says that its groups are not lines of a matrix.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

ORIENTATIONS = ("rowwise", "columnwise", "channelwise", "scalar")

_AXIS = {"rowwise": 0, "columnwise": 1, "channelwise": 2}


def scale_shape(input_shape: Sequence[int], orientation: str) -> Tuple[int, ...]:
    input_shape = tuple(int(d) for d in input_shape)
    if orientation in _AXIS:
        axis = _AXIS[orientation]
        return tuple(input_shape[i] if i == axis else 1 for i in range(len(input_shape)))
    if orientation == "scalar":
        return (1,)
    raise ValueError(
        f"Invalid scaler application: {orientation}. Expected rowwise, columnwise or scalar."
    )


def group_descriptor(param_shape: Sequence[int], scale_shape_: Sequence[int]) -> Tuple[int, int, int]:
    param_shape = tuple(int(d) for d in param_shape)
    scale_shape_ = tuple(int(d) for d in scale_shape_)
    numel = math.prod(param_shape) if param_shape else 1
    if numel <= 0:
        raise ValueError(f"parameter must be non-empty, got shape {param_shape}")
    if len(scale_shape_) == 1 and scale_shape_[0] == 1:
        return 1, 1, numel
    if len(scale_shape_) != len(param_shape):
        raise ValueError(
            f"scale shape {scale_shape_} is not broadcast-compatible with parameter shape {param_shape}: "
            "rank must match (or the scale must be (1,))"
        )
    axes = [i for i, d in enumerate(scale_shape_) if d != 1]
    if not axes:
        return 1, 1, numel
    if len(axes) > 1:
        raise ValueError(f"scale shape {scale_shape_} has more than one non-unit axis")
    a = axes[0]
    if scale_shape_[a] != param_shape[a]:
        raise ValueError(f"scale axis {a} has length {scale_shape_[a]}, parameter has {param_shape[a]}")
    outer = math.prod(param_shape[:a]) if a > 0 else 1
    inner = math.prod(param_shape[a + 1:]) if a + 1 < len(param_shape) else 1
    return outer, param_shape[a], inner


def memory_order(shape: Sequence[int], strides: Sequence[int]) -> Optional[Tuple[int, ...]]:
    """Logical axes from the slowest- to the fastest-varying one in memory, or ``None`` when the tensor is not a dense
    permutation of a contiguous array (gaps, overlaps, broadcast strides).  Unit axes keep their logical position."""
    shape, strides = tuple(int(d) for d in shape), tuple(int(d) for d in strides)
    order = sorted(range(len(shape)), key=lambda a: (-strides[a] if shape[a] != 1 else 0, a))
    # unit axes may carry any stride: place them by position only (their stride never addresses anything)
    real = [a for a in order if shape[a] != 1]
    expect = 1
    for a in reversed(real):
        if strides[a] != expect:
            return None
        expect *= shape[a]
    units = [a for a in range(len(shape)) if shape[a] == 1]
    return tuple(real + units) if real else tuple(range(len(shape)))


def memory_descriptor(shape: Sequence[int], strides: Sequence[int], scale_shape_: Sequence[int]) -> Optional[Tuple[int, int, int]]:
    """(outer, G, inner) over the parameter's elements IN MEMORY ORDER, or ``None`` when the memory is not a dense permutation
    of the logical axes.  Equals ``group_descriptor`` for a contiguous parameter."""
    shape = tuple(int(d) for d in shape)
    scale_shape_ = tuple(int(d) for d in scale_shape_)
    order = memory_order(shape, strides)
    if order is None:
        return None
    if order == tuple(range(len(shape))) or (len(scale_shape_) == 1 and scale_shape_[0] == 1):
        return group_descriptor(shape, scale_shape_)
    if len(scale_shape_) != len(shape):
        return group_descriptor(shape, scale_shape_)          # raises with the usual message
    return group_descriptor(tuple(shape[a] for a in order), tuple(scale_shape_[a] for a in order))


def _check_group_size(group_size) -> int:
    if isinstance(group_size, bool) or int(group_size) != group_size or int(group_size) < 1:
        raise ValueError(f"group_size must be an integer >= 1, got {group_size!r}")
    return int(group_size)


def groupwise_scale_shape(param_shape: Sequence[int], group_size: int) -> Tuple[int, int]:
    """Scale shape of ``orientation="groupwise"``: one scale per group of ``group_size`` consecutive inputs of each output unit.
    The LAST logical axis holds the output units (Dense ``(in, out)``, conv HWIO ``(kh, kw, ci, co)``) and the others are its
    inputs, ``fan_in`` of them; ``nb = ceil(fan_in / group_size)`` (the last group may be short).  A 2-D parameter gets
    ``(nb, out)`` -- its memory is ``(in, out)``, the groups run along the strided axis -- and a parameter of more axes gets
    ``(out, nb)``: its groups run along the contiguous (ci, kh, kw) run of each output channel of an OIHW-stored kernel."""
    param_shape = tuple(int(d) for d in param_shape)
    gs = _check_group_size(group_size)
    if len(param_shape) < 2 or min(param_shape) <= 0:
        raise ValueError(f"group-wise scales need a parameter of at least two non-empty axes (inputs..., outputs), got shape {param_shape}")
    out = param_shape[-1]
    nb = -(-math.prod(param_shape[:-1]) // gs)
    return (nb, out) if len(param_shape) == 2 else (out, nb)


def group_geometry(shape: Sequence[int], strides: Sequence[int], scale_shape_: Sequence[int], group_size: int) -> Tuple[int, int, int]:
    """(R, C, axis) of include/lq_hip.h's group-wise entry points for a parameter of ``shape`` / ``strides`` and a 2-D scale:
    the parameter's axes IN MEMORY ORDER split into a slow part of R and a contiguous part of C elements such that the scale is
    ``(R, ceil(C / group_size))`` (axis 1, groups along the contiguous axis) or ``(ceil(R / group_size), C)`` (axis 0, groups
    along the strided axis).  Raises ValueError when the memory is not a dense permutation of the logical axes or no split fits
    -- the groups are defined in memory order, so a scale built for another storage order does not fit."""
    shape = tuple(int(d) for d in shape)
    scale_shape_ = tuple(int(d) for d in scale_shape_)
    gs = _check_group_size(group_size)
    order = memory_order(shape, strides)
    if order is None:
        raise ValueError(f"group-wise scales need a dense parameter (a permutation of a contiguous array), got shape {shape} "
                         f"with strides {tuple(int(d) for d in strides)}")
    if len(scale_shape_) != 2:
        raise ValueError(f"a group-wise scale is a matrix, got shape {scale_shape_}")
    dims = [shape[a] for a in order]
    if not dims or math.prod(dims) <= 0:
        raise ValueError(f"parameter must be non-empty, got shape {shape}")
    if math.prod(dims) >= 1 << 31:
        raise ValueError(f"group-wise scales take parameters below 2^31 elements, got {math.prod(dims)}")
    for k in range(1, len(dims)):
        R, C = math.prod(dims[:k]), math.prod(dims[k:])
        if scale_shape_ == (R, -(-C // gs)):
            return R, C, 1
        if scale_shape_ == (-(-R // gs), C):
            return R, C, 0
    raise ValueError(f"scale shape {scale_shape_} fits no split of the parameter's memory-order extents {tuple(dims)} into [R][C] "
                     f"with groups of {gs} along one axis (the groups are defined in memory order)")


def init_geometry(shape: Sequence[int], strides: Sequence[int], scale_shape_: Sequence[int],
                  group_size: Optional[int] = None) -> Tuple[int, int, int, int]:
    """(R, C, axis, gs) of include/lq_hip.h's lq_scale_init_group for ANY scale of a clipped layer.  A group-wise scale
    (``group_size`` given) goes through ``group_geometry``.  A one-axis or scalar scale goes through its ``memory_descriptor``
    (outer, G, inner), whose groups are lines of a matrix in three cases: G == 1 -> (1, numel, 1, numel), one group (a bias, a
    scalar scale); outer == 1 -> (G, inner, 1, inner), every row is a group; inner == 1 -> (outer, G, 0, outer), every column is
    a group.  That covers every Dense orientation, biases, scalar scales and channel-wise conv kernels stored OIHW.  With
    outer > 1, G > 1 and inner > 1 a group is a set of separate runs (the reference's row- / column-wise scales of a 4-D conv
    kernel, channel-wise on HWIO storage): ValueError."""
    shape = tuple(int(d) for d in shape)
    scale_shape_ = tuple(int(d) for d in scale_shape_)
    if group_size is not None:
        R, C, axis = group_geometry(shape, strides, scale_shape_, group_size)
        return R, C, axis, _check_group_size(group_size)
    desc = memory_descriptor(shape, strides, scale_shape_)
    if desc is None:
        raise ValueError(f"scale initialisation needs a dense parameter (a permutation of a contiguous array), got shape {shape} "
                         f"with strides {tuple(int(d) for d in strides)}")
    outer, G, inner = desc
    numel = outer * G * inner
    if numel >= 1 << 31:
        raise ValueError(f"scale initialisation takes parameters below 2^31 elements, got {numel}")
    if G == 1:
        return 1, numel, 1, numel
    if outer == 1:
        return G, inner, 1, inner
    if inner == 1:
        return outer, G, 0, outer
    raise ValueError(f"scale shape {scale_shape_} on a parameter of shape {shape}: in memory order the groups are "
                     f"(outer, G, inner) = {desc}, {outer} separate runs of {inner} elements each -- the groups are not lines of a "
                     "matrix, which scale initialisation needs; use a scalar, channel-wise (OIHW storage) or group-wise scale, "
                     "or set the scales directly")
