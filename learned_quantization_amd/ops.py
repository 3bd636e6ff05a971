"""Operators of the learned-quantization hot path on top of the C ABI (include/lq_hip.h).

``my_custom_gradient`` keeps the reference's name, argument order and meaning:
  * 3-argument form ``(parameter, scale, penalty_threshold)`` = nested-quantization op
    /root/reference/MNIST/nested_quantization_layer/custom_components/custom_layers.py:49-120
  * 2-argument form ``(parameter, scale)`` = STE-only op
    /root/reference/CIFAR-10/custom_loss_terms/custom_components/custom_layers.py:49-64

Raw (non-autograd) wrappers ``fq_forward``, ``fq_scale_grad``, ``fq_scale_grad_ste``, ``fq_forward_clip``,
``fq_backward_clip``, ``fq_forward_group``, ``fq_backward_group``, ``fq_forward_group_affine``, ``fq_backward_group_affine``,
``scale_init_group``, ``scale_init_group_minmax``, ``group_stats``, ``fq_fwd_bwd_fused``, ``quantized_integers`` ... are thin: argument checking + one C-ABI call each.
Everything runs on the HIP device; there is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _hip
from .descriptor import group_descriptor, group_geometry, init_geometry, memory_descriptor

_QDTYPES = {
    torch.float32: _hip.LQ_Q_F32,
    torch.int32: _hip.LQ_Q_I32,
    torch.int8: _hip.LQ_Q_I8,
}


def _desc(parameter: torch.Tensor, scale: torch.Tensor) -> Tuple[int, int, int]:
    return group_descriptor(tuple(parameter.shape), tuple(scale.shape))


def _q_buffer(p: torch.Tensor, q_dtype: Optional[torch.dtype]):
    """(q, the C ABI's name of its type) for the integer side output of a forward: (None, LQ_Q_NONE) without ``q_dtype``."""
    if q_dtype is None:
        return None, _hip.LQ_Q_NONE
    if q_dtype not in _QDTYPES:
        raise TypeError(f"q_dtype must be one of {list(_QDTYPES)}, got {q_dtype}")
    return torch.empty_like(p, dtype=q_dtype), _QDTYPES[q_dtype]


def _param(parameter: torch.Tensor, scale: torch.Tensor):
    """(P, s, descriptor) as the kernels read them.  A parameter whose memory is a dense permutation of its logical axes -- a
    conv kernel shaped HWIO (custom_layers.py:321) and stored OIHW, layers.py ``kernel_storage`` -- is NOT copied: the groups
    are described in memory order, and every same-shaped output is allocated with the parameter's strides, so that logically
    (index by index) the results are those of the contiguous tensor."""
    p = _hip.require_device_f32(parameter, "parameter", dense_ok=True)
    s = _hip.require_device_f32(scale, "scale")
    return p, s, memory_descriptor(tuple(p.shape), p.stride(), tuple(s.shape))


# --------------------------------------------------------------------------- raw wrappers
def fq_forward(parameter: torch.Tensor, scale: torch.Tensor, q_dtype: Optional[torch.dtype] = None,
               want_out: bool = True):
    """K1.  Returns ``out`` (and ``q`` when ``q_dtype`` is given).  custom_layers.py:55-60."""
    lib = _hip.load()
    p, s, (outer, G, inner) = _param(parameter, scale)
    out = torch.empty_like(p) if want_out else None
    q, qd = _q_buffer(p, q_dtype)
    if out is None and q is None:
        raise ValueError("nothing to compute: want_out=False and q_dtype=None")
    _hip.check(lib.lq_fq_forward(_hip.ptr(p), _hip.ptr(s), _hip.ptr(out), _hip.ptr(q), qd,
                                 outer, G, inner, _hip.stream_ptr(p.device)), "lq_fq_forward")
    if q is None:
        return out
    return (out, q) if want_out else q


def quantized_integers(parameter: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32):
    """floor(P/s): the integer view of callbacks/export (custom_callbacks.py:85-87, log_scripts.py:74-79)."""
    return fq_forward(parameter, scale, q_dtype=dtype, want_out=False)


def fq_scale_grad(parameter: torch.Tensor, scale: torch.Tensor, dy: torch.Tensor, penalty_threshold: float,
                  return_parts: bool = False):
    """K2+K3: the hand-written scale gradient of custom_layers.py:62-118.  Returns ds (shape of scale)."""
    lib = _hip.load()
    p, s, (outer, G, inner) = _param(parameter, scale)
    d = _hip.require_device_f32(dy, "dy", like=p)
    ds = torch.empty_like(s)
    parts = torch.empty(3 * G, dtype=torch.float32, device=p.device) if return_parts else None
    ws = _hip.workspace_for(p.device, outer, G, inner)
    _hip.check(lib.lq_fq_scale_grad(_hip.ptr(p), _hip.ptr(s), _hip.ptr(d), float(penalty_threshold),
                                    _hip.ptr(ds), _hip.ptr(parts), _hip.ptr(ws), ws.numel(),
                                    outer, G, inner, _hip.stream_ptr(p.device)), "lq_fq_scale_grad")
    if return_parts:
        return ds, parts.view(3, G)
    return ds


def fq_scale_grad_ste(parameter: torch.Tensor, scale: torch.Tensor, dy: torch.Tensor, grad_scale: float = 1.0):
    """The straight-through scale gradient (include/lq_hip.h, lq_fq_scale_grad_ste):
    ds[g] = grad_scale * sum_{i in g} dy_i * (floor(P_i/s_g) - P_i/s_g), K1's fp32 quotient, f64 sum.  Returns ds (shape of scale)."""
    lib = _hip.load()
    p, s, (outer, G, inner) = _param(parameter, scale)
    d = _hip.require_device_f32(dy, "dy", like=p)
    ds = torch.empty_like(s)
    ws = _hip.workspace_for(p.device, outer, G, inner)
    _hip.check(lib.lq_fq_scale_grad_ste(_hip.ptr(p), _hip.ptr(s), _hip.ptr(d), float(grad_scale), _hip.ptr(ds),
                                        _hip.ptr(ws), ws.numel(), outer, G, inner, _hip.stream_ptr(p.device)),
               "lq_fq_scale_grad_ste")
    return ds


Q_LIMIT = 1 << 24      # integers up to 2^24 in magnitude are exact in fp32


def check_q_range(qmin, qmax) -> Tuple[int, int]:
    """(qmin, qmax) as ints, or ValueError: qmin <= qmax, both inside +-2^24 (include/lq_hip.h, clipped fake-quant)."""
    if int(qmin) != qmin or int(qmax) != qmax:
        raise ValueError(f"q_range must be two integers, got ({qmin!r}, {qmax!r})")
    qmin, qmax = int(qmin), int(qmax)
    if qmin > qmax:
        raise ValueError(f"q_range needs qmin <= qmax, got ({qmin}, {qmax})")
    if qmin < -Q_LIMIT or qmax > Q_LIMIT:
        raise ValueError(f"q_range ({qmin}, {qmax}) is outside +-2^24, the integers fp32 holds exactly")
    return qmin, qmax


def q_range_of(bits=None, signed=True, q_range=None) -> Optional[Tuple[int, int]]:
    """The integer range of a layer: ``bits`` = b gives [-2^(b-1), 2^(b-1) - 1] (signed) or [0, 2^b - 1] (unsigned), 1 <= b <= 24;
    ``q_range`` = (qmin, qmax) gives it directly; neither gives None (the unbounded quantizer).  Both together are an error."""
    if bits is not None and q_range is not None:
        raise ValueError("give bits or q_range, not both")
    if q_range is not None:
        if len(tuple(q_range)) != 2:
            raise ValueError(f"q_range must be (qmin, qmax), got {q_range!r}")
        return check_q_range(*q_range)
    if bits is None:
        return None
    if int(bits) != bits or not 1 <= int(bits) <= 24:
        raise ValueError(f"bits must be an integer in 1..24, got {bits!r}")
    b = int(bits)
    return (-(1 << (b - 1)), (1 << (b - 1)) - 1) if signed else (0, (1 << b) - 1)


ROUNDINGS = ("floor", "nearest")      # include/lq_hip.h: LQ_ROUND_FLOOR, LQ_ROUND_NEAREST_EVEN


def check_rounding(rounding, has_range: bool = True) -> int:
    """The C ABI's value of ``rounding``, or ValueError: one of ROUNDINGS, and "nearest" only for a quantizer with a range."""
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be one of {ROUNDINGS}, got {rounding!r}")
    if rounding == "nearest" and not has_range:
        raise ValueError("rounding='nearest' needs bits or q_range (the unbounded nearest quantizer is q_range=(-2**24, 2**24))")
    return ROUNDINGS.index(rounding)


def fq_forward_clip(parameter: torch.Tensor, scale: torch.Tensor, qmin: int, qmax: int, q_dtype: Optional[torch.dtype] = None,
                    *, rounding: str = "floor"):
    """Clipped forward (include/lq_hip.h, lq_fq_forward_clip_r): out = clamp(rnd(P/s), qmin, qmax) * s with rnd = floor, or rint
    (round half to even) for ``rounding="nearest"``.  Returns ``out``, or ``(out, q)`` with the clamped integers when ``q_dtype``
    is given."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    lib = _hip.load()
    p, s, (outer, G, inner) = _param(parameter, scale)
    out = torch.empty_like(p)
    q, qd = _q_buffer(p, q_dtype)
    _hip.check(lib.lq_fq_forward_clip_r(_hip.ptr(p), _hip.ptr(s), _hip.ptr(out), _hip.ptr(q), qd, qmin, qmax, rnd,
                                        outer, G, inner, _hip.stream_ptr(p.device)), "lq_fq_forward_clip_r")
    return out if q is None else (out, q)


def fq_backward_clip(parameter: torch.Tensor, scale: torch.Tensor, dy: torch.Tensor, qmin: int, qmax: int,
                     grad_scale: float = 1.0, want_ds: bool = True, want_clipped: bool = False, *, rounding: str = "floor"):
    """Clipped backward (include/lq_hip.h, lq_fq_backward_clip_r; ``rounding`` as fq_forward_clip).  Returns
    ``(dP, ds, clipped)``: dP = dy inside the range and +0 outside, with the parameter's strides; ds (shape of scale; None unless
    ``want_ds``) = grad_scale * sum dy * r; clipped (int32 tensor holding the uint32 counts per group, shape of scale; None
    unless ``want_clipped``)."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    lib = _hip.load()
    p, s, (outer, G, inner) = _param(parameter, scale)
    d = _hip.require_device_f32(dy, "dy", like=p)
    dP = torch.empty_like(p)
    ds = torch.empty_like(s) if want_ds else None
    clipped = torch.empty_like(s, dtype=torch.int32) if want_clipped else None
    ws = _hip.workspace_for(p.device, outer, G, inner)
    _hip.check(lib.lq_fq_backward_clip_r(_hip.ptr(p), _hip.ptr(s), _hip.ptr(d), qmin, qmax, rnd, float(grad_scale), _hip.ptr(dP),
                                         _hip.ptr(ds), _hip.ptr(clipped), _hip.ptr(ws), ws.numel(), outer, G, inner,
                                         _hip.stream_ptr(p.device)), "lq_fq_backward_clip_r")
    return dP, ds, clipped


def _group_param(parameter: torch.Tensor, scale: torch.Tensor, group_size: int):
    """(P, s, (R, C, axis)) as the group-wise kernels read them: the parameter in its own memory order (descriptor.group_geometry)."""
    p = _hip.require_device_f32(parameter, "parameter", dense_ok=True)
    s = _hip.require_device_f32(scale, "scale")
    return p, s, group_geometry(tuple(p.shape), p.stride(), tuple(s.shape), group_size)


def fq_forward_group(parameter: torch.Tensor, scale: torch.Tensor, qmin: int, qmax: int, group_size: int,
                     q_dtype: Optional[torch.dtype] = None, *, rounding: str = "floor"):
    """Clipped forward with group-wise scales (include/lq_hip.h, lq_fq_forward_group): ``scale`` is the matrix of
    descriptor.groupwise_scale_shape, one scale per ``group_size`` elements along one axis of the parameter's memory.  Returns
    ``out`` (the parameter's strides), or ``(out, q)`` with the clamped integers when ``q_dtype`` is given."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    lib = _hip.load()
    p, s, (R, C, axis) = _group_param(parameter, scale, group_size)
    out = torch.empty_like(p)
    q, qd = _q_buffer(p, q_dtype)
    _hip.check(lib.lq_fq_forward_group(_hip.ptr(p), _hip.ptr(s), _hip.ptr(out), _hip.ptr(q), qd, qmin, qmax, rnd,
                                       R, C, axis, int(group_size), _hip.stream_ptr(p.device)), "lq_fq_forward_group")
    return out if q is None else (out, q)


def fq_backward_group(parameter: torch.Tensor, scale: torch.Tensor, dy: torch.Tensor, qmin: int, qmax: int, group_size: int,
                      grad_scale: float = 1.0, want_ds: bool = True, want_clipped: bool = False, *, rounding: str = "floor"):
    """Clipped backward with group-wise scales (include/lq_hip.h, lq_fq_backward_group).  Returns ``(dP, ds, clipped)`` as
    ``fq_backward_clip`` does: dP with the parameter's strides, ds and clipped (int32 tensor holding the uint32 counts) in the
    shape of ``scale``, None where not wanted."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    lib = _hip.load()
    p, s, (R, C, axis) = _group_param(parameter, scale, group_size)
    d = _hip.require_device_f32(dy, "dy", like=p)
    dP = torch.empty_like(p)
    ds = torch.empty_like(s) if want_ds else None
    clipped = torch.empty_like(s, dtype=torch.int32) if want_clipped else None
    need = lib.lq_group_workspace_bytes(R, C, axis, int(group_size))
    ws = _hip.workspace(p.device, need) if need else None
    _hip.check(lib.lq_fq_backward_group(_hip.ptr(p), _hip.ptr(s), _hip.ptr(d), qmin, qmax, rnd, float(grad_scale), _hip.ptr(dP),
                                        _hip.ptr(ds), _hip.ptr(clipped), _hip.ptr(ws), ws.numel() if ws is not None else 0,
                                        R, C, axis, int(group_size), _hip.stream_ptr(p.device)), "lq_fq_backward_group")
    return dP, ds, clipped


SCALE_INITS = ("absmax", "lsq", "mse")      # include/lq_hip.h: LQ_INIT_ABSMAX, LQ_INIT_LSQ, LQ_INIT_MSE
SCALE_INIT = float(np.float32(float(np.finfo(np.float32).eps) * 100))      # the library's initial scale and minimum (layers.SCALE_INIT)


def check_scale_init(method) -> int:
    """The C ABI's value of a scale-initialisation ``method``, or ValueError: one of SCALE_INITS."""
    if method not in SCALE_INITS:
        raise ValueError(f"scale_init must be one of {SCALE_INITS}, got {method!r}")
    return SCALE_INITS.index(method)


LAYER_SCALE_INITS = SCALE_INITS + ("minmax",)      # what layers, models and drivers accept; "minmax" writes scale AND offset


def check_layer_scale_init(method) -> str:
    """``method`` if a layer can be initialised with it (LAYER_SCALE_INITS; "minmax" only where the layer is asymmetric: the
    layer checks that), or ValueError."""
    if method not in LAYER_SCALE_INITS:
        raise ValueError(f"scale_init must be one of {LAYER_SCALE_INITS}, got {method!r}")
    return method


def scale_init_group(parameter: torch.Tensor, scale: torch.Tensor, qmin: int, qmax: int, group_size: Optional[int], method: str,
                     rounding: str = "floor", min_value: float = SCALE_INIT) -> torch.Tensor:
    """Writes ``scale`` IN PLACE from ``parameter`` (include/lq_hip.h, lq_scale_init_group): per group "absmax" (the smallest
    scale, up to a 2^-22 margin, under which no element is clipped), "lsq" (2 mean|P| / sqrt(Qp)) or "mse" (the candidate
    below absmax with the smallest squared error of this quantizer; ``rounding`` matters here only), never below ``min_value``.
    ``scale`` is a group-wise matrix with its ``group_size`` (descriptor.group_geometry), or, with ``group_size=None``, any
    one-axis or scalar scale whose groups are lines of the parameter's memory (descriptor.init_geometry).  A group that holds a
    NaN or an Inf gets NaN.  One launch, no synchronisation.  Returns ``scale``."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    m = check_scale_init(method)
    if method == "lsq" and qmin == 0 and qmax == 0:
        raise ValueError('scale_init "lsq" divides by sqrt(Qp): the range [0, 0] has no bound to scale by')
    min_value = float(min_value)
    if not (min_value > 0.0 and math.isfinite(min_value)):
        raise ValueError(f"min_value must be a positive finite number, got {min_value!r}")
    p = _hip.require_device_f32(parameter, "parameter", dense_ok=True)
    s = _hip.require_device_f32(scale, "scale")
    if s is not scale:
        raise ValueError("scale must be contiguous: it is written in place")
    R, C, axis, gs = init_geometry(tuple(p.shape), p.stride(), tuple(s.shape), group_size)
    lib = _hip.load()
    _hip.check(lib.lq_scale_init_group(_hip.ptr(p), _hip.ptr(s), qmin, qmax, rnd, m, min_value, R, C, axis, gs,
                                       _hip.stream_ptr(p.device)), "lq_scale_init_group")
    return scale


def _offset_like(offset: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    b = _hip.require_device_f32(offset, "offset")
    if b.shape != s.shape:
        raise ValueError(f"offset shape {tuple(b.shape)} != scale shape {tuple(s.shape)}: one offset per group")
    return b


def fq_forward_group_affine(parameter: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: int, qmax: int,
                            group_size: int, q_dtype: Optional[torch.dtype] = None, *, rounding: str = "floor"):
    """Asymmetric group-wise forward (include/lq_hip.h, lq_fq_forward_group_affine): ``out = clamp(rnd((P - b) / s)) * s + b``
    with ``offset`` (b) a matrix of the scale's shape.  Returns ``out``, or ``(out, q)`` with the clamped integers."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    lib = _hip.load()
    p, s, (R, C, axis) = _group_param(parameter, scale, group_size)
    b = _offset_like(offset, s)
    out = torch.empty_like(p)
    q, qd = _q_buffer(p, q_dtype)
    _hip.check(lib.lq_fq_forward_group_affine(_hip.ptr(p), _hip.ptr(s), _hip.ptr(b), _hip.ptr(out), _hip.ptr(q), qd, qmin, qmax, rnd,
                                              R, C, axis, int(group_size), _hip.stream_ptr(p.device)), "lq_fq_forward_group_affine")
    return out if q is None else (out, q)


def fq_backward_group_affine(parameter: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, dy: torch.Tensor, qmin: int,
                             qmax: int, group_size: int, grad_scale: float = 1.0, offset_grad_scale: Optional[float] = None,
                             want_ds: bool = True, want_db: bool = True, want_clipped: bool = False, *, rounding: str = "floor"):
    """Asymmetric group-wise backward (include/lq_hip.h, lq_fq_backward_group_affine).  Returns ``(dP, ds, db, clipped)``: dP
    with the parameter's strides; ds, db (``offset_grad_scale`` times the sum of dy over the group's clipped elements; the
    factor defaults to ``grad_scale``, as LSQ+) and clipped (int32 tensor holding the uint32 counts) in the shape of ``scale``,
    None where not wanted."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    lib = _hip.load()
    p, s, (R, C, axis) = _group_param(parameter, scale, group_size)
    b = _offset_like(offset, s)
    d = _hip.require_device_f32(dy, "dy", like=p)
    dP = torch.empty_like(p)
    ds = torch.empty_like(s) if want_ds else None
    db = torch.empty_like(s) if want_db else None
    clipped = torch.empty_like(s, dtype=torch.int32) if want_clipped else None
    kb = float(grad_scale if offset_grad_scale is None else offset_grad_scale)
    need = lib.lq_group_workspace_bytes(R, C, axis, int(group_size))
    ws = _hip.workspace(p.device, need) if need else None
    _hip.check(lib.lq_fq_backward_group_affine(_hip.ptr(p), _hip.ptr(s), _hip.ptr(b), _hip.ptr(d), qmin, qmax, rnd, float(grad_scale),
                                               kb, _hip.ptr(dP), _hip.ptr(ds), _hip.ptr(db), _hip.ptr(clipped), _hip.ptr(ws),
                                               ws.numel() if ws is not None else 0, R, C, axis, int(group_size),
                                               _hip.stream_ptr(p.device)), "lq_fq_backward_group_affine")
    return dP, ds, db, clipped


def check_minmax_range(qmin: int, qmax: int) -> None:
    """"minmax" spreads a group's values over the range: it needs two codes at least and bounds within +-2^22."""
    if qmin >= qmax:
        raise ValueError(f'scale_init "minmax" needs a range of two codes at least: [{qmin}, {qmax}] has one, there is no width '
                         "to spread the group's values over")
    if qmin < -(1 << 22) or qmax > (1 << 22):
        raise ValueError(f'scale_init "minmax": range [{qmin}, {qmax}] is outside +-2^22')


def scale_init_group_minmax(parameter: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, qmin: int, qmax: int,
                            group_size: int, rounding: str = "floor", min_value: float = SCALE_INIT):
    """Writes ``scale`` and ``offset`` IN PLACE from ``parameter`` (include/lq_hip.h, lq_scale_init_group_minmax): per group the
    step that spreads [min, max] over the range and the offset that centres it, so that no element is clipped (the header states
    when).  A group that holds a NaN or an Inf gets NaN in both.  One launch, no synchronisation.  Returns ``(scale, offset)``."""
    qmin, qmax = check_q_range(qmin, qmax)
    check_minmax_range(qmin, qmax)
    rnd = check_rounding(rounding)
    min_value = float(min_value)
    if not (min_value > 0.0 and math.isfinite(min_value)):
        raise ValueError(f"min_value must be a positive finite number, got {min_value!r}")
    p, s, (R, C, axis) = _group_param(parameter, scale, group_size)
    b = _offset_like(offset, s)
    if s is not scale or b is not offset:
        raise ValueError("scale and offset must be contiguous: they are written in place")
    lib = _hip.load()
    _hip.check(lib.lq_scale_init_group_minmax(_hip.ptr(p), _hip.ptr(s), _hip.ptr(b), qmin, qmax, rnd, min_value, R, C, axis,
                                              int(group_size), _hip.stream_ptr(p.device)), "lq_scale_init_group_minmax")
    return scale, offset


# --------------------------------------------------------------------------- OCP microscaling element formats
class ElementFormat(NamedTuple):
    """One row of include/lq_hip.h's lq_elem_format table."""
    id: int
    bits: int
    E: int
    M: int
    emin: int
    emax: int
    max: float


ELEMENT_FORMATS = {
    "fp4_e2m1": ElementFormat(0, 4, 2, 1, 0, 2, 6.0),
    "fp6_e2m3": ElementFormat(1, 6, 2, 3, 0, 2, 7.5),
    "fp6_e3m2": ElementFormat(2, 6, 3, 2, -2, 4, 28.0),
    "fp8_e4m3": ElementFormat(3, 8, 4, 3, -6, 8, 448.0),       # OCP e4m3fn
    "fp8_e5m2": ElementFormat(4, 8, 5, 2, -14, 15, 57344.0),   # OCP e5m2
}
SCALE_FORMATS = ("e8m0", "fp32")       # include/lq_hip.h: LQ_SCALE_E8M0, LQ_SCALE_FP32
MX_SCALE_INITS = ("mx", "cover")       # include/lq_hip.h: LQ_MX_INIT_OCP, LQ_MX_INIT_COVER
MX_GROUP_SIZE = 32                     # the block of the OCP MX formats: the default group size of a layer with an element format


def check_element_format(element_format) -> ElementFormat:
    """The table row of ``element_format``, or ValueError: one of ELEMENT_FORMATS."""
    if not isinstance(element_format, str) or element_format not in ELEMENT_FORMATS:
        raise ValueError(f"element_format must be one of {tuple(ELEMENT_FORMATS)}, got {element_format!r}")
    return ELEMENT_FORMATS[element_format]


def check_scale_format(scale_format) -> int:
    """The C ABI's value of ``scale_format``, or ValueError: one of SCALE_FORMATS."""
    if scale_format not in SCALE_FORMATS:
        raise ValueError(f"scale_format must be one of {SCALE_FORMATS}, got {scale_format!r}")
    return SCALE_FORMATS.index(scale_format)


def check_mx_scale_init(method) -> int:
    """The C ABI's value of a microscaling scale-initialisation ``method``, or ValueError: one of MX_SCALE_INITS."""
    if method not in MX_SCALE_INITS:
        raise ValueError(f"scale_init of a layer with an element format must be one of {MX_SCALE_INITS}, got {method!r}")
    return MX_SCALE_INITS.index(method)


def mx_decode_table(element_format) -> np.ndarray:
    """float32 [2^bits]: the value of every code of ``element_format`` (include/lq_hip.h, "Code view"); the fp8 formats hold NaN
    (fp8_e4m3: S.1111.111) and +-Inf / NaN (fp8_e5m2: the top exponent) where OCP defines them."""
    f = check_element_format(element_format)
    codes = np.arange(1 << f.bits)
    mag = codes & ((1 << (f.bits - 1)) - 1)
    ef, mf = mag >> f.M, mag & ((1 << f.M) - 1)
    val = np.where(ef == 0, mf * 2.0 ** (f.emin - f.M), (1.0 + mf / 2.0 ** f.M) * np.exp2((ef - 1 + f.emin).astype(np.float64)))
    if element_format == "fp8_e4m3":
        val = np.where(mag == 127, np.nan, val)
    if element_format == "fp8_e5m2":
        val = np.where(ef == 31, np.where(mf == 0, np.inf, np.nan), val)
    return (np.where(codes >> (f.bits - 1), -1.0, 1.0) * val).astype(np.float32)


def mx_effective_scale(scale: np.ndarray, scale_format) -> np.ndarray:
    """Host restatement of s_eff (include/lq_hip.h): float32 in the shape of ``scale``; NaN marks an E8M0 scale that is not
    positive, normal and finite or that rounds past 2^127.  For the exports, which read the scales on the host anyway."""
    check_scale_format(scale_format)
    s = np.ascontiguousarray(scale, np.float32)
    if scale_format == "fp32":
        return s
    b = s.view(np.uint32).astype(np.uint64)
    nb = (b + 0x004AFB0D) & 0x7F800000
    ok = (b >= 0x00800000) & (b < 0x7F800000) & (nb < 0x7F800000)
    return np.where(ok, nb.astype(np.uint32).view(np.float32), np.float32(np.nan)).astype(np.float32)


def _mx_param(parameter: torch.Tensor, scale: torch.Tensor, group_size: Optional[int]):
    """(P, s, (R, C, axis, gs)): a group-wise scale matrix with its ``group_size``, or (``group_size=None``) a one-axis or scalar
    scale whose groups are lines of the parameter's memory -- a bias is one group (descriptor.init_geometry)."""
    p = _hip.require_device_f32(parameter, "parameter", dense_ok=True)
    s = _hip.require_device_f32(scale, "scale")
    return p, s, init_geometry(tuple(p.shape), p.stride(), tuple(s.shape), group_size)


def fq_forward_mx(parameter: torch.Tensor, scale: torch.Tensor, element_format: str, group_size: Optional[int] = MX_GROUP_SIZE,
                  scale_format: str = "e8m0", q_dtype: Optional[torch.dtype] = None):
    """Microscaling forward (include/lq_hip.h, lq_fq_forward_mx): every element rounded to the ``element_format`` minifloat grid
    (ties to even, saturating at the format's max) under its group's scale -- rounded to a power of two for
    ``scale_format="e8m0"``, as it is for "fp32".  Returns ``out`` (the parameter's strides), or ``(out, code)`` with the
    elements' encodings when ``q_dtype`` is given."""
    fmt = check_element_format(element_format)
    sf = check_scale_format(scale_format)
    lib = _hip.load()
    p, s, (R, C, axis, gs) = _mx_param(parameter, scale, group_size)
    out = torch.empty_like(p)
    q, qd = _q_buffer(p, q_dtype)
    _hip.check(lib.lq_fq_forward_mx(_hip.ptr(p), _hip.ptr(s), _hip.ptr(out), _hip.ptr(q), qd, fmt.id, sf, R, C, axis, gs,
                                    _hip.stream_ptr(p.device)), "lq_fq_forward_mx")
    return out if q is None else (out, q)


def fq_backward_mx(parameter: torch.Tensor, scale: torch.Tensor, dy: torch.Tensor, element_format: str,
                   group_size: Optional[int] = MX_GROUP_SIZE, scale_format: str = "e8m0", grad_scale: float = 1.0,
                   want_ds: bool = True, want_clipped: bool = False):
    """Microscaling backward (include/lq_hip.h, lq_fq_backward_mx).  Returns ``(dP, ds, clipped)`` as ``fq_backward_group`` does:
    dP = dy where the element is inside the format's range and +0 where it saturates; ds (shape of scale) the straight-through
    gradient of the stored scale; clipped the count of saturated elements per group (int32 tensor holding the uint32 counts)."""
    fmt = check_element_format(element_format)
    sf = check_scale_format(scale_format)
    lib = _hip.load()
    p, s, (R, C, axis, gs) = _mx_param(parameter, scale, group_size)
    d = _hip.require_device_f32(dy, "dy", like=p)
    dP = torch.empty_like(p)
    ds = torch.empty_like(s) if want_ds else None
    clipped = torch.empty_like(s, dtype=torch.int32) if want_clipped else None
    _hip.check(lib.lq_fq_backward_mx(_hip.ptr(p), _hip.ptr(s), _hip.ptr(d), fmt.id, sf, float(grad_scale), _hip.ptr(dP),
                                     _hip.ptr(ds), _hip.ptr(clipped), R, C, axis, gs, _hip.stream_ptr(p.device)),
               "lq_fq_backward_mx")
    return dP, ds, clipped


def scale_init_mx(parameter: torch.Tensor, scale: torch.Tensor, element_format: str, group_size: Optional[int] = MX_GROUP_SIZE,
                  method: str = "mx", min_value: float = SCALE_INIT) -> torch.Tensor:
    """Writes ``scale`` IN PLACE from ``parameter`` (include/lq_hip.h, lq_scale_init_mx): per group a power of two, "mx" the OCP
    rule 2^(floor(log2 absmax) - emax) (the largest elements may saturate), "cover" the smallest power of two under which none
    does; never below ``min_value``.  A group that holds a NaN or an Inf gets NaN.  One launch.  Returns ``scale``."""
    fmt = check_element_format(element_format)
    m = check_mx_scale_init(method)
    min_value = float(min_value)
    if not (min_value > 0.0 and math.isfinite(min_value)):
        raise ValueError(f"min_value must be a positive finite number, got {min_value!r}")
    p, s, (R, C, axis, gs) = _mx_param(parameter, scale, group_size)
    if s is not scale:
        raise ValueError("scale must be contiguous: it is written in place")
    lib = _hip.load()
    _hip.check(lib.lq_scale_init_mx(_hip.ptr(p), _hip.ptr(s), fmt.id, m, min_value, R, C, axis, gs, _hip.stream_ptr(p.device)),
               "lq_scale_init_mx")
    return scale


# --------------------------------------------------------------------------- packed MX operands and the block-scaled GEMM
MX_OPERAND_FORMATS = ("fp4_e2m1", "fp8_e4m3", "fp8_e5m2")      # what the fragments are built for (include/lq_hip.h)


class MxOperand(NamedTuple):
    """A matrix of ``lines`` by ``K`` in the order gfx950's block-scaled matrix instruction consumes it (include/lq_hip.h, "packed
    MX operands"): ``codes`` and ``scales`` are opaque uint8 buffers of lq_mx_operand_bytes' sizes."""
    codes: torch.Tensor
    scales: torch.Tensor
    format: str
    lines: int
    K: int


def check_mx_operand_format(element_format) -> ElementFormat:
    """The table row of an operand's ``element_format``, or ValueError: the fp6 formats are not built."""
    fmt = check_element_format(element_format)
    if element_format not in MX_OPERAND_FORMATS:
        raise ValueError(f"element_format={element_format!r}: fp6 operands are not supported (6-bit lanes need a fragment packing "
                         f"of their own); the block-scaled GEMM takes one of {MX_OPERAND_FORMATS}")
    return fmt


def check_mx_operand_layer(element_format, scale_format, group_size) -> ElementFormat:
    """What a quantizer must be to run on the block-scaled matrix instruction, or ValueError naming the reason."""
    if element_format is None:
        raise ValueError("the block-scaled GEMM needs a layer with an element_format (a microscaling layer)")
    fmt = check_mx_operand_format(element_format)
    if scale_format != "e8m0":
        raise ValueError(f'scale_format={scale_format!r}: the block-scaled matrix instruction takes E8M0 (power-of-two) scales only')
    if group_size != MX_GROUP_SIZE:
        raise ValueError(f"group_size={group_size!r}: the block of the block-scaled matrix instruction is {MX_GROUP_SIZE}")
    return fmt


def mx_operand_bytes(element_format: str, lines: int, K: int) -> Tuple[int, int]:
    """(code_bytes, scale_bytes) of an operand (include/lq_hip.h, lq_mx_operand_bytes).  Needs no device."""
    import ctypes
    fmt = check_mx_operand_format(element_format)
    cb, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _hip.check(_hip.load().lq_mx_operand_bytes(fmt.id, int(lines), int(K), ctypes.byref(cb), ctypes.byref(sb)), "lq_mx_operand_bytes")
    return int(cb.value), int(sb.value)


def _mx_operand_buffers(element_format: str, lines: int, K: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    cb, sb = mx_operand_bytes(element_format, lines, K)
    return torch.empty(cb, dtype=torch.uint8, device=device), torch.empty(sb, dtype=torch.uint8, device=device)


def mx_operand_pack(parameter: torch.Tensor, scale: torch.Tensor, element_format: str, group_size: int = MX_GROUP_SIZE,
                    scale_format: str = "e8m0") -> MxOperand:
    """The operand of a stored parameter under its stored group-wise scales (include/lq_hip.h, lq_mx_operand_pack): the codes are
    those of ``fq_forward_mx``'s code view, the scale bytes the exponents of its effective scales.  The lines are the parameter's
    columns when the blocks run along its strided axis (a Dense kernel (in, out)), its rows otherwise.  One launch."""
    fmt = check_mx_operand_layer(element_format, scale_format, group_size)
    lib = _hip.load()
    p, s, (R, C, axis) = _group_param(parameter, scale, group_size)
    lines, K = (C, R) if axis == 0 else (R, C)
    codes, scales = _mx_operand_buffers(element_format, lines, K, p.device)
    _hip.check(lib.lq_mx_operand_pack(_hip.ptr(p), _hip.ptr(s), fmt.id, check_scale_format(scale_format), R, C, axis, int(group_size),
                                      _hip.ptr(codes), _hip.ptr(scales), _hip.stream_ptr(p.device)), "lq_mx_operand_pack")
    return MxOperand(codes, scales, element_format, lines, K)


def mx_operand_quantize(x: torch.Tensor, element_format: str = "fp8_e4m3", method: str = "mx") -> MxOperand:
    """The operand of a row-major activation matrix ``x (M, K)`` under scales taken from ``x`` itself (include/lq_hip.h,
    lq_mx_operand_quantize): per block of 32 along K what ``scale_init_mx(method, min_value=2^-126)`` writes, then the codes of
    ``fq_forward_mx`` under it.  No learned state, no backward.  One launch, one read of ``x``."""
    fmt = check_mx_operand_format(element_format)
    m = check_mx_scale_init(method)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"x must be a matrix (M, K), got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    lib = _hip.load()
    xc = _hip.require_device_f32(x, "x")
    M, K = (int(d) for d in xc.shape)
    codes, scales = _mx_operand_buffers(element_format, M, K, xc.device)
    _hip.check(lib.lq_mx_operand_quantize(_hip.ptr(xc), fmt.id, m, M, K, _hip.ptr(codes), _hip.ptr(scales),
                                          _hip.stream_ptr(xc.device)), "lq_mx_operand_quantize")
    return MxOperand(codes, scales, element_format, M, K)


def mx_operand_decode(operand: MxOperand) -> torch.Tensor:
    """float32 ``(lines, K)``: value(code) * 2^(byte - 127) of every element (include/lq_hip.h, lq_mx_operand_decode)."""
    fmt = check_mx_operand_format(operand.format)
    lib = _hip.load()
    out = torch.empty((operand.lines, operand.K), dtype=torch.float32, device=operand.codes.device)
    _hip.check(lib.lq_mx_operand_decode(_hip.ptr(operand.codes), _hip.ptr(operand.scales), fmt.id, operand.lines, operand.K,
                                        _hip.ptr(out), _hip.stream_ptr(out.device)), "lq_mx_operand_decode")
    return out


def _gemm_output(a, b, bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, fp32_out: bool = True):
    """``(bias, out, ldy)`` of the product of two operands: the bias checked, ``out`` checked or made, its leading dimension.
    ``fp32_out=False`` (the operand-out epilogue writes no fp32 matrix) checks the bias alone."""
    M, N = a.lines, b.lines
    if bias is not None:
        bias = _hip.require_device_f32(bias, "bias")
        if tuple(bias.shape) != (N,):
            raise ValueError(f"bias must have shape ({N},), got {tuple(bias.shape)}")
    if not fp32_out:
        return bias, None, 0
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.codes.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, N) or (N > 1 and out.stride(1) != 1) or not out.is_cuda:
        raise ValueError(f"out must be a float32 device matrix ({M}, {N}) with unit column stride")
    return bias, out, out.stride(0) if M > 1 else max(N, out.stride(0))


def mx_gemm(a: MxOperand, b: MxOperand, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Y (a.lines, b.lines) = A B^T (+ bias)`` in fp32 on v_mfma_scale_f32_16x16x128_f8f6f4 (include/lq_hip.h, lq_mx_gemm).
    ``out``: a float32 matrix to write into; its row stride is the leading dimension."""
    fa, fb = check_mx_operand_format(a.format), check_mx_operand_format(b.format)
    if a.K != b.K:
        raise ValueError(f"the operands reduce over different K: {a.K} and {b.K}")
    lib = _hip.load()
    M, N = a.lines, b.lines
    dev = a.codes.device
    bias, out, ldy = _gemm_output(a, b, bias, out)
    _hip.check(lib.lq_mx_gemm(_hip.ptr(a.codes), _hip.ptr(a.scales), fa.id, _hip.ptr(b.codes), _hip.ptr(b.scales), fb.id,
                              _hip.ptr(bias), _hip.ptr(out), M, N, a.K, ldy, _hip.stream_ptr(dev)), "lq_mx_gemm")
    return out


# --------------------------------------------------------------------------- packed int8 operands and the int8 GEMM
I8_RANGE = (-128, 127)       # what an operand byte of v_mfma_i32_16x16x64_i8 holds
I8_BLOCK_UNIT = 64           # K of one instruction: a scale block is a whole number of them (include/lq_hip.h)
I8_MAX_PERIOD = 65536        # the longest run of k between two scale changes whose int32 sum cannot overflow


class I8Operand(NamedTuple):
    """A matrix of ``lines`` by ``K`` in the order gfx950's int8 matrix instruction consumes it (include/lq_hip.h, "packed int8
    operands"): ``codes`` (uint8) and ``scales`` (float32) are opaque buffers of lq_i8_operand_bytes' sizes; ``block`` is the
    number of consecutive k that share a scale, 0 for one scale per line."""
    codes: torch.Tensor
    scales: torch.Tensor
    lines: int
    K: int
    block: int


class I8AffineOperand(I8Operand):
    """An I8Operand of a parameter with an offset per group (``i8_operand_pack(..., offset=...)``): the same five fields, and
    ``offsets``, a float32 buffer in the layout of ``scales`` (include/lq_hip.h, "offsets on the B operand").  Only the B side of a
    product carries offsets."""
    offsets: Optional[torch.Tensor] = None


def _i8_offsets(operand: I8Operand) -> Optional[torch.Tensor]:
    """The offsets buffer of an operand, or None for a symmetric one."""
    return getattr(operand, "offsets", None) if isinstance(operand, I8AffineOperand) else None


def _check_i8_a_operand(a: I8Operand) -> None:
    if _i8_offsets(a) is not None:
        raise ValueError("only the B operand carries offsets: activation offsets are not built")


I8_OFFSETS_OPT_IN = ("pass offsets=True (i8_operand / call_i8 / i8_hardware; train.py --i8-eval-offsets) to add the offset's "
                     "row-sum term, which costs matrix instructions that a symmetric product does not pay")


def check_i8_block(block) -> int:
    """``block`` as an int, or ValueError: 0 (one scale per line) or a positive multiple of 64."""
    if isinstance(block, bool) or int(block) != block or int(block) < 0 or int(block) % I8_BLOCK_UNIT:
        raise ValueError(f"block={block!r}: a scale block is 0 (one scale per line) or a multiple of {I8_BLOCK_UNIT}, the K of one "
                         "int8 matrix instruction")
    return int(block)


def check_i8_operand_layer(q_range, orientation, group_size=None, asymmetric=False, element_format=None, fan_in=None, *,
                           offsets=False) -> Tuple[int, int]:
    """What a quantizer must be to run on the int8 matrix instruction -- (qmin, qmax) -- or ValueError naming the reason.
    ``offsets=True`` opts into the offset's row-sum term, with which an asymmetric layer passes."""
    if element_format is not None:
        raise ValueError(f"element_format={element_format!r}: a microscaling layer runs on the block-scaled matrix instruction "
                         "(mx_hardware), not on the int8 one")
    if q_range is None:
        raise ValueError("the int8 GEMM needs a layer with bits or q_range: the reference's unbounded quantizer has no range that "
                         "fits a byte")
    qmin, qmax = check_q_range(*q_range)
    if qmin < I8_RANGE[0] or qmax > I8_RANGE[1]:
        raise ValueError(f"q_range ({qmin}, {qmax}) is not inside [{I8_RANGE[0]}, {I8_RANGE[1]}], the signed bytes the int8 matrix "
                         "instruction multiplies (an unsigned 8-bit range does not fit)")
    if asymmetric and not offsets:
        raise ValueError("asymmetric=True: an offset per group needs the row sums of the activation codes in the product; "
                         + I8_OFFSETS_OPT_IN)
    if orientation == "rowwise":
        raise ValueError('orientation="rowwise": a scale per input row varies along K inside a step of the instruction')
    if orientation not in ("scalar", "columnwise", "groupwise"):
        raise ValueError(f"orientation={orientation!r}: the int8 GEMM takes scalar, columnwise or groupwise scales")
    if orientation == "groupwise" and (fan_in is None or group_size < fan_in) and group_size % I8_BLOCK_UNIT:
        raise ValueError(f"group_size={group_size!r}: a scale block of the int8 GEMM is the whole input or a multiple of "
                         f"{I8_BLOCK_UNIT}, the K of one instruction")
    return qmin, qmax


def check_i8_conv_operand_layer(q_range, orientation, group_size=None, asymmetric=False, element_format=None, fan_in=None,
                                kernel_storage="oihw", *, offsets=False) -> Tuple[int, int]:
    """What a conv layer's quantizer must be to run on the int8 matrix instruction -- (qmin, qmax) -- or ValueError naming the
    reason.  ``fan_in`` is ci kh kw, the K of the im2col operand.  A conv kernel is HWIO-shaped, so "rowwise", "columnwise" and
    "channelwise" put the scale on kh, kw and ci: it varies along K inside a step of the instruction -- the Dense check's
    acceptance of "columnwise" does not carry over.  Eligible: "scalar", and "groupwise" with a group size that is a multiple of 64
    or at least ``fan_in`` (one scale per output channel)."""
    # range, offset and element format first, as the Dense check words them; the orientation is judged here
    qmin, qmax = check_i8_operand_layer(q_range, "groupwise" if orientation == "groupwise" else "scalar", group_size, asymmetric,
                                        element_format, fan_in, offsets=offsets)
    if orientation in ("rowwise", "columnwise", "channelwise"):
        axis = {"rowwise": "kh", "columnwise": "kw", "channelwise": "ci"}[orientation]
        raise ValueError(f'orientation="{orientation}": on an HWIO-shaped conv kernel the scale lies on {axis} and varies along '
                         "K = (ci, kh, kw) inside a step of the instruction")
    if orientation not in ("scalar", "groupwise"):
        raise ValueError(f"orientation={orientation!r}: the int8 GEMM of a conv layer takes scalar or groupwise scales")
    if kernel_storage != "oihw":
        raise ValueError(f'kernel_storage="{kernel_storage}": the int8 GEMM reduces over the (ci, kh, kw) memory run of a kernel '
                         'stored "oihw"')
    return qmin, qmax


def i8_operand_bytes(lines: int, K: int, block: int = 0) -> Tuple[int, int]:
    """(code_bytes, scale_bytes) of an operand (include/lq_hip.h, lq_i8_operand_bytes).  Needs no device."""
    import ctypes
    cb, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _hip.check(_hip.load().lq_i8_operand_bytes(int(lines), int(K), check_i8_block(block), ctypes.byref(cb), ctypes.byref(sb)),
               "lq_i8_operand_bytes")
    return int(cb.value), int(sb.value)


def _i8_operand_buffers(lines: int, K: int, block: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    cb, sb = i8_operand_bytes(lines, K, block)
    return torch.empty(cb, dtype=torch.uint8, device=device), torch.empty(sb // 4, dtype=torch.float32, device=device)


def i8_operand_pack(parameter: torch.Tensor, scale: torch.Tensor, qmin: int, qmax: int, group_size: int,
                    rounding: str = "floor", offset: Optional[torch.Tensor] = None) -> I8Operand:
    """The operand of a stored parameter under its stored group-wise scales (include/lq_hip.h, lq_i8_operand_pack): the codes are
    the clamped integers of ``fq_forward_group``'s int8 view, the scales are ``scale`` bit for bit.  The lines are the parameter's
    columns when the groups run along its strided axis (a Dense kernel (in, out)), its rows otherwise.  ``group_size`` at least the
    line length gives one scale per line; otherwise it must be a multiple of 64.  One launch.
    ``offset`` (the scale's shape): the operand of an asymmetric parameter, an I8AffineOperand (lq_i8_operand_pack_affine) whose
    codes are ``fq_forward_group_affine``'s and whose ``offsets`` are ``offset`` bit for bit."""
    qmin, qmax = check_q_range(qmin, qmax)
    if qmin < I8_RANGE[0] or qmax > I8_RANGE[1]:
        raise ValueError(f"range ({qmin}, {qmax}) is not inside [{I8_RANGE[0]}, {I8_RANGE[1]}], the signed bytes the int8 matrix "
                         "instruction multiplies")
    rnd = check_rounding(rounding)
    p, s, (R, C, axis) = _group_param(parameter, scale, group_size)
    b = None if offset is None else _offset_like(offset, s)
    lines, K = (C, R) if axis == 0 else (R, C)
    gs = int(group_size)
    if gs < K and gs % I8_BLOCK_UNIT:
        raise ValueError(f"group_size={gs}: a scale block of the int8 GEMM is the whole line ({K}) or a multiple of {I8_BLOCK_UNIT}")
    block = 0 if gs >= K else gs
    lib = _hip.load()
    codes, scales = _i8_operand_buffers(lines, K, block, p.device)
    if b is not None:
        offsets = torch.empty_like(scales)
        _hip.check(lib.lq_i8_operand_pack_affine(_hip.ptr(p), _hip.ptr(s), _hip.ptr(b), qmin, qmax, rnd, R, C, axis, gs,
                                                 _hip.ptr(codes), _hip.ptr(scales), _hip.ptr(offsets), _hip.stream_ptr(p.device)),
                   "lq_i8_operand_pack_affine")
        op = I8AffineOperand(codes, scales, lines, K, block)
        op.offsets = offsets
        return op
    _hip.check(lib.lq_i8_operand_pack(_hip.ptr(p), _hip.ptr(s), qmin, qmax, rnd, R, C, axis, gs, _hip.ptr(codes), _hip.ptr(scales),
                                      _hip.stream_ptr(p.device)), "lq_i8_operand_pack")
    return I8Operand(codes, scales, lines, K, block)


def i8_operand_quantize(x: torch.Tensor, block: int = 0) -> I8Operand:
    """The operand of a row-major activation matrix ``x (M, K)`` under scales taken from ``x`` itself (include/lq_hip.h,
    lq_i8_operand_quantize): per row and scale block what ``scale_init_group("absmax", -127, 127, min_value=2^-126)`` writes, then
    the nearest-rounded clipped integers under it.  No learned state, no backward.  One launch."""
    block = check_i8_block(block)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"x must be a matrix (M, K), got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    lib = _hip.load()
    xc = _hip.require_device_f32(x, "x")
    M, K = (int(d) for d in xc.shape)
    codes, scales = _i8_operand_buffers(M, K, block, xc.device)
    _hip.check(lib.lq_i8_operand_quantize(_hip.ptr(xc), M, K, block, _hip.ptr(codes), _hip.ptr(scales), _hip.stream_ptr(xc.device)),
               "lq_i8_operand_quantize")
    return I8Operand(codes, scales, M, K, block)


def i8_operand_decode(operand: I8Operand) -> torch.Tensor:
    """float32 ``(lines, K)``: code * scale of every element (include/lq_hip.h, lq_i8_operand_decode); of an I8AffineOperand
    ``code * scale + offset``, two roundings (lq_i8_operand_decode_affine)."""
    lib = _hip.load()
    out = torch.empty((operand.lines, operand.K), dtype=torch.float32, device=operand.codes.device)
    offsets = _i8_offsets(operand)
    if offsets is not None:
        _hip.check(lib.lq_i8_operand_decode_affine(_hip.ptr(operand.codes), _hip.ptr(operand.scales), _hip.ptr(offsets),
                                                   operand.lines, operand.K, check_i8_block(operand.block), _hip.ptr(out),
                                                   _hip.stream_ptr(out.device)), "lq_i8_operand_decode_affine")
        return out
    _hip.check(lib.lq_i8_operand_decode(_hip.ptr(operand.codes), _hip.ptr(operand.scales), operand.lines, operand.K,
                                        check_i8_block(operand.block), _hip.ptr(out), _hip.stream_ptr(out.device)),
               "lq_i8_operand_decode")
    return out


def i8_period(a_block: int, b_block: int, K: int) -> int:
    """The length of a period of the int8 GEMM -- a maximal run of k on which neither operand's scale changes (the last may be
    shorter) -- or ValueError: two non-zero blocks of which neither divides the other, or a period above 65536."""
    a_block, b_block = check_i8_block(a_block), check_i8_block(b_block)
    lo, hi = min(a_block, b_block), max(a_block, b_block)
    if lo > 0 and hi % lo:
        raise ValueError(f"scale blocks {a_block} and {b_block}: the larger must be a multiple of the smaller")
    F = lo if lo > 0 else hi
    period = min(F, K) if F > 0 else K
    if period > I8_MAX_PERIOD:
        raise ValueError(f"a period of {period} k between two scale changes is above {I8_MAX_PERIOD}: its int32 sum could overflow")
    return period


def i8_gemm(a: I8Operand, b: I8Operand, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``Y (a.lines, b.lines) = A B^T (+ bias)`` on v_mfma_i32_16x16x64_i8 (include/lq_hip.h, lq_i8_gemm): exact int32 sums per
    period, scaled into fp32 by the product of the two operands' scales, bit for bit the definition stated there.
    ``out``: a float32 matrix to write into; its row stride is the leading dimension."""
    if a.K != b.K:
        raise ValueError(f"the operands reduce over different K: {a.K} and {b.K}")
    _check_i8_a_operand(a)
    i8_period(a.block, b.block, a.K)
    lib = _hip.load()
    M, N = a.lines, b.lines
    dev = a.codes.device
    bias, out, ldy = _gemm_output(a, b, bias, out)
    offsets = _i8_offsets(b)
    if offsets is not None:      # B = q s + b: the offset's row-sum term (lq_i8_gemm_affine)
        _hip.check(lib.lq_i8_gemm_affine(_hip.ptr(a.codes), _hip.ptr(a.scales), a.block, _hip.ptr(b.codes), _hip.ptr(b.scales),
                                         _hip.ptr(offsets), b.block, _hip.ptr(bias), _hip.ptr(out), ldy, M, N, a.K,
                                         _hip.stream_ptr(dev)), "lq_i8_gemm_affine")
        return out
    _hip.check(lib.lq_i8_gemm(_hip.ptr(a.codes), _hip.ptr(a.scales), a.block, _hip.ptr(b.codes), _hip.ptr(b.scales), b.block,
                              _hip.ptr(bias), _hip.ptr(out), ldy, M, N, a.K, _hip.stream_ptr(dev)), "lq_i8_gemm")
    return out


MX_ACTIVATIONS = (None, "relu")        # include/lq_hip.h: LQ_ACT_NONE, LQ_ACT_RELU


def check_mx_activation(activation) -> int:
    """The C ABI's value of an ``activation`` fused into the operand-out epilogue, or ValueError: one of MX_ACTIVATIONS."""
    if activation is not None and not isinstance(activation, str) or activation not in MX_ACTIVATIONS:
        raise ValueError(f"activation must be one of {MX_ACTIVATIONS}, got {activation!r}: the operand-out epilogue fuses relu only")
    return MX_ACTIVATIONS.index(activation)


def mx_gemm_quantize(a: MxOperand, b: MxOperand, bias: Optional[torch.Tensor] = None, activation=None, out_format: str = "fp8_e4m3",
                     method: str = "mx") -> MxOperand:
    """The operand of ``activation(A B^T (+ bias))`` for the next product, ``a.lines`` lines over ``K = b.lines``, written by the
    GEMM's own epilogue (include/lq_hip.h, lq_mx_gemm_quantize): byte for byte
    ``mx_operand_quantize(act(mx_gemm(a, b, bias)), out_format, method)``, in one launch and without the fp32 matrix."""
    fa, fb, fo = check_mx_operand_format(a.format), check_mx_operand_format(b.format), check_mx_operand_format(out_format)
    m = check_mx_scale_init(method)
    act = check_mx_activation(activation)
    if a.K != b.K:
        raise ValueError(f"the operands reduce over different K: {a.K} and {b.K}")
    lib = _hip.load()
    M, N = a.lines, b.lines
    dev = a.codes.device
    bias = _gemm_output(a, b, bias, fp32_out=False)[0]
    codes, scales = _mx_operand_buffers(out_format, M, N, dev)
    _hip.check(lib.lq_mx_gemm_quantize(_hip.ptr(a.codes), _hip.ptr(a.scales), fa.id, _hip.ptr(b.codes), _hip.ptr(b.scales), fb.id,
                                       _hip.ptr(bias), act, fo.id, m, _hip.ptr(codes), _hip.ptr(scales), M, N, a.K,
                                       _hip.stream_ptr(dev)), "lq_mx_gemm_quantize")
    return MxOperand(codes, scales, out_format, M, N)


I8_ACTIVATIONS = MX_ACTIVATIONS        # the two epilogues fuse the same activations, under the same C values
I8_OUT_BLOCK = 64                      # the scale block the int8 epilogue writes: one thread block's 64 columns
check_activation = check_mx_activation


def check_i8_out_block(out_block) -> int:
    """``out_block`` of the int8 operand-out epilogue as an int, or ValueError: it writes scale blocks of 64 only."""
    if isinstance(out_block, bool) or not isinstance(out_block, int) or out_block != I8_OUT_BLOCK:
        raise ValueError(f"out_block={out_block!r}: the int8 operand-out epilogue writes scale blocks of {I8_OUT_BLOCK}, the columns "
                         "of one thread block; one scale per row (0) or a larger block needs every column tile of a row before its "
                         "first code")
    return out_block


def i8_gemm_quantize(a: I8Operand, b: I8Operand, bias: Optional[torch.Tensor] = None, activation=None,
                     out_block: int = I8_OUT_BLOCK) -> I8Operand:
    """The int8 operand of ``activation(A B^T (+ bias))`` for the next product, ``a.lines`` lines over ``K = b.lines`` with scale
    blocks of ``out_block`` (64), written by the GEMM's own epilogue (include/lq_hip.h, lq_i8_gemm_quantize): byte for byte
    ``i8_operand_quantize(act(i8_gemm(a, b, bias)), out_block)``, in one launch and without the fp32 matrix."""
    out_block = check_i8_out_block(out_block)
    act = check_activation(activation)
    if a.K != b.K:
        raise ValueError(f"the operands reduce over different K: {a.K} and {b.K}")
    _check_i8_a_operand(a)
    i8_period(a.block, b.block, a.K)
    lib = _hip.load()
    M, N = a.lines, b.lines
    dev = a.codes.device
    bias = _gemm_output(a, b, bias, fp32_out=False)[0]
    codes, scales = _i8_operand_buffers(M, N, out_block, dev)
    offsets = _i8_offsets(b)
    if offsets is not None:
        _hip.check(lib.lq_i8_gemm_quantize_affine(_hip.ptr(a.codes), _hip.ptr(a.scales), a.block, _hip.ptr(b.codes),
                                                  _hip.ptr(b.scales), _hip.ptr(offsets), b.block, _hip.ptr(bias), act, out_block,
                                                  _hip.ptr(codes), _hip.ptr(scales), M, N, a.K, _hip.stream_ptr(dev)),
                   "lq_i8_gemm_quantize_affine")
        return I8Operand(codes, scales, M, N, out_block)
    _hip.check(lib.lq_i8_gemm_quantize(_hip.ptr(a.codes), _hip.ptr(a.scales), a.block, _hip.ptr(b.codes), _hip.ptr(b.scales), b.block,
                                       _hip.ptr(bias), act, out_block, _hip.ptr(codes), _hip.ptr(scales), M, N, a.K,
                                       _hip.stream_ptr(dev)), "lq_i8_gemm_quantize")
    return I8Operand(codes, scales, M, N, out_block)


class MxConvOperand(MxOperand):
    """The MxOperand of an im2col matrix (``mx_operand_im2col``): the same five fields, and ``out_hw = (OH, OW)`` of the convolution
    whose ``lines = B * OH * OW`` it holds."""
    out_hw: Tuple[int, int] = (0, 0)


def _conv_geom(shape, stride, kernel_size, strides, padding) -> "_hip.ConvGeom":
    def ints(v, n, what):
        v = (v,) * n if isinstance(v, int) else tuple(v)
        if len(v) != n or not all(isinstance(e, int) and not isinstance(e, bool) for e in v):
            raise ValueError(f"{what} must be {n} integers, got {v!r}")
        return v
    shape = tuple(int(d) for d in shape)
    if len(shape) != 4:
        raise ValueError(f"the input must have four axes (B, C, H, W), got shape {shape}")
    (kh, kw), (sh, sw) = ints(kernel_size, 2, "kernel_size"), ints(strides, 2, "strides")
    top, bottom, left, right = ints(padding, 4, "padding (top, bottom, left, right)")
    for what, v in (("kernel_size", (kh, kw)), ("strides", (sh, sw)), ("padding", (top, bottom, left, right))):
        if any(abs(e) >= 1 << 31 for e in v):
            raise ValueError(f"{what} {v!r} does not fit 32 bits")
    return _hip.ConvGeom(*shape, *(int(e) for e in stride), kh, kw, sh, sw, top, left, bottom, right)


def mx_im2col_dims(input_shape, kernel_size, strides=(1, 1), padding=(0, 0, 0, 0)) -> Tuple[int, int, int, int]:
    """``(M, K, OH, OW)`` of the im2col matrix of an input ``(B, C, H, W)`` (include/lq_hip.h, lq_mx_im2col_dims): ``OH = (H + top +
    bottom - KH) // stride_h + 1``, ``M = B OH OW`` lines over ``K = C KH KW``.  ``padding`` is (top, bottom, left, right).  Needs no
    device, and answers for an ``M * K`` that the operand itself refuses."""
    return _geom_dims(_hip.load(), _conv_geom(input_shape, (0, 0, 0, 0), kernel_size, strides, padding))


def _geom_dims(lib, g: "_hip.ConvGeom") -> Tuple[int, int, int, int]:
    from ctypes import byref, c_int64
    M, K, OH, OW = c_int64(0), c_int64(0), c_int64(0), c_int64(0)
    _hip.check(lib.lq_mx_im2col_dims(byref(g), byref(M), byref(K), byref(OH), byref(OW)), "lq_mx_im2col_dims")
    return M.value, K.value, OH.value, OW.value


def _require_conv_input(x) -> None:
    """``x`` as both im2col operands read it -- float32, four axes, any strides, on the current device -- or an exception."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"x must have four axes (B, C, H, W), got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if not x.is_cuda:
        raise RuntimeError(f"x is on {x.device}: the learned-quantization ops run only on a HIP device (MI355X); there is no CPU fallback")
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32, got {x.dtype}")
    if x.device.index is not None and x.device.index != torch.cuda.current_device():
        raise RuntimeError(f"x lives on {x.device} but the current device is cuda:{torch.cuda.current_device()}: call "
                           "torch.cuda.set_device(...) before using the ops")


def im2col_runs(B: int, lines_per_image: int, K: int, max_lines: Optional[int] = None):
    """``[(b0, b1), ...]``: the batch ``range(B)`` cut, in order, into runs of whole images whose im2col operand the C surface takes
    (``lines * K < 2^31``), whose product the grid of either GEMM takes (65535 * 64 lines) and that hold at most ``max_lines``
    lines.  A run is never shorter than one image: a single image beyond a limit is left to the C surface to refuse."""
    fit = min(((1 << 31) - 1) // K, 65535 * 64)
    if max_lines is not None:
        fit = min(fit, int(max_lines))
    images = max(1, min(B, fit // lines_per_image))
    return [(b0, min(B, b0 + images)) for b0 in range(0, B, images)]


def mx_operand_im2col(x: torch.Tensor, kernel_size, strides=(1, 1), padding=(0, 0, 0, 0), element_format: str = "fp8_e4m3",
                      method: str = "mx") -> MxOperand:
    """The operand of the im2col matrix of ``x (B, C, H, W)`` -- line ``(b OH + oh) OW + ow``, reduction index ``(c KH + i) KW + j``,
    zero ``padding`` (top, bottom, left, right) -- under scales taken from it (include/lq_hip.h, lq_mx_operand_im2col): byte for
    byte ``mx_operand_quantize`` of that matrix, which is never built.  ``x`` is read through its own strides (NCHW-contiguous,
    channels_last or any view): no copy.  One launch.  The result is an MxOperand whose ``out_hw`` is ``(OH, OW)``."""
    import ctypes
    fmt = check_mx_operand_format(element_format)
    m = check_mx_scale_init(method)
    _require_conv_input(x)
    lib = _hip.load()
    g = _conv_geom(x.shape, x.stride(), kernel_size, strides, padding)
    M, K, OH, OW = _geom_dims(lib, g)
    codes, scales = _mx_operand_buffers(element_format, M, K, x.device)
    _hip.check(lib.lq_mx_operand_im2col(_hip.ptr(x), ctypes.byref(g), fmt.id, m, _hip.ptr(codes), _hip.ptr(scales),
                                        _hip.stream_ptr(x.device)), "lq_mx_operand_im2col")
    op = MxConvOperand(codes, scales, element_format, M, K)
    op.out_hw = (OH, OW)
    return op


class I8ConvOperand(I8Operand):
    """The I8Operand of an im2col matrix (``i8_operand_im2col``): the same five fields, and ``out_hw = (OH, OW)`` of the convolution
    whose ``lines = B * OH * OW`` it holds."""
    out_hw: Tuple[int, int] = (0, 0)


def i8_operand_im2col(x: torch.Tensor, kernel_size, strides=(1, 1), padding=(0, 0, 0, 0), block: int = 0) -> I8Operand:
    """The int8 operand of the im2col matrix of ``x (B, C, H, W)`` -- line ``(b OH + oh) OW + ow``, reduction index
    ``(c KH + i) KW + j``, zero ``padding`` (top, bottom, left, right) -- under absmax scales taken from it per line and ``block``
    consecutive k (0: per line) (include/lq_hip.h, lq_i8_operand_im2col): byte for byte ``i8_operand_quantize`` of that matrix,
    which is never built.  ``x`` is read through its own strides (NCHW-contiguous, channels_last or any view): no copy.  One launch.
    The result is an I8Operand whose ``out_hw`` is ``(OH, OW)``."""
    import ctypes
    block = check_i8_block(block)
    _require_conv_input(x)
    lib = _hip.load()
    g = _conv_geom(x.shape, x.stride(), kernel_size, strides, padding)
    M, K, OH, OW = _geom_dims(lib, g)
    codes, scales = _i8_operand_buffers(M, K, block, x.device)
    _hip.check(lib.lq_i8_operand_im2col(_hip.ptr(x), ctypes.byref(g), block, _hip.ptr(codes), _hip.ptr(scales),
                                        _hip.stream_ptr(x.device)), "lq_i8_operand_im2col")
    op = I8ConvOperand(codes, scales, M, K, block)
    op.out_hw = (OH, OW)
    return op


STATS_MAX_BINS = 4096   # include/lq_hip.h, lq_group_stats: the widest range whose codes it bins


class GroupStats(NamedTuple):
    """What ``group_stats`` returns, all on the device: ``below`` / ``above`` (int32 tensors holding the uint32 counts) and
    ``err2`` / ``sig2`` (float64) in the scale's shape, ``hist`` (int32, qmax - qmin + 1 bins) or None."""
    below: torch.Tensor
    above: torch.Tensor
    err2: torch.Tensor
    sig2: torch.Tensor
    hist: Optional[torch.Tensor]


class MxStats(NamedTuple):
    """What ``mx_stats`` returns, all on the device: ``below`` / ``above`` / ``flushed`` (int32 tensors holding the uint32 counts)
    and ``err2`` / ``sig2`` (float64) in the scale's shape, ``hist`` (int32, 2^bits bins in code order) or None."""
    below: torch.Tensor
    above: torch.Tensor
    flushed: torch.Tensor
    err2: torch.Tensor
    sig2: torch.Tensor
    hist: Optional[torch.Tensor]


def _stats_outputs(s: torch.Tensor, counts: int, nbins: Optional[int]) -> list:
    """The outputs of a statistics call in its argument order: ``counts`` int32 and two float64 tensors in the scale's shape, and
    the zeroed histogram of ``nbins`` bins (None: no histogram)."""
    out = [torch.empty_like(s, dtype=torch.int32) for _ in range(counts)] + [torch.empty_like(s, dtype=torch.float64) for _ in range(2)]
    return out + [None if nbins is None else torch.zeros(nbins, dtype=torch.int32, device=s.device)]


def group_stats(parameter: torch.Tensor, scale: torch.Tensor, qmin: int, qmax: int, group_size: Optional[int], *,
                offset: Optional[torch.Tensor] = None, rounding: str = "floor", want_hist: bool = True) -> GroupStats:
    """Statistics of the clipped quantizer on ``parameter`` under ``scale`` (and ``offset``) as they are now (include/lq_hip.h,
    lq_group_stats): per group the elements clipped below and above the range and the f64 sums of squared error and squared
    signal, per tensor the histogram of the codes.  ``scale`` is a group-wise matrix with its ``group_size``, or, with
    ``group_size=None``, any scale descriptor.init_geometry accepts (as ``scale_init_group``).  Ranges of more than
    STATS_MAX_BINS codes have no histogram: pass ``want_hist=False``.  One launch, read only, no synchronisation."""
    qmin, qmax = check_q_range(qmin, qmax)
    rnd = check_rounding(rounding)
    if want_hist and qmax - qmin + 1 > STATS_MAX_BINS:
        raise ValueError(f"the range [{qmin}, {qmax}] has {qmax - qmin + 1} codes, the histogram at most {STATS_MAX_BINS}: "
                         "pass want_hist=False")
    p = _hip.require_device_f32(parameter, "parameter", dense_ok=True)
    s = _hip.require_device_f32(scale, "scale")
    b = None if offset is None else _offset_like(offset, s)
    R, C, axis, gs = init_geometry(tuple(p.shape), p.stride(), tuple(s.shape), group_size)
    out = _stats_outputs(s, 2, qmax - qmin + 1 if want_hist else None)
    _hip.check(_hip.load().lq_group_stats(_hip.ptr(p), _hip.ptr(s), _hip.ptr(b), qmin, qmax, rnd, *map(_hip.ptr, out), R, C, axis, gs,
                                          _hip.stream_ptr(p.device)), "lq_group_stats")
    return GroupStats(*out)


def mx_stats(parameter: torch.Tensor, scale: torch.Tensor, element_format: str, group_size: Optional[int] = MX_GROUP_SIZE,
             scale_format: str = "e8m0", *, want_hist: bool = True) -> MxStats:
    """Statistics of the microscaling quantizer on ``parameter`` under ``scale`` as it is now (include/lq_hip.h, lq_mx_stats): per
    group the elements that saturate below -max and above +max, the non-zero elements the grid flushes to zero, and the f64 sums
    of squared error and squared signal; per tensor the histogram of the elements' encodings (the forward's code view).  Geometry
    as ``fq_forward_mx``.  One launch, read only, no synchronisation."""
    fmt = check_element_format(element_format)
    sf = check_scale_format(scale_format)
    lib = _hip.load()
    p, s, (R, C, axis, gs) = _mx_param(parameter, scale, group_size)
    out = _stats_outputs(s, 3, 1 << fmt.bits if want_hist else None)
    _hip.check(lib.lq_mx_stats(_hip.ptr(p), _hip.ptr(s), fmt.id, sf, *map(_hip.ptr, out), R, C, axis, gs, _hip.stream_ptr(p.device)),
               "lq_mx_stats")
    return MxStats(*out)


def _sqnr_db(sig2: float, err2: float) -> float:
    """10 log10(sig2 / err2) in float64: inf for zero error, -inf for zero signal under an error, NaN where either sum is NaN
    or both are infinite."""
    if math.isnan(sig2) or math.isnan(err2) or (math.isinf(sig2) and math.isinf(err2)):
        return math.nan
    if err2 == 0.0 or math.isinf(sig2):
        return math.inf
    if sig2 == 0.0 or math.isinf(err2):
        return -math.inf
    ratio = sig2 / err2
    if 0.0 < ratio < math.inf:
        return 10.0 * math.log10(ratio)
    return 10.0 * (math.log10(sig2) - math.log10(err2))      # the quotient itself left the float64 range


def _stats_to_host(records):
    """The records' tensors in ONE device->host copy, as records (of their own type) of NumPy arrays: float64 sums, int64 counts
    and bins (the uint32 values behind the int32 tensors, which float64 carries exactly)."""
    def f64(t):
        t = t.reshape(-1)
        if t.dtype == torch.int32:
            return (t.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)
        return t.to(torch.float64)

    parts = [f64(t) for rec in records for t in rec if t is not None]
    if not parts:
        return []
    flat = torch.cat(parts).cpu().numpy()
    host, at = [], 0
    for rec in records:
        fields = []
        for t in rec:
            if t is None:
                fields.append(None)
                continue
            a = flat[at:at + t.numel()].reshape(tuple(t.shape))
            at += t.numel()
            fields.append(a if t.dtype.is_floating_point else a.astype(np.int64))
        host.append(type(rec)(*fields))
    return host


def _host_record(record, numel):
    """(``record`` with NumPy fields, after ONE device->host copy where a field is a tensor; ``numel`` as a positive int)"""
    numel = int(numel)
    if numel < 1:
        raise ValueError(f"numel must be positive, got {numel}")
    if any(isinstance(t, torch.Tensor) for t in record):
        record = _stats_to_host([type(record)(*(t if t is None or isinstance(t, torch.Tensor) else torch.as_tensor(t) for t in record))])[0]
    return record, numel


def _summarize_sums(rec) -> dict:
    """What both summaries compute alike: ``sqnr_db``, ``worst_group_sqnr_db``, and from the histogram (None without one) ``used``
    (bins that occur) and ``entropy_bits``."""
    err2 = np.asarray(rec.err2, dtype=np.float64).reshape(-1)
    sig2 = np.asarray(rec.sig2, dtype=np.float64).reshape(-1)
    out = {"sqnr_db": _sqnr_db(float(sig2.sum()), float(err2.sum())),
           "worst_group_sqnr_db": min((_sqnr_db(float(a), float(e)) for a, e in zip(sig2, err2)),
                                      key=lambda v: -math.inf if math.isnan(v) else v),
           "used": None, "entropy_bits": None}
    if rec.hist is not None:
        h = np.asarray(rec.hist, dtype=np.float64).reshape(-1)
        used, total = h[h > 0], float(h.sum())
        out["used"] = int(used.size)
        pr = used / total if total > 0 else used
        out["entropy_bits"] = float(max(0.0, -(pr * np.log2(pr)).sum())) if used.size else 0.0
    return out


def _share(counts, numel: int) -> float:
    return float(np.asarray(counts, dtype=np.float64).sum() / float(numel))


def _summarize_host(rec: GroupStats, numel: int) -> dict:
    c = _summarize_sums(rec)
    return {"clip_low": _share(rec.below, numel), "clip_high": _share(rec.above, numel), "sqnr_db": c["sqnr_db"],
            "worst_group_sqnr_db": c["worst_group_sqnr_db"], "used_levels": c["used"], "entropy_bits": c["entropy_bits"]}


def _summarize_mx_host(rec: MxStats, numel: int, element_format: str) -> dict:
    fmt = check_element_format(element_format)
    if rec.hist is not None and np.size(rec.hist) != 1 << fmt.bits:
        raise ValueError(f"a histogram of {np.size(rec.hist)} bins is not {element_format}'s ({1 << fmt.bits} codes)")
    c = _summarize_sums(rec)
    out = {"sat_low": _share(rec.below, numel), "sat_high": _share(rec.above, numel), "flushed": _share(rec.flushed, numel),
           "sqnr_db": c["sqnr_db"], "worst_group_sqnr_db": c["worst_group_sqnr_db"], "used_codes": c["used"],
           "entropy_bits": c["entropy_bits"], "zero": None, "subnormal": None}
    if rec.hist is not None:
        h = np.asarray(rec.hist, dtype=np.float64).reshape(-1)
        total = float(h.sum())
        mag = np.arange(h.size) & ((1 << (fmt.bits - 1)) - 1)      # the code below its sign bit: exponent field, then M mantissa bits
        out["zero"] = float(h[mag == 0].sum() / total) if total > 0 else 0.0
        out["subnormal"] = float(h[(mag >> fmt.M == 0) & (mag != 0)].sum() / total) if total > 0 else 0.0
    return out


def summarize_stats(record: GroupStats, numel: int) -> dict:
    """Host floats of one ``group_stats`` record of a tensor of ``numel`` elements, computed in float64 on the host after ONE
    device->host copy: ``clip_low`` / ``clip_high`` (shares of the elements clipped below / above), ``sqnr_db`` = 10 log10(sum
    sig2 / sum err2) (inf for zero error), ``worst_group_sqnr_db`` (the smallest group's; NaN if a group's is NaN),
    ``used_levels`` (codes that occur) and ``entropy_bits`` (Shannon entropy of the code distribution; both None without a
    histogram).  The record's fields may be device tensors, host tensors or NumPy arrays."""
    return _summarize_host(*_host_record(record, numel))


def summarize_stats_many(records, numels) -> list:
    """``summarize_stats`` of several records with all of them copied to the host together (one device->host copy)."""
    return [_summarize_host(rec, int(n)) for rec, n in zip(_stats_to_host(list(records)), numels)]


def summarize_mx_stats(record: MxStats, numel: int, *, element_format: str) -> dict:
    """Host floats of one ``mx_stats`` record of a tensor of ``numel`` elements, computed in float64 on the host after ONE
    device->host copy: ``sat_low`` / ``sat_high`` / ``flushed`` (shares of the elements saturated below / above and flushed to
    zero), ``sqnr_db`` and ``worst_group_sqnr_db`` (``summarize_stats``' conventions), and from the histogram (None without one)
    ``used_codes``, ``entropy_bits``, ``zero`` (share of the codes +0 and -0) and ``subnormal`` (share of the codes with exponent
    field 0 and a non-zero mantissa).  ``element_format`` names the fields of a code.  The record's fields may be device tensors,
    host tensors or NumPy arrays."""
    return _summarize_mx_host(*_host_record(record, numel), element_format)


def summarize_mx_stats_many(records, numels, element_formats) -> list:
    """``summarize_mx_stats`` of several records with all of them copied to the host together (one device->host copy)."""
    return [_summarize_mx_host(rec, int(n), f) for rec, n, f in zip(_stats_to_host(list(records)), numels, element_formats)]


def fq_fwd_bwd_fused(parameter: torch.Tensor, scale: torch.Tensor, dy: torch.Tensor, penalty_threshold: float,
                     out: Optional[torch.Tensor] = None, ds: Optional[torch.Tensor] = None):
    """K4: forward and NQ backward in one pass over P (benchmark path).  Returns (out, ds)."""
    lib = _hip.load()
    p, s, (outer, G, inner) = _param(parameter, scale)
    d = _hip.require_device_f32(dy, "dy", like=p)
    if out is None:
        out = torch.empty_like(p)
    elif not _hip.same_layout(out, p):
        raise ValueError("out must have the parameter's shape and strides")
    if ds is None:
        ds = torch.empty_like(s)
    ws = _hip.workspace_for(p.device, outer, G, inner)
    _hip.check(lib.lq_fq_fwd_bwd_fused(_hip.ptr(p), _hip.ptr(s), _hip.ptr(d), float(penalty_threshold),
                                       _hip.ptr(out), _hip.ptr(ds), _hip.ptr(ws), ws.numel(),
                                       outer, G, inner, _hip.stream_ptr(p.device)), "lq_fq_fwd_bwd_fused")
    return out, ds


def q_absmax_over_axis(parameter: torch.Tensor, scale: torch.Tensor, axis: int) -> torch.Tensor:
    """max |floor(P/s)| reduced over ``axis`` (custom_callbacks.py:98-99 uses axis=1)."""
    lib = _hip.load()
    p = _hip.require_device_f32(parameter, "parameter")
    s = _hip.require_device_f32(scale, "scale")
    outer, G, inner = _desc(p, s)
    shape = tuple(p.shape)
    axis = axis % len(shape)
    pre = 1
    for d in shape[:axis]:
        pre *= d
    post = 1
    for d in shape[axis + 1:]:
        post *= d
    res = torch.empty(shape[:axis] + shape[axis + 1:], dtype=torch.float32, device=p.device)
    _hip.check(lib.lq_q_absmax_over_axis(_hip.ptr(p), _hip.ptr(s), _hip.ptr(res), pre, shape[axis], post,
                                         outer, G, inner, _hip.stream_ptr(p.device)), "lq_q_absmax_over_axis")
    return res


_MAX_BINS = 1 << 26   # 256 MiB of uint32 bins; beyond that the integers are not "a few quantisation levels"


def q_unique(parameter: torch.Tensor, scale: torch.Tensor):
    """np.unique(floor(P/s), return_counts=True) of the callbacks (custom_callbacks.py:92, 142) computed on the
    device: range by lq_q_minmax, counts by lq_q_histogram.  Returns (values int32, counts int64), both on the device.
    One small device->host read (the range) is needed to size the histogram -- this is a per-epoch statistic."""
    lib = _hip.load()
    p = _hip.require_device_f32(parameter, "parameter")
    s = _hip.require_device_f32(scale, "scale")
    outer, G, inner = _desc(p, s)
    st = _hip.stream_ptr(p.device)
    mm = torch.tensor([2 ** 31 - 1, -(2 ** 31)], dtype=torch.int32, device=p.device)
    _hip.check(lib.lq_q_minmax(_hip.ptr(p), _hip.ptr(s), _hip.ptr(mm), outer, G, inner, st), "lq_q_minmax")
    lo, hi = (int(v) for v in mm.tolist())
    if lo > hi:                                            # nothing countable (all NaN/Inf)
        return (torch.empty(0, dtype=torch.int32, device=p.device), torch.empty(0, dtype=torch.int64, device=p.device))
    nbins = hi - lo + 1
    if nbins > _MAX_BINS:
        raise ValueError(f"integer range [{lo}, {hi}] too wide for a histogram ({nbins} bins)")
    bins = torch.zeros(nbins, dtype=torch.int32, device=p.device)
    _hip.check(lib.lq_q_histogram(_hip.ptr(p), _hip.ptr(s), lo, nbins, _hip.ptr(bins), outer, G, inner, st), "lq_q_histogram")
    nz = torch.nonzero(bins, as_tuple=False).flatten()
    return (nz + lo).to(torch.int32), bins[nz].to(torch.int64)


def q_minmax(parameter: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(min, max) of floor(P/s) as a 2-element int32 device tensor, without a device->host read; ``out`` (a contiguous
    2-element int32 device tensor) lets a caller gather many ranges into one buffer.  NaN/Inf/beyond-int32 quotients are
    skipped: an all-skipped tensor gives min > max."""
    lib = _hip.load()
    p = _hip.require_device_f32(parameter, "parameter")
    s = _hip.require_device_f32(scale, "scale")
    outer, G, inner = _desc(p, s)
    if out is None:
        out = torch.empty(2, dtype=torch.int32, device=p.device)
    elif out.dtype != torch.int32 or out.numel() != 2 or not out.is_contiguous():
        raise ValueError("out must be a contiguous 2-element int32 tensor")
    out[0], out[1] = 2 ** 31 - 1, -(2 ** 31)
    _hip.check(lib.lq_q_minmax(_hip.ptr(p), _hip.ptr(s), _hip.ptr(out), outer, G, inner, _hip.stream_ptr(p.device)),
               "lq_q_minmax")
    return out


def packed_words(numel: int, bits: int) -> int:
    """Number of uint32 words of the packed stream: ceil(numel * bits / 32)."""
    return (int(numel) * int(bits) + 31) // 32


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    return t if t.data_ptr() % 16 == 0 else t.clone()


def q_pack(parameter: torch.Tensor, scale: torch.Tensor, qmin: Optional[int] = None, bits: Optional[int] = None,
           bad: Optional[torch.Tensor] = None):
    """Bit-packs q = floor(P/s) (K1's division, custom_layers.py:55-60) losslessly: returns ``(words, qmin, bits)`` with
    ``words`` an int32 device tensor holding the uint32 stream of include/lq_hip.h (codes q - qmin, LSB-first), in the
    parameter's LOGICAL C order whatever its memory order.  Without ``qmin``/``bits`` the range is read from the device
    (lq_q_minmax, one sync).  Without ``bad`` the call checks the element count the kernel rejected and raises ValueError;
    with ``bad`` (a 1-element int64 device tensor) that count is added to it and checking it is the caller's business."""
    lib = _hip.load()
    p = _aligned16(_hip.require_device_f32(parameter, "parameter"))
    s = _hip.require_device_f32(scale, "scale")
    outer, G, inner = _desc(p, s)
    if qmin is None or bits is None:
        lo, hi = (int(v) for v in q_minmax(p, s).tolist())
        if lo > hi:
            raise ValueError("no finite integer in floor(P/s): nothing to pack")
        qmin, bits = lo, (hi - lo).bit_length()
    if not 0 <= int(bits) <= 32:
        raise ValueError(f"bits must be in 0..32, got {bits}")
    check_here = bad is None
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int64, device=p.device)
    elif bad.dtype != torch.int64 or bad.numel() != 1 or not bad.is_cuda:
        raise TypeError("bad must be a 1-element int64 device tensor")
    words = torch.empty(packed_words(p.numel(), bits), dtype=torch.int32, device=p.device)
    _hip.check(lib.lq_q_pack(_hip.ptr(p), _hip.ptr(s), int(qmin), int(bits), _hip.ptr(words) if words.numel() else None,
                             _hip.ptr(bad), outer, G, inner, _hip.stream_ptr(p.device)), "lq_q_pack")
    if check_here and int(bad.item()):
        raise ValueError(f"{int(bad.item())} elements of floor(P/s) are NaN, Inf, beyond int32 or outside "
                         f"[{qmin}, {qmin} + 2^{bits} - 1]")
    return words, int(qmin), int(bits)


def q_unpack(words: torch.Tensor, qmin: int, bits: int, scale: torch.Tensor, shape, want_out: bool = True,
             want_q: bool = True, want_restore: bool = True, bad: Optional[torch.Tensor] = None):
    """Inverse of ``q_pack``: returns ``(out, q, p_restore)`` of ``shape`` (contiguous; None where not wanted).
    out = q * s bit for bit as K1's out (a -0 of P comes back +0), q int32, p_restore a float whose floor(P/s) is q.  Every
    p_restore is divided back on the device; without ``bad`` a miss raises ValueError (|q| >= 2^22 can miss), with ``bad``
    the misses are added to it."""
    lib = _hip.load()
    s = _hip.require_device_f32(scale, "scale")
    shape = tuple(int(d) for d in shape)
    outer, G, inner = group_descriptor(shape, tuple(s.shape))
    n = outer * G * inner
    if not 0 <= int(bits) <= 32:
        raise ValueError(f"bits must be in 0..32, got {bits}")
    if int(bits) and (words.dtype != torch.int32 or not words.is_cuda or not words.is_contiguous()
                      or words.numel() != packed_words(n, bits)):
        raise ValueError(f"words must be a contiguous int32 device tensor of {packed_words(n, bits)} elements")
    if not (want_out or want_q or want_restore):
        raise ValueError("nothing to compute")
    out = torch.empty(shape, dtype=torch.float32, device=s.device) if want_out else None
    q = torch.empty(shape, dtype=torch.int32, device=s.device) if want_q else None
    pr = torch.empty(shape, dtype=torch.float32, device=s.device) if want_restore else None
    check_here = want_restore and bad is None
    if check_here:
        bad = torch.zeros(1, dtype=torch.int64, device=s.device)
    elif bad is not None and (bad.dtype != torch.int64 or bad.numel() != 1 or not bad.is_cuda):
        raise TypeError("bad must be a 1-element int64 device tensor")
    _hip.check(lib.lq_q_unpack(_hip.ptr(words) if int(bits) else None, int(qmin), int(bits), _hip.ptr(s), _hip.ptr(out),
                               _hip.ptr(q), _hip.ptr(pr), _hip.ptr(bad), outer, G, inner, _hip.stream_ptr(s.device)),
               "lq_q_unpack")
    if check_here and int(bad.item()):
        raise ValueError(f"{int(bad.item())} restored values do not floor back to their integer (|q| too large for an exact "
                         "float restore)")
    return out, q, pr


def min_value_project_(w: torch.Tensor, min_value: float) -> torch.Tensor:
    """In-place MinValueConstraint: w <- max(w, min_value)  (custom_layers.py:42-43)."""
    lib = _hip.load()
    if not w.is_contiguous():
        raise ValueError("min_value_project_ needs a contiguous tensor (in-place)")
    _hip.require_device_f32(w, "w")
    _hip.check(lib.lq_min_value_project(_hip.ptr(w), w.numel(), float(min_value), _hip.stream_ptr(w.device)),
               "lq_min_value_project")
    return w


def _check_adam_args(scale: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor) -> None:
    for name, t in (("scale", scale), ("grad", grad), ("m", m), ("v", v)):
        _hip.require_device_f32(t, name)
        if not t.is_contiguous() or t.numel() != scale.numel():
            raise ValueError(f"{name} must be contiguous with {scale.numel()} elements")


def scale_adam_step_(scale: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int,
                     lr: float = 1e-4, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-7,
                     min_value: float = 0.0, mode: str = "keras") -> None:
    """K6: Adam + MinValueConstraint projection in one launch (custom_layers.py:158; Keras 2.11 Adam)."""
    lib = _hip.load()
    _check_adam_args(scale, grad, m, v)
    md = _hip.adam_mode(mode)
    _hip.check(lib.lq_scale_adam_step(_hip.ptr(scale), _hip.ptr(grad), _hip.ptr(m), _hip.ptr(v), scale.numel(),
                                      lr, beta1, beta2, eps, int(step), float(min_value), md,
                                      _hip.stream_ptr(scale.device)), "lq_scale_adam_step")


def scale_adam_step_dev_(scale: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step_dev: torch.Tensor,
                         lr: float = 1e-4, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-7,
                         min_value: float = 0.0, mode: str = "keras") -> None:
    """K6, hipGraph-capturable form: ``step_dev`` is a 1-element int64 device tensor holding the 1-based step."""
    lib = _hip.load()
    _check_adam_args(scale, grad, m, v)
    if step_dev.dtype != torch.int64 or not step_dev.is_cuda or step_dev.numel() != 1:
        raise TypeError("step_dev must be a 1-element int64 device tensor")
    md = _hip.adam_mode(mode)
    _hip.check(lib.lq_scale_adam_step_dev(_hip.ptr(scale), _hip.ptr(grad), _hip.ptr(m), _hip.ptr(v), scale.numel(),
                                          lr, beta1, beta2, eps, _hip.ptr(step_dev), float(min_value), md,
                                          _hip.stream_ptr(scale.device)), "lq_scale_adam_step_dev")


# --------------------------------------------------------------------------- autograd ops
class _NestedQuantFn(torch.autograd.Function):
    """custom_layers.py:49-120 -- forward K1, backward (dy, K2+K3, None)."""

    @staticmethod
    def forward(ctx, parameter, scale, penalty_threshold, defer_scale_grad=False):
        ctx.save_for_backward(parameter, scale)
        ctx.penalty_threshold = float(penalty_threshold)
        ctx.defer = bool(defer_scale_grad)
        return fq_forward(parameter, scale)

    @staticmethod
    def backward(ctx, dy):
        parameter, scale = ctx.saved_tensors
        ds = None
        # defer: exact data-parallel mode recomputes ds from the all-reduced dP after the exchange (ddp.py, mode B)
        if ctx.needs_input_grad[1] and not ctx.defer:
            ds = fq_scale_grad(parameter, scale, dy, ctx.penalty_threshold)
        return (dy if ctx.needs_input_grad[0] else None), ds, None, None      # :118  dP is dy itself (STE)


def _conv_extents(shape):
    kh, kw, ci, co = (int(d) for d in shape)
    return kh * kw, ci, co


def fq_forward_oihw(kernel: torch.Tensor, scale: torch.Tensor, hwio_out: bool = True):
    """K1 on an HWIO conv kernel (custom_layers.py:321, 340) that also emits the OIHW tensor MIOpen consumes: returns
    (out_hwio, out_oihw) with out_oihw == out_hwio.permute(3, 2, 0, 1) bit for bit, in ONE launch (no transpose kernel).
    ``hwio_out=False``: where the LDS-tile kernel takes the tensor, only the OIHW tensor is written (8 bytes per element
    instead of 12) and out_hwio is the permuted view of it."""
    lib = _hip.load()
    p = _hip.require_device_f32(kernel, "kernel")
    s = _hip.require_device_f32(scale, "scale")
    if p.dim() != 4:
        raise ValueError("fq_forward_oihw needs an HWIO conv kernel (kh, kw, ci, co)")
    hw, ci, co = _conv_extents(p.shape)
    outer, G, inner = _desc(p, s)
    companion_only = (not hwio_out) and p.data_ptr() % 16 == 0 and lib.lq_conv_tile_supported(hw, ci, co, outer, G, inner) == 1
    out = None if companion_only else torch.empty_like(p)
    out_oihw = torch.empty((co, ci, p.shape[0], p.shape[1]), dtype=torch.float32, device=p.device)
    _hip.check(lib.lq_fq_forward_oihw(_hip.ptr(p), _hip.ptr(s), _hip.ptr(out), _hip.ptr(out_oihw), hw, ci, co,
                                      outer, G, inner, _hip.stream_ptr(p.device)), "lq_fq_forward_oihw")
    return (out if out is not None else out_oihw.permute(2, 3, 1, 0)), out_oihw


def fq_scale_grad_oihw(kernel: torch.Tensor, scale: torch.Tensor, dy_oihw: torch.Tensor, penalty_threshold: float):
    """K2+K3 with the upstream gradient in OIHW order (MIOpen's weight gradient as it stands): returns (ds, dP_hwio);
    ds is bit-identical to ``fq_scale_grad(kernel, scale, dy_oihw.permute(2, 3, 1, 0))``, dP is that permuted dy."""
    lib = _hip.load()
    p = _hip.require_device_f32(kernel, "kernel")
    s = _hip.require_device_f32(scale, "scale")
    d = _hip.require_device_f32(dy_oihw, "dy_oihw")
    hw, ci, co = _conv_extents(p.shape)
    if tuple(d.shape) != (co, ci, p.shape[0], p.shape[1]):
        raise ValueError(f"dy_oihw shape {tuple(d.shape)} does not match the kernel {tuple(p.shape)}")
    outer, G, inner = _desc(p, s)
    ds = torch.empty_like(s)
    dP = torch.empty_like(p)
    ws = _hip.workspace(p.device, lib.lq_conv_workspace_bytes(hw, ci, co, outer, G, inner))
    _hip.check(lib.lq_fq_scale_grad_oihw(_hip.ptr(p), _hip.ptr(s), _hip.ptr(d), float(penalty_threshold), _hip.ptr(ds),
                                         _hip.ptr(dP), _hip.ptr(ws), ws.numel(), hw, ci, co, outer, G, inner,
                                         _hip.stream_ptr(p.device)), "lq_fq_scale_grad_oihw")
    return ds, dP


class _NestedQuantConvFn(torch.autograd.Function):
    """The nested-quantization op on an HWIO conv kernel, handing MIOpen its OIHW tensor directly: forward K1 with the OIHW
    companion store, backward K2+K3 reading MIOpen's OIHW weight gradient and returning dP in HWIO order.  Same q, out and
    ds as ``_NestedQuantFn`` bit for bit (custom_layers.py:49-120, 338-350); two transposition launches fewer per layer."""

    @staticmethod
    def forward(ctx, kernel, scale, penalty_threshold, defer_scale_grad=False):
        ctx.save_for_backward(kernel, scale)
        ctx.penalty_threshold = float(penalty_threshold)
        ctx.defer = bool(defer_scale_grad)
        return fq_forward_oihw(kernel, scale, hwio_out=False)[1]

    @staticmethod
    def backward(ctx, dy_oihw):
        kernel, scale = ctx.saved_tensors
        if ctx.defer or not ctx.needs_input_grad[1]:
            return (dy_oihw.permute(2, 3, 1, 0) if ctx.needs_input_grad[0] else None), None, None, None
        ds, dP = fq_scale_grad_oihw(kernel, scale, dy_oihw, ctx.penalty_threshold)
        return (dP if ctx.needs_input_grad[0] else None), ds, None, None


def my_custom_gradient_oihw(kernel, scale, penalty_threshold, *, defer_scale_grad=False):
    """``my_custom_gradient`` for an HWIO conv kernel whose consumer wants OIHW: returns the fake-quantised kernel in OIHW
    layout (co, ci, kh, kw), contiguous.  Gradients flow back to the HWIO parameter."""
    if isinstance(penalty_threshold, torch.Tensor):
        penalty_threshold = float(penalty_threshold)
    return _NestedQuantConvFn.apply(kernel, scale, penalty_threshold, defer_scale_grad)


class _STEQuantFn(torch.autograd.Function):
    """CL custom_layers.py:49-64 -- forward K1, backward (dy, zeros_like(scale))."""

    @staticmethod
    def forward(ctx, parameter, scale):
        ctx.save_for_backward(scale)
        return fq_forward(parameter, scale)

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        ds = torch.zeros_like(scale) if ctx.needs_input_grad[1] else None    # :62
        return (dy if ctx.needs_input_grad[0] else None), ds


class _STEScaleQuantFn(torch.autograd.Function):
    """Forward K1, backward (dy, straight-through scale gradient): the variant the reference's paper_implementation leaves
    as a TODO (its scale gradient is zeros)."""

    @staticmethod
    def forward(ctx, parameter, scale, grad_scale, defer_scale_grad=False):
        ctx.save_for_backward(parameter, scale)
        ctx.grad_scale = float(grad_scale)
        ctx.defer = bool(defer_scale_grad)
        return fq_forward(parameter, scale)

    @staticmethod
    def backward(ctx, dy):
        parameter, scale = ctx.saved_tensors
        ds = None
        # defer: the batch computes every scale gradient of the step in two launches (batch.py)
        if ctx.needs_input_grad[1] and not ctx.defer:
            ds = fq_scale_grad_ste(parameter, scale, dy, ctx.grad_scale)
        return (dy if ctx.needs_input_grad[0] else None), ds, None, None


class _ClipQuantFn(torch.autograd.Function):
    """The clipped pair: forward lq_fq_forward_clip_r, backward lq_fq_backward_clip_r (``rounding``: floor or nearest).
    ``want_ds``: the scale receives the LSQ gradient (scale_gradient="ste"); otherwise zeros like the STE-only op (the
    loss-term-only rule) and the kernel's sum is dropped."""

    @staticmethod
    def forward(ctx, parameter, scale, qmin, qmax, grad_scale, want_ds, rounding="floor"):
        ctx.save_for_backward(parameter, scale)
        ctx.rounding = rounding
        ctx.q_range = (int(qmin), int(qmax))
        ctx.grad_scale = float(grad_scale)
        ctx.want_ds = bool(want_ds)
        return fq_forward_clip(parameter, scale, qmin, qmax, rounding=rounding)

    @staticmethod
    def backward(ctx, dy):
        parameter, scale = ctx.saved_tensors
        want_ds = ctx.want_ds and ctx.needs_input_grad[1]
        dP, ds, _ = fq_backward_clip(parameter, scale, dy, *ctx.q_range, grad_scale=ctx.grad_scale, want_ds=want_ds,
                                     rounding=ctx.rounding)
        if ds is None and ctx.needs_input_grad[1]:
            ds = torch.zeros_like(scale)
        return (dP if ctx.needs_input_grad[0] else None), ds, None, None, None, None, None


class _GroupQuantFn(torch.autograd.Function):
    """``_ClipQuantFn`` with group-wise scales: forward lq_fq_forward_group, backward lq_fq_backward_group."""

    @staticmethod
    def forward(ctx, parameter, scale, qmin, qmax, group_size, grad_scale, want_ds, rounding="floor"):
        ctx.save_for_backward(parameter, scale)
        ctx.rounding = rounding
        ctx.q_range = (int(qmin), int(qmax))
        ctx.group_size = int(group_size)
        ctx.grad_scale = float(grad_scale)
        ctx.want_ds = bool(want_ds)
        return fq_forward_group(parameter, scale, qmin, qmax, group_size, rounding=rounding)

    @staticmethod
    def backward(ctx, dy):
        parameter, scale = ctx.saved_tensors
        want_ds = ctx.want_ds and ctx.needs_input_grad[1]
        dP, ds, _ = fq_backward_group(parameter, scale, dy, *ctx.q_range, ctx.group_size, grad_scale=ctx.grad_scale,
                                      want_ds=want_ds, rounding=ctx.rounding)
        if ds is None and ctx.needs_input_grad[1]:
            ds = torch.zeros_like(scale)
        return (dP if ctx.needs_input_grad[0] else None), ds, None, None, None, None, None, None


class _GroupAffineQuantFn(torch.autograd.Function):
    """``_GroupQuantFn`` with an offset per group: forward lq_fq_forward_group_affine, backward lq_fq_backward_group_affine.
    The offset's gradient is scaled like the scale's (LSQ+)."""

    @staticmethod
    def forward(ctx, parameter, scale, offset, qmin, qmax, group_size, grad_scale, rounding="floor"):
        ctx.save_for_backward(parameter, scale, offset)
        ctx.rounding = rounding
        ctx.q_range = (int(qmin), int(qmax))
        ctx.group_size = int(group_size)
        ctx.grad_scale = float(grad_scale)
        return fq_forward_group_affine(parameter, scale, offset, qmin, qmax, group_size, rounding=rounding)

    @staticmethod
    def backward(ctx, dy):
        parameter, scale, offset = ctx.saved_tensors
        dP, ds, db, _ = fq_backward_group_affine(parameter, scale, offset, dy, *ctx.q_range, ctx.group_size,
                                                 grad_scale=ctx.grad_scale, want_ds=ctx.needs_input_grad[1],
                                                 want_db=ctx.needs_input_grad[2], rounding=ctx.rounding)
        return (dP if ctx.needs_input_grad[0] else None), ds, db, None, None, None, None, None


class _MxQuantFn(torch.autograd.Function):
    """``_GroupQuantFn`` on a microscaling element grid: forward lq_fq_forward_mx, backward lq_fq_backward_mx.  ``group_size`` None:
    a one-axis or scalar scale (a bias: one group)."""

    @staticmethod
    def forward(ctx, parameter, scale, element_format, scale_format, group_size, grad_scale):
        ctx.save_for_backward(parameter, scale)
        ctx.mx = (element_format, group_size, scale_format)
        ctx.grad_scale = float(grad_scale)
        return fq_forward_mx(parameter, scale, element_format, group_size, scale_format)

    @staticmethod
    def backward(ctx, dy):
        parameter, scale = ctx.saved_tensors
        dP, ds, _ = fq_backward_mx(parameter, scale, dy, *ctx.mx, grad_scale=ctx.grad_scale, want_ds=ctx.needs_input_grad[1])
        return (dP if ctx.needs_input_grad[0] else None), ds, None, None, None, None


SCALE_GRADIENTS = (None, "ste")


def my_custom_gradient(parameter, scale, penalty_threshold=None, *, scale_gradient=None, grad_scale=1.0, defer_scale_grad=False,
                       q_range=None, rounding="floor", group_size=None, offset=None, element_format=None, scale_format="e8m0"):
    """The reference op.  With ``penalty_threshold`` -> nested-quantization variant
    (custom_layers.py:49-120); without -> STE-only variant (CL custom_layers.py:49-64).
    ``scale_gradient="ste"`` (not in the reference, only without ``penalty_threshold``): the scale receives the
    straight-through gradient ``grad_scale * sum dy * (floor(P/s) - P/s)`` instead of zeros.
    ``defer_scale_grad`` (not in the reference): backward returns dP only; the caller computes ds later from the
    all-reduced dP (exact data-parallel mode, ddp.py).
    ``q_range=(qmin, qmax)`` (not in the reference, only without ``penalty_threshold``): the clipped quantizer -- integers
    saturate at the range, clipped elements pass no gradient to ``parameter``; with ``scale_gradient="ste"`` the scale gets the
    LSQ gradient (clipped elements pull it by ``dy * qmin`` / ``dy * qmax``), with ``None`` it gets zeros.
    ``rounding="nearest"`` (not in the reference, only with ``q_range``): the integers are rint(P/s), round half to even, instead
    of floor(P/s), and the LSQ residual is rint(t) - t in [-1/2, 1/2].
    ``group_size=gs`` (not in the reference, only with ``q_range``): ``scale`` is a group-wise scale matrix
    (descriptor.groupwise_scale_shape): one scale per ``gs`` elements along one axis of the parameter's memory.
    ``offset=b`` (not in the reference, only with ``group_size`` and ``scale_gradient="ste"``): the asymmetric quantizer
    ``clamp(rnd((P - b) / s)) * s + b`` with one learned offset per group (``b`` has the scale's shape); gradients go to the
    parameter, the scale and the offset (LSQ+: the sum of dy over the group's clipped elements, times ``grad_scale``).
    ``element_format=F`` (not in the reference; one of ops.ELEMENT_FORMATS): the OCP microscaling quantizer -- elements on the
    minifloat grid of ``F`` under one scale per group, a power of two for ``scale_format="e8m0"`` (the default) or the scale as it
    is for "fp32".  ``scale`` is a group-wise matrix with its ``group_size``, or with ``group_size=None`` a scalar or one-axis
    scale (a bias: one group).  Gradients are the straight-through ones (``scale_gradient`` may be left out or "ste")."""
    if element_format is not None:
        check_element_format(element_format)
        check_scale_format(scale_format)
        if penalty_threshold is not None:
            raise ValueError("element_format with a penalty_threshold: the nested-quantization vote is defined on the unclipped "
                             "integer quantizer")
        if q_range is not None:
            raise ValueError("element_format with a q_range: an element format brings its own grid and range")
        if rounding != "floor":
            raise ValueError("element_format with a rounding: a minifloat grid rounds to nearest, ties to even, and nothing else")
        if offset is not None:
            raise ValueError("element_format with an offset: the microscaling formats are symmetric")
        if scale_gradient not in (None, "ste"):
            raise ValueError(f'element_format needs scale_gradient="ste", got {scale_gradient!r}')
        if defer_scale_grad:
            raise ValueError("element_format with defer_scale_grad: the all-reduced dP of a saturating layer no longer holds the dy "
                             "of its saturated elements, so ds cannot be recomputed from it")
        return _MxQuantFn.apply(parameter, scale, element_format, scale_format, None if group_size is None else int(group_size),
                                float(grad_scale))
    if offset is not None:
        if group_size is None:
            raise ValueError("offset needs a group_size: the asymmetric quantizer exists for group-wise scales only (a group_size "
                             "of the line length or more gives per-channel offsets)")
        if q_range is None:
            raise ValueError("offset needs a q_range: the asymmetric quantizer places a chosen integer range over each group")
        if penalty_threshold is not None:
            raise ValueError("offset with a penalty_threshold: the nested-quantization vote is defined on the unclipped "
                             "symmetric quantizer")
        if scale_gradient != "ste":
            raise ValueError('offset needs scale_gradient="ste": the loss-term-only rule has no gradient for an offset')
    if group_size is not None:
        if q_range is None:
            raise ValueError("group_size needs a q_range: group-wise scales exist for the clipped quantizer only (the unclipped "
                             "ops broadcast one-axis scales)")
        if penalty_threshold is not None:
            raise ValueError("group_size with a penalty_threshold: the nested-quantization vote is defined on the unclipped "
                             "quantizer with one-axis scales")
        if defer_scale_grad:
            raise ValueError("group_size with defer_scale_grad: the all-reduced dP of a clipped layer no longer holds the dy of "
                             "its clipped elements, so ds cannot be recomputed from it")
    if scale_gradient not in SCALE_GRADIENTS:
        raise ValueError(f"scale_gradient must be one of {SCALE_GRADIENTS}, got {scale_gradient!r}")
    check_rounding(rounding, q_range is not None)
    if q_range is not None:
        if penalty_threshold is not None:
            raise ValueError("q_range with a penalty_threshold: the nested-quantization vote is defined on the unclipped "
                             "quantizer; a clipped layer needs penalty_threshold=None")
        if defer_scale_grad:
            raise ValueError("q_range with defer_scale_grad: the all-reduced dP of a clipped layer no longer holds the dy of its "
                             "clipped elements, so ds cannot be recomputed from it")
        qmin, qmax = check_q_range(*q_range)
        if offset is not None:
            return _GroupAffineQuantFn.apply(parameter, scale, offset, qmin, qmax, int(group_size), float(grad_scale), rounding)
        if group_size is not None:
            return _GroupQuantFn.apply(parameter, scale, qmin, qmax, int(group_size), float(grad_scale), scale_gradient == "ste",
                                       rounding)
        return _ClipQuantFn.apply(parameter, scale, qmin, qmax, float(grad_scale), scale_gradient == "ste", rounding)
    if scale_gradient == "ste":
        if penalty_threshold is not None:
            raise ValueError('scale_gradient="ste" replaces the nested-quantization vote: it needs penalty_threshold=None')
        return _STEScaleQuantFn.apply(parameter, scale, float(grad_scale), defer_scale_grad)
    if penalty_threshold is None:
        return _STEQuantFn.apply(parameter, scale)
    if isinstance(penalty_threshold, torch.Tensor):
        penalty_threshold = float(penalty_threshold)      # tf.stop_gradient(penalty_threshold), :55
    return _NestedQuantFn.apply(parameter, scale, penalty_threshold, defer_scale_grad)


# --------------------------------------------------------------------------- penalty terms
def _up(grad_out: torch.Tensor) -> torch.Tensor:
    g = grad_out.reshape(1)
    return _hip.require_device_f32(g, "upstream gradient")


class _MaxBinTerm(torch.autograd.Function):
    """mean_g max_{i in g} |P_i|/s_g  (custom_loss_functions.py:90-100,110) -- K5a."""

    @staticmethod
    def forward(ctx, parameter, scale):
        lib = _hip.load()
        p, s, (outer, G, inner) = _param(parameter, scale)
        mb = torch.empty(G, dtype=torch.float32, device=p.device)
        ties = torch.empty(G, dtype=torch.int32, device=p.device)
        term = torch.empty((), dtype=torch.float32, device=p.device)
        ws = _hip.workspace_for(p.device, outer, G, inner)
        _hip.check(lib.lq_penalty_maxbin_fwd(_hip.ptr(p), _hip.ptr(s), _hip.ptr(mb), _hip.ptr(ties), _hip.ptr(term),
                                             _hip.ptr(ws), ws.numel(), outer, G, inner,
                                             _hip.stream_ptr(p.device)), "lq_penalty_maxbin_fwd")
        ctx.save_for_backward(p, s, mb, ties)
        ctx.desc = (outer, G, inner)
        return term

    @staticmethod
    def backward(ctx, grad_out):
        lib = _hip.load()
        p, s, mb, ties = ctx.saved_tensors
        outer, G, inner = ctx.desc
        c = _up(grad_out)
        dP = torch.empty_like(p)
        ds = torch.empty_like(s)
        _hip.check(lib.lq_penalty_maxbin_bwd(_hip.ptr(p), _hip.ptr(s), _hip.ptr(mb), _hip.ptr(ties), _hip.ptr(c), 1.0,
                                             _hip.ptr(dP), _hip.ptr(ds), outer, G, inner,
                                             _hip.stream_ptr(p.device)), "lq_penalty_maxbin_bwd")
        return dP, ds


class _DifferenceTerm(torch.autograd.Function):
    """mean |P - P/s|  (custom_loss_functions.py:172-176) -- K5b."""

    @staticmethod
    def forward(ctx, parameter, scale):
        lib = _hip.load()
        p, s, (outer, G, inner) = _param(parameter, scale)
        term = torch.empty((), dtype=torch.float32, device=p.device)
        ws = _hip.workspace_for(p.device, outer, G, inner)
        _hip.check(lib.lq_penalty_difference_fwd(_hip.ptr(p), _hip.ptr(s), _hip.ptr(term), _hip.ptr(ws), ws.numel(),
                                                 outer, G, inner, _hip.stream_ptr(p.device)),
                   "lq_penalty_difference_fwd")
        ctx.save_for_backward(p, s)
        ctx.desc = (outer, G, inner)
        return term

    @staticmethod
    def backward(ctx, grad_out):
        lib = _hip.load()
        p, s = ctx.saved_tensors
        outer, G, inner = ctx.desc
        c = _up(grad_out)
        dP = torch.empty_like(p)
        ds = torch.empty_like(s)
        ws = _hip.workspace_for(p.device, outer, G, inner)
        _hip.check(lib.lq_penalty_difference_bwd(_hip.ptr(p), _hip.ptr(s), _hip.ptr(c), 1.0, _hip.ptr(dP), _hip.ptr(ds),
                                                 _hip.ptr(ws), ws.numel(), outer, G, inner,
                                                 _hip.stream_ptr(p.device)), "lq_penalty_difference_bwd")
        return dP, ds


class _InverseTerm(torch.autograd.Function):
    """mean 1/where(s==0, eps, s)  (custom_loss_functions.py:252-256) -- K5c."""

    @staticmethod
    def forward(ctx, scale):
        lib = _hip.load()
        s = _hip.require_device_f32(scale, "scale")
        term = torch.empty((), dtype=torch.float32, device=s.device)
        _hip.check(lib.lq_penalty_inverse_fwd(_hip.ptr(s), _hip.ptr(term), s.numel(), _hip.stream_ptr(s.device)),
                   "lq_penalty_inverse_fwd")
        ctx.save_for_backward(s)
        return term

    @staticmethod
    def backward(ctx, grad_out):
        lib = _hip.load()
        (s,) = ctx.saved_tensors
        c = _up(grad_out)
        ds = torch.empty_like(s)
        _hip.check(lib.lq_penalty_inverse_bwd(_hip.ptr(s), _hip.ptr(c), 1.0, _hip.ptr(ds), s.numel(),
                                              _hip.stream_ptr(s.device)), "lq_penalty_inverse_bwd")
        return ds


def maxbin_term(parameter: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return _MaxBinTerm.apply(parameter, scale)


def difference_term(parameter: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return _DifferenceTerm.apply(parameter, scale)


def inverse_term(scale: torch.Tensor) -> torch.Tensor:
    return _InverseTerm.apply(scale)
