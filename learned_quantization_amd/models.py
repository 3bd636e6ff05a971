"""The three topologies of the reference's experiments, built from this package's custom layers (SURVEY f-3).

  mnist_dense      /root/reference/MNIST/nested_quantization_layer/experiment.py:119-162
                   Flatten -> CustomDense(128) -> relu -> CustomDense(10) -> softmax
  cifar_cnn        /root/reference/CIFAR-10/nested_quantization_layer/experiment.py:279-432
                   3 x [CustomConv(f) relu BN CustomConv(f) relu BN MaxPool Dropout], f = 32/64/128,
                   Dense(128, relu) BN Dropout(0.5) Dense(10, softmax)
  resnet18_like    /root/reference/IMAGENETTE/nested_quantization_layer/experiment.py:627-760
                   CustomConv 7x7/2 BN relu MaxPool3x3/2 Dropout(0.2); 8 basic blocks 64,64,128,128,256,256,512,512
                   (stride 2 + quantised 1x1 shortcut conv + BN at each widening, l2(1e-4) on block convs);
                   Dropout GAP Dropout Dense(softmax)

Only the custom layers are this package's product; BatchNorm / pooling / dropout / plain Dense / the
convolution itself are stock torch (MIOpen / rocBLAS).  Keras defaults are mirrored where they affect
semantics: BatchNormalization(momentum=0.99, epsilon=1e-3) == torch momentum 0.01, eps 1e-3;
RandomNormal stddev 0.05 for kernels AND biases of custom layers (custom_layers.py:318-319); plain Dense
layers get RandomNormal kernels and zero biases.  Models output class probabilities (softmax), as the
reference's do, so ``compute_total_loss(y_true, y_pred)`` keeps its meaning; like Keras' softmax activation the output
carries its logits (``losses.softmax``), from which the cross-entropy is computed.  Activations are NCHW.

``mode="nq"``: ``value`` is the penalty_threshold (nested-quantization scale gradient);
``mode="cl"``: ``value`` is the penalty_rate (STE-only op; scales learn through a custom loss term);
``mode="ste"``: the straight-through scale gradient (ops.fq_scale_grad_ste), no loss term, ``value`` is ignored;
``mode="stecl"``: the same plus a custom loss term, ``value`` is the penalty_rate.
``bits`` / ``signed`` / ``q_range`` (``build_model``; modes "cl", "ste", "stecl"): every quantised tensor uses the clipped
quantizer with that integer range (layers.py); ``rounding="nearest"`` makes it round to nearest (ties to even), not down.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .layers import CustomConv2DLayer, CustomDenseLayer, RandomNormal, i8_dense_chain, l2, mx_dense_chain
from .losses import softmax


def _bn(c: int) -> nn.BatchNorm2d:
    return nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)


def _kw(mode: str, value: float):
    if mode == "nq":
        return dict(penalty_threshold=value)
    if mode == "cl":
        return dict(penalty_threshold=None, penalty_rate=value)
    if mode == "nqcl":      # (penalty_threshold, penalty_rate): nested-quantization op + a loss term (extension, train.py)
        return dict(penalty_threshold=value[0], penalty_rate=value[1])
    if mode == "ste":       # straight-through scale gradient, no loss term (extension: the reference leaves this slot a TODO)
        return dict(penalty_threshold=None, scale_gradient="ste")
    if mode == "stecl":     # the same + a loss term
        return dict(penalty_threshold=None, penalty_rate=value, scale_gradient="ste")
    raise ValueError("mode must be 'nq', 'cl', 'nqcl', 'ste' or 'stecl'")


def _plain_dense(n_in: int, n_out: int, seed: Optional[int]) -> nn.Linear:
    lin = nn.Linear(n_in, n_out)
    with torch.no_grad():
        lin.weight.copy_(RandomNormal(seed=seed)((n_out, n_in)))
        lin.bias.zero_()
    return lin


class MNISTDense(nn.Module):
    """784 -> 128 -> 10, both layers quantised (101 770 quantised elements)."""

    def __init__(self, mode="nq", value=1e-10, seed=42, orientation="rowwise", input_shape=(28, 28, 1), device=None,
                 trained_weights=None):
        super().__init__()
        n_in = 1
        for d in input_shape:
            n_in *= d
        init = RandomNormal(seed=seed)
        tw = trained_weights or [None, None]
        self.dense_1 = CustomDenseLayer(seed=seed, units=128, orientation=orientation, initializer=init,
                                        name="custom_dense_layer_1", regularizer=None, trained_weights=tw[0],
                                        input_shape=n_in, device=device, **_kw(mode, value))
        self.dense_2 = CustomDenseLayer(seed=seed, units=10, orientation=orientation, initializer=init,
                                        name="custom_dense_layer_2", regularizer=None, trained_weights=tw[1],
                                        input_shape=128, device=device, **_kw(mode, value))

    def mx_chain(self):
        """The Dense tail as layers.mx_dense_chain takes it: nothing but relu lies between the two layers."""
        return [(self.dense_1, "relu"), (self.dense_2, None)]

    i8_chain = mx_chain        # the same tail, as layers.i8_dense_chain takes it

    def logits(self, x):
        x = torch.flatten(x, 1)
        fused = getattr(self, "_mx_fused", None)
        if fused is not None and not self.training:               # inside layers.mx_hardware(..., fused=True), eval mode
            return mx_dense_chain(x, self.mx_chain(), *fused[0], **fused[1])
        fused = getattr(self, "_i8_fused", None)
        if fused is not None and not self.training:               # inside layers.i8_hardware(..., fused=True), eval mode
            return i8_dense_chain(x, self.i8_chain(), *fused[0], **fused[1])
        x = F.relu(self.dense_1(x))
        return self.dense_2(x)

    def forward(self, x):
        return softmax(self.logits(x), dim=1)


class CIFARCNN(nn.Module):
    """Six quantised 3x3 convs (287 008 quantised elements) + two plain Dense layers."""

    def __init__(self, mode="nq", value=1e-11, seed=42, orientation="channelwise", input_shape=(3, 32, 32),
                 num_classes=10, device=None):
        super().__init__()
        init = RandomNormal(seed=seed)
        kw = _kw(mode, value)
        chans = [(input_shape[0], 32, "32_1"), (32, 32, "32_2"), (32, 64, "64_1"), (64, 64, "64_2"),
                 (64, 128, "128_1"), (128, 128, "128_2")]
        self.convs = nn.ModuleList()
        self.bns = nn.ModuleList()
        for ci, co, tag in chans:
            self.convs.append(CustomConv2DLayer(seed=seed, orientation=orientation, initializer=init, filters=co,
                                                kernel_size=(3, 3), strides=(1, 1), padding="same",
                                                name=f"custom_conv2d_layer_{tag}", regularizer=None, trained_weights=None,
                                                input_shape=ci, device=device, **kw))
            self.bns.append(_bn(co))
        self.drops = nn.ModuleList([nn.Dropout(0.2), nn.Dropout(0.3), nn.Dropout(0.4)])
        h, w = input_shape[1] // 8, input_shape[2] // 8
        self.dense_1 = _plain_dense(128 * h * w, 128, seed)
        self.bn_dense = nn.BatchNorm1d(128, eps=1e-3, momentum=0.01)
        self.drop_dense = nn.Dropout(0.5)
        self.out = _plain_dense(128, num_classes, seed)
        if device is not None:
            self.to(device)

    def forward(self, x):
        for blk in range(3):
            for j in range(2):
                k = 2 * blk + j
                x = self.bns[k](F.relu(self.convs[k](x)))      # conv -> relu -> BN (experiment.py:309-311)
            x = self.drops[blk](F.max_pool2d(x, 2))
        x = torch.flatten(x.permute(0, 2, 3, 1), 1)           # Keras flattens NHWC
        x = self.drop_dense(self.bn_dense(F.relu(self.dense_1(x))))
        return softmax(self.out(x), dim=1)


class _ResidualBlock(nn.Module):
    """ResNet v1 basic block of IMAGENETTE/.../experiment.py:627-704."""

    def __init__(self, ci, filters, stride, idx, mode, value, seed, orientation, device):
        super().__init__()
        init = RandomNormal(seed=seed)
        reg = l2(1e-4)
        kw = _kw(mode, value)
        mk = lambda cin, k, s, name: CustomConv2DLayer(                                      # noqa: E731
            seed=seed, orientation=orientation, initializer=init, filters=filters, kernel_size=k, strides=s,
            padding="same", name=name, regularizer=reg, input_shape=cin, device=device, **kw)
        self.conv1 = mk(ci, (3, 3), stride, f"custom_conv2d_layer_{filters}_{idx}_0")
        self.bn1 = _bn(filters)
        self.conv2 = mk(filters, (3, 3), (1, 1), f"custom_conv2d_layer_{filters}_{idx}_1")
        self.bn2 = _bn(filters)
        self.shortcut = None
        if tuple(stride) != (1, 1):
            self.shortcut = mk(ci, (1, 1), stride, "custom_conv2d_layer_shortcut")
            self.bn_s = _bn(filters)

    def forward(self, x):
        sc = x
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        if self.shortcut is not None:
            sc = self.bn_s(self.shortcut(x))
        return F.relu(y + sc)


class ResNet18Like(nn.Module):
    """20 quantised convs: kernels 11 166 912 + biases 4 800 = 11 171 712 quantised elements."""

    def __init__(self, mode="nq", value=1e-11, seed=42, orientation="channelwise", input_shape=(3, 224, 224),
                 num_classes=10, device=None):
        super().__init__()
        init = RandomNormal(seed=seed)
        self.stem = CustomConv2DLayer(seed=seed, orientation=orientation, initializer=init, filters=64, kernel_size=(7, 7),
                                      strides=(2, 2), padding="same", name="custom_conv2d_layer_64_0", regularizer=None,
                                      input_shape=input_shape[0], device=device, **_kw(mode, value))
        self.bn0 = _bn(64)
        self.drop0 = nn.Dropout(0.2)
        cfg = [(64, 64, (1, 1), 1), (64, 64, (1, 1), 2), (64, 128, (2, 2), 1), (128, 128, (1, 1), 2),
               (128, 256, (2, 2), 1), (256, 256, (1, 1), 2), (256, 512, (2, 2), 1), (512, 512, (1, 1), 2)]
        self.blocks = nn.ModuleList([_ResidualBlock(ci, co, st, idx, mode, value, seed, orientation, device)
                                     for ci, co, st, idx in cfg])
        self.drop1 = nn.Dropout(0.3)
        self.drop2 = nn.Dropout(0.3)
        self.out = _plain_dense(512, num_classes, seed)
        if device is not None:
            self.to(device)

    def forward(self, x):
        x = F.relu(self.bn0(self.stem(x)))
        # MaxPooling2D(pool 3, stride 2, padding "same"): for even extents TF pads (0, 1); -inf padding
        h, w = x.shape[-2:]
        ph = max((-(-h // 2) - 1) * 2 + 3 - h, 0)
        pw = max((-(-w // 2) - 1) * 2 + 3 - w, 0)
        x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2), value=float("-inf"))
        x = self.drop0(F.max_pool2d(x, 3, 2))
        for b in self.blocks:
            x = b(x)
        x = self.drop2(torch.mean(self.drop1(x), dim=(2, 3)))
        return softmax(self.out(x), dim=1)


class _BottleneckBlock(nn.Module):
    """ResNet v1 bottleneck (1x1 reduce, 3x3, 1x1 expand x4) in the style of ``_ResidualBlock``: quantised convs with bias,
    BN after every conv, quantised 1x1 projection shortcut where the shape changes, l2(1e-4) on the block convs."""

    def __init__(self, ci, width, stride, project, idx, values, seed, orientation, device, mode):
        super().__init__()
        init = RandomNormal(seed=seed)
        reg = l2(1e-4)
        co = 4 * width

        def mk(cin, cout, k, s, name, value):
            return CustomConv2DLayer(seed=seed, orientation=orientation, initializer=init, filters=cout, kernel_size=k, strides=s,
                                     padding="same", name=name, regularizer=reg, input_shape=cin, device=device, **_kw(mode, value))
        self.conv1 = mk(ci, width, (1, 1), (1, 1), f"custom_conv2d_layer_{width}_{idx}_0", values[0])
        self.bn1 = _bn(width)
        self.conv2 = mk(width, width, (3, 3), stride, f"custom_conv2d_layer_{width}_{idx}_1", values[1])
        self.bn2 = _bn(width)
        self.conv3 = mk(width, co, (1, 1), (1, 1), f"custom_conv2d_layer_{width}_{idx}_2", values[2])
        self.bn3 = _bn(co)
        self.shortcut = None
        if project:
            self.shortcut = mk(ci, co, (1, 1), stride, "custom_conv2d_layer_shortcut", values[3])
            self.bn_s = _bn(co)

    def forward(self, x):
        sc = x
        y = F.relu(self.bn1(self.conv1(x)))
        y = F.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        if self.shortcut is not None:
            sc = self.bn_s(self.shortcut(x))
        return F.relu(y + sc)


class ResNet50Like(nn.Module):
    """BASELINE.json configs[4] ("IMAGENETTE ResNet-50, mixed 4/8-bit learned scales").  EXTENSION WITHOUT A REFERENCE CALL
    SITE: the reference's only ResNets are the ResNet-18-like net above and CIFAR-10/paper_implementation/resnet.py:139-140;
    there is no bit-width parameter anywhere -- quantisation intensity follows from the threshold / rate, so
    "mixed" is modelled as a per-layer ``value``: ``value`` may be a pair (coarse, fine); 3x3 convs get the first entry,
    1x1 convs, the stem and the classifier the second.  The fake-quant op itself is shape-generic and is checked against
    the oracle on exactly these tensors (tests/test_gpu_parity.py::test_resnet50_kernel_shapes_full_size).
    53 quantised convs (with bias) + a quantised Dense classifier = 108 quantised tensors, 23.5 M quantised elements."""

    def __init__(self, mode="nq", value=(1e-10, 1e-11), seed=42, orientation="channelwise", input_shape=(3, 224, 224),
                 num_classes=10, device=None):
        super().__init__()
        # mode "nqcl": value is (penalty_threshold, penalty_rate) for every layer, not a (coarse, fine) pair
        coarse, fine = (value if (isinstance(value, (tuple, list)) and mode != "nqcl") else (value, value))
        init = RandomNormal(seed=seed)
        self.stem = CustomConv2DLayer(seed=seed, orientation=orientation, initializer=init, filters=64, kernel_size=(7, 7),
                                      strides=(2, 2), padding="same", name="custom_conv2d_layer_64_0", regularizer=None,
                                      input_shape=input_shape[0], device=device, **_kw(mode, fine))
        self.bn0 = _bn(64)
        blocks = []
        ci = 64
        for stage, (width, n) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3))):
            for j in range(n):
                stride = (2, 2) if (j == 0 and stage > 0) else (1, 1)
                blocks.append(_BottleneckBlock(ci, width, stride, j == 0, j + 1, (fine, coarse, fine, fine), seed, orientation,
                                               device, mode))
                ci = 4 * width
        self.blocks = nn.ModuleList(blocks)
        self.out = CustomDenseLayer(seed=seed, units=num_classes, orientation="rowwise" if orientation == "channelwise" else orientation,
                                    initializer=init, name="custom_dense_layer_out", regularizer=None, input_shape=2048,
                                    device=device, **_kw(mode, fine))
        if device is not None:
            self.to(device)

    def forward(self, x):
        x = F.relu(self.bn0(self.stem(x)))
        h, w = x.shape[-2:]
        ph = max((-(-h // 2) - 1) * 2 + 3 - h, 0)
        pw = max((-(-w // 2) - 1) * 2 + 3 - w, 0)
        x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2), value=float("-inf"))
        x = F.max_pool2d(x, 3, 2)
        for b in self.blocks:
            x = b(x)
        return softmax(self.out(torch.mean(x, dim=(2, 3))), dim=1)


CLIP_MODES = ("cl", "ste", "stecl")


def check_clip_mode(mode: str) -> None:
    """A model with an integer range needs a mode without the nested-quantization vote."""
    if mode not in CLIP_MODES:
        raise ValueError(f"bits / q_range with mode {mode!r}: the nested-quantization vote is defined on the unclipped quantizer; "
                         f"a clipped model needs one of the modes {CLIP_MODES}")


GROUP_MODES = ("ste",)


def check_group_mode(mode: str, has_range: bool) -> None:
    """Group-wise scales need the clipped quantizer and a mode whose scale gradient is "ste" without a loss term."""
    if not has_range:
        raise ValueError("group_size needs bits / q_range: group-wise scales exist for the clipped quantizer only")
    if mode in ("cl", "stecl", "nqcl"):
        raise ValueError(f"group_size with mode {mode!r}: the loss-term penalty kernels broadcast one-axis scales; group-wise scales "
                         f"train with one of the modes {GROUP_MODES}")
    if mode not in GROUP_MODES:
        raise ValueError(f"group_size with mode {mode!r}: group-wise scales train with one of the modes {GROUP_MODES}")


def check_asymmetric_model(mode: str, has_range: bool, group_size, kernel_storage=None) -> None:
    """An asymmetric model needs group-wise scales, a range, mode "ste" and conv kernels in the convolution's memory order."""
    if group_size is None:
        raise ValueError("asymmetric=True needs group_size (orientation=\"groupwise\"): offsets exist per group; a group_size of the "
                         "line length or more gives per-channel offsets")
    if not has_range:
        raise ValueError("asymmetric=True needs bits / q_range: the offset places a chosen integer range over each group")
    if mode in ("cl", "stecl", "nqcl"):
        raise ValueError(f"asymmetric=True with mode {mode!r}: the loss-term penalty kernels know scales only, an offset would get no "
                         f"gradient from them; asymmetric layers train with one of the modes {GROUP_MODES}")
    if mode in ("nq",):
        raise ValueError(f"asymmetric=True with mode {mode!r}: the nested-quantization vote is defined on the unclipped symmetric "
                         f"quantizer; asymmetric layers train with one of the modes {GROUP_MODES}")
    if mode not in GROUP_MODES:
        raise ValueError(f"asymmetric=True with mode {mode!r}: asymmetric layers train with one of the modes {GROUP_MODES}")
    if kernel_storage == "hwio":
        raise ValueError('asymmetric=True with kernel_storage="hwio": the groups and their offsets are defined in the convolution\'s '
                         'memory order; store the kernel "oihw"')


MX_MODES = ("ste",)


def check_mx_model(mode: str, bits=None, signed=True, q_range=None, rounding="floor", asymmetric=False, kernel_storage=None,
                   scale_init=None) -> None:
    """A model with an element format trains in mode "ste", on conv kernels in the convolution's memory order, and takes neither an
    integer range, a rounding, offsets nor an integer scale initialisation."""
    from .ops import MX_SCALE_INITS
    if bits is not None or q_range is not None or not signed:
        raise ValueError("element_format with bits / q_range / signed: an element format brings its own grid, range and sign")
    if rounding != "floor":
        raise ValueError(f"element_format with rounding={rounding!r}: a minifloat grid rounds to nearest, ties to even, and nothing "
                         "else; leave rounding at its default")
    if asymmetric:
        raise ValueError("element_format with asymmetric=True: the microscaling formats are symmetric, a block has a scale and no offset")
    if mode in ("cl", "stecl", "nqcl"):
        raise ValueError(f"element_format with mode {mode!r}: the loss-term penalty kernels know the integer quantizer with one-axis "
                         f"scales only; a model with an element format trains with one of the modes {MX_MODES}")
    if mode == "nq":
        raise ValueError(f"element_format with mode {mode!r}: the nested-quantization vote is defined on the unclipped integer "
                         f"quantizer; a model with an element format trains with one of the modes {MX_MODES}")
    if mode not in MX_MODES:
        raise ValueError(f"element_format with mode {mode!r}: a model with an element format trains with one of the modes {MX_MODES}")
    if kernel_storage == "hwio":
        raise ValueError('element_format with kernel_storage="hwio": the blocks are defined in the convolution\'s memory order; store '
                         'the kernel "oihw"')
    if scale_init is not None and scale_init not in MX_SCALE_INITS:
        raise ValueError(f"scale_init {scale_init!r} on a model with an element format: a microscaling scale is a power of two, "
                         f"written by one of {MX_SCALE_INITS}")


def build_model(config: str, kernel_storage: str = None, grad_scale=None, bits=None, signed=True, q_range=None, rounding="floor",
                group_size=None, scale_init=None, asymmetric=False, element_format=None, scale_format="e8m0", **kw) -> nn.Module:
    """config: 'mnist' (C1), 'cifar' (C2/C4), 'imagenette' (C3), 'resnet50' (C5, extension).
    ``kernel_storage``: memory order of the conv kernels, "oihw" (default) or "hwio" (layers.py).
    ``grad_scale`` (modes "ste" / "stecl"): factor of every straight-through scale gradient, a float or "rsqrt_group".
    ``bits`` (1..24) with ``signed``, or ``q_range=(qmin, qmax)`` (modes "cl" / "ste" / "stecl"): the integer range of every
    quantised tensor, carried by the host layers and both of their nested layers.
    ``rounding`` ("floor" / "nearest"; "nearest" only with a range): how that quantizer rounds P/s, carried the same way.
    ``group_size`` (with a range, mode "ste"): every quantised kernel gets group-wise scales, one per ``group_size`` consecutive
    inputs of each output unit (layers.py ``orientation="groupwise"``; it replaces ``orientation``); biases keep a scalar scale.
    ``scale_init`` ("absmax" / "lsq" / "mse"; needs a range and ``device``): every scale starts from its weights
    (layers.init_scales) instead of the library's initial value, applied after the ranges and group sizes are in place.
    ``asymmetric`` (with ``group_size``, mode "ste"): every group-wise kernel also learns an offset per group (layers.py
    ``asymmetric=True``); biases stay symmetric.  ``scale_init="minmax"`` exists for such models only: scale and offset of every
    group from its minimum and maximum, biases by "absmax".
    ``element_format`` (one of ops.ELEMENT_FORMATS; mode "ste") with ``scale_format`` ("e8m0" / "fp32"): the OCP microscaling
    quantizer for every quantised tensor (layers.py ``element_format=``): kernels in blocks of ``group_size`` (32 by default),
    biases as one group.  It replaces ``orientation`` and takes no range, rounding or offsets; ``scale_init`` is "mx" or "cover"."""
    from .ops import check_rounding
    if element_format is not None:
        from .layers import _HostLayer, init_scales
        from .ops import check_element_format, check_scale_format
        check_element_format(element_format)
        check_scale_format(scale_format)
        check_mx_model(kw.get("mode", "nq"), bits, signed, q_range, rounding, asymmetric, kernel_storage, scale_init)
        model = build_model(config, kernel_storage=kernel_storage, grad_scale=grad_scale, **{**kw, "orientation": "scalar"})
        for m in model.modules():
            if isinstance(m, _HostLayer):
                m.make_mx(element_format, scale_format, group_size)
        return model if scale_init is None else init_scales(model, scale_init)
    if scale_init in ("mx", "cover"):
        raise ValueError(f"scale_init {scale_init!r} on a model without an element format: it writes the power-of-two scale of a "
                         "microscaling block")
    check_rounding(rounding, bits is not None or q_range is not None)
    if asymmetric:
        check_asymmetric_model(kw.get("mode", "nq"), bits is not None or q_range is not None, group_size, kernel_storage)
    if scale_init is not None:
        from .layers import init_scales
        from .ops import check_layer_scale_init, check_minmax_range, q_range_of
        check_layer_scale_init(scale_init)
        if bits is None and q_range is None:
            raise ValueError("scale_init needs bits / q_range: the unbounded quantizer clips nothing, there is no range to cover")
        if scale_init == "minmax":
            if not asymmetric:
                raise ValueError('scale_init "minmax" on a symmetric model: it places each group\'s range over [min, max] through an '
                                 "offset, which only asymmetric=True layers have")
            check_minmax_range(*q_range_of(bits, signed, q_range))
        model = build_model(config, kernel_storage=kernel_storage, grad_scale=grad_scale, bits=bits, signed=signed, q_range=q_range,
                            rounding=rounding, group_size=group_size, asymmetric=asymmetric, **kw)
        return init_scales(model, scale_init)
    if asymmetric:
        from .layers import _HostLayer
        model = build_model(config, kernel_storage=kernel_storage, grad_scale=grad_scale, bits=bits, signed=signed, q_range=q_range,
                            rounding=rounding, group_size=group_size, **kw)
        for m in model.modules():
            if isinstance(m, _HostLayer):
                m.make_asymmetric()
        return model
    if group_size is not None:
        from .layers import _HostLayer
        check_group_mode(kw.get("mode", "nq"), bits is not None or q_range is not None)
        model = build_model(config, kernel_storage=kernel_storage, grad_scale=grad_scale, bits=bits, signed=signed, q_range=q_range,
                            rounding=rounding, **{**kw, "orientation": "scalar"})
        for m in model.modules():
            if isinstance(m, _HostLayer):
                m.make_groupwise(group_size)
        return model
    if bits is not None or q_range is not None:
        from .layers import CustomQuantizedScaleLayer, _HostLayer
        from .ops import q_range_of
        rng = q_range_of(bits, signed, q_range)
        check_clip_mode(kw.get("mode", "nq"))
        model = build_model(config, kernel_storage=kernel_storage, grad_scale=grad_scale, **kw)
        for m in model.modules():
            if isinstance(m, (CustomQuantizedScaleLayer, _HostLayer)):
                m.q_range = rng
                m.rounding = rounding
        return model
    if grad_scale is not None:
        from .layers import CustomQuantizedScaleLayer
        model = build_model(config, kernel_storage=kernel_storage, **kw)
        for m in model.modules():
            if isinstance(m, CustomQuantizedScaleLayer):
                m.grad_scale = grad_scale if grad_scale == "rsqrt_group" else float(grad_scale)
        return model
    if kernel_storage is not None:
        from .layers import default_kernel_storage
        with default_kernel_storage(kernel_storage):
            return build_model(config, **kw)
    if config == "resnet50":
        return ResNet50Like(**kw)
    if config == "mnist":
        return MNISTDense(**kw)
    if config == "cifar":
        return CIFARCNN(**kw)
    if config == "imagenette":
        return ResNet18Like(**kw)
    raise ValueError(f"unknown config {config!r}")


INPUT_SHAPES = {"mnist": (1, 28, 28), "cifar": (3, 32, 32), "imagenette": (3, 224, 224), "resnet50": (3, 224, 224)}
