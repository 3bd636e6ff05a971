"""CPU tests of the direct int8 convolution: every refusal of the C surface (every call fails in validation) and of the layers,
tests/_i8_direct_reference.py against a float64 convolution of the decoded operands, and sa == 1.0 of the exact GPU inputs."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_direct_reference as D                                                              # noqa: E402
from _bounds import assert_within_terms                                                       # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

LQ_EINVAL, LQ_EALIGN = -1, -4
_BUF = (ctypes.c_float * 64)()
P = (ctypes.addressof(_BUF) + 15) & ~15                   # 16-byte aligned; never dereferenced: every call fails in validation


def _g(B=2, C=32, H=5, W=7, xs=(1120, 35, 7, 1), KH=3, KW=3, sh=1, sw=1, pads=(1, 1, 1, 1)):      # pads: (top, left, bottom, right)
    return _hip.ConvGeom(B, C, H, W, *xs, KH, KW, sh, sw, *pads)


_ref = lambda g: None if g is False else ctypes.byref(g or _g())                              # noqa: E731
_px = lambda X=P, g=None, codes=P, scales=P: ("lq_i8_pixels_quantize", (X, _ref(g), codes, scales, None))      # noqa: E731
_pk = lambda Pk=P, s=P, lo=-128, hi=127, rnd=0, ext=(10, 32, 3, 3), codes=P, scales=P: ("lq_i8_conv_kernel_pack", (Pk, s, lo, hi, rnd, *ext, codes, scales, None))  # noqa: E731
_cv = lambda pc=P, ps=P, kc=P, ks=P, bias=None, Y=P, ldy=10, g=None, co=10: ("lq_i8_conv2d", (pc, ps, kc, ks, bias, Y, ldy, _ref(g), co, None))  # noqa: E731

_GEOMETRY = [(dict(B=0), "extents must be positive"), (dict(C=-1), "extents must be positive"), (dict(H=0), "extents must be positive"), (dict(W=0), "extents must be positive"),
             (dict(C=65537), "above 65536"), (dict(B=1 << 20, H=64, W=64), "not below 2^31")]
_WINDOW = [(dict(KW=-3), "kernel size must be positive"), (dict(sh=0), "strides must be positive"), (dict(pads=(1, 1, 1, -2)), "padding must not be negative"),
           (dict(KH=8), "does not fit the padded input (OH=0 OW=7)"), (dict(KW=10), "does not fit the padded input (OH=5 OW=0)"),
           (dict(B=65536, H=9, W=9, pads=(0, 0, 0, 0), KH=1, KW=1), "above 65535 * 64"), (dict(pads=((1 << 31) - 4, 1, 1, 1), sh=1 << 30), "does not fit 32 bits")]
REFUSALS = (
    [(_px(**{k: None}), LQ_EINVAL, "is NULL") for k in ("X", "codes", "scales")] + [(_px(g=False), LQ_EINVAL, "'g' is NULL")]
    + [(_pk(**{k: None}), LQ_EINVAL, "is NULL") for k in ("Pk", "s", "codes", "scales")]
    + [(_cv(**{k: None}), LQ_EINVAL, "is NULL") for k in ("pc", "ps", "kc", "ks", "Y")] + [(_cv(g=False), LQ_EINVAL, "'g' is NULL")]
    + [(f(g=_g(**kw)), LQ_EINVAL, why) for kw, why in _GEOMETRY for f in (_px, _cv)] + [(_cv(g=_g(**kw)), LQ_EINVAL, why) for kw, why in _WINDOW]
    + [(_px(g=_g(xs=tuple(-v if k == n else v for n, v in enumerate((1120, 35, 7, 1))))), LQ_EINVAL, "strides of X must not be negative") for k in range(4)]
    + [(_cv(ldy=9), LQ_EINVAL, "ldy = 9 is below N = 10"), (_cv(co=0), LQ_EINVAL, "extents must be positive")]
    + [(_pk(ext=e), LQ_EINVAL, why) for e, why in (((0, 32, 3, 3), "extents must be positive"), ((10, 32, 3, -1), "kernel size must be positive"),
                                                   ((10, 65537, 3, 3), "above 65536"), ((1 << 20, 64, 7, 7), "not below 2^31"))]
    + [(_pk(lo=lo, hi=hi), LQ_EINVAL, "not inside [-128, 127]") for lo, hi in ((-129, 127), (-128, 128), (0, 255))]
    + [(_pk(lo=5, hi=-5), LQ_EINVAL, "qmin"), (_pk(rnd=7), LQ_EINVAL, "bad rounding")]
    + [(_px(X=P + 2), LQ_EALIGN, "4-byte aligned"), (_pk(Pk=P + 2), LQ_EALIGN, "4-byte aligned"), (_pk(s=P + 1), LQ_EALIGN, "4-byte aligned"),
       (_cv(bias=P + 2), LQ_EALIGN, "bias"), (_cv(Y=P + 2), LQ_EALIGN, "4-byte aligned")]
    + [(f(**{k: P + 4}), LQ_EALIGN, "16-byte aligned") for f, ks in ((_px, ("codes", "scales")), (_pk, ("codes", "scales")), (_cv, ("pc", "ps", "kc", "ks")))
       for k in ks])


@pytest.mark.parametrize("call,rc,why", REFUSALS, ids=[f"{c[0]}-{k}" for k, (c, _, _) in enumerate(REFUSALS)])
def test_refusals_of_the_c_surface(call, rc, why):
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    assert getattr(lib, call[0])(*call[1]) == rc and why in lib.lq_last_error().decode()


def _conv(cls=L.CustomConv2DLayer, **kw):
    kw.setdefault("input_shape", 32)
    return cls(filters=8, kernel_size=(3, 3), initializer=L.RandomNormal(seed=1), scale_gradient="ste", **kw)


@pytest.mark.parametrize("cls", [L.CustomConv2DLayer, L.CustomConv2DLayerNoBias], ids=["bias", "nobias"])
@pytest.mark.parametrize("kw,needle", [
    (dict(bits=8, orientation="scalar"), None), (dict(bits=4, orientation="groupwise", group_size=288), None),
    (dict(bits=4, orientation="groupwise", group_size=300), None), (dict(bits=4, orientation="groupwise", group_size=64), "one scale per filter"),
    (dict(bits=4, orientation="groupwise", group_size=64, asymmetric=True), "asymmetric=True"),
    (dict(bits=8, orientation="channelwise"), 'orientation="channelwise"'), (dict(bits=8, orientation="scalar", kernel_storage="hwio"), 'kernel_storage="hwio"'),
    (dict(bits=8, signed=False, orientation="scalar"), "not inside [-128, 127]"), (dict(bits=8, orientation="scalar", input_shape=None), "not built yet")])
def test_layer_eligibility_and_refusals(cls, kw, needle):
    """An eligible layer passes every check and fails at the first launch; every other names its reason."""
    c, x = _conv(cls, **kw), torch.zeros(2, 32, 6, 6)
    assert L.i8_direct_eligible(c) == (needle is None)
    with pytest.raises(RuntimeError if needle is None else ValueError, match=re.escape(needle or "no CPU fallback")):
        c.call_i8_direct(x) if c.built else c.i8_direct_operand()
    with pytest.raises(ValueError, match="max_lines"):
        c.call_i8_direct(x, max_lines=0)


def test_model_rule_sizes_and_operand_checks():
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8, orientation="scalar")
    assert [L.i8_direct_eligible(c) for c in m.convs] == [True] * 6 and [L._takes_direct(c) for c in m.convs] == [False] + [True] * 5
    assert L.i8_hardware(m).direct is False and L.i8_hardware(m, convs=True, direct=True).direct is True
    pix = ops.I8Pixels(torch.zeros(2, 6, 6, 32, dtype=torch.uint8), torch.zeros(2, 6, 5), (2, 32, 6, 6))      # a scale buffer too short
    with pytest.raises(ValueError, match="pixels.scales must be a contiguous"):
        ops.i8_conv2d(pix, ops.I8ConvKernel(torch.zeros(16 * 9 * 32, dtype=torch.uint8), torch.zeros(16), 8, 32, (3, 3)))


@pytest.mark.parametrize("g", D.GEOMS)
def test_reference_is_a_float64_convolution_of_the_decoded_operands(g):
    """1e-5 * sum|terms| covers the at most KH KW + 2 <= 51 roundings of 2^-24 relative (3.1e-6) of the definition."""
    pix, q, sk, bias = D.conv_case(g)
    top, bottom, left, right = D.padding_of(g)
    x = torch.from_numpy((pix["codes"][..., :g[1]].astype(np.float64) * pix["scales"].astype(np.float64)[..., None]).transpose(0, 3, 1, 2).copy())
    w, b = torch.from_numpy(q.astype(np.float64) * sk.astype(np.float64)[:, None, None, None]), torch.from_numpy(bias.astype(np.float64))
    ref = F.conv2d(F.pad(x, (left, right, top, bottom)), w, b, g[7]).permute(0, 2, 3, 1).reshape(-1, g[4])
    terms = F.conv2d(F.pad(x.abs(), (left, right, top, bottom)), w.abs(), b.abs(), g[7]).permute(0, 2, 3, 1).reshape(-1, g[4])
    assert_within_terms(D.conv_reference(pix, q, sk, bias, g[7], D.padding_of(g)), ref.numpy(), terms.numpy(), str(g))
    assert g not in D.EXACT or (D.pixels_of(D.exact_case(g)[0])["scales"] == np.float32(1.0)).all(), "the exact GPU inputs: sa == 1.0"
