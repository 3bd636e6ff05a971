"""CPU tests of the stem convolution: the reference pinned on one hand-written case, the six names in the header and the binding
table, the refusals of the C surface (every call fails in validation) and of the Python surface, and the options' defaults."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_stem_reference as S                                                                # noqa: E402
from test_i8_direct_cpu import LQ_EALIGN, LQ_EINVAL, P, _g                                    # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, train                                 # noqa: E402

NAMES = ["lq_i8_rows_bytes", "lq_i8_rows_quantize", "lq_i8_stem_kernel_bytes", "lq_i8_stem_kernel_pack", "lq_i8_stem_conv2d",
         "lq_i8_stem_conv2d_quantize"]


def test_reference_on_a_hand_written_case():
    """One image of one channel, rows [1, 2, 127] and [-4, 0, 2], a 2 x 2 kernel [[1, 2], [3, -1]], VALID.  Row scales: 1 + 2^-22 and
    RN(RN(4 / 127) (1 + 2^-22)); codes [1, 2, 127] and [-127, 0, 63] (the margin puts 2 / s1 just below 63.5).  Row sums: (5, 256)
    and (-381, -63); y = RN(RN(I0 s0) + RN(I1 s1)) sk."""
    x = np.array([[[[1, 2, 127], [-4, 0, 2]]]], np.float32)
    rows = S.rows_of(x)
    f = np.float32
    s0, s1 = f(1.0) + f(2.0 ** -22), f(f(4.0) / f(127.0)) * (f(1.0) + f(2.0 ** -22))
    assert rows["scales"].tolist() == [[s0, s1]] and rows["codes"][0, :, :, 0].tolist() == [[1, 2, 127], [-127, 0, 63]]
    assert not rows["codes"][..., 1:].any()
    q = np.array([[[[1, 2], [3, -1]]]], np.int8)
    y = S.conv_reference(rows, q, np.array([0.5], f), None, (1, 1), (0, 0, 0, 0))
    want = [(f(f(5) * s0) + f(f(-381) * s1)) * f(0.5), (f(f(256) * s0) + f(f(-63) * s1)) * f(0.5)]
    assert y.dtype == f and y.reshape(-1).tolist() == want
    buf, scales = S.pack_kernel(q, np.array([0.5], f))
    frag = buf.view(np.int8).reshape(1, 2, 64, 8)
    assert frag[0, :, 0].tolist() == [[1, 0, 0, 0, 2, 0, 0, 0], [3, 0, 0, 0, -1, 0, 0, 0]] and not frag[0, :, 1:].any()
    assert scales.tolist() == [0.5] + [1.0] * 15


def test_header_and_binding_table_hold_the_six_names():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "lq_hip.h")).read()
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    for name in NAMES:
        assert re.search(rf"^int {name}\(", header, re.M) and name in _hip.SIGNATURES and hasattr(lib, name)


def _conv(rc=P, rs=P, kc=P, ks=P, bias=None, Y=P, ldy=None, g=None, co=10):
    return "lq_i8_stem_conv2d", (rc, rs, kc, ks, bias, Y, co if ldy is None else ldy, ctypes.byref(g or _s()), co, None)


def _quant(g=None, co=10, act=0, first=0, post_scale=None, post_shift=None, oc=P):
    return "lq_i8_stem_conv2d_quantize", (P, P, P, P, None, ctypes.byref(g or _s()), co, post_scale, post_shift, act, first, oc, P, None)


_s = lambda **kw: _g(**{"C": 3, "xs": (105, 35, 7, 1), **kw})                                 # noqa: E731
_rows = lambda X=P, g=None, codes=P, scales=P: ("lq_i8_rows_quantize", (X, ctypes.byref(g or _s()), codes, scales, None))      # noqa: E731
_pack = lambda ext=(10, 3, 3, 3), lo=-128, hi=127, rnd=0, codes=P: ("lq_i8_stem_kernel_pack", (P, P, lo, hi, rnd, *ext, codes, P, None))  # noqa: E731
REFUSALS = [
    (_rows(g=_s(C=5)), LQ_EINVAL, "C = 5 channels is above 4"), (_rows(g=_s(B=0)), LQ_EINVAL, "extents must be positive"),
    (_rows(g=_s(xs=(105, -35, 7, 1))), LQ_EINVAL, "must not be negative"), (_rows(X=None), LQ_EINVAL, "is NULL"),
    (_rows(g=_s(B=1 << 20, H=1 << 5, W=1 << 4)), LQ_EINVAL, "are not below 2^31"), (_rows(codes=P + 4), LQ_EALIGN, "16-byte aligned"),
    (_pack(ext=(10, 5, 3, 3)), LQ_EINVAL, "ci = 5 channels is above 4"), (_pack(ext=(10, 3, 3, 9)), LQ_EINVAL, "KW = 9 is above 8"),
    (_pack(ext=(10, 3, 17, 3)), LQ_EINVAL, "KH = 17 is above 16"), (_pack(ext=(0, 3, 3, 3)), LQ_EINVAL, "extents must be positive"),
    (_pack(hi=128), LQ_EINVAL, "not inside [-128, 127]"), (_pack(rnd=7), LQ_EINVAL, "rounding"), (_pack(codes=None), LQ_EINVAL, "is NULL"),
    (_conv(g=_s(C=5)), LQ_EINVAL, "C = 5 channels is above 4"), (_conv(g=_s(W=12, KW=9)), LQ_EINVAL, "KW = 9 is above 8"),
    (_conv(g=_s(sh=0)), LQ_EINVAL, "strides must be positive"), (_conv(g=_s(KH=8)), LQ_EINVAL, "does not fit the padded input"),
    (_conv(rc=None), LQ_EINVAL, "is NULL"), (_conv(Y=None), LQ_EINVAL, "is NULL"), (_conv(ldy=9), LQ_EINVAL, "ldy = 9 is below N = 10"),
    (_conv(g=_s(B=65536, H=9, W=9, pads=(0, 0, 0, 0), KH=1, KW=1)), LQ_EINVAL, "above 65535 * 64"), (_conv(ks=P + 4), LQ_EALIGN, "16-byte aligned"),
    (_quant(co=129), LQ_EINVAL, "co = 129 is above 128"), (_quant(g=_s(C=5)), LQ_EINVAL, "C = 5 channels is above 4"),
    (_quant(act=2), LQ_EINVAL, "bad activation 2"), (_quant(first=2), LQ_EINVAL, "affine_first"),
    (_quant(post_scale=P), LQ_EINVAL, "both be given or both be NULL"), (_quant(oc=None), LQ_EINVAL, "is NULL"),
    (_quant(post_scale=P + 2, post_shift=P), LQ_EALIGN, "post_scale or post_shift")]


@pytest.mark.parametrize("call,rc,why", REFUSALS, ids=[f"{k}-{c[0][0][6:]}" for k, c in enumerate(REFUSALS)])
def test_refusals_of_the_c_surface(call, rc, why):
    lib = _hip.load()
    assert getattr(lib, call[0])(*call[1]) == rc and why in lib.lq_last_error().decode()


def test_python_refusals_and_defaults():
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8, orientation="scalar").eval()
    assert L.i8_stem_eligible(m.convs[0]) and L._takes_stem(m.convs[0]) and not L.i8_stem_eligible(m.convs[1]) and not L._takes_stem(m.convs[1])
    with pytest.raises(ValueError, match="32 input channels: the stem convolution takes at most 4"):
        m.convs[1].i8_stem_operand()
    with pytest.raises(ValueError, match="takes no epilogue"):
        m.convs[0].call_i8_stem(torch.zeros(1, 3, 8, 8), activation="relu")
    x, chain = torch.zeros(1, 32, 8, 8), [(m.convs[1], None, None, False)]
    with pytest.raises(ValueError, match="stem=True: .*at most 4"):
        L.i8_conv_chain(x, chain, stem=True)
    with pytest.raises(ValueError, match="needs convs=True and direct=True"):
        L.i8_hardware(m, convs=True, stem_convs=True)
    with pytest.raises(ValueError, match="emulate=True with stem_convs=True"):
        L.i8_hardware(m, convs=True, direct=True, emulate=True, stem_convs=True)
    hw = L.i8_hardware(m, convs=True, direct=True)
    assert hw.stem_convs is False and hw.stem_layers == [] and m.convs[0]._i8_stem_hw is None
    assert inspect.signature(L.i8_conv_chain).parameters["stem"].default is False
    assert inspect.signature(train.i8_eval).parameters["stem_convs"].default is False
    assert train.build_parser().parse_args([]).i8_eval_stem_convs is False
