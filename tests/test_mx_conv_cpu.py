"""CPU tests of the im2col operand of a convolution (include/lq_hip.h: lq_mx_im2col_dims / lq_mx_operand_im2col) and of the conv
layers' path onto the block-scaled GEMM: the entry points, the output extents against F.conv2d, every refusal of the C surface (no
pointer is dereferenced: every call fails in validation) and of Python, eligibility, the NumPy reference itself (against F.unfold and
F.conv2d) and the conditions of the exact data sets tests/test_gpu_mx_conv.py runs on the device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _mx_conv_reference as C                                                                # noqa: E402
import _mx_gemm_reference as G                                                                # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ_EINVAL, LQ_EALIGN = -1, -4
FP4, FP6A, FP6B, E4M3, E5M2 = 0, 1, 2, 3, 4
_gid = C.geom_id


def _err():
    return _hip.load().lq_last_error().decode()


def _geom(B=2, Cc=3, H=5, W=5, xs=(75, 25, 5, 1), KH=3, KW=3, sh=1, sw=1, pads=(1, 1, 1, 1)):
    """pads: (top, left, bottom, right), the order of the struct."""
    return _hip.ConvGeom(B, Cc, H, W, *xs, KH, KW, sh, sw, *pads)


def test_entry_points_are_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    for fn in ("lq_mx_im2col_dims", "lq_mx_operand_im2col"):
        assert fn in declared and hasattr(lib, fn) and fn in _hip.SIGNATURES, fn
    assert "typedef struct lq_conv_geom" in header and ctypes.sizeof(_hip.ConvGeom) == 8 * 8 + 8 * 4
    assert len(_hip.SIGNATURES["lq_mx_operand_im2col"][1]) == 7 and len(_hip.SIGNATURES["lq_mx_im2col_dims"][1]) == 5
    assert lq.mx_operand_im2col is ops.mx_operand_im2col and lq.mx_im2col_dims is ops.mx_im2col_dims
    assert lq.mx_conv_eligible is L.mx_conv_eligible
    assert issubclass(ops.MxConvOperand, ops.MxOperand) and ops.MxOperand._fields == ("codes", "scales", "format", "lines", "K")


@pytest.mark.parametrize("g", C.GEOMS, ids=_gid)
def test_dims_are_those_of_conv2d(g):
    """ops.mx_im2col_dims against the reference's formulas, layers._same_padding and the shape F.conv2d gives the padded input."""
    top, bottom, left, right = C.padding_of(g)
    if g.padding == "SAME":
        assert (top, bottom) == L._same_padding(g.H, g.KH, g.sh) and (left, right) == L._same_padding(g.W, g.KW, g.sw)
    M, K, OH, OW = ops.mx_im2col_dims((g.B, g.C, g.H, g.W), (g.KH, g.KW), (g.sh, g.sw), (top, bottom, left, right))
    assert (M, K, OH, OW) == C.dims(g)
    y = F.conv2d(F.pad(torch.zeros(g.B, g.C, g.H, g.W), (left, right, top, bottom)), torch.zeros(1, g.C, g.KH, g.KW), None, (g.sh, g.sw))
    assert tuple(y.shape) == (g.B, 1, OH, OW) and M == g.B * OH * OW and K == g.C * g.KH * g.KW
    if g.padding == "SAME":
        assert (OH, OW) == (-(-g.H // g.sh), -(-g.W // g.sw))


def test_what_the_geometries_exercise():
    d = [C.dims(g) for g in C.GEOMS]
    assert d[0][:2] == (50, 27) and d[1][1] == 245 and C.padding_of(C.GEOMS[1])[2:] == (2, 3)
    assert d[2][:2] == (16, 576) and G.layout_dims(16, 576) == (1, 5, 2)
    assert C.padding_of(C.GEOMS[3]) == (0, 0, 0, 0) and d[4][1] == 160 and d[6][0] == 245
    assert ops.mx_im2col_dims((1 << 20, 64, 8, 8), 3, 1, (1, 1, 1, 1))[:2] == (1 << 26, 576)      # an M K the operand refuses


def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    im, dims = lib.lq_mx_operand_im2col, lib.lq_mx_im2col_dims
    o = [ctypes.c_int64(0) for _ in range(4)]
    refs = [ctypes.byref(v) for v in o]
    ok = _geom()
    assert dims(ctypes.byref(ok), *refs) == 0 and [v.value for v in o] == [50, 27, 5, 5]
    # null pointers
    assert dims(None, *refs) == LQ_EINVAL and "'g' is NULL" in _err()
    for k, name in enumerate(("M", "K", "OH", "OW")):
        args = list(refs)
        args[k] = None
        assert dims(ctypes.byref(ok), *args) == LQ_EINVAL and f"'{name}' is NULL" in _err()
    assert im(None, ctypes.byref(ok), E4M3, 0, p, p, None) == LQ_EINVAL and "'X' is NULL" in _err()
    assert im(p, None, E4M3, 0, p, p, None) == LQ_EINVAL and "'g' is NULL" in _err()
    assert im(p, ctypes.byref(ok), E4M3, 0, None, p, None) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert im(p, ctypes.byref(ok), E4M3, 0, p, None, None) == LQ_EINVAL and "'scales' is NULL" in _err()
    # the geometry, through both entry points
    for g, needle in ((_geom(B=0), "extents must be positive"), (_geom(Cc=-1), "extents must be positive"),
                      (_geom(H=0), "extents must be positive"), (_geom(W=0), "extents must be positive"),
                      (_geom(KH=0), "kernel size must be positive"), (_geom(KW=-3), "kernel size must be positive"),
                      (_geom(sh=0), "strides must be positive"), (_geom(sw=-1), "strides must be positive"),
                      (_geom(pads=(-1, 1, 1, 1)), "padding must not be negative"), (_geom(pads=(1, -1, 1, 1)), "padding must not be negative"),
                      (_geom(pads=(1, 1, -1, 1)), "padding must not be negative"), (_geom(pads=(1, 1, 1, -2)), "padding must not be negative"),
                      (_geom(KH=8), "does not fit the padded input (OH=0 OW=5)"), (_geom(KW=9), "does not fit the padded input (OH=5 OW=0)")):
        assert dims(ctypes.byref(g), *refs) == LQ_EINVAL and needle in _err(), needle
        assert im(p, ctypes.byref(g), E4M3, 0, p, p, None) == LQ_EINVAL and needle in _err(), needle
    # formats and methods
    for bad, needle in ((FP6A, "fp6 operands are not supported"), (FP6B, "fp6 operands are not supported"), (-1, "bad element format"),
                        (5, "bad element format")):
        assert im(p, ctypes.byref(ok), bad, 0, p, p, None) == LQ_EINVAL and needle in _err()
    for method in (-1, 2):
        assert im(p, ctypes.byref(ok), E4M3, method, p, p, None) == LQ_EINVAL and "bad method" in _err()
    # M * K >= 2^31: accepted by the dims call, refused by the operand
    big = _geom(B=1 << 20, Cc=64, H=8, W=8, xs=(4096, 64, 8, 1))
    assert dims(ctypes.byref(big), *refs) == 0 and o[0].value * o[1].value >= 1 << 31
    assert im(p, ctypes.byref(big), E4M3, 0, p, p, None) == LQ_EINVAL and "not below 2^31" in _err()
    # a negative stride of X
    for k in range(4):
        xs = [75, 25, 5, 1]
        xs[k] = -xs[k]
        assert im(p, ctypes.byref(_geom(xs=tuple(xs))), E4M3, 0, p, p, None) == LQ_EINVAL and "strides of X must not be negative" in _err()
    # alignment
    assert im(p, ctypes.byref(ok), FP4, 0, p + 4, p, None) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert im(p, ctypes.byref(ok), FP4, 0, p, p + 2, None) == LQ_EALIGN and "scales is not 4-byte aligned" in _err()
    assert im(p + 2, ctypes.byref(ok), FP4, 0, p, p, None) == LQ_EALIGN and "'X' is not 4-byte aligned" in _err()


def _conv(cls=L.CustomConv2DLayer, **kw):
    kw.setdefault("input_shape", 5)
    return cls(filters=8, kernel_size=(3, 3), initializer=L.RandomNormal(seed=1), **kw)


def test_refusals_of_the_python_surface():
    x = torch.zeros(2, 5, 6, 6)
    for name in ("fp6_e2m3", "fp6_e3m2"):
        with pytest.raises(ValueError, match="fp6 operands are not supported"):
            ops.mx_operand_im2col(x, 3, element_format=name)
    with pytest.raises(ValueError, match="must be one of"):
        ops.mx_operand_im2col(x, 3, method="absmax")
    with pytest.raises(ValueError, match="four axes"):
        ops.mx_operand_im2col(torch.zeros(5, 6, 6), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mx_operand_im2col(x, 3)
    with pytest.raises(ValueError, match="padding .* must be 4 integers"):
        ops.mx_im2col_dims(x.shape, 3, 1, (1, 1))
    with pytest.raises(_hip.LQError, match="padding must not be negative"):
        ops.mx_im2col_dims(x.shape, 3, 1, (0, -1, 0, 0))
    with pytest.raises(_hip.LQError, match="does not fit the padded input"):
        ops.mx_im2col_dims(x.shape, 7)
    # layers: the checks and messages of check_mx_operand_layer, hwio, an unbuilt layer
    for cls in (L.CustomConv2DLayer, L.CustomConv2DLayerNoBias):
        for kw, needle in ((dict(orientation="groupwise", group_size=32, bits=4, scale_gradient="ste"), "needs a layer with an element_format"),
                           (dict(), "needs a layer with an element_format"),
                           (dict(orientation="groupwise", element_format="fp4_e2m1", scale_format="fp32"), "E8M0"),
                           (dict(orientation="groupwise", element_format="fp6_e2m3"), "fp6 operands are not supported"),
                           (dict(orientation="groupwise", element_format="fp6_e3m2"), "fp6 operands are not supported"),
                           (dict(orientation="groupwise", element_format="fp8_e4m3", group_size=16), "group_size=16"),
                           (dict(orientation="groupwise", element_format="fp8_e4m3", group_size=64), "group_size=64")):
            c = _conv(cls, **kw)
            with pytest.raises(ValueError, match=re.escape(needle)):
                c.mx_operand()
            with pytest.raises(ValueError, match=re.escape(needle)):
                c.call_mx(x)
            assert not L.mx_conv_eligible(c) and not L.mx_hardware_eligible(c)
        c = _conv(cls, orientation="groupwise", element_format="fp4_e2m1")
        c.kernel_storage = "hwio"                          # an MX layer cannot be built hwio: the refusal guards the attribute
        with pytest.raises(ValueError, match='kernel_storage="hwio"'):
            c.mx_operand()
        with pytest.raises(ValueError, match='kernel_storage="hwio"'):
            c.call_mx(x)
        assert not L.mx_conv_eligible(c)
        c = _conv(cls, orientation="groupwise", element_format="fp4_e2m1", input_shape=None)
        assert not c.built and not L.mx_conv_eligible(c)
        with pytest.raises(ValueError, match="not built yet"):
            c.mx_operand()
        c = _conv(cls, orientation="groupwise", element_format="fp4_e2m1")
        for kw, needle in ((dict(act_format="fp6_e2m3"), "fp6 operands"), (dict(act_scale="absmax"), "must be one of"),
                           (dict(max_lines=0), "max_lines"), (dict(max_lines=2.5), "max_lines")):
            with pytest.raises(ValueError, match=re.escape(needle)):
                c.call_mx(x, **kw)


def test_eligibility():
    for cls in (L.CustomConv2DLayer, L.CustomConv2DLayerNoBias):
        for name in G.OPERAND_FORMATS:
            c = _conv(cls, orientation="groupwise", element_format=name)
            assert L.mx_conv_eligible(c) and not L.mx_hardware_eligible(c)
    d = L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), input_shape=70, orientation="groupwise", element_format="fp4_e2m1")
    assert L.mx_hardware_eligible(d) and not L.mx_conv_eligible(d)
    assert "no implicit GEMM is built" in L.mx_hardware_eligible.__doc__
    m = lq.build_model("cifar", mode="ste", value=0.0, element_format="fp4_e2m1")
    assert sum(L.mx_conv_eligible(c) for c in L.custom_layers_of(m)) == 6 and not any(L.mx_hardware_eligible(c) for c in L.custom_layers_of(m))
    hw = L.mx_hardware(m)
    assert hw.convs is False and L.mx_hardware(m, convs=True).convs is True


def test_driver_refusal(capsys):
    from learned_quantization_amd import train
    with pytest.raises(SystemExit):
        train.main(["--config", "cifar", "--mode", "ste", "--element-format", "fp4_e2m1", "--mx-eval-convs"])
    assert "--mx-eval-convs needs --mx-eval" in capsys.readouterr().err


# ----------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("g", C.GEOMS, ids=_gid)
def test_im2col_is_unfold_and_conv2d(g):
    """im2col equals F.unfold(F.pad(x)) transposed, and on small-integer data F.conv2d in float64 equals im2col(x) @ w.reshape(co, -1).T
    exactly: the order (c, i, j) is pinned against torch's own convolution."""
    top, bottom, left, right = C.padding_of(g)
    M, K, OH, OW = C.dims(g)
    x = C.gaussian_input(g)
    A = C.im2col(x, g)
    assert A.shape == (M, K) and A.dtype == np.float32
    u = F.unfold(F.pad(torch.from_numpy(x), (left, right, top, bottom)), (g.KH, g.KW), stride=(g.sh, g.sw))      # (B, K, OH OW)
    assert np.array_equal(A, u.transpose(1, 2).reshape(M, K).numpy())
    rng = np.random.default_rng(G.stable_seed("mx-conv-int", tuple(g)))
    xi = rng.integers(-4, 5, size=(g.B, g.C, g.H, g.W)).astype(np.float64)
    w = rng.integers(-4, 5, size=(7, g.C, g.KH, g.KW)).astype(np.float64)
    y = F.conv2d(F.pad(torch.from_numpy(xi), (left, right, top, bottom)), torch.from_numpy(w), None, (g.sh, g.sw)).numpy()
    got = (C.im2col(xi, g) @ w.reshape(7, -1).T).reshape(g.B, OH, OW, 7).transpose(0, 3, 1, 2)
    assert np.array_equal(got, y)


def test_windows_covering_counts_taps():
    g = C.GEOMS[0]                                         # 3 x 3, stride 1, pad 1 on 5 x 5: an inner pixel lies in 9 windows, a corner in 4
    assert C.windows_covering(g, 1, 2, 2, 2).sum() == 9 and C.windows_covering(g, 0, 0, 0, 0).sum() == 4
    cover = C.windows_covering(g, 1, 2, 2, 2)
    assert cover.shape == (50, 1) and not cover[:25].any()
    g = C.GEOMS[2]                                         # K = 576: channel 10 is k = 90 .. 98, blocks 2 and 3
    cover = C.windows_covering(g, 0, 10, 1, 1)
    assert cover.shape == (16, 18) and set(np.flatnonzero(cover.any(axis=0))) == {2, 3}


# ----------------------------------------------------------------------------------- the exact-data condition used on the GPU
@pytest.mark.parametrize("g", C.EXACT_GEOMS, ids=_gid)
def test_exact_sets_are_exact_in_every_format(g):
    """Activations and kernels drawn from G.EXACT_VALUES: under the scale either rule takes from a block the reference operand
    decodes to A bit for bit in every format, the kernel under unit E8M0 scales decodes to itself, and every float32 partial sum
    of an output is exact: the convolution in float64 is a float32, so the device's result can be held to it bit for bit."""
    co = 24
    x = C.exact_input(g)
    k, bias = C.exact_kernel(g, co)
    A, Wm = C.im2col(x, g), C.kernel_matrix(k)
    assert (A == 0).any() and set(np.unique(A)) <= set(G.EXACT_VALUES.tolist())
    for name in G.OPERAND_FORMATS:
        for method in C.METHODS:
            op, _ = G.operand_of_activation(A, name, method)
            assert np.array_equal(G.decode(op), A.astype(np.float64)), (name, method)
            assert op.bytes.min() >= 1 and op.bytes.max() <= 254
        nb = -(-Wm.shape[1] // 32)
        wop = G.operand_of_parameter(Wm, np.ones((co, nb), np.float32), name, 1)
        assert np.array_equal(G.decode(wop), Wm.astype(np.float64)) and (wop.bytes == 127).all()
    terms = A.astype(np.float64)[:, None, :] * Wm.astype(np.float64)[None, :, :]
    assert np.array_equal(terms * 4, np.round(terms * 4)) and np.abs(terms).max() <= 4.0      # multiples of 1/4, sums below 2^12
    ref = terms.sum(axis=-1) + bias.astype(np.float64)[None, :]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.abs(terms).sum(axis=-1).max() < 2.0 ** 12
    top, bottom, left, right = C.padding_of(g)
    w_oihw = torch.from_numpy(np.ascontiguousarray(k.transpose(3, 2, 0, 1)).astype(np.float64))
    y = F.conv2d(F.pad(torch.from_numpy(x.astype(np.float64)), (left, right, top, bottom)), w_oihw, torch.from_numpy(bias.astype(np.float64)),
                 (g.sh, g.sw)).numpy()
    M, K, OH, OW = C.dims(g)
    assert np.array_equal(y, ref.reshape(g.B, OH, OW, co).transpose(0, 3, 1, 2))
