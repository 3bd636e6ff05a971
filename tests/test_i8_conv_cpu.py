"""CPU tests of the int8 im2col operand of a convolution (include/lq_hip.h: lq_i8_operand_im2col) and of the conv layers' path onto
the int8 GEMM: the entry point, the reference's im2col against F.unfold for the geometries the int8 tests add, every refusal of
the C surface (no pointer is dereferenced: every call fails in validation) and of Python, eligibility, the proof that the case
table reaches every branch of the launch rule (tests/_i8_conv_forms.py), and the conditions of the inputs
tests/test_gpu_i8_conv.py runs on the device, asserted on the reference alone."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_forms as FM                                                                   # noqa: E402
import _i8_conv_reference as R                                                                # noqa: E402
import _i8_reference as I                                                                     # noqa: E402
import _mx_conv_reference as C                                                                # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ_EINVAL, LQ_EALIGN = -1, -4
_gid = C.geom_id
NEW_GEOMS = [R.LONG_ROW, R.CHUNKED, R.PADDING_ONLY]


def _err():
    return _hip.load().lq_last_error().decode()


def _geom(B=2, Cc=3, H=5, W=5, xs=(75, 25, 5, 1), KH=3, KW=3, sh=1, sw=1, pads=(1, 1, 1, 1)):
    """pads: (top, left, bottom, right), the order of the struct."""
    return _hip.ConvGeom(B, Cc, H, W, *xs, KH, KW, sh, sw, *pads)


def test_entry_point_is_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                          # an addition only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    fn = "lq_i8_operand_im2col"
    assert fn in declared and hasattr(lib, fn) and fn in _hip.SIGNATURES and len(_hip.SIGNATURES[fn][1]) == 6
    assert len(re.findall(r"\bint lq_\w*im2col_dims\s*\(", header)) == 1, "one dims function serves every format"
    assert lq.i8_operand_im2col is ops.i8_operand_im2col and lq.i8_conv_eligible is L.i8_conv_eligible
    assert lq.check_i8_conv_operand_layer is ops.check_i8_conv_operand_layer
    assert issubclass(ops.I8ConvOperand, ops.I8Operand) and ops.I8Operand._fields == ("codes", "scales", "lines", "K", "block")
    for doc in (header, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()):
        assert "Not built: conv layers" not in doc


# ----------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("g", NEW_GEOMS, ids=_gid)
def test_im2col_and_dims_are_unfold(g):
    top, bottom, left, right = C.padding_of(g)
    M, K, OH, OW = C.dims(g)
    assert ops.mx_im2col_dims((g.B, g.C, g.H, g.W), (g.KH, g.KW), (g.sh, g.sw), (top, bottom, left, right)) == (M, K, OH, OW)
    x = R.gaussian_input(g)
    A = C.im2col(x, g)
    u = F.unfold(F.pad(torch.from_numpy(x), (left, right, top, bottom)), (g.KH, g.KW), stride=(g.sh, g.sw))      # (B, K, OH OW)
    assert A.shape == (M, K) and np.array_equal(A, u.transpose(1, 2).reshape(M, K).numpy())


def test_what_the_geometries_exercise():
    assert [C.dims(g)[:2] for g in NEW_GEOMS] == [(16, 1152), (294, 36), (72, 80)]
    assert [C.dims(g)[1] for g in C.GEOMS] == [27, 245, 576, 360, 160, 18, 36]
    assert len(R.CASES) == 30 and len(set(R.CASES)) == 30
    assert FM.i8_im2col_form(R.PADDING_ONLY, 0)["padded_windows"] == 2 * (36 - 16)
    assert ops.i8_operand_bytes(16, 1152, 128) == (18 * 1024, 9 * 64)


def test_windows_covering_counts_taps():
    g = C.GEOMS[0]                                         # 3 x 3, stride 1, pad 1 on 5 x 5: an inner pixel lies in 9 windows, a corner in 4
    for block in R.BLOCKS:                                 # K = 27: one scale block whatever the block
        assert R.windows_covering(g, block, 1, 2, 2, 2).shape == (50, 1)
        assert R.windows_covering(g, block, 1, 2, 2, 2).sum() == 9 and R.windows_covering(g, block, 0, 0, 0, 0).sum() == 4
    g = C.GEOMS[2]                                         # K = 576: channel 10 is k = 90 .. 98
    assert set(np.flatnonzero(R.windows_covering(g, 64, 0, 10, 1, 1).any(axis=0))) == {1}
    assert set(np.flatnonzero(R.windows_covering(g, 128, 0, 14, 1, 1).any(axis=0))) == {0, 1}       # k = 126 .. 134
    assert R.windows_covering(g, 0, 0, 10, 1, 1).shape == (16, 1)
    # with blocks of 32 it is the MX helper
    assert np.array_equal(R.windows_covering(g, 64, 0, 10, 1, 1), C.windows_covering(g, 0, 10, 1, 1).reshape(16, 9, 2).any(axis=2))


# ------------------------------------------------------------------------------------------------------------ the launch forms
def test_the_table_reaches_every_branch():
    forms = {case: FM.i8_im2col_form(*case) for case in FM.FORMS}
    f = list(forms.values())
    assert {d["S"] for d in f} == {1, FM.SLICES}
    # both sides of the one threshold: the longest plain span and the shortest split one
    assert {d["units"] for d in f if d["S"] == 1} == {FM.CACHE} and min(d["units"] for d in f if d["S"] == FM.SLICES) == 2 * FM.CACHE
    for S in (1, FM.SLICES):
        mine = [d for d in f if d["S"] == S]
        blocks = [b for d in mine for b in d["blocks_of_k"]]
        assert any(d["chunks"] > 1 for d in mine) and any(d["chunks"] == 1 for d in mine), S
        assert any(d["idle_threads"] > 0 for d in mine) and any(d["dead_lines"] > 0 for d in mine) and any(d["dead_lines"] == 0 for d in mine), S
        assert any(d["nbs"] > 1 for d in mine) and any(d["nbs"] == 1 for d in mine), S
        assert any(b["ragged"] for b in blocks) and any(not b["ragged"] for b in blocks), S
        assert any(b["written"] > b["read"] for b in blocks), f"S = {S}: the k padding of a last block"
        assert any(not b["last"] for b in blocks), S
        assert any(d["padded_windows"] for d in mine) and any(d["j_wrap"] and d["i_wrap"] for d in mine), S
    plain = [b for d in f if d["S"] == 1 for b in d["blocks_of_k"]]
    assert not any(b["tail_read"] or b["tail_write"] for b in plain), "the plain form holds its whole span in registers"
    split = [b for d in f if d["S"] == FM.SLICES for b in d["blocks_of_k"]]
    assert any(b["tail_read"] for b in split) and any(not b["tail_write"] for b in split)        # past the register cache and inside it
    assert any(b["idle_slices"] for b in split), "a span of fewer units than slices"
    # the rows the int8 tests add: the long row, chunks of lines past 245, padded windows in either form
    old = [FM.i8_im2col_form(g, b) for g in C.GEOMS for b in R.BLOCKS]
    assert not any(d["padded_windows"] for d in old) and max(d["chunks"] for d in old if d["S"] == 1) == 1
    assert forms[(R.LONG_ROW, 0)]["blocks_of_k"][0]["read"] == 72 and forms[(R.LONG_ROW, 128)]["nbs"] == 9
    assert forms[(R.CHUNKED, 0)]["chunks"] == 2 and forms[(R.CHUNKED, 0)]["S"] == 1 and forms[(R.CHUNKED, 128)]["S"] == 1


def test_the_form_is_the_host_rule_text():
    """The constants of the restated rule are those of the source."""
    src = open(os.path.join(ROOT, "learned_quantization_amd", "csrc", "lq_kernels.hip")).read()
    hdr = open(os.path.join(ROOT, "learned_quantization_amd", "csrc", "lq_i8_conv.hpp")).read()
    assert "return units > kI8ConvCache ? kI8ConvSlices : 1;" in src
    assert f"kI8ConvUnit = {FM.UNIT};" in hdr and f"kI8ConvCache = {FM.CACHE};" in hdr and f"kI8ConvSlices = {FM.SLICES};" in hdr


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    im = lib.lq_i8_operand_im2col
    ok = _geom()
    assert im(None, ctypes.byref(ok), 0, p, p, None) == LQ_EINVAL and "'X' is NULL" in _err()
    assert im(p, None, 0, p, p, None) == LQ_EINVAL and "'g' is NULL" in _err()
    assert im(p, ctypes.byref(ok), 0, None, p, None) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert im(p, ctypes.byref(ok), 0, p, None, None) == LQ_EINVAL and "'scales' is NULL" in _err()
    for g, needle in ((_geom(B=0), "extents must be positive"), (_geom(Cc=-1), "extents must be positive"),
                      (_geom(H=0), "extents must be positive"), (_geom(W=0), "extents must be positive"),
                      (_geom(KH=0), "kernel size must be positive"), (_geom(KW=-3), "kernel size must be positive"),
                      (_geom(sh=0), "strides must be positive"), (_geom(sw=-1), "strides must be positive"),
                      (_geom(pads=(-1, 1, 1, 1)), "padding must not be negative"), (_geom(pads=(1, -1, 1, 1)), "padding must not be negative"),
                      (_geom(pads=(1, 1, -1, 1)), "padding must not be negative"), (_geom(pads=(1, 1, 1, -2)), "padding must not be negative"),
                      (_geom(KH=8), "does not fit the padded input (OH=0 OW=5)"), (_geom(KW=9), "does not fit the padded input (OH=5 OW=0)")):
        assert im(p, ctypes.byref(g), 0, p, p, None) == LQ_EINVAL and needle in _err(), needle
    for k in range(4):                                     # a negative stride of X
        xs = [75, 25, 5, 1]
        xs[k] = -xs[k]
        assert im(p, ctypes.byref(_geom(xs=tuple(xs))), 0, p, p, None) == LQ_EINVAL and "strides of X must not be negative" in _err()
    # what lq_i8_operand_quantize refuses about M, K and block
    big = _geom(B=1 << 20, Cc=64, H=8, W=8, xs=(4096, 64, 8, 1))
    assert im(p, ctypes.byref(big), 0, p, p, None) == LQ_EINVAL and "not below 2^31" in _err()
    for block in (-64, 32, 65, 100, (1 << 30) + 64):
        assert im(p, ctypes.byref(ok), block, p, p, None) == LQ_EINVAL and "scale block" in _err(), block
        assert lib.lq_i8_operand_quantize(p, 50, 27, block, p, p, None) == LQ_EINVAL, block
    # alignment
    assert im(p, ctypes.byref(ok), 0, p + 4, p, None) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert im(p, ctypes.byref(ok), 64, p, p + 4, None) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()
    assert im(p + 2, ctypes.byref(ok), 0, p, p, None) == LQ_EALIGN and "'X' is not 4-byte aligned" in _err()


def test_refusals_of_the_operand_call():
    x = torch.zeros(2, 5, 6, 6)
    for block in (32, -64, 1.5, True):
        with pytest.raises(ValueError, match="scale block"):
            ops.i8_operand_im2col(x, 3, block=block)
    with pytest.raises(ValueError, match="four axes"):
        ops.i8_operand_im2col(torch.zeros(5, 6, 6), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.i8_operand_im2col(x, 3)


CONV_K = 5 * 3 * 3


def test_the_conv_check():
    chk = ops.check_i8_conv_operand_layer
    assert chk((-128, 127), "scalar", None, fan_in=CONV_K) == (-128, 127)
    assert chk((-8, 7), "groupwise", 64, fan_in=640) == (-8, 7) and chk((-8, 7), "groupwise", 128, fan_in=640) == (-8, 7)
    assert chk((-8, 7), "groupwise", CONV_K, fan_in=CONV_K) == (-8, 7) and chk((-8, 7), "groupwise", 50, fan_in=CONV_K) == (-8, 7)
    for orientation, axis in (("rowwise", "kh"), ("columnwise", "kw"), ("channelwise", "ci")):
        with pytest.raises(ValueError, match=f'orientation="{orientation}".*lies on {axis}'):
            chk((-128, 127), orientation, None, fan_in=CONV_K)
    assert ops.check_i8_operand_layer((-128, 127), "columnwise") == (-128, 127)      # the Dense check accepts it; it must not leak
    for args, kw, needle in ((((-128, 127), "scalar"), dict(kernel_storage="hwio"), 'kernel_storage="hwio"'),
                             ((None, "scalar"), {}, "needs a layer with bits or q_range"),
                             (((0, 255), "scalar"), {}, "not inside [-128, 127]"),
                             (((-129, 127), "scalar"), {}, "not inside [-128, 127]"),
                             (((-8, 7), "groupwise", 64), dict(asymmetric=True), "asymmetric=True"),
                             (((-8, 7), "groupwise", 32), dict(element_format="fp4_e2m1"), "element_format"),
                             (((-8, 7), "groupwise", 32), dict(fan_in=CONV_K + 19), "group_size=32"),
                             (((-8, 7), "groupwise", 96), dict(fan_in=640), "group_size=96"),
                             (((-8, 7), "diagonal"), {}, "orientation='diagonal'")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            chk(*args, **kw)


def _conv(cls=L.CustomConv2DLayer, **kw):
    kw.setdefault("input_shape", 5)
    kw.setdefault("scale_gradient", "ste")
    return cls(filters=8, kernel_size=(3, 3), initializer=L.RandomNormal(seed=1), **kw)


def test_refusals_of_the_layers():
    x = torch.zeros(2, 5, 6, 6)
    for cls in (L.CustomConv2DLayer, L.CustomConv2DLayerNoBias):
        for kw, needle in ((dict(bits=8, orientation="rowwise"), 'orientation="rowwise"'),
                           (dict(bits=8, orientation="columnwise"), 'orientation="columnwise"'),
                           (dict(bits=8, orientation="channelwise"), 'orientation="channelwise"'),
                           (dict(bits=8, orientation="scalar", kernel_storage="hwio"), 'kernel_storage="hwio"'),
                           (dict(orientation="scalar", scale_gradient=None), "needs a layer with bits or q_range"),
                           (dict(bits=8, signed=False, orientation="scalar"), "not inside [-128, 127]"),
                           (dict(bits=9, orientation="scalar"), "not inside [-128, 127]"),
                           (dict(bits=4, orientation="groupwise", group_size=32, asymmetric=True), "asymmetric=True"),
                           (dict(orientation="groupwise", element_format="fp4_e2m1", scale_gradient=None), "element_format"),
                           (dict(bits=4, orientation="groupwise", group_size=32), "group_size=32"),
                           (dict(bits=8, orientation="scalar", input_shape=None), "not built yet")):
            c = _conv(cls, **kw)
            with pytest.raises(ValueError, match=re.escape(needle)):
                c.i8_operand()
            assert not L.i8_conv_eligible(c) and not L.i8_hardware_eligible(c), kw
            if c.built:
                with pytest.raises(ValueError, match=re.escape(needle)):
                    c.call_i8(x)
        c = _conv(cls, bits=8, orientation="scalar")
        for kw, needle in ((dict(act_block=32), "scale block"), (dict(max_lines=0), "max_lines"), (dict(max_lines=2.5), "max_lines"),
                           (dict(max_lines=True), "max_lines")):
            with pytest.raises(ValueError, match=re.escape(needle)):
                c.call_i8(x, **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # every check passed: the first launch needs the device
            c.call_i8(x)


def test_eligibility():
    for cls in (L.CustomConv2DLayer, L.CustomConv2DLayerNoBias):
        for kw in (dict(bits=8, orientation="scalar"), dict(bits=4, orientation="scalar"), dict(q_range=(-127, 127), orientation="scalar"),
                   dict(bits=4, orientation="groupwise", group_size=64), dict(bits=4, orientation="groupwise", group_size=CONV_K),
                   dict(bits=4, orientation="groupwise", group_size=CONV_K + 3),
                   dict(bits=4, orientation="groupwise", group_size=128, input_shape=40)):
            c = _conv(cls, **kw)
            assert L.i8_conv_eligible(c) and not L.i8_hardware_eligible(c), kw
    d = L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), input_shape=70, orientation="columnwise", bits=8, scale_gradient="ste")
    assert L.i8_hardware_eligible(d) and not L.i8_conv_eligible(d)
    for kw in (dict(bits=8, orientation="scalar"), dict(bits=4, group_size=64)):
        m = lq.build_model("cifar", mode="ste", value=0.0, **kw)
        assert [c.kernel_storage for c in m.convs] == ["oihw"] * 6
        assert sum(L.i8_conv_eligible(c) for c in L.custom_layers_of(m)) == 6 and not any(L.i8_hardware_eligible(c) for c in L.custom_layers_of(m))
        hw = L.i8_hardware(m)
        assert hw.convs is False and L.i8_hardware(m, convs=True).convs is True
        with pytest.raises(ValueError, match="no Dense layer that can run on the int8 matrix instruction"):
            train.i8_eval(m, torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.long))
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8)       # the model's default: channelwise
    assert not any(L.i8_conv_eligible(c) for c in L.custom_layers_of(m))
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8, orientation="scalar", kernel_storage="hwio")
    assert not any(L.i8_conv_eligible(c) for c in L.custom_layers_of(m))


def test_driver_refusal(capsys):
    with pytest.raises(SystemExit):
        train.main(["--config", "cifar", "--mode", "ste", "--bits", "8", "--i8-eval-convs"])
    assert "--i8-eval-convs needs --i8-eval" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------- the conditions of the GPU inputs
@pytest.mark.parametrize("g", R.GEOMS, ids=_gid)
def test_gaussian_inputs_give_codes_in_every_live_block(g):
    x = R.gaussian_input(g)
    for block in R.BLOCKS:
        op, cbuf, sbuf = R.reference(x, g, block)
        M, K, _, _ = C.dims(g)
        nbs = op["scales"].shape[1]
        span = R.span_of(g, block)
        live = R.live_pairs(g, block)
        padded = np.zeros((M, nbs * span), np.int8)
        padded[:, :K] = op["codes"]
        nonzero = (padded.reshape(M, nbs, span) != 0).any(axis=2)
        assert np.array_equal(nonzero, live), "a live pair holds a non-zero code, a pair of padding none"
        assert np.isfinite(op["scales"]).all() and (op["scales"][~live] == R.MIN_SCALE).all() and (op["scales"][live] > R.MIN_SCALE).all()
        assert (np.abs(padded.reshape(M, nbs, span).astype(np.int32)).max(axis=2)[live] == 127).all()      # the absmax element
        assert (cbuf.size, sbuf.size * 4) == ops.i8_operand_bytes(M, K, block)
    if g == R.PADDING_ONLY:
        assert (~R.live_pairs(g, 0)).sum() == 40 and R.live_pairs(g, 0).sum() == 32


@pytest.mark.parametrize("g,zero_channels", R.PLANTED, ids=["k245", "k576"])
def test_planted_pixels_spoil_some_pairs_and_not_all(g, zero_channels):
    x, nan_at, inf_at, big_at = R.planted_input(g, list(zero_channels))
    M, K, _, _ = C.dims(g)
    for block in R.BLOCKS:
        cover = R.windows_covering(g, block, *nan_at) | R.windows_covering(g, block, *inf_at)
        assert 0 < cover.sum() < cover.size, block
        op, _, _ = R.reference(x, g, block)
        assert np.array_equal(np.isnan(op["scales"]), cover)
        span = R.span_of(g, block)
        nbs = cover.shape[1]
        padded = np.zeros((M, nbs * span), np.int8)
        padded[:, :K] = op["codes"]
        assert not padded.reshape(M, nbs, span)[cover].any(), "the codes under a NaN scale are 0"
        big = R.windows_covering(g, block, *big_at) & ~cover
        assert big.any() and (op["scales"][big] > 1e27).all()
        if block:                                          # the zero channels fill whole scale blocks
            A = np.zeros((M, nbs * span), np.float32)
            A[:, :K] = C.im2col(np.nan_to_num(x, nan=1.0, neginf=1.0), g)
            zero = (A.reshape(M, nbs, span) == 0).all(axis=2)
            assert zero.any() == (not (block == 128 and K == 245)), "K = 245 has no all-zero block of 128"
            assert not (zero & cover).any() and (op["scales"][zero] == R.MIN_SCALE).all()


@pytest.mark.parametrize("g", R.EXACT_GEOMS, ids=_gid)
def test_exact_inputs_have_absmax_127_in_every_row(g):
    """The codes are the pixels, every scale is 1 + 2^-22, and the float64 convolution of the pixels times that margin with the
    kernel rounds ONCE to the device's product: every integer sum stays below 2^24, where float32 holds it exactly."""
    x = R.exact_input(g)
    A = C.im2col(x, g)
    assert (np.abs(A).max(axis=1) == 127).all() and np.array_equal(A, np.round(A))
    op, _, _ = R.reference(x, g, 0)
    assert np.array_equal(op["codes"], A.astype(np.int8)) and (op["scales"] == R.MARGIN).all()
    k, bias, scale, bscale = R.exact_kernel(g, 24)
    Wm = C.kernel_matrix(k)
    q = Wm / scale
    assert np.array_equal(q, np.round(q)) and q.min() >= -128 and q.max() <= 127 and np.abs(q).max() >= 127
    wop = I.operand_of_parameter(Wm, np.full((24, 1), scale, np.float32), -128, 127, 1, Wm.shape[1], "floor")
    assert np.array_equal(wop["codes"], q.astype(np.int8)) and wop["block"] == 0
    assert (np.abs(A.astype(np.int64)) @ np.abs(q.astype(np.int64)).T).max() < 1 << 24
    qb = bias / bscale
    assert np.array_equal(qb, np.round(qb)) and np.abs(qb).max() <= 128
