"""The int8 GEMM's offset term without a device (include/lq_hip.h, "offsets on the B operand"): the NumPy reference
(tests/_i8_affine_reference.py) on a hand-worked case and against tests/_i8_reference.py at offsets 0, every refusal of the four C
entry points through a NULL stream, the Python refusals and opt-ins, the parser rules, and the conditions of the data sets that
tests/test_gpu_i8_affine.py compares bit for bit."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_affine_reference as A                                                              # noqa: E402
import _i8_reference as G                                                                     # noqa: E402

from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402
from learned_quantization_amd.models import build_model                                       # noqa: E402

LQ_EINVAL, LQ_EALIGN = -1, -4
ENTRY_POINTS = ("lq_i8_operand_pack_affine", "lq_i8_operand_decode_affine", "lq_i8_gemm_affine", "lq_i8_gemm_quantize_affine")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _hip.load().lq_last_error().decode()


def test_entry_points_are_declared_and_exported():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    for name in ENTRY_POINTS:
        assert callable(getattr(lib, name)) and f"int {name}(" in header
    assert "offsets on the A operand (asymmetric activations)" in header and "asymmetric (offset) layers" not in header


# ------------------------------------------------------------------------------------------- the reference
def test_reference_on_a_hand_worked_case():
    """Two periods of 64, M = 2, N = 2.  Row 0: codes 3 then -2 in the first period (R = 1), 5 in the second; row 1: -4 in the first
    (R = -4, a negative row sum), 0 in the second.  Column 0 has offset 0 in both periods; column 1 offsets 0.5 and -2."""
    a = np.zeros((2, 128), np.int8)
    a[0, 0], a[0, 1], a[0, 64] = 3, -2, 5
    a[1, 7] = -4
    b = np.zeros((2, 128), np.int8)
    b[0, 0], b[0, 64], b[1, 1], b[1, 7] = 2, 1, 10, 1
    A_ = dict(codes=a, scales=np.array([[0.5, 2.0], [1.0, 4.0]], np.float32), block=64)
    B_ = dict(codes=b, scales=np.array([[1.0, 0.25], [2.0, 1.0]], np.float32), offsets=np.array([[0.0, 0.0], [0.5, -2.0]], np.float32),
              block=64)
    # period 0: I = [[6, -20], [0, -4]], t = [[.5, 1], [1, 2]], R = [1, -4], c = [.5, -4]; period 1: I = [[5, 0], [0, 0]], t = [[.5, 2], [1, 4]], R = [5, 0], c = [10, 0]
    want = np.array([[6 * .5 + 5 * .5, -20 * 1 + .5 * .5 + 10 * -2.0],
                     [0.0, -4 * 2 + -4 * .5]], np.float32)
    got = A.gemm_affine_reference(A_, B_)
    assert np.array_equal(got, want), (got, want)
    assert [r.tolist() for r in A.row_sums(A_, B_)] == [[1, -4], [5, 0]]
    bias = np.array([1.0, -1.0], np.float32)
    assert np.array_equal(A.gemm_affine_reference(A_, B_, bias), want + bias)
    ref64, terms = A.gemm_affine_f64(A_, B_, bias)
    assert np.array_equal(ref64, (want + bias).astype(np.float64)) and (terms >= np.abs(ref64)).all()
    # decode: code * scale + offset
    dec = A.decode_affine(B_)
    assert dec[1, 1] == 10 * 2.0 + 0.5 and dec[1, 64] == -2.0 and dec[0, 64] == 0.25 and dec.dtype == np.float32


def test_offset_term_rounds_on_its_own():
    """c = RN(R sa) and RN(c ob) are separate roundings: R = 3, sa = 1/3 (rounded), ob = 3 gives RN(RN(3 * RN(1/3)) * 3) = 3, and the
    sum with a large symmetric term loses it entirely."""
    third = np.float32(1.0) / np.float32(3.0)
    a = np.zeros((1, 64), np.int8)
    a[0, :3] = 1
    b = np.zeros((1, 64), np.int8)
    A_ = dict(codes=a, scales=np.array([[third]], np.float32), block=0)
    B_ = dict(codes=b, scales=np.ones((1, 1), np.float32), offsets=np.array([[3.0]], np.float32), block=0)
    c = np.float32(3.0) * third
    assert A.gemm_affine_reference(A_, B_)[0, 0] == np.float32(c * np.float32(3.0))
    b[0, 0] = 127
    A_["scales"][:] = np.float32(2.0 ** 30)
    B_["offsets"][:] = np.float32(2.0 ** -30)
    y = A.gemm_affine_reference(A_, B_)[0, 0]
    assert y == np.float32(127 * 2.0 ** 30)       # 3 * 2^30 * 2^-30 = 3 is below half an ulp of 127 * 2^30


def test_zero_offsets_give_the_symmetric_reference_bit_for_bit():
    for a, b, bias in G.all_gemm_cases():
        for off in (0.0, -0.0):
            bz = dict(b, offsets=np.full(b["scales"].shape, off, np.float32))
            for bs in (None, bias):
                got, want = A.gemm_affine_reference(a, bz, bs), G.gemm_reference(a, b, bs)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_operand_of_parameter_affine_at_offset_zero_is_the_symmetric_operand():
    R_, C, axis, gs = G.PACK_CASES[3]
    P, s = G.pack_case(R_, C, axis, gs)
    for rounding in ("floor", "nearest"):
        sym = G.operand_of_parameter(P, s, -8, 7, axis, gs, rounding)
        aff = A.operand_of_parameter_affine(P, s, np.zeros_like(s), -8, 7, axis, gs, rounding)
        assert np.array_equal(sym["codes"], aff["codes"]) and aff["block"] == sym["block"] and not aff["offsets"].any()
        assert A.offsets_layout(aff).shape == G.pack_layout(sym)[1].shape


# ------------------------------------------------------------------------------------------- refusals of the C surface
def _with(args, **at):
    args = list(args)
    for k, v in at.items():
        args[int(k[1:])] = v
    return args


def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    pack, dec, gemm, gq = (getattr(lib, n) for n in ENTRY_POINTS)
    ok_pack = [p, p, p, -128, 127, 0, 160, 17, 0, 64, p, p, p, None]       # P s b qmin qmax rounding R C axis gs codes scales offsets
    ok_dec = [p, p, p, 5, 100, 0, None, None]                               # codes scales offsets L K block out: out NULL is the last check
    ok_gemm = [p, p, 0, p, p, p, 0, None, p, 16, 16, 16, 128, None]         # a.. b_codes b_scales b_offsets b_block bias Y ldy M N K
    ok_gq = [p, p, 0, p, p, p, 0, None, 0, 64, p, p, 16, 16, 128, None]     # .. bias act out_block out_codes out_scales M N K
    # what is new: NULL b / offsets, offsets off the 16-byte grid, b off the 4-byte grid
    assert pack(*_with(ok_pack, _2=None)) == LQ_EINVAL and "'b' is NULL" in _err()
    assert pack(*_with(ok_pack, _2=p + 2)) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert pack(*_with(ok_pack, _12=None)) == LQ_EINVAL and "'offsets' is NULL" in _err()
    assert pack(*_with(ok_pack, _12=p + 4)) == LQ_EALIGN and "offsets is not 16-byte aligned" in _err()
    assert dec(*_with(ok_dec, _2=None)) == LQ_EINVAL and "'offsets' is NULL" in _err()
    assert dec(*_with(ok_dec, _2=p + 8)) == LQ_EALIGN and "offsets is not 16-byte aligned" in _err()
    assert dec(*ok_dec) == LQ_EINVAL and "'out' is NULL" in _err()
    assert gemm(*_with(ok_gemm, _5=None)) == LQ_EINVAL and "'offsets' is NULL" in _err()
    assert gemm(*_with(ok_gemm, _5=p + 4)) == LQ_EALIGN and "offsets is not 16-byte aligned" in _err()
    assert gq(*_with(ok_gq, _5=None)) == LQ_EINVAL and "'offsets' is NULL" in _err()
    assert gq(*_with(ok_gq, _5=p + 4)) == LQ_EALIGN and "offsets is not 16-byte aligned" in _err()
    # what the symmetric twins refuse: pack
    for k, name in ((0, "'P'"), (1, "'s'"), (10, "'codes'"), (11, "'scales'")):
        assert pack(*_with(ok_pack, **{f"_{k}": None})) == LQ_EINVAL and f"{name} is NULL" in _err()
    for qmin, qmax in ((0, 255), (-129, 0), (-128, 128)):
        assert pack(*_with(ok_pack, _3=qmin, _4=qmax)) == LQ_EINVAL and "not inside [-128, 127]" in _err()
    assert pack(*_with(ok_pack, _3=5, _4=4)) == LQ_EINVAL and "qmin 5 > qmax 4" in _err()
    assert pack(*_with(ok_pack, _5=7)) == LQ_EINVAL and "bad rounding" in _err()
    assert pack(*_with(ok_pack, _8=2)) == LQ_EINVAL and "bad axis" in _err()
    for gs in (32, 100):
        assert pack(*_with(ok_pack, _9=gs)) == LQ_EINVAL and "neither the whole line" in _err()
    assert pack(*_with(ok_pack, _9=0)) == LQ_EINVAL and "group size 0 < 1" in _err()
    assert pack(*_with(ok_pack, _6=0)) == LQ_EINVAL and "extents must be positive" in _err()
    assert pack(*_with(ok_pack, _6=1 << 20, _7=1 << 11)) == LQ_EINVAL and "not below 2^31" in _err()
    assert pack(*_with(ok_pack, _10=p + 4)) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert pack(*_with(ok_pack, _11=p + 4)) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()
    # decode
    assert dec(*_with(ok_dec, _0=None)) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert dec(*_with(ok_dec, _1=None)) == LQ_EINVAL and "'scales' is NULL" in _err()
    assert dec(*_with(ok_dec, _5=48)) == LQ_EINVAL and "neither 0" in _err()
    assert dec(*_with(ok_dec, _3=0)) == LQ_EINVAL and "extents must be positive" in _err()
    assert dec(*_with(ok_dec, _1=p + 8)) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()
    assert dec(*_with(ok_dec, _6=p + 1)) == LQ_EALIGN and "not 4-byte aligned" in _err()
    # the two products: (function, ok arguments, index of M, N, K, and of the first output pointer)
    for fn, ok, iM, iN, iK, iout in ((gemm, ok_gemm, 10, 11, 12, 8), (gq, ok_gq, 12, 13, 14, 10)):
        for k in (0, 1, 3, 4, iout):
            assert fn(*_with(ok, **{f"_{k}": None})) == LQ_EINVAL and "NULL" in _err(), k
        for bad in (-64, 1, 32, 100):
            assert fn(*_with(ok, _2=bad)) == LQ_EINVAL and "neither 0" in _err()
            assert fn(*_with(ok, _6=bad)) == LQ_EINVAL and "neither 0" in _err()
        assert fn(*_with(ok, **{"_2": 128, "_6": 192, f"_{iK}": 1024})) == LQ_EINVAL and "multiple of the smaller" in _err()
        assert fn(*_with(ok, **{f"_{iK}": 65600})) == LQ_EINVAL and "period of 65600" in _err()
        assert fn(*_with(ok, **{f"_{iM}": 0})) == LQ_EINVAL and "extents must be positive" in _err()
        assert fn(*_with(ok, **{f"_{iN}": 0})) == LQ_EINVAL and "extents must be positive" in _err()
        assert fn(*_with(ok, **{f"_{iM}": 1 << 20, f"_{iK}": 1 << 11})) == LQ_EINVAL and "not below 2^31" in _err()
        assert fn(*_with(ok, _3=p + 8)) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
        assert fn(*_with(ok, _1=p + 4)) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()
        assert fn(*_with(ok, _7=p + 1)) == LQ_EALIGN and "bias is not 4-byte aligned" in _err()
    assert gemm(*_with(ok_gemm, _9=15)) == LQ_EINVAL and "is below N" in _err()
    assert gemm(*_with(ok_gemm, _10=65535 * 64 + 1, _12=64)) == LQ_EINVAL and "above 65535 * 64" in _err()
    assert gemm(*_with(ok_gemm, _8=p + 2)) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert gq(*_with(ok_gq, _9=128)) == LQ_EINVAL and "out_block = 128" in _err()
    assert gq(*_with(ok_gq, _9=0)) == LQ_EINVAL and "out_block = 0" in _err()
    assert gq(*_with(ok_gq, _8=2)) == LQ_EINVAL and "bad activation" in _err()
    assert gq(*_with(ok_gq, _11=p + 4)) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()


# ------------------------------------------------------------------------------------------- the Python surface
def _dense(**kw):
    kw.setdefault("scale_gradient", "ste")
    return L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), input_shape=70, **kw)


def _conv(**kw):
    kw.setdefault("input_shape", 5)
    kw.setdefault("scale_gradient", "ste")
    return L.CustomConv2DLayer(filters=8, kernel_size=(3, 3), initializer=L.RandomNormal(seed=1), **kw)


def test_operand_types():
    assert ops.I8Operand._fields == ("codes", "scales", "lines", "K", "block")
    assert issubclass(ops.I8AffineOperand, ops.I8Operand) and ops.I8AffineOperand._fields == ops.I8Operand._fields
    op = ops.I8AffineOperand(torch.zeros(16, dtype=torch.uint8), torch.zeros(16), 16, 128, 0)
    assert op.offsets is None
    op.offsets = torch.zeros(16)
    assert op.offsets is not None and tuple(op)[2:] == (16, 128, 0)


def test_offsets_on_a_are_refused():
    u8, f32 = torch.zeros(16, dtype=torch.uint8), torch.zeros(16)
    a = ops.I8AffineOperand(u8, f32, 16, 128, 0)
    a.offsets = f32
    b = ops.I8Operand(u8, f32, 16, 128, 0)
    for fn in (ops.i8_gemm, ops.i8_gemm_quantize):
        with pytest.raises(ValueError, match="only the B operand carries offsets: activation offsets are not built"):
            fn(a, b)


def test_default_refusals_stand_and_name_the_opt_in():
    with pytest.raises(ValueError, match=re.escape("asymmetric=True")) as e:
        ops.check_i8_operand_layer((-8, 7), "groupwise", 64, True)
    assert "offsets=True" in str(e.value) and "--i8-eval-offsets" in str(e.value) and "not built" not in str(e.value)
    with pytest.raises(ValueError, match=re.escape("asymmetric=True")) as e:
        ops.check_i8_conv_operand_layer((-8, 7), "groupwise", 64, asymmetric=True)
    assert "offsets=True" in str(e.value)
    with pytest.raises(TypeError):
        ops.check_i8_operand_layer((-8, 7), "groupwise", 64, True, None, None, True)      # keyword-only
    d = _dense(orientation="groupwise", group_size=64, bits=4, asymmetric=True)
    c = _conv(orientation="groupwise", group_size=64, bits=4, asymmetric=True)
    for layer, x in ((d, torch.zeros(3, 70)), (c, torch.zeros(1, 5, 6, 6))):
        with pytest.raises(ValueError, match=re.escape("asymmetric=True")):
            layer.i8_operand()
        with pytest.raises(ValueError, match=re.escape("asymmetric=True")):
            layer.call_i8(x)
    assert not L.i8_hardware_eligible(d) and not L.i8_conv_eligible(c)
    assert L.i8_hardware_eligible(d, offsets=True) and L.i8_conv_eligible(c, offsets=True)
    assert not L.i8_hardware_eligible(c, offsets=True) and not L.i8_conv_eligible(d, offsets=True)
    with pytest.raises(ValueError, match=re.escape("asymmetric=True")):
        L.i8_dense_chain(torch.zeros(3, 70), [(d, None)])


def test_opt_in_accepts_asymmetric_layers_and_keeps_the_other_reasons_in_order():
    assert ops.check_i8_operand_layer((-8, 7), "groupwise", 64, True, offsets=True) == (-8, 7)
    assert ops.check_i8_conv_operand_layer((-8, 7), "groupwise", 64, asymmetric=True, offsets=True) == (-8, 7)
    assert ops.check_i8_operand_layer((-8, 7), "groupwise", 64, False, offsets=True) == (-8, 7)      # a symmetric layer: as before
    for args, kw, needle in ((((-8, 7), "groupwise", 64, True, "fp4_e2m1"), {}, "a microscaling layer"),
                             ((None, "groupwise", 64, True), {}, "needs a layer with bits or q_range"),
                             (((0, 255), "groupwise", 64, True), {}, "not inside [-128, 127]"),
                             (((-8, 7), "rowwise", None, True), {}, 'orientation="rowwise"'),
                             (((-8, 7), "groupwise", 32, True), {}, "group_size=32")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            ops.check_i8_operand_layer(*args, offsets=True, **kw)
    # without the opt-in the asymmetric refusal still precedes the group-size one; with it the group size is what is named
    with pytest.raises(ValueError, match=re.escape("asymmetric=True")):
        ops.check_i8_conv_operand_layer((-8, 7), "groupwise", 32, asymmetric=True)
    with pytest.raises(ValueError, match=re.escape("group_size=32")):
        ops.check_i8_conv_operand_layer((-8, 7), "groupwise", 32, asymmetric=True, offsets=True)
    with pytest.raises(ValueError, match=re.escape('kernel_storage="hwio"')):
        ops.check_i8_conv_operand_layer((-8, 7), "groupwise", 64, asymmetric=True, kernel_storage="hwio", offsets=True)
    d32 = _dense(orientation="groupwise", group_size=32, bits=4, asymmetric=True)
    with pytest.raises(ValueError, match=re.escape("group_size=32")):
        d32.i8_operand(offsets=True)
    assert not L.i8_hardware_eligible(d32, offsets=True)
    unbuilt = L.CustomDenseLayer(units=4, bits=4, orientation="groupwise", group_size=64, asymmetric=True, scale_gradient="ste")
    with pytest.raises(ValueError, match="not built yet"):
        unbuilt.i8_operand(offsets=True)


def test_i8_hardware_takes_the_keyword():
    m = build_model("mnist", mode="ste", value=0.0, bits=4, group_size=128, asymmetric=True)
    dense = [x for x in L.custom_layers_of(m) if isinstance(x, L.CustomDenseLayer)]
    assert dense and not any(L.i8_hardware_eligible(x) for x in dense) and all(L.i8_hardware_eligible(x, offsets=True) for x in dense)
    hw = L.i8_hardware(m, 64, fused=True, offsets=True)
    assert hw.offsets is True and L.i8_hardware(m).offsets is False
    with pytest.raises(ValueError, match="emulate=True with fused=True"):
        L.i8_hardware(m, 64, emulate=True, fused=True, offsets=True)


def test_parser_rules(capsys):
    base = ["--config", "mnist", "--mode", "ste", "--bits", "4", "--group-size", "128", "--asymmetric"]
    with pytest.raises(SystemExit):
        train.main(base + ["--i8-eval"])
    assert "--i8-eval-offsets" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.main(base + ["--i8-eval-offsets"])
    assert "--i8-eval-offsets needs --i8-eval" in capsys.readouterr().err
    ns = train.build_parser().parse_args(base + ["--i8-eval", "--i8-eval-offsets"])
    assert ns.i8_eval and ns.i8_eval_offsets is True and ns.asymmetric
    assert train.build_parser().parse_args([]).i8_eval_offsets is False


# ------------------------------------------------------------------------------------------- conditions of the GPU data sets
def test_every_period_sum_and_row_sum_of_the_gpu_data_sets_fits():
    for key in A.all_gemm_affine_keys():
        a, b, _ = A.gemm_affine_case(*key)
        for _, I, _ in G.period_sums(a, b):
            assert I.min() >= -2 ** 31 and I.max() < 2 ** 31
        for R_ in A.row_sums(a, b):
            assert np.abs(R_).max() <= 2 ** 23
        off = b["offsets"]
        assert (off < 0).any() and (off == 0).any() and (off > 0).any() and np.isfinite(off).all()
    assert (16, 16, 64, 0, 0) in A.all_gemm_affine_keys()


def test_pin_cases_are_exact_and_below_2_24():
    b = A.pin_b()
    off = b["offsets"]
    assert b["scales"].shape == (A.PIN_N, 3) and not b["codes"].any() and (b["scales"] == 1).all()
    assert len(np.unique(np.abs(off))) > 1 and all(len(np.unique(np.abs(off[:, p]))) == A.PIN_N for p in range(3))
    assert all(len(np.unique(np.abs(off[n]))) == 3 for n in range(A.PIN_N)) and (off < 0).any()
    assert (np.frexp(np.abs(off))[0] == 0.5).all()                                     # powers of two
    cases = [A.pin_one_hot_a(k) for k in (0, 63, 64, 127, 128, 159)] + [A.pin_random_a()]
    for a in cases:
        ref = A.gemm_affine_reference(a, b)
        ref64, _ = A.gemm_affine_f64(a, b)
        assert np.array_equal(ref.astype(np.float64), ref64)                           # exact: every partial sum survives float32
        R_ = np.stack(A.row_sums(a, b))
        assert np.abs(R_).max() < 2 ** 24
        want = sum(R_[p][:, None].astype(np.float64) * off[:, p][None, :].astype(np.float64) for p in range(3))
        assert np.array_equal(ref64, want)
    assert (np.stack(A.row_sums(A.pin_one_hot_a(3), b))[:, 0] < 0).any()               # a negative row sum
    a, bx = A.pin_extreme()
    R_ = A.row_sums(a, bx)
    assert len(R_) == 1 and (R_[0] == -2 ** 23).all()
    ref = A.gemm_affine_reference(a, bx)
    assert np.array_equal(ref.astype(np.float64), A.gemm_affine_f64(a, bx)[0])


def test_exact_dense_case_is_exact():
    x, W, s, b, bias = A.exact_dense_case()
    assert (np.abs(x).max(axis=1) == 127).all() and (x == np.rint(x)).all()
    assert (np.frexp(s)[0] == 0.5).all() and (b / s == np.rint(b / s)).all()
    y64 = x.astype(np.float64) @ W.astype(np.float64) + bias
    assert np.array_equal(y64.astype(np.float32).astype(np.float64), y64) and np.abs(y64).max() < 2 ** 24
    # every partial sum in the definition's order survives float32: the reference on the exact operands equals float64
    g = np.arange(x.shape[1]) // 64
    q = np.rint((W - b[g]) / s[g])
    assert np.array_equal(q * s[g] + b[g], W) and q.min() >= -8 and q.max() <= 7
    a_op = dict(codes=x.astype(np.int8), scales=np.ones((x.shape[0], 1), np.float32), block=0)
    b_op = dict(codes=q.T.astype(np.int8), scales=np.ascontiguousarray(s.T), offsets=np.ascontiguousarray(b.T), block=64)
    ref = A.gemm_affine_reference(a_op, b_op, bias)
    assert np.array_equal(ref.astype(np.float64), y64)
