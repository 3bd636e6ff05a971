"""CPU tests of the packed MX operands and the block-scaled GEMM (include/lq_hip.h: lq_mx_operand_* / lq_mx_gemm): sizes, every
refusal through the C surface and through Python, and the conditions of the data sets tests/test_gpu_mx_gemm.py runs on the
device (tests/_mx_gemm_reference.py builds them), asserted here so that the GPU file need not.  Also the NumPy packer of the
documented operand layout (round trip, sizes, padding, a table of offsets worked out by hand from the header) and the conditions of
the one-term sweeps of tests/test_gpu_mx_gemm_codes.py: every product of two codes is an fp32, the classes of the scale sweep."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _mx_gemm_reference as G                                                                # noqa: E402
import _mx_reference as X                                                                     # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402
from learned_quantization_amd.models import build_model                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ_EINVAL, LQ_EALIGN = -1, -4
FP4, FP6A, FP6B, E4M3, E5M2 = 0, 1, 2, 3, 4


def _err():
    return _hip.load().lq_last_error().decode()


def _bytes(fmt, L_, K):
    cb, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = _hip.load().lq_mx_operand_bytes(fmt, L_, K, ctypes.byref(cb), ctypes.byref(sb))
    return rc, cb.value, sb.value


def test_entry_points_are_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    for fn in ("lq_mx_operand_bytes", "lq_mx_operand_pack", "lq_mx_operand_quantize", "lq_mx_operand_decode", "lq_mx_gemm"):
        assert fn in declared and hasattr(lib, fn) and fn in _hip.SIGNATURES, fn
    assert lq.mx_gemm is ops.mx_gemm and lq.mx_operand_pack is ops.mx_operand_pack and lq.mx_hardware is L.mx_hardware
    assert ops.MX_OPERAND_FORMATS == G.OPERAND_FORMATS


@pytest.mark.parametrize("fmt,fb", [(FP4, 16), (E4M3, 32), (E5M2, 32)])
def test_sizes(fmt, fb):
    """code_bytes = ceil(L / 16) ceil(K / 128) 64 FB; scale_bytes = ceil(L / 16) ceil(ceil(K / 128) / 4) 256."""
    for L_, K in ((1, 1), (16, 128), (17, 129), (40, 70), (10, 784), (4096, 4096), (33, 513)):
        LT, KT = -(-L_ // 16), -(-K // 128)
        assert _bytes(fmt, L_, K) == (0, LT * KT * 64 * fb, LT * -(-KT // 4) * 256), (L_, K)
    assert ops.mx_operand_bytes(("fp4_e2m1", None, None, "fp8_e4m3", "fp8_e5m2")[fmt], 40, 70) == _bytes(fmt, 40, 70)[1:]


def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    cb, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    size, pack, quant, dec, gemm = (lib.lq_mx_operand_bytes, lib.lq_mx_operand_pack, lib.lq_mx_operand_quantize,
                                    lib.lq_mx_operand_decode, lib.lq_mx_gemm)
    # fp6 and unknown formats, everywhere
    for bad, needle in ((FP6A, "fp6 operands are not supported"), (FP6B, "fp6 operands are not supported"), (-1, "bad element format"),
                        (5, "bad element format")):
        assert size(bad, 16, 128, ctypes.byref(cb), ctypes.byref(sb)) == LQ_EINVAL and needle in _err()
        assert pack(p, p, bad, 0, 70, 40, 0, 32, p, p, None) == LQ_EINVAL and needle in _err()
        assert quant(p, bad, 0, 5, 100, p, p, None) == LQ_EINVAL and needle in _err()
        assert dec(p, p, bad, 5, 100, p, None) == LQ_EINVAL and needle in _err()
        assert gemm(p, p, bad, p, p, FP4, None, p, 16, 16, 128, 16, None) == LQ_EINVAL and needle in _err()
        assert gemm(p, p, FP4, p, p, bad, None, p, 16, 16, 128, 16, None) == LQ_EINVAL and needle in _err()
    # gs != 32 and fp32 scales
    for gs in (16, 31, 33, 64, 70):
        assert pack(p, p, FP4, 0, 70, 40, 0, gs, p, p, None) == LQ_EINVAL and "the instruction's block is 32" in _err()
    assert pack(p, p, FP4, 1, 70, 40, 0, 32, p, p, None) == LQ_EINVAL and "E8M0 scales only" in _err()
    assert pack(p, p, FP4, 2, 70, 40, 0, 32, p, p, None) == LQ_EINVAL and "bad scale format" in _err()
    for axis in (-1, 2):
        assert pack(p, p, FP4, 0, 70, 40, axis, 32, p, p, None) == LQ_EINVAL and "bad axis" in _err()
    for method in (-1, 2):
        assert quant(p, E4M3, method, 5, 100, p, p, None) == LQ_EINVAL and "bad method" in _err()
    # null pointers
    assert size(FP4, 16, 128, None, ctypes.byref(sb)) == LQ_EINVAL and "NULL" in _err()
    assert size(FP4, 16, 128, ctypes.byref(cb), None) == LQ_EINVAL and "NULL" in _err()
    assert pack(None, p, FP4, 0, 70, 40, 0, 32, p, p, None) == LQ_EINVAL and "'P' is NULL" in _err()
    assert pack(p, None, FP4, 0, 70, 40, 0, 32, p, p, None) == LQ_EINVAL and "'s' is NULL" in _err()
    assert pack(p, p, FP4, 0, 70, 40, 0, 32, None, p, None) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert pack(p, p, FP4, 0, 70, 40, 0, 32, p, None, None) == LQ_EINVAL and "'scales' is NULL" in _err()
    assert quant(None, E4M3, 0, 5, 100, p, p, None) == LQ_EINVAL and "'X' is NULL" in _err()
    assert quant(p, E4M3, 0, 5, 100, None, p, None) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert quant(p, E4M3, 0, 5, 100, p, None, None) == LQ_EINVAL and "'scales' is NULL" in _err()
    assert dec(None, p, E4M3, 5, 100, p, None) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert dec(p, None, E4M3, 5, 100, p, None) == LQ_EINVAL and "'scales' is NULL" in _err()
    assert dec(p, p, E4M3, 5, 100, None, None) == LQ_EINVAL and "'out' is NULL" in _err()
    for k in (0, 1, 3, 4, 7):                              # every pointer of the GEMM but the bias
        args = [p, p, E4M3, p, p, FP4, None, p, 16, 16, 128, 16, None]
        args[k] = None
        assert gemm(*args) == LQ_EINVAL and "NULL" in _err(), k
    # extents, the leading dimension
    for L_, K in ((0, 128), (16, 0), (-1, 128)):
        assert size(FP4, L_, K, ctypes.byref(cb), ctypes.byref(sb)) == LQ_EINVAL and "extents must be positive" in _err()
        assert quant(p, FP4, 0, L_, K, p, p, None) == LQ_EINVAL and "extents must be positive" in _err()
        assert gemm(p, p, FP4, p, p, FP4, None, p, L_, 16, K, 16, None) == LQ_EINVAL and "extents must be positive" in _err()
    assert size(FP4, 1 << 20, 1 << 11, ctypes.byref(cb), ctypes.byref(sb)) == LQ_EINVAL and "not below 2^31" in _err()
    for ldy in (15, 0, -1):
        assert gemm(p, p, FP4, p, p, FP4, None, p, 16, 16, 128, ldy, None) == LQ_EINVAL and "is below N" in _err()
    # alignment
    assert pack(p, p, FP4, 0, 70, 40, 0, 32, p + 4, p, None) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert pack(p, p, FP4, 0, 70, 40, 0, 32, p, p + 2, None) == LQ_EALIGN and "scales is not 4-byte aligned" in _err()
    assert quant(p + 2, FP4, 0, 5, 100, p, p, None) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert gemm(p, p, FP4, p + 8, p, FP4, None, p, 16, 16, 128, 16, None) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert gemm(p, p, FP4, p, p, FP4, p + 1, p, 16, 16, 128, 16, None) == LQ_EALIGN and "bias is not 4-byte aligned" in _err()
    assert gemm(p, p, FP4, p, p, FP4, None, p + 2, 16, 16, 128, 16, None) == LQ_EALIGN and "not 4-byte aligned" in _err()


def _dense(**kw):
    return L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), input_shape=70, **kw)


def test_refusals_of_the_python_surface():
    P, s = torch.zeros(70, 40), torch.ones(3, 40)
    for name in ("fp6_e2m3", "fp6_e3m2"):
        with pytest.raises(ValueError, match="fp6 operands are not supported"):
            ops.mx_operand_pack(P, s, name)
        with pytest.raises(ValueError, match="fp6 operands are not supported"):
            ops.mx_operand_quantize(P, name)
        with pytest.raises(ValueError, match="fp6 operands are not supported"):
            ops.mx_operand_bytes(name, 16, 128)
    with pytest.raises(ValueError, match="element_format must be"):
        ops.mx_operand_quantize(P, "fp5")
    with pytest.raises(ValueError, match="E8M0"):
        ops.mx_operand_pack(P, s, "fp4_e2m1", scale_format="fp32")
    for gs in (16, 64):
        with pytest.raises(ValueError, match="block-scaled matrix instruction is 32"):
            ops.mx_operand_pack(P, s, "fp4_e2m1", group_size=gs)
    with pytest.raises(ValueError, match="must be one of"):
        ops.mx_operand_quantize(P, "fp8_e4m3", method="absmax")
    with pytest.raises(ValueError, match="x must be a matrix"):
        ops.mx_operand_quantize(torch.zeros(2, 3, 4), "fp8_e4m3")
    u8 = torch.zeros(16, dtype=torch.uint8)
    a, b = ops.MxOperand(u8, u8, "fp8_e4m3", 16, 128), ops.MxOperand(u8, u8, "fp4_e2m1", 16, 160)
    with pytest.raises(ValueError, match="different K: 128 and 160"):
        ops.mx_gemm(a, b)
    with pytest.raises(ValueError, match="fp6 operands are not supported"):
        ops.mx_gemm(a, ops.MxOperand(u8, u8, "fp6_e2m3", 16, 128))
    with pytest.raises(ValueError, match="fp6 operands are not supported"):
        ops.mx_operand_decode(ops.MxOperand(u8, u8, "fp6_e3m2", 16, 128))
    # layers
    for kw, needle in ((dict(orientation="groupwise", group_size=32, bits=4, scale_gradient="ste"), "needs a layer with an element_format"),
                       (dict(), "needs a layer with an element_format"),
                       (dict(orientation="groupwise", element_format="fp4_e2m1", scale_format="fp32"), "E8M0"),
                       (dict(orientation="groupwise", element_format="fp6_e2m3"), "fp6 operands are not supported"),
                       (dict(orientation="groupwise", element_format="fp6_e3m2"), "fp6 operands are not supported"),
                       (dict(orientation="groupwise", element_format="fp8_e4m3", group_size=16), "group_size=16"),
                       (dict(orientation="groupwise", element_format="fp8_e4m3", group_size=64), "group_size=64")):
        d = _dense(**kw)
        with pytest.raises(ValueError, match=re.escape(needle)):
            d.mx_operand()
        with pytest.raises(ValueError, match=re.escape(needle)):
            d.call_mx(torch.zeros(3, 70))
        assert not L.mx_hardware_eligible(d)
    assert L.mx_hardware_eligible(_dense(orientation="groupwise", element_format="fp4_e2m1"))
    m = build_model("mnist", mode="ste", value=0.0, element_format="fp4_e2m1")
    for kw, needle in ((dict(act_format="fp6_e2m3"), "fp6 operands"), (dict(act_format="int8"), "element_format must be"),
                       (dict(act_scale="absmax"), "must be one of")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            L.mx_hardware(m, **kw)


def test_driver_refusal():
    from learned_quantization_amd import train
    with pytest.raises(SystemExit):
        train.main(["--config", "mnist", "--mode", "ste", "--mx-eval"])


# ------------------------------------------------------------------------------------------- conditions of the GPU data sets
@pytest.mark.parametrize("shape,identity", G.EXACT_CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_exact_sets_sum_exactly_in_every_order(shape, identity):
    """Every element is on the grid of all three formats under its scale, the nonzero terms of an output span at most 2^12, and
    the float32 sum of each output's terms in natural, reversed and pairwise order equals the float64 sum."""
    M, N, K = shape
    case = G.exact_case(M, N, K, identity)
    ops_ = {pair: G.exact_operands(case, *pair) for pair in (("fp4_e2m1", "fp8_e5m2"), ("fp8_e4m3", "fp4_e2m1"))}
    A = G.decode(ops_[("fp4_e2m1", "fp8_e5m2")][0])
    B = G.decode(ops_[("fp4_e2m1", "fp8_e5m2")][1])
    for a, b in ops_.values():                             # the formats hold the same values: nothing is rounded
        assert np.array_equal(G.decode(a), case["A"].astype(np.float64)) and np.array_equal(G.decode(b), case["W"].T.astype(np.float64))
        for o in (a, b):
            assert o.bytes.min() >= 125 and o.bytes.max() <= 130
    assert not np.array_equal(B[:min(N, K), :min(N, K)], B[:min(N, K), :min(N, K)].T), "B must be asymmetric"
    terms = A[:, None, :] * B[None, :, :]                  # (M, N, K) float64, exact
    nz = np.abs(terms[terms != 0])
    assert nz.max() / nz.min() <= 2.0 ** 12
    assert np.array_equal(terms.astype(np.float32).astype(np.float64), terms)
    ref = terms.sum(axis=-1)
    for got in G.sums_f32(terms):
        assert np.array_equal(got.astype(np.float64), ref)
    Y, _ = G.gemm_reference(*ops_[("fp8_e4m3", "fp4_e2m1")], case["bias"])
    assert np.array_equal(Y, ref + case["bias"][None, :]) and np.array_equal(Y.astype(np.float32).astype(np.float64), Y)
    if identity:
        hot = (37 * np.arange(M) + 5) % K
        assert np.array_equal((A != 0).sum(axis=1), np.ones(M)) and np.array_equal(np.argmax(A != 0, axis=1), hot)


@pytest.mark.parametrize("shape", G.RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pair", G.PAIRS, ids=lambda p: "-".join(p))
def test_random_sets_hold_no_special_codes(shape, pair):
    """No NaN / Inf code occurs and every scale byte lies inside 1 .. 254, under both activation rules."""
    case = G.random_case(*shape, *pair)
    b = G.operand_of_parameter(case["W"], case["sw"], pair[1], 0)
    for method in ("mx", "cover"):
        a, _ = G.operand_of_activation(case["x"], pair[0], method)
        for o in (a, b):
            assert np.isfinite(X.decode_table(X.FORMATS[o.name])[o.codes]).all()
            assert o.bytes.min() >= 1 and o.bytes.max() <= 254
    Y, T = G.gemm_reference(a, b, case["bias"])
    assert np.isfinite(Y).all() and (T > 0).all()


def test_quantize_set_holds_its_special_blocks():
    for M, K in G.QUANT_SHAPES:
        x = G.quantize_case(M, K)
        for method in ("mx", "cover"):
            op, s = G.operand_of_activation(x, "fp8_e4m3", method)
            assert op.bytes[1, 1] == 1 and (op.codes[1, 32:64] == 0).all()            # the zero block: scale 2^-126
            assert (op.bytes == 255).sum() == 1 and op.bytes[M - 1, (K - 3) // 32] == 255
            assert np.isnan(s).sum() == 1


# --------------------------------------------------------------------------------------- the documented layout, restated in NumPy
def _random_operand(name, L_, K, seed=0):
    rng = np.random.default_rng(G.stable_seed("mx-layout", name, L_, K, seed))
    return G.RefOperand(rng.integers(0, 16 if name == "fp4_e2m1" else 256, size=(L_, K)), rng.integers(0, 256, size=(L_, -(-K // 32))),
                        name, None)


@pytest.mark.parametrize("shape", [(19, 160), (37, 784)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", G.OPERAND_FORMATS)
def test_layout_round_trip_sizes_and_padding(name, shape):
    """unpack_layout(pack_layout(op)) is op for random codes and bytes (every value of both), the buffers have lq_mx_operand_bytes'
    sizes, and what no live (line, k) addresses is code 0 and byte 127: changing the live part changes nothing else."""
    L_, K = shape
    op = _random_operand(name, L_, K)
    cbuf, sbuf = G.pack_layout(op.codes, op.bytes, name)
    assert cbuf.dtype == sbuf.dtype == np.uint8 and (cbuf.size, sbuf.size) == ops.mx_operand_bytes(name, L_, K)
    codes, bytes_ = G.unpack_layout(cbuf, sbuf, name, L_, K)
    assert np.array_equal(codes, op.codes) and np.array_equal(bytes_, op.bytes)
    assert G.layout_mismatch(cbuf, sbuf, op) is None
    # the live bytes are the same set for every content, and the rest is the padding
    full = G.pack_layout(np.full_like(op.codes, 15 if name == "fp4_e2m1" else 255), np.full_like(op.bytes, 255), name)
    none = G.pack_layout(np.zeros_like(op.codes), np.full_like(op.bytes, 127), name)
    assert not none[0].any() and (none[1] == 127).all()
    live_c, live_s = full[0] != 0, full[1] != 127
    bits = 4 if name == "fp4_e2m1" else 8
    assert np.unpackbits(full[0]).sum() == L_ * K * bits and live_s.sum() == L_ * -(-K // 32)
    assert not cbuf[~live_c].any() and (sbuf[~live_s] == 127).all()
    LT, KT, KG = G.layout_dims(L_, K)
    assert live_s.sum() < sbuf.size and (4 * KG > KT or 16 * LT > L_)
    # and a difference is named by its logical position
    other = op.codes.copy()
    other[L_ - 1, K - 1] ^= 1
    assert f"(line, k) = ({L_ - 1}, {K - 1})" in G.layout_mismatch(*G.pack_layout(other, op.bytes, name), op)
    pad = sbuf.copy()
    pad[np.flatnonzero(~live_s)[-1]] = 126
    assert "padding scale bytes are not 127" in G.layout_mismatch(cbuf, pad, op)


# (format, L, K, line, k) -> (byte offset of the code, shift of its nibble, byte offset of its block's scale), each worked out by hand
# from include/lq_hip.h ("packed MX operands"): codes [LT][KT][64][FB], scales [LT][KG][64][4], lane = 16 g + (line & 15).
# (37, 784): LT 3, KT 7, KG 2.  (37, 1184): KT 10, KG 3.
LAYOUT_TABLE = [
    ("fp4_e2m1", 37, 784, 0, 0, 0, 0, 0),
    # fp4, block g = 1, j = 5: lane 16 + 3 = 19, byte 19 * 16 + (5 >> 1), high nibble; scale dword 19, u = 0
    ("fp4_e2m1", 37, 784, 3, 37, 306, 4, 76),
    # fp8, k >= 64: kk = 77 is the second half (h = 1) of g = (77 & 63) >> 4 = 0, j = 13: lane 5, byte 5 * 32 + 16 + 13; its block
    # is g = 2: scale dword 32 + 5
    ("fp8_e4m3", 37, 784, 5, 77, 189, 0, 148),
    # a second K step: kt = 1, kk = 5: tile 1, lane 2, byte (64 + 2) * 32 + 5; block 4 = step 1, g = 0: dword 2, u = 1
    ("fp8_e5m2", 37, 784, 2, 133, 2117, 0, 9),
    # a second line tile: lt = 1, r = 4, kt = 1, kk = 72: g = 2, j = 8: tile 1 * 7 + 1 = 8, lane 36, byte (512 + 36) * 16 + 4, low
    # nibble; block 6 = step 1, g = 2: cell 1 * 2 + 0 = 2, dword 128 + 36, u = 1
    ("fp4_e2m1", 37, 784, 20, 200, 8772, 0, 657),
    # the third line tile, kt = 5, kk = 127: h = 1, g = 3, j = 15: tile 2 * 7 + 5 = 19, lane 52, byte (1216 + 52) * 32 + 31; block 23 =
    # step 5, g = 3: kg = 1, u = 1: cell 2 * 2 + 1 = 5, dword 320 + 52
    ("fp8_e4m3", 37, 784, 36, 767, 40607, 0, 1489),
    # a scale byte with u = 3 and kg = 1: k = 975 is step 7, kk = 79: h = 1, g = 0, j = 15: tile 1 * 10 + 7 = 17, lane 5, byte
    # (1088 + 5) * 32 + 31; block 30 = step 7, g = 2: cell 1 * 3 + 1 = 4, dword 256 + 37, byte 3
    ("fp8_e5m2", 37, 1184, 21, 975, 35007, 0, 1175),
]


@pytest.mark.parametrize("entry", LAYOUT_TABLE, ids=lambda e: f"{e[0]}-{e[1]}x{e[2]}-{e[3]}-{e[4]}")
def test_layout_table_worked_out_by_hand(entry):
    name, L_, K, ln, k, code_off, shift, scale_off = entry
    code = 0xB if name == "fp4_e2m1" else 0xA5
    codes, bytes_ = np.zeros((L_, K), np.int64), np.full((L_, -(-K // 32)), 127, np.int64)
    codes[ln, k], bytes_[ln, k // 32] = code, 200
    cbuf, sbuf = G.pack_layout(codes, bytes_, name)
    assert np.flatnonzero(cbuf).tolist() == [code_off] and cbuf[code_off] == code << shift
    assert np.flatnonzero(sbuf != 127).tolist() == [scale_off] and sbuf[scale_off] == 200


def test_decode_reference_at_the_ends_of_the_scale_range():
    """Byte 0 is 2^-127, byte 255 NaN, and the float32 view is the exact product rounded once, subnormals included."""
    for name in G.OPERAND_FORMATS:
        op = G.decode_sweep_operand(name)
        assert op.codes.shape == (256, 256) and np.array_equal(op.bytes[:, 0], np.arange(256)) and (op.bytes == op.bytes[:, :1]).all()
        assert np.array_equal(op.codes[7], np.arange(256) % (16 if name == "fp4_e2m1" else 256))
        d64, d32 = G.decode(op), G.decode(op, np.float32)
        one = G.code_of(name, 1.0)
        assert d64[0, one] == 2.0 ** -127 and d64[1, one] == 2.0 ** -126 and d64[254, one] == 2.0 ** 127 and np.isnan(d64[255]).all()
        assert d32.dtype == np.float32 and d32[0, one].view(np.uint32) == 0x00400000 and d32[1, one].view(np.uint32) == 0x00800000
        assert np.array_equal(np.isnan(d32), np.isnan(d64))
        sub = (np.abs(d64) < 2.0 ** -126) & (d64 != 0)
        assert sub.any() and np.array_equal(np.isinf(d32), np.isinf(d64) | (np.abs(d64) >= 2.0 ** 128))
        # one rounding to nearest even on the subnormal grid of 2^-149
        want = np.round(d64[sub] / 2.0 ** -149) * 2.0 ** -149
        assert np.array_equal(d32[sub].astype(np.float64), want)


# ------------------------------------------------------------------------------------ one term per output: codes and scale bytes
@pytest.mark.parametrize("pair", G.PAIRS, ids=lambda p: "-".join(p))
def test_code_sweep_products_are_float32(pair):
    """Every finite product of two codes is exactly a float32 and none is subnormal; the reference of the one-term GEMM is the
    outer product of the two decode tables, 0 * Inf = NaN rows and columns included, for every k0."""
    ta, tb = (ops.mx_decode_table(n).astype(np.float64) for n in pair)
    with np.errstate(all="ignore"):
        outer = ta[:, None] * tb[None, :]
    fin = np.isfinite(outer)
    assert np.array_equal(outer[fin].astype(np.float32).astype(np.float64), outer[fin])
    nz = np.abs(outer[fin & (outer != 0)])
    assert nz.min() >= 2.0 ** -32 > 2.0 ** -126 and nz.max() <= 57344.0 ** 2 < 2.0 ** 127      # 2.3e-10 and 3.3e9: fp8_e5m2 squared
    if pair == ("fp8_e5m2", "fp8_e5m2"):
        assert nz.min() == 2.0 ** -32 and nz.max() == 57344.0 ** 2
    special = {"fp4_e2m1": 0, "fp8_e4m3": 2, "fp8_e5m2": 8}                               # NaN and Inf codes
    assert [int((~np.isfinite(t)).sum()) for t in (ta, tb)] == [special[n] for n in pair]
    for k0 in G.CODE_K0S:
        ra, rb = G.code_sweep_operand(pair[0], k0), G.code_sweep_operand(pair[1], k0)
        assert ra.codes.shape == (ta.size, 160) and rb.codes.shape == (tb.size, 160)
        assert (ra.bytes == 127).all() and np.array_equal(np.flatnonzero(ra.codes.any(axis=0)), [k0])
        assert np.array_equal(ra.codes[:, k0], np.arange(ta.size)) and np.array_equal(rb.codes[:, k0], np.arange(tb.size))
        with np.errstate(all="ignore"):
            ref, _ = G.gemm_reference(ra, rb)
        assert np.array_equal(np.isnan(ref), np.isnan(outer)) and np.array_equal(ref[~np.isnan(ref)], outer[~np.isnan(outer)])
        if pair[0] == "fp8_e5m2":                                                         # 0 * Inf: part of the expectation
            assert np.isnan(ref[0x7C, 0]) and np.isnan(ref[0xFC, 0])
    assert {k0 & 127 < 64 for k0 in G.CODE_K0S} == {True, False} and max(G.CODE_K0S) >= 128


@pytest.mark.parametrize("pair", G.SCALE_PAIRS, ids=lambda p: "-".join(p))
def test_scale_sweep_classes(pair):
    """The one-term products +-2.25 * 2^(m + n - 254) under bytes m and n: the three classes are non-empty, the float32 range holds
    the first exactly, and pairs whose operands overflow or underflow float32 on their own lie in it."""
    ra, rb = G.scale_sweep_operand(pair[0], False), G.scale_sweep_operand(pair[1], True)
    assert np.array_equal(ra.bytes[:, G.SCALE_K0 // 32], np.arange(256)) and (np.delete(ra.bytes, G.SCALE_K0 // 32, axis=1) == 127).all()
    assert np.array_equal(G.decode(ra)[:255, G.SCALE_K0], 1.5 * np.ldexp(1.0, np.arange(255) - 127))
    assert np.array_equal(G.decode(rb)[:255, G.SCALE_K0], np.where(np.arange(255) & 1, -1.5, 1.5) * np.ldexp(1.0, np.arange(255) - 127))
    with np.errstate(all="ignore"):
        ref, _ = G.gemm_reference(ra, rb)
    m, n = np.arange(256)[:, None], np.arange(256)[None, :]
    assert np.array_equal(np.isnan(ref), (m == 255) | (n == 255))
    live = ~np.isnan(ref)
    want = np.where(n & 1, -2.25, 2.25) * np.ldexp(1.0, m + n - 254)
    assert np.array_equal(ref[live], want[live])
    normal, over, under = G.scale_sweep_classes(ref)
    assert normal.any() and over.any() and under.any() and np.array_equal(normal | over | under, live)
    assert np.array_equal(normal, live & (m + n >= 127) & (m + n <= 380))
    for pos in ((254, 1), (1, 254), (0, 254), (200, 60)):
        assert normal[pos], pos
    assert np.array_equal(ref[normal].astype(np.float32).astype(np.float64), ref[normal])
    assert 0 < G.decode(ra, np.float32)[0, G.SCALE_K0] < 2.0 ** -126      # (0, 254): A's scaled element alone is a float32 subnormal
