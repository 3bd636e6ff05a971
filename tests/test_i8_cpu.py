"""CPU tests of the packed int8 operands and the int8 GEMM (include/lq_hip.h: lq_i8_operand_* / lq_i8_gemm): the NumPy packer of the
documented layout (round trip, sizes, padding, a table of offsets worked out by hand from the header), the reference GEMM on a
hand-worked case with two periods, every refusal through the C surface (NULL stream: validation comes before any launch) and
through Python, and the condition of the data sets tests/test_gpu_i8.py runs on the device: every period sum fits int32."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_reference as G                                                                     # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402
from learned_quantization_amd.models import build_model                                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ_EINVAL, LQ_EALIGN = -1, -4
ENTRY_POINTS = ("lq_i8_operand_bytes", "lq_i8_operand_pack", "lq_i8_operand_quantize", "lq_i8_operand_decode", "lq_i8_gemm")


def _err():
    return _hip.load().lq_last_error().decode()


def _bytes(L_, K, block):
    cb, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = _hip.load().lq_i8_operand_bytes(L_, K, block, ctypes.byref(cb), ctypes.byref(sb))
    return rc, cb.value, sb.value


def test_entry_points_are_declared_exported_and_bound():
    lib = _hip.load()
    assert lib.lq_version() == 3                          # additions only
    header = open(os.path.join(ROOT, "include", "lq_hip.h")).read()
    declared = set(re.findall(r"\b(lq_[a-z0-9_]+)\s*\(", header))
    for fn in ENTRY_POINTS:
        assert fn in declared and hasattr(lib, fn) and fn in _hip.SIGNATURES, fn
    assert lq.i8_gemm is ops.i8_gemm and lq.i8_operand_pack is ops.i8_operand_pack and lq.i8_hardware is L.i8_hardware
    assert lq.I8Operand is ops.I8Operand and lq.i8_hardware_eligible is L.i8_hardware_eligible
    assert (ops.I8_BLOCK_UNIT, ops.I8_MAX_PERIOD) == (G.UNIT, G.MAX_PERIOD)


def test_sizes():
    """code_bytes = ceil(L / 16) ceil(K / 64) 1024; scale_bytes = nbs ceil(L / 16) 64."""
    for L_, K, block in ((1, 1, 0), (16, 64, 0), (17, 65, 64), (40, 70, 0), (10, 784, 64), (10, 784, 128), (4096, 4096, 0), (33, 513, 192),
                         (5, 70, 128)):
        LT, KT, nbs = G.layout_dims(L_, K, block)
        assert _bytes(L_, K, block) == (0, LT * KT * 1024, nbs * LT * 64), (L_, K, block)
        assert ops.i8_operand_bytes(L_, K, block) == (LT * KT * 1024, nbs * LT * 64)


# ------------------------------------------------------------------------------------------- the packer
# (LT, KT are those of L = 40, K = 130: 3 x 3 tiles) worked out by hand from the header: tile (line >> 4) * KT + (k >> 6), 1024 bytes
# each; inside it lane 16 * ((k & 63) >> 4) + (line & 15), 16 bytes each; byte k & 15
OFFSET_TABLE = [((0, 0), 0), ((1, 0), 16), ((0, 15), 15), ((0, 16), 256), ((5, 37), (32 + 5) * 16 + 5), ((0, 63), 48 * 16 + 15),
                ((15, 63), 1023), ((0, 64), 1024), ((0, 129), 2 * 1024 + 1), ((16, 0), 3 * 1024), ((17, 70), 4 * 1024 + 16 + 6),
                ((39, 129), 8 * 1024 + 7 * 16 + 1)]


@pytest.mark.parametrize("entry", OFFSET_TABLE, ids=lambda e: f"{e[0][0]}_{e[0][1]}")
def test_layout_table_worked_out_by_hand(entry):
    (line, k), want = entry
    assert G.code_offset(3, line, k) == want
    codes = np.zeros((40, 130), np.int8)
    codes[line, k] = -77
    cbuf, _ = G.pack_layout(dict(codes=codes, scales=np.ones((40, 1), np.float32), block=0))
    assert np.flatnonzero(cbuf).tolist() == [want] and cbuf[want] == 256 - 77


@pytest.mark.parametrize("L_,K,block", [(16, 64, 0), (40, 130, 0), (40, 130, 64), (7, 320, 128), (33, 70, 128)])
def test_layout_round_trip_sizes_and_padding(L_, K, block):
    rng = np.random.default_rng(L_ * K + block)
    op = G.random_operand(rng, L_, K, block)
    cbuf, sbuf = G.pack_layout(op)
    LT, KT, nbs = G.layout_dims(L_, K, block)
    assert (cbuf.size, sbuf.size * 4) == _bytes(L_, K, block)[1:]
    back = G.unpack_layout(cbuf, sbuf, L_, K, block)
    assert np.array_equal(back["codes"], op["codes"]) and np.array_equal(back["scales"], op["scales"])
    assert G.buffers_mismatch(cbuf, sbuf, op) is None
    # every byte that is no element is 0, every scale that is no line's is 1.0: the offsets are a bijection onto the rest
    full = dict(codes=np.full((L_, K), -1, np.int8), scales=np.full((L_, nbs), 7.0, np.float32), block=block)
    cb, sb = G.pack_layout(full)
    assert int((cb == 255).sum()) == L_ * K and int((cb == 0).sum()) == cb.size - L_ * K
    sb = sb.reshape(nbs, 16 * LT)
    assert (sb[:, :L_] == 7.0).all() and (sb[:, L_:] == 1.0).all()
    # a fragment is 16 consecutive k of one line
    frag = back["codes"][L_ - 1, 16:32]
    o = G.code_offset(KT, L_ - 1, 16)
    assert np.array_equal(cbuf[o:o + 16].view(np.int8), frag)
    cbuf[3] ^= 1
    assert "code bytes differ" in G.buffers_mismatch(cbuf, sbuf, op)


def test_int8_view():
    q = np.array([-128.0, -1.0, -0.0, 0.0, 1.0, 127.0, np.nan], np.float32)
    assert G.i8_view(q).tolist() == [-128, -1, 0, 0, 1, 127, 0]


# ------------------------------------------------------------------------------------------- the reference GEMM
def test_reference_gemm_on_a_hand_worked_case():
    """2 x 2 x 128, blocks of 64 on both sides: two periods.
    A row 0 = 1 | 2, row 1 = -1 | 3; B row 0 = 1 | 1, row 1 = 2 | -1 (first | second period, constant inside each)
    I_0 = [[64, 128], [-64, -128]], I_1 = [[128, -128], [192, -192]]
    sa = [[.5, .25], [1, 2]], sb = [[1, 4], [2, .5]]: t_0 = [[.5, 1], [1, 2]], t_1 = [[1, .125], [8, 1]]
    Y = [[32 + 128, 128 - 16], [-64 + 1536, -256 - 192]]"""
    a = dict(codes=np.repeat(np.array([[1, 2], [-1, 3]], np.int8), 64, axis=1), scales=np.array([[.5, .25], [1, 2]], np.float32), block=64)
    b = dict(codes=np.repeat(np.array([[1, 1], [2, -1]], np.int8), 64, axis=1), scales=np.array([[1, 4], [2, .5]], np.float32), block=64)
    sums = G.period_sums(a, b)
    assert [s[0] for s in sums] == [slice(0, 64), slice(64, 128)]
    assert sums[0][1].tolist() == [[64, 128], [-64, -128]] and sums[1][1].tolist() == [[128, -128], [192, -192]]
    assert G.gemm_reference(a, b).tolist() == [[160.0, 112.0], [1472.0, -448.0]]
    assert G.gemm_reference(a, b, np.array([0.5, -2.0], np.float32)).tolist() == [[160.5, 110.0], [1472.5, -450.0]]
    # A with one scale per line: the same two periods, sa constant
    a0 = dict(a, scales=np.array([[.5], [2]], np.float32), block=0)
    assert G.gemm_reference(a0, b).tolist() == [[32 + 256.0, 128 - 32.0], [-128 + 1536.0, -512 - 192.0]]
    # both per line: one period, one product
    b0 = dict(b, scales=np.array([[1], [.5]], np.float32), block=0)
    assert [s[0] for s in G.period_sums(a0, b0)] == [slice(0, 128)]
    assert G.gemm_reference(a0, b0).tolist() == [[96.0, 0.0], [256.0, -320.0]]


def test_reference_gemm_rounds_each_step_on_its_own():
    """One output, three periods with full-mantissa scales: the vectorised reference against the definition spelled out one float32
    operation at a time, and the order of the periods matters."""
    rng = np.random.default_rng(5)
    a, b = G.random_operand(rng, 1, 192, 64), G.random_operand(rng, 1, 192, 64)
    a["scales"] = (a["scales"] * np.float32(1.2345678)).astype(np.float32)
    y = np.float32(0.0)
    for p in range(3):
        I = int(a["codes"][0, 64 * p:64 * p + 64].astype(np.int64) @ b["codes"][0, 64 * p:64 * p + 64].astype(np.int64))
        t = np.float32(a["scales"][0, p] * b["scales"][0, p])
        y = np.float32(y + np.float32(np.float32(I) * t))
    assert G.gemm_reference(a, b)[0, 0].tobytes() == y.tobytes()
    ref64, terms = G.gemm_f64(a, b)
    assert abs(float(y) - ref64[0, 0]) <= 1e-6 * terms[0, 0]


def test_period_rules():
    assert G.period_of(0, 0, 784) == 784 and G.period_of(0, 64, 784) == 64 and G.period_of(128, 64, 784) == 64
    assert G.period_of(128, 128, 70) == 70 and G.period_of(0, 0, 65536) == 65536
    for bad in ((64, 192, 1000, False), (192, 64, 1000, False), (128, 192, 1000, True), (0, 0, 65600, True), (0, 65600 - 65600 % 64 + 64, 70000, True)):
        a_block, b_block, K, refused = bad
        if refused:
            with pytest.raises(ValueError):
                G.period_of(a_block, b_block, K)
            with pytest.raises(ValueError):
                ops.i8_period(a_block, b_block, K)
        else:
            assert G.period_of(a_block, b_block, K) == ops.i8_period(a_block, b_block, K) == 64


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    cb, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    size, pack, quant, dec, gemm = (lib.lq_i8_operand_bytes, lib.lq_i8_operand_pack, lib.lq_i8_operand_quantize,
                                    lib.lq_i8_operand_decode, lib.lq_i8_gemm)
    ok_pack = [p, p, -128, 127, 0, 160, 17, 0, 64, p, p, None]
    ok_gemm = [p, p, 0, p, p, 0, None, p, 16, 16, 16, 128, None]

    def with_(args, **at):
        args = list(args)
        for k, v in at.items():
            args[int(k[1:])] = v
        return args

    # the scale block, everywhere
    for bad in (-64, 1, 32, 63, 65, 100):
        assert size(16, 128, bad, ctypes.byref(cb), ctypes.byref(sb)) == LQ_EINVAL and "neither 0" in _err()
        assert quant(p, 5, 100, bad, p, p, None) == LQ_EINVAL and "neither 0" in _err()
        assert dec(p, p, 5, 100, bad, p, None) == LQ_EINVAL and "neither 0" in _err()
        assert gemm(*with_(ok_gemm, _2=bad)) == LQ_EINVAL and "neither 0" in _err()
        assert gemm(*with_(ok_gemm, _5=bad)) == LQ_EINVAL and "neither 0" in _err()
    # pack: the range, the group size, and everything lq_fq_forward_group refuses
    for qmin, qmax in ((0, 255), (-129, 127), (-128, 128), (-32768, 32767)):
        assert pack(*with_(ok_pack, _2=qmin, _3=qmax)) == LQ_EINVAL and "not inside [-128, 127]" in _err()
    for gs in (16, 32, 63, 65, 100, 159):
        assert pack(*with_(ok_pack, _8=gs)) == LQ_EINVAL and "neither the whole line" in _err()
    for gs in (64, 128, 160, 1000):                        # accepted sizes get past the check: they fail on the NULL codes next
        assert pack(*with_(ok_pack, _8=gs, _9=None)) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert pack(*with_(ok_pack, _2=5, _3=4)) == LQ_EINVAL and "qmin 5 > qmax 4" in _err()
    assert pack(*with_(ok_pack, _2=-(1 << 25))) == LQ_EINVAL and "outside +-2^24" in _err()
    for rounding in (-1, 2):
        assert pack(*with_(ok_pack, _4=rounding)) == LQ_EINVAL and "bad rounding" in _err()
    for axis in (-1, 2):
        assert pack(*with_(ok_pack, _7=axis)) == LQ_EINVAL and "bad axis" in _err()
    assert pack(*with_(ok_pack, _8=0)) == LQ_EINVAL and "group size 0 < 1" in _err()
    for R, C in ((0, 17), (160, 0), (-1, 17)):
        assert pack(*with_(ok_pack, _5=R, _6=C)) == LQ_EINVAL and "extents must be positive" in _err()
    assert pack(*with_(ok_pack, _5=1 << 20, _6=1 << 11)) == LQ_EINVAL and "not below 2^31" in _err()
    # the GEMM's periods
    # 192 = 3 * 64 is a multiple of the smaller block: the definition accepts the pair (it fails on the NULL codes next)
    assert gemm(*with_(ok_gemm, _2=64, _5=192, _11=1024, _0=None)) == LQ_EINVAL and "NULL" in _err()
    for a_block, b_block in ((128, 192), (192, 128), (320, 192)):
        assert gemm(*with_(ok_gemm, _2=a_block, _5=b_block, _11=1024)) == LQ_EINVAL and "multiple of the smaller" in _err()
    assert gemm(*with_(ok_gemm, _11=65600)) == LQ_EINVAL and "period of 65600" in _err()
    assert gemm(*with_(ok_gemm, _2=65536 + 64, _11=70000)) == LQ_EINVAL and "period of 65600" in _err()
    assert gemm(*with_(ok_gemm, _2=65536 + 64, _5=64, _11=70000, _0=None)) == LQ_EINVAL and "NULL" in _err()      # period 64: accepted
    assert gemm(*with_(ok_gemm, _11=65536, _0=None)) == LQ_EINVAL and "NULL" in _err()                            # the limit itself
    # null pointers
    assert size(16, 128, 0, None, ctypes.byref(sb)) == LQ_EINVAL and "NULL" in _err()
    assert size(16, 128, 0, ctypes.byref(cb), None) == LQ_EINVAL and "NULL" in _err()
    for k, name in ((0, "'P'"), (1, "'s'"), (9, "'codes'"), (10, "'scales'")):
        assert pack(*with_(ok_pack, **{f"_{k}": None})) == LQ_EINVAL and f"{name} is NULL" in _err()
    assert quant(None, 5, 100, 0, p, p, None) == LQ_EINVAL and "'X' is NULL" in _err()
    assert quant(p, 5, 100, 0, None, p, None) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert quant(p, 5, 100, 0, p, None, None) == LQ_EINVAL and "'scales' is NULL" in _err()
    assert dec(None, p, 5, 100, 0, p, None) == LQ_EINVAL and "'codes' is NULL" in _err()
    assert dec(p, None, 5, 100, 0, p, None) == LQ_EINVAL and "'scales' is NULL" in _err()
    assert dec(p, p, 5, 100, 0, None, None) == LQ_EINVAL and "'out' is NULL" in _err()
    for k in (0, 1, 3, 4, 7):                              # every pointer of the GEMM but the bias
        assert gemm(*with_(ok_gemm, **{f"_{k}": None})) == LQ_EINVAL and "NULL" in _err(), k
    # extents, the leading dimension
    for L_, K in ((0, 128), (16, 0), (-1, 128)):
        assert size(L_, K, 0, ctypes.byref(cb), ctypes.byref(sb)) == LQ_EINVAL and "extents must be positive" in _err()
        assert quant(p, L_, K, 0, p, p, None) == LQ_EINVAL and "extents must be positive" in _err()
        assert dec(p, p, L_, K, 0, p, None) == LQ_EINVAL and "extents must be positive" in _err()
        assert gemm(*with_(ok_gemm, _9=L_, _11=K)) == LQ_EINVAL and "extents must be positive" in _err()
        assert gemm(*with_(ok_gemm, _10=L_, _11=K)) == LQ_EINVAL and "extents must be positive" in _err()
    assert size(1 << 20, 1 << 11, 0, ctypes.byref(cb), ctypes.byref(sb)) == LQ_EINVAL and "not below 2^31" in _err()
    for ldy in (15, 0, -1):
        assert gemm(*with_(ok_gemm, _8=ldy)) == LQ_EINVAL and "is below N" in _err()
    assert gemm(*with_(ok_gemm, _9=1 << 20, _11=1 << 11)) == LQ_EINVAL and "not below 2^31" in _err()
    assert gemm(*with_(ok_gemm, _9=65535 * 64 + 1, _11=64, _8=16)) == LQ_EINVAL and "above 65535 * 64" in _err()
    # alignment
    assert pack(*with_(ok_pack, _9=p + 4)) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert pack(*with_(ok_pack, _10=p + 4)) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()
    assert pack(*with_(ok_pack, _0=p + 2)) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert quant(p + 2, 5, 100, 0, p, p, None) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert quant(p, 5, 100, 0, p + 8, p, None) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert dec(p, p + 8, 5, 100, 0, p, None) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()
    assert dec(p, p, 5, 100, 0, p + 1, None) == LQ_EALIGN and "not 4-byte aligned" in _err()
    assert gemm(*with_(ok_gemm, _3=p + 8)) == LQ_EALIGN and "codes is not 16-byte aligned" in _err()
    assert gemm(*with_(ok_gemm, _1=p + 4)) == LQ_EALIGN and "scales is not 16-byte aligned" in _err()
    assert gemm(*with_(ok_gemm, _6=p + 1)) == LQ_EALIGN and "bias is not 4-byte aligned" in _err()
    assert gemm(*with_(ok_gemm, _7=p + 2)) == LQ_EALIGN and "not 4-byte aligned" in _err()


def _dense(**kw):
    return L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), input_shape=70, **kw)


def test_refusals_of_the_python_surface():
    P = torch.zeros(160, 17)
    for rng_ in ((0, 255), (-129, 0), (-128, 128)):
        with pytest.raises(ValueError, match=re.escape("not inside [-128, 127]")):
            ops.i8_operand_pack(P, torch.ones(3, 17), *rng_, 64)
    with pytest.raises(ValueError, match="qmin <= qmax"):
        ops.i8_operand_pack(P, torch.ones(3, 17), 3, 2, 64)
    with pytest.raises(ValueError, match="rounding must be one of"):
        ops.i8_operand_pack(P, torch.ones(3, 17), -8, 7, 64, rounding="up")
    for block in (-64, 1, 32, 100, 64.5, True):
        with pytest.raises(ValueError, match="a scale block is 0"):
            ops.i8_operand_quantize(P, block)
        with pytest.raises(ValueError, match="a scale block is 0"):
            ops.i8_operand_bytes(16, 128, block)
        with pytest.raises(ValueError, match="a scale block is 0"):
            L.i8_hardware(torch.nn.Linear(2, 2), act_block=block)
    with pytest.raises(ValueError, match="x must be a matrix"):
        ops.i8_operand_quantize(torch.zeros(2, 3, 4))
    u8, f32 = torch.zeros(16, dtype=torch.uint8), torch.zeros(16)
    op = lambda K, block=0: ops.I8Operand(u8, f32, 16, K, block)
    with pytest.raises(ValueError, match="different K: 128 and 192"):
        ops.i8_gemm(op(128), op(192))
    with pytest.raises(ValueError, match="multiple of the smaller"):
        ops.i8_gemm(op(1024, 128), op(1024, 192))
    with pytest.raises(ValueError, match="period of 65600"):
        ops.i8_gemm(op(65600), op(65600))
    with pytest.raises(ValueError, match="a scale block is 0"):
        ops.i8_operand_decode(op(128, 48))
    # check_i8_operand_layer names its reason
    for args, needle in (((None, "scalar"), "needs a layer with bits or q_range"),
                         (((0, 255), "scalar"), "not inside [-128, 127]"),
                         (((-8, 7), "groupwise", 64, True), "asymmetric=True"),
                         (((-8, 7), "rowwise"), 'orientation="rowwise"'),
                         (((-8, 7), "channelwise"), "orientation='channelwise'"),
                         (((-8, 7), "groupwise", 64, False, "fp4_e2m1"), "a microscaling layer"),
                         (((-8, 7), "groupwise", 32), "group_size=32"),
                         (((-8, 7), "groupwise", 100, False, None, 101), "group_size=100")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            ops.check_i8_operand_layer(*args)
    assert ops.check_i8_operand_layer((-8, 7), "groupwise", 100, False, None, 100) == (-8, 7)
    assert ops.check_i8_operand_layer((-128, 127), "columnwise") == (-128, 127)
    # layers
    ste = dict(scale_gradient="ste")
    for kw, needle in ((dict(), "needs a layer with bits or q_range"),
                       (dict(bits=8, signed=False, **ste), "not inside [-128, 127]"),
                       (dict(bits=9, **ste), "not inside [-128, 127]"),
                       (dict(orientation="groupwise", group_size=64, bits=4, asymmetric=True, **ste), "asymmetric=True"),
                       (dict(orientation="rowwise", bits=8, **ste), 'orientation="rowwise"'),
                       (dict(orientation="groupwise", element_format="fp4_e2m1"), "a microscaling layer"),
                       (dict(orientation="groupwise", group_size=32, bits=4, **ste), "group_size=32")):
        d = _dense(**kw)
        with pytest.raises(ValueError, match=re.escape(needle)):
            d.i8_operand()
        with pytest.raises(ValueError, match=re.escape(needle)):
            d.call_i8(torch.zeros(3, 70))
        assert not L.i8_hardware_eligible(d)
    unbuilt = L.CustomDenseLayer(units=4, bits=8, **ste)
    with pytest.raises(ValueError, match="not built yet"):
        unbuilt.i8_operand()
    assert not L.i8_hardware_eligible(unbuilt)
    with pytest.raises(ValueError, match="a scale block is 0"):
        _dense(bits=8, **ste).call_i8(torch.zeros(3, 70), act_block=32)
    for kw in (dict(bits=8), dict(bits=4, orientation="columnwise"), dict(bits=4, orientation="groupwise", group_size=64),
               dict(q_range=(-7, 7), orientation="groupwise", group_size=128)):
        assert L.i8_hardware_eligible(_dense(**kw, **ste)), kw
    assert not L.i8_hardware_eligible(torch.nn.Linear(2, 2))
    # the context manager switches eligible layers only and restores them
    m = build_model("mnist", mode="ste", value=0.0, bits=8, orientation="columnwise")
    dense = [x for x in L.custom_layers_of(m) if isinstance(x, L.CustomDenseLayer)]
    assert dense and all(L.i8_hardware_eligible(x) for x in dense)
    assert all(getattr(x, "_i8_hw", None) is None for x in dense)


def test_driver_refusal():
    from learned_quantization_amd import train
    with pytest.raises(SystemExit):
        train.main(["--config", "mnist", "--mode", "ste", "--i8-eval"])                       # the unbounded quantizer: no eligible layer


# ------------------------------------------------------------------------------------------- conditions of the GPU data sets
def test_every_period_sum_of_the_gpu_data_sets_fits_int32():
    cases = [c[:2] for c in G.all_gemm_cases()] + [G.one_hot_case(k) for k in (0, 63, 64, 127)] + [G.code_sweep_case()]
    for a, b in cases:
        for ks, I, mag in G.period_sums(a, b):
            assert int(mag.max()) < 2 ** 31, (a["codes"].shape, b["codes"].shape, ks)
    # the extremes: constant operands, so one row and one column stand for all
    for bcode, want in ((-128, 2 ** 30), (127, -128 * 127 * 65536)):
        a, b = G.extreme_case(bcode)
        total = int(a["codes"][0].astype(np.int64) @ b["codes"][0].astype(np.int64))
        assert total == want and -2 ** 31 <= total < 2 ** 31 and int(np.abs(a["codes"][0].astype(np.int64)) @ np.abs(b["codes"][0].astype(np.int64))) < 2 ** 31
        assert float(np.float32(total)) == total           # the int -> float conversion of the extremes is exact


def test_gpu_data_sets_hold_what_they_promise():
    for R, C, axis, gs in G.PACK_CASES:
        P, s = G.pack_case(R, C, axis, gs)
        assert np.isnan(P).sum() == 1 and np.isnan(s).sum() == 1
        op = G.operand_of_parameter(P, s, -8, 7, axis, gs, "nearest")
        assert op["codes"].min() == -8 and op["codes"].max() == 7 and op["block"] == (0 if gs >= (R if axis == 0 else C) else gs)
        out = G.fq_out_of_parameter(P, s, -8, 7, axis, gs, "nearest")
        dec = G.decode(op)
        dec = dec.T if axis == 0 else dec
        elem = ~np.isnan(P)                                    # equal as values (-0.0 == +0.0), NaN under the NaN scale ...
        assert np.array_equal(dec[elem], out[elem], equal_nan=True) and np.isnan(out[elem]).sum() > 0
        assert (dec[~elem] == 0).all() and np.isnan(out[~elem]).all()      # ... and the NaN element, whose code is 0, decodes as 0
    for M, K in G.QUANT_SHAPES:
        x = G.quantize_case(M, K)
        for block in G.QUANT_BLOCKS:
            op = G.operand_of_activation(x, block)
            nbs = G.layout_dims(M, K, block)[2]
            assert op["scales"].shape == (M, nbs) and op["block"] == (0 if block == 0 or block >= K else block)
            assert (op["scales"][0] == np.float32(G.MIN_SCALE)).all() and not op["codes"][0].any()      # the zero row
            assert np.isnan(op["scales"][1]).sum() == (1 if nbs == 1 else 2)                           # the NaN and the Inf
            span = block if nbs > 1 else K
            for g in np.flatnonzero(np.isnan(op["scales"][1])):
                assert not op["codes"][1, g * span:(g + 1) * span].any()
            assert (op["scales"][M - 1] == np.float32(G.MIN_SCALE)).all() and not op["codes"][M - 1].any()      # the row of 1e-40
            if M > 3:
                assert np.isfinite(op["scales"][2:M - 1]).all() and np.abs(op["codes"][2:M - 1]).max() == 127
