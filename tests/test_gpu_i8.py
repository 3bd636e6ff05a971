"""The packed int8 operands and the int8 GEMM on the device (include/lq_hip.h: lq_i8_operand_* / lq_i8_gemm), against
tests/_i8_reference.py.  The integer sums are exact and the definition states every rounding, so every comparison here is bit for
bit or byte for byte; tests/_bounds.py's yardstick against a float64 product is a second, independent check only.

 1 lane map     one-hot operands for every k = 0 .. 127 (A: m + 1 in column k, B: 3 n - 20 in column k: a row / column swap shows) and
                every code -128 .. 127 against {-128, -1, 1, 127}, one term per output
 2 pack         buffers == the NumPy packer (padding included); decode == fq_forward_group's out as values
 3 quantize     buffers == the composition reference == the device composition (scale_init_group, then fq_forward_group's int8 view)
 4 gemm         == the NumPy definition: every shape class of the 64 x 64 block / 32 x 32 wave geometry, six block pairs with a ragged
                last period, with and without bias, out= with a row stride, two runs
 5 extremes     period sums of +2^30 and -128 * 127 * 65536; NaN scales spoil their row or column only
 6 memory       guard bands around every output; operands cut out of a NaN-filled buffer
 7 capture      the four entry points in one graph
 8 layers       call_i8 on exact data; i8_hardware on the MNIST model, 8 bit and 4 bit with groups of 64

The conditions of the data sets (every period sum fits int32, the planted NaN / Inf / zero rows) are asserted in
tests/test_i8_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_reference as G                                                                     # noqa: E402
from _arena import SENTINEL_WORD, Arena                                                       # noqa: E402
from _bounds import assert_within_terms                                                       # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

pytestmark = pytest.mark.gpu
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _upload(op, dev):
    """A reference operand as the device's, through the NumPy packer."""
    cbuf, sbuf = G.pack_layout(op)
    return ops.I8Operand(_t(cbuf, dev), _t(sbuf, dev), op["codes"].shape[0], op["codes"].shape[1], op["block"])


def _same_bits(got, ref, what):
    """float32 arrays equal bit for bit; a NaN equals a NaN whatever its payload."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, f"{what}: shapes {got.shape} {ref.shape}"
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        i = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} differ, first at {i}: got {got[i]!r} want {ref[i]!r}")


_CASES = {}


def _gemm_case(key):
    """(a, b, bias, reference without bias, reference with bias), computed once per case."""
    if key not in _CASES:
        a, b, bias = G.gemm_case(*key)
        _CASES[key] = (a, b, bias, G.gemm_reference(a, b), G.gemm_reference(a, b, bias))
    return _CASES[key]


# -------------------------------------------------------------------------------------------------------------- 1 lane map
def test_one_hot_sweep_over_every_k(dev):
    """For every k of two K steps: Y[m][n] = (m + 1) * (3 n - 20), the single term.  Both operands packed by the documented rule: a k
    that the two sides of the instruction took from different (lane >> 4, byte) pairs would give 0, a row / column swap the
    transpose."""
    want = (np.arange(16)[:, None] + 1) * (3 * np.arange(16)[None, :] - 20)
    for k in range(128):
        a, b = G.one_hot_case(k)
        y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev)))
        assert np.array_equal(y, want.astype(np.float32)), f"k = {k}"


def test_every_code_against_the_corner_codes(dev):
    a, b = G.code_sweep_case()
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev)))
    want = np.arange(-128, 128)[:, None] * np.array([-128, -1, 1, 127])[None, :]
    assert np.array_equal(y, want.astype(np.float32))
    _same_bits(y, G.gemm_reference(a, b), "code sweep")


# -------------------------------------------------------------------------------------------------------------- 2 pack
@pytest.mark.parametrize("qrange", G.PACK_RANGES, ids=_ids)
@pytest.mark.parametrize("rounding", ["floor", "nearest"])
@pytest.mark.parametrize("case", G.PACK_CASES, ids=_ids)
def test_pack_is_the_reference_operand_and_decodes_to_the_fake_quantised_parameter(dev, case, rounding, qrange):
    R, C, axis, gs = case
    qmin, qmax = qrange
    P, s = G.pack_case(R, C, axis, gs)
    ref = G.operand_of_parameter(P, s, qmin, qmax, axis, gs, rounding)
    op = ops.i8_operand_pack(_t(P, dev), _t(s, dev), qmin, qmax, gs, rounding)
    assert (op.lines, op.K, op.block) == (ref["codes"].shape[0], ref["codes"].shape[1], ref["block"])
    assert (op.codes.numel(), op.scales.numel() * 4) == ops.i8_operand_bytes(op.lines, op.K, op.block)
    bad = G.buffers_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, bad
    out, q = ops.fq_forward_group(_t(P, dev), _t(s, dev), qmin, qmax, gs, q_dtype=torch.int8, rounding=rounding)
    got = G.unpack_layout(_np(op.codes), _np(op.scales), op.lines, op.K, op.block)
    assert np.array_equal(got["codes"], _np(q).T if axis == 0 else _np(q)), "the codes are not fq_forward_group's int8 view"
    dec = _np(ops.i8_operand_decode(op))
    _same_bits(dec, G.decode(ref), "decode")
    dec, out = (dec.T if axis == 0 else dec), _np(out)
    elem = ~np.isnan(P)      # equal as values: -0.0 == +0.0; NaN under the NaN scale; the NaN element has code 0 and decodes as 0
    assert np.array_equal(dec[elem], out[elem], equal_nan=True) and (dec[~elem] == 0).all()


# -------------------------------------------------------------------------------------------------------------- 3 quantize
@pytest.mark.parametrize("block", G.QUANT_BLOCKS)
@pytest.mark.parametrize("shape", G.QUANT_SHAPES, ids=_ids)
def test_quantize_is_scale_init_then_forward(dev, shape, block):
    M, K = shape
    x = G.quantize_case(M, K)
    ref = G.operand_of_activation(x, block)
    xd = _t(x, dev)
    op = ops.i8_operand_quantize(xd, block)
    assert (op.lines, op.K, op.block) == (M, K, block)
    bad = G.buffers_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, bad
    # the device composition: scale_init_group with ABSMAX, then fq_forward_group's integers, through the packer
    gs = block if block else K
    s = torch.empty(G.scale_shape(M, K, 1, min(gs, K)), device=dev)
    ops.scale_init_group(xd, s, -127, 127, gs, "absmax", rounding="nearest", min_value=G.MIN_SCALE)
    _, q = ops.fq_forward_group(xd, s, -127, 127, gs, q_dtype=torch.int8, rounding="nearest")
    comp = dict(codes=_np(q), scales=_np(s), block=ref["block"])
    bad = G.buffers_mismatch(_np(op.codes), _np(op.scales), comp)
    assert bad is None, "against the device composition: " + str(bad)
    packed = ops.i8_operand_pack(xd, s, -127, 127, gs, "nearest")
    assert torch.equal(packed.codes, op.codes) and torch.equal(packed.scales.view(torch.int32), op.scales.view(torch.int32))
    # an unaligned base takes the scalar form: the same bytes
    shifted = torch.empty(M * K + 1, device=dev)[1:].view(M, K).copy_(xd)
    op1 = ops.i8_operand_quantize(shifted, block)
    assert torch.equal(op1.codes, op.codes) and torch.equal(op1.scales.view(torch.int32), op.scales.view(torch.int32))


def test_quantize_rows_longer_than_the_register_cache(dev):
    """Rows of 4100 and 4160 elements: past the 4096 (16-byte loads) and 1024 (4-byte loads) a team keeps in registers."""
    for M, K in G.LONG_QUANT_SHAPES:
        x = np.random.default_rng(K).normal(0.0, 1.0, (M, K)).astype(np.float32)
        x[0, K - 2] = 7.5                                  # the row's maximum lies in the tail
        for xd in (_t(x, dev), torch.empty(M * K + 1, device=dev)[1:].view(M, K).copy_(_t(x, dev))):
            op = ops.i8_operand_quantize(xd, 0)
            bad = G.buffers_mismatch(_np(op.codes), _np(op.scales), G.operand_of_activation(x, 0))
            assert bad is None, bad


# -------------------------------------------------------------------------------------------------------------- 4 gemm
_GEMM_KEYS = [s + (0, 0) for s in G.GEMM_SHAPES] + [G.BLOCK_PAIR_SHAPE + p for p in G.BLOCK_PAIRS if p != (0, 0)] + \
    [G.BLOCK_PAIR_SHAPE + (0, 0)] + G.EXTRA_GEMM_KEYS


@pytest.mark.parametrize("key", _GEMM_KEYS, ids=_ids)
def test_gemm_is_the_definition_bit_for_bit(dev, key):
    a, b, bias, ref, ref_bias = _gemm_case(key)
    da, db = _upload(a, dev), _upload(b, dev)
    y = ops.i8_gemm(da, db)
    _same_bits(_np(y), ref, f"gemm {key}")
    yb = ops.i8_gemm(da, db, _t(bias, dev))
    _same_bits(_np(yb), ref_bias, f"gemm {key} with bias")
    assert torch.equal(ops.i8_gemm(da, db, _t(bias, dev)).view(torch.int32), yb.view(torch.int32)), "two runs differ"
    ref64, terms = G.gemm_f64(a, b, bias)
    assert_within_terms(_np(yb), ref64, terms, f"gemm {key} against the float64 product of the decoded operands")
    # the device's decode agrees with the reference's: the two checks above stand on the same operands
    _same_bits(_np(ops.i8_operand_decode(da)), G.decode(a), "decode of A")


def test_gemm_out_with_a_row_stride(dev):
    key = (19, 21, 160, 0, 0)
    a, b, bias, _, ref_bias = _gemm_case(key)
    M, N = 19, 21
    da, db, bd = _upload(a, dev), _upload(b, dev), _t(bias, dev)
    buf = torch.full((M, N + 3), -7.0, device=dev)
    out = buf[:, :N]
    assert ops.i8_gemm(da, db, bd, out=out) is out
    _same_bits(_np(buf[:, :N]), ref_bias, "out=")
    assert (buf[:, N:] == -7.0).all()
    for bad in (torch.empty((M, N + 1), device=dev), torch.empty((N, M), device=dev), torch.empty((M, N), dtype=torch.float64, device=dev),
                torch.empty((N, M), device=dev).t(), torch.empty((M, 2 * N), device=dev)[:, ::2]):
        with pytest.raises(ValueError, match="out must be a float32 device matrix"):
            ops.i8_gemm(da, db, bd, out=bad)
    with pytest.raises(ValueError, match="bias must have shape"):
        ops.i8_gemm(da, db, torch.zeros(N + 1, device=dev))


# -------------------------------------------------------------------------------------------------------------- 5 extremes
@pytest.mark.parametrize("bcode,total", [(-128, 2 ** 30), (127, -128 * 127 * 65536)])
def test_extreme_period_sums(dev, bcode, total):
    a, b = G.extreme_case(bcode)
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev)))
    assert np.array_equal(y, np.full((16, 16), float(total), np.float32))


def test_nan_scales_spoil_their_row_or_column_only(dev):
    for blocks in ((0, 0), (64, 128)):
        a, b, bias = G.gemm_case(37, 21, 320, *blocks, seed=1)
        a["scales"][5, -1] = np.nan                        # the last scale block of row 5
        b["scales"][17, 0] = np.nan                        # the first of column 17
        ref = G.gemm_reference(a, b, bias)
        y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev), _t(bias, dev)))
        spoiled = np.zeros((37, 21), bool)
        spoiled[5, :] = spoiled[:, 17] = True
        assert np.isnan(y[spoiled]).all() and np.isfinite(y[~spoiled]).all()
        _same_bits(y, ref, f"NaN scales {blocks}")
        dec = _np(ops.i8_operand_decode(_upload(a, dev)))
        assert np.isnan(dec).any(axis=1).tolist() == [m == 5 for m in range(37)]


# -------------------------------------------------------------------------------------------------------------- 6 memory contract
@pytest.mark.parametrize("case", [(160, 17, 0, 64), (33, 320, 1, 128), (70, 40, 0, 70)], ids=_ids)
def test_memory_contract_of_pack(dev, case):
    """Guard bands around the code and scale buffers at their exact sizes; P and s 4 bytes off the 16-byte grid.  Range [-8, 7]: no
    four codes spell the arena's sentinel word."""
    R, C, axis, gs = case
    P, s = G.pack_case(R, C, axis, gs)
    ref = G.operand_of_parameter(P, s, -8, 7, axis, gs, "nearest")
    cb, sb = ops.i8_operand_bytes(*ref["codes"].shape, ref["block"])
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=4, row_bytes=C * 4)
    ar.add("s", "in", data=s, residue=4)
    ar.add("codes", "out", nbytes=cb)
    ar.add("scales", "out", nbytes=sb)
    ar.build()
    _hip.check(_hip.load().lq_i8_operand_pack(ar.ptr("P"), ar.ptr("s"), -8, 7, 1, R, C, axis, gs, ar.ptr("codes"), ar.ptr("scales"),
                                              _hip.stream_ptr(dev)), "lq_i8_operand_pack")
    torch.cuda.synchronize()
    ar.check(f"pack {case}")
    bad = G.buffers_mismatch(ar.numpy("codes", np.uint8), ar.numpy("scales", np.float32), ref)
    assert bad is None, bad


@pytest.mark.parametrize("block", [0, 64])
@pytest.mark.parametrize("shape", [(3, 70), (37, 784)], ids=_ids)
def test_memory_contract_of_quantize_and_decode(dev, shape, block):
    M, K = shape
    x = G.quantize_case(M, K)
    ref = G.operand_of_activation(x, block)
    cb, sb = ops.i8_operand_bytes(M, K, block)
    ar = Arena(dev)
    ar.add("X", "in", data=x, residue=4, row_bytes=K * 4)
    ar.add("codes", "some", nbytes=cb)                     # a run of saturated codes 127 would be the sentinel word
    ar.add("scales", "out", nbytes=sb)
    ar.add("D", "some", nbytes=M * K * 4, residue=4, row_bytes=K * 4)
    ar.build()
    lib = _hip.load()
    _hip.check(lib.lq_i8_operand_quantize(ar.ptr("X"), M, K, block, ar.ptr("codes"), ar.ptr("scales"), _hip.stream_ptr(dev)), "quantize")
    _hip.check(lib.lq_i8_operand_decode(ar.ptr("codes"), ar.ptr("scales"), M, K, block, ar.ptr("D"), _hip.stream_ptr(dev)), "decode")
    torch.cuda.synchronize()
    ar.check(f"quantize {shape} {block}")
    bad = G.buffers_mismatch(ar.numpy("codes", np.uint8), ar.numpy("scales", np.float32), ref)
    assert bad is None, bad
    _same_bits(ar.numpy("D", np.float32).reshape(M, K), G.decode(ref), "decode")


@pytest.mark.parametrize("key", [(19, 21, 160, 0, 0), (37, 10, 784, 0, 0), (81, 70, 192, 64, 128)], ids=_ids)
def test_memory_contract_of_gemm(dev, key):
    """Guard bands around Y with ldy = N + 3: the three columns between the rows keep the sentinel; the bias 4 bytes off the grid."""
    M, N, K = key[:3]
    a, b, bias, _, ref_bias = _gemm_case(key)
    (ac, as_), (bc, bs) = G.pack_layout(a), G.pack_layout(b)
    ldy = N + 3
    ar = Arena(dev)
    for name, data in (("a_codes", ac), ("a_scales", as_), ("b_codes", bc), ("b_scales", bs)):
        ar.add(name, "in", data=data)
    ar.add("bias", "in", data=bias, residue=4)
    ar.add("Y", "some", nbytes=((M - 1) * ldy + N) * 4, residue=4, row_bytes=ldy * 4)
    ar.build()
    _hip.check(_hip.load().lq_i8_gemm(ar.ptr("a_codes"), ar.ptr("a_scales"), a["block"], ar.ptr("b_codes"), ar.ptr("b_scales"), b["block"],
                                      ar.ptr("bias"), ar.ptr("Y"), ldy, M, N, K, _hip.stream_ptr(dev)), "lq_i8_gemm")
    torch.cuda.synchronize()
    ar.check(f"gemm {key}")
    flat = np.concatenate([ar.numpy("Y", np.uint32), np.full(3, SENTINEL_WORD, np.uint32)]).reshape(M, ldy)
    assert (flat[:, N:] == SENTINEL_WORD).all(), "the columns between the rows of Y were written"
    _same_bits(np.ascontiguousarray(flat[:, :N]).view(np.float32), ref_bias, "Y in the arena")


def test_operands_cut_out_of_a_nan_filled_buffer(dev):
    """The four buffers lie back to back (on the 16-byte grid) inside one buffer of NaN: a fragment or scale load past an operand's
    extent would multiply NaN bytes or scale by NaN."""
    key = (81, 70, 192, 64, 128)
    a, b, bias, ref, _ = _gemm_case(key)
    parts = [p for op in (a, b) for p in G.pack_layout(op)]
    sizes = [p.nbytes for p in parts]
    assert all(n % 16 == 0 for n in sizes)
    pool = torch.full((sum(sizes) // 4 + 64,), float("nan"), device=dev)
    raw, at, views = pool.view(torch.uint8), 64, []
    for p in parts:
        raw[at:at + p.nbytes].copy_(_t(p.reshape(-1).view(np.uint8), dev))
        views.append(raw[at:at + p.nbytes])
        at += p.nbytes
    da = ops.I8Operand(views[0], views[1].view(torch.float32), 81, 192, 64)
    db = ops.I8Operand(views[2], views[3].view(torch.float32), 70, 192, 128)
    _same_bits(_np(ops.i8_gemm(da, db)), ref, "operands inside a NaN-filled buffer")
    _same_bits(_np(ops.i8_operand_decode(db)), G.decode(b), "decode inside a NaN-filled buffer")


# -------------------------------------------------------------------------------------------------------------- 7 capture
def test_capture_and_replay(dev):
    """pack -> quantize -> gemm -> decode, one launch each, captured into pre-allocated buffers in one graph and replayed once; the
    poisoned outputs then equal the eager results bit for bit."""
    M, N, K, gs = 19, 21, 160, 64
    rng = np.random.default_rng(11)
    x, W = _t(rng.normal(0, 1, (M, K)).astype(np.float32), dev), _t(rng.normal(0, 1, (K, N)).astype(np.float32), dev)
    sw, bias = _t(np.exp2(rng.uniform(-7, -5, (3, N))).astype(np.float32), dev), _t(rng.normal(0, 1, N).astype(np.float32), dev)
    ea, eb = ops.i8_operand_quantize(x, 0), ops.i8_operand_pack(W, sw, -8, 7, gs, "nearest")
    eager = [eb.codes, eb.scales, ea.codes, ea.scales, ops.i8_gemm(ea, eb, bias), ops.i8_operand_decode(ea)]
    (acb, asb), (bcb, bsb) = ops.i8_operand_bytes(M, K, 0), ops.i8_operand_bytes(N, K, gs)
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)      # noqa: E731
    ac, as_, bc, bs = u8(acb), u8(asb), u8(bcb), u8(bsb)
    Y, D = torch.empty((M, N), device=dev), torch.empty((M, K), device=dev)
    outs = [bc, bs, ac, as_, Y, D]
    lib, p = _hip.load(), _hip.ptr

    def launch():
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_i8_operand_pack(p(W), p(sw), -8, 7, 1, K, N, 0, gs, p(bc), p(bs), st), "pack")
        _hip.check(lib.lq_i8_operand_quantize(p(x), M, K, 0, p(ac), p(as_), st), "quantize")
        _hip.check(lib.lq_i8_gemm(p(ac), p(as_), 0, p(bc), p(bs), gs, p(bias), p(Y), N, M, N, K, st), "gemm")
        _hip.check(lib.lq_i8_operand_decode(p(ac), p(as_), M, K, 0, p(D), st), "decode")

    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for o in outs:
        o.fill_(0xEE if o.dtype == torch.uint8 else -7.0)
    g.replay()
    torch.cuda.synchronize(dev)
    for k, (o, e) in enumerate(zip(outs, eager)):
        assert torch.equal(o.view(torch.uint8).reshape(-1), e.contiguous().view(torch.uint8).reshape(-1)), f"output {k} of the replay differs"
    ref = G.gemm_reference(G.operand_of_activation(_np(x), 0), G.operand_of_parameter(_np(W), _np(sw), -8, 7, 0, gs, "nearest"), _np(bias))
    _same_bits(_np(Y), ref, "captured gemm")


# -------------------------------------------------------------------------------------------------------------- 8 layers
@pytest.mark.parametrize("orientation", ["scalar", "columnwise"])
def test_call_i8_on_exact_data_is_the_float64_linear_layer(dev, orientation):
    """Integer-valued inputs up to 127 with a maximum of exactly 127 in every row, a kernel on its own grid under power-of-two
    scales: the codes are the inputs and the kernel's integers themselves, and one period covers K, so the layer's result has ONE
    rounding of the product and one of the bias.  LQ_INIT_ABSMAX carries a margin of 1 + 2^-22: the activation scale of such a row
    is exactly that number, not 1, so the float64 yardstick is F.linear of the inputs times 1 + 2^-22 (exact in float64) with the
    fake-quantised kernel (exact); rounding it to float32 once and adding the fake-quantised bias in float32 are the two roundings
    the definition states.  Bit for bit."""
    rng = np.random.default_rng(3)
    fan_in, units, M = 200, 24, 37
    layer = lq.CustomDenseLayer(units=units, orientation=orientation, bits=8, scale_gradient="ste", initializer=lq.RandomNormal(seed=5),
                                input_shape=fan_in, device=dev)
    e = rng.integers(-9, -3, units if orientation == "columnwise" else 1)
    sw = np.exp2(e).astype(np.float32)
    qw = rng.integers(-128, 128, (fan_in, units))
    with torch.no_grad():
        layer.nested_q_w_layer.scale.copy_(_t(sw.reshape(tuple(layer.nested_q_w_layer.scale.shape)), dev))
        layer.W.copy_(_t((qw * sw[None, :]).astype(np.float32), dev))
        layer.nested_q_b_layer.scale.fill_(2.0 ** -6)
        layer.b.copy_(_t((rng.integers(-128, 128, units) * 2.0 ** -6).astype(np.float32), dev))
        fq_w, fq_b = layer.nested_q_w_layer(layer.W), layer.nested_q_b_layer(layer.b)
    assert torch.equal(fq_w, layer.W) and torch.equal(fq_b, layer.b), "the kernel is not on its own grid"
    x = rng.integers(-127, 128, (M, fan_in)).astype(np.float32)
    x[np.arange(M), rng.integers(0, fan_in, M)] = np.where(np.arange(M) % 2, 127.0, -127.0)
    xd = _t(x, dev)
    a = ops.i8_operand_quantize(xd)
    got = G.unpack_layout(_np(a.codes), _np(a.scales), M, fan_in, 0)
    margin = np.float32(1.0 + 2.0 ** -22)
    assert np.array_equal(got["codes"], x.astype(np.int8)) and (got["scales"] == margin).all()
    lin64 = F.linear(xd.double() * float(margin), fq_w.double().t())
    want = lin64.float() + fq_b[None, :]
    y = layer.call_i8(xd)
    assert y.shape == (M, units) and not y.requires_grad
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    y3 = layer.call_i8(xd.reshape(1, M, fan_in))
    assert y3.shape == (1, M, units) and torch.equal(y3[0], y)


def _layer_reference(layer, x, act_block):
    """(Y, sum|terms|) in float64: quantize -> decode -> matmul with the fake-quantised weight, plus the fake-quantised bias."""
    with torch.no_grad():
        A = _np(ops.i8_operand_decode(ops.i8_operand_quantize(x.reshape(-1, x.shape[-1]), act_block))).astype(np.float64)
        qw, qb = _np(layer.nested_q_w_layer(layer.W)).astype(np.float64), _np(layer.nested_q_b_layer(layer.b)).astype(np.float64)
    return A @ qw + qb[None, :], np.abs(A) @ np.abs(qw) + np.abs(qb)[None, :]


@pytest.mark.parametrize("kw,act_block", [(dict(bits=8, orientation="columnwise"), 0), (dict(bits=8, orientation="scalar"), 64),
                                          (dict(bits=4, group_size=64), 0), (dict(bits=4, group_size=64, rounding="nearest"), 128)],
                         ids=["8bit_columnwise", "8bit_scalar_act64", "4bit_gs64", "4bit_gs64_nearest_act128"])
def test_i8_hardware_on_the_mnist_model(dev, kw, act_block):
    """784 = 12 * 64 + 16: the last group of dense_1 is ragged.  Inside the context the eval logits equal call_i8 layer by layer (bit
    for bit) and lie within the yardstick of emulate=True; outside it and in training mode the model is bit-identical."""
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", **kw)
    x = torch.rand(37, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    model.eval()
    with torch.no_grad():
        before, before_d1 = model(x), model.dense_1(torch.flatten(x, 1))
    dense = (("dense_1", model.dense_1), ("dense_2", model.dense_2))
    assert all(L.i8_hardware_eligible(m) for _, m in dense)
    op = model.dense_1.i8_operand()
    assert (op.lines, op.K, op.block) == (128, 784, 64 if "group_size" in kw else 0)
    with torch.no_grad():
        _same_bits(_np(ops.i8_operand_decode(op)), _np(model.dense_1.nested_q_w_layer(model.dense_1.W)).T + 0.0,
                   "the operand is not the fake-quantised kernel")
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, i, o, k=k: seen.__setitem__(k, (i[0].detach(), o.detach()))) for k, m in dense]
    with L.i8_hardware(model, act_block=act_block) as hw:
        assert hw.layers == [model.dense_1, model.dense_2]
        with torch.no_grad():
            inside = model(x)
        hard = dict(seen)
        for k, m in dense:                                  # per layer, from the input the layer saw
            xin, out = hard[k]
            assert torch.equal(out.view(torch.int32), m.call_i8(xin, act_block).view(torch.int32)), f"{k} is not call_i8"
            ref, terms = _layer_reference(m, xin, act_block)
            assert_within_terms(_np(out), ref, terms, f"i8_hardware {k}")
        model.train()                                       # training-mode calls keep the fake-quantised path
        assert torch.equal(model(x).detach().view(torch.int32), before.view(torch.int32))
        model.eval()
    with L.i8_hardware(model, act_block=act_block, emulate=True) as hw, torch.no_grad():
        assert hw.layers == [model.dense_1, model.dense_2]
        model(x)
        for k, m in dense:
            xin, out = seen[k]
            want = torch.add(torch.matmul(ops.i8_operand_decode(ops.i8_operand_quantize(xin, act_block)), m.nested_q_w_layer(m.W)),
                             m.nested_q_b_layer(m.b))
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), f"emulate=True {k}"
            ref, terms = _layer_reference(m, xin, act_block)
            assert_within_terms(_np(out), ref, terms, f"emulate=True {k} against float64")
            if k == "dense_1":                              # the same input on both paths: hardware against emulation directly
                assert_within_terms(_np(hard[k][1]), _np(out).astype(np.float64), terms, "hardware against emulate=True")
    for h in hooks:
        h.remove()
    assert model.dense_1._i8_hw is None and model.dense_2._i8_hw is None
    assert inside.shape == before.shape
    assert not torch.equal(hard["dense_1"][1], before_d1), "the hardware path quantises the activations: it cannot equal the fake-quantised layer"
    with torch.no_grad():
        assert torch.equal(model(x).view(torch.int32), before.view(torch.int32)), "forward outside the context changed"


def test_driver_i8_eval(dev):
    from learned_quantization_amd import train
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", bits=8, orientation="columnwise")
    g = torch.Generator(device=dev).manual_seed(4)
    x, y = torch.rand(64, 1, 28, 28, device=dev, generator=g), torch.randint(0, 10, (64,), device=dev, generator=g)
    model.train()
    out = train.i8_eval(model, x, y, act_block=64)
    assert model.training and out["i8_eval_layers"] == 2 and out["i8_eval_act_block"] == 64
    assert all(0.0 <= out[k] <= 1.0 for k in ("i8_eval_accuracy", "i8_eval_accuracy_emulated", "i8_eval_accuracy_fake"))
    assert np.isfinite(out["i8_eval_max_logit_diff"]) and 0.0 < out["i8_eval_max_logit_diff_fake"] < float("inf")
    with pytest.raises(ValueError, match="no Dense layer that can run on the int8 matrix instruction"):
        train.i8_eval(lq.build_model("mnist", mode="ste", value=0.0, device=dev), x, y)
