"""The int8 operands with offsets and the int8 GEMM's offset term on the device (include/lq_hip.h: lq_i8_operand_pack_affine /
lq_i8_operand_decode_affine / lq_i8_gemm_affine / lq_i8_gemm_quantize_affine), against tests/_i8_affine_reference.py.  The row sums
are exact and the definition states every rounding, so every comparison is bit for bit or byte for byte, with one exception: the
hardware path against ``emulate=True``, which stays within 1e-5 * sum|terms| (tests/_bounds.py) with
terms = sum_k |x_k| (|q_k s| + |b|) + |bias| -- the two parts of W round separately in the emulation.

 1 pack       buffers == the NumPy packer, offsets included; b == 0 gives lq_i8_operand_pack's bytes; decode == fq_forward_group_affine
 2 gemm       == the NumPy definition on every shape class and block pair; offsets == 0 gives i8_gemm's bits
 3 row sums   B codes 0, scales 1, offsets powers of two: a one-hot sweep over every k of K = 160, a full-byte A, R = -2^23
 4 specials   a NaN offset spoils its column only, a NaN A-scale its row only
 5 memory     guard bands around Y and the output operand under three presets; every pointer a region of tests/_arena.py's poisoned
              arena; the four entry points in one graph
 6 fused      i8_gemm_quantize with an affine b == the composition on the device == the reference
 7 layers     Dense and conv call_i8(offsets=True), the dense chain, i8_hardware and train.i8_eval on asymmetric models

The conditions of the data sets are asserted in tests/test_i8_affine_cpu.py.

A conv layer quantises its own activations, and LQ_INIT_ABSMAX's margin makes their scale 1 + 2^-22 where the row absmax is 127: with
the offset term the definition then rounds two products and their sum, where a float64 F.conv2d rounds once.  So the conv layer is
compared bit for bit with the NumPy definition on the reference im2col operand (asymmetric "SAME" padding, stride 2: a padded tap
holds code 0 and adds no offset) and with the float64 F.conv2d within the bound above; the Dense layer, which takes an operand as
it is, is compared with the float64 matmul bit for bit on the exact data."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_affine_reference as A                                                              # noqa: E402
import _i8_conv_reference as CR                                                               # noqa: E402
import _i8_fused_reference as FR                                                              # noqa: E402
import _i8_reference as G                                                                     # noqa: E402
import _mx_conv_reference as C                                                                # noqa: E402
from _arena import SENTINEL_WORD, Arena                                                       # noqa: E402
from _bounds import assert_within_terms                                                       # noqa: E402
from _group_reference import scale_shape                                                      # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402

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
    """A reference operand as the device's, through the NumPy packer; with offsets an I8AffineOperand."""
    cbuf, sbuf = G.pack_layout(op)
    args = (_t(cbuf, dev), _t(sbuf, dev), op["codes"].shape[0], op["codes"].shape[1], op["block"])
    if "offsets" not in op:
        return ops.I8Operand(*args)
    out = ops.I8AffineOperand(*args)
    out.offsets = _t(A.offsets_layout(op), dev)
    return out


def _bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, f"{what}: shapes {got.shape} {ref.shape}"
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        i = tuple(int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} differ, first at {i}: got {got[i]!r} want {ref[i]!r}")


def _tbits(got, want):
    return got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


_CASES = {}


def _case(key, dev):
    """(a, b, bias, device a, b, bias, reference without bias, with bias), computed once per case."""
    if key not in _CASES:
        a, b, bias = A.gemm_affine_case(*key)
        _CASES[key] = (a, b, bias, _upload(a, dev), _upload(b, dev), _t(bias, dev), A.gemm_affine_reference(a, b),
                       A.gemm_affine_reference(a, b, bias))
    return _CASES[key]


# -------------------------------------------------------------------------------------------------------------- 1 pack, decode
def _pack_case(R, C_, axis, gs):
    P, s = G.pack_case(R, C_, axis, gs)
    rng = np.random.default_rng([7, R, C_, axis, gs])
    b = rng.normal(0.0, 0.02, s.shape).astype(np.float32)
    b[0, 0] = np.nan                                        # a NaN offset; pack_case plants a NaN element and a NaN scale
    return P, s, b


@pytest.mark.parametrize("qrange", G.PACK_RANGES, ids=_ids)
@pytest.mark.parametrize("rounding", ["floor", "nearest"])
@pytest.mark.parametrize("case", G.PACK_CASES, ids=_ids)
def test_pack_is_the_reference_operand_and_decodes_to_the_fake_quantised_parameter(dev, case, rounding, qrange):
    R, C_, axis, gs = case
    qmin, qmax = qrange
    P, s, b = _pack_case(R, C_, axis, gs)
    ref = A.operand_of_parameter_affine(P, s, b, qmin, qmax, axis, gs, rounding)
    op = ops.i8_operand_pack(_t(P, dev), _t(s, dev), qmin, qmax, gs, rounding, _t(b, dev))
    assert isinstance(op, ops.I8AffineOperand) and (op.lines, op.K, op.block) == (*ref["codes"].shape, ref["block"])
    assert (op.codes.numel(), op.scales.numel() * 4) == ops.i8_operand_bytes(op.lines, op.K, op.block)
    assert op.offsets.shape == op.scales.shape and op.offsets.dtype == torch.float32
    bad = G.buffers_mismatch(_np(op.codes), _np(op.scales), ref) or A.offsets_mismatch(_np(op.offsets), ref)
    assert bad is None, bad
    out, q = ops.fq_forward_group_affine(_t(P, dev), _t(s, dev), _t(b, dev), qmin, qmax, gs, q_dtype=torch.int8, rounding=rounding)
    got = G.unpack_layout(_np(op.codes), _np(op.scales), op.lines, op.K, op.block)
    assert np.array_equal(got["codes"], _np(q).T if axis == 0 else _np(q)), "the codes are not fq_forward_group_affine's int8 view"
    dec = _np(ops.i8_operand_decode(op))
    _bits(dec, A.decode_affine(ref), "decode")
    dec, out = (dec.T if axis == 0 else dec), _np(out)
    elem = ~np.isnan(P)      # the NaN element has code 0 and decodes as its offset: the stated exception
    _bits(dec[elem], out[elem], "decode against fq_forward_group_affine")
    # b == 0: the symmetric pack's bytes
    z = ops.i8_operand_pack(_t(P, dev), _t(s, dev), qmin, qmax, gs, rounding, torch.zeros_like(_t(s, dev)))
    sym = ops.i8_operand_pack(_t(P, dev), _t(s, dev), qmin, qmax, gs, rounding)
    assert type(sym) is ops.I8Operand and torch.equal(z.codes, sym.codes)
    assert torch.equal(z.scales.view(torch.int32), sym.scales.view(torch.int32)) and not z.offsets.view(torch.int32).any()


def test_pack_refuses_a_wrong_offset_shape(dev):
    P, s = torch.zeros(160, 17, device=dev), torch.ones(3, 17, device=dev)
    with pytest.raises(ValueError, match="one offset per group"):
        ops.i8_operand_pack(P, s, -8, 7, 64, "floor", torch.zeros(17, 3, device=dev))


# -------------------------------------------------------------------------------------------------------------- 2 gemm
@pytest.mark.parametrize("key", A.all_gemm_affine_keys(), ids=_ids)
def test_gemm_is_the_definition(dev, key):
    a, b, bias, da, db, dbias, ref, ref_b = _case(key, dev)
    M, N = key[:2]
    _bits(_np(ops.i8_gemm(da, db)), ref, f"{key} no bias")
    y = ops.i8_gemm(da, db, dbias)
    _bits(_np(y), ref_b, f"{key} bias")
    assert torch.equal(ops.i8_gemm(da, db, dbias).view(torch.int32), y.view(torch.int32)), "two runs differ"
    ref64, terms = A.gemm_affine_f64(a, b, bias)
    assert_within_terms(_np(y), ref64, terms, f"{key} against float64")
    big = torch.full((M, N + 5), -7.0, device=dev)
    ops.i8_gemm(da, db, dbias, out=big[:, :N])
    _bits(_np(big[:, :N]), ref_b, f"{key} out= with a row stride")
    assert (big[:, N:] == -7.0).all()
    # offsets == 0: the symmetric kernel's Y, whose operand this is without the offsets
    bz = _upload(dict(b, offsets=np.zeros_like(b["offsets"])), dev)
    sym = ops.I8Operand(*db)
    assert _tbits(ops.i8_gemm(da, bz, dbias), ops.i8_gemm(da, sym, dbias)) and _tbits(ops.i8_gemm(da, bz), ops.i8_gemm(da, sym))
    assert not _tbits(y, ops.i8_gemm(da, sym, dbias)), "the offsets change nothing"


# -------------------------------------------------------------------------------------------------------------- 3 row-sum pins
def test_one_hot_sweep_counts_every_k_once_in_its_own_block(dev):
    """K = 160 with blocks of 64: three steps, the last ragged.  A has m - 7 in column k and B's codes are 0, so
    Y[m][n] = (m - 7) * ob[n][k // 64] exactly: a k counted twice, not at all, or against another block's offset shows."""
    b = A.pin_b()
    db = _upload(b, dev)
    rows = (np.arange(16) - 7).astype(np.float32)
    for k in range(A.PIN_K):
        y = _np(ops.i8_gemm(_upload(A.pin_one_hot_a(k), dev), db))
        want = rows[:, None] * b["offsets"][:, k // A.PIN_BLOCK][None, :]
        assert np.array_equal(y, want), f"k = {k}"


def test_row_sums_of_a_full_byte_a_and_of_the_longest_period(dev):
    b = A.pin_b()
    a = A.pin_random_a()
    want = sum(r[:, None].astype(np.float64) * b["offsets"][:, p][None, :] for p, r in enumerate(A.row_sums(a, b)))
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev)))
    assert np.array_equal(y.astype(np.float64), want)
    _bits(y, A.gemm_affine_reference(a, b), "full-byte A")
    a, b = A.pin_extreme()
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev)))
    assert np.array_equal(y.astype(np.float64), -(2.0 ** 23) * np.broadcast_to(b["offsets"][:, 0].astype(np.float64), (16, 16)))


# -------------------------------------------------------------------------------------------------------------- 4 special values
def test_nan_offset_spoils_its_column_and_nan_a_scale_its_row(dev):
    key = (*G.BLOCK_PAIR_SHAPE, 64, 128)
    a, b, bias = A.gemm_affine_case(*key)
    b["offsets"][4, 1] = np.nan
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev), _t(bias, dev)))
    _bits(y, A.gemm_affine_reference(a, b, bias), "NaN offset")
    assert np.isnan(y[:, 4]).all() and not np.isnan(np.delete(y, 4, axis=1)).any()
    a, b, bias = A.gemm_affine_case(*key)
    a["scales"][9, 2] = np.nan
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev), _t(bias, dev)))
    _bits(y, A.gemm_affine_reference(a, b, bias), "NaN A scale")
    assert np.isnan(y[9]).all() and not np.isnan(np.delete(y, 9, axis=0)).any()


# -------------------------------------------------------------------------------------------------------------- 5 memory, capture
@pytest.mark.parametrize("key", [(37, 21, 320, 64, 128), (17, 129, 128, 0, 0)], ids=_ids)
def test_memory_contract(dev, key):
    """Y (with a row stride) and the fused call's output operand carved out of one allocation between 4 KiB guards: the guards and
    the gaps of the rows keep their preset, and what is written does not depend on it."""
    M, N, K, a_block, b_block = key
    a, b, bias, da, db, dbias, _, ref_b = _case(key, dev)
    rc, rs = G.pack_layout(G.operand_of_activation(FR.act(ref_b, "relu"), 64))
    cb, sb = ops.i8_operand_bytes(M, N, 64)
    ldy, guard = N + 3, 4096
    yb = ((M * ldy * 4 + 15) // 16) * 16
    y0, c0 = guard, 2 * guard + yb
    s0 = c0 + cb + guard
    total = s0 + sb + guard
    lib, st = _hip.load(), _hip.stream_ptr(dev)
    for preset in (0xA5, 0x00, 0xFF):
        buf = torch.full((total,), preset, dtype=torch.uint8, device=dev)
        Y, codes, scales = buf[y0:y0 + M * ldy * 4].view(torch.float32).view(M, ldy), buf[c0:c0 + cb], buf[s0:s0 + sb]
        _hip.check(lib.lq_i8_gemm_affine(_hip.ptr(da.codes), _hip.ptr(da.scales), a_block, _hip.ptr(db.codes), _hip.ptr(db.scales),
                                         _hip.ptr(db.offsets), b_block, _hip.ptr(dbias), _hip.ptr(Y), ldy, M, N, K, st), "gemm_affine")
        _hip.check(lib.lq_i8_gemm_quantize_affine(_hip.ptr(da.codes), _hip.ptr(da.scales), a_block, _hip.ptr(db.codes),
                                                  _hip.ptr(db.scales), _hip.ptr(db.offsets), b_block, _hip.ptr(dbias), 1, 64,
                                                  _hip.ptr(codes), _hip.ptr(scales), M, N, K, st), "gemm_quantize_affine")
        torch.cuda.synchronize(dev)
        for lo, hi in ((0, y0), (y0 + M * ldy * 4, c0), (c0 + cb, s0), (s0 + sb, total)):
            assert (buf[lo:hi] == preset).all(), f"guard [{lo}, {hi}) was written (preset {preset:#x})"
        assert (Y[:, N:].contiguous().view(torch.uint8) == preset).all(), "the gap of Y's rows was written"
        _bits(_np(Y[:, :N]), ref_b, f"Y under preset {preset:#x}")
        assert np.array_equal(_np(codes), rc) and np.array_equal(_np(scales).view(np.uint32), rs.view(np.uint32)), f"preset {preset:#x}"


@pytest.mark.parametrize("key", [(37, 21, 320, 64, 128), (17, 129, 128, 0, 0)], ids=_ids)
def test_memory_contract_in_the_arena(dev, key):
    """tests/_arena.py: every pointer of lq_i8_gemm_affine and lq_i8_operand_decode_affine is a region of one poisoned allocation at
    its exact size.  The inputs -- B's offsets among them -- stay bit for bit what was uploaded, every guard keeps the sentinel, and
    the three columns between the rows of Y (ldy = N + 3) keep it too; the bias and Y sit 4 bytes off the 16-byte grid."""
    M, N, K = key[:3]
    a, b, bias, _, _, _, _, ref_b = _case(key, dev)
    (ac, as_), (bc, bs) = G.pack_layout(a), G.pack_layout(b)
    ldy = N + 3
    ar = Arena(dev)
    for name, data in (("a_codes", ac), ("a_scales", as_), ("b_codes", bc), ("b_scales", bs), ("b_offsets", A.offsets_layout(b))):
        ar.add(name, "in", data=data)
    ar.add("bias", "in", data=bias, residue=4)
    ar.add("Y", "some", nbytes=((M - 1) * ldy + N) * 4, residue=4, row_bytes=ldy * 4)
    ar.add("D", "out", nbytes=N * K * 4, residue=4, row_bytes=K * 4)
    ar.build()
    lib, st = _hip.load(), _hip.stream_ptr(dev)
    _hip.check(lib.lq_i8_gemm_affine(ar.ptr("a_codes"), ar.ptr("a_scales"), a["block"], ar.ptr("b_codes"), ar.ptr("b_scales"),
                                     ar.ptr("b_offsets"), b["block"], ar.ptr("bias"), ar.ptr("Y"), ldy, M, N, K, st), "lq_i8_gemm_affine")
    _hip.check(lib.lq_i8_operand_decode_affine(ar.ptr("b_codes"), ar.ptr("b_scales"), ar.ptr("b_offsets"), N, K, b["block"], ar.ptr("D"),
                                               st), "lq_i8_operand_decode_affine")
    torch.cuda.synchronize()
    ar.check(f"gemm_affine {key}")
    flat = np.concatenate([ar.numpy("Y", np.uint32), np.full(3, SENTINEL_WORD, np.uint32)]).reshape(M, ldy)
    assert (flat[:, N:] == SENTINEL_WORD).all(), "the columns between the rows of Y were written"
    _bits(np.ascontiguousarray(flat[:, :N]).view(np.float32), ref_b, "Y in the arena")
    _bits(ar.numpy("D", np.float32).reshape(N, K), A.decode_affine(b), "decode in the arena")


def test_capture_and_replay(dev):
    """pack_affine -> gemm_quantize_affine -> gemm_affine -> decode_affine, one launch each, in one graph, replayed twice."""
    M, H, N, K = 19, 70, 10, 200
    rng = np.random.default_rng(11)
    x = _t(rng.normal(0, 1, (M, K)).astype(np.float32), dev)
    W1, s1, o1 = (_t(v, dev) for v in (rng.normal(0, .05, (K, H)).astype(np.float32), np.full((4, H), 2.0 ** -6, np.float32),
                                        rng.normal(0, .02, (4, H)).astype(np.float32)))
    w2 = _upload(A.with_offsets(G.random_operand(rng, N, H, 64)), dev)
    b1, b2 = _t(rng.normal(0, 1, H).astype(np.float32), dev), _t(rng.normal(0, 1, N).astype(np.float32), dev)
    ea = ops.i8_operand_quantize(x, 64)
    e1 = ops.i8_operand_pack(W1, s1, -8, 7, 64, "nearest", o1)
    eh = ops.i8_gemm_quantize(ea, e1, b1, "relu")
    eager = [e1.codes, e1.scales, e1.offsets, eh.codes, eh.scales, ops.i8_gemm(eh, w2, b2), ops.i8_operand_decode(e1)]
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)      # noqa: E731
    wc, ws, hc, hs = (u8(n) for n in ops.i8_operand_bytes(H, K, 64) + ops.i8_operand_bytes(M, H, 64))
    wo, Y, D = u8(ws.numel()), torch.empty((M, N), device=dev), torch.empty((H, K), device=dev)
    outs = [wc, ws, wo, hc, hs, Y, D]
    lib = _hip.load()

    def launch():
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_i8_operand_pack_affine(_hip.ptr(W1), _hip.ptr(s1), _hip.ptr(o1), -8, 7, 1, K, H, 0, 64, _hip.ptr(wc),
                                                 _hip.ptr(ws), _hip.ptr(wo), st), "pack_affine")
        _hip.check(lib.lq_i8_gemm_quantize_affine(_hip.ptr(ea.codes), _hip.ptr(ea.scales), 64, _hip.ptr(wc), _hip.ptr(ws), _hip.ptr(wo),
                                                  64, _hip.ptr(b1), 1, 64, _hip.ptr(hc), _hip.ptr(hs), M, H, K, st), "gemm_quantize_affine")
        _hip.check(lib.lq_i8_gemm_affine(_hip.ptr(hc), _hip.ptr(hs), 64, _hip.ptr(w2.codes), _hip.ptr(w2.scales), _hip.ptr(w2.offsets),
                                         64, _hip.ptr(b2), _hip.ptr(Y), N, M, N, H, st), "gemm_affine")
        _hip.check(lib.lq_i8_operand_decode_affine(_hip.ptr(wc), _hip.ptr(ws), _hip.ptr(wo), H, K, 64, _hip.ptr(D), st), "decode_affine")

    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        for o in outs:
            o.fill_(0xEE if o.dtype == torch.uint8 else -7.0)
        g.replay()
        torch.cuda.synchronize(dev)
        for k, (o, e) in enumerate(zip(outs, eager)):
            assert torch.equal(o.view(torch.uint8).reshape(-1), e.contiguous().view(torch.uint8).reshape(-1)), \
                f"output {k} of the replay differs from the eager call"


# -------------------------------------------------------------------------------------------------------------- 6 fused
def _relu(v):
    return torch.where(v > 0, v, torch.where(v != v, v, torch.zeros_like(v)))


@pytest.mark.parametrize("key", FR.CASES, ids=_ids)
def test_fused_equals_the_composition_and_the_reference(dev, key):
    a, b, bias, da, db, dbias, ref, ref_b = _case(key, dev)
    M, N = key[:2]
    for activation in FR.ACTIVATIONS:
        for yref, bv in ((ref_b, dbias), (ref, None)):
            got = ops.i8_gemm_quantize(da, db, bv, activation)
            what = f"{key} {activation} bias={bv is not None}"
            y = ops.i8_gemm(da, db, bv)
            want = ops.i8_operand_quantize(_relu(y) if activation == "relu" else y, 64)
            assert type(got) is ops.I8Operand and (got.lines, got.K, got.block) == (M, N, 64), what
            bad = G.buffers_mismatch(_np(got.codes), _np(got.scales), G.operand_of_activation(FR.act(yref, activation), 64))
            assert bad is None, f"{what}: {bad}"
            assert torch.equal(got.codes, want.codes) and torch.equal(got.scales.view(torch.int32), want.scales.view(torch.int32)), what


# -------------------------------------------------------------------------------------------------------------- 7 layers
def _dense(dev, n_in, units, seed=1, trained=None, **kw):
    kw.setdefault("bits", 4)
    layer = lq.CustomDenseLayer(units=units, scale_gradient="ste", initializer=lq.RandomNormal(seed=seed), input_shape=n_in, device=dev,
                                orientation="groupwise", asymmetric=True, trained_weights=trained, **kw)
    if trained is None:
        layer.init_scales("minmax")
    return layer.eval()


def _conv(dev, g, co, group_size, seed=3, **kw):
    layer = lq.CustomConv2DLayer(filters=co, kernel_size=(g.KH, g.KW), strides=(g.sh, g.sw), padding=g.padding.lower(),
                                 scale_gradient="ste", initializer=lq.RandomNormal(seed=seed), input_shape=g.C, device=dev, bits=4,
                                 orientation="groupwise", group_size=group_size, asymmetric=True, **kw)
    layer.init_scales("minmax")
    return layer.eval()


@pytest.mark.parametrize("group_size", [64, 128, 1000])
def test_dense_call_i8_is_the_composition(dev, group_size):
    layer = _dense(dev, 200, 21, group_size=group_size)
    assert bool(layer.nested_q_w_layer.offset.detach().abs().max() > 0)
    x = torch.randn(19, 200, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    op = layer.i8_operand(offsets=True)
    assert isinstance(op, ops.I8AffineOperand) and (op.lines, op.K, op.block) == (21, 200, 0 if group_size >= 200 else group_size)
    with torch.no_grad():
        qb = layer.nested_q_b_layer(layer.b)
        for act_block in (0, 64):
            want = ops.i8_gemm(ops.i8_operand_quantize(x, act_block), op, qb)
            assert _tbits(layer.call_i8(x, act_block, offsets=True), want)
        # the operand is the reference's, and the product the definition's
        W, s, b = (_np(v.detach()) for v in (layer.W, layer.nested_q_w_layer.scale, layer.nested_q_w_layer.offset))
        ref = A.operand_of_parameter_affine(W, s, b, *layer.q_range, 0, group_size, layer.rounding)
        assert (G.buffers_mismatch(_np(op.codes), _np(op.scales), ref) or A.offsets_mismatch(_np(op.offsets), ref)) is None
        a = G.operand_of_activation(_np(x), 64)
        _bits(_np(layer.call_i8(x, 64, offsets=True)), A.gemm_affine_reference(a, ref, _np(qb)), "Dense against the definition")
    with pytest.raises(ValueError, match="asymmetric=True"):
        layer.call_i8(x)


def test_dense_call_i8_on_exact_data_is_the_float64_matmul(dev):
    x, W, s, b, bias = A.exact_dense_case()
    layer = _dense(dev, W.shape[0], W.shape[1], trained=[W, bias], group_size=64)
    with torch.no_grad():
        layer.nested_q_w_layer.scale.copy_(_t(s, dev))
        layer.nested_q_w_layer.offset.copy_(_t(b, dev))
        layer.nested_q_b_layer.scale.fill_(1.0)
        assert torch.equal(layer.nested_q_w_layer(layer.W), layer.W), "the kernel is not on its own grid"
    a = _upload(dict(codes=x.astype(np.int8), scales=np.ones((x.shape[0], 1), np.float32), block=0), dev)
    got = _np(layer.call_i8(a, offsets=True))
    want = x.astype(np.float64) @ W.astype(np.float64) + bias
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("group_size", [64, 128])
def test_conv_call_i8_is_the_composition_and_the_definition(dev, group_size):
    g = C.GEOMS[1]                                          # 7 x 7, stride 2, "SAME" on 9 x 10: the pads differ left and right
    top, bottom, left, right = C.padding_of(g)
    assert g.sh == 2 and left != right
    co = 24
    layer = _conv(dev, g, co, group_size)
    M, K, OH, OW = C.dims(g)
    x = C.gaussian_input(g, seed=4)
    op = layer.i8_operand(offsets=True)
    Wm = _np(layer.kernel.detach().permute(3, 2, 0, 1).reshape(co, K))
    s, b = _np(layer.nested_q_k_layer.scale.detach()), _np(layer.nested_q_k_layer.offset.detach())
    assert s.shape == (co, -(-K // group_size)) and np.abs(b).max() > 0
    ref = A.operand_of_parameter_affine(Wm, s, b, *layer.q_range, 1, group_size, layer.rounding)
    assert (G.buffers_mismatch(_np(op.codes), _np(op.scales), ref) or A.offsets_mismatch(_np(op.offsets), ref)) is None
    with torch.no_grad():
        qb = layer.nested_q_b_layer(layer.b)
    for act_block in (0, 64):
        got = layer.call_i8(_t(x, dev), act_block, offsets=True)
        a_dev = ops.i8_operand_im2col(_t(x, dev), layer.kernel_size, layer.strides, (top, bottom, left, right), act_block)
        want = ops.i8_gemm(a_dev, op, qb).reshape(g.B, OH, OW, co).permute(0, 3, 1, 2)
        assert _tbits(got, want), act_block
        a, _, _ = CR.reference(x, g, act_block)
        wantr = A.gemm_affine_reference(a, ref, _np(qb)).reshape(g.B, OH, OW, co).transpose(0, 3, 1, 2)
        _bits(_np(got), wantr, f"conv against the definition, act_block {act_block}")
    # float64 conv2d of the decoded activations with the fake-quantised kernel, within the project's bound
    a, _, _ = CR.reference(x, g, 0)
    ref64, terms = A.gemm_affine_f64(a, ref, _np(qb))
    assert_within_terms(_np(layer.call_i8(_t(x, dev), 0, offsets=True).permute(0, 2, 3, 1)).reshape(M, co), ref64, terms, "conv f64")
    with pytest.raises(ValueError, match="asymmetric=True"):
        layer.call_i8(_t(x, dev))


@pytest.fixture(scope="module")
def mnist(dev):
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, scale_init="minmax", bits=4, group_size=128, asymmetric=True)
    # zero-mean inputs: under the floor quantiser W sits half a step low, and all-positive pixels would leave every hidden unit
    # negative -- relu would hand the second layer zeros and the chain tests would compare biases
    x = torch.randn(5, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    with torch.no_grad():
        hidden = model.eval().dense_1(torch.flatten(x, 1))
    assert int((hidden > 0).sum()) > hidden.numel() // 8, "the hidden layer is dead: the fixture tests nothing"
    return model.eval(), x


def test_dense_chain_and_fused_hardware_equal_the_unfused_path(dev, mnist):
    model, x = mnist
    fake = model(x).detach()
    with L.i8_hardware(model, 64) as none:
        assert none.layers == [] and _tbits(model(x).detach(), fake), "offsets=False must switch no asymmetric layer"
    with L.i8_hardware(model, 64, offsets=True) as hw:
        assert len(hw.layers) == 2 and all(m.asymmetric for m in hw.layers)
        plain, logits = model(x).detach(), model.logits(x).detach()
    assert not _tbits(plain, fake)
    with L.i8_hardware(model, 64, fused=True, offsets=True) as hwf:
        assert len(hwf.fused_layers) == 2
        assert _tbits(model(x).detach(), plain) and _tbits(model.logits(x).detach(), logits)
    flat = x.reshape(x.shape[0], -1)
    chain = model.i8_chain()
    assert _tbits(L.i8_dense_chain(flat, chain, 64, offsets=True), logits)
    with pytest.raises(ValueError, match="asymmetric=True"):
        L.i8_dense_chain(flat, chain, 64)
    assert all(getattr(m, "_i8_hw", None) is None for m in L.custom_layers_of(model)) and getattr(model, "_i8_fused", None) is None


def _terms_of_dense(model, x, dev):
    """sum_k |x_k| (|q_k s| + |b|) + |bias| of the model's last Dense layer under i8_hardware(emulate=True, offsets=True)."""
    last = [m for m in L.custom_layers_of(model) if isinstance(m, L.CustomDenseLayer)][-1]
    seen = []
    hook = last.register_forward_hook(lambda m, i, o: seen.append((i[0].detach(), o.detach())))
    try:
        with L.i8_hardware(model, 64, emulate=True, offsets=True):
            model(x)
    finally:
        hook.remove()
    inp, emu = seen[-1]
    with torch.no_grad():
        dec = ops.i8_operand_decode(ops.i8_operand_quantize(inp.reshape(-1, inp.shape[-1]), 64)).double()
        w = last.nested_q_w_layer
        g = torch.arange(last.W.shape[0], device=dev) // last.group_size
        ob = w.offset.detach().double()[g]
        qs = w(last.W).detach().double() - ob
        terms = dec.abs() @ (qs.abs() + ob.abs()) + last.nested_q_b_layer(last.b).detach().double().abs()
    return last, emu, terms


def test_hardware_against_the_emulation_within_the_bound(dev, mnist):
    model, x = mnist
    last, emu, terms = _terms_of_dense(model, x, dev)
    seen = []
    hook = last.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    try:
        with L.i8_hardware(model, 64, offsets=True):
            model(x)
    finally:
        hook.remove()
    hwy = seen[-1]
    worst = float(((hwy.double() - emu.double()).abs() / terms).max())
    print(f"hardware against emulate=True, asymmetric MNIST logits: max |diff| / sum|terms| = {worst:.3e}")
    assert_within_terms(_np(hwy), _np(emu).astype(np.float64), _np(terms), "hardware against emulate=True")


def test_cifar_convs_switch_with_the_opt_in_only(dev):
    model = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=dev, scale_init="minmax", kernel_storage="oihw", bits=4,
                           group_size=64, asymmetric=True).eval()
    x = torch.rand(2, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    fake = model(x).detach()
    with L.i8_hardware(model, convs=True) as none:
        assert not [m for m in none.layers if m.asymmetric] and _tbits(model(x).detach(), fake)
    with L.i8_hardware(model, convs=True, offsets=True) as hw:
        convs = [m for m in hw.layers if L.i8_conv_eligible(m, offsets=True)]
        assert len(convs) == 6 and all(m.asymmetric for m in convs)
        y = model(x).detach()
    with L.i8_hardware(model, convs=True, offsets=True, emulate=True) as hwe:
        assert len(hwe.layers) == len(hw.layers) and torch.isfinite(model(x)).all()
    assert not _tbits(y, fake) and torch.isfinite(y).all()
    y_t = torch.arange(2, device=dev) % 10
    out = train.i8_eval(model, x, y_t, convs=True, offsets=True)
    assert out["i8_eval_conv_layers"] == 6 and np.isfinite(out["i8_eval_conv_max_logit_diff"])
    with pytest.raises(ValueError):
        train.i8_eval(model, x, y_t, convs=True)


def test_i8_eval_with_offsets_returns_its_fields(dev, mnist):
    model, x = mnist
    y = torch.arange(x.shape[0], device=dev) % 10
    model.train()
    try:
        out = train.i8_eval(model, x, y, act_block=64, fused=True, offsets=True)
    finally:
        model.eval()
    assert out["i8_eval_layers"] == 2 and out["i8_eval_act_block"] == 64
    assert out["i8_eval_fused_layers"] == 2 and out["i8_eval_fused_max_logit_diff"] == 0.0
    assert all(0.0 <= out[k] <= 1.0 for k in ("i8_eval_accuracy", "i8_eval_accuracy_emulated", "i8_eval_accuracy_fake"))
    assert np.isfinite(out["i8_eval_max_logit_diff"]) and 0.0 < out["i8_eval_max_logit_diff_fake"] < float("inf")
    with pytest.raises(ValueError, match="no Dense layer that can run"):
        train.i8_eval(model, x, y, act_block=64)
