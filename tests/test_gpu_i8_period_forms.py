"""The period bookkeeping of the int8 GEMMs on the device, in the three kernels that tests/test_gpu_matrix_forms.py does not run:
k_i8_gemm_quantize<false>, k_i8_gemm_quantize<true> (csrc/lq_i8_gemm_quant.hpp: the 1 x 4 kernel has its own written-out copy of
the loop over K, and its host function its own copy of the ps / a_every / b_every rule) and k_i8_gemm<true> (csrc/lq_i8_gemm.hpp:
its own register allocation, and B's offset reloaded beside B's scale).  The rows are tests/_matrix_forms.py's NEW_I8_FUSED and
NEW_I8_GEMM; tests/test_i8_period_forms_cpu.py proves that they reach every branch of the bookkeeping and of the 1 x 4 tiling, that
the shapes of tests/test_gpu_i8_fused.py and tests/test_gpu_i8_affine.py do not, and that the data tells a scale or an offset of the
wrong block from the right one.

Every comparison is on bits and bytes, whole buffers and so padding included: this file has no tolerance.

 1 fused, symmetric   ops.i8_gemm_quantize on the ten rows, both activations, with and without bias, against FR.reference and
                      against i8_gemm -> relu -> i8_operand_quantize(64) on the device
 2 fused, affine      the same rows with offsets on B, against operand_of_activation(act(gemm_affine_reference)) and the composition
 3 affine fp32 GEMM   k_i8_gemm<true> on the eight NEW_I8_GEMM rows against the definition; with offsets of +0 against ops.i8_gemm
 4 memory contract    the output operand between 4 KiB guards under three presets, symmetric and affine, through the C ABI
 5 layers             Dense layers with group_size 192 and 256 on an input width of 448 (b_every 3 and 4 against the activations'
                      blocks of 64, b_every 2 and ps 2 against blocks of 128): symmetric 8-bit and asymmetric 4-bit, call_i8
                      against the composition and the NumPy definition, the operand-out call, and i8_dense_chain over three of them

The chain needs layers whose output is the next one's input, so its two hidden products are 33 x 448 x 448; everything else is at
most 33 x 130 x 448.  Evidence that the rows bite: profiles/i8_period_forms/mutations.txt."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _i8_affine_reference as A                                                              # noqa: E402
import _i8_fused_reference as FR                                                              # noqa: E402
import _i8_reference as R                                                                     # noqa: E402
import _matrix_forms as MF                                                                    # noqa: E402
from test_gpu_i8_affine import _bits, _relu, _tbits, _upload                                  # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

pytestmark = pytest.mark.gpu
NEW_FUSED = [c for c, _ in MF.NEW_I8_FUSED]
NEW_GEMM = [c for c, _ in MF.NEW_I8_GEMM]
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(key):
    """(a, b, b with offsets, bias) of a row: _i8_reference.gemm_case's seed 0 and _i8_affine_reference.with_offsets."""
    a, b, bias = R.gemm_case(*key)
    return a, b, A.with_offsets(b), bias


def _reference_y(a, b, bias):
    return A.gemm_affine_reference(a, b, bias) if "offsets" in b else R.gemm_reference(a, b, bias)


def _fused_against_both(dev, key, affine):
    a, b_sym, b_aff, bias = _case(key)
    b = b_aff if affine else b_sym
    M, N = key[:2]
    da, db, dbias = _upload(a, dev), _upload(b, dev), _t(bias, dev)
    assert type(db) is (ops.I8AffineOperand if affine else ops.I8Operand)
    for activation in FR.ACTIVATIONS:
        for rb, bv in ((bias, dbias), (None, None)):
            what = f"{key} {activation} bias={bv is not None} affine={affine}"
            got = ops.i8_gemm_quantize(da, db, bv, activation)
            assert type(got) is ops.I8Operand and (got.lines, got.K, got.block) == (M, N, 64), what
            assert (got.codes.numel(), got.scales.numel() * 4) == ops.i8_operand_bytes(M, N, 64), what
            ref = R.operand_of_activation(FR.act(A.gemm_affine_reference(a, b, rb), activation), FR.OUT_BLOCK) if affine else \
                FR.reference(a, b, rb, activation)
            bad = R.buffers_mismatch(_np(got.codes), _np(got.scales), ref)
            assert bad is None, f"{what}: the fused buffers differ from the reference: {bad}"
            y = ops.i8_gemm(da, db, bv)
            want = ops.i8_operand_quantize(_relu(y) if activation == "relu" else y, 64)
            assert torch.equal(got.codes, want.codes), f"{what}: codes differ from the composition's"
            assert torch.equal(got.scales.view(torch.int32), want.scales.view(torch.int32)), f"{what}: scales differ from the composition's"


# ------------------------------------------------------------------------------------------------ 1, 2 the operand-out kernels
@pytest.mark.parametrize("key", NEW_FUSED, ids=_ids)
def test_fused_symmetric_period_bookkeeping(dev, key):
    _fused_against_both(dev, key, affine=False)


@pytest.mark.parametrize("key", NEW_FUSED, ids=_ids)
def test_fused_affine_period_bookkeeping(dev, key):
    _fused_against_both(dev, key, affine=True)


# ------------------------------------------------------------------------------------------------------ 3 the affine fp32 GEMM
@pytest.mark.parametrize("key", NEW_GEMM, ids=_ids)
def test_affine_gemm_period_bookkeeping(dev, key):
    a, b_sym, b, bias = _case(key)
    da, db, dbias = _upload(a, dev), _upload(b, dev), _t(bias, dev)
    _bits(_np(ops.i8_gemm(da, db)), A.gemm_affine_reference(a, b), f"{key} no bias")
    y = ops.i8_gemm(da, db, dbias)
    _bits(_np(y), A.gemm_affine_reference(a, b, bias), f"{key} bias")
    # offsets of +0 on the same operands: the symmetric kernel's bits (tests/test_i8_period_forms_cpu.py: the reference agrees)
    bz, sym = _upload(A.with_offsets(b_sym, zero=True), dev), _upload(b_sym, dev)
    assert type(bz) is ops.I8AffineOperand and type(sym) is ops.I8Operand and not bz.offsets.view(torch.int32).any()
    assert _tbits(ops.i8_gemm(da, bz, dbias), ops.i8_gemm(da, sym, dbias)) and _tbits(ops.i8_gemm(da, bz), ops.i8_gemm(da, sym))
    assert not _tbits(y, ops.i8_gemm(da, sym, dbias)), "the offsets change nothing"


# ------------------------------------------------------------------------------------------------------------ 4 memory contract
@pytest.mark.parametrize("affine", [False, True], ids=["symmetric", "affine"])
@pytest.mark.parametrize("key", MF.I8_CONTRACT_KEYS, ids=_ids)
def test_memory_contract(dev, key, affine):
    """The output buffers carved out of one allocation with 4 KiB guards: the guards keep their preset, and the buffers do not
    depend on theirs (0xA5, 0x00, 0xFF) -- every byte of them, the padding and the clamped tiles' columns included, is written."""
    M, N, K, a_block, b_block = key
    a, b_sym, b_aff, bias = _case(key)
    b = b_aff if affine else b_sym
    da, db, dbias = _upload(a, dev), _upload(b, dev), _t(bias, dev)
    rc, rs = R.pack_layout(R.operand_of_activation(FR.act(_reference_y(a, b, bias), "relu"), FR.OUT_BLOCK))
    cb, sb = ops.i8_operand_bytes(M, N, 64)
    guard = 4096
    c0, s0 = guard, 2 * guard + cb                         # cb is a multiple of 1024: both starts stay on the 16-byte grid
    total = s0 + sb + guard
    lib, st = _hip.load(), _hip.stream_ptr(dev)
    seen = []
    for preset in (0xA5, 0x00, 0xFF):
        buf = torch.full((total,), preset, dtype=torch.uint8, device=dev)
        codes, scales = buf[c0:c0 + cb], buf[s0:s0 + sb]
        if affine:
            _hip.check(lib.lq_i8_gemm_quantize_affine(_hip.ptr(da.codes), _hip.ptr(da.scales), a_block, _hip.ptr(db.codes),
                                                      _hip.ptr(db.scales), _hip.ptr(db.offsets), b_block, _hip.ptr(dbias), 1, 64,
                                                      _hip.ptr(codes), _hip.ptr(scales), M, N, K, st), "lq_i8_gemm_quantize_affine")
        else:
            _hip.check(lib.lq_i8_gemm_quantize(_hip.ptr(da.codes), _hip.ptr(da.scales), a_block, _hip.ptr(db.codes), _hip.ptr(db.scales),
                                               b_block, _hip.ptr(dbias), 1, 64, _hip.ptr(codes), _hip.ptr(scales), M, N, K, st),
                       "lq_i8_gemm_quantize")
        torch.cuda.synchronize(dev)
        for lo, hi in ((0, c0), (c0 + cb, s0), (s0 + sb, total)):
            assert (buf[lo:hi] == preset).all(), f"guard [{lo}, {hi}) was written (preset {preset:#x})"
        seen.append((_np(codes).copy(), _np(scales).copy()))
        assert np.array_equal(seen[-1][0], rc) and np.array_equal(seen[-1][1].view(np.uint32), rs.view(np.uint32)), f"preset {preset:#x}"
    assert all(np.array_equal(c, seen[0][0]) and np.array_equal(s, seen[0][1]) for c, s in seen[1:]), "the bytes depend on the preset"


# --------------------------------------------------------------------------------------------------------------------- 5 layers
IN, ROWS = 448, 33
# nearest rounding for the 4-bit layers: under the floor quantiser W sits half a step low, which on the all-positive output of a
# relu leaves nearly every unit of the next layer negative, and the chain would compare biases
KINDS = {"8bit-symmetric": dict(bits=8), "4bit-asymmetric": dict(bits=4, asymmetric=True, rounding="nearest")}


def _dense(dev, kind, units, group_size, seed):
    kw = KINDS[kind]
    layer = lq.CustomDenseLayer(units=units, scale_gradient="ste", initializer=lq.RandomNormal(seed=seed), input_shape=IN, device=dev,
                                orientation="groupwise", group_size=group_size, **kw)
    layer.init_scales("minmax" if kw.get("asymmetric") else "absmax")
    return layer.eval()


def _download(op):
    """A device operand as a reference operand: the logical codes and scales, and the offsets where it has them."""
    out = R.unpack_layout(_np(op.codes), _np(op.scales), op.lines, op.K, op.block)
    if isinstance(op, ops.I8AffineOperand):
        LT, _, nbs = R.layout_dims(op.lines, op.K, op.block)
        out["offsets"] = np.ascontiguousarray(_np(op.offsets).reshape(nbs, 16 * LT)[:, :op.lines].T)
    return out


def _x(dev, seed=1):
    return torch.randn(ROWS, IN, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


@pytest.mark.parametrize("group_size", [192, 256])
@pytest.mark.parametrize("kind", list(KINDS))
def test_dense_with_wide_groups_is_the_composition_and_the_definition(dev, kind, group_size):
    """448 inputs in groups of 192 (192, 192, 64) or 256 (256, 192) against activations in blocks of 64 and 128, and with one scale
    per row: b_every is 3 or 4 at act_block 64; at 128 the pairs are (128, 256) -- ps = 2, b_every = 2 -- and (128, 192), which the
    product refuses (neither block divides the other: asserted); at 0 the periods are the layer's groups, ps = 3 or 4."""
    offsets = bool(KINDS[kind].get("asymmetric"))
    layer = _dense(dev, kind, 40, group_size, seed=5)
    x = _x(dev)
    op = layer.i8_operand(offsets=offsets)
    assert type(op) is (ops.I8AffineOperand if offsets else ops.I8Operand) and (op.lines, op.K, op.block) == (40, IN, group_size)
    ref_b = _download(op)
    assert ref_b["scales"].shape == (40, -(-IN // group_size)) and (ref_b["codes"] != 0).mean() > 0.5
    if offsets:
        assert bool(layer.nested_q_w_layer.offset.detach().abs().max() > 0) and np.abs(ref_b["offsets"]).max() > 0
    with torch.no_grad():
        qb = layer.nested_q_b_layer(layer.b)
        for act_block in (64, 128, 0):
            if act_block and max(act_block, group_size) % min(act_block, group_size):
                with pytest.raises(ValueError, match="the larger must be a multiple of the smaller"):
                    layer.call_i8(x, act_block, offsets=offsets)
                continue
            da = ops.i8_operand_quantize(x, act_block)
            got = layer.call_i8(x, act_block, offsets=offsets)
            assert _tbits(got, ops.i8_gemm(da, op, qb)), (kind, group_size, act_block)
            # the NumPy definition on the layer's own operand as it lies on the device, and the reference's activation operand
            a = R.operand_of_activation(_np(x), act_block)
            assert R.buffers_mismatch(_np(da.codes), _np(da.scales), a) is None
            _bits(_np(got), _reference_y(a, ref_b, _np(qb)), f"{kind} gs {group_size} act_block {act_block} against the definition")
        # the operand-out call: the chain's form, a_block = 64 against the layer's group
        h = layer.call_i8(x, 64, out_block=64, activation="relu", offsets=offsets)
        da = ops.i8_operand_quantize(x, 64)
        want = ops.i8_operand_quantize(_relu(ops.i8_gemm(da, op, qb)), 64)
        assert (h.lines, h.K, h.block) == (ROWS, 40, 64) and torch.equal(h.codes, want.codes)
        assert torch.equal(h.scales.view(torch.int32), want.scales.view(torch.int32))
        ref = R.operand_of_activation(FR.act(_reference_y(R.operand_of_activation(_np(x), 64), ref_b, _np(qb)), "relu"), 64)
        bad = R.buffers_mismatch(_np(h.codes), _np(h.scales), ref)
        assert bad is None, f"{kind} gs {group_size}: the operand-out call against the definition: {bad}"
        assert (ref["codes"] != 0).mean() > 0.125, "relu emptied the operand: the comparison tests nothing"


@pytest.mark.parametrize("group_size", [192, 256])
@pytest.mark.parametrize("kind", list(KINDS))
def test_dense_chain_over_wide_groups_equals_the_layers_one_by_one(dev, kind, group_size):
    offsets = bool(KINDS[kind].get("asymmetric"))
    d1, d2, d3 = _dense(dev, kind, IN, group_size, 5), _dense(dev, kind, IN, group_size, 6), _dense(dev, kind, 10, group_size, 7)
    x = _x(dev, seed=2)
    chain = [(d1, "relu"), (d2, "relu"), (d3, None)]
    kw = dict(offsets=True) if offsets else {}
    with torch.no_grad():
        h1 = F.relu(d1.call_i8(x, 64, **kw))
        h2 = F.relu(d2.call_i8(h1, 64, **kw))
        want = d3.call_i8(h2, 64, **kw)
        for h in (h1, h2):
            assert float((h > 0).float().mean()) > 0.125, "a hidden layer is dead: the chain would compare biases"
        got = L.i8_dense_chain(x, chain, 64, **kw)
        assert got.shape == (ROWS, 10) and _tbits(got, want), (kind, group_size)
        # the hidden operands themselves, written by the epilogue at b_every = group_size / 64
        o1 = d1.call_i8(x, 64, out_block=64, activation="relu", **kw)
        w1 = ops.i8_operand_quantize(h1, 64)
        assert torch.equal(o1.codes, w1.codes) and torch.equal(o1.scales.view(torch.int32), w1.scales.view(torch.int32))
        o2 = d2.call_i8(o1, out_block=64, activation="relu", **kw)
        w2 = ops.i8_operand_quantize(h2, 64)
        assert torch.equal(o2.codes, w2.codes) and torch.equal(o2.scales.view(torch.int32), w2.scales.view(torch.int32))
        assert _tbits(d3.call_i8(o2, **kw), want)
        # no activation between the layers
        want = d3.call_i8(d2.call_i8(d1.call_i8(x, 64, **kw), 64, **kw), 64, **kw)
        assert _tbits(L.i8_dense_chain(x, [(d1, None), (d2, None), (d3, None)], 64, **kw), want)
