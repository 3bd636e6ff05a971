"""The launch forms of the matrix-path kernels that the earlier files do not reach, on the device, byte for byte: one test per row
that tests/_matrix_forms.py adds to the case tables (tests/test_matrix_forms_cpu.py proves that the tables reach every branch of
the host's launch arithmetic, and that they do not without these rows).  The references are the NumPy ones of the sibling files --
tests/_i8_reference.py, tests/_mx_gemm_reference.py, tests/_mx_conv_reference.py -- and every comparison is on bits and bytes, whole
buffers and so padding included: this file has no tolerance.

 1 k_i8_quantize   scale blocks longer than the register cache: the tail loops of a NON-last block end at the block's end
 2 k_i8_gemm       periods of two and three steps inside scale blocks of two and three periods, a block that is not 0 but above K,
                   and lq_i8_operand_quantize(block = 128) of K = 70 handed to the GEMM
 3 k_mx_im2col     two, three and four chunks of 256 lines per k block, a full last chunk, windows wholly in the padding,
                   asymmetric explicit padding, a kernel row of 35 taps, KT = 4 (no idle scale byte), a batch axis of stride 0; the
                   chunked geometries once more inside a poisoned arena
 4 k_mx_gemm_quantize   N a multiple of 32, the one value of tests/test_matrix_forms_cpu.py's reach list that BIG and SMALL of
                   tests/test_gpu_mx_gemm_fused.py leave out

k_mx_operand, k_mx_gemm and k_i8_pack get no row: the shapes of tests/test_gpu_mx_gemm.py and tests/test_gpu_i8.py reach every form
of them, and for these kernels the CPU reach assertion (test_the_earlier_shapes_reach_every_form_of_the_other_kernels) is the
deliverable.  Evidence that the rows bite: profiles/matrix_forms/mutations.txt."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_reference as I                                                                     # noqa: E402
import _matrix_forms as MF                                                                    # noqa: E402
import _mx_conv_reference as C                                                                # noqa: E402
import _mx_gemm_reference as G                                                                # noqa: E402
import _mx_reference as X                                                                     # noqa: E402
from _arena import Arena                                                                      # noqa: E402
from test_gpu_i8 import _same_bits, _upload                                                   # noqa: E402
from test_gpu_mx_conv import _args, _input, _reference, _unfolded                             # noqa: E402

from learned_quantization_amd import _hip, ops                                                # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(G.OPERAND_FORMATS)
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------- 1 k_i8_quantize
@functools.lru_cache(maxsize=None)
def _long_case(M, K, block):
    x, _ = MF.long_quantize_case(M, K, block)
    x.setflags(write=False)
    return x, I.operand_of_activation(x, block)


@pytest.mark.parametrize("case", [c for c, _ in MF.NEW_I8_QUANTIZE], ids=_ids)
def test_quantize_scale_blocks_longer_than_the_register_cache(dev, case):
    """The maximum of every long block lies past what the registers hold (tests/test_matrix_forms_cpu.py), so a tail loop of the read
    pass that stops early gives another scale, and one of the write pass that stops early leaves codes of the buffer's preset."""
    M, K, block, aligned = case
    x, ref = _long_case(M, K, block)
    xa = _t(x, dev)
    xd = xa if aligned else torch.empty(M * K + 1, device=dev)[1:].view(M, K).copy_(xa)
    assert (xd.data_ptr() % 16 == 0) == aligned
    cb, sb = ops.i8_operand_bytes(M, K, block)
    codes, scales = torch.empty(cb, dtype=torch.uint8, device=dev), torch.empty(sb // 4, device=dev)
    for preset in (0x7F, 0xFF):                            # the result must not depend on what the buffers held
        codes.fill_(preset)
        scales.view(torch.uint8).fill_(preset)
        _hip.check(_hip.load().lq_i8_operand_quantize(_hip.ptr(xd), M, K, block, _hip.ptr(codes), _hip.ptr(scales), _hip.stream_ptr(dev)),
                   "lq_i8_operand_quantize")
        bad = I.buffers_mismatch(_np(codes), _np(scales), ref)
        assert bad is None, f"preset {preset:#x}: {bad}"
    op = ops.i8_operand_quantize(xd, block)
    assert (op.lines, op.K, op.block) == (M, K, block) and torch.equal(op.codes, codes)
    # the device composition: scale_init_group with ABSMAX, then fq_forward_group's integers, through the packer
    s = torch.empty(I.scale_shape(M, K, 1, block), device=dev)
    ops.scale_init_group(xa, s, -127, 127, block, "absmax", rounding="nearest", min_value=I.MIN_SCALE)
    _, q = ops.fq_forward_group(xa, s, -127, 127, block, q_dtype=torch.int8, rounding="nearest")
    bad = I.buffers_mismatch(_np(op.codes), _np(op.scales), dict(codes=_np(q), scales=_np(s), block=block))
    assert bad is None, "against the device composition: " + str(bad)
    packed = ops.i8_operand_pack(xa, s, -127, 127, block, "nearest")
    assert torch.equal(packed.codes, op.codes) and torch.equal(packed.scales.view(torch.int32), op.scales.view(torch.int32))


# -------------------------------------------------------------------------------------------------------------- 2 k_i8_gemm
@functools.lru_cache(maxsize=None)
def _gemm_case(key):
    a, b, bias = I.gemm_case(*key)
    return a, b, bias, I.gemm_reference(a, b), I.gemm_reference(a, b, bias)


@pytest.mark.parametrize("key", [c for c, _ in MF.NEW_I8_GEMM], ids=_ids)
def test_gemm_period_bookkeeping(dev, key):
    a, b, bias, ref, ref_bias = _gemm_case(key)
    da, db = _upload(a, dev), _upload(b, dev)
    _same_bits(_np(ops.i8_gemm(da, db)), ref, f"gemm {key}")
    _same_bits(_np(ops.i8_gemm(da, db, _t(bias, dev))), ref_bias, f"gemm {key} with bias")


def test_quantize_with_a_block_above_k_into_the_gemm(dev):
    """lq_i8_operand_quantize(block = 128) of K = 70 writes one scale block and hands block = 128 to the GEMM.  Two Gaussian rows
    and a row of 1e-40 against a Gaussian kernel: the product holds distinct finite values throughout (tests/test_matrix_forms_cpu.py)."""
    e = MF.I8_END_TO_END
    x, P, s = MF.end_to_end_case()
    ra, rb = I.operand_of_activation(x, e["act_block"]), I.operand_of_parameter(P, s, -128, 127, 0, e["gs"], "nearest")
    a = ops.i8_operand_quantize(_t(x, dev), e["act_block"])
    b = ops.i8_operand_pack(_t(P, dev), _t(s, dev), -128, 127, e["gs"], "nearest")
    assert (a.lines, a.K, a.block, b.lines, b.K, b.block) == (3, 70, 128, 40, 70, 0)
    for op, ref in ((a, ra), (b, rb)):
        bad = I.buffers_mismatch(_np(op.codes), _np(op.scales), ref)
        assert bad is None, bad
    bias = np.random.default_rng(70).normal(0.0, 1.0, 40).astype(np.float32)
    _same_bits(_np(ops.i8_gemm(a, b)), I.gemm_reference(ra, rb), "quantize(block 128) x pack")
    _same_bits(_np(ops.i8_gemm(a, b, _t(bias, dev))), I.gemm_reference(ra, rb, bias), "quantize(block 128) x pack with bias")


# ------------------------------------------------------------------------------------------------------------ 3 k_mx_im2col
@pytest.mark.parametrize("method", C.METHODS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("g", MF.NEW_GEOMS, ids=C.geom_id)
def test_im2col_operand_bytes(dev, g, name, method):
    M, K, OH, OW = C.dims(g)
    ref, wc, ws = _reference(g, name, method)
    x = _t(_input(g), dev)
    op = ops.mx_operand_im2col(x, *_args(g), name, method)
    assert (op.lines, op.K, op.format, op.out_hw) == (M, K, name, (OH, OW))
    assert (op.codes.numel(), op.scales.numel()) == ops.mx_operand_bytes(name, M, K)
    bad = G.layout_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, f"against the NumPy reference: {bad}"
    assert np.array_equal(_np(op.codes), wc) and np.array_equal(_np(op.scales), ws)
    want = ops.mx_operand_quantize(_unfolded(x, *_args(g)), name, method)
    assert torch.equal(op.codes, want.codes) and torch.equal(op.scales, want.scales), "against mx_operand_quantize(unfold(x))"


@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e4m3"])
def test_im2col_of_an_expanded_batch(dev, name):
    """x (1, C, H, W) expanded to three images: a batch stride of 0, four chunks of lines.  The bytes are those of the contiguous copy."""
    g = MF.EXPANDED_GEOM
    one = _t(_input(MF.TWO_CHUNKS), dev)
    xv = one.expand(g.B, -1, -1, -1)
    assert xv.stride(0) == 0 and tuple(xv.shape) == (g.B, g.C, g.H, g.W)
    ref, _ = G.operand_of_activation(C.im2col(_np(xv.contiguous()), g), name, "mx")
    op = ops.mx_operand_im2col(xv, *_args(g), name, "mx")
    assert (op.lines, op.K) == C.dims(g)[:2]
    bad = G.layout_mismatch(_np(op.codes), _np(op.scales), ref)
    assert bad is None, bad
    want = ops.mx_operand_im2col(xv.contiguous(), *_args(g), name, "mx")
    assert torch.equal(op.codes, want.codes) and torch.equal(op.scales, want.scales)


@pytest.mark.parametrize("name", ["fp4_e2m1", "fp8_e4m3"])
@pytest.mark.parametrize("g", [MF.TWO_CHUNKS, MF.THREE_CHUNKS], ids=C.geom_id)
def test_im2col_chunks_in_a_poisoned_arena(dev, g, name):
    """X (4 bytes off the 16-byte grid), codes and scales carved out of one poisoned arena: the guards keep the sentinel and X its
    bits.  Four code bytes 0x7F in a row are legitimate in an fp8 operand, so completeness is shown by the same bytes after a
    prefill with the sentinel and with 0xFF, not by the absence of the sentinel word."""
    M, K, _, _ = C.dims(g)
    cb, sb = ops.mx_operand_bytes(name, M, K)
    _, wc, ws = _reference(g, name, "mx")
    ar = Arena(dev)
    ar.add("X", "in", data=_input(g), residue=4, row_bytes=g.W * 4)
    ar.add("codes", "some", nbytes=cb)
    ar.add("scales", "some", nbytes=sb)
    ar.build()
    top, bottom, left, right = C.padding_of(g)
    geom = _hip.ConvGeom(g.B, g.C, g.H, g.W, g.C * g.H * g.W, g.H * g.W, g.W, 1, g.KH, g.KW, g.sh, g.sw, top, left, bottom, right)
    lib = _hip.load()
    for preset in (0x7F, 0xFF):
        ar.fill("codes", preset)
        ar.fill("scales", preset)
        _hip.check(lib.lq_mx_operand_im2col(ar.ptr("X"), ctypes.byref(geom), X.FORMATS[name].id, 0, ar.ptr("codes"), ar.ptr("scales"),
                                            _hip.stream_ptr(dev)), "lq_mx_operand_im2col")
        torch.cuda.synchronize()
        ar.check(f"im2col {name} {C.geom_id(g)} preset {preset:#x}")
        assert np.array_equal(ar.numpy("codes", np.uint8), wc) and np.array_equal(ar.numpy("scales", np.uint8), ws), hex(preset)


# ----------------------------------------------------------------------------------------------------- 4 k_mx_gemm_quantize
@pytest.mark.parametrize("method", C.METHODS)
@pytest.mark.parametrize("out_format", ["fp8_e4m3", "fp4_e2m1"])
@pytest.mark.parametrize("shape", [s for s, _ in MF.NEW_FUSED], ids=_ids)
def test_fused_gemm_with_whole_output_blocks(dev, shape, out_format, method):
    """Against the composition mx_gemm -> relu -> mx_operand_quantize on the same device, byte for byte, and the NumPy operand of the
    device's own Y."""
    M, N, _ = shape
    fa, fb = MF.FUSED_PAIR
    c = G.random_case(*shape, fa, fb)
    a = ops.mx_operand_quantize(_t(c["x"], dev), fa, "mx")
    b = ops.mx_operand_pack(_t(c["W"], dev), _t(c["sw"], dev), fb)
    bias = _t(c["bias"], dev)
    got = ops.mx_gemm_quantize(a, b, bias, "relu", out_format, method)
    y = ops.mx_gemm(a, b, bias)
    y = torch.where(y > 0, y, torch.where(y != y, y, torch.zeros_like(y)))
    want = ops.mx_operand_quantize(y, out_format, method)
    assert (got.lines, got.K) == (M, N) and (got.codes.numel(), got.scales.numel()) == ops.mx_operand_bytes(out_format, M, N)
    ref, _ = G.operand_of_activation(_np(y), out_format, method)
    bad = G.layout_mismatch(_np(got.codes), _np(got.scales), ref)
    assert bad is None, bad
    assert torch.equal(got.codes, want.codes) and torch.equal(got.scales, want.scales)
