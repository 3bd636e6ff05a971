"""GPU tests that put EVERY element code and EVERY scale byte through v_mfma_scale_f32_16x16x128_f8f6f4 and through
lq_mx_operand_decode, one term per output (include/lq_hip.h: lq_mx_gemm, lq_mx_operand_decode; tests/_mx_gemm_reference.py builds the
operands, tests/test_mx_gemm_cpu.py asserts their conditions without a device).

The exact sets of tests/test_gpu_mx_gemm.py hold seven values under six scale bytes, and its random sets no special code.  Here the
operands are zero except one column k0, so that Y[m][n] = value(m) * value(n) * 2^(byte_m + byte_n - 254) plus zeros: nothing is
summed and nothing is rounded, and a misdecoded subnormal, a wrong binade, a wrong format immediate or a scale applied to one
operand at a time in fp32 shows as a wrong bit.  The buffers are built on the host by G.pack_layout -- the layout as documented, which
test_gpu_mx_gemm.py holds the device's own buffers to -- because no quantizer emits a NaN or Inf code, byte 0 or a byte above 127 next
to a saturated element.  K = 160: two K steps, the second a quarter full; k0 = 5, 77, 133: the first and the second half of an fp8
fragment, and the second K step.  The 256-line operands give a 4 x 4 grid of blocks: every block index up to 3 on both axes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _mx_gemm_reference as G                                                                # noqa: E402
from _clip_reference import bits_equal                                                        # noqa: E402

from learned_quantization_amd import ops                                                      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _operand(ref, dev):
    """The device operand whose buffers are the documented layout of a logical one."""
    cbuf, sbuf = G.pack_layout(ref.codes, ref.bytes, ref.name)
    L, K = ref.codes.shape
    assert (cbuf.size, sbuf.size) == ops.mx_operand_bytes(ref.name, L, K)
    return ops.MxOperand(torch.from_numpy(cbuf).to(dev), torch.from_numpy(sbuf).to(dev), ref.name, L, K)


def _first(mask, Y, ref):
    m, n = np.argwhere(mask)[0]
    return f"{int(mask.sum())} of {mask.size} outputs, first at (m, n) = ({m}, {n}): got {Y[m, n]!r}, reference {ref[m, n]!r}"


@pytest.mark.parametrize("k0", G.CODE_K0S)
@pytest.mark.parametrize("pair", G.PAIRS, ids=lambda p: "-".join(p))
def test_gemm_of_every_code_pair(dev, pair, k0):
    """Line i of each operand holds code i at k0 under byte 127: Y[m][n] = value(m) * value(n), exactly a float32 and never
    subnormal.  NaN where the reference is NaN (a NaN code, or 0 * Inf), +-Inf with the reference's sign, every finite product
    equal.  The sign of a ZERO result is not pinned: the one term is added to the zeros of the other 159 elements (-0 + +0)."""
    ra, rb = G.code_sweep_operand(pair[0], k0), G.code_sweep_operand(pair[1], k0)
    with np.errstate(all="ignore"):
        ref, _ = G.gemm_reference(ra, rb)
    Y = ops.mx_gemm(_operand(ra, dev), _operand(rb, dev)).cpu().numpy()
    assert Y.shape == ref.shape and Y.dtype == np.float32
    nan = np.isnan(ref)
    wrong = np.isnan(Y) != nan
    assert not wrong.any(), "NaN positions differ: " + _first(wrong, Y, ref)
    wrong = ~nan & (Y.astype(np.float64) != ref)
    assert not wrong.any(), "products differ: " + _first(wrong, Y, ref)


@pytest.mark.parametrize("pair", G.SCALE_PAIRS, ids=lambda p: "-".join(p))
def test_gemm_of_every_scale_byte_pair(dev, pair):
    """Line i holds +-1.5 at k0 = 77 under byte i (0 .. 255): Y[m][n] = +-2.25 * 2^(m + n - 254).  Inside float32's normal range
    the result is exact BIT FOR BIT, also where one operand's scaled element is itself below 2^-126 (byte 0: 2^-127) -- the scales
    are not applied to one operand at a time in fp32.  From 2^128 it is +-Inf; a line under byte 255 is NaN.  Below 2^-126 the
    instruction gives the correctly rounded float32 SUBNORMAL (to nearest, ties to even: 2.25 * 2^-148 = 4.5 * 2^-149 gives 4 * 2^-149;
    measured on an MI355X, 2772 non-zero subnormal results of 8128 per pair, the same for the three pairs) and nothing is flushed;
    what rounds to zero (below 2^-150) is +0 whatever the product's sign, the one term being added to zeros, as in the code sweep."""
    ra, rb = G.scale_sweep_operand(pair[0], False), G.scale_sweep_operand(pair[1], True)
    with np.errstate(all="ignore"):
        ref, _ = G.gemm_reference(ra, rb)
        ref32 = ref.astype(np.float32)
    Y = ops.mx_gemm(_operand(ra, dev), _operand(rb, dev)).cpu().numpy()
    normal, over, under = G.scale_sweep_classes(ref)
    yb, rb32 = Y.view(np.uint32), ref32.view(np.uint32)
    rounded, zero = under & (Y == ref32), under & (Y == 0)
    print(f"mx_gemm {pair[0]} x {pair[1]}: of {int(under.sum())} products below 2^-126, {int(rounded.sum())} are the correctly rounded "
          f"float32 ({int((rounded & ~zero).sum())} of them not zero) and {int((zero & ~rounded).sum())} are flushed to zero")
    wrong = np.isnan(Y) != np.isnan(ref)
    assert not wrong.any(), "NaN positions differ: " + _first(wrong, Y, ref)
    wrong = normal & (yb != rb32)
    assert not wrong.any(), "products inside the normal range differ: " + _first(wrong, Y, ref)
    wrong = over & (Y != np.where(ref > 0, np.inf, -np.inf))
    assert not wrong.any(), "products from 2^128 are not the reference's Inf: " + _first(wrong, Y, ref)
    wrong = under & ((Y != ref32) | ((ref32 != 0) & (yb != rb32)))
    assert not wrong.any(), "products below 2^-126 are not the correctly rounded float32: " + _first(wrong, Y, ref)
    assert (under & (ref32 != 0)).sum() >= 2000 and (under & (ref32 == 0)).any()


@pytest.mark.parametrize("name", G.OPERAND_FORMATS)
def test_decode_of_every_code_under_every_scale_byte(dev, name):
    """256 lines by 256: line i under byte i, column c holding code c mod 2^bits.  out = value(code) * 2^(byte - 127) in ONE fp32
    multiplication: byte 0 is 2^-127, byte 255 NaN, products below 2^-126 are float32 subnormals, from 2^128 +-Inf."""
    ref = G.decode_sweep_operand(name)
    got = ops.mx_operand_decode(_operand(ref, dev)).cpu().numpy()
    want = G.decode(ref, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN positions differ"
    wrong = ~np.isnan(want) & (got.view(np.uint32) != want.view(np.uint32))
    assert not wrong.any(), "decode differs: " + _first(wrong, got, want)
    assert bits_equal(got, want)
