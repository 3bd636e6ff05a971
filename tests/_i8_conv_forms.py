"""The launch rule of the int8 im2col operand (csrc/lq_kernels.hip: lq_i8_operand_im2col / i8_conv_slices; csrc/lq_i8_conv.hpp:
k_i8_im2col<S>) restated in Python, and the case table that reaches every run-time branch of it.

As in tests/_matrix_forms.py, ``i8_im2col_form`` is written from the text of the host function and of the kernel and exists ONLY so
that tests/test_i8_conv_cpu.py can prove that the table takes every branch; it is never used to compute an expected output: those
come from tests/_i8_conv_reference.py alone."""
import numpy as np

import _i8_conv_reference as R
import _mx_conv_reference as C

K_BLOCK = 256                 # threads of a block (csrc/lq_common.hpp: kBlock)
UNIT = 16                     # csrc/lq_i8_conv.hpp: kI8ConvUnit, the k of one 16-byte fragment
CACHE = 4                     # kI8ConvCache: units per thread held in registers
SLICES = 4                    # kI8ConvSlices: slices of the split form


def _cdiv(a, b):
    return -(-a // b)


def i8_im2col_form(g, block):
    """Keys: S (slices: 1 where a thread's CACHE units hold the longest span, else SLICES), units (of the longest span), pairs,
    nbs, chunks (thread blocks per scale block), grid, idle_threads (per slice: threads of the last chunk past the padded lines; in
    the split form they only meet the barrier), dead_lines (padded lines past M: code 0, scale
    1), padded_windows (lines whose window lies wholly in the padding), and ``blocks_of_k``: per scale block a dict with read
    (units read, the last rounded up), written (units written: the last block runs to 64 KT), ragged (the last unit read is cut by
    K), tail_read / tail_write (a slice runs the loops past its CACHE units), idle_slices (slices without a unit to read), last.
    j_wrap / i_wrap: a unit in which the column / row index returns to 0 with a tap after it."""
    M, K, OH, OW = C.dims(g)
    top, _, left, _ = C.padding_of(g)
    LT, KT = _cdiv(M, 16), _cdiv(K, 64)
    nbs = _cdiv(K, block) if block else 1
    lines = LT * 16
    units = (block if nbs > 1 else KT * 64) // UNIT
    pairs = lines * nbs
    S = SLICES if units > CACHE else 1
    per = K_BLOCK // S
    chunks = _cdiv(lines, per)
    span = block if block else K
    of_k = []
    for sb in range(nbs):
        c0 = sb * span
        c1 = min(c0 + span, K)
        last = sb == nbs - 1
        c1s = KT * 64 if last else c0 + span
        nu1, nus = _cdiv(c1 - c0, UNIT), (c1s - c0) // UNIT
        of_k.append(dict(read=nu1, written=nus, ragged=(c1 - c0) % UNIT != 0, tail_read=nu1 > CACHE * S, tail_write=nus > CACHE * S,
                         idle_slices=max(0, S - nu1), last=last))
    ih0, iw0 = np.arange(OH) * g.sh - top, np.arange(OW) * g.sw - left
    out_h, out_w = (ih0 + g.KH <= 0) | (ih0 >= g.H), (iw0 + g.KW <= 0) | (iw0 >= g.W)
    j_wrap = i_wrap = False
    for k0 in range(0, K, UNIT):
        inner = np.arange(k0 + 1, min(k0 + UNIT, K))
        j_wrap |= bool((inner % g.KW == 0).any())
        i_wrap |= bool((inner % (g.KH * g.KW) == 0).any())
    return dict(S=S, units=units, pairs=pairs, nbs=nbs, chunks=chunks, grid=chunks * nbs, idle_threads=chunks * per - lines,
                dead_lines=lines - M, padded_windows=g.B * int((out_h[:, None] | out_w[None, :]).sum()), blocks_of_k=of_k,
                j_wrap=j_wrap, i_wrap=i_wrap)


# (geometry, block): what tests/test_gpu_i8_conv.py::test_operand_bytes runs
FORMS = list(R.CASES)
