"""The launch rules of the matrix-path kernels restated in Python, and one case table per kernel that reaches every run-time branch
of them: the packed int8 operands and the int8 GEMM (csrc/lq_i8_operand.hpp, lq_i8_gemm.hpp), the packed MX operands, the im2col
operand and the two block-scaled GEMMs (lq_mx_operand.hpp, lq_mx_conv.hpp, lq_mx_gemm.hpp).

Every ``*_form`` function is written from the text of the host function in csrc/lq_kernels.hip that launches the kernel (and, for
what the kernel decides from its block and thread index, from the kernel's text) and returns a small dict.  As in
tests/_group_forms.py they exist ONLY so that tests/test_matrix_forms_cpu.py can prove that a table takes every branch, and that
the rows this file adds are needed for it; they are never used to compute an expected output: those come from
tests/_i8_reference.py, tests/_mx_gemm_reference.py and tests/_mx_conv_reference.py alone.

Each ``FORMS_*`` table is the union of the shapes the earlier GPU files already run (imported, not copied) and the ``NEW_*`` rows
that tests/test_gpu_matrix_forms.py runs.  The second half builds the inputs of the new quantize cases, so that the CPU file can
assert their conditions on the reference without a device.

``i8_gemm_quantize_form``, ``FORMS_I8_FUSED`` and ``FORMS_I8_GEMM_AFFINE`` do the same for the three other kernels that carry the
int8 GEMM's period bookkeeping (k_i8_gemm<true>, k_i8_gemm_quantize<false> and <true>): tests/test_i8_period_forms_cpu.py holds
their reach proof and tests/test_gpu_i8_period_forms.py runs their new rows."""
import numpy as np

import _i8_affine_reference as AF
import _i8_fused_reference as FR
import _i8_reference as I
import _mx_conv_reference as C
import _mx_gemm_reference as G

K_BLOCK = 256                 # threads of a block (csrc/lq_common.hpp: kBlock)
I8_CACHE = 16                 # csrc/lq_i8_operand.hpp: kI8Cache, accesses per lane held in registers
ONE_PER_LINE = "line"         # a_every / b_every of an operand with one scale per line (INT32_MAX on the device)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ int8 operands
def i8_quantize_form(M, K, block, aligned=True):
    """lq_i8_operand_quantize / k_i8_quantize<V>.  Keys: V, log_team, team, step (= team * V), nbs, pairs, per_block, blocks,
    dead_rows (rows of the last tile past M: their teams read nothing and write code 0 and scale 1), dead_teams (teams of the last
    thread block without a pair), cache (elements of a scale block the registers hold) and ``blocks_of_k``: per scale block a dict
    with length (elements read), written (codes written: the last block runs to 64 KT), cached (accesses of the first loop that
    read), tail_read / tail_write (the loops past the cache run), last.  nonlast_tail: a block other than the last has a tail."""
    V = 4 if K % 4 == 0 and aligned else 1
    LT, KT = _cdiv(M, 16), _cdiv(K, 64)
    nbs = _cdiv(K, block) if block else 1
    span = min(block if block else KT * 64, 64 * V)
    log_team = 0
    while log_team < 6 and (V << log_team) < span:
        log_team += 1
    T = 1 << log_team
    step = T * V
    pairs, per_block = LT * 16 * nbs, K_BLOCK >> log_team
    blocks = _cdiv(pairs, per_block)
    of_k = []
    for blk in range(nbs):
        kspan = block if block else K
        c0 = blk * kspan
        c1 = min(c0 + kspan, K)
        last = blk == nbs - 1
        c1s = KT * 64 if last else c0 + kspan
        of_k.append(dict(length=c1 - c0, written=c1s - c0, cached=sum(c0 + it * step < c1 for it in range(I8_CACHE)),
                         tail_read=c0 + I8_CACHE * step < c1, tail_write=c0 + I8_CACHE * step < c1s, last=last))
    return dict(V=V, log_team=log_team, team=T, step=step, nbs=nbs, pairs=pairs, per_block=per_block, blocks=blocks,
                dead_rows=LT * 16 - M, dead_teams=blocks * per_block - pairs, cache=I8_CACHE * step, blocks_of_k=of_k,
                nonlast_tail=any(b["tail_write"] and not b["last"] for b in of_k),
                last_tail=any(b["tail_write"] and b["last"] for b in of_k))


def i8_pack_form(R, C_, axis, gs):
    """lq_i8_operand_pack / k_i8_pack<RNE, LINE_FAST>: one thread per (line, 16 k)."""
    L, K = (C_, R) if axis == 0 else (R, C_)
    LT, KT = _cdiv(L, 16), _cdiv(K, 64)
    threads = LT * 16 * KT * 4
    blocks = _cdiv(threads, K_BLOCK)
    return dict(line_fast=axis == 0, block=0 if gs >= K else gs, threads=threads, blocks=blocks, dead_threads=blocks * K_BLOCK - threads,
                dead_lines=LT * 16 - L, dead_runs=KT * 4 - _cdiv(K, 16))


def _waves(MT, NT):
    """Of a grid of 64 x 64 blocks whose waves own 2 x 2 tiles: the grid, a clamped second tile on either axis, waves that leave."""
    gx, gy = _cdiv(NT, 4), _cdiv(MT, 4)
    live = _cdiv(MT, 2) * _cdiv(NT, 2)
    return dict(grid=(gx, gy), clamped_m=MT % 2 == 1, clamped_n=NT % 2 == 1, leaving=4 * gx * gy - live)


def _period_rule(K, a_block, b_block):
    """The ``ps`` / ``a_every`` / ``b_every`` rule that the host functions i8_gemm and i8_gemm_quantize each write out, and what
    the kernels' loop over K does with it.  The loop is walked as the kernels write it: ``left`` counts down from ps, a period ends on
    ``--left == 0 || kt == KT - 1``, then ``++ca == a_every`` resets ca and advances ia (the same for B), and the scales of the next
    period are read at ia / ib unless this was the last K step.  a_changes / b_changes: the reloads that read an index advanced
    since the last read; a_wraps / b_wraps: those of them under ``every >= 2``, that is the resets of ca / cb to 0 after which the
    index is read (with every == 1 the counter never leaves 0 between periods, and a reset at the end of K is read by nobody)."""
    KT = _cdiv(K, 64)
    lo, hi = min(a_block, b_block), max(a_block, b_block)
    assert lo == 0 or hi % lo == 0
    F = lo if lo > 0 else hi
    ps = min(F // 64, KT) if F > 0 else KT
    every = lambda blk: blk // F if blk > 0 else ONE_PER_LINE      # noqa: E731
    ev = dict(a=every(a_block), b=every(b_block))
    steps, count, idx, seen = [], dict(a=0, b=0), dict(a=0, b=0), dict(a=0, b=0)
    changes, wraps = dict(a=0, b=0), dict(a=0, b=0)
    left, run = ps, 0
    for kt in range(KT):
        left, run = left - 1, run + 1
        if left == 0 or kt == KT - 1:
            steps.append(run)
            left, run = ps, 0
            for o in "ab":
                count[o] += 1
                if count[o] == ev[o]:                      # ONE_PER_LINE never compares equal: INT32_MAX on the device
                    count[o], idx[o] = 0, idx[o] + 1
            if kt != KT - 1:
                for o in "ab":
                    if idx[o] != seen[o]:
                        changes[o] += 1
                        wraps[o] += ev[o] >= 2
                        seen[o] = idx[o]
    # what the reloads read stays inside the scale buffers: the largest index read is below the operand's number of scale blocks
    for o, blk in (("a", a_block), ("b", b_block)):
        assert seen[o] < (_cdiv(K, blk) if blk else 1), (K, a_block, b_block)
    return dict(ps=ps, KT=KT, a_every=ev["a"], b_every=ev["b"], periods=len(steps), steps=steps, short_last=KT % ps != 0,
                a_whole=a_block >= K, b_whole=b_block >= K, a_above=a_block > K, b_above=b_block > K,
                a_changes=changes["a"], b_changes=changes["b"], a_wraps=wraps["a"], b_wraps=wraps["b"])


def i8_gemm_form(M, N, K, a_block, b_block):
    """lq_i8_gemm / k_i8_gemm<AFF>.  ps: K steps per period; a_every / b_every: periods per scale block (ONE_PER_LINE for block 0);
    periods: their number; steps: the length of each; short_last: the last period is cut by K; a_whole / b_whole: a block that is
    not 0 but at least K (one scale block); a_above / b_above: a block above K, where the host's ``min(F / 64, KT)`` can cut;
    a_changes / b_changes / a_wraps / b_wraps: see _period_rule."""
    d = _waves(_cdiv(M, 16), _cdiv(N, 16))
    d.update(_period_rule(K, a_block, b_block))
    return d


def i8_gemm_quantize_form(M, N, K, a_block, b_block):
    """lq_i8_gemm_quantize / k_i8_gemm_quantize<AFF>: a wave owns 1 x 4 tiles, a thread block 64 x 64, and along n the grid spans the
    padded OUTPUT operand.  grid = (OKT, ceil(MT / 4)); leaving: the waves with mt >= MT (every block column has the same
    ``leaving // OKT`` of them, in its last block row); clamped_last = 4 OKT - NT: the tiles of the last block column that are
    ``min(nt0 + j, NT - 1)`` copies of B's last tile, all of their columns masked by live_n; masked_cols: the columns past N of B's
    last tile itself (live_n masks part of a tile); dead_lines: the rows past M of the last row tile (live_m); the period keys are
    _period_rule's, which this host function writes out a second time."""
    MT, NT, OKT = _cdiv(M, 16), _cdiv(N, 16), _cdiv(N, 64)
    gy = _cdiv(MT, 4)
    d = dict(grid=(OKT, gy), leaving=(4 * gy - MT) * OKT, clamped_last=4 * OKT - NT, masked_cols=16 * NT - N, dead_lines=16 * MT - M)
    d.update(_period_rule(K, a_block, b_block))
    return d


# -------------------------------------------------------------------------------------------------------------- MX operands
def mx_operand_form(L, K, fp4, vec, line_fast):
    """launch_mx_operand / k_mx_operand<DYN, METHOD, FP4, VEC, LINE_FAST>: one thread per (line, block of 32 k)."""
    assert not (vec and line_fast)
    LT, KT, KG = G.layout_dims(L, K)
    threads = LT * 16 * KT * 4
    blocks = _cdiv(threads, K_BLOCK)
    return dict(fp4=fp4, vec=vec, line_fast=line_fast, threads=threads, blocks=blocks, dead_threads=blocks * K_BLOCK - threads,
                dead_lines=LT * 16 - L, dead_kblocks=KT * 4 - _cdiv(K, 32), idle_scale_bytes=4 * KG - KT)


def mx_im2col_form(g):
    """lq_mx_operand_im2col / k_mx_im2col: a thread block is 256 consecutive lines of one k block.  chunks: thread blocks per k block;
    grid = chunks * KT * 4; idle_threads: threads of the last chunk past the padded lines (they return); dead_lines: padded lines
    past M (code 0, byte 127); full_last_chunk: M a multiple of 256; padded_windows: lines whose window lies wholly in the padding;
    j_wrap / i_wrap: a block of 32 taps in which the column index j / the row index i returns to 0 with a tap after it (an i wrap is
    the step to the next channel); flat_block: a block of 32 live taps inside one kernel row (no wrap fires in it)."""
    M, K, OH, OW = C.dims(g)
    top, _, left, _ = C.padding_of(g)
    LT, KT, KG = G.layout_dims(M, K)
    chunks = _cdiv(LT * 16, K_BLOCK)
    ih0, iw0 = np.arange(OH) * g.sh - top, np.arange(OW) * g.sw - left
    out_h, out_w = (ih0 + g.KH <= 0) | (ih0 >= g.H), (iw0 + g.KW <= 0) | (iw0 >= g.W)
    j_wrap = i_wrap = flat = False
    for k0 in range(0, K, 32):
        k1 = min(k0 + 32, K)
        inner = np.arange(k0 + 1, k1)                          # taps with a tap of the same block in front of them
        j_wrap |= bool((inner % g.KW == 0).any())
        i_wrap |= bool((inner % (g.KH * g.KW) == 0).any())
        flat |= k1 - k0 == 32 and not (inner % g.KW == 0).any()
    return dict(M=M, K=K, chunks=chunks, grid=chunks * KT * 4, idle_threads=chunks * K_BLOCK - LT * 16, dead_lines=LT * 16 - M,
                full_last_chunk=M % K_BLOCK == 0, dead_kblocks=KT * 4 - _cdiv(K, 32), idle_scale_bytes=4 * KG - KT,
                padded_windows=g.B * int((out_h[:, None] | out_w[None, :]).sum()), j_wrap=j_wrap, i_wrap=i_wrap, flat_block=flat,
                wide_kernel=g.KW > 32)


def mx_gemm_form(M, N, K):
    """lq_mx_gemm / k_mx_gemm<FA, FB>."""
    MT, KT, KG = G.layout_dims(M, K)
    d = _waves(MT, _cdiv(N, 16))
    d.update(KT=KT, KG=KG, short_last_group=KT % 4 != 0)
    return d


def mx_gemm_quantize_form(M, N, K):
    """lq_mx_gemm_quantize / k_mx_gemm_quantize: along n the grid spans the padded OUTPUT operand, 2 OKT blocks of 64 columns.
    no_k: waves past B's last tile (they write padding only); idle: waves of the output's last K step where it leaves idle scale
    bytes to write; odd_mt: a wave whose second tile row does not exist (the ``break``); n_mod32: N % 32."""
    MT, NT = _cdiv(M, 16), _cdiv(N, 16)
    _, OKT, OKG = G.layout_dims(M, N)
    gx, gy = 2 * OKT, _cdiv(MT, 4)
    rows = _cdiv(MT, 2)                                        # wave rows that stay
    return dict(grid=(gx, gy), leaving=(2 * gy - rows) * 2 * gx, no_k=rows * (2 * gx - _cdiv(NT, 2)), clamped_n=NT % 2 == 1,
                idle=rows * 4 if 4 * OKG > OKT else 0, idle_scale_bytes=4 * OKG - OKT, odd_mt=MT % 2 == 1, n_mod32=N % 32)


# ---------------------------------------------------------------------------------------------------------------- the tables
# i8 quantize (M, K, block, aligned): test_quantize_is_scale_init_then_forward runs every shape x block on an aligned and a shifted
# base, test_quantize_rows_longer_than_the_register_cache the long rows with block 0
OLD_I8_QUANTIZE = [(M, K, b, al) for M, K in I.QUANT_SHAPES for b in I.QUANT_BLOCKS for al in (True, False)] + \
    [(M, K, 0, al) for M, K in I.LONG_QUANT_SHAPES for al in (True, False)]
NEW_I8_QUANTIZE = [
    ((2, 8420, 4160, True), "V = 4, three blocks, 64 elements past the 4096 cached in two non-last blocks, a last block of 100"),
    ((2, 8420, 4160, False), "the same data one float off the 16-byte grid: V = 1, 3136 elements past the 1024 cached"),
    ((2, 2246, 1088, True), "K % 4 == 2: V = 1 by the extent; blocks of 1088, 1088 and 70"),
]
FORMS_I8_QUANTIZE = OLD_I8_QUANTIZE + [c for c, _ in NEW_I8_QUANTIZE]

FORMS_I8_PACK = list(I.PACK_CASES)                            # (R, C, axis, gs): nothing to add, see test_matrix_forms_cpu.py

# i8 GEMM (M, N, K, a_block, b_block)
OLD_I8_GEMM = [s + (0, 0) for s in I.GEMM_SHAPES] + [I.BLOCK_PAIR_SHAPE + p for p in I.BLOCK_PAIRS] + I.EXTRA_GEMM_KEYS
NEW_I8_GEMM = [
    ((17, 18, 448, 128, 256), "ps = 2, b_every = 2: periods of 2, 2, 2 and 1 steps"),
    ((17, 18, 448, 256, 128), "its mirror: a_every = 2"),
    ((17, 18, 448, 64, 192), "b_every = 3"),
    ((17, 18, 448, 192, 64), "a_every = 3"),
    ((17, 18, 448, 192, 192), "ps = 3: periods of 3, 3 and 1 steps"),
    ((17, 18, 320, 384, 0), "a block of A that is not 0 but above K: ps = KT, one scale block"),
    ((17, 18, 320, 0, 384), "the same on B"),
    ((17, 18, 320, 384, 128), "A's block above K next to three blocks of B: a_every = 3 is never completed"),
]
FORMS_I8_GEMM = OLD_I8_GEMM + [c for c, _ in NEW_I8_GEMM]
# k_i8_gemm<true>: tests/test_gpu_i8_affine.py runs all_gemm_affine_keys(), tests/test_gpu_i8_period_forms.py the NEW_I8_GEMM rows
FORMS_I8_GEMM_AFFINE = AF.all_gemm_affine_keys() + [c for c, _ in NEW_I8_GEMM]

# k_i8_gemm_quantize<false> and <true> (M, N, K, a_block, b_block): tests/test_gpu_i8_fused.py and the fused tests of
# tests/test_gpu_i8_affine.py run FR.CASES, tests/test_gpu_i8_period_forms.py the new rows
NEW_I8_FUSED = [
    ((33, 40, 320, 128, 64), "a_every = 2 over three blocks of A: ia is read after two wraps; NT = 3: one clamped tile, 8 masked "
                             "columns; MT = 3: one leaving wave"),
    ((17, 40, 448, 64, 192), "b_every = 3, seven periods: cb wraps twice (blocks of 192, 192 and 64)"),
    ((17, 96, 448, 192, 64), "a_every = 3; NT = 6: the second column block has two clamped tiles"),
    ((17, 96, 448, 128, 256), "ps = 2, b_every = 2: periods of 2, 2, 2 and 1 steps"),
    ((17, 65, 448, 256, 128), "its mirror: a_every = 2"),
    ((17, 40, 448, 192, 192), "ps = 3: periods of 3, 3 and 1 steps"),
    ((17, 65, 320, 384, 0), "A's block above K: ps = KT, one scale block"),
    ((17, 65, 320, 0, 384), "the same on B"),
    ((17, 65, 320, 384, 128), "A's block above K beside three blocks of B"),
    ((33, 130, 448, 64, 256), "the fused chain's shape: a_block = 64 from the previous epilogue, b_every = 4 over two blocks of B"),
]
FORMS_I8_FUSED = list(FR.CASES) + [c for c, _ in NEW_I8_FUSED]
I8_CONTRACT_KEYS = [(17, 96, 448, 192, 64), (33, 40, 320, 128, 64)]      # the rows of the new memory-contract test
I8_END_TO_END = dict(x=(3, 70), act_block=128, w=(70, 40), gs=70)      # quantize(block = 128 >= K) times a packed (70, 40) kernel

# MX operand (L, K, fp4, vec, line_fast): pack runs PACK_SHAPES aligned in all three formats, its memory contract (70, 40, 0) and
# (33, 288, 1) 4 bytes off the grid; quantize runs QUANT_SHAPES aligned, its memory contract the same shapes off the grid
FORMS_MX_OPERAND = [((C_, R) if axis == 0 else (R, C_)) + (fp4, axis == 1 and C_ % 4 == 0, axis == 0)
                    for R, C_, axis in G.PACK_SHAPES for fp4 in (True, False)] + \
    [(33, 288, fp4, False, False) for fp4 in (True, False)] + \
    [(M, K, fp4, vec and K % 4 == 0, False) for M, K in G.QUANT_SHAPES for fp4 in (True, False) for vec in (True, False)]

# im2col
_G = C.Geom
NEW_IM2COL = [
    (_G(1, 3, 17, 17, 3, 3, 1, 1, "SAME"), "M = 289: two chunks, 15 dead lines; K = 27: one live k block of four"),
    (_G(3, 20, 15, 15, 3, 3, 1, 1, "SAME"), "M = 675: three chunks; K = 180: KT = 2, two idle scale bytes"),
    (_G(1, 4, 16, 16, 3, 3, 1, 1, "SAME"), "M = 256: the last chunk is full"),
    (_G(2, 3, 4, 4, 3, 3, 1, 1, (3, 3, 3, 3)), "the corner windows lie wholly in the padding"),
    (_G(1, 5, 6, 7, 3, 2, 2, 1, (0, 2, 1, 0)), "asymmetric explicit padding"),
    (_G(1, 2, 3, 40, 1, 35, 1, 1, "VALID"), "KW = 35 > 32: no wrap fires inside the first block"),
    (_G(1, 43, 4, 4, 3, 3, 1, 1, "SAME"), "K = 387: KT = 4 = 4 KG, no idle scale byte (the table had 1, 2 and 3 only); a last block of 3"),
]
NEW_GEOMS = [g for g, _ in NEW_IM2COL]
TWO_CHUNKS, THREE_CHUNKS, PADDED_GEOM = NEW_GEOMS[0], NEW_GEOMS[1], NEW_GEOMS[3]
EXPANDED_GEOM = TWO_CHUNKS._replace(B=3)                      # x (1, C, H, W) expanded to three images: batch stride 0
FORMS_IM2COL = list(C.GEOMS) + NEW_GEOMS

# the two block-scaled GEMMs (M, N, K)
FORMS_MX_GEMM = list(dict.fromkeys(G.EXACT_SHAPES + G.RANDOM_SHAPES))


OLD_FUSED = [G.FUSED_BIG] + list(G.FUSED_SMALL)               # what tests/test_gpu_mx_gemm_fused.py runs
NEW_FUSED = [((17, 32, 160), "N % 32 == 0: a last block without a masked column")]
FUSED_PAIR = ("fp8_e4m3", "fp4_e2m1")                         # the input formats of the new row, as the edge shapes of that file


# -------------------------------------------------------------------------------------------------------------- the inputs
def end_to_end_case():
    """(x (3, 70), P (70, 40), s) of the quantize(block = 128) -> GEMM row: two Gaussian rows of different magnitude and one
    row of 1e-40, as tests/_i8_reference.py's quantize_case has it (a subnormal: the scale is raised to 2^-126, every code 0); the
    kernel is pack_case's, one NaN element and one NaN scale included."""
    e = I8_END_TO_END
    rng = np.random.default_rng([128, *e["x"]])
    x = (rng.normal(0.0, 1.0, e["x"]) * np.exp2([[3.0], [-5.0], [0.0]])).astype(np.float32)
    x[2] = np.float32(1e-40)
    P, s = I.pack_case(*e["w"], 0, e["gs"])
    return x, P, s
def long_quantize_case(M, K, block):
    """x (M, K) standard normal with one planted value per (row, scale block) that holds more than 4096 -- 1024 where K % 4 != 0 --
    elements: 7.5 + row + blk / 4 with alternating sign at the block's last but one element, which lies past what the registers
    hold in the 16-byte form and in the 4-byte form alike.  The planted value is the block's maximum, so it alone fixes the scale."""
    rng = np.random.default_rng([M, K, block])
    x = rng.normal(0.0, 1.0, (M, K)).astype(np.float32)
    cache = 4096 if K % 4 == 0 else 1024
    planted = []
    for blk in range(_cdiv(K, block)):
        c0, c1 = blk * block, min((blk + 1) * block, K)
        if c1 - c0 > cache:
            for r in range(M):
                x[r, c1 - 2] = (7.5 + r + blk / 4) * (-1.0) ** (r + blk)
                planted.append((r, blk, c1 - 2))
    return x, planted


def i8_saturated_share(op):
    return float((np.abs(op["codes"].astype(np.int64)) >= 127).mean())


def mx_saturated_share(ref):
    """The share of an MX reference operand's codes at the largest finite magnitude of its format."""
    from learned_quantization_amd import ops
    mag = np.abs(ops.mx_decode_table(ref.name).astype(np.float64))
    top = mag[np.isfinite(mag)].max()
    return float((mag[ref.codes] == top).mean())
