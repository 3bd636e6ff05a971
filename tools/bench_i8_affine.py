#!/usr/bin/env python3
"""The cost of the int8 GEMM's offset term (lq_i8_gemm_affine, lq_i8_gemm_quantize_affine) next to its yardstick, in one process.
The protocol is tools/bench_i8_gemm.py's: rotating buffer sets, every round times each variant once (an event-timed run of
``--inner`` back-to-back calls), the order of the variants rotates from round to round, the figure is the median over the rounds in
microseconds per call with its min-max, and the whole comparison is repeated ``--repeats`` times.

  * ``gemm``: ops.i8_gemm with an affine B (codes, scales, offsets) next to the SYMMETRIC ops.i8_gemm on the same A and the same
    B codes and scales -- the yardstick: its kernel's instruction stream is the parent's (profiles/i8_affine/asm_compare.txt) -- and
    next to ``torch.matmul`` in fp32 on the decoded operands, what the emulated path multiplies with.  ``b_block`` 0 and 128,
    ``a_block`` 0.  The expectation from the instruction count is a ratio of at most 6/4 on the compute-bound shapes.
  * ``gemm_quantize``: the same for ops.i8_gemm_quantize (relu, blocks of 64 out); expectation at most 5/4.

One JSON line per workload, shape, block and repeat.

    python tools/bench_i8_affine.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learned_quantization_amd import ops  # noqa: E402
from tools.bench_i8_gemm import timed  # noqa: E402

GEMM_SHAPES = [(4096, 4096, 4096), (16384, 4096, 4096), (256, 4096, 4096), (256, 784, 128)]      # (M, K, N)
FUSED_SHAPES = GEMM_SHAPES[:3]
B_BLOCKS = [0, 128]
EXPECTED = {"gemm": 6 / 4, "gemm_quantize": 5 / 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)

    for repeat in range(args.repeats):
        g = torch.Generator(device=dev).manual_seed(42 + repeat)
        for workload, shapes in (("gemm", GEMM_SHAPES), ("gemm_quantize", FUSED_SHAPES)):
            for M, K, N in shapes:
                x = torch.empty(M, K, device=dev).normal_(generator=g)
                w = torch.empty(K, N, device=dev).normal_(generator=g) * 0.05 + 0.03      # one-sided enough for a real offset
                bias = torch.empty(N, device=dev).normal_(generator=g)
                for bb in B_BLOCKS:
                    gs = bb if bb else K
                    s, o = torch.empty(-(-K // gs), N, device=dev), torch.empty(-(-K // gs), N, device=dev)
                    ops.scale_init_group_minmax(w, s, o, -8, 7, gs, rounding="nearest")
                    a = [ops.i8_operand_quantize(x, 0) for _ in range(args.sets)]
                    aff = [ops.i8_operand_pack(w, s, -8, 7, gs, "nearest", o) for _ in range(args.sets)]
                    sym = [ops.I8Operand(*op) for op in aff]      # the same codes and scales, no offsets: the parent's product
                    if workload == "gemm":
                        ys = [torch.empty(M, N, device=dev) for _ in range(args.sets)]
                        dA = [ops.i8_operand_decode(op) for op in a]
                        dBt = [ops.i8_operand_decode(op).t().contiguous() for op in aff]
                        variants = {"symmetric": lambda k: ops.i8_gemm(a[k], sym[k], bias, out=ys[k]),
                                    "affine": lambda k: ops.i8_gemm(a[k], aff[k], bias, out=ys[k]),
                                    "torch_matmul_fp32": lambda k: torch.matmul(dA[k], dBt[k], out=ys[k])}
                    else:
                        variants = {"symmetric": lambda k: ops.i8_gemm_quantize(a[k], sym[k], bias, "relu"),
                                    "affine": lambda k: ops.i8_gemm_quantize(a[k], aff[k], bias, "relu")}
                    times = timed(variants, args.sets, args.rounds, args.inner, dev)
                    row = {"workload": workload, "M": M, "K": K, "N": N, "a_block": 0, "b_block": bb, "repeat": repeat,
                           "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets}
                    for n in variants:
                        us = statistics.median(times[n])
                        row[f"us_{n}"], row[f"us_{n}_min_max"] = us, [min(times[n]), max(times[n])]
                        row[f"tops_{n}"] = 2.0 * M * N * K / us * 1e-6
                    row["affine_over_symmetric"] = row["us_affine"] / row["us_symmetric"]
                    row["expected_at_most"] = EXPECTED[workload]
                    if "us_torch_matmul_fp32" in row:
                        row["affine_over_matmul"] = row["us_affine"] / row["us_torch_matmul_fp32"]
                    emit(row)
                    del variants, a, aff, sym
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
