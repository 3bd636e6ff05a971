#!/usr/bin/env python3
"""The int8 GEMM on a packed 4-bit B operand (lq_i8_gemm_w4, lq_i8_gemm_quantize_w4) next to its yardstick, the same product on the
same codes stored in bytes (lq_i8_gemm, lq_i8_gemm_quantize), in one process.  The protocol is tools/bench_i8_gemm.py's: rotating
buffer sets, every round times each variant once (an event-timed run of ``--inner`` back-to-back calls), the order of the variants
rotates from round to round, the figure is the median over the rounds in microseconds per call with its min and max, and the whole
comparison is repeated ``--repeats`` times.  Before a shape is timed the two results are compared bit for bit.

One JSON line per shape, block and repeat: ``us_*`` medians, ``us_*_min_max``, ``w4_over_byte`` (ratio of the medians, < 1: the
packed operand is faster) and ``w4_median_within_byte_max`` (the packed median at or below the yardstick's slowest round).

    python tools/bench_i4_gemm.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out FILE]
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
from tools.bench_i8_gemm import GEMM_SHAPES, timed  # noqa: E402

B_BLOCKS = [0, 128]


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
    for repeat in range(args.repeats):
        g = torch.Generator(device=dev).manual_seed(42 + repeat)
        for M, K, N in GEMM_SHAPES:
            x = torch.empty(M, K, device=dev).normal_(generator=g)
            w = torch.empty(K, N, device=dev).normal_(generator=g) * 0.05
            ys = [torch.empty(M, N, device=dev) for _ in range(args.sets)]
            for block in B_BLOCKS:
                gs = block if block else K
                s = torch.empty(-(-K // gs), N, device=dev)
                ops.scale_init_group(w, s, -8, 7, gs, "absmax", rounding="nearest")
                a = [ops.i8_operand_quantize(x, block) for _ in range(args.sets)]
                b8 = [ops.i8_operand_pack(w, s, -8, 7, gs, "nearest") for _ in range(args.sets)]
                b4 = [ops.i4_operand_pack(w, s, -8, 7, gs, "nearest") for _ in range(args.sets)]
                y8, y4 = ops.i8_gemm(a[0], b8[0]), ops.i8_gemm(a[0], b4[0])
                q8, q4 = ops.i8_gemm_quantize(a[0], b8[0], None, "relu"), ops.i8_gemm_quantize(a[0], b4[0], None, "relu")
                same = bool(torch.equal(y8.view(torch.int32), y4.view(torch.int32)) and torch.equal(q8.codes, q4.codes)
                            and torch.equal(q8.scales.view(torch.int32), q4.scales.view(torch.int32)))
                del y8, y4, q8, q4
                variants = {
                    "gemm_byte": lambda k: ops.i8_gemm(a[k], b8[k], None, out=ys[k]),
                    "gemm_w4": lambda k: ops.i8_gemm(a[k], b4[k], None, out=ys[k]),
                    "quantize_byte": lambda k: ops.i8_gemm_quantize(a[k], b8[k], None, "relu"),
                    "quantize_w4": lambda k: ops.i8_gemm_quantize(a[k], b4[k], None, "relu"),
                }
                times = timed(variants, args.sets, args.rounds, args.inner, dev)
                row = {"M": M, "K": K, "N": N, "b_block": block, "a_block": block, "repeat": repeat, "rounds": args.rounds,
                       "inner": args.inner, "buffer_sets": args.sets, "bit_identical": same,
                       "b_code_bytes_byte": b8[0].codes.numel(), "b_code_bytes_w4": b4[0].codes.numel()}
                for n in variants:
                    row[f"us_{n}"], row[f"us_{n}_min_max"] = statistics.median(times[n]), [min(times[n]), max(times[n])]
                for kind in ("gemm", "quantize"):
                    row[f"{kind}_w4_over_byte"] = row[f"us_{kind}_w4"] / row[f"us_{kind}_byte"]
                    row[f"{kind}_w4_median_within_byte_max"] = row[f"us_{kind}_w4"] <= max(times[f"{kind}_byte"])
                    row[f"tops_{kind}_w4"] = 2.0 * M * N * K / row[f"us_{kind}_w4"] * 1e-6
                line = json.dumps(row)
                print(line, flush=True)
                lines.append(line)
                del a, b8, b4, variants
            del ys
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
