#!/usr/bin/env python3
"""The block-scaled GEMM with an fp6 side (lq_mx6_gemm) next to the two existing kernels it is measured against, in one process:
fp8_e4m3 x fp8_e4m3 and fp8_e4m3 x fp4_e2m1 (lq_mx_gemm, code this change does not touch).  The protocol is
tools/bench_mx_gemm.py's (its ``timed``): rotating buffer sets, every round times each variant once, the order of the variants
rotates from round to round, the figure is the median over the rounds in microseconds per call, and the whole comparison is repeated
``--repeats`` times.

The mark: on the two large shapes the median of a pair with an fp6 side is at or below the SLOWEST round of fp8 x fp8 -- an fp6
fragment is 24 bytes and 6 registers where fp8's is 32 and 8.  ``met_<pair>`` says whether it was; the 256-row shapes are reported
and not gated.  One JSON line per shape and repeat.

    python tools/bench_mx6_gemm.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out profiles/mx6/bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_mx_gemm import timed  # noqa: E402
from learned_quantization_amd import ops  # noqa: E402

SHAPES = [(4096, 4096, 4096), (16384, 4096, 4096), (256, 4096, 4096), (256, 784, 128)]      # (M, K, N)
GATED = SHAPES[:2]
YARDSTICKS = [("fp8_e4m3", "fp8_e4m3"), ("fp8_e4m3", "fp4_e2m1")]
PAIRS = [("fp8_e4m3", "fp6_e2m3"), ("fp8_e4m3", "fp6_e3m2"), ("fp6_e2m3", "fp6_e2m3"), ("fp6_e3m2", "fp6_e3m2")]


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
        for M, K, N in SHAPES:
            x = torch.empty(M, K, device=dev).normal_(generator=g)
            w = torch.empty(K, N, device=dev).normal_(generator=g) * 0.05
            ys = [torch.empty(M, N, device=dev) for _ in range(args.sets)]
            variants = {}
            for an, bn in YARDSTICKS + PAIRS:
                s = torch.empty(-(-K // 32), N, device=dev)
                ops.scale_init_mx(w, s, bn, 32, "cover", min_value=2.0 ** -126)
                quantize = ops.mx6_operand_quantize if an in ops.MX6_OPERAND_FORMATS else ops.mx_operand_quantize
                pack = ops.mx6_operand_pack if bn in ops.MX6_OPERAND_FORMATS else ops.mx_operand_pack
                a = [quantize(x, an, "mx") for _ in range(args.sets)]
                b = [pack(w, s, bn) for _ in range(args.sets)]
                variants[f"{an}_x_{bn}"] = (lambda a, b: lambda k: ops.mx_gemm(a[k], b[k], None, out=ys[k]))(a, b)
            times = timed(variants, args.sets, args.rounds, args.inner, dev)
            row = {"workload": "mx6_gemm", "M": M, "K": K, "N": N, "repeat": repeat, "rounds": args.rounds, "inner": args.inner,
                   "buffer_sets": args.sets, "gated": (M, K, N) in GATED}
            for n in variants:
                us = statistics.median(times[n])
                row[f"us_{n}"], row[f"us_{n}_min_max"] = us, [min(times[n]), max(times[n])]
                row[f"tflops_{n}"] = 2.0 * M * N * K / us * 1e-6
            slowest = max(times["fp8_e4m3_x_fp8_e4m3"])
            for an, bn in PAIRS:
                n = f"{an}_x_{bn}"
                row[f"{n}_over_fp8_x_fp8"] = row[f"us_{n}"] / row["us_fp8_e4m3_x_fp8_e4m3"]
                row[f"{n}_over_fp8_x_fp4"] = row[f"us_{n}"] / row["us_fp8_e4m3_x_fp4_e2m1"]
                row[f"met_{n}"] = row[f"us_{n}"] <= slowest
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            del variants, ys
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
