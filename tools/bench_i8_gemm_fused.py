#!/usr/bin/env python3
"""The operand-out epilogue of the int8 GEMM (lq_i8_gemm_quantize) next to what it replaces, in one process.  The protocol is
tools/bench_mx_gemm.py's: rotating buffer sets, every round times each variant once (an event-timed run of ``--inner``
back-to-back calls), the order of the variants rotates from round to round, the figure is the median over the rounds in
microseconds per call, and the whole comparison is repeated ``--repeats`` times.

Per shape (M, K, N), 8-bit activations times an 8-bit weight operand with one scale per line (b_block = 0) and a bias, once with
one activation scale per row (a_block = 0) and once with a_block = 64 -- what a chain feeds its second layer:

  * ``gemm``         (a) lq_i8_gemm alone: the fp32 Y.
  * ``composition``  (b) lq_i8_gemm -> F.relu -> lq_i8_operand_quantize(block 64): three launches, Y written, read, written and read
                         again.  What the model runs between two integer Dense layers without the epilogue: the yardstick.
  * ``fused``        (c) lq_i8_gemm_quantize with LQ_ACT_RELU: one launch, the next operand only.

One JSON line per shape, a_block and repeat: the three medians, their min / max over the rounds, fused / composition and
fused / gemm.  us_gemm of the a_block = 64 line over that of the a_block = 0 line is the price of one-step periods.

    python tools/bench_i8_gemm_fused.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from learned_quantization_amd import _hip, ops  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402

SHAPES = [(256, 784, 128), (256, 4096, 4096), (4096, 4096, 4096), (16384, 4096, 4096)]      # (M, K, N)
A_BLOCKS = [0, 64]
OUT_BLOCK = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib, sp, ptr = _hip.load(), _hip.stream_ptr(dev), _hip.ptr
    lines = []
    for repeat in range(args.repeats):
        g = torch.Generator(device=dev).manual_seed(42 + repeat)
        for M, K, N in SHAPES:
            x = torch.empty(M, K, device=dev).normal_(generator=g)
            w = torch.empty(N, K, device=dev).normal_(generator=g) * 0.05
            bias = torch.empty(N, device=dev).normal_(generator=g) * 0.1
            b = [ops.i8_operand_quantize(w, 0) for _ in range(args.sets)]
            ys = [torch.empty(M, N, device=dev) for _ in range(args.sets)]
            outs = [ops._i8_operand_buffers(M, N, OUT_BLOCK, dev) for _ in range(args.sets)]
            del w
            for a_block in A_BLOCKS:
                a = [ops.i8_operand_quantize(x, a_block) for _ in range(args.sets)]

                def gemm(k):
                    _hip.check(lib.lq_i8_gemm(ptr(a[k].codes), ptr(a[k].scales), a_block, ptr(b[k].codes), ptr(b[k].scales), 0, ptr(bias),
                                              ptr(ys[k]), N, M, N, K, sp), "lq_i8_gemm")

                def composition(k):
                    gemm(k)
                    h = F.relu(ys[k])
                    _hip.check(lib.lq_i8_operand_quantize(ptr(h), M, N, OUT_BLOCK, ptr(outs[k][0]), ptr(outs[k][1]), sp),
                               "lq_i8_operand_quantize")

                def fused(k):
                    _hip.check(lib.lq_i8_gemm_quantize(ptr(a[k].codes), ptr(a[k].scales), a_block, ptr(b[k].codes), ptr(b[k].scales), 0,
                                                       ptr(bias), 1, OUT_BLOCK, ptr(outs[k][0]), ptr(outs[k][1]), M, N, K, sp),
                               "lq_i8_gemm_quantize")

                # the two paths write the same bytes: checked here once, outside the clock
                composition(0)
                want = (outs[0][0].clone(), outs[0][1].clone())
                outs[0][0].fill_(0xEE)
                outs[0][1].fill_(-7.0)
                fused(0)
                torch.cuda.synchronize(dev)
                if not (torch.equal(outs[0][0], want[0]) and torch.equal(outs[0][1].view(torch.int32), want[1].view(torch.int32))):
                    raise SystemExit(f"{(M, K, N)} a_block {a_block}: the fused buffers differ from the composition's")
                del want
                variants = {"gemm": gemm, "composition": composition, "fused": fused}
                times = timed(variants, args.sets, args.rounds, args.inner, dev)
                row = {"workload": "i8_gemm_quantize", "M": M, "K": K, "N": N, "a_block": a_block, "b_block": 0, "out_block": OUT_BLOCK,
                       "activation": "relu", "repeat": repeat, "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets}
                for n in variants:
                    row[f"us_{n}"], row[f"us_{n}_min_max"] = statistics.median(times[n]), [min(times[n]), max(times[n])]
                row["fused_over_composition"] = row["us_fused"] / row["us_composition"]
                row["fused_over_gemm"] = row["us_fused"] / row["us_gemm"]
                line = json.dumps(row)
                print(line, flush=True)
                lines.append(line)
                del a
            del x, b, ys, outs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
