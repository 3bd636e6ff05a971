#!/usr/bin/env python3
"""The operand-out epilogue of the block-scaled GEMM (lq_mx_gemm_quantize) next to what it replaces, in one process.  The protocol
is tools/bench_mx_gemm.py's: rotating buffer sets, every round times each variant once (an event-timed run of ``--inner``
back-to-back calls), the order of the variants rotates from round to round, the figure is the median over the rounds in
microseconds per call, and the whole comparison is repeated ``--repeats`` times.

Per shape (M, K, N), fp8_e4m3 activations times fp4_e2m1 weights with a bias, and per output format (fp8_e4m3, fp4_e2m1):

  * ``gemm``         (a) lq_mx_gemm alone: the fp32 Y.
  * ``composition``  (b) lq_mx_gemm -> F.relu -> lq_mx_operand_quantize: three launches, Y written, read, written and read again.
                         What CustomDenseLayer._matrix_product and the model run between two MX layers without the epilogue: the yardstick.
  * ``fused``        (c) lq_mx_gemm_quantize with LQ_ACT_RELU: one launch, the next operand only.

One JSON line per shape, output format and repeat: the three medians, their min / max over the rounds, fused / composition and
fused / gemm.

    python tools/bench_mx_gemm_fused.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out FILE]
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
A_FORMAT, B_FORMAT = "fp8_e4m3", "fp4_e2m1"
OUT_FORMATS = ["fp8_e4m3", "fp4_e2m1"]


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
    fa, fb = ops.ELEMENT_FORMATS[A_FORMAT].id, ops.ELEMENT_FORMATS[B_FORMAT].id
    lines = []
    for repeat in range(args.repeats):
        g = torch.Generator(device=dev).manual_seed(42 + repeat)
        for M, K, N in SHAPES:
            x = torch.empty(M, K, device=dev).normal_(generator=g)
            w = torch.empty(K, N, device=dev).normal_(generator=g) * 0.05
            bias = torch.empty(N, device=dev).normal_(generator=g) * 0.1
            s = torch.empty(-(-K // 32), N, device=dev)
            ops.scale_init_mx(w, s, B_FORMAT, 32, "cover", min_value=2.0 ** -126)
            a = [ops.mx_operand_quantize(x, A_FORMAT, "mx") for _ in range(args.sets)]
            b = [ops.mx_operand_pack(w, s, B_FORMAT) for _ in range(args.sets)]
            ys = [torch.empty(M, N, device=dev) for _ in range(args.sets)]
            del x, w
            for out_format in OUT_FORMATS:
                fo = ops.ELEMENT_FORMATS[out_format].id
                outs = [ops._mx_operand_buffers(out_format, M, N, dev) for _ in range(args.sets)]

                def gemm(k):
                    _hip.check(lib.lq_mx_gemm(ptr(a[k].codes), ptr(a[k].scales), fa, ptr(b[k].codes), ptr(b[k].scales), fb, ptr(bias),
                                              ptr(ys[k]), M, N, K, N, sp), "lq_mx_gemm")

                def composition(k):
                    gemm(k)
                    h = F.relu(ys[k])
                    _hip.check(lib.lq_mx_operand_quantize(ptr(h), fo, 0, M, N, ptr(outs[k][0]), ptr(outs[k][1]), sp), "lq_mx_operand_quantize")

                def fused(k):
                    _hip.check(lib.lq_mx_gemm_quantize(ptr(a[k].codes), ptr(a[k].scales), fa, ptr(b[k].codes), ptr(b[k].scales), fb,
                                                       ptr(bias), 1, fo, 0, ptr(outs[k][0]), ptr(outs[k][1]), M, N, K, sp),
                               "lq_mx_gemm_quantize")

                # the two paths write the same bytes: checked here once, outside the clock
                composition(0)
                want = (outs[0][0].clone(), outs[0][1].clone())
                outs[0][0].fill_(0xEE)
                outs[0][1].fill_(0xEE)
                fused(0)
                torch.cuda.synchronize(dev)
                if not (torch.equal(outs[0][0], want[0]) and torch.equal(outs[0][1], want[1])):
                    raise SystemExit(f"{(M, K, N)} -> {out_format}: the fused buffers differ from the composition's")
                del want
                variants = {"gemm": gemm, "composition": composition, "fused": fused}
                times = timed(variants, args.sets, args.rounds, args.inner, dev)
                row = {"workload": "gemm_quantize", "M": M, "K": K, "N": N, "a_format": A_FORMAT, "b_format": B_FORMAT,
                       "out_format": out_format, "activation": "relu", "repeat": repeat, "rounds": args.rounds, "inner": args.inner,
                       "buffer_sets": args.sets}
                for n in variants:
                    row[f"us_{n}"], row[f"us_{n}_min_max"] = statistics.median(times[n]), [min(times[n]), max(times[n])]
                row["fused_over_composition"] = row["us_fused"] / row["us_composition"]
                row["fused_over_gemm"] = row["us_fused"] / row["us_gemm"]
                line = json.dumps(row)
                print(line, flush=True)
                lines.append(line)
                del outs
            del a, b, ys
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
