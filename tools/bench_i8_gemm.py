#!/usr/bin/env python3
"""The dynamic int8 activation quantizer (lq_i8_operand_quantize) and the int8 GEMM (lq_i8_gemm) next to their yardsticks, in one
process.  The protocol is tools/bench_mx_gemm.py's: rotating buffer sets, every round times each variant once (an event-timed run
of ``--inner`` back-to-back calls), the order of the variants rotates from round to round, the figure is the median over the rounds
in microseconds per call, and the whole comparison is repeated ``--repeats`` times.

  * ``quantize``: lq_i8_operand_quantize of X (M, K) with one scale per row (block 0) and per 128 inputs, next to an fp32 device
    copy of the same tensor.  The quantizer reads 4 bytes and writes about 1 per element; the copy reads 4 and writes 4.  Reported in
    us, in GB/s of the bytes each variant moves and as a fraction of the HBM specification (``--hbm-tbs``, 8 TB/s).
  * ``gemm``: lq_i8_gemm with scale blocks (0, 0) and (128, 128) at M x K x N next to ``torch.matmul`` in fp32 on the decoded
    operands -- what the fake-quantised model evaluates with today -- and next to ops.mx_gemm with fp8_e4m3 x fp8_e4m3 operands of
    the same shape: the same instruction rate in the same tiling, the figure the int8 kernel should sit near.  Reported in us and
    TOP/s (2 M N K per call).

One JSON line per workload, shape and repeat.

    python tools/bench_i8_gemm.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learned_quantization_amd import _hip, ops  # noqa: E402

QUANT_SHAPES = [(16384, 4096)]
QUANT_BLOCKS = [0, 128]
GEMM_SHAPES = [(256, 784, 128), (256, 4096, 4096), (4096, 4096, 4096), (16384, 4096, 4096)]      # (M, K, N)
BLOCK_PAIRS = [(0, 0), (128, 128)]


def timed(variants, sets, rounds, inner, dev):
    """{name: [us per call, one per round]}: the variants interleaved, their order rotated by one every round."""
    names = list(variants)
    for n in names:
        variants[n](0)
    torch.cuda.synchronize(dev)
    times, k = {n: [] for n in names}, 0
    for r in range(rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                variants[n](k % sets)
                k += 1
            b.record()
            torch.cuda.synchronize(dev)
            times[n].append(a.elapsed_time(b) / inner * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM specification in TB/s the bandwidth fractions are taken of")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib, sp, ptr = _hip.load(), _hip.stream_ptr(dev), _hip.ptr
    lines = []

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)

    for repeat in range(args.repeats):
        g = torch.Generator(device=dev).manual_seed(42 + repeat)
        for M, K in QUANT_SHAPES:
            xs = [torch.empty(M, K, device=dev).normal_(generator=g) for _ in range(args.sets)]
            copies = [torch.empty_like(x) for x in xs]
            bufs = {block: [ops._i8_operand_buffers(M, K, block, dev) for _ in range(args.sets)] for block in QUANT_BLOCKS}

            def quantize(block):
                def run(k):
                    c, s = bufs[block][k]
                    _hip.check(lib.lq_i8_operand_quantize(ptr(xs[k]), M, K, block, ptr(c), ptr(s), sp), "lq_i8_operand_quantize")
                return run

            variants = {"copy_fp32": lambda k: copies[k].copy_(xs[k])}
            moved = {"copy_fp32": 8.0 * M * K}
            for block in QUANT_BLOCKS:
                variants[f"quantize_block{block}"] = quantize(block)
                moved[f"quantize_block{block}"] = 4.0 * M * K + sum(ops.i8_operand_bytes(M, K, block))
            times = timed(variants, args.sets, args.rounds, args.inner, dev)
            row = {"workload": "quantize", "M": M, "K": K, "repeat": repeat, "rounds": args.rounds, "inner": args.inner,
                   "buffer_sets": args.sets}
            for n in variants:
                us = statistics.median(times[n])
                row[f"us_{n}"], row[f"us_{n}_min_max"] = us, [min(times[n]), max(times[n])]
                row[f"gbs_{n}"] = moved[n] / us * 1e-3
                row[f"hbm_fraction_{n}"] = moved[n] / us * 1e-6 / args.hbm_tbs
            emit(row)
            del xs, copies, bufs
        for M, K, N in GEMM_SHAPES:
            x = torch.empty(M, K, device=dev).normal_(generator=g)
            w = torch.empty(K, N, device=dev).normal_(generator=g) * 0.05
            ys = [torch.empty(M, N, device=dev) for _ in range(args.sets)]
            variants, decoded = {}, {}
            for ab, bb in BLOCK_PAIRS:
                gs = bb if bb else K
                s = torch.empty(-(-K // gs), N, device=dev)
                ops.scale_init_group(w, s, -128, 127, gs, "absmax", rounding="nearest")
                a = [ops.i8_operand_quantize(x, ab) for _ in range(args.sets)]
                b = [ops.i8_operand_pack(w, s, -128, 127, gs, "nearest") for _ in range(args.sets)]
                variants[f"i8_gemm_{ab}_{bb}"] = (lambda a, b: lambda k: ops.i8_gemm(a[k], b[k], None, out=ys[k]))(a, b)
                if not decoded:
                    decoded = dict(A=[ops.i8_operand_decode(o) for o in a], Bt=[ops.i8_operand_decode(o).t().contiguous() for o in b])
            sm = torch.empty(-(-K // 32), N, device=dev)
            ops.scale_init_mx(w, sm, "fp8_e4m3", 32, "cover", min_value=2.0 ** -126)
            ma = [ops.mx_operand_quantize(x, "fp8_e4m3", "mx") for _ in range(args.sets)]
            mb = [ops.mx_operand_pack(w, sm, "fp8_e4m3") for _ in range(args.sets)]
            variants["mx_gemm_fp8_e4m3_x_fp8_e4m3"] = lambda k: ops.mx_gemm(ma[k], mb[k], None, out=ys[k])
            variants["torch_matmul_fp32"] = lambda k: torch.matmul(decoded["A"][k], decoded["Bt"][k], out=ys[k])
            times = timed(variants, args.sets, args.rounds, args.inner, dev)
            row = {"workload": "gemm", "M": M, "K": K, "N": N, "repeat": repeat, "rounds": args.rounds, "inner": args.inner,
                   "buffer_sets": args.sets}
            for n in variants:
                us = statistics.median(times[n])
                row[f"us_{n}"], row[f"us_{n}_min_max"] = us, [min(times[n]), max(times[n])]
                row[f"tops_{n}"] = 2.0 * M * N * K / us * 1e-6
            for ab, bb in BLOCK_PAIRS:
                row[f"i8_gemm_{ab}_{bb}_over_matmul"] = row[f"us_i8_gemm_{ab}_{bb}"] / row["us_torch_matmul_fp32"]
                row[f"i8_gemm_{ab}_{bb}_over_mx_gemm"] = row[f"us_i8_gemm_{ab}_{bb}"] / row["us_mx_gemm_fp8_e4m3_x_fp8_e4m3"]
            emit(row)
            del variants, decoded, ys, ma, mb
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
