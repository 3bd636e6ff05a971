"""Times the stem convolution (conv.call_i8_stem: ops.i8_rows_quantize + ops.i8_stem_conv2d) on the two first-layer shapes of
tools/bench_mx_conv.py -- resnet18_stem (batch 32) and cifar_32_1 (batch 256) -- against the yardsticks on the same tensors: the
im2col path (call_i8, act_block 0), the direct path with its padded channels (call_i8_direct) and F.conv2d in fp32 on NCHW input;
and, on cifar_32_1, the relu + affine pixel-operand epilogue (ops.i8_stem_conv2d_quantize) against ops.i8_pixels_quantize +
ops.i8_conv2d_quantize at C = 3.  The variants alternate inside one process (tools/bench_mx_gemm.timed: order rotated every round,
every shape warmed), three repeats with fresh data; one JSON line per shape and repeat: the median and the fastest round of every
variant in microseconds, and the stem call over the fastest yardstick's fastest round.

THE MARK, stated before measuring: each stem call is at or below the fastest yardstick's fastest round (`meets_mark`).  Counted
bytes of the ResNet stem at batch 32: 19.3 MB of fp32 image read, 6.4 MB of codes written and (through the cache) read, 102.8 MB of
fp32 Y -- about 135 MB against about 275 MB for im2col -- so the call should land near half of the im2col call.

    python tools/bench_i8_stem.py --out profiles/i8_stem/bench.jsonl
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

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import layers, ops  # noqa: E402
from tools.bench_mx_conv import SHAPES  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402

STEM_SHAPES = [s for s in SHAPES if s[0] in ("resnet18_stem", "cifar_32_1")]


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
        gen = torch.Generator(device=dev).manual_seed(42 + repeat)
        for name, B, C, H, W, co, k, stride in STEM_SHAPES:
            layer = lq.CustomConv2DLayer(filters=co, kernel_size=(k, k), strides=(stride, stride), padding="same", orientation="scalar",
                                         bits=8, scale_gradient="ste", initializer=lq.RandomNormal(seed=7), input_shape=C, device=dev).eval()
            layer.init_scales("absmax")
            top, bottom, left, right = padding = layer._mx_padding(H, W)
            with torch.no_grad():
                stem, direct, im2col = layer.i8_stem_operand(), layer.i8_direct_operand(), layer.i8_operand()
                w, qb = (t.detach() for t in layer.quantized_parameters())
                w = w.contiguous()
            xs = [torch.empty(B, C, H, W, device=dev).normal_(generator=gen) for _ in range(args.sets)]
            rows = [ops.i8_rows_quantize(x) for x in xs]
            M = ops.mx_im2col_dims((B, C, H, W), (k, k), (stride, stride), padding)[0]
            out = torch.empty((M, co), device=dev)
            affine = (torch.empty(co, device=dev).normal_(1.0, 0.5, generator=gen), torch.empty(co, device=dev).normal_(generator=gen))

            def conv2d(i):
                if top == bottom and left == right:
                    y = F.conv2d(xs[i], w, None, layer.strides, (top, left))
                else:
                    y = F.conv2d(F.pad(xs[i], (left, right, top, bottom)), w, None, layer.strides, 0)
                return torch.add(y, qb.view(1, -1, 1, 1))

            yardsticks = {
                "conv2d_fp32": conv2d,
                "call_i8_act0": lambda i: layer._matrix_conv(xs[i], im2col, qb, layers._I8, (0,)),
                "direct": lambda i: layer._direct_conv(xs[i], direct, qb),
            }
            variants = {
                **yardsticks,
                "stem": lambda i: layer._direct_step(xs[i], stem, qb),
                "stem_rows": lambda i: ops.i8_rows_quantize(xs[i]),
                "stem_product": lambda i: ops.i8_stem_conv2d(rows[i], stem, qb, layer.strides, padding, out=out),
            }
            pairs = {"stem": list(yardsticks)}
            if name == "cifar_32_1":      # the relu + affine pixel-operand epilogue, against the parent's two launches at C = 3
                variants["direct_quantize"] = lambda i: ops.i8_conv2d_quantize(ops.i8_pixels_quantize(xs[i]), direct, qb, layer.strides,
                                                                               padding, "relu", affine)
                variants["stem_quantize"] = lambda i: ops.i8_stem_conv2d_quantize(ops.i8_rows_quantize(xs[i]), stem, qb, layer.strides,
                                                                                 padding, "relu", affine)
                pairs["stem_quantize"] = ["direct_quantize"]
            with torch.no_grad():
                t = timed(variants, args.sets, args.rounds, args.inner, dev)
            med = {n: statistics.median(v) for n, v in t.items()}
            rec = {"shape": name, "repeat": repeat, "B": B, "C": C, "H": H, "W": W, "co": co, "k": k, "stride": stride, "M": M,
                   **{f"{n}_us": round(med[n], 2) for n in med}, **{f"{n}_min_us": round(min(v), 2) for n, v in t.items()},
                   **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()}}
            for ours, against in pairs.items():
                best = min(against, key=lambda n: min(t[n]))
                rec.update({f"{ours}_fastest_yardstick": best, f"{ours}_over_fastest_yardstick": round(med[ours] / min(t[best]), 3),
                            f"{ours}_meets_mark": med[ours] <= min(t[best]),
                            **{f"{ours}_over_{n}": round(med[ours] / med[n], 3) for n in against}})
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
