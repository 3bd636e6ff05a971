"""Times the direct int8 convolution's pixel-operand epilogue (ops.i8_conv2d_quantize: conv, relu, affine and the next conv's pixel
operand in one launch) against the composition it replaces on the same operands -- ops.i8_conv2d -> torch relu, mul, add ->
ops.i8_pixels_quantize -- on the 3 x 3 shapes of tools/bench_mx_conv.py with C >= 32, plus the fp32-out ops.i8_conv2d alone for
orientation.  The variants alternate inside one process (tools/bench_mx_gemm.timed: order rotated every round, every shape
warmed), three repeats with fresh data; one JSON line per shape and repeat: the median microseconds of each, the composition's
fastest round, and the ratios.  The mark: the fused median at or below the composition's fastest round.

    python tools/bench_i8_conv_fused.py --out profiles/i8_conv_fused/bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import ops  # noqa: E402
from tools.bench_mx_conv import SHAPES  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402


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
        for name, B, C, H, W, co, k, stride in SHAPES:
            if k != 3 or C < 32:
                continue
            layer = lq.CustomConv2DLayer(filters=co, kernel_size=(k, k), strides=(stride, stride), padding="same", orientation="scalar",
                                         bits=8, scale_gradient="ste", initializer=lq.RandomNormal(seed=7), input_shape=C, device=dev).eval()
            layer.init_scales("absmax")
            padding = layer._mx_padding(H, W)
            with torch.no_grad():
                operand = layer.i8_direct_operand()
                qb = layer.nested_q_b_layer(layer.b).detach()
            g = torch.empty(co, device=dev).normal_(1.0, 0.25, generator=gen)
            h = torch.empty(co, device=dev).normal_(generator=gen)
            pixels = [ops.i8_pixels_quantize(torch.empty(B, C, H, W, device=dev).normal_(generator=gen)) for _ in range(args.sets)]
            M, _, OH, OW = ops.mx_im2col_dims((B, C, H, W), (k, k), (stride, stride), padding)
            out = torch.empty((M, co), device=dev)

            def composition(i):
                y = ops.i8_conv2d(pixels[i], operand, qb, layer.strides, padding, out=out)
                y = torch.relu(y).mul(g).add(h)
                return ops.i8_pixels_quantize(y.view(B, OH, OW, co).permute(0, 3, 1, 2))

            variants = {
                "fused": lambda i: ops.i8_conv2d_quantize(pixels[i], operand, qb, layer.strides, padding, "relu", (g, h), False),
                "composition": composition,
                "conv2d_fp32_out": lambda i: ops.i8_conv2d(pixels[i], operand, qb, layer.strides, padding, out=out),
            }
            t = timed(variants, args.sets, args.rounds, args.inner, dev)
            med = {n: statistics.median(v) for n, v in t.items()}
            rec = {"shape": name, "repeat": repeat, "B": B, "C": C, "H": H, "W": W, "co": co, "k": k, "stride": stride, "M": M,
                   **{f"{n}_us": round(med[n], 2) for n in med},
                   **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                   "composition_fastest_us": round(min(t["composition"]), 2),
                   "fused_over_composition": round(med["fused"] / med["composition"], 3),
                   "fused_over_composition_fastest": round(med["fused"] / min(t["composition"]), 3),
                   "fused_over_conv2d_fp32_out": round(med["fused"] / med["conv2d_fp32_out"], 3),
                   "mark_met": med["fused"] <= min(t["composition"])}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
