"""Times the direct int8 convolution (conv.call_i8_direct: ops.i8_pixels_quantize + ops.i8_conv2d) on the nine conv shapes of
tools/bench_mx_conv.py against the yardsticks on the same tensors: the im2col path (call_i8 with act_block 0 and 128) and
F.conv2d in fp32 on NCHW input.  The variants alternate inside one process (tools/bench_mx_gemm.timed: order rotated every round,
every shape warmed), three repeats with fresh data; one JSON line per shape and repeat: the median microseconds of the pixel
quantizer, the product and the whole call, the yardsticks, and the ratios.

    python tools/bench_i8_direct.py --out profiles/i8_direct/bench.jsonl
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
            layer = lq.CustomConv2DLayer(filters=co, kernel_size=(k, k), strides=(stride, stride), padding="same", orientation="scalar",
                                         bits=8, scale_gradient="ste", initializer=lq.RandomNormal(seed=7), input_shape=C, device=dev).eval()
            layer.init_scales("absmax")
            top, bottom, left, right = padding = layer._mx_padding(H, W)
            with torch.no_grad():
                direct, im2col = layer.i8_direct_operand(), layer.i8_operand()
                w, qb = (t.detach() for t in layer.quantized_parameters())
                w = w.contiguous()
            xs = [torch.empty(B, C, H, W, device=dev).normal_(generator=gen) for _ in range(args.sets)]
            pixels = [ops.i8_pixels_quantize(x) for x in xs]
            M = ops.mx_im2col_dims((B, C, H, W), (k, k), (stride, stride), padding)[0]
            out = torch.empty((M, co), device=dev)

            def conv2d(i):
                if top == bottom and left == right:
                    y = F.conv2d(xs[i], w, None, layer.strides, (top, left))
                else:
                    y = F.conv2d(F.pad(xs[i], (left, right, top, bottom)), w, None, layer.strides, 0)
                return torch.add(y, qb.view(1, -1, 1, 1))

            variants = {
                "conv2d_fp32": conv2d,
                "call_i8_act0": lambda i: layer._matrix_conv(xs[i], im2col, qb, layers._I8, (0,)),
                "call_i8_act128": lambda i: layer._matrix_conv(xs[i], im2col, qb, layers._I8, (128,)),
                "direct": lambda i: layer._direct_conv(xs[i], direct, qb),
                "direct_pixels": lambda i: ops.i8_pixels_quantize(xs[i]),
                "direct_product": lambda i: ops.i8_conv2d(pixels[i], direct, qb, layer.strides, padding, out=out),
            }
            t = timed(variants, args.sets, args.rounds, args.inner, dev)
            med = {n: statistics.median(v) for n, v in t.items()}
            rec = {"shape": name, "repeat": repeat, "B": B, "C": C, "H": H, "W": W, "co": co, "k": k, "stride": stride, "M": M,
                   **{f"{n}_us": round(med[n], 2) for n in med},
                   **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                   "direct_over_call_i8_act0": round(med["direct"] / med["call_i8_act0"], 3),
                   "direct_over_call_i8_act128": round(med["direct"] / med["call_i8_act128"], 3),
                   "direct_over_conv2d_fp32": round(med["direct"] / med["conv2d_fp32"], 3)}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
