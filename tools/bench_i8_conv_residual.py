"""Times the direct int8 convolution's residual epilogue (ops.i8_conv2d_quantize with ``residual=``: conv, BatchNorm affine, the
shortcut's add, relu and the next conv's pixel operand in one launch) against the composition it replaces on the same operands --
ops.i8_conv2d -> torch mul, add -> add of the residual, decoded to fp32 beforehand (the composition is not charged for the
decode) -> relu -> ops.i8_pixels_quantize -- and against the same epilogue without a residual, on the 3 x 3 convs of the
ResNet-18 basic blocks at batch 32: the four stride-1 shapes and the two stride-2 ones up to 256 filters.  The variants alternate
inside one process (tools/bench_mx_gemm.timed: order rotated every round, every shape warmed), three repeats with fresh data; one
JSON line per shape and repeat: the median microseconds of each, the composition's fastest round, and the ratios.  The mark: the
fused median at or below the composition's fastest round.

    python tools/bench_i8_conv_residual.py --out profiles/i8_conv_residual/bench.jsonl
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
from tools.bench_mx_gemm import timed  # noqa: E402

SHAPES = [("block_64_56", 32, 64, 56, 56, 64, 1), ("block_128_28", 32, 128, 28, 28, 128, 1), ("block_256_14", 32, 256, 14, 14, 256, 1),
          ("block_512_7", 32, 512, 7, 7, 512, 1), ("block_64_128_56s2", 32, 64, 56, 56, 128, 2), ("block_128_256_28s2", 32, 128, 28, 28, 256, 2)]


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
        for name, B, C, H, W, co, stride in SHAPES:
            layer = lq.CustomConv2DLayer(filters=co, kernel_size=(3, 3), strides=(stride, stride), padding="same", orientation="scalar",
                                         bits=8, scale_gradient="ste", initializer=lq.RandomNormal(seed=7), input_shape=C, device=dev).eval()
            layer.init_scales("absmax")
            padding = layer._mx_padding(H, W)
            with torch.no_grad():
                operand = layer.i8_direct_operand()
                qb = layer.nested_q_b_layer(layer.b).detach()
            g = torch.empty(co, device=dev).normal_(1.0, 0.25, generator=gen)
            h = torch.empty(co, device=dev).normal_(generator=gen)
            pixels = [ops.i8_pixels_quantize(torch.empty(B, C, H, W, device=dev).normal_(generator=gen)) for _ in range(args.sets)]
            M, _, OH, OW = ops.mx_im2col_dims((B, C, H, W), (3, 3), (stride, stride), padding)
            residuals = [ops.i8_pixels_quantize(torch.empty(B, co, OH, OW, device=dev).normal_(generator=gen)) for _ in range(args.sets)]
            decoded = [(r.codes[..., :co].view(torch.int8).float() * r.scales.unsqueeze(-1)).reshape(M, co) for r in residuals]
            out = torch.empty((M, co), device=dev)

            def composition(i):
                y = ops.i8_conv2d(pixels[i], operand, qb, layer.strides, padding, out=out)
                y = torch.relu(y.mul(g).add(h).add(decoded[i]))
                return ops.i8_pixels_quantize(y.view(B, OH, OW, co).permute(0, 3, 1, 2))

            variants = {
                "fused": lambda i: ops.i8_conv2d_quantize(pixels[i], operand, qb, layer.strides, padding, "relu", (g, h), True, residuals[i]),
                "composition": composition,
                "no_residual": lambda i: ops.i8_conv2d_quantize(pixels[i], operand, qb, layer.strides, padding, "relu", (g, h), True),
            }
            t = timed(variants, args.sets, args.rounds, args.inner, dev)
            med = {n: statistics.median(v) for n, v in t.items()}
            rec = {"shape": name, "repeat": repeat, "B": B, "C": C, "H": H, "W": W, "co": co, "k": 3, "stride": stride, "M": M,
                   **{f"{n}_us": round(med[n], 2) for n in med},
                   **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                   "composition_fastest_us": round(min(t["composition"]), 2),
                   "fused_over_composition": round(med["fused"] / med["composition"], 3),
                   "fused_over_composition_fastest": round(med["fused"] / min(t["composition"]), 3),
                   "fused_over_no_residual": round(med["fused"] / med["no_residual"], 3),
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
