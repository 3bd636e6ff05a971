"""Times the direct int8 convolution's pooled pixel-operand epilogue (ops.i8_conv2d_quantize with ``pool=2``: conv, relu, affine,
MaxPool(2) and the next conv's pixel operand in one launch) against the composition it replaces on the same operands --
ops.i8_conv2d -> torch relu, mul, add -> F.max_pool2d -> ops.i8_pixels_quantize -- on the three pooled convs of the CIFAR CNN at
batch 256 and one row-per-block shape, plus the unpooled epilogue on the same conv (the same matrix work, four times the rows to
quantise and store).  The variants alternate inside one process (tools/bench_mx_gemm.timed: order rotated every round, every
shape warmed), three repeats with fresh data; one JSON line per shape and repeat.  The mark: the fused median at or below the
composition's fastest round.  ``--model``: also the CIFAR model's eval forward under ``fused_convs`` with and without
``pooled_convs``, one JSON line per repeat.

    python tools/bench_i8_conv_pool.py --model --out profiles/i8_conv_pool/bench.jsonl
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
from learned_quantization_amd import layers as L, ops  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402

SHAPES = [("cifar_32_2", 256, 32, 32, 32, 32), ("cifar_64_2", 256, 64, 16, 16, 64), ("cifar_128_2", 256, 128, 8, 8, 128),
          ("block_256", 32, 256, 14, 14, 256)]      # (name, B, C, H, W, co): 3 x 3, stride 1, 'same'


def conv_line(name, B, C, H, W, co, repeat, gen, args, dev):
    layer = lq.CustomConv2DLayer(filters=co, kernel_size=(3, 3), strides=(1, 1), padding="same", orientation="scalar", bits=8,
                                 scale_gradient="ste", initializer=lq.RandomNormal(seed=7), input_shape=C, device=dev).eval()
    layer.init_scales("absmax")
    padding = layer._mx_padding(H, W)
    with torch.no_grad():
        operand = layer.i8_direct_operand()
        qb = layer.nested_q_b_layer(layer.b).detach()
    g = torch.empty(co, device=dev).normal_(1.0, 0.25, generator=gen)
    h = torch.empty(co, device=dev).normal_(generator=gen)
    pixels = [ops.i8_pixels_quantize(torch.empty(B, C, H, W, device=dev).normal_(generator=gen)) for _ in range(args.sets)]
    M, _, OH, OW = ops.mx_im2col_dims((B, C, H, W), (3, 3), (1, 1), padding)
    out = torch.empty((M, co), device=dev)

    def composition(i):
        y = ops.i8_conv2d(pixels[i], operand, qb, layer.strides, padding, out=out)
        y = torch.relu(y).mul(g).add(h)
        return ops.i8_pixels_quantize(F.max_pool2d(y.view(B, OH, OW, co).permute(0, 3, 1, 2), 2))

    variants = {
        "fused": lambda i: ops.i8_conv2d_quantize(pixels[i], operand, qb, layer.strides, padding, "relu", (g, h), False, pool=2),
        "composition": composition,
        "unpooled": lambda i: ops.i8_conv2d_quantize(pixels[i], operand, qb, layer.strides, padding, "relu", (g, h), False),
    }
    t = timed(variants, args.sets, args.rounds, args.inner, dev)
    med = {n: statistics.median(v) for n, v in t.items()}
    return {"shape": name, "repeat": repeat, "B": B, "C": C, "H": H, "W": W, "co": co, "M": M, "PM": B * (OH // 2) * (OW // 2),
            **{f"{n}_us": round(med[n], 2) for n in med},
            **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
            "composition_fastest_us": round(min(t["composition"]), 2),
            "fused_over_composition": round(med["fused"] / med["composition"], 3),
            "fused_over_composition_fastest": round(med["fused"] / min(t["composition"]), 3),
            "fused_over_unpooled": round(med["fused"] / med["unpooled"], 3),
            "mark_met": med["fused"] <= min(t["composition"])}


def model_line(repeat, gen, args, dev):
    def build():      # two copies of one model (the same seed), each inside its own context
        return lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", kernel_storage="oihw", bits=8,
                              orientation="scalar").eval()
    plain, pooled = build(), build()
    xs = [torch.rand(256, 3, 32, 32, device=dev, generator=gen) for _ in range(args.sets)]
    with torch.no_grad(), L.i8_hardware(plain, convs=True, direct=True, fused_convs=True), \
            L.i8_hardware(pooled, convs=True, direct=True, fused_convs=True, pooled_convs=True):
        t = timed({"fused_convs": lambda i: plain(xs[i]), "pooled_convs": lambda i: pooled(xs[i])}, args.sets, args.rounds, args.inner, dev)
    med = {n: statistics.median(v) for n, v in t.items()}
    return {"shape": "cifar_model_eval_b256", "repeat": repeat, **{f"{n}_us": round(med[n], 2) for n in med},
            **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
            "pooled_over_fused": round(med["pooled_convs"] / med["fused_convs"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", action="store_true", help="also time the CIFAR model's eval forward with and without pooled_convs")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for repeat in range(args.repeats):
        gen = torch.Generator(device=dev).manual_seed(42 + repeat)
        recs = [conv_line(*shape, repeat, gen, args, dev) for shape in SHAPES] + ([model_line(repeat, gen, args, dev)] if args.model else [])
        for rec in recs:
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
