"""Times the wide pixel-operand epilogue of the direct int8 convolution (ops.i8_conv2d_quantize with ``wide=True`` and more than 512
filters: the output row parked in LDS, csrc/lq_i8_direct_quant_wide.hpp) against the composition it replaces on the same operands
-- ops.i8_conv2d -> torch mul, add (-> add of the residual, decoded to fp32 beforehand: the composition is not charged for the
decode -> relu) -> ops.i8_pixels_quantize -- on the ResNet-50 shapes at batch 32: the expanding 1 x 1 convs 256 -> 1024 @ 14^2 and
512 -> 2048 @ 7^2 (with the block's residual and relu) and the stride-2 projection shortcuts 512 -> 1024 and 1024 -> 2048 (affine
only).  One more shape, 128 -> 512 @ 28^2 with a residual, runs the wide kernel through its C entry point against the shipped
row-per-block form on the same operands: what the parking costs.  The variants alternate inside one process
(tools/bench_mx_gemm.timed: order rotated every round, every shape warmed), three repeats with fresh data; one JSON line per shape
and repeat: the median microseconds of each, the yardstick's fastest round, and the ratios.  The mark: the fused median at or
below the composition's fastest round.

    python tools/bench_i8_conv_wide.py --out profiles/i8_conv_wide/bench.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import _hip, ops  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402

# (name, B, C, H, W, co, stride, the block's residual and relu)
SHAPES = [("expand_256_1024_14", 32, 256, 14, 14, 1024, 1, True), ("expand_512_2048_7", 32, 512, 7, 7, 2048, 1, True),
          ("shortcut_512_1024_28s2", 32, 512, 28, 28, 1024, 2, False), ("shortcut_1024_2048_14s2", 32, 1024, 14, 14, 2048, 2, False),
          ("parking_128_512_28", 32, 128, 28, 28, 512, 1, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    lines = []
    for repeat in range(args.repeats):
        gen = torch.Generator(device=dev).manual_seed(42 + repeat)
        for name, B, C, H, W, co, stride, block in SHAPES:
            layer = lq.CustomConv2DLayer(filters=co, kernel_size=(1, 1), strides=(stride, stride), padding="same", orientation="scalar",
                                         bits=8, scale_gradient="ste", initializer=lq.RandomNormal(seed=7), input_shape=C, device=dev).eval()
            layer.init_scales("absmax")
            padding = layer._mx_padding(H, W)
            with torch.no_grad():
                operand = layer.i8_direct_operand()
                qb = layer.nested_q_b_layer(layer.b).detach()
            g = torch.empty(co, device=dev).normal_(1.0, 0.25, generator=gen)
            h = torch.empty(co, device=dev).normal_(generator=gen)
            pixels = [ops.i8_pixels_quantize(torch.empty(B, C, H, W, device=dev).normal_(generator=gen)) for _ in range(args.sets)]
            M, _, OH, OW = ops.mx_im2col_dims((B, C, H, W), (1, 1), (stride, stride), padding)
            residuals = [ops.i8_pixels_quantize(torch.empty(B, co, OH, OW, device=dev).normal_(generator=gen)) if block else None
                         for _ in range(args.sets)]
            decoded = [(r.codes[..., :co].view(torch.int8).float() * r.scales.unsqueeze(-1)).reshape(M, co) if block else None for r in residuals]
            out = torch.empty((M, co), device=dev)
            act = "relu" if block else None

            def composition(i):
                y = ops.i8_conv2d(pixels[i], operand, qb, layer.strides, padding, out=out).mul(g).add(h)
                if block:
                    y = torch.relu(y.add(decoded[i]))
                return ops.i8_pixels_quantize(y.view(B, OH, OW, co).permute(0, 3, 1, 2))

            def fused(i):
                return ops.i8_conv2d_quantize(pixels[i], operand, qb, layer.strides, padding, act, (g, h), True, residuals[i], wide=True)

            geom = ops._conv_geom(pixels[0].shape, (0, 0, 0, 0), operand.kernel_size, layer.strides, padding)
            dst = ops.I8Pixels(torch.empty_like(residuals[0].codes), torch.empty_like(residuals[0].scales), residuals[0].shape) if co <= 512 else None

            def parked(i):        # co <= 512 through the wide kernel: its C entry point, into one preallocated output
                _hip.check(lib.lq_i8_conv2d_quantize_wide(
                    _hip.ptr(pixels[i].codes), _hip.ptr(pixels[i].scales), _hip.ptr(operand.codes), _hip.ptr(operand.scales), _hip.ptr(qb),
                    ctypes.byref(geom), co, _hip.ptr(g), _hip.ptr(h), 1, 1, _hip.ptr(residuals[i].codes), _hip.ptr(residuals[i].scales),
                    _hip.ptr(dst.codes), _hip.ptr(dst.scales), _hip.stream_ptr(dev)), "lq_i8_conv2d_quantize_wide")
                return dst

            if co > 512:
                variants, yard = {"fused": fused, "composition": composition}, "composition"
            else:                 # the yardstick is the shipped row-per-block form (ops routes co <= 512 there)
                assert all(torch.equal(parked(i).codes, fused(i).codes) and torch.equal(dst.scales, fused(i).scales) for i in range(args.sets))
                variants, yard = {"fused": parked, "shipped": fused, "composition": composition}, "shipped"
            t = timed(variants, args.sets, args.rounds, args.inner, dev)
            med = {n: statistics.median(v) for n, v in t.items()}
            rec = {"shape": name, "repeat": repeat, "B": B, "C": C, "H": H, "W": W, "co": co, "k": 1, "stride": stride, "M": M,
                   "residual": block, "yardstick": yard,
                   **{f"{n}_us": round(med[n], 2) for n in med},
                   **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                   f"{yard}_fastest_us": round(min(t[yard]), 2),
                   f"fused_over_{yard}": round(med["fused"] / med[yard], 3),
                   f"fused_over_{yard}_fastest": round(med["fused"] / min(t[yard]), 3),
                   "mark_met": med["fused"] <= min(t[yard])}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
