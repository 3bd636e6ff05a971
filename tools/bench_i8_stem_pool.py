"""Times the stem convolution's pooled epilogue (ops.i8_stem_conv2d_quantize, pool=3: conv -> BatchNorm affine -> relu -> 3 x 3 / 2
maximum -> the next conv's pixel operand, one launch) on the ResNet-18 stem at batch 32 and at batch 256, against the composition on
the parent's kernels with the same operands: ops.i8_stem_conv2d -> torch's affine, relu, F.pad(-inf), F.max_pool2d(3, 2) ->
ops.i8_pixels_quantize.  Reported beside them, not gated: ops.i8_stem_conv2d_quantize without a pool, and (once, at batch 32) the
eval forward of models.ResNet18Like under layers.i8_hardware with and without stem_pool.  The variants alternate inside one
process (tools/bench_mx_gemm.timed: order rotated every round, every shape warmed, device events), three repeats with fresh data;
one JSON line per shape and repeat: the median and the fastest round of every variant in microseconds.

THE MARK, stated before measuring: the pooled call's median is at or below the composition's fastest round, on both shapes, in
every repeat (`meets_mark`).  Counted bytes at batch 32: the composition writes 102.8 MB of fp32 Y and torch's passes read and
write tensors of that order four times; the pooled call reads 6.4 MB of row codes and writes 6.4 MB of pooled codes.

    python tools/bench_i8_stem_pool.py --out profiles/i8_stem_pool/bench.jsonl
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
from tools.bench_mx_gemm import timed  # noqa: E402

SHAPES = [("resnet18_stem_b32", 32, 3, 224, 224, 64, 7, 2), ("resnet18_stem_b256", 256, 3, 224, 224, 64, 7, 2)]


def model_forward(dev, rounds, inner):
    """{variant: [microseconds per round]} of ResNet18Like's eval forward at batch 32 under i8_hardware, with and without stem_pool."""
    model = lq.build_model("imagenette", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", kernel_storage="oihw", bits=8,
                           orientation="scalar").eval()
    x = torch.rand(32, 3, 224, 224, device=dev)
    flags = dict(convs=True, direct=True, fused_convs=True, stem_convs=True)
    out = {}
    with torch.no_grad():
        for name, pool in (("forward_stem_pool", True), ("forward_no_stem_pool", False)):
            with layers.i8_hardware(model, **flags, stem_pool=pool):
                out[name] = timed({name: lambda i: model(x)}, 1, rounds, inner, dev)[name]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-model", action="store_true", help="skip the ResNet18Like forward")
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
            padding = layer._mx_padding(H, W)
            with torch.no_grad():
                stem = layer.i8_stem_operand()
                qb = layer.quantized_parameters()[1].detach()
            rows = [ops.i8_rows_quantize(torch.empty(B, C, H, W, device=dev).normal_(generator=gen)) for _ in range(args.sets)]
            M, _, OH, OW = ops.mx_im2col_dims((B, C, H, W), (k, k), (stride, stride), padding)
            y = torch.empty((M, co), device=dev)
            affine = (torch.empty(co, device=dev).normal_(1.0, 0.5, generator=gen), torch.empty(co, device=dev).normal_(generator=gen))
            pool_padding = (OH % 2, 1, OW % 2, 1)

            def composition(i):
                ops.i8_stem_conv2d(rows[i], stem, qb, layer.strides, padding, out=y)
                v = F.relu(y.view(B, OH, OW, co).permute(0, 3, 1, 2).mul(affine[0].view(1, -1, 1, 1)).add(affine[1].view(1, -1, 1, 1)))
                v = F.pad(v, (pool_padding[2], pool_padding[3], pool_padding[0], pool_padding[1]), value=float("-inf"))
                return ops.i8_pixels_quantize(F.max_pool2d(v, 3, 2))

            variants = {
                "composition": composition,
                "pooled": lambda i: ops.i8_stem_conv2d_quantize(rows[i], stem, qb, layer.strides, padding, "relu", affine, True, pool=3,
                                                                pool_padding=pool_padding),
                "unpooled": lambda i: ops.i8_stem_conv2d_quantize(rows[i], stem, qb, layer.strides, padding, "relu", affine, True),
            }
            with torch.no_grad():
                assert torch.equal(variants["pooled"](0).codes, composition(0).codes)
                t = timed(variants, args.sets, args.rounds, args.inner, dev)
                if name.endswith("b32") and repeat == 0 and not args.no_model:
                    t.update(model_forward(dev, args.rounds, 2))
            med = {n: statistics.median(v) for n, v in t.items()}
            rec = {"shape": name, "repeat": repeat, "B": B, "C": C, "H": H, "W": W, "co": co, "k": k, "stride": stride, "M": M,
                   **{f"{n}_us": round(med[n], 2) for n in med}, **{f"{n}_min_us": round(min(v), 2) for n, v in t.items()},
                   **{f"{n}_spread": round((max(v) - min(v)) / med[n], 3) for n, v in t.items()},
                   "pooled_over_composition_min": round(med["pooled"] / min(t["composition"]), 3),
                   "pooled_over_unpooled": round(med["pooled"] / med["unpooled"], 3), "meets_mark": med["pooled"] <= min(t["composition"])}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
