#!/usr/bin/env python3
"""A conv layer on the block-scaled GEMM (ops.mx_operand_im2col -> ops.mx_gemm, what ``call_mx`` and ``mx_hardware(convs=True)`` run)
next to what it replaces, in one process.  The protocol is tools/bench_mx_gemm.py's: rotating buffer sets, every round times each
variant once (an event-timed run of ``--inner`` back-to-back calls), the order of the variants rotates from round to round, the
figure is the median over the rounds in microseconds per call, every shape is warmed on every buffer set before it is timed, and the
whole comparison is repeated ``--repeats`` times.

Per shape, an fp4_e2m1 layer with fp8_e4m3 activations (the defaults of mx_hardware); kernel operand, fake-quantised kernel and
fake-quantised bias are built once, outside the clock, as mx_hardware builds them on entry:

  * ``conv2d``       (a) the fake-quantised eval path: F.conv2d in fp32 with the fake-quantised kernel, plus the bias add.
  * ``composition``  (b) what could already be run: F.pad -> F.unfold -> transposing copy -> mx_operand_quantize -> mx_gemm.
  * ``mx_nchw``      (c) the layer's hardware path on an NCHW-contiguous input: lq_mx_operand_im2col -> lq_mx_gemm.
  * ``mx_nhwc``      (c) the same on a channels-last input.
  * ``im2col``           lq_mx_operand_im2col alone, into pre-allocated buffers (NCHW input); ``im2col_hbm_share`` is the bytes the
                         algorithm needs -- X once plus the code and scale bytes -- over its time, as a share of ``--hbm-tbs``.

Before a shape is timed, (c) on both inputs is checked bit for bit against (b).  One JSON line per shape and repeat.

    python tools/bench_mx_conv.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out FILE]
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
import torch.nn.functional as F  # noqa: E402

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import _hip, layers, ops  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402

# (name, B, C, H, W, co, k, stride)
SHAPES = [("cifar_32_1", 256, 3, 32, 32, 32, 3, 1), ("cifar_32_2", 256, 32, 32, 32, 32, 3, 1), ("cifar_64_1", 256, 32, 16, 16, 64, 3, 1),
          ("cifar_64_2", 256, 64, 16, 16, 64, 3, 1), ("cifar_128_1", 256, 64, 8, 8, 128, 3, 1), ("cifar_128_2", 256, 128, 8, 8, 128, 3, 1),
          ("resnet18_stem", 32, 3, 224, 224, 64, 7, 2), ("conv3x3_64_56", 32, 64, 56, 56, 64, 3, 1), ("conv1x1s2_64_128_56", 32, 64, 56, 56, 128, 1, 2)]
W_FORMAT, ACT_FORMAT, ACT_SCALE = "fp4_e2m1", "fp8_e4m3", "mx"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM specification in TB/s the bandwidth share is taken of")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib, sp, ptr = _hip.load(), _hip.stream_ptr(dev), _hip.ptr
    fa = ops.ELEMENT_FORMATS[ACT_FORMAT].id
    lines = []
    for repeat in range(args.repeats):
        gen = torch.Generator(device=dev).manual_seed(42 + repeat)
        for name, B, C, H, W, co, k, stride in SHAPES:
            layer = lq.CustomConv2DLayer(filters=co, kernel_size=(k, k), strides=(stride, stride), padding="same", orientation="groupwise",
                                         element_format=W_FORMAT, initializer=lq.RandomNormal(seed=7), input_shape=C, device=dev).eval()
            layer.init_scales("cover")
            padding = layer._mx_padding(H, W)
            M, K, OH, OW = ops.mx_im2col_dims((B, C, H, W), (k, k), (stride, stride), padding)
            with torch.no_grad():
                operand = layer.mx_operand()
                w, qb = (t.detach() for t in layer.quantized_parameters())
                w = w.contiguous()
            xs = [torch.empty(B, C, H, W, device=dev).normal_(generator=gen) for _ in range(args.sets)]
            xl = [x.contiguous(memory_format=torch.channels_last) for x in xs]
            bufs = [ops._mx_operand_buffers(ACT_FORMAT, M, K, dev) for _ in range(args.sets)]
            geoms = [ops._conv_geom(x.shape, x.stride(), (k, k), (stride, stride), padding) for x in xs]
            top, bottom, left, right = padding

            def conv2d(i):
                x = xs[i]
                if top == bottom and left == right:
                    y = F.conv2d(x, w, None, layer.strides, (top, left))
                else:
                    y = F.conv2d(F.pad(x, (left, right, top, bottom)), w, None, layer.strides, 0)
                return torch.add(y, qb.view(1, -1, 1, 1))

            def composition(i):
                u = F.unfold(F.pad(xs[i], (left, right, top, bottom)), (k, k), stride=(stride, stride))
                a = ops.mx_operand_quantize(u.transpose(1, 2).reshape(M, K).contiguous(), ACT_FORMAT, ACT_SCALE)
                return ops.mx_gemm(a, operand, qb)

            def mx_nchw(i):
                return layer._matrix_conv(xs[i], operand, qb, layers._MX, (ACT_FORMAT, ACT_SCALE))

            def mx_nhwc(i):
                return layer._matrix_conv(xl[i], operand, qb, layers._MX, (ACT_FORMAT, ACT_SCALE))

            def im2col(i):
                _hip.check(lib.lq_mx_operand_im2col(ptr(xs[i]), ctypes.byref(geoms[i]), fa, 0, ptr(bufs[i][0]), ptr(bufs[i][1]), sp),
                           "lq_mx_operand_im2col")

            with torch.no_grad():
                # (c) equals (b) bit for bit at this size: checked once, outside the clock
                want = composition(0).view(B, OH, OW, co).permute(0, 3, 1, 2)
                for fn in (mx_nchw, mx_nhwc):
                    got = fn(0)
                    if got.shape != want.shape or not torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)):
                        raise SystemExit(f"{name}: {fn.__name__} differs from the composition")
                del want, got
                variants = {"conv2d": conv2d, "composition": composition, "mx_nchw": mx_nchw, "mx_nhwc": mx_nhwc, "im2col": im2col}
                for i in range(args.sets):                     # every shape warmed on every buffer set
                    for fn in variants.values():
                        fn(i)
                times = timed(variants, args.sets, args.rounds, args.inner, dev)
            row = {"workload": "mx_conv", "shape": name, "B": B, "C": C, "H": H, "W": W, "co": co, "kernel": k, "stride": stride, "M": M, "K": K,
                   "w_format": W_FORMAT, "act_format": ACT_FORMAT, "repeat": repeat, "rounds": args.rounds, "inner": args.inner,
                   "buffer_sets": args.sets}
            for n in variants:
                row[f"us_{n}"], row[f"us_{n}_min_max"] = statistics.median(times[n]), [min(times[n]), max(times[n])]
            for n in ("mx_nchw", "mx_nhwc"):
                row[f"{n}_over_composition"] = row[f"us_{n}"] / row["us_composition"]
                row[f"{n}_over_conv2d"] = row[f"us_{n}"] / row["us_conv2d"]
            need = B * C * H * W * 4 + bufs[0][0].numel() + bufs[0][1].numel()
            row["im2col_bytes_needed"] = need
            row["im2col_hbm_share"] = need / (row["us_im2col"] * 1e-6) / (args.hbm_tbs * 1e12)
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            del xs, xl, bufs, layer, operand, w
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
