#!/usr/bin/env python3
"""A conv layer on the int8 GEMM (ops.i8_operand_im2col -> ops.i8_gemm, what ``call_i8`` and ``i8_hardware(convs=True)`` run) next to
its yardsticks, in one process.  The shapes and the protocol are tools/bench_mx_conv.py's: rotating buffer sets, every round times
each variant once (an event-timed run of ``--inner`` back-to-back calls), the order of the variants rotates from round to round, the
figure is the median over the rounds in microseconds per call, every shape is warmed on every buffer set before it is timed, and the
whole comparison is repeated ``--repeats`` times.

Per shape, an 8-bit layer with a scalar scale (and, for ``call_mx``, an fp8_e4m3 layer of the same geometry); operands and
fake-quantised parameters are built once, outside the clock.  With B in {0, 128}, the activation's scale block:

  * ``i8_im2col_bB``    lq_i8_operand_im2col alone, into pre-allocated buffers (NCHW input); ``i8_im2col_bB_hbm_share`` is the bytes the
                        algorithm needs -- X once plus the code and scale bytes -- over its time, as a share of ``--hbm-tbs``.
  * ``mx_im2col``       lq_mx_operand_im2col fp8_e4m3 on the same geometry: it writes the same number of code bytes.
  * ``quantize_bB``     lq_i8_operand_quantize on the materialised im2col matrix (built outside the clock).
  * ``composition_bB``  F.pad -> F.unfold -> transposing copy -> i8_operand_quantize: the operand as it could already be built.
  * ``call_i8_bB``      the layer's hardware path on an NCHW-contiguous input: lq_i8_operand_im2col -> lq_i8_gemm.
  * ``call_mx``         the fp8_e4m3 layer's path with fp8_e4m3 activations: lq_mx_operand_im2col -> lq_mx_gemm.
  * ``conv2d_nchw`` / ``conv2d_nhwc``   F.conv2d in fp32 with the fake-quantised kernel plus the bias add, NCHW and channels-last input.

Before a shape is timed, the im2col operand is checked byte for byte against the composition's.  One JSON line per shape and repeat.

    python tools/bench_i8_conv.py [--rounds 9] [--inner 5] [--sets 3] [--repeats 3] [--out FILE]
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
from tools.bench_mx_conv import SHAPES  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402

BLOCKS = (0, 128)
MX_FORMAT = "fp8_e4m3"


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
    fa = ops.ELEMENT_FORMATS[MX_FORMAT].id
    lines = []
    for repeat in range(args.repeats):
        gen = torch.Generator(device=dev).manual_seed(42 + repeat)
        for name, B, C, H, W, co, k, stride in SHAPES:
            kw = dict(filters=co, kernel_size=(k, k), strides=(stride, stride), padding="same", initializer=lq.RandomNormal(seed=7),
                      input_shape=C, device=dev)
            layer = lq.CustomConv2DLayer(orientation="scalar", bits=8, scale_gradient="ste", **kw).eval()
            layer.init_scales("absmax")
            mx_layer = lq.CustomConv2DLayer(orientation="groupwise", element_format=MX_FORMAT, **kw).eval()
            mx_layer.init_scales("cover")
            padding = layer._mx_padding(H, W)
            M, K, OH, OW = ops.mx_im2col_dims((B, C, H, W), (k, k), (stride, stride), padding)
            top, bottom, left, right = padding
            with torch.no_grad():
                operand, mx_operand = layer.i8_operand(), mx_layer.mx_operand()
                w, qb = (t.detach() for t in layer.quantized_parameters())
                w = w.contiguous()
                mx_qb = mx_layer.nested_q_b_layer(mx_layer.b).detach()
            xs = [torch.empty(B, C, H, W, device=dev).normal_(generator=gen) for _ in range(args.sets)]
            xl = [x.contiguous(memory_format=torch.channels_last) for x in xs]

            def unfolded(i):
                u = F.unfold(F.pad(xs[i], (left, right, top, bottom)), (k, k), stride=(stride, stride))
                return u.transpose(1, 2).reshape(M, K).contiguous()

            mats = [unfolded(i) for i in range(args.sets)]
            bufs = {b: [ops._i8_operand_buffers(M, K, b, dev) for _ in range(args.sets)] for b in BLOCKS}
            mx_bufs = [ops._mx_operand_buffers(MX_FORMAT, M, K, dev) for _ in range(args.sets)]
            geoms = [ops._conv_geom(x.shape, x.stride(), (k, k), (stride, stride), padding) for x in xs]

            def conv2d(x):
                if top == bottom and left == right:
                    y = F.conv2d(x, w, None, layer.strides, (top, left))
                else:
                    y = F.conv2d(F.pad(x, (left, right, top, bottom)), w, None, layer.strides, 0)
                return torch.add(y, qb.view(1, -1, 1, 1))

            def i8_im2col(b):
                def run(i):
                    _hip.check(lib.lq_i8_operand_im2col(ptr(xs[i]), ctypes.byref(geoms[i]), b, ptr(bufs[b][i][0]), ptr(bufs[b][i][1]), sp),
                               "lq_i8_operand_im2col")
                return run

            def quantize(b):
                def run(i):
                    _hip.check(lib.lq_i8_operand_quantize(ptr(mats[i]), M, K, b, ptr(bufs[b][i][0]), ptr(bufs[b][i][1]), sp),
                               "lq_i8_operand_quantize")
                return run

            def mx_im2col(i):
                _hip.check(lib.lq_mx_operand_im2col(ptr(xs[i]), ctypes.byref(geoms[i]), fa, 0, ptr(mx_bufs[i][0]), ptr(mx_bufs[i][1]), sp),
                           "lq_mx_operand_im2col")

            variants = {"mx_im2col": mx_im2col,
                        "call_mx": lambda i: mx_layer._matrix_conv(xs[i], mx_operand, mx_qb, layers._MX, (MX_FORMAT, "mx")),
                        "conv2d_nchw": lambda i: conv2d(xs[i]), "conv2d_nhwc": lambda i: conv2d(xl[i])}
            for b in BLOCKS:
                variants[f"i8_im2col_b{b}"] = i8_im2col(b)
                variants[f"quantize_b{b}"] = quantize(b)
                variants[f"composition_b{b}"] = lambda i, b=b: ops.i8_operand_quantize(unfolded(i), b)
                variants[f"call_i8_b{b}"] = lambda i, b=b: layer._matrix_conv(xs[i], operand, qb, layers._I8, (b,))

            with torch.no_grad():
                for b in BLOCKS:                               # the gathered operand equals the composition's byte for byte: checked once
                    want = ops.i8_operand_quantize(mats[0], b)
                    got = ops.i8_operand_im2col(xs[0], (k, k), (stride, stride), padding, b)
                    if not (torch.equal(got.codes, want.codes) and torch.equal(got.scales.view(torch.int32), want.scales.view(torch.int32))):
                        raise SystemExit(f"{name}: the im2col operand differs from the composition's at block {b}")
                    del want, got
                for i in range(args.sets):                     # every shape warmed on every buffer set
                    for fn in variants.values():
                        fn(i)
                times = timed(variants, args.sets, args.rounds, args.inner, dev)
            row = {"workload": "i8_conv", "shape": name, "B": B, "C": C, "H": H, "W": W, "co": co, "kernel": k, "stride": stride, "M": M, "K": K,
                   "mx_format": MX_FORMAT, "repeat": repeat, "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets}
            for n in variants:
                row[f"us_{n}"], row[f"us_{n}_min_max"] = statistics.median(times[n]), [min(times[n]), max(times[n])]
            for b in BLOCKS:
                row[f"i8_im2col_b{b}_over_mx_im2col"] = row[f"us_i8_im2col_b{b}"] / row["us_mx_im2col"]
                row[f"i8_im2col_b{b}_over_quantize"] = row[f"us_i8_im2col_b{b}"] / row[f"us_quantize_b{b}"]
                row[f"i8_im2col_b{b}_over_composition"] = row[f"us_i8_im2col_b{b}"] / row[f"us_composition_b{b}"]
                row[f"call_i8_b{b}_over_call_mx"] = row[f"us_call_i8_b{b}"] / row["us_call_mx"]
                row[f"call_i8_b{b}_over_conv2d_nchw"] = row[f"us_call_i8_b{b}"] / row["us_conv2d_nchw"]
                row[f"call_i8_b{b}_over_conv2d_nhwc"] = row[f"us_call_i8_b{b}"] / row["us_conv2d_nhwc"]
                need = B * C * H * W * 4 + bufs[b][0][0].numel() + bufs[b][0][1].numel() * 4
                row[f"i8_im2col_b{b}_hbm_share"] = need / (row[f"us_i8_im2col_b{b}"] * 1e-6) / (args.hbm_tbs * 1e12)
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            del xs, xl, mats, bufs, mx_bufs, layer, mx_layer, operand, mx_operand, w
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
