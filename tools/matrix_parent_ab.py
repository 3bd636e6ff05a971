#!/usr/bin/env python3
"""The conv layers' matrix path of this build next to the parent commit's, in one process (profiles/matrix_shared).

    git worktree add PARENT HEAD~1 && make -C PARENT/learned_quantization_amd/csrc
    python3 tools/matrix_parent_ab.py --parent PARENT [--out FILE]

``--parent`` names a checkout of the parent commit with its library built.  Its package is loaded as a second package,
``lq_parent``, beside this tree's: its own Python and its own liblq_hip.so.  Per shape of tools/bench_mx_conv.py, both sides build
the same seeded layers and time, on the same inputs:

  * ``im2col``        lq_mx_operand_im2col alone (fp8_e4m3, "mx"), into pre-allocated buffers: the kernel.
  * ``mx_nchw``       the layer's block-scaled path (im2col operand -> GEMM) on an NCHW-contiguous input.
  * ``mx_nhwc``       the same on a channels-last input.
  * ``i8_b0``, ``i8_b128``  the layer's int8 path with one scale per line and with scale blocks of 128.

The clock is tools/bench_mx_gemm.py's ``timed``: device events around ``--inner`` back-to-back calls, all ten variants interleaved,
their order rotated every round, the figure the median over the rounds.  That is repeated ``--repeats`` times, parent and new
alternating inside every repeat (the ``--time`` protocol of tools/batch_parent_ab.py).  Before a shape is timed the two sides'
results are compared bit for bit.  One JSON line per shape and variant; exit status 1 unless every new median lies inside or below
the parent's own min-max range."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import learned_quantization_amd as lq_new  # noqa: E402
from tools.bench_mx_conv import ACT_FORMAT, ACT_SCALE, SHAPES, W_FORMAT  # noqa: E402
from tools.bench_mx_gemm import timed  # noqa: E402

I8_BLOCKS = (0, 128)


def load_parent(tree):
    init = os.path.join(os.path.abspath(tree), "learned_quantization_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location("lq_parent", init, submodule_search_locations=[os.path.dirname(init)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lq_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def conv_calls(lq, layer, operand, qb, family):
    """(x, *act) -> the layer's matrix path, under either side's private name for it."""
    if hasattr(layer, "_matrix_conv"):
        fam = getattr(lq.layers, "_MX" if family == "mx" else "_I8")
        return lambda x, *act: layer._matrix_conv(x, operand, qb, fam, act)
    fn = layer._mx_conv if family == "mx" else layer._i8_conv
    return lambda x, *act: fn(x, operand, qb, *act)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="a checkout of the parent commit, its library built")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the JSON lines to this file as well")
    args = ap.parse_args()
    sides = (("parent", load_parent(args.parent)), ("new", lq_new))
    dev = torch.device("cuda:0")
    lines, bad = [], 0
    for name, B, C, H, W, co, k, stride in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(42)
        xs = [torch.empty(B, C, H, W, device=dev).normal_(generator=gen) for _ in range(args.sets)]
        xl = [x.contiguous(memory_format=torch.channels_last) for x in xs]
        variants, keep = {}, []
        for side, lq in sides:
            ops, _hip = lq.ops, lq._hip
            kw = dict(filters=co, kernel_size=(k, k), strides=(stride, stride), padding="same", initializer=lq.RandomNormal(seed=7),
                      input_shape=C, device=dev)
            mx = lq.CustomConv2DLayer(orientation="groupwise", element_format=W_FORMAT, **kw).eval()
            mx.init_scales("cover")
            i8 = lq.CustomConv2DLayer(orientation="scalar", bits=8, scale_gradient="ste", **kw).eval()
            i8.init_scales("absmax")
            padding = (*lq.layers._same_padding(H, k, stride), *lq.layers._same_padding(W, k, stride))
            M, K, _, _ = ops.mx_im2col_dims((B, C, H, W), (k, k), (stride, stride), padding)
            with torch.no_grad():
                call_mx = conv_calls(lq, mx, mx.mx_operand(), mx.nested_q_b_layer(mx.b).detach(), "mx")
                call_i8 = conv_calls(lq, i8, i8.i8_operand(), i8.nested_q_b_layer(i8.b).detach(), "i8")
            lib, sp, fa = _hip.load(), _hip.stream_ptr(dev), ops.ELEMENT_FORMATS[ACT_FORMAT].id
            bufs = [ops._mx_operand_buffers(ACT_FORMAT, M, K, dev) for _ in range(args.sets)]
            geoms = [ops._conv_geom(x.shape, x.stride(), (k, k), (stride, stride), padding) for x in xs]
            keep += [mx, i8, bufs, geoms]

            def im2col(i, _hip=_hip, lib=lib, sp=sp, fa=fa, bufs=bufs, geoms=geoms):
                _hip.check(lib.lq_mx_operand_im2col(_hip.ptr(xs[i]), ctypes.byref(geoms[i]), fa, 0, _hip.ptr(bufs[i][0]),
                                                    _hip.ptr(bufs[i][1]), sp), "lq_mx_operand_im2col")
                return bufs[i]

            variants[f"{side}:im2col"] = im2col
            variants[f"{side}:mx_nchw"] = lambda i, f=call_mx: f(xs[i], ACT_FORMAT, ACT_SCALE)
            variants[f"{side}:mx_nhwc"] = lambda i, f=call_mx: f(xl[i], ACT_FORMAT, ACT_SCALE)
            for b in I8_BLOCKS:
                variants[f"{side}:i8_b{b}"] = lambda i, f=call_i8, b=b: f(xs[i], b)
        columns = [n.split(":", 1)[1] for n in variants if n.startswith("new:")]
        with torch.no_grad():
            for col in columns:                            # the two sides agree bit for bit: checked once, outside the clock
                a, b = variants[f"parent:{col}"](0), variants[f"new:{col}"](0)
                a, b = (a, b) if isinstance(a, tuple) else ((a.contiguous().view(torch.int32),), (b.contiguous().view(torch.int32),))
                if not all(torch.equal(p, q) for p, q in zip(a, b)):
                    raise SystemExit(f"{name}: {col} of this build differs from the parent's")
            for i in range(args.sets):                     # every variant warmed on every buffer set
                for fn in variants.values():
                    fn(i)
            us = {n: [] for n in variants}
            for _ in range(args.repeats):
                for n, t in timed(variants, args.sets, args.rounds, args.inner, dev).items():
                    us[n].append(statistics.median(t))
        for col in columns:
            p, n = us[f"parent:{col}"], us[f"new:{col}"]
            ok = statistics.median(n) <= max(p)
            bad += 0 if ok else 1
            lines.append(json.dumps({"shape": name, "variant": col, "rounds": args.rounds, "inner": args.inner, "repeats": args.repeats,
                                     "parent_us": [round(v, 2) for v in p], "new_us": [round(v, 2) for v in n],
                                     "parent_range_us": [round(min(p), 2), round(max(p), 2)], "new_median_us": round(statistics.median(n), 2),
                                     "new_inside_or_below_parent_range": ok}))
            print(lines[-1], flush=True)
        del xs, xl, variants, keep
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
