#!/usr/bin/env python3
"""The microscaling pair (lq_fq_forward_mx / lq_fq_backward_mx) next to its yardstick, the integer group-wise pair
(lq_fq_forward_group / lq_fq_backward_group, [-8, 7], nearest) on the same buffers, interleaved in one process.  The protocol is
tools/bench_group_stats.py's.

Two workloads, group size 32 (the MX block):

  * ``matrix_4224x2048``: one matrix, groups along axis 0 (scale (132, 2048)), 8.65 M elements;
  * ``imagenette``: every quantised tensor of the ResNet-18-like net (biases: one scalar scale each, through the group entry
    points as R = 1, axis 1, gs = numel), one call per tensor.

Both pairs move the same bytes (forward: read 4, write 4 per element; backward: read 8, write 4); the MX pair adds a few integer
and VALU operations per element.  Raw C-ABI calls on rotating buffer sets (``--sets`` copies of P, dy, out and dP); every round
times each variant once (event-timed run of ``--inner`` back-to-back passes over the workload), the rounds interleave the
variants, the figure is the median over the rounds in microseconds per pass.  The whole comparison is repeated ``--repeats`` times:
the integer pair's own max / min over the repeats is the noise the ratios are read against.  One JSON line per workload and
repeat, and one summary line per workload.

    python tools/bench_mx.py [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--out FILE]
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
from learned_quantization_amd import _hip  # noqa: E402
from learned_quantization_amd.descriptor import init_geometry  # noqa: E402

MX_VARIANTS = {"fp4_e2m1_e8m0": (0, 0), "fp8_e4m3_fp32": (3, 1)}      # (lq_elem_format, lq_scale_format)


def weight_set(config, gs, dev):
    """[(R, C, axis, gs), scale shape] of every quantised tensor of the model."""
    lq.reset_layer_names()
    model = lq.build_model(config, mode="ste", value=0.0, seed=1, device=dev, bits=4, group_size=gs)
    return [(init_geometry(tuple(p.shape), p.data.stride(), tuple(nested.scale.shape), nested.group_size), tuple(nested.scale.shape))
            for _, p, nested in lq.quantized_tensors(model)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--group-size", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr
    gs = args.group_size
    workloads = {"matrix_4224x2048": [((4224, 2048, 0, gs), (-(-4224 // gs), 2048))], "imagenette": weight_set("imagenette", gs, dev)}
    lines, rows = [], {name: [] for name in workloads}
    for repeat in range(args.repeats):
        for name, specs in workloads.items():
            g = torch.Generator(device=dev).manual_seed(42 + repeat)
            tensors = []
            for geom, sshape in specs:
                s = torch.exp2(torch.empty(sshape, device=dev).uniform_(-9.0, -5.0, generator=g))
                tensors.append(dict(geom=geom, s=s, ds=torch.empty_like(s), cl=torch.empty_like(s, dtype=torch.int32)))
            sets = []
            for _ in range(args.sets):
                bufs = []
                for t in tensors:
                    R, C, _, _ = t["geom"]
                    P = torch.empty(R * C, device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7)
                    bufs.append((P, torch.empty_like(P).normal_(generator=g), torch.empty_like(P), torch.empty_like(P)))
                sets.append(bufs)

            def int_forward(k):
                for t, (P, _, out, _) in zip(tensors, sets[k]):
                    _hip.check(lib.lq_fq_forward_group(ptr(P), ptr(t["s"]), ptr(out), None, 0, -8, 7, 1, *t["geom"], sp), "forward_group")

            def int_backward(k):
                for t, (P, dy, _, dP) in zip(tensors, sets[k]):
                    _hip.check(lib.lq_fq_backward_group(ptr(P), ptr(t["s"]), ptr(dy), -8, 7, 1, 1.0, ptr(dP), ptr(t["ds"]), ptr(t["cl"]),
                                                        None, 0, *t["geom"], sp), "backward_group")

            def mx_forward(fmt, sf):
                def run(k):
                    for t, (P, _, out, _) in zip(tensors, sets[k]):
                        _hip.check(lib.lq_fq_forward_mx(ptr(P), ptr(t["s"]), ptr(out), None, 0, fmt, sf, *t["geom"], sp), "forward_mx")
                return run

            def mx_backward(fmt, sf):
                def run(k):
                    for t, (P, dy, _, dP) in zip(tensors, sets[k]):
                        _hip.check(lib.lq_fq_backward_mx(ptr(P), ptr(t["s"]), ptr(dy), fmt, sf, 1.0, ptr(dP), ptr(t["ds"]), ptr(t["cl"]),
                                                         *t["geom"], sp), "backward_mx")
                return run

            variants = {"forward_group": int_forward, "backward_group": int_backward}
            for key, (fmt, sf) in MX_VARIANTS.items():
                variants[f"forward_mx_{key}"] = mx_forward(fmt, sf)
                variants[f"backward_mx_{key}"] = mx_backward(fmt, sf)
            times = {k: [] for k in variants}
            k_set = 0
            for fn in variants.values():          # warm-up: every kernel of every shape once
                fn(0)
            torch.cuda.synchronize(dev)
            for _ in range(args.rounds):
                for key, fn in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.inner):
                        fn(k_set % len(sets))
                        k_set += 1
                    b.record()
                    torch.cuda.synchronize(dev)
                    times[key].append(a.elapsed_time(b) / args.inner * 1e3)
            row = {"workload": name, "tensors": len(tensors), "elements": sum(t["geom"][0] * t["geom"][1] for t in tensors),
                   "group_size": gs, "repeat": repeat, "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets}
            for key in variants:
                row[f"us_{key}"] = statistics.median(times[key])
                row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
            for key in MX_VARIANTS:
                row[f"forward_mx_{key}_over_group"] = row[f"us_forward_mx_{key}"] / row["us_forward_group"]
                row[f"backward_mx_{key}_over_group"] = row[f"us_backward_mx_{key}"] / row["us_backward_group"]
            rows[name].append(row)
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            del sets
    for name, rs in rows.items():      # the yardstick's own spread over the repeats next to the ratios
        summary = {"workload": name, "summary": True, "repeats": len(rs)}
        for d in ("forward", "backward"):
            base = [r[f"us_{d}_group"] for r in rs]
            summary[f"{d}_group_max_over_min"] = max(base) / min(base)
            for key in MX_VARIANTS:
                summary[f"{d}_mx_{key}_over_group"] = [r[f"{d}_mx_{key}_over_group"] for r in rs]
        line = json.dumps(summary)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
