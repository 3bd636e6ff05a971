#!/usr/bin/env python3
"""Microscaling statistics (lq_mx_stats, with and without the histogram) next to their yardsticks on the same buffers, interleaved
in one process: (a) lq_fq_backward_mx, (b) lq_group_stats with [-8, 7], nearest.  lq_fq_forward_mx and lq_fq_forward_group run in
the same rounds, so that the session's own cost of the minifloat element step over the integer one (forward_mx / forward_group)
stands next to mx_stats / group_stats.  The protocol is tools/bench_group_stats.py's, with one addition: each variant's place in
the round rotates from round to round (an order effect of up to x1.2 is on record for the MX batch when it does not).

Two workloads, ``gs = 32`` (the MX block):

  * ``matrix_4224x2048``: one matrix, groups along axis 0 (scale (132, 2048)), 8.65 M elements;
  * ``imagenette``: every quantised tensor of the ResNet-18-like net (biases: one scalar scale each, R = 1, axis 1, gs = numel),
    one call per tensor.

Raw C-ABI calls on rotating buffer sets (``--sets`` copies of P, dy and the element-sized output); every round times each variant
once (event-timed run of ``--inner`` back-to-back passes over the workload); the figure is the median over the rounds in
microseconds per pass.  The whole comparison is repeated ``--repeats`` times so that the yardsticks' own run-to-run spread is
visible.  One JSON line per workload and repeat.

    python tools/bench_mx_stats.py [--element-format fp4_e2m1] [--scale-format e8m0] [--rounds 15] [--inner 10] [--sets 4]
                                   [--repeats 3] [--out FILE]
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
from learned_quantization_amd import _hip, ops  # noqa: E402
from learned_quantization_amd.descriptor import init_geometry  # noqa: E402


def weight_set(config, element_format, gs, dev):
    """[(R, C, axis, gs), scale shape] of every quantised tensor of the model."""
    lq.reset_layer_names()
    model = lq.build_model(config, mode="ste", value=0.0, seed=1, device=dev, element_format=element_format, group_size=gs)
    return [(init_geometry(tuple(p.shape), p.data.stride(), tuple(nested.scale.shape), nested.group_size), tuple(nested.scale.shape))
            for _, p, nested in lq.quantized_tensors(model)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--element-format", default="fp4_e2m1", choices=list(ops.ELEMENT_FORMATS))
    ap.add_argument("--scale-format", default="e8m0", choices=list(ops.SCALE_FORMATS))
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
    fmt = ops.check_element_format(args.element_format)
    sf = ops.check_scale_format(args.scale_format)
    gsz = args.group_size
    workloads = {"matrix_4224x2048": [((4224, 2048, 0, gsz), (-(-4224 // gsz), 2048))],
                 "imagenette": weight_set("imagenette", args.element_format, gsz, dev)}
    lines = []
    for repeat in range(args.repeats):
        for name, specs in workloads.items():
            g = torch.Generator(device=dev).manual_seed(42 + repeat)
            tensors = []
            for geom, sshape in specs:
                s = torch.exp2(torch.empty(sshape, device=dev).uniform_(-9.0, -5.0, generator=g))
                i32 = lambda: torch.empty_like(s, dtype=torch.int32)      # noqa: E731
                f64 = lambda: torch.empty_like(s, dtype=torch.float64)    # noqa: E731
                tensors.append(dict(geom=geom, s=s, ds=torch.empty_like(s), cl=i32(), below=i32(), above=i32(), flushed=i32(), err2=f64(),
                                    sig2=f64(), hist=torch.zeros(1 << fmt.bits, dtype=torch.int32, device=dev),
                                    hist16=torch.zeros(16, dtype=torch.int32, device=dev)))
            sets = []
            for _ in range(args.sets):
                bufs = []
                for t in tensors:
                    R, C, _, _ = t["geom"]
                    P = torch.empty(R * C, device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7)
                    bufs.append((P, torch.empty_like(P).normal_(generator=g), torch.empty_like(P)))
                sets.append(bufs)

            def each(call, what):
                def run(k):
                    for t, (P, dy, o) in zip(tensors, sets[k]):
                        _hip.check(call(t, P, dy, o, *t["geom"]), what)
                return run

            variants = {
                "backward_mx": each(lambda t, P, dy, o, R, C, axis, gs: lib.lq_fq_backward_mx(
                    ptr(P), ptr(t["s"]), ptr(dy), fmt.id, sf, 1.0, ptr(o), ptr(t["ds"]), ptr(t["cl"]), R, C, axis, gs, sp), "backward_mx"),
                "mx_stats": each(lambda t, P, dy, o, R, C, axis, gs: lib.lq_mx_stats(
                    ptr(P), ptr(t["s"]), fmt.id, sf, ptr(t["below"]), ptr(t["above"]), ptr(t["flushed"]), ptr(t["err2"]), ptr(t["sig2"]),
                    ptr(t["hist"]), R, C, axis, gs, sp), "mx_stats"),
                "mx_stats_no_hist": each(lambda t, P, dy, o, R, C, axis, gs: lib.lq_mx_stats(
                    ptr(P), ptr(t["s"]), fmt.id, sf, ptr(t["below"]), ptr(t["above"]), ptr(t["flushed"]), ptr(t["err2"]), ptr(t["sig2"]),
                    None, R, C, axis, gs, sp), "mx_stats"),
                "group_stats": each(lambda t, P, dy, o, R, C, axis, gs: lib.lq_group_stats(
                    ptr(P), ptr(t["s"]), None, -8, 7, 1, ptr(t["below"]), ptr(t["above"]), ptr(t["err2"]), ptr(t["sig2"]), ptr(t["hist16"]),
                    R, C, axis, gs, sp), "group_stats"),
                "forward_mx": each(lambda t, P, dy, o, R, C, axis, gs: lib.lq_fq_forward_mx(
                    ptr(P), ptr(t["s"]), ptr(o), None, 0, fmt.id, sf, R, C, axis, gs, sp), "forward_mx"),
                "forward_group": each(lambda t, P, dy, o, R, C, axis, gs: lib.lq_fq_forward_group(
                    ptr(P), ptr(t["s"]), ptr(o), None, 0, -8, 7, 1, R, C, axis, gs, sp), "forward_group"),
            }
            keys = list(variants)
            times = {k: [] for k in keys}
            k_set = 0
            for fn in variants.values():          # warm-up: every kernel of every shape once
                fn(0)
            torch.cuda.synchronize(dev)
            for rnd in range(args.rounds):
                order = keys[rnd % len(keys):] + keys[:rnd % len(keys)]      # each variant's place in the round rotates
                for key in order:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.inner):
                        variants[key](k_set % len(sets))
                        k_set += 1
                    b.record()
                    torch.cuda.synchronize(dev)
                    times[key].append(a.elapsed_time(b) / args.inner * 1e3)
            row = {"workload": name, "tensors": len(tensors), "elements": sum(t["geom"][0] * t["geom"][1] for t in tensors),
                   "group_size": gsz, "element_format": args.element_format, "scale_format": args.scale_format, "repeat": repeat,
                   "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets}
            for key in keys:
                row[f"us_{key}"] = statistics.median(times[key])
                row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
            row["mx_stats_over_backward_mx"] = row["us_mx_stats"] / row["us_backward_mx"]
            row["mx_stats_no_hist_over_backward_mx"] = row["us_mx_stats_no_hist"] / row["us_backward_mx"]
            row["mx_stats_over_group_stats"] = row["us_mx_stats"] / row["us_group_stats"]
            row["forward_mx_over_forward_group"] = row["us_forward_mx"] / row["us_forward_group"]
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            del sets
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
