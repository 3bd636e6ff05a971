#!/usr/bin/env python3
"""Quantization statistics (lq_group_stats, with and without the histogram) next to its yardstick, lq_fq_backward_group on the
same buffers, interleaved in one process.  The protocol is tools/bench_group_batch.py's.

Two workloads:

  * ``matrix_4224x2048``: one matrix, groups along axis 0, ``gs = 128`` (scale (33, 2048)), 8.65 M elements;
  * ``imagenette``: every quantised tensor of the ResNet-18-like net with group-wise scales of 128 (biases: one scalar scale
    each, through the group entry points as R = 1, axis 1, gs = numel), one call per tensor.

The statistics read 4 bytes per element and write a few numbers per group; the backward reads 8 and writes 4.  Raw C-ABI calls
on rotating buffer sets (``--sets`` copies of P, dy and dP, so that a call does not find its input in the cache its predecessor
left); every round times each variant once (event-timed run of ``--inner`` back-to-back passes over the workload), the rounds
interleave the variants, the figure is the median over the rounds in microseconds per pass.  The whole comparison is repeated
``--repeats`` times so that the yardstick's own run-to-run spread is visible.  One JSON line per workload and repeat.

    python tools/bench_group_stats.py [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--asymmetric] [--out FILE]
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


def weight_set(config, bits, gs, dev):
    """[(R, C, axis, gs), scale shape, q_range] of every quantised tensor of the model."""
    lq.reset_layer_names()
    model = lq.build_model(config, mode="ste", value=0.0, seed=1, device=dev, bits=bits, group_size=gs)
    return [(init_geometry(tuple(p.shape), p.data.stride(), tuple(nested.scale.shape), nested.group_size), tuple(nested.scale.shape),
             nested.q_range) for _, p, nested in lq.quantized_tensors(model)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--asymmetric", action="store_true", help="an offset per group: the affine backward against the statistics with b")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr
    qr = lq.q_range_of(args.bits)
    workloads = {"matrix_4224x2048": [((4224, 2048, 0, args.group_size), (-(-4224 // args.group_size), 2048), qr)],
                 "imagenette": weight_set("imagenette", args.bits, args.group_size, dev)}
    lines = []
    for repeat in range(args.repeats):
        for name, specs in workloads.items():
            g = torch.Generator(device=dev).manual_seed(42 + repeat)
            tensors = []
            for (R, C, axis, gs), sshape, (qmin, qmax) in specs:
                s = torch.exp2(torch.empty(sshape, device=dev).uniform_(-9.0, -5.0, generator=g))
                b = torch.empty_like(s).uniform_(-6.0, 6.0, generator=g) * s if args.asymmetric else None
                tensors.append(dict(geom=(R, C, axis, gs), qmin=qmin, qmax=qmax, s=s, b=b, ds=torch.empty_like(s), db=torch.empty_like(s),
                                    cl=torch.empty_like(s, dtype=torch.int32), below=torch.empty_like(s, dtype=torch.int32),
                                    above=torch.empty_like(s, dtype=torch.int32), err2=torch.empty_like(s, dtype=torch.float64),
                                    sig2=torch.empty_like(s, dtype=torch.float64),
                                    hist=torch.zeros(qmax - qmin + 1, dtype=torch.int32, device=dev)))
            sets = []
            for _ in range(args.sets):
                bufs = []
                for t in tensors:
                    R, C, _, _ = t["geom"]
                    P = torch.empty(R * C, device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7)
                    bufs.append((P, torch.empty_like(P).normal_(generator=g), torch.empty_like(P)))
                sets.append(bufs)

            def backward(k):
                for t, (P, dy, dP) in zip(tensors, sets[k]):
                    R, C, axis, gs = t["geom"]
                    if args.asymmetric:
                        rc = lib.lq_fq_backward_group_affine(ptr(P), ptr(t["s"]), ptr(t["b"]), ptr(dy), t["qmin"], t["qmax"], 0, 1.0, 1.0,
                                                             ptr(dP), ptr(t["ds"]), ptr(t["db"]), ptr(t["cl"]), None, 0, R, C, axis, gs, sp)
                    else:
                        rc = lib.lq_fq_backward_group(ptr(P), ptr(t["s"]), ptr(dy), t["qmin"], t["qmax"], 0, 1.0, ptr(dP), ptr(t["ds"]),
                                                      ptr(t["cl"]), None, 0, R, C, axis, gs, sp)
                    _hip.check(rc, "backward_group")

            def stats(with_hist):
                def run(k):
                    for t, (P, _, _) in zip(tensors, sets[k]):
                        R, C, axis, gs = t["geom"]
                        _hip.check(lib.lq_group_stats(ptr(P), ptr(t["s"]), ptr(t["b"]), t["qmin"], t["qmax"], 0, ptr(t["below"]),
                                                      ptr(t["above"]), ptr(t["err2"]), ptr(t["sig2"]), ptr(t["hist"]) if with_hist else None,
                                                      R, C, axis, gs, sp), "group_stats")
                return run

            variants = {"backward_group": backward, "group_stats": stats(True), "group_stats_no_hist": stats(False)}
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
                   "group_size": args.group_size, "q_range": list(qr), "asymmetric": bool(args.asymmetric), "repeat": repeat,
                   "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets}
            for key in variants:
                row[f"us_{key}"] = statistics.median(times[key])
                row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
            row["stats_over_backward"] = row["us_group_stats"] / row["us_backward_group"]
            row["stats_no_hist_over_backward"] = row["us_group_stats_no_hist"] / row["us_backward_group"]
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
