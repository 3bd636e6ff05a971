#!/usr/bin/env python3
"""The group-wise clipped pair next to its yardstick, the shipped per-channel clipped pair, interleaved in one process.

Two tensors, the largest of tests/test_gpu_groupwise.py in both orientations, ``gs = 128``:

  * ``dense_4608x512``: W (in, out) = 4608 x 512 contiguous; group-wise axis 0 (scale (36, 512)) against column-wise (1, 512);
  * ``conv_512x4608``: a 3 x 3 x 512 x 512 kernel stored OIHW = 512 rows of 4608; group-wise axis 1 (scale (512, 36)) against
    row-wise (512, 1).

Both move the same 8 (forward) + 12 (backward) bytes per element.  Raw C-ABI calls into preallocated outputs on rotating buffer
sets; every round times each variant once (event-timed run of ``--inner`` back-to-back calls), the rounds interleave the variants,
the figure is the median over the rounds in microseconds.  The whole comparison is repeated ``--repeats`` times so that the
yardstick's own run-to-run spread is visible.  One JSON line per tensor and repeat.

    python tools/bench_groupwise.py [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learned_quantization_amd import _hip, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr
    qmin, qmax = ops.q_range_of(args.bits)
    gs = args.group_size
    # (name, R, C, axis of the groups, one-axis descriptor (outer, G, inner) of the yardstick)
    cases = [("dense_4608x512", 4608, 512, 0, (4608, 512, 1)), ("conv_512x4608", 512, 4608, 1, (1, 512, 4608))]
    lines = []
    for repeat in range(args.repeats):
        for name, R, C, axis, (outer, G, inner) in cases:
            g = torch.Generator(device=dev).manual_seed(42 + repeat)
            nb = -(-(R if axis == 0 else C) // gs)
            s_group = torch.exp2(torch.empty((nb, C) if axis == 0 else (R, nb), device=dev).uniform_(-9.0, -5.0, generator=g))
            s_axis = torch.exp2(torch.empty(G, device=dev).uniform_(-9.0, -5.0, generator=g))
            sets = []
            for _ in range(args.sets):
                P = torch.empty((R, C), device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7)
                dy = torch.empty((R, C), device=dev).normal_(generator=g)
                sets.append((P, dy, torch.empty_like(P)))
            ds_g, cl_g = torch.empty_like(s_group), torch.empty_like(s_group, dtype=torch.int32)
            ds_a, cl_a = torch.empty_like(s_axis), torch.empty_like(s_axis, dtype=torch.int32)
            ws = _hip.workspace_for(dev, outer, G, inner)
            need = lib.lq_group_workspace_bytes(R, C, axis, gs)
            ws_g = _hip.workspace(dev, need) if need else None

            def fwd_axis(P, dy, out):
                _hip.check(lib.lq_fq_forward_clip_r(ptr(P), ptr(s_axis), ptr(out), None, _hip.LQ_Q_NONE, qmin, qmax, 0, outer, G, inner, sp),
                           "forward_clip_r")

            def fwd_group(P, dy, out):
                _hip.check(lib.lq_fq_forward_group(ptr(P), ptr(s_group), ptr(out), None, _hip.LQ_Q_NONE, qmin, qmax, 0, R, C, axis, gs, sp),
                           "forward_group")

            def bwd_axis(P, dy, out):
                _hip.check(lib.lq_fq_backward_clip_r(ptr(P), ptr(s_axis), ptr(dy), qmin, qmax, 0, 1.0, ptr(out), ptr(ds_a), ptr(cl_a),
                                                     ptr(ws), ws.numel(), outer, G, inner, sp), "backward_clip_r")

            def bwd_group(P, dy, out):
                _hip.check(lib.lq_fq_backward_group(ptr(P), ptr(s_group), ptr(dy), qmin, qmax, 0, 1.0, ptr(out), ptr(ds_g), ptr(cl_g),
                                                    ptr(ws_g), need, R, C, axis, gs, sp), "backward_group")

            variants = {"forward_per_channel": fwd_axis, "forward_group": fwd_group, "backward_per_channel": bwd_axis,
                        "backward_group": bwd_group}
            times = {k: [] for k in variants}
            k_set = 0
            for fn in variants.values():
                for P, dy, out in sets:
                    fn(P, dy, out)
            torch.cuda.synchronize(dev)
            for _ in range(args.rounds):
                for key, fn in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.inner):
                        fn(*sets[k_set % len(sets)])
                        k_set += 1
                    b.record()
                    torch.cuda.synchronize(dev)
                    times[key].append(a.elapsed_time(b) / args.inner * 1e3)
            row = {"tensor": name, "R": R, "C": C, "axis": axis, "group_size": gs, "yardstick_descriptor": [outer, G, inner],
                   "q_range": [qmin, qmax], "repeat": repeat, "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets}
            for key in variants:
                row[f"us_{key}"] = statistics.median(times[key])
                row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
            row["forward_group_over_per_channel"] = row["us_forward_group"] / row["us_forward_per_channel"]
            row["backward_group_over_per_channel"] = row["us_backward_group"] / row["us_backward_per_channel"]
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
