#!/usr/bin/env python3
"""Scale initialisation (lq_scale_init_group, all three methods) next to its yardstick, lq_fq_forward_group on the same tensors,
interleaved in one process.  The protocol is tools/bench_groupwise.py's.

Three tensors:

  * ``dense_4608x512``: W (in, out) = 4608 x 512 contiguous, groups along axis 0, ``gs = 128`` (scale (36, 512));
  * ``conv_512x4608``: a 3 x 3 x 512 x 512 kernel stored OIHW = 512 rows of 4608, groups along axis 1, ``gs = 128`` (scale (512, 36));
  * ``scalar_2359296``: the same 2.36 M elements under ONE scale (R = 1, axis 1, gs = C): a single team of 64 lanes walks the whole
    tensor, the worst case of the row form.

absmax and lsq read 4 bytes per element in one pass; the forward reads 4 and writes 4.  mse walks each group twice (the column form
five times: the absmax pass and four chunks of candidates) and divides 28 times per element.  Raw C-ABI calls on rotating buffer
sets; every round times each variant once (event-timed run of ``--inner`` back-to-back calls; the scalar tensor's mse, tens of
milliseconds per call, runs ``--inner-slow``), the rounds interleave the variants, the figure is the median over the rounds in
microseconds.  The whole comparison is repeated ``--repeats`` times so that the yardstick's own run-to-run spread is visible.
One JSON line per tensor and repeat.

    python tools/bench_scale_init.py [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--out FILE]
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
    ap.add_argument("--inner-slow", type=int, default=2)
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
    n = 4608 * 512
    # (name, R, C, axis, gs)
    cases = [("dense_4608x512", 4608, 512, 0, args.group_size), ("conv_512x4608", 512, 4608, 1, args.group_size),
             (f"scalar_{n}", 1, n, 1, n)]
    lines = []
    for repeat in range(args.repeats):
        for name, R, C, axis, gs in cases:
            g = torch.Generator(device=dev).manual_seed(42 + repeat)
            nb = -(-(R if axis == 0 else C) // gs)
            shape = (nb, C) if axis == 0 else (R, nb)
            sets = []
            for _ in range(args.sets):
                P = torch.empty((R, C), device=dev).normal_(generator=g) * 0.05
                sets.append((P, torch.empty_like(P), torch.empty(shape, device=dev)))
            s_fwd = torch.empty(shape, device=dev)
            _hip.check(lib.lq_scale_init_group(ptr(sets[0][0]), ptr(s_fwd), qmin, qmax, 0, 0, ops.SCALE_INIT, R, C, axis, gs, sp), "init")

            def forward(P, out, s):
                _hip.check(lib.lq_fq_forward_group(ptr(P), ptr(s_fwd), ptr(out), None, _hip.LQ_Q_NONE, qmin, qmax, 0, R, C, axis, gs, sp),
                           "forward_group")

            def init(method):
                def run(P, out, s):
                    _hip.check(lib.lq_scale_init_group(ptr(P), ptr(s), qmin, qmax, 0, method, ops.SCALE_INIT, R, C, axis, gs, sp),
                               "scale_init_group")
                return run

            variants = {"forward_group": forward, "absmax": init(0), "lsq": init(1), "mse": init(2)}
            inner = {k: (args.inner_slow if (k == "mse" and nb * (C if axis == 0 else R) == 1) else args.inner) for k in variants}
            times = {k: [] for k in variants}
            k_set = 0
            for fn in variants.values():
                fn(*sets[0])
            torch.cuda.synchronize(dev)
            for _ in range(args.rounds):
                for key, fn in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(inner[key]):
                        fn(*sets[k_set % len(sets)])
                        k_set += 1
                    b.record()
                    torch.cuda.synchronize(dev)
                    times[key].append(a.elapsed_time(b) / inner[key] * 1e3)
            row = {"tensor": name, "R": R, "C": C, "axis": axis, "group_size": gs, "groups": nb * (C if axis == 0 else R),
                   "q_range": [qmin, qmax], "repeat": repeat, "rounds": args.rounds, "inner": inner, "buffer_sets": args.sets}
            for key in variants:
                row[f"us_{key}"] = statistics.median(times[key])
                row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
            for key in ("absmax", "lsq", "mse"):
                row[f"{key}_over_forward"] = row[f"us_{key}"] / row["us_forward_group"]
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
