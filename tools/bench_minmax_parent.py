#!/usr/bin/env python3
"""lq_scale_init_group_minmax of a library built from the parent commit against this build's, interleaved in ONE process
(profiles/group_unify/bench.jsonl).

    python tools/bench_minmax_parent.py --parent-lib PARENT/liblq_hip.so [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--out FILE]

The protocol is tools/bench_group_affine.py's: raw C-ABI calls on rotating buffer sets; every round times each variant once (an
event-timed run of ``--inner`` back-to-back calls), the rounds interleave the variants, the figure is the median over the rounds in
microseconds; the whole comparison is repeated ``--repeats`` times.  Both libraries are loaded next to each other and bound with this
build's prototypes.  The tensors are that tool's two (float4 forms) and the same two with a width that is no multiple of 4 (scalar
forms), at ``gs`` = 32 and 128.  absmax is called in both libraries as well: its kernels are the same code in both, so its ratio shows
what the method resolves.

Output: one JSON line per tensor, group size and repeat (``us_<call>_<library>``), then one summary line per tensor, group size and
call: the parent's three medians, this build's, ``parent_spread_max_over_min`` (max / min of the parent's medians -- the only margin),
``ratio_this_over_parent`` (median of this build's medians over the median of the parent's) and ``inside_parent_spread`` (ratio <=
spread).  Exit status 1 if a min-max row is outside."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from learned_quantization_amd import _hip, ops  # noqa: E402

CASES = [("dense_4608x512", 4608, 512, 0), ("conv_512x4608", 512, 4608, 1), ("dense_4608x510_scalar", 4608, 510, 0),
         ("conv_512x4606_scalar", 512, 4606, 1)]


def bind(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("lq_scale_init_group", "lq_scale_init_group_minmax"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _hip.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="liblq_hip.so of the parent commit")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--group-sizes", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--out", default=None, help="write the JSON lines to this file as well")
    args = ap.parse_args()
    libs = {"parent": bind(args.parent_lib), "this": bind(_hip.LIB_PATH)}
    dev = torch.device("cuda:0")
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr
    qmin, qmax = ops.q_range_of(4)
    mv = float(ops.SCALE_INIT)
    rows = []
    for repeat in range(args.repeats):
        for gs in args.group_sizes:
            for name, R, C, axis in CASES:
                g = torch.Generator(device=dev).manual_seed(42 + repeat)
                nb = -(-(R if axis == 0 else C) // gs)
                shape = (nb, C) if axis == 0 else (R, nb)
                sets = [torch.empty((R, C), device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7) for _ in range(args.sets)]
                s_out, b_out = torch.empty(shape, device=dev), torch.empty(shape, device=dev)

                def absmax(lib):
                    return lambda P: lib.lq_scale_init_group(ptr(P), ptr(s_out), qmin, qmax, 0, 0, mv, R, C, axis, gs, sp)

                def minmax(lib):
                    return lambda P: lib.lq_scale_init_group_minmax(ptr(P), ptr(s_out), ptr(b_out), qmin, qmax, 0, mv, R, C, axis, gs, sp)

                variants = {f"{call}_{which}": make(lib) for call, make in (("absmax", absmax), ("minmax", minmax))
                            for which, lib in libs.items()}
                times = {k: [] for k in variants}
                k_set = 0
                for key, fn in variants.items():
                    for P in sets:
                        if fn(P) != 0:
                            raise RuntimeError(f"{key} failed")
                torch.cuda.synchronize(dev)
                for _ in range(args.rounds):
                    for key, fn in variants.items():
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(args.inner):
                            fn(sets[k_set % len(sets)])
                            k_set += 1
                        e.record()
                        torch.cuda.synchronize(dev)
                        times[key].append(a.elapsed_time(e) / args.inner * 1e3)
                row = {"tensor": name, "R": R, "C": C, "axis": axis, "group_size": gs, "repeat": repeat, "rounds": args.rounds,
                       "inner": args.inner, "buffer_sets": args.sets}
                row.update({f"us_{k}": statistics.median(v) for k, v in times.items()})
                rows.append(row)
                print(json.dumps(row), flush=True)
    summary, outside = [], 0
    for name, _, _, _ in CASES:
        for gs in args.group_sizes:
            for call in ("minmax", "absmax"):
                a = [r[f"us_{call}_parent"] for r in rows if r["tensor"] == name and r["group_size"] == gs]
                b = [r[f"us_{call}_this"] for r in rows if r["tensor"] == name and r["group_size"] == gs]
                spread, ratio = max(a) / min(a), statistics.median(b) / statistics.median(a)
                summary.append({"summary": call, "tensor": name, "group_size": gs, "parent_us_medians": a, "this_us_medians": b,
                                "parent_spread_max_over_min": spread, "ratio_this_over_parent": ratio,
                                "inside_parent_spread": bool(ratio <= spread)})
                outside += int(call == "minmax" and ratio > spread)
                print(json.dumps(summary[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows + summary) + "\n")
    return 1 if outside else 0


if __name__ == "__main__":
    sys.exit(main())
