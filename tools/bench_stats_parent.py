#!/usr/bin/env python3
"""The statistics entry points (lq_group_stats, lq_mx_stats) of this build next to the parent commit's, timed on the same buffers
in one process (profiles/stats_unify/bench.jsonl).

    python3 tools/bench_stats_parent.py --parent-lib PARENT/liblq_hip.so [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--out FILE]

``--parent-lib`` names a liblq_hip.so built from the parent commit; it is loaded next to this build's (as
tools/bench_group_affine.py does) and both are bound with this build's prototypes.  Workloads and protocol are those of
tools/bench_group_stats.py (4 bits, gs = 128, without and with an offset) and tools/bench_mx_stats.py (fp4_e2m1 under E8M0,
gs = 32): the 4224 x 2048 matrix along axis 0 and every quantised tensor of the imagenette net, raw C-ABI calls on rotating
buffer sets, every round times each variant once over ``--inner`` back-to-back passes, each variant's place in the round rotates,
the figure is the median over the rounds in microseconds per pass, the whole comparison is repeated ``--repeats`` times.

The yardstick is the parent measured against itself: it runs twice in every round (parent_a, parent_b).  Per family, workload
and histogram choice the summary line holds

  spread   (max - min) / min over the parent's 2 x repeats medians
  ratio    median of this build's medians / median of the parent's medians

and the exit status is 1 where a ratio exceeds 1 + spread.  One JSON line per family, workload and repeat, then the summary lines.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import _hip, ops  # noqa: E402
import bench_group_stats  # noqa: E402
import bench_mx_stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="write the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr

    def bind(path):
        lib = ctypes.CDLL(os.path.abspath(path))
        for name in ("lq_group_stats", "lq_mx_stats", "lq_last_error"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _hip.SIGNATURES[name]
        return lib

    parent, this = bind(args.parent_lib), bind(_hip.LIB_PATH)
    fmt, sf = ops.check_element_format("fp4_e2m1"), ops.check_scale_format("e8m0")
    qmin, qmax = lq.q_range_of(4)
    int_specs = {"matrix_4224x2048": [((4224, 2048, 0, 128), (33, 2048))],
                 "imagenette": [(geom, sshape) for geom, sshape, _ in bench_group_stats.weight_set("imagenette", 4, 128, dev)]}
    mx_specs = {"matrix_4224x2048": [((4224, 2048, 0, 32), (132, 2048))],
                "imagenette": bench_mx_stats.weight_set("imagenette", "fp4_e2m1", 32, dev)}

    def call(lib, family, t, P, with_hist):
        R, C, axis, gs = t["geom"]
        if family == "mx":
            return lib.lq_mx_stats(ptr(P), ptr(t["s"]), fmt.id, sf, ptr(t["below"]), ptr(t["above"]), ptr(t["flushed"]), ptr(t["err2"]),
                                   ptr(t["sig2"]), ptr(t["hist_mx"]) if with_hist else None, R, C, axis, gs, sp)
        return lib.lq_group_stats(ptr(P), ptr(t["s"]), ptr(t["b"]) if family == "group_affine" else None, qmin, qmax, 0, ptr(t["below"]),
                                  ptr(t["above"]), ptr(t["err2"]), ptr(t["sig2"]), ptr(t["hist"]) if with_hist else None, R, C, axis, gs, sp)

    lines, medians = [], {}
    for repeat in range(args.repeats):
        for family, workloads in (("group", int_specs), ("group_affine", int_specs), ("mx", mx_specs)):
            for name, specs in workloads.items():
                g = torch.Generator(device=dev).manual_seed(42 + repeat)
                tensors = []
                for geom, sshape in specs:
                    s = torch.exp2(torch.empty(sshape, device=dev).uniform_(-9.0, -5.0, generator=g))
                    i32 = lambda: torch.empty_like(s, dtype=torch.int32)      # noqa: E731
                    f64 = lambda: torch.empty_like(s, dtype=torch.float64)    # noqa: E731
                    tensors.append(dict(geom=geom, s=s, b=torch.empty_like(s).uniform_(-6.0, 6.0, generator=g) * s, below=i32(), above=i32(),
                                        flushed=i32(), err2=f64(), sig2=f64(), hist=torch.zeros(qmax - qmin + 1, dtype=torch.int32, device=dev),
                                        hist_mx=torch.zeros(1 << fmt.bits, dtype=torch.int32, device=dev)))
                sets = [[torch.empty(t["geom"][0] * t["geom"][1], device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7) for t in tensors]
                        for _ in range(args.sets)]

                def variant(lib, with_hist):
                    def run(k):
                        for t, P in zip(tensors, sets[k]):
                            rc = call(lib, family, t, P, with_hist)
                            if rc != 0:
                                raise RuntimeError(f"{family} statistics returned {rc}: {lib.lq_last_error().decode()}")
                    return run

                variants = {(who, h): variant(lib, h == "hist") for h in ("hist", "no_hist")
                            for who, lib in (("parent_a", parent), ("this", this), ("parent_b", parent))}
                keys = list(variants)
                times = {k: [] for k in keys}
                k_set = 0
                for fn in variants.values():          # warm-up: every kernel of every shape once
                    fn(0)
                torch.cuda.synchronize(dev)
                for rnd in range(args.rounds):
                    for key in keys[rnd % len(keys):] + keys[:rnd % len(keys)]:      # each variant's place in the round rotates
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(args.inner):
                            variants[key](k_set % len(sets))
                            k_set += 1
                        b.record()
                        torch.cuda.synchronize(dev)
                        times[key].append(a.elapsed_time(b) / args.inner * 1e3)
                row = {"family": family, "workload": name, "tensors": len(tensors),
                       "elements": sum(t["geom"][0] * t["geom"][1] for t in tensors), "repeat": repeat, "rounds": args.rounds,
                       "inner": args.inner, "buffer_sets": args.sets}
                for who, h in keys:
                    row[f"us_{who}_{h}"] = statistics.median(times[who, h])
                    row[f"us_{who}_{h}_min_max"] = [min(times[who, h]), max(times[who, h])]
                    medians.setdefault((family, name, h), {}).setdefault(who[:6], []).append(row[f"us_{who}_{h}"])      # "parent" / "this"
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
                del sets
    slower = 0
    for (family, name, h), m in medians.items():
        spread = (max(m["parent"]) - min(m["parent"])) / min(m["parent"])
        ratio = statistics.median(m["this"]) / statistics.median(m["parent"])
        slower += ratio > 1.0 + spread
        lines.append(json.dumps({"summary": family, "workload": name, "histogram": h == "hist", "us_parent": statistics.median(m["parent"]),
                                 "us_this": statistics.median(m["this"]), "ratio": ratio, "parent_spread": spread,
                                 "within_spread": bool(ratio <= 1.0 + spread)}))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
