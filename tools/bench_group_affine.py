#!/usr/bin/env python3
"""The asymmetric group-wise pair next to its yardstick, the symmetric group-wise pair, and min-max initialisation next to absmax,
interleaved in one process.

Two tensors, the largest of tests/test_gpu_groupwise.py in both orientations, at ``gs`` = 32 and 128:

  * ``dense_4608x512``: W (in, out) = 4608 x 512 contiguous, groups along axis 0 (scale and offset (nb, 512));
  * ``conv_512x4608``: a 3 x 3 x 512 x 512 kernel stored OIHW = 512 rows of 4608, groups along axis 1 (scale and offset (512, nb)).

The two pairs move the same 8 (forward) + 12 (backward) bytes per element; the affine pair reads the offset matrix on top and writes
db, a 1 / gs share each.  ``--parent-lib`` names a liblq_hip.so built from the parent commit: the symmetric pair and absmax are then
called in THAT library (loaded next to this one), so the yardstick is the parent's code, not this build's copy of it.  Raw C-ABI calls
into preallocated outputs on rotating buffer sets; every round times each variant once (event-timed run of ``--inner`` back-to-back
calls), the rounds interleave the variants, the figure is the median over the rounds in microseconds.  The whole comparison is repeated
``--repeats`` times so that the yardstick's own run-to-run spread is visible.  One JSON line per tensor, group size and repeat.

    python tools/bench_group_affine.py [--parent-lib FILE] [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--out FILE]
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

from learned_quantization_amd import _hip, ops  # noqa: E402
import _devlib  # noqa: E402,F401  (LQ_HIP_LIB: another build of this commit's ABI in place of the shipped library)


def _yardstick(path):
    """The symmetric entry points of another build of the same ABI, bound with this build's prototypes."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("lq_fq_forward_group", "lq_fq_backward_group", "lq_scale_init_group", "lq_last_error"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _hip.SIGNATURES[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblq_hip.so of the parent commit: the yardstick's calls go there")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--group-sizes", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    sym = _yardstick(args.parent_lib) if args.parent_lib else lib
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr
    qmin, qmax = ops.q_range_of(args.bits)
    mv = float(ops.SCALE_INIT)

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} returned {rc}")

    cases = [("dense_4608x512", 4608, 512, 0), ("conv_512x4608", 512, 4608, 1)]
    lines = []
    for repeat in range(args.repeats):
        for gs in args.group_sizes:
            for name, R, C, axis in cases:
                g = torch.Generator(device=dev).manual_seed(42 + repeat)
                nb = -(-(R if axis == 0 else C) // gs)
                shape = (nb, C) if axis == 0 else (R, nb)
                s = torch.exp2(torch.empty(shape, device=dev).uniform_(-9.0, -5.0, generator=g))
                b = torch.empty(shape, device=dev).uniform_(-6.0, 6.0, generator=g) * s
                sets = []
                for _ in range(args.sets):
                    P = torch.empty((R, C), device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7)
                    dy = torch.empty((R, C), device=dev).normal_(generator=g)
                    sets.append((P, dy, torch.empty_like(P)))
                ds, db, cl = torch.empty_like(s), torch.empty_like(s), torch.empty_like(s, dtype=torch.int32)
                s_out, b_out = torch.empty_like(s), torch.empty_like(s)

                def fwd_sym(P, dy, out):
                    ok(sym.lq_fq_forward_group(ptr(P), ptr(s), ptr(out), None, _hip.LQ_Q_NONE, qmin, qmax, 0, R, C, axis, gs, sp), "forward_group")

                def fwd_affine(P, dy, out):
                    ok(lib.lq_fq_forward_group_affine(ptr(P), ptr(s), ptr(b), ptr(out), None, _hip.LQ_Q_NONE, qmin, qmax, 0, R, C, axis, gs, sp),
                       "forward_group_affine")

                def bwd_sym(P, dy, out):
                    ok(sym.lq_fq_backward_group(ptr(P), ptr(s), ptr(dy), qmin, qmax, 0, 1.0, ptr(out), ptr(ds), ptr(cl), None, 0,
                                                R, C, axis, gs, sp), "backward_group")

                def bwd_affine(P, dy, out):
                    ok(lib.lq_fq_backward_group_affine(ptr(P), ptr(s), ptr(b), ptr(dy), qmin, qmax, 0, 1.0, 1.0, ptr(out), ptr(ds), ptr(db),
                                                       ptr(cl), None, 0, R, C, axis, gs, sp), "backward_group_affine")

                def init_absmax(P, dy, out):
                    ok(sym.lq_scale_init_group(ptr(P), ptr(s_out), qmin, qmax, 0, 0, mv, R, C, axis, gs, sp), "scale_init_group")

                def init_minmax(P, dy, out):
                    ok(lib.lq_scale_init_group_minmax(ptr(P), ptr(s_out), ptr(b_out), qmin, qmax, 0, mv, R, C, axis, gs, sp),
                       "scale_init_group_minmax")

                variants = {"forward_group": fwd_sym, "forward_affine": fwd_affine, "backward_group": bwd_sym,
                            "backward_affine": bwd_affine, "init_absmax": init_absmax, "init_minmax": init_minmax}
                times = {k: [] for k in variants}
                k_set = 0
                for fn in variants.values():
                    for P, dy, out in sets:
                        fn(P, dy, out)
                torch.cuda.synchronize(dev)
                for _ in range(args.rounds):
                    for key, fn in variants.items():
                        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(args.inner):
                            fn(*sets[k_set % len(sets)])
                            k_set += 1
                        e.record()
                        torch.cuda.synchronize(dev)
                        times[key].append(a.elapsed_time(e) / args.inner * 1e3)
                row = {"tensor": name, "R": R, "C": C, "axis": axis, "group_size": gs, "q_range": [qmin, qmax], "repeat": repeat,
                       "rounds": args.rounds, "inner": args.inner, "buffer_sets": args.sets,
                       "yardstick": "parent library" if args.parent_lib else "this library", "offset_share": 1.0 / gs}
                for key in variants:
                    row[f"us_{key}"] = statistics.median(times[key])
                    row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
                row["forward_affine_over_group"] = row["us_forward_affine"] / row["us_forward_group"]
                row["backward_affine_over_group"] = row["us_backward_affine"] / row["us_backward_group"]
                row["init_minmax_over_absmax"] = row["us_init_minmax"] / row["us_init_absmax"]
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
