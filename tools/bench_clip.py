#!/usr/bin/env python3
"""The clipped fake-quant pair next to its yardsticks, interleaved in one process on rotating buffers.

  * ``lq_fq_forward_clip`` against ``lq_fq_forward`` (one read, one write);
  * ``lq_fq_backward_clip`` against ``lq_fq_fwd_bwd_fused`` (two reads, one write, a per-group reduction);
  * the round-to-nearest pair (``lq_fq_forward_clip_r`` / ``lq_fq_backward_clip_r`` with LQ_ROUND_NEAREST_EVEN) against the floor
    pair, which is its yardstick.  The margin is the floor pair's own spread: the rounds are cut into ``--repeats`` consecutive
    blocks, each block has its median, and ``*_floor_spread`` is (max - min) / median of the floor kernel's block medians; a
    ``nearest_*_over_floor`` ratio further from 1 than that spread is outside the margin;

on the BENCH tensor (256, 3, 50176) and on the largest ResNet-18-like weight (3, 3, 512, 512), channel-wise, stored OIHW.
Raw C-ABI calls into preallocated outputs; every round times each variant once (event-timed run of ``--inner`` back-to-back
calls, each on the next buffer set), the rounds interleave the variants, the figure is the median over the rounds.  One JSON
line per tensor.  Run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel figures.

    python tools/bench_clip.py [--rounds 15] [--inner 10] [--sets 3] [--repeats 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3, help="blocks of rounds whose medians give the floor pair's own spread")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    sp = _hip.stream_ptr(dev)
    qmin, qmax = ops.q_range_of(args.bits)
    cases = [("bench", (256, 3, 50176), (1, 3, 1), None),
             ("resnet18_conv_512x512", (3, 3, 512, 512), (1, 1, 512, 1), "oihw")]
    for name, shape, sshape, storage in cases:
        g = torch.Generator(device=dev).manual_seed(42)
        sets = []
        for _ in range(args.sets):
            P = torch.empty(shape, device=dev).normal_(generator=g) * 0.05
            dy = torch.empty(shape, device=dev).normal_(generator=g)
            if storage == "oihw":
                P = P.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)
                dy = dy.permute(3, 2, 0, 1).contiguous().permute(2, 3, 1, 0)
            sets.append((P, dy, torch.empty_like(P)))
        s = torch.full(sshape, 0.05 / 2 ** (args.bits - 2), device=dev)
        p0, s0, (outer, G, inner) = ops._param(sets[0][0], s)
        ds = torch.empty_like(s0)
        clipped = torch.empty_like(s0, dtype=torch.int32)
        ws = _hip.workspace_for(dev, outer, G, inner)
        ptr = _hip.ptr

        def fwd(P, dy, out):
            _hip.check(lib.lq_fq_forward(ptr(P), ptr(s0), ptr(out), None, _hip.LQ_Q_NONE, outer, G, inner, sp), "fwd")

        def fwd_clip(P, dy, out):
            _hip.check(lib.lq_fq_forward_clip(ptr(P), ptr(s0), ptr(out), None, _hip.LQ_Q_NONE, qmin, qmax, outer, G, inner, sp), "fwd_clip")

        def fused(P, dy, out):
            _hip.check(lib.lq_fq_fwd_bwd_fused(ptr(P), ptr(s0), ptr(dy), 1e-11, ptr(out), ptr(ds), ptr(ws), ws.numel(), outer, G, inner, sp), "fused")

        def bwd_clip(P, dy, out):
            _hip.check(lib.lq_fq_backward_clip(ptr(P), ptr(s0), ptr(dy), qmin, qmax, 1.0, ptr(out), ptr(ds), ptr(clipped), ptr(ws),
                                               ws.numel(), outer, G, inner, sp), "bwd_clip")

        def bwd_clip_mask(P, dy, out):
            _hip.check(lib.lq_fq_backward_clip(ptr(P), ptr(s0), ptr(dy), qmin, qmax, 1.0, ptr(out), None, None, ptr(ws),
                                               ws.numel(), outer, G, inner, sp), "bwd_clip_mask")

        nearest = 1      # LQ_ROUND_NEAREST_EVEN

        def fwd_clip_rne(P, dy, out):
            _hip.check(lib.lq_fq_forward_clip_r(ptr(P), ptr(s0), ptr(out), None, _hip.LQ_Q_NONE, qmin, qmax, nearest, outer, G, inner, sp),
                       "fwd_clip_rne")

        def bwd_clip_rne(P, dy, out):
            _hip.check(lib.lq_fq_backward_clip_r(ptr(P), ptr(s0), ptr(dy), qmin, qmax, nearest, 1.0, ptr(out), ptr(ds), ptr(clipped), ptr(ws),
                                                 ws.numel(), outer, G, inner, sp), "bwd_clip_rne")

        def bwd_clip_rne_mask(P, dy, out):
            _hip.check(lib.lq_fq_backward_clip_r(ptr(P), ptr(s0), ptr(dy), qmin, qmax, nearest, 1.0, ptr(out), None, None, ptr(ws),
                                                 ws.numel(), outer, G, inner, sp), "bwd_clip_rne_mask")

        variants = {"forward": fwd, "forward_clip": fwd_clip, "forward_clip_nearest": fwd_clip_rne, "fused": fused,
                    "backward_clip": bwd_clip, "backward_clip_nearest": bwd_clip_rne, "backward_clip_mask_only": bwd_clip_mask,
                    "backward_clip_nearest_mask_only": bwd_clip_rne_mask}
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
        n = sets[0][0].numel()
        row = {"tensor": name, "shape": list(shape), "descriptor": [outer, G, inner], "q_range": [qmin, qmax], "rounds": args.rounds,
               "inner": args.inner, "buffer_sets": args.sets}
        for key in variants:
            row[f"us_{key}"] = statistics.median(times[key])
            row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
        row["tb_per_s_forward_clip"] = 8 * n / row["us_forward_clip"] / 1e6
        row["tb_per_s_backward_clip"] = 12 * n / row["us_backward_clip"] / 1e6
        row["forward_clip_over_forward"] = row["us_forward_clip"] / row["us_forward"]
        row["backward_clip_over_fused"] = row["us_backward_clip"] / row["us_fused"]

        def block_medians(key):
            n_blocks = max(1, min(args.repeats, len(times[key])))
            size = len(times[key]) // n_blocks
            return [statistics.median(times[key][b * size:(b + 1) * size]) for b in range(n_blocks)]

        for what, floor_key, near_key in (("forward", "forward_clip", "forward_clip_nearest"),
                                          ("backward", "backward_clip", "backward_clip_nearest"),
                                          ("backward_mask_only", "backward_clip_mask_only", "backward_clip_nearest_mask_only")):
            blocks = block_medians(floor_key)
            row[f"us_{floor_key}_block_medians"] = blocks
            row[f"us_{near_key}_block_medians"] = block_medians(near_key)
            spread = (max(blocks) - min(blocks)) / row[f"us_{floor_key}"]
            ratio = row[f"us_{near_key}"] / row[f"us_{floor_key}"]
            row[f"{what}_floor_spread"] = spread
            row[f"nearest_{what}_over_floor"] = ratio
            row[f"nearest_{what}_within_floor_spread"] = abs(ratio - 1.0) <= spread
        print(json.dumps(row), flush=True)
        del sets


if __name__ == "__main__":
    main()
