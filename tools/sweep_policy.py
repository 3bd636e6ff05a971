#!/usr/bin/env python3
"""Sweep of the cache-policy mix of K1 and K2 in the BENCH step ("Cache-policy mix").

Needs the development library (make -C learned_quantization_amd/csrc dev; LQ_HIP_LIB=.../liblq_hip_dev.so).  A point is a pair:
K1's rule -- the tail of P it loads with the default policy (tenths of the tensor; "tail44" is 0.3 = 46 MB, the 44 MiB that were
shipped before the mix) and the mix word of the blocks before it -- times K2's rule -- its own tail, a mix mask for P and one
for dy.  lq_dev_set_policy_mix takes
the two mix words (bits 24-27 of K1's hold K1's own tail), lq_dev_set_flags bits 0xf00 K2's tail.  The BENCH tensor, four
rotating buffer sets, the split step K1, K2, K3 back to back as bench.py runs it, every point in turn in one process.  Per point
and round: the un-profiled step time (two events around STEPS steps) and the durations of K1 and K2 stamped by their own
dispatches (lq_profile_events).  "parent" is the rule of the commit before the mix: the tail in both kernels, no mask; "shipped"
runs the constants of this build (kMixK1, kMixK2, kMallKeepBytes).

    python3 tools/sweep_policy.py [--rounds 3] > sweep.jsonl
    python3 tools/sweep_policy.py --summary sweep.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, STEPS, STAMPED = 8, 60, 40


def word(mask_p=0, mask_dy=0, log2run=0):
    return mask_p | (mask_dy << 8) | (log2run << 16)


# K1: (name, tail code: 1 + tenths of the tensor, mix word); a block is 2048 elements
K1 = [("tail44", 4, word()),
      ("run8 3/8", 1, word(0x15, 0, 3)),
      ("run16 3/8", 1, word(0x15, 0, 4)),
      ("run32 1/4", 1, word(0x11, 0, 5)),
      ("tail44 + run8 1/8", 4, word(0x01, 0, 3)),
      ("tail44 + run8 1/4", 4, word(0x11, 0, 3))]
# K2: (name, tail code, mix word); a unit is 4096 elements, so K1's runs of 8 blocks are K2's runs of 4 units
K2 = [("tail44", 4, word()),
      ("tail44 + P blk 1/8", 4, word(0x01)),
      ("P blk 3/8", 1, word(0x15)),
      ("P blk 1/4", 1, word(0x11)),
      ("P run4 3/8", 1, word(0x15, 0, 2)),
      ("P run8 3/8", 1, word(0x15, 0, 3)),
      ("tail44 + dy blk 1/8", 4, word(0, 0x01)),
      ("dy blk 3/8", 1, word(0, 0x15))]


def points():
    pts = []
    for n1, t1, w1 in K1:
        for n2, t2, w2 in K2:
            pts.append({"k1": n1, "k2": n2, "flags": t2 << 8, "w1": w1 | (t1 << 24), "w2": w2})
    pts[0]["parent"] = True
    pts.append({"k1": "shipped", "k2": "shipped", "flags": 0, "w1": 0xffffffff, "w2": 0xffffffff})
    return pts


def summary(path):
    rows = {}
    for ln in open(path):
        if ln.startswith("{"):
            r = json.loads(ln)
            rows.setdefault((r["k1"], r["k2"]), []).append(r)
    print("| K1 | K2 | step µs (rounds) | K1 / K2 µs stamped |")
    print("|---|---|---|---|")
    for (a, b), rs in sorted(rows.items(), key=lambda kv: sorted(r["step_us"] for r in kv[1])[len(kv[1]) // 2]):
        st = [r["step_us"] for r in rs]
        print(f"| {a} | {b} | {min(st):.1f}–{max(st):.1f} | {sum(r['k1_us'] for r in rs) / len(rs):.1f} / "
              f"{sum(r['k2_us'] for r in rs) / len(rs):.1f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lam", type=float, default=1e-11)
    ap.add_argument("--summary")
    args = ap.parse_args()
    if args.summary:
        return summary(args.summary)

    import torch
    import learned_quantization_amd as lq
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _devlib  # noqa: F401  (LQ_HIP_LIB -> _hip.use_library)
    lib = lq._hip.load()
    lib.lq_dev_set_flags.restype = ctypes.c_int
    lib.lq_dev_set_flags.argtypes = [ctypes.c_int]
    lib.lq_dev_set_policy_mix.restype = ctypes.c_int
    lib.lq_dev_set_policy_mix.argtypes = [ctypes.c_uint, ctypes.c_uint]
    dev = torch.device("cuda:0")
    outer, G, inner = 256, 3, 224 * 224
    n, nsets = outer * G * inner, 4
    g = torch.Generator(device=dev).manual_seed(42)
    xs = [torch.rand(n, device=dev, generator=g) * 255.0 for _ in range(nsets)]
    dys = [torch.randn(n, device=dev, generator=g) * 1e-3 for _ in range(nsets)]
    outs = [torch.empty(n, device=dev) for _ in range(nsets)]
    s = torch.tensor([0.5, 1.0, 2.0], device=dev)
    ds = torch.zeros(G, device=dev)
    ws = torch.empty(lib.lq_workspace_bytes(outer, G, inner), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def fwd(k):
        return lib.lq_fq_forward(xs[k].data_ptr(), s.data_ptr(), outs[k].data_ptr(), None, 0, outer, G, inner, None)

    def bwd(k):
        return lib.lq_fq_scale_grad(xs[k].data_ptr(), s.data_ptr(), dys[k].data_ptr(), args.lam, ds.data_ptr(), None, ws.data_ptr(),
                                    ws.numel(), outer, G, inner, None)

    Ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    ev = [(Ev(), Ev(), Ev(), Ev()) for _ in range(STAMPED)]
    for q in ev:
        for e in q:
            e.record(stream)
    t0, t1 = Ev(), Ev()
    torch.cuda.synchronize(dev)
    ref = None
    for rnd in range(args.rounds):
        for pt in points():
            assert lib.lq_dev_set_flags(pt["flags"]) == 0
            assert lib.lq_dev_set_policy_mix(pt["w1"], pt["w2"]) == 0
            rc = 0
            for i in range(WARM):
                rc |= fwd(i % nsets) | bwd(i % nsets)
            t0.record(stream)
            for i in range(STEPS):
                rc |= fwd(i % nsets) | bwd(i % nsets)
            t1.record(stream)
            for j in range(STAMPED):
                k = j % nsets
                lib.lq_profile_events(ev[j][0].cuda_event, ev[j][1].cuda_event)
                rc |= fwd(k)
                lib.lq_profile_events(ev[j][2].cuda_event, ev[j][3].cuda_event)
                rc |= bwd(k)
            lib.lq_profile_events(None, None)
            assert rc == 0, lib.lq_last_error()
            torch.cuda.synchronize(dev)
            # every point computes the same bits
            sig = (ds.cpu().numpy().tobytes(), float(outs[(STAMPED - 1) % nsets].double().sum()))
            if ref is None:
                ref = sig
            assert sig == ref, "a point changed the results"
            k1 = sum(q[0].elapsed_time(q[1]) for q in ev[4:]) / (STAMPED - 4) * 1e3
            k2 = sum(q[2].elapsed_time(q[3]) for q in ev[4:]) / (STAMPED - 4) * 1e3
            print(json.dumps({"round": rnd, "k1": pt["k1"], "k2": pt["k2"], "parent": bool(pt.get("parent")), "w1": pt["w1"],
                              "w2": pt["w2"], "flags": pt["flags"], "step_us": t0.elapsed_time(t1) / STEPS * 1e3, "k1_us": k1,
                              "k2_us": k2}), flush=True)
    lib.lq_dev_set_flags(0)
    lib.lq_dev_set_policy_mix(0xffffffff, 0xffffffff)


if __name__ == "__main__":
    main()
