#!/usr/bin/env python3
"""Sweep of the Infinity Cache reuse between K1 and K2 of the BENCH step ("Infinity Cache reuse").

Needs the development library (make -C learned_quantization_amd/csrc dev; LQ_HIP_LIB=.../liblq_hip_dev.so): every point is a
value of lq_dev_set_flags -- the fraction T of P that K1 loads with the default policy and K2 expects in the cache (0xf00), the
cache policy of K1's `out` stores (0x70) and K2's walk direction (0x1000) -- on the BENCH tensor, four rotating buffer sets,
the split step K1, K2, K3 back to back as bench.py runs it.  Per point and round: the un-profiled step time (two events around
STEPS steps) and the durations of K1 and K2 stamped by their own dispatches (lq_profile_events).

    python3 tools/sweep_mall.py [--rounds 3] > sweep.jsonl
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/sweep_mall.py --rounds 1 > points.jsonl
    python3 tools/sweep_mall.py --parse-trace DIR/.../*_kernel_trace.csv --points points.jsonl      # rocprofv3's K1 / K2 per point
"""
import argparse
import csv
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, STEPS, STAMPED = 8, 60, 40
STORE = {6: "nt", 1: "default", 2: "sc1 nt", 3: "sc0 sc1 nt", 4: "sc1", 5: "sc0 sc1"}


def points(stores):
    pts = [{"T": 0.0, "store": "nt", "walk": "forward", "flags": 0x1000 | (1 << 8) | (6 << 4)},      # the parent's step
           {"T": "shipped", "store": "shipped", "walk": "reverse", "flags": 0}]
    for st in stores:
        for t in range(6):
            pts.append({"T": t / 10.0, "store": STORE[st], "walk": "reverse", "flags": ((t + 1) << 8) | (st << 4)})
    return pts


def parse_trace(path, pts_path):
    pts = [json.loads(ln) for ln in open(pts_path) if ln.startswith("{")]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    k1 = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "k_flat_fwd" in r["Kernel_Name"]]
    k2 = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if "k_row_stream" in r["Kernel_Name"]]
    per = WARM + STEPS + STAMPED
    assert len(k1) == len(k2) == per * len(pts), (len(k1), len(k2), per, len(pts))
    for i, pt in enumerate(pts):
        a, b = k1[i * per + WARM:(i + 1) * per], k2[i * per + WARM:(i + 1) * per]
        print(json.dumps({"T": pt["T"], "store": pt["store"], "walk": pt["walk"], "rocprofv3_k1_us": sum(a) / len(a) / 1e3,
                          "rocprofv3_k2_us": sum(b) / len(b) / 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stores", default="6,1,2,3")
    ap.add_argument("--lam", type=float, default=1e-11)
    ap.add_argument("--parse-trace")
    ap.add_argument("--points")
    args = ap.parse_args()
    if args.parse_trace:
        return parse_trace(args.parse_trace, args.points)

    import torch
    import learned_quantization_amd as lq
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _devlib  # noqa: F401  (LQ_HIP_LIB -> _hip.use_library)
    lib = lq._hip.load()
    lib.lq_dev_set_flags.restype = ctypes.c_int
    lib.lq_dev_set_flags.argtypes = [ctypes.c_int]
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

    def step(k):
        rc = lib.lq_fq_forward(xs[k].data_ptr(), s.data_ptr(), outs[k].data_ptr(), None, 0, outer, G, inner, None)
        rc |= lib.lq_fq_scale_grad(xs[k].data_ptr(), s.data_ptr(), dys[k].data_ptr(), args.lam, ds.data_ptr(), None, ws.data_ptr(),
                                   ws.numel(), outer, G, inner, None)
        assert rc == 0, lib.lq_last_error()

    Ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    ev = [(Ev(), Ev(), Ev(), Ev()) for _ in range(STAMPED)]
    for q in ev:
        for e in q:
            e.record(stream)
    t0, t1 = Ev(), Ev()
    torch.cuda.synchronize(dev)
    ref = None
    for rnd in range(args.rounds):
        for pt in points([int(v) for v in args.stores.split(",")]):
            assert lib.lq_dev_set_flags(pt["flags"]) == 0
            for i in range(WARM):
                step(i % nsets)
            t0.record(stream)
            for i in range(STEPS):
                step(i % nsets)
            t1.record(stream)
            for j in range(STAMPED):
                k = j % nsets
                lib.lq_profile_events(ev[j][0].cuda_event, ev[j][1].cuda_event)
                rc = lib.lq_fq_forward(xs[k].data_ptr(), s.data_ptr(), outs[k].data_ptr(), None, 0, outer, G, inner, None)
                lib.lq_profile_events(ev[j][2].cuda_event, ev[j][3].cuda_event)
                rc |= lib.lq_fq_scale_grad(xs[k].data_ptr(), s.data_ptr(), dys[k].data_ptr(), args.lam, ds.data_ptr(), None,
                                           ws.data_ptr(), ws.numel(), outer, G, inner, None)
                assert rc == 0, lib.lq_last_error()
            lib.lq_profile_events(None, None)
            torch.cuda.synchronize(dev)
            # every point computes the same bits
            sig = (ds.cpu().numpy().tobytes(), float(outs[(STAMPED - 1) % nsets].double().sum()))
            if ref is None:
                ref = sig
            assert sig == ref, "a point changed the results"
            k1 = sum(q[0].elapsed_time(q[1]) for q in ev[4:]) / (STAMPED - 4) * 1e3
            k2 = sum(q[2].elapsed_time(q[3]) for q in ev[4:]) / (STAMPED - 4) * 1e3
            print(json.dumps({"round": rnd, "T": pt["T"], "store": pt["store"], "walk": pt["walk"],
                              "step_us": t0.elapsed_time(t1) / STEPS * 1e3, "k1_us": k1, "k2_us": k2}), flush=True)
    lib.lq_dev_set_flags(0)


if __name__ == "__main__":
    main()
