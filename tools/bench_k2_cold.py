#!/usr/bin/env python3
"""K2 (lq_fq_scale_grad) and K1 (lq_fq_forward) of the BENCH tensor ALONE, in a loop over four rotating buffer sets, so that
P is never in the Infinity Cache when a kernel starts: the cold case of the cache reuse between K1 and K2 (DESIGN.md section 3,
"Infinity Cache reuse"), which must cost nothing there.  The kernels' own durations (lq_profile_events), one JSON line.

    python3 tools/bench_k2_cold.py [--root OTHER_CHECKOUT] [--label NAME] [--n 100]

--root: import the package (and its in-tree library) from another checkout of this repository, e.g. the parent commit, for
alternating A/B runs in one job."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--n", type=int, default=100)
ap.add_argument("--lam", type=float, default=1e-11)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402

from learned_quantization_amd import _hip  # noqa: E402

lib = _hip.load()
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
Ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
WARM = 8


def k2(k):
    return lib.lq_fq_scale_grad(xs[k].data_ptr(), s.data_ptr(), dys[k].data_ptr(), args.lam, ds.data_ptr(), None, ws.data_ptr(),
                                ws.numel(), outer, G, inner, None)


def k1(k):
    return lib.lq_fq_forward(xs[k].data_ptr(), s.data_ptr(), outs[k].data_ptr(), None, 0, outer, G, inner, None)


def alone(fn):
    ev = [(Ev(), Ev()) for _ in range(args.n + WARM)]
    for a, b in ev:                 # torch creates the hipEvent_t at the first record
        a.record(stream)
        b.record(stream)
    torch.cuda.synchronize(dev)
    rc = 0
    for j, (a, b) in enumerate(ev):
        lib.lq_profile_events(a.cuda_event, b.cuda_event)
        rc |= fn(j % nsets)
    lib.lq_profile_events(None, None)
    assert rc == 0, lib.lq_last_error()
    torch.cuda.synchronize(dev)
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[WARM:])
    return {"mean_us": sum(t) / len(t), "median_us": t[len(t) // 2], "min_us": t[0]}


res = {"label": args.label, "n": args.n, "lam": args.lam, "k2_alone": alone(k2), "k1_alone": alone(k1)}
print(json.dumps(res))
