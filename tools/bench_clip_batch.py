#!/usr/bin/env python3
"""The clipped multi-tensor batch next to what it replaces and next to its yardstick, on the ResNet-18-like weight set of
tools/bench_weights.py (config "imagenette": 40 tensors, 11.2 M elements, conv kernels stored OIHW), rule "ste".

One process alternates three steps, raw C-ABI calls into preallocated buffers, no optimizer:

  (a) ``clip_batch``   lq_batch_forward_clip + lq_batch_backward_clip                    3 launches, 8 + 12 = 20 B per element
  (b) ``clip_single``  lq_fq_forward_clip_r + lq_fq_backward_clip_r, one call per tensor: what a ``bits`` model runs without the batch
  (c) ``ste_batch``    lq_batch_forward + lq_batch_scale_grad_ste (the unclipped batch)  3 launches, 8 + 8 = 16 B per element

Every round times each variant once (device events around ``--inner`` back-to-back steps), the rounds interleave the variants,
the figure is the median over the rounds.  ``frac_of_8tbs_*`` is (bytes per element x elements / time) / 8 TB/s with 20 B for
(a) and (b) and 16 B for (c): a whole-step rate over the HBM peak, not a kernel's share of it (the 45 MB of weights stay in the
256 MB Infinity Cache between the launches of a step).  One JSON line per rounding.

    python tools/bench_clip_batch.py [--rounds 15] [--inner 10] [--bits 4] [--config imagenette]
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

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import _hip, ops  # noqa: E402


def build(config, dev, bits, rounding, orientation):
    lq.reset_layer_names()
    kw = dict(bits=bits, rounding=rounding) if bits is not None else {}
    model = lq.build_model(config, mode="ste", value=0.0, seed=42, orientation=orientation, device=dev, grad_scale="rsqrt_group", **kw)
    with torch.no_grad():          # weights ~ N(0, 0.05): the range's edges sit about two standard deviations out
        for s in lq.scale_parameters(model):
            s.fill_(0.05 / 2 ** ((bits or 4) - 2))
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--config", default="imagenette")
    ap.add_argument("--orientation", default="channelwise")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr
    plain = lq.FakeQuantBatch(build(args.config, dev, None, "floor", args.orientation), autograd=False)
    assert plain.ste and not plain.clipped
    for rounding in ops.ROUNDINGS:
        rnd = ops.check_rounding(rounding)
        cb = lq.FakeQuantBatch(build(args.config, dev, args.bits, rounding, args.orientation), autograd=False, clipped=True)
        n = len(cb.entries)
        g = torch.Generator(device=dev).manual_seed(42)
        dys = [torch.empty_like(e.param.data).normal_(generator=g) * 1e-3 for e in cb.entries]           # the parameter's strides
        ptrs = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dys])
        n_el = sum(e.param.numel() for e in cb.entries)
        assert [tuple(e.param.shape) for e in plain.entries] == [tuple(e.param.shape) for e in cb.entries]
        single, keep = [], []                 # (b): per tensor, preallocated out / dP / ds / counts (kept alive in ``keep``)
        for e in cb.entries:
            p, s, (outer, G, inner) = ops._param(e.param.data, e.nested.scale.data)
            bufs = [torch.empty_like(p), torch.empty_like(p), torch.empty_like(s), torch.empty_like(s, dtype=torch.int32)]
            keep.append(bufs)
            single.append((ptr(p), ptr(s), *[ptr(t) for t in bufs], e.nested.q_range, float(e.nested.grad_scale_value(p.numel())),
                           outer, G, inner))
        ws1 = _hip.workspace(dev, max(lib.lq_workspace_bytes(*t[8:]) for t in single))

        def clip_batch():
            _hip.check(lib.lq_batch_forward_clip(cb._handle, sp), "lq_batch_forward_clip")
            _hip.check(lib.lq_batch_backward_clip(cb._handle, ptrs, cb._grad_scales, ptr(cb.ws), cb.ws.numel(), sp), "lq_batch_backward_clip")

        def clip_single():
            for (P, s, out, dP, ds, cl, (qmin, qmax), gs, outer, G, inner), d in zip(single, dys):
                _hip.check(lib.lq_fq_forward_clip_r(P, s, out, None, _hip.LQ_Q_NONE, qmin, qmax, rnd, outer, G, inner, sp), "forward_clip")
                _hip.check(lib.lq_fq_backward_clip_r(P, s, ptr(d), qmin, qmax, rnd, gs, dP, ds, cl, ptr(ws1), ws1.numel(), outer, G, inner, sp),
                           "backward_clip")

        def ste_batch():
            _hip.check(lib.lq_batch_forward(plain._handle, sp), "lq_batch_forward")
            _hip.check(lib.lq_batch_scale_grad_ste(plain._handle, ptrs, plain._grad_scales, ptr(plain.ws), plain.ws.numel(), sp),
                       "lq_batch_scale_grad_ste")

        variants = {"clip_batch": clip_batch, "clip_single": clip_single, "ste_batch": ste_batch}
        times = {key: [] for key in variants}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize(dev)
        for _ in range(args.rounds):
            for key, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    fn()
                b.record()
                torch.cuda.synchronize(dev)
                times[key].append(a.elapsed_time(b) / args.inner * 1e3)
        row = {"config": args.config, "orientation": args.orientation, "tensors": n, "elements": n_el, "bits": args.bits, "rounding": rounding,
               "rule": "ste", "rounds": args.rounds, "inner": args.inner}
        for key, nbytes in (("clip_batch", 20), ("clip_single", 20), ("ste_batch", 16)):
            row[f"us_{key}"] = statistics.median(times[key])
            row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
            row[f"frac_of_8tbs_{key}"] = nbytes * n_el / row[f"us_{key}"] / 1e6 / 8.0
        row["clip_batch_over_clip_single"] = row["us_clip_batch"] / row["us_clip_single"]
        row["clip_batch_over_ste_batch"] = row["us_clip_batch"] / row["us_ste_batch"]
        row["byte_ratio_20_over_16"] = 1.25
        print(json.dumps(row), flush=True)
        del cb


if __name__ == "__main__":
    main()
