#!/usr/bin/env python3
"""The straight-through scale gradient next to the nested-quantization one, same session, same buffers.

  * batch: ``lq_batch_scale_grad_ste`` against ``lq_batch_scale_grad`` on the ResNet-18-like and ResNet-50-like weight sets
    (channelwise, kernels stored OIHW); both read P and dy (8 B per element), each is a traversal + a finalize launch;
  * one streaming tensor: ``lq_fq_scale_grad_ste`` (generic bodies, 256-thread units at every size) against ``lq_fq_scale_grad``
    (K2's streaming forms) on the BENCH tensor (256, 3, 50176).

Event-timed loops of back-to-back calls (microseconds per call, traversal + finalize); run it under
``rocprofv3 --kernel-trace --stats`` for the per-kernel figures.  One JSON line per measurement.

    python tools/bench_ste_scale.py [--steps 200] [--sets imagenette,resnet50] [--no-bench-tensor]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import learned_quantization_amd as lq  # noqa: E402


def timed(fn, steps, dev):
    for _ in range(10):
        fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sets", default="imagenette,resnet50")
    ap.add_argument("--no-bench-tensor", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = lq._hip.load()
    sp = lq._hip.stream_ptr(dev)
    for config in [c for c in args.sets.split(",") if c]:
        row = {"config": config, "orientation": "channelwise", "kernel_storage": "oihw"}
        for rule in ("nq", "ste"):
            lq.reset_layer_names()
            value = (1e-10, 1e-11) if (config == "resnet50" and rule == "nq") else 1e-11
            model = lq.build_model(config, mode=rule, value=value, seed=42, orientation="channelwise", device=dev)
            batch = lq.FakeQuantBatch(model)
            g = torch.Generator(device=dev).manual_seed(42)
            dys = [torch.empty_like(e.param.data).normal_(generator=g) * 1e-3 for e in batch.entries]
            ptrs = (ctypes.c_void_p * len(dys))(*[d.data_ptr() for d in dys])
            row["tensors"], row["elements"] = len(batch.entries), sum(e.param.numel() for e in batch.entries)
            if rule == "nq":
                def call():
                    lq._hip.check(lib.lq_batch_scale_grad(batch._handle, ptrs, batch.ws.data_ptr(), batch.ws.numel(), sp), "nq")
            else:
                def call():
                    lq._hip.check(lib.lq_batch_scale_grad_ste(batch._handle, ptrs, None, batch.ws.data_ptr(), batch.ws.numel(), sp), "ste")
            row[f"us_per_call_{rule}"] = timed(call, args.steps, dev)
            del batch, model
        row["ste_over_nq"] = row["us_per_call_ste"] / row["us_per_call_nq"]
        print(json.dumps(row), flush=True)
    if not args.no_bench_tensor:
        shape = (256, 3, 50176)
        g = torch.Generator(device=dev).manual_seed(42)
        P = torch.empty(shape, device=dev).normal_(generator=g) * 0.05
        dy = torch.empty(shape, device=dev).normal_(generator=g) * 1e-3
        s = torch.full((1, 3, 1), lq.SCALE_INIT, device=dev)
        row = {"tensor": list(shape), "bytes_read": 8 * P.numel()}
        row["us_per_call_nq"] = timed(lambda: lq.fq_scale_grad(P, s, dy, 1e-11), max(args.steps // 2, 10), dev)
        row["us_per_call_ste"] = timed(lambda: lq.fq_scale_grad_ste(P, s, dy), max(args.steps // 2, 10), dev)
        for k in ("nq", "ste"):
            row[f"tb_per_s_{k}"] = row["bytes_read"] / row[f"us_per_call_{k}"] / 1e6
        row["ste_over_nq"] = row["us_per_call_ste"] / row["us_per_call_nq"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
