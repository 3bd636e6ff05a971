#!/usr/bin/env python3
"""End-to-end cost of ``Trainer(loss_values=True)``: images/s of the CIFAR-CNN step in mode "cl" with the MaxBin term
(synthetic data, batch 256), the cases alternating in one process:

    batched_graph / batched_graph_loss_values            the batched, graphed step without and with the penalty value + device log
    per_tensor_eager / ..._log_every_step / ..._loss_values   the per-tensor eager step: plain, with the loss object's host-side
                                                         per-step logs (a device->host synchronisation per step), with the
                                                         device-side log instead

    python3 tools/e2e_loss_values.py [--steps 200] [--warmup 30] [--batch 256] > profiles/penalty_values/e2e.jsonl
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from learned_quantization_amd.train import Trainer, synthetic_batch  # noqa: E402


def run(tag, args, dev, log_every_step=False, **kw):
    graph = kw.get("graph", False)
    tr = Trainer("cifar", "cl", 1e-7, "channelwise", "maxbin", device=dev, log_dir=tempfile.mkdtemp(), **kw)
    if log_every_step:
        tr.loss_obj.log_every_step = True
    do = tr.step_graphed if graph else tr.step
    g = torch.Generator(device=dev).manual_seed(42)
    bs = [synthetic_batch("cifar", args.batch, dev, g) for _ in range(4)]
    for i in range(args.warmup):
        do(*bs[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = do(*bs[i % 4])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if tr.loss_log is not None:
        tr.flush_loss_log()
    print(json.dumps({"case": tag, "images_per_s": args.batch * args.steps / dt, "ms_per_step": dt / args.steps * 1e3,
                      "final_loss": float(loss.detach()), **kw}), flush=True)
    del tr
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for _ in range(3):
        run("batched_graph", args, dev, batched=True, graph=True)
        run("batched_graph_loss_values", args, dev, batched=True, graph=True, loss_values=True)
    for _ in range(2):
        run("per_tensor_eager", args, dev, batched=False)
        run("per_tensor_eager_log_every_step", args, dev, log_every_step=True, batched=False)
        run("per_tensor_eager_loss_values", args, dev, batched=False, loss_values=True)


if __name__ == "__main__":
    main()
