#!/usr/bin/env python3
"""Symmetric + absmax against asymmetric + minmax on the MNIST config (synthetic batches), an observation for DESIGN.md: the share
of the first layer's weights that the first forward clips, the squared quantization error of that layer at the start, and the mean
loss of the last 20 of ``--steps`` training steps, at 3 and 4 bits, group size 64, both roundings.  One JSON line per setting.

    python tools/affine_training_note.py [--steps 200] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd.train import Trainer, synthetic_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--group-size", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for bits in (3, 4):
        for rounding in ("floor", "nearest"):
            for asymmetric, init in ((False, "absmax"), (True, "minmax")):
                tr = Trainer(config="mnist", mode="ste", value=0.0, device=dev, log_dir=tempfile.mkdtemp(), seed=7, bits=bits,
                             group_size=args.group_size, rounding=rounding, asymmetric=asymmetric, scale_init=init, lr=1e-3)
                layer = tr.custom_layers[0]
                nested, W = layer.nested_q_w_layer, layer.W.data
                zero = torch.zeros_like(W)
                if asymmetric:
                    out = lq.fq_forward_group_affine(W, nested.scale.data, nested.offset.data, *tr.q_range, args.group_size, rounding=rounding)
                    clipped = lq.fq_backward_group_affine(W, nested.scale.data, nested.offset.data, zero, *tr.q_range, args.group_size,
                                                          want_ds=False, want_db=False, want_clipped=True, rounding=rounding)[3]
                else:
                    out = lq.fq_forward_group(W, nested.scale.data, *tr.q_range, args.group_size, rounding=rounding)
                    clipped = lq.fq_backward_group(W, nested.scale.data, zero, *tr.q_range, args.group_size, want_ds=False,
                                                   want_clipped=True, rounding=rounding)[2]
                g = torch.Generator(device=dev).manual_seed(7)
                batches = [synthetic_batch("mnist", 128, dev, g) for _ in range(4)]
                losses = [float(tr.step(*batches[i % 4])) for i in range(args.steps)]
                row = {"bits": bits, "rounding": rounding, "asymmetric": asymmetric, "scale_init": init, "group_size": args.group_size,
                       "first_layer_clip_share": float(clipped.sum()) / W.numel(),
                       "first_layer_squared_error": float(((W - out).double() ** 2).sum()), "steps": args.steps,
                       "loss_first": losses[0], "loss_last20_mean": sum(losses[-20:]) / 20}
                line = json.dumps(row)
                print(line, flush=True)
                lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
