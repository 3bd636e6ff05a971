#!/usr/bin/env python3
"""This build's batch.py next to the parent commit's, on the one built library (profiles/batch_kinds).

    git show HEAD~1:learned_quantization_amd/batch.py > PARENT.py
    python3 tools/batch_parent_ab.py --parent PARENT.py --bits [--out FILE]
    python3 tools/batch_parent_ab.py --parent PARENT.py --time [--out FILE]

``--parent`` names the parent commit's batch.py; it is loaded as a second module of the package (its relative imports resolve to
this tree: same _hip, same layers, same liblq_hip.so), so the only difference between the two sides is the Python of batch.py.

Four configurations: the default batch over a nested-quantization model, ``clipped=True``, ``group_batch=True`` and
``group_batch=True, asymmetric=True`` over 4-bit "ste" models (group size 64).  Both sides build the same seeded model, with
scales drawn from U(1e-3, 1e-2) and offsets from U(-3e-3, 3e-3).  A step is ``quantize_all()``, a seeded ``dy`` assigned to
every leaf, ``finish_backward()``, ``BatchedScaleAdam.step()``.

``--bits``: the ``mnist`` model (4 tensors) and the ``cifar`` CNN (12 tensors), three steps with ``autograd=False`` per
configuration and three with ``autograd=True`` for the default kind.  After every step every ``out``, ``dP``, ``scale.grad``,
``offset.grad``, ``clip_counts()``, scale and offset of the two sides are compared with ``torch.equal`` on their raw bits.  One
line per run; exit status 1 unless no tensor differs.

``--time``: the ``autograd=False`` step on the CIFAR CNN: host clock over 2000 iterations after 200 warm-ups, one device
synchronise after the loop (tools/host_overhead.py); parent and new alternately in one process, three repeats each.  One JSON
line per configuration; exit status 1 unless every new median lies inside or below the parent's own min-max range."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("default", dict(mode="nq", value=1e-3), dict()),
           ("clipped", dict(mode="ste", value=0.0, bits=4), dict(clipped=True)),
           ("group", dict(mode="ste", value=0.0, bits=4, group_size=64), dict(group_batch=True)),
           ("group asymmetric", dict(mode="ste", value=0.0, bits=4, group_size=64, asymmetric=True), dict(group_batch=True, asymmetric=True))]
STEPS, WARMUP, ITERS, REPEATS = 3, 200, 2000, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's learned_quantization_amd/batch.py")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--bits", action="store_true")
    what.add_argument("--time", action="store_true")
    ap.add_argument("--out", default=None, help="write the report to this file as well")
    args = ap.parse_args()

    import torch
    import learned_quantization_amd as lq
    from learned_quantization_amd import batch as new

    spec = importlib.util.spec_from_file_location("learned_quantization_amd._parent_batch", os.path.abspath(args.parent))
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    sides = (("parent", parent), ("new", new))
    dev = torch.device("cuda:0")

    def raw(t):
        return t.detach().contiguous().view(torch.uint8)

    def build(mod, config, model_kw, batch_kw, autograd):
        """(batch, optimizer) over a freshly built model: the same weights, scales and offsets on every call."""
        lq.reset_layer_names()
        model = lq.build_model(config, seed=3, device=dev, **model_kw)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for layer in lq.custom_layers_of(model):
                for _, nested, _ in layer.scale_pairs():
                    nested.scale.copy_((torch.rand(nested.scale.shape, generator=g) * 9e-3 + 1e-3).to(dev))
                    if getattr(nested, "asymmetric", False):
                        nested.offset.copy_(((torch.rand(nested.offset.shape, generator=g) - 0.5) * 6e-3).to(dev))
        batch = mod.FakeQuantBatch(model, hwio_out=False, autograd=autograd, **batch_kw)
        return batch, mod.BatchedScaleAdam(batch)

    def upstream(batch, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        # in the parameter's element order: no relayout copy inside the step
        return [torch.empty_like(e.param.data).copy_(torch.randn(e.param.shape, device=dev, generator=g).mul_(1e-3)) for e in batch.entries]

    def step(batch, opt, dys):
        opt.zero_grad()
        for e in batch.entries:
            e.param.grad = None
        outs = batch.quantize_all()
        if batch.autograd:
            torch.autograd.backward(outs, dys)
        else:
            for i, d in enumerate(dys):
                # a companion-only kernel has its leaf in OIHW order
                if batch._leaf[i] is not None:
                    batch._leaf[i].grad = d
                else:
                    batch._leaf_o[i].grad = d.permute(3, 2, 0, 1).contiguous()
            batch.finish_backward()
        opt.step()

    def snapshot(batch, counts):
        got = []
        for e in batch.entries:
            got += [e.out if e.out is not None else e.out_oihw, e.param.grad, e.scale.grad, e.scale.data]
            if e.offset is not None:
                got += [e.offset.grad, e.offset.data]
        if counts:
            got += batch.clip_counts()
        return [None if t is None else raw(t).clone() for t in got]

    report = []

    def say(line):
        report.append(line)
        print(line, flush=True)

    bad = 0
    if args.bits:
        runs = [(config, name, mkw, bkw, False) for config in ("mnist", "cifar") for name, mkw, bkw in CONFIGS]
        runs += [(config, "default", CONFIGS[0][1], CONFIGS[0][2], True) for config in ("mnist", "cifar")]
        for config, name, mkw, bkw, autograd in runs:
            shots = {}
            for side, mod in sides:
                batch, opt = build(mod, config, mkw, bkw, autograd)
                shots[side] = []
                for k in range(STEPS):
                    step(batch, opt, upstream(batch, 100 + k))
                    shots[side] += snapshot(batch, counts=bool(bkw))
                torch.cuda.synchronize(dev)
            a, b = shots["parent"], shots["new"]
            assert len(a) == len(b) and any(t is not None for t in a)
            differ = sum(1 for x, y in zip(a, b) if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)))
            compared = sum(1 for x in a if x is not None)
            bad += differ
            say(f"{config:6s} {name:17s} autograd={autograd!s:5s} {STEPS} steps: tensors compared {compared:4d}  differing {differ}")
        say(f"total differing tensors: {bad}")
    else:
        for name, mkw, bkw in CONFIGS:
            built = {}
            for side, mod in sides:
                batch, opt = build(mod, "cifar", mkw, bkw, False)
                built[side] = (batch, opt, upstream(batch, 100))
            us = {"parent": [], "new": []}
            for _ in range(REPEATS):
                for side, _mod in sides:
                    batch, opt, dys = built[side]
                    for _ in range(WARMUP):
                        step(batch, opt, dys)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(ITERS):
                        step(batch, opt, dys)
                    t1 = time.perf_counter()
                    torch.cuda.synchronize(dev)
                    us[side].append((t1 - t0) / ITERS * 1e6)
            lo, hi, med = min(us["parent"]), max(us["parent"]), statistics.median(us["new"])
            ok = med <= hi
            bad += 0 if ok else 1
            say(json.dumps({"config": name, "model": "cifar", "tensors": len(built["new"][0].entries), "iters": ITERS, "warmup": WARMUP,
                            "parent_host_us": [round(v, 2) for v in us["parent"]], "new_host_us": [round(v, 2) for v in us["new"]],
                            "parent_range_us": [round(lo, 2), round(hi, 2)], "new_median_us": round(med, 2),
                            "new_inside_or_below_parent_range": ok}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
