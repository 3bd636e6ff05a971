#!/usr/bin/env python3
"""Times lq_q_pack and lq_q_unpack (to `out`) with device events on the BENCH tensor (256x3x224x224 fp32, bench.py):
per-channel scales [0.5, 1, 2] (rand*255: 9 bits), per-tensor 1 (8 bits), and BENCH-wlike (N(0, 0.05), s = 1.1920929e-05:
~16 bits).  Buffer sets rotate (>= 4, > 1 GiB in all) so that no launch finds its operands in the 256 MiB MALL.
Reports the median kernel time, the algorithmic bytes (4 + bits/8) * n and the fraction of the 8 TB/s HBM spec.

    python3 tools/bench_pack.py [--iters 50] [--sets 4] [--model resnet50]

``--model``: also the wall time (host included) of save_packed_parameters / load_packed_parameters of that model."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import _hip, ops  # noqa: E402
from learned_quantization_amd.descriptor import group_descriptor  # noqa: E402

HBM_SPEC = 8.0e12
SHAPE = (256, 3, 224, 224)


def time_launches(fn, sets, iters, warmup=5):
    st = torch.cuda.current_stream()
    for k in range(warmup):
        fn(k % sets)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for k, (a, b) in enumerate(evs):
        a.record(st)
        fn(k % sets)
        b.record(st)
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    return t[len(t) // 2], t[0]


def case(name, xs, s, iters):
    lib = _hip.load()
    dev = xs[0].device
    n = xs[0].numel()
    outer, G, inner = group_descriptor(tuple(xs[0].shape), tuple(s.shape))
    _, qmin, bits = ops.q_pack(xs[0], s)
    words = [torch.empty(ops.packed_words(n, bits), dtype=torch.int32, device=dev) for _ in xs]
    outs = [torch.empty_like(x) for x in xs]
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = _hip.stream_ptr(dev)

    def pack(k):
        lib.lq_q_pack(xs[k].data_ptr(), s.data_ptr(), qmin, bits, words[k].data_ptr(), bad.data_ptr(), outer, G, inner, stream)

    def unpack(k):
        lib.lq_q_unpack(words[k].data_ptr(), qmin, bits, s.data_ptr(), outs[k].data_ptr(), None, None, None, outer, G, inner,
                        stream)

    pk, pk_min = time_launches(pack, len(xs), iters)
    uk, uk_min = time_launches(unpack, len(xs), iters)
    assert int(bad.item()) == 0
    assert torch.equal(outs[0], ops.fq_forward(xs[0], s))            # the timed unpack reproduces K1's out
    nbytes = (4 + bits / 8) * n
    total = sum(x.numel() * 4 for x in xs) + sum(w.numel() * 4 for w in words) + sum(o.numel() * 4 for o in outs)
    return {"case": name, "numel": n, "bits": bits, "sets": len(xs), "buffers_gib": total / 2 ** 30,
            "algorithmic_bytes": nbytes,
            "pack_us": pk, "pack_us_min": pk_min, "pack_frac_of_8TBs": nbytes / (pk * 1e-6) / HBM_SPEC,
            "unpack_us": uk, "unpack_us_min": uk_min, "unpack_frac_of_8TBs": nbytes / (uk * 1e-6) / HBM_SPEC}


def model_wall(config, dev):
    lq.reset_layer_names()
    m = lq.build_model(config, device=dev)
    with tempfile.TemporaryDirectory() as d:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = lq.save_packed_parameters(m, d)
        t1 = time.perf_counter()
        lq.reset_layer_names()
        fresh = lq.build_model(config, device=dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        lq.load_packed_parameters(fresh, d)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
    n = sum(p.numel() for _, p, _ in lq.export.quantized_tensors(m))
    return {"model": config, "quantized_elements": n, "tensors": len(lq.export.quantized_tensors(m)),
            "export_s": t1 - t0, "restore_s": t3 - t2, **info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--model", default=None, help="also time the whole-model export / restore of this build_model config")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(42)
    sets = max(4, args.sets)
    xs = [torch.rand(SHAPE, device=dev, generator=g) * 255.0 for _ in range(sets)]
    res = [case("bench_per_channel", xs, torch.tensor([0.5, 1.0, 2.0], device=dev).view(1, 3, 1, 1), args.iters),
           case("bench_per_tensor", xs, torch.tensor([1.0], device=dev), args.iters)]
    for x in xs:
        x.normal_(0.0, 0.05, generator=g)
    res.append(case("bench_wlike", xs, torch.tensor([1.1920929e-05], device=dev), args.iters))
    for r in res:
        print(json.dumps(r))
    if args.model:
        del xs
        torch.cuda.empty_cache()
        print(json.dumps(model_wall(args.model, dev)))


if __name__ == "__main__":
    main()
