#!/usr/bin/env python3
"""Times the batched penalty entry points with device events on the ResNet-18-like and ResNet-50-like weight sets:

    parent_grads_a / parent_grads_b   lq_batch_penalty_grads of ANOTHER build of the library (``--parent-lib``: the parent
                                      commit's liblq_hip.so), measured twice in the same alternation -- their difference is
                                      the spread of the method
    grads                             lq_batch_penalty_grads of the shipped library
    grads_values                      lq_batch_penalty_grads_values
    values                            lq_batch_penalty_values

The variants alternate inside one process, launch by launch; buffer sets (model copies) rotate as in tools/bench_pack.py;
warm-up, then the median of ``--iters`` event pairs per variant; the order of the variants rotates from one iteration to
the next (the first launch on a new buffer set runs cold).  One JSON line per (model, kind).

    python3 tools/bench_penalty.py [--parent-lib path/to/parent/liblq_hip.so] [--iters 50] [--sets 4] [--orientation channelwise]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import learned_quantization_amd as lq  # noqa: E402
from learned_quantization_amd import _hip  # noqa: E402

KINDS = {"maxbin": 0, "difference": 1, "inverse": 2}


def bind(path):
    """Another build of the same C ABI next to the shipped one (only the entry points it exports are bound)."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in _hip.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = restype
            fn.argtypes = argtypes
    return lib


def descriptors(batch):
    n = len(batch.entries)
    arr = (_hip.TensorDesc * n)()
    for i, e in enumerate(batch.entries):
        arr[i] = _hip.TensorDesc(e.param.data_ptr(), e.nested.scale.data_ptr(), None, _hip.ptr(e.out), e.ds.data_ptr(),
                                 e.m.data_ptr(), e.v.data_ptr(), e.desc[0], e.desc[1], e.desc[2], float("nan"), float("-inf"),
                                 None, None, 0, 0, 0)
    return arr


class Set:
    """One buffer set: a model, its batch in the shipped library and -- ``parent`` -- the same batch in the other build."""

    def __init__(self, config, orientation, dev, seed, parent):
        lq.reset_layer_names()
        self.model = lq.build_model(config, mode="cl", value=1e-7, seed=seed, orientation=orientation, device=dev)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for s in lq.scale_parameters(self.model):
                s.copy_((torch.rand(s.shape, generator=g) * (1.0 - 1e-3) + 1e-3).to(dev))
        self.batch = lq.FakeQuantBatch(self.model)
        n = len(self.batch.entries)
        total = float(sum(e.param.numel() for e in self.batch.entries))
        self.coeff = (ctypes.c_float * n)(*[1e-7 * e.param.numel() / total for e in self.batch.entries])
        self.grad_t = [torch.zeros_like(e.param.data) for e in self.batch.entries]
        self.grads = (ctypes.c_void_p * n)(*[g.data_ptr() for g in self.grad_t])
        self.dims, self.start, self.terms, self.penalty = self.batch._value_buffers()
        self.parent = parent
        self.parent_handle = None
        if parent is not None:
            h = ctypes.c_void_p()
            self._descs = descriptors(self.batch)
            _hip.check(parent.lq_batch_create(self._descs, n, ctypes.byref(h)), "parent lq_batch_create")
            self.parent_handle = h
            self.parent_ws = torch.empty(parent.lq_batch_workspace_bytes(h), dtype=torch.uint8, device=dev)

    def close(self):
        if self.parent_handle is not None:
            self.parent.lq_batch_destroy(self.parent_handle)
            self.parent_handle = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblq_hip.so of the commit to compare lq_batch_penalty_grads with")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--orientation", default="channelwise")
    ap.add_argument("--models", default="imagenette,resnet50")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    parent = bind(args.parent_lib) if args.parent_lib else None
    stream = _hip.stream_ptr(dev)
    st = torch.cuda.current_stream()
    for config in args.models.split(","):
        sets = [Set(config, args.orientation, dev, 40 + k, parent) for k in range(max(1, args.sets))]
        numel = sum(e.param.numel() for e in sets[0].batch.entries)
        for kind, kid in KINDS.items():
            def grads(s, which=lib, handle=None, ws=None):
                b = s.batch
                rc = which.lq_batch_penalty_grads(handle or b._handle, kid, s.coeff, s.grads, _hip.ptr(ws if ws is not None else b.ws),
                                                  (ws if ws is not None else b.ws).numel(), stream)
                assert rc == 0, rc

            def grads_values(s):
                b = s.batch
                rc = lib.lq_batch_penalty_grads_values(b._handle, kid, s.coeff, s.grads, s.dims, s.start, s.terms.data_ptr(),
                                                       s.penalty.data_ptr(), _hip.ptr(b.ws), b.ws.numel(), stream)
                assert rc == 0, rc

            def values(s):
                b = s.batch
                rc = lib.lq_batch_penalty_values(b._handle, kid, s.dims, s.start, s.terms.data_ptr(), s.penalty.data_ptr(),
                                                 _hip.ptr(b.ws), b.ws.numel(), stream)
                assert rc == 0, rc

            variants = []
            if parent is not None:
                variants.append(("parent_grads_a", lambda s: grads(s, parent, s.parent_handle, s.parent_ws)))
            variants += [("grads", grads), ("grads_values", grads_values), ("values", values)]
            if parent is not None:
                variants.append(("parent_grads_b", lambda s: grads(s, parent, s.parent_handle, s.parent_ws)))
            times = {name: [] for name, _ in variants}
            events = []
            for k in range(args.warmup + args.iters):
                s = sets[k % len(sets)]
                # the first launch after a change of buffer set finds nothing of it in the caches (10-16 us on these sets): the
                # order of the variants rotates, so that every variant takes every position equally often
                r = k % len(variants)
                for name, fn in variants[r:] + variants[:r]:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(st)
                    fn(s)
                    b.record(st)
                    if k >= args.warmup:
                        events.append((name, a, b))
            torch.cuda.synchronize()
            for name, a, b in events:
                times[name].append(a.elapsed_time(b) * 1e3)
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            row = {"model": config, "orientation": args.orientation, "kind": kind, "tensors": len(sets[0].batch.entries),
                   "elements": numel, "sets": len(sets), "iters": args.iters,
                   **{f"{name}_us": round(v, 2) for name, v in med.items()},
                   **{f"{name}_us_min": round(min(times[name]), 2) for name in med},
                   "values_minus_grads_us": round(med["grads_values"] - med["grads"], 2)}
            if parent is not None:
                row["parent_spread_us"] = round(abs(med["parent_grads_a"] - med["parent_grads_b"]), 2)
                row["grads_minus_parent_us"] = round(med["grads"] - 0.5 * (med["parent_grads_a"] + med["parent_grads_b"]), 2)
            print(json.dumps(row), flush=True)
        for s in sets:
            s.close()
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
