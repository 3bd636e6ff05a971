#!/usr/bin/env python3
"""The group-wise entry points of this build next to the parent commit's, output byte by output byte (profiles/group_unify).

    python3 tools/group_parent_bits.py --parent-lib PARENT/liblq_hip.so [--out FILE]
    python3 tools/group_parent_bits.py --check-cases          # CPU only: the NumPy reference's view of the cases

``--parent-lib`` names a liblq_hip.so built from the parent commit; it is loaded next to this build's (as
tools/bench_group_affine.py does) and both are bound with this build's prototypes.  The cases are tests/_group_forms.py::FORM_CASES
without LARGE, built with _group_reference.make_case, each once with the dense bases (P, dy, out / dP) on the 16-byte grid and once
one float off it.  Both libraries run on the same inputs; every output is poisoned before the call and compared as raw bytes, so NaN
payloads and bytes a call does not write count as well:

  forward   out and q (int8), floor and nearest: symmetric, and affine with a non-zero offset
  backward  dP, ds, db and the clip counts, floor and nearest, and with ds / db / clipped NULL in turn
  batch     lq_group_batch forward and backward (with and without grad_scale) over the same tensors as one batch
  init      lq_scale_init_group with its three methods and lq_scale_init_group_minmax, and both again with a NaN in one group and
            an Inf in another

One line per call family with the bytes compared and the bytes that differ; exit status 1 unless every count is 0.
``--check-cases`` asserts on the reference that every backward case, symmetric and affine, holds a clipped and an unclipped element,
so that ds, db and the counts are not trivially zero."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _group_forms import FORM_CASES, LARGE              # noqa: E402
from _group_reference import expand_scale, group_reference, make_case  # noqa: E402

CASES = [c for c in FORM_CASES if c != LARGE]
QMIN, QMAX = -8, 7
K, KB = 0.75, 1.25
MIN_VALUE = 2.0 ** -14
ROUNDINGS = (("floor", 0), ("nearest", 1))


def inputs(i, case):
    """(P, s, b, dy) of case i as float32 arrays; b = U(-6, 6) * s, never zero."""
    R, C, axis, gs = case
    P, s, dy = make_case(1000 + i, R, C, axis, gs)
    b = (np.random.default_rng(2000 + i).uniform(-6.0, 6.0, size=s.shape).astype(np.float32) * s).astype(np.float32)
    assert np.all(b != 0)
    return P, s, b, dy


def check_cases():
    for i, case in enumerate(CASES):
        R, C, axis, gs = case
        P, s, b, dy = inputs(i, case)
        for name, rounding in (("floor", "floor"), ("nearest", "nearest")):
            for what, data in (("symmetric", P), ("affine", P - expand_scale(b, R, C, axis, gs))):
                ref = group_reference(data, s, dy, QMIN, QMAX, axis, gs, K, rounding)
                clipped, inside = int(ref["clipped"].sum()), int(ref["inside"].sum())
                assert clipped > 0 and inside > 0, (case, name, what, clipped, inside)
                assert np.any(ref["ds"] != 0), (case, name, what)
        print(f"{case}: clipped and unclipped elements in all four variants")
    print(f"{len(CASES)} cases ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--check-cases", action="store_true")
    ap.add_argument("--out", default=None, help="write the report to this file as well")
    args = ap.parse_args()
    if args.check_cases:
        check_cases()
        return 0
    if not args.parent_lib:
        ap.error("--parent-lib is required")

    import torch
    from learned_quantization_amd import _hip

    def bind(path):
        lib = ctypes.CDLL(os.path.abspath(path))
        for name, (restype, argtypes) in _hip.SIGNATURES.items():
            if name.startswith(("lq_fq_forward_group", "lq_fq_backward_group", "lq_scale_init_group", "lq_group_batch_", "lq_last_error")):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
        return lib

    libs = {"parent": bind(args.parent_lib), "this": bind(_hip.LIB_PATH)}
    dev = torch.device("cuda:0")
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr

    def ok(lib, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} returned {rc}: {lib.lq_last_error().decode()}")

    def dense(a, shift):
        """``a`` on the device with its base ``shift`` floats past a 16-byte boundary."""
        flat = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
        assert flat.data_ptr() % 16 == 0
        view = flat[shift:shift + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        return view

    def poison(like, shift=0, dtype=torch.float32):
        n = like.numel()
        flat = torch.empty(n + 4, dtype=dtype, device=dev)
        flat.view(torch.uint8).fill_(0xA5)
        return flat[shift:shift + n].view(like.shape)

    def raw(t):
        return None if t is None else t.contiguous().view(torch.uint8).cpu().numpy().tobytes()

    report, total_diff = [], [0]

    def compare(what, got):
        """got: {"parent": [tensors], "this": [tensors]}"""
        a, b = [raw(t) for t in got["parent"]], [raw(t) for t in got["this"]]
        assert len(a) == len(b)
        n = sum(len(x) for x in a if x is not None)
        d = sum(int(np.count_nonzero(np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8))) for x, y in zip(a, b) if x is not None)
        total_diff[0] += d
        report.append(f"{what:58s} bytes compared {n:10d}  differing {d}")
        print(report[-1], flush=True)

    tensors = []
    for shift in (0, 1):
        tag = "aligned" if shift == 0 else "one float off"
        per = {k: {"parent": [], "this": []} for k in ("forward", "forward affine", "backward", "backward affine", "init", "init NaN / Inf")}
        for i, case in enumerate(CASES):
            R, C, axis, gs = case
            Ph, sh, bh, dyh = inputs(i, case)
            P, dy = dense(Ph, shift), dense(dyh, shift)
            s, b = torch.from_numpy(sh).to(dev), torch.from_numpy(bh).to(dev)
            Pbad = Ph.copy()
            Pbad[0, 0], Pbad[R - 1, C - 1] = np.nan, np.inf
            Pbad = dense(Pbad, shift)
            tensors.append((case, P, s, dy, shift))
            for name, lib in libs.items():
                for rname, r in ROUNDINGS:
                    out, q = poison(P, shift), poison(P, 0, torch.int8)
                    ok(lib, lib.lq_fq_forward_group(ptr(P), ptr(s), ptr(out), ptr(q), _hip.LQ_Q_I8, QMIN, QMAX, r, R, C, axis, gs, sp), "forward")
                    per["forward"][name] += [out, q]
                    out, q = poison(P, shift), poison(P, 0, torch.int8)
                    ok(lib, lib.lq_fq_forward_group_affine(ptr(P), ptr(s), ptr(b), ptr(out), ptr(q), _hip.LQ_Q_I8, QMIN, QMAX, r, R, C, axis,
                                                           gs, sp), "forward affine")
                    per["forward affine"][name] += [out, q]
                    for drop in (None, "ds", "db", "clipped"):
                        dP, ds, cl = poison(P, shift), poison(s), poison(s, 0, torch.int32)
                        if drop != "db":      # the symmetric pair has no db
                            ok(lib, lib.lq_fq_backward_group(ptr(P), ptr(s), ptr(dy), QMIN, QMAX, r, K, ptr(dP), None if drop == "ds" else ptr(ds),
                                                             None if drop == "clipped" else ptr(cl), None, 0, R, C, axis, gs, sp), "backward")
                            per["backward"][name] += [dP, ds, cl]
                        dP, ds, db, cl = poison(P, shift), poison(s), poison(s), poison(s, 0, torch.int32)
                        ok(lib, lib.lq_fq_backward_group_affine(ptr(P), ptr(s), ptr(b), ptr(dy), QMIN, QMAX, r, K, KB, ptr(dP),
                                                                None if drop == "ds" else ptr(ds), None if drop == "db" else ptr(db),
                                                                None if drop == "clipped" else ptr(cl), None, 0, R, C, axis, gs, sp),
                           "backward affine")
                        per["backward affine"][name] += [dP, ds, db, cl]
                for key, src in (("init", P), ("init NaN / Inf", Pbad)):
                    for method, r in ((0, 0), (1, 0), (2, 0), (2, 1)):
                        s_out = poison(s)
                        ok(lib, lib.lq_scale_init_group(ptr(src), ptr(s_out), QMIN, QMAX, r, method, MIN_VALUE, R, C, axis, gs, sp), "init")
                        per[key][name].append(s_out)
                    for rname, r in ROUNDINGS:
                        s_out, b_out = poison(s), poison(s)
                        ok(lib, lib.lq_scale_init_group_minmax(ptr(src), ptr(s_out), ptr(b_out), QMIN, QMAX, r, MIN_VALUE, R, C, axis, gs, sp),
                           "min-max")
                        per[key][name] += [s_out, b_out]
        torch.cuda.synchronize(dev)
        for key, got in per.items():
            compare(f"{key}, {len(CASES)} cases, {tag}", got)

    # the same tensors (both alignments) as one lq_group_batch
    n = len(tensors)
    for rname, r in ROUNDINGS:
        got = {k: {"parent": [], "this": []} for k in ("batch forward", "batch backward", "batch backward, mask only")}
        for name, lib in libs.items():
            descs = (_hip.GroupDesc * n)()
            outs, dps, dss = [], [], []
            for j, (case, P, s, dy, shift) in enumerate(tensors):
                R, C, axis, gs = case
                outs.append(poison(P, shift))
                dps.append(poison(P, shift))
                dss.append(poison(s))
                descs[j] = _hip.GroupDesc(ptr(P), ptr(s), ptr(outs[j]), ptr(dps[j]), ptr(dss[j]), R, C, gs, axis, QMIN, QMAX)
            handle = ctypes.c_void_p()
            ok(lib, lib.lq_group_batch_create(descs, n, r, ctypes.byref(handle)), "batch create")
            ok(lib, lib.lq_group_batch_forward(handle, sp), "batch forward")
            got["batch forward"][name] += outs
            dys = (ctypes.c_void_p * n)(*[ptr(t[3]) for t in tensors])
            scales = (ctypes.c_float * n)(*[K + 0.01 * j for j in range(n)])

            def counts():
                """Copies of the batch's clip counts: the memory belongs to the handle, so clone before lq_group_batch_destroy.
                (uint32 counts viewed as int32: only their bytes are compared.)"""
                res = []
                for j in range(n):
                    d, g = ctypes.c_void_p(), ctypes.c_int64()
                    ok(lib, lib.lq_group_batch_clip_counts(handle, j, ctypes.byref(d), ctypes.byref(g)), "clip counts")
                    iface = type("W", (), {"__cuda_array_interface__": {"shape": (g.value,), "typestr": "<i4", "data": (d.value, False),
                                                                         "version": 2}})()
                    res.append(torch.as_tensor(iface, device=dev).clone())
                return res

            ok(lib, lib.lq_group_batch_backward(handle, dys, scales, None, 0, sp), "batch backward")
            got["batch backward"][name] += [t.clone() for t in dps] + [t.clone() for t in dss] + counts()
            for t in dps:      # the mask-only pass writes dP and the counts; ds is neither written nor compared there
                t.view(torch.uint8).fill_(0xA5)
            ok(lib, lib.lq_group_batch_backward(handle, dys, None, None, 0, sp), "batch backward, mask only")
            got["batch backward, mask only"][name] += [t.clone() for t in dps] + counts()
            torch.cuda.synchronize(dev)
            ok(lib, lib.lq_group_batch_destroy(handle), "batch destroy")
        for key, g in got.items():
            compare(f"{key}, {n} tensors, {rname}", g)

    report.append(f"total differing bytes: {total_diff[0]}")
    print(report[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")
    return 0 if total_diff[0] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
