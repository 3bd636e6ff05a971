#!/usr/bin/env python3
"""The statistics entry points of this build next to the parent commit's, output byte by output byte (profiles/stats_unify).

    python3 tools/stats_parent_bits.py --parent-lib PARENT/liblq_hip.so [--out FILE]

``--parent-lib`` names a liblq_hip.so built from the parent commit; it is loaded next to this build's (as
tools/group_parent_bits.py does) and both are bound with this build's prototypes.  The geometries are the smallest that reach each
launch form (tests/_mx_stats_reference.py: FORM_GEOMETRIES and BIAS), each once with P on the 16-byte grid and once one float off
it.  The inputs are the tests' (_group_reference.make_case / _group_affine_reference.make_affine_case with the seed of
tests/test_gpu_group_stats.py, _mx_stats_reference.case): tests/test_group_stats_cpu.py and tests/test_mx_stats_cpu.py assert on
the reference that they hold clipped, saturated, flushed and subnormal elements.  Both libraries run on the same inputs; every
output is poisoned before the call (the histogram zeroed: the call adds to it) and compared as raw bytes:

  lq_group_stats  floor and nearest, without and with an offset, with and without the histogram: below, above, err2, sig2, hist
  lq_mx_stats     every element format under both scale formats, with and without the histogram: the same and flushed

One line per call family with the bytes compared and the bytes that differ; exit status 1 unless every count is 0 (the f64 sums
have one fixed order)."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mx_stats_reference as M                         # noqa: E402
from _group_affine_reference import make_affine_case    # noqa: E402
from _group_reference import make_case                  # noqa: E402

GEOMETRIES = M.FORM_GEOMETRIES + [M.BIAS]
SEED = 20
QMIN, QMAX = -8, 7
ROUNDINGS = (("floor", 0), ("nearest", 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=None, help="write the report to this file as well")
    args = ap.parse_args()

    import torch
    from learned_quantization_amd import _hip, ops

    def bind(path):
        lib = ctypes.CDLL(os.path.abspath(path))
        for name in ("lq_group_stats", "lq_mx_stats", "lq_last_error"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _hip.SIGNATURES[name]
        return lib

    libs = {"parent": bind(args.parent_lib), "this": bind(_hip.LIB_PATH)}
    dev = torch.device("cuda:0")
    sp = _hip.stream_ptr(dev)
    ptr = _hip.ptr

    def dense(a, shift):
        """``a`` on the device with its base ``shift`` floats past a 16-byte boundary."""
        flat = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
        assert flat.data_ptr() % 16 == 0
        view = flat[shift:shift + a.size].view(a.shape)
        view.copy_(torch.from_numpy(np.array(a)))
        return view

    def poison(like, dtype):
        t = torch.empty(like.shape, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(0xA5)
        return t

    report, total_diff = [], [0]

    def compare(what, got):
        a, b = [[t.view(torch.uint8).cpu().numpy() for t in got[k]] for k in ("parent", "this")]
        assert len(a) == len(b) and len(a) > 0
        n = sum(x.size for x in a)
        d = sum(int(np.count_nonzero(x != y)) for x, y in zip(a, b))
        total_diff[0] += d
        report.append(f"{what:62s} bytes compared {n:9d}  differing {d}")
        print(report[-1], flush=True)

    def run(lib, what, call, s, nbins, flushed):
        """The outputs of one call: below, above, (flushed,) err2, sig2, (hist)."""
        out = [poison(s, torch.int32), poison(s, torch.int32)] + ([poison(s, torch.int32)] if flushed else [])
        out += [poison(s, torch.float64), poison(s, torch.float64)]
        hist = torch.zeros(nbins, dtype=torch.int32, device=dev) if nbins else None
        rc = call(lib, *[ptr(t) for t in out], None if hist is None else ptr(hist))
        if rc != 0:
            raise RuntimeError(f"{what} returned {rc}: {lib.lq_last_error().decode()}")
        return out + ([] if hist is None else [hist])

    for shift in (0, 1):
        tag = "aligned" if shift == 0 else "one float off"
        for affine in (False, True):
            for rname, r in ROUNDINGS:
                for nbins in (QMAX - QMIN + 1, 0):
                    got = {"parent": [], "this": []}
                    for R, C, axis, gs in GEOMETRIES:
                        Ph, sh, bh = make_affine_case(SEED, R, C, axis, gs)[:3] if affine else (*make_case(SEED, R, C, axis, gs)[:2], None)
                        P, s = dense(Ph, shift), torch.from_numpy(np.array(sh)).to(dev)
                        b = None if bh is None else torch.from_numpy(np.array(bh)).to(dev)
                        for name, lib in libs.items():
                            got[name] += run(lib, "lq_group_stats", lambda lib, below, above, err2, sig2, hist: lib.lq_group_stats(
                                ptr(P), ptr(s), None if b is None else ptr(b), QMIN, QMAX, r, below, above, err2, sig2, hist, R, C, axis, gs,
                                sp), s, nbins, False)
                    torch.cuda.synchronize(dev)
                    compare(f"group {'affine ' if affine else ''}{rname}, {'hist' if nbins else 'no hist'}, {len(GEOMETRIES)} shapes, {tag}", got)
        for fname in M.FORMATS:
            fmt = ops.check_element_format(fname)
            for sfname in M.SCALE_FORMATS:
                sf = ops.check_scale_format(sfname)
                for nbins in (1 << fmt.bits, 0):
                    got = {"parent": [], "this": []}
                    for geo in GEOMETRIES:
                        R, C, axis, gs = geo
                        Ph, sh = M.case(fname, sfname, geo)
                        P, s = dense(Ph, shift), torch.from_numpy(np.array(sh)).to(dev)
                        for name, lib in libs.items():
                            got[name] += run(lib, "lq_mx_stats", lambda lib, below, above, flushed, err2, sig2, hist: lib.lq_mx_stats(
                                ptr(P), ptr(s), fmt.id, sf, below, above, flushed, err2, sig2, hist, R, C, axis, gs, sp), s, nbins, True)
                    torch.cuda.synchronize(dev)
                    compare(f"mx {fname} {sfname}, {'hist' if nbins else 'no hist'}, {len(GEOMETRIES)} shapes, {tag}", got)

    report.append(f"total differing bytes: {total_diff[0]}")
    print(report[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(report) + "\n")
    return 0 if total_diff[0] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
