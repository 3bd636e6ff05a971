#!/usr/bin/env python3
"""The group batch next to what it replaces, interleaved in one process.

Sets: the group-wise weight sets (``bits=4, group_size=128``, rule "ste") of three models -- the CIFAR CNN (``cifar``), the
ResNet-18-like net (``imagenette``) and the ResNet-50-like net (``resnet50``): every conv / dense kernel with its group-wise scale
matrix and every bias with its scalar scale.

Yardstick: what the per-tensor path launches for the same tensors -- ``lq_fq_forward_group`` + ``lq_fq_backward_group`` per
kernel, ``lq_fq_forward_clip_r`` + ``lq_fq_backward_clip_r`` per bias -- as raw C-ABI calls, back to back, into preallocated
outputs.  The batch: ``lq_group_batch_forward`` (one launch) and ``lq_group_batch_backward`` (one launch) over the same tensors.

Protocol of tools/bench_groupwise.py: ``--sets`` rotating buffer sets (P, dy, out, dP of every tensor; a batch handle per set,
the scales shared), every round times each of the four variants once (an event-timed run of ``--inner`` back-to-back passes over
the whole weight set), the rounds interleave the variants, the figure is the median over the rounds in microseconds per pass.  The
whole comparison is repeated ``--repeats`` times in the process, so the yardstick's own run-to-run spread is visible.  One JSON
line per set and repeat.

``--asymmetric``: the same three weight sets with a learned offset per group on every kernel (the biases stay symmetric and
scalar, as in an asymmetric model).  Yardstick: ``lq_fq_forward_group_affine`` + ``lq_fq_backward_group_affine`` per kernel plus the
three launches per bias.  Candidate: the batch of ``lq_group_batch_create_affine`` (two launches).  A third pair of variants, timed in
the same rounds, is the SYMMETRIC batch over the same buffers (it ignores the offsets): what the offsets cost inside the batch.
Before anything is timed the tool asserts that out, dP, ds and db of the affine batch equal the per-tensor calls' bit for bit.

``--element-format F [--scale-format S]``: the same three weight sets as microscaling tensors at ``gs = 32`` (every kernel in blocks
of 32, every bias one block).  Yardstick: the per-tensor MX path, ``lq_fq_forward_mx`` + ``lq_fq_backward_mx`` per kernel AND per
bias (two launches each).  Candidate: the batch of ``lq_group_batch_create_mx`` (two launches).  A third pair of variants, timed in
the same rounds, is the INTEGER group batch (range [-8, 7], nearest, ``gs = 32``) over the same buffers: the denominator of what the
minifloat step costs inside the batch.  Before anything is timed the tool asserts that out, dP and ds of the MX batch equal the
per-tensor calls' bit for bit, biases included.

    python tools/bench_group_batch.py [--configs cifar imagenette resnet50] [--rounds 15] [--inner 10] [--sets 4] [--repeats 3] [--out FILE]
                                      [--asymmetric | --element-format F [--scale-format S]] [--rotate-variants]
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
from learned_quantization_amd.descriptor import group_geometry  # noqa: E402


def weight_set(config, bits, gs, dev):
    """[(kind, shape, strides, scale shape, q_range)] of every quantised tensor of the model, in the batch's order."""
    lq.reset_layer_names()
    model = lq.build_model(config, mode="ste", value=0.0, seed=1, device=dev, bits=bits, group_size=gs)
    out = []
    for layer in lq.custom_layers_of(model):
        for attr, pname in (("nested_q_w_layer", "W"), ("nested_q_k_layer", "kernel"), ("nested_q_b_layer", "b")):
            nested = getattr(layer, attr, None)
            if nested is None or (pname == "b" and not getattr(layer, "_has_bias", True)):
                continue
            p = getattr(layer, pname)
            out.append((nested.group_size, tuple(p.shape), tuple(p.data.stride()), tuple(nested.scale.shape), nested.q_range))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cifar", "imagenette", "resnet50"])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--group-size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--asymmetric", action="store_true", help="kernels with an offset per group: the affine batch against the affine per-tensor calls")
    ap.add_argument("--element-format", default=None, choices=list(ops.ELEMENT_FORMATS),
                    help="microscaling tensors at gs = 32: the MX batch against the per-tensor MX calls, and against the integer group batch")
    ap.add_argument("--scale-format", default="e8m0", choices=list(ops.SCALE_FORMATS))
    ap.add_argument("--rotate-variants", action="store_true",
                    help="round r starts with variant r mod n instead of the first one: every variant follows every other equally often, "
                         "which separates what a variant costs from what running after another one costs")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    mx = args.element_format is not None
    if mx and args.asymmetric:
        ap.error("--element-format with --asymmetric: the microscaling formats are symmetric")
    if mx:
        args.bits, args.group_size = 4, 32          # the integer batch of the comparison: [-8, 7], nearest, on the MX block size
        fid, sid = ops.ELEMENT_FORMATS[args.element_format].id, ops.SCALE_FORMATS.index(args.scale_format)
    rnd = 1 if mx else 0
    dev = torch.device("cuda:0")
    lib = _hip.load()
    sp = _hip.stream_ptr(dev)
    lines = []
    specs = {c: weight_set(c, args.bits, args.group_size, dev) for c in args.configs}
    for repeat in range(args.repeats):
        for config in args.configs:
            g = torch.Generator(device=dev).manual_seed(42 + repeat)
            tensors = []          # per tensor: geometry, range, scale, ds, counts, one-axis workspace
            for gs, shape, strides, sshape, (qmin, qmax) in specs[config]:
                numel = 1
                for d in shape:
                    numel *= d
                if gs is not None:
                    R, C, axis = group_geometry(shape, strides, sshape, gs)
                    geom = (R, C, axis, gs)
                else:
                    geom = (1, numel, 1, numel)
                s = torch.exp2(torch.empty(sshape, device=dev).uniform_(-9.0, -5.0, generator=g))
                affine = args.asymmetric and gs is not None
                tensors.append(dict(geom=geom, group=gs is not None, numel=numel, qmin=qmin, qmax=qmax, s=s, ds=torch.empty_like(s),
                                    b=torch.empty_like(s).uniform_(-6.0, 6.0, generator=g) * s if affine else None,
                                    db=torch.empty_like(s) if affine else None,
                                    cl=torch.empty_like(s, dtype=torch.int32),
                                    ws=None if gs is not None else _hip.workspace_for(dev, 1, 1, numel).clone()))
            n = len(tensors)
            sets, handles = [], []
            for _ in range(args.sets):
                bufs = []
                for t in tensors:
                    P = torch.empty(t["numel"], device=dev).normal_(generator=g) * (8.0 * 2.0 ** -7)
                    dy = torch.empty(t["numel"], device=dev).normal_(generator=g)
                    bufs.append((P, dy, torch.empty_like(P), torch.empty_like(P)))
                arr = (_hip.GroupDesc * n)(*[_hip.GroupDesc(P.data_ptr(), t["s"].data_ptr(), out.data_ptr(), dp.data_ptr(), t["ds"].data_ptr(),
                                                            t["geom"][0], t["geom"][1], t["geom"][3], t["geom"][2], t["qmin"], t["qmax"])
                                             for t, (P, dy, out, dp) in zip(tensors, bufs)])
                h, hs = ctypes.c_void_p(), ctypes.c_void_p()
                if mx:
                    fmts = (_hip.GroupMxFormat * n)(*[_hip.GroupMxFormat(fid, sid) for _ in tensors])
                    _hip.check(lib.lq_group_batch_create_mx(arr, fmts, n, ctypes.byref(h)), "lq_group_batch_create_mx")
                    _hip.check(lib.lq_group_batch_create(arr, n, rnd, ctypes.byref(hs)), "lq_group_batch_create")
                elif args.asymmetric:
                    offs = (_hip.GroupOffset * n)(*[_hip.GroupOffset(_hip.ptr(t["b"]), _hip.ptr(t["db"]), 1.0) for t in tensors])
                    _hip.check(lib.lq_group_batch_create_affine(arr, offs, n, 0, ctypes.byref(h)), "lq_group_batch_create_affine")
                    _hip.check(lib.lq_group_batch_create(arr, n, 0, ctypes.byref(hs)), "lq_group_batch_create")
                else:
                    _hip.check(lib.lq_group_batch_create(arr, n, 0, ctypes.byref(h)), "lq_group_batch_create")
                dys = (ctypes.c_void_p * n)(*[dy.data_ptr() for _, dy, _, _ in bufs])
                sets.append(bufs)
                handles.append((h, dys, hs))
            ks = (ctypes.c_float * n)(*([1.0] * n))
            need = lib.lq_group_batch_workspace_bytes(handles[0][0])
            bws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

            def fwd_per_tensor(k):
                rc = 0
                for t, (P, dy, out, dp) in zip(tensors, sets[k]):
                    R, C, axis, gs = t["geom"]
                    if mx:
                        rc |= lib.lq_fq_forward_mx(P.data_ptr(), t["s"].data_ptr(), out.data_ptr(), None, _hip.LQ_Q_NONE, fid, sid, R, C, axis, gs, sp)
                    elif t["b"] is not None:
                        rc |= lib.lq_fq_forward_group_affine(P.data_ptr(), t["s"].data_ptr(), t["b"].data_ptr(), out.data_ptr(), None,
                                                             _hip.LQ_Q_NONE, t["qmin"], t["qmax"], 0, R, C, axis, gs, sp)
                    elif t["group"]:
                        rc |= lib.lq_fq_forward_group(P.data_ptr(), t["s"].data_ptr(), out.data_ptr(), None, _hip.LQ_Q_NONE, t["qmin"], t["qmax"], 0,
                                                R, C, axis, gs, sp)
                    else:
                        rc |= lib.lq_fq_forward_clip_r(P.data_ptr(), t["s"].data_ptr(), out.data_ptr(), None, _hip.LQ_Q_NONE, t["qmin"], t["qmax"], 0,
                                                 1, 1, C, sp)
                return rc

            def bwd_per_tensor(k):
                rc = 0
                for t, (P, dy, out, dp) in zip(tensors, sets[k]):
                    R, C, axis, gs = t["geom"]
                    if mx:
                        rc |= lib.lq_fq_backward_mx(P.data_ptr(), t["s"].data_ptr(), dy.data_ptr(), fid, sid, 1.0, dp.data_ptr(), t["ds"].data_ptr(),
                                                    t["cl"].data_ptr(), R, C, axis, gs, sp)
                    elif t["b"] is not None:
                        rc |= lib.lq_fq_backward_group_affine(P.data_ptr(), t["s"].data_ptr(), t["b"].data_ptr(), dy.data_ptr(), t["qmin"],
                                                              t["qmax"], 0, 1.0, 1.0, dp.data_ptr(), t["ds"].data_ptr(), t["db"].data_ptr(),
                                                              t["cl"].data_ptr(), None, 0, R, C, axis, gs, sp)
                    elif t["group"]:
                        rc |= lib.lq_fq_backward_group(P.data_ptr(), t["s"].data_ptr(), dy.data_ptr(), t["qmin"], t["qmax"], 0, 1.0, dp.data_ptr(),
                                                 t["ds"].data_ptr(), t["cl"].data_ptr(), None, 0, R, C, axis, gs, sp)
                    else:
                        rc |= lib.lq_fq_backward_clip_r(P.data_ptr(), t["s"].data_ptr(), dy.data_ptr(), t["qmin"], t["qmax"], 0, 1.0, dp.data_ptr(),
                                                  t["ds"].data_ptr(), t["cl"].data_ptr(), t["ws"].data_ptr(), t["ws"].numel(), 1, 1, C, sp)
                return rc

            def fwd_batch(k):
                return lib.lq_group_batch_forward(handles[k][0], sp)

            def bwd_batch(k):
                return lib.lq_group_batch_backward(handles[k][0], handles[k][1], ks, bws.data_ptr() if need else None, need, sp)

            variants = {"forward_per_tensor": fwd_per_tensor, "forward_batch": fwd_batch, "backward_per_tensor": bwd_per_tensor,
                        "backward_batch": bwd_batch}
            if mx:
                variants["forward_integer_batch"] = lambda k: lib.lq_group_batch_forward(handles[k][2], sp)
                variants["backward_integer_batch"] = lambda k: lib.lq_group_batch_backward(handles[k][2], handles[k][1], ks, None, 0, sp)
            if args.asymmetric:
                variants["forward_symmetric_batch"] = lambda k: lib.lq_group_batch_forward(handles[k][2], sp)
                variants["backward_symmetric_batch"] = lambda k: lib.lq_group_batch_backward(handles[k][2], handles[k][1], ks, None, 0, sp)

            def outputs():
                torch.cuda.synchronize(dev)
                return ([(out.clone(), dp.clone()) for _, _, out, dp in sets[0]], [t["ds"].clone() for t in tensors],
                        [t["db"].clone() for t in tensors if t["db"] is not None])

            if mx:                   # before anything is timed: the candidate computes what the yardstick computes, bit for bit
                _hip.check(fwd_per_tensor(0) | bwd_per_tensor(0), "per-tensor pass")
                w_out, w_ds, _ = outputs()
                for t in tensors:
                    t["ds"].fill_(float("nan"))
                _hip.check(fwd_batch(0) | bwd_batch(0), "batch pass")
                g_out, g_ds, _ = outputs()
                assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(g_out, w_out)), "out / dP differ"
                assert all(torch.equal(a, b) and not bool(torch.isnan(a).any()) for a, b in zip(g_ds, w_ds)), "ds of a tensor differs"
                assert all(bool((dp != 0).any()) for _, dp in g_out), "a tensor saturates everywhere"
                assert all(bool((dp == 0).any()) for (_, dp), t in zip(g_out, tensors) if t["group"]), "a kernel saturates nowhere"
            if args.asymmetric:      # before anything is timed: the candidate computes what the yardstick computes, bit for bit
                _hip.check(fwd_per_tensor(0) | bwd_per_tensor(0), "per-tensor pass")
                w_out, w_ds, w_db = outputs()
                for t in tensors:
                    t["ds"].fill_(float("nan"))
                    if t["db"] is not None:
                        t["db"].fill_(float("nan"))
                _hip.check(fwd_batch(0) | bwd_batch(0), "batch pass")
                g_out, g_ds, g_db = outputs()
                assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(g_out, w_out)), "out / dP differ"
                assert all(torch.equal(a, b) for a, b, t in zip(g_ds, w_ds, tensors) if t["group"]), "ds of a kernel differs"
                assert len(g_db) == sum(t["group"] for t in tensors) and all(torch.equal(a, b) for a, b in zip(g_db, w_db)), "db differs"
                assert all(bool((d != 0).any()) for d in g_db), "an offset gradient is zero everywhere: nothing clips"
            times = {k: [] for k in variants}
            for key, fn in variants.items():
                for k in range(args.sets):
                    _hip.check(fn(k), key)
            torch.cuda.synchronize(dev)
            k_set = 0
            for rnd_no in range(args.rounds):
                order = list(variants.items())
                if args.rotate_variants:
                    order = order[rnd_no % len(order):] + order[:rnd_no % len(order)]
                for key, fn in order:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.inner):
                        fn(k_set % args.sets)
                        k_set += 1
                    b.record()
                    torch.cuda.synchronize(dev)
                    times[key].append(a.elapsed_time(b) / args.inner * 1e3)
            # the two paths must have computed the same thing on the last set they both touched
            fwd_per_tensor(0), bwd_per_tensor(0)
            torch.cuda.synchronize(dev)
            want = [(out.clone(), dp.clone()) for _, _, out, dp in sets[0]]
            want_ds = [t["ds"].clone() for t in tensors]
            fwd_batch(0), bwd_batch(0)
            torch.cuda.synchronize(dev)
            same = all(torch.equal(o, wo) and torch.equal(d, wd) for (_, _, o, d), (wo, wd) in zip(sets[0], want))
            same_ds = all(torch.equal(t["ds"], w) for t, w in zip(tensors, want_ds) if t["group"] or mx)
            row = {"set": config, "tensors": n, "kernels": sum(t["group"] for t in tensors), "elements": sum(t["numel"] for t in tensors),
                   "bits": args.bits, "group_size": args.group_size, "repeat": repeat, "rounds": args.rounds, "inner": args.inner,
                   "buffer_sets": args.sets, "launches_per_tensor_path": sum(2 if t["group"] or mx else 3 for t in tensors),
                   "launches_batch": 2, "out_dp_bit_identical": bool(same), "kernel_ds_bit_identical": bool(same_ds)}
            if args.rotate_variants:
                row["rotate_variants"] = True
            if mx:
                row.update({"element_format": args.element_format, "scale_format": args.scale_format,
                            "ds_bit_identical_before_timing_biases_included": True})      # asserted above
            if args.asymmetric:
                row["asymmetric"] = True
                row["kernel_ds_db_bit_identical_before_timing"] = True      # asserted above
            for key in variants:
                row[f"us_{key}"] = statistics.median(times[key])
                row[f"us_{key}_min_max"] = [min(times[key]), max(times[key])]
            row["us_sum_per_tensor"] = row["us_forward_per_tensor"] + row["us_backward_per_tensor"]
            row["us_sum_batch"] = row["us_forward_batch"] + row["us_backward_batch"]
            row["batch_over_per_tensor"] = row["us_sum_batch"] / row["us_sum_per_tensor"]
            if mx:
                row["us_sum_integer_batch"] = row["us_forward_integer_batch"] + row["us_backward_integer_batch"]
                row["mx_batch_over_integer_batch"] = row["us_sum_batch"] / row["us_sum_integer_batch"]
                row["per_tensor_over_batch"] = row["us_sum_per_tensor"] / row["us_sum_batch"]
            if args.asymmetric:
                row["us_sum_symmetric_batch"] = row["us_forward_symmetric_batch"] + row["us_backward_symmetric_batch"]
                row["affine_batch_over_symmetric_batch"] = row["us_sum_batch"] / row["us_sum_symmetric_batch"]
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
            for h, _, hs in handles:
                lib.lq_group_batch_destroy(h)
                if hs:
                    lib.lq_group_batch_destroy(hs)
            del sets, handles, tensors
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
