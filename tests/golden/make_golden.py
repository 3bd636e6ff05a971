"""Generates tests/golden/golden_cases.npz and tests/golden/mnist_expected.npz.

    python tests/golden/make_golden.py
    python tests/golden/make_golden.py --workspace-bytes PATH/liblq_hip.so     # writes workspace_bytes.json only

The reference cannot run here (TensorFlow 2.11 not installed, no network) and ships no
golden vectors, so these fixtures are produced by the float32 restatement oracle/lq_oracle.py,
after tests/test_oracle.py has pinned that restatement against (a) the hand-derived KAT
kat_survey.json, (b) the float64 thesis-math restatement and (c) the scalar C restatement.
They are REGRESSION pins of the oracle and transport vectors to the GPU box (where
/root/reference does not exist); they are not reference outputs.

Cases: every (rank, orientation) pair incl. the degenerate ones of SURVEY 8a (channelwise on
rank 2 -> all-ones scale), edge cases (zeros, out == 0, lambda = 0, all-above, mostly-below,
NaN dy, negative zero), and the real MNIST baseline weights at several scales.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
from oracle import lq_oracle as O  # noqa: E402


def case(rng, shape, orientation, lam, s_lo, s_hi, p_std=0.05, dy_std=1e-3, tweak=None):
    P = rng.normal(0.0, p_std, size=shape).astype(np.float32)
    dy = rng.normal(0.0, dy_std, size=shape).astype(np.float32)
    sshape = O.scale_shape(shape, orientation)
    s = rng.uniform(s_lo, s_hi, size=sshape).astype(np.float32)
    if tweak:
        P, dy, s = tweak(P, dy, s)
    q, out = O.fq_forward(P, s)
    _, ds, im = O.nq_backward(P, s, lam, dy, return_intermediates=True)
    return dict(P=P, s=s, dy=dy, lam=np.float32(lam), q=q, out=out, ds=ds,
                maxq=im["maxvalue"], mean=im["mean"])


def main():
    rng = np.random.default_rng(42)
    cases = {}
    shapes = {"dense": (37, 20), "conv": (3, 3, 5, 7), "bias": (11,)}
    i = 0
    for name, shape in shapes.items():
        for orient in O.ORIENTATIONS:
            if len(shape) == 1 and orient != "scalar":
                continue   # bias scale is always scalar (custom_layers.py:225-227)
            for lam in (0.0, 1e-10, 5e-2):
                cases[f"c{i:02d}_{name}_{orient}_lam{lam:g}"] = case(rng, shape, orient, lam, 1e-3, 3e-2)
                i += 1
    # init-scale case: s = 100*eps everywhere, |q| ~ 2e4
    cases["init_scale_conv_channelwise"] = case(
        rng, (3, 3, 8, 16), "channelwise", 1e-11, 1, 1,
        tweak=lambda P, dy, s: (P, dy, np.full_like(s, O.SCALE_INIT)))

    def zeros(P, dy, s):
        P[...] = 0.0
        return P, dy, s
    cases["edge_all_zero_param"] = case(rng, (6, 9), "rowwise", 1e-3, 1e-2, 2e-2, tweak=zeros)

    def out_zero(P, dy, s):
        P = np.abs(P) * 1e-3       # 0 <= P < s  -> q = 0, out = 0 -> eps substitution (:63)
        return P.astype(np.float32), dy, s
    cases["edge_out_zero"] = case(rng, (6, 9), "columnwise", 1e-3, 1e-2, 2e-2, tweak=out_zero)

    def neg_zero(P, dy, s):
        P[0, :] = -0.0
        P[1, :] = -1e-9            # q = -1 -> out = -s (not zero)
        return P, dy, s
    cases["edge_negative_zero"] = case(rng, (4, 8), "rowwise", 1e-2, 1e-2, 2e-2, tweak=neg_zero)

    def all_above(P, dy, s):
        return P, (np.sign(dy) * (np.abs(dy) + 10.0)).astype(np.float32), s
    cases["edge_all_above"] = case(rng, (5, 12), "rowwise", 1e-3, 1e-2, 2e-2, tweak=all_above)

    def mostly_below(P, dy, s):
        return P, (dy * 1e-6).astype(np.float32), s
    cases["edge_mostly_below_big_lambda"] = case(rng, (5, 12), "columnwise", 0.7, 1e-2, 2e-2, tweak=mostly_below)

    def nan_dy(P, dy, s):
        dy[1, 3] = np.nan
        return P, dy, s
    cases["edge_nan_dy"] = case(rng, (4, 8), "rowwise", 1e-3, 1e-2, 2e-2, tweak=nan_dy)

    # activation-like: U[0,255) data, per-channel scales 0.5/1/2, tiny spatial extent
    def act(P, dy, s):
        P = rng.uniform(0, 255, size=P.shape).astype(np.float32)
        s = np.array([0.5, 1.0, 2.0], np.float32).reshape(1, 3, 1, 1)
        return P, dy, s
    c = case(rng, (4, 3, 8, 8), "columnwise", 1e-3, 1, 1, tweak=act)
    cases["bench_like_nchw_per_channel"] = c

    flat = {}
    for k, v in cases.items():
        for kk, vv in v.items():
            flat[f"{k}/{kk}"] = vv
    np.savez_compressed(os.path.join(HERE, "golden_cases.npz"), **flat)
    print("golden_cases.npz:", len(cases), "cases")

    # ---- real weights -------------------------------------------------------------------
    w = np.load(os.path.join(HERE, "mnist_baseline_weights.npz"))
    exp = {}
    meta = {}
    for name in ("W1", "b1", "W2", "b2"):
        P = w[name]
        for sval in (float(O.SCALE_INIT), 1e-3, 0.0123):
            q = O.quantized_integers(P, np.array([sval], np.float32)).astype(np.int32)
            key = f"{name}@{sval:.9g}"
            meta[key] = dict(sum=int(q.astype(np.int64).sum()), abssum=int(np.abs(q.astype(np.int64)).sum()),
                             min=int(q.min()), max=int(q.max()),
                             sha256=hashlib.sha256(np.ascontiguousarray(q).tobytes()).hexdigest())
            if sval == float(O.SCALE_INIT):
                exp[f"{name}_q_init"] = q.astype(np.int16) if np.abs(q).max() < 32768 else q
        if P.ndim == 2:
            for orient in ("rowwise", "columnwise"):
                sshape = O.scale_shape(P.shape, orient)
                s = (np.abs(P).max(axis=1 if orient == "rowwise" else 0).reshape(sshape) / 12.0 + 1e-6).astype(np.float32)
                q = O.quantized_integers(P, s).astype(np.int32)
                meta[f"{name}@{orient}_absmax12"] = dict(
                    sum=int(q.astype(np.int64).sum()), abssum=int(np.abs(q.astype(np.int64)).sum()),
                    min=int(q.min()), max=int(q.max()),
                    sha256=hashlib.sha256(np.ascontiguousarray(q).tobytes()).hexdigest())
    np.savez_compressed(os.path.join(HERE, "mnist_expected.npz"), **exp)
    with open(os.path.join(HERE, "mnist_expected.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("mnist_expected:", len(meta), "entries")


# ---- workspace contract ---------------------------------------------------------------
# lq_workspace_bytes / lq_conv_workspace_bytes are ABI: callers size buffers by them.  The pin is taken from a library built
# BEFORE a change to the host planning code and reproduced by the library under test (tests/test_host_cpu.py); both functions
# are pure host code, no device is needed.
WS_OUTER = (1, 2, 3, 31, 32, 33, 256, 4096, 100003)
WS_G = (1, 2, 3, 9, 10, 64, 65, 200, 256, 257, 320, 512, 1000, 1024, 4096)
WS_INNER = (1, 2, 3, 4, 5, 8, 15, 16, 17, 49, 64, 68, 100, 199, 200, 1023, 1024, 1025, 1225, 2047, 2048, 4100, 50176)
WS_CONV_CONFIGS = ("imagenette", "resnet50")      # the ResNet-18-like and ResNet-50-like sets of tools/bench_weights.py
WS_ORIENTATIONS = ("rowwise", "columnwise", "channelwise", "scalar")


def workspace_conv_cases():
    """[hw, ci, co, outer, G, inner] of every distinct conv kernel of the two sets, for the four orientations."""
    import torch
    import learned_quantization_amd as lq
    cases = []
    for config in WS_CONV_CONFIGS:
        lq.reset_layer_names()
        model = lq.build_model(config, mode="nq", value=(1e-10, 1e-11) if config == "resnet50" else 1e-11, seed=42,
                               orientation="rowwise", device=torch.device("cpu"))
        shapes = sorted({tuple(m.kernel.shape) for m in model.modules() if getattr(m, "kernel", None) is not None and m.kernel.dim() == 4})
        for kh, kw, ci, co in shapes:
            for orient in WS_ORIENTATIONS:
                outer, G, inner = lq.group_descriptor((kh, kw, ci, co), lq.scale_shape((kh, kw, ci, co), orient))
                c = [kh * kw, ci, co, outer, G, inner]
                if c not in cases:
                    cases.append(c)
    return cases


def workspace_bytes(lib_path):
    """The contract as `lib_path` answers it: {"grid": [...], "conv": [[hw, ci, co, outer, G, inner, bytes], ...]}."""
    import ctypes
    lib = ctypes.CDLL(lib_path)
    for fn, n in ((lib.lq_workspace_bytes, 3), (lib.lq_conv_workspace_bytes, 6)):
        fn.restype = ctypes.c_size_t
        fn.argtypes = [ctypes.c_int64] * n
    grid = [int(lib.lq_workspace_bytes(o, g, i)) for o in WS_OUTER for g in WS_G for i in WS_INNER]
    conv = [c + [int(lib.lq_conv_workspace_bytes(*c))] for c in workspace_conv_cases()]
    return {"grid": grid, "conv": conv}


def main_workspace(lib_path, commit):
    doc = {"header": "lq_workspace_bytes over outer x G x inner (outer-major, the WS_* tuples of make_golden.py) and "
                     "lq_conv_workspace_bytes of the conv kernels of the ResNet-18-like and ResNet-50-like sets; generated from a "
                     "library built at the PARENT commit " + commit + ", never from the library under test",
           "outer": list(WS_OUTER), "G": list(WS_G), "inner": list(WS_INNER)}
    doc.update(workspace_bytes(lib_path))
    with open(os.path.join(HERE, "workspace_bytes.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("workspace_bytes.json:", len(doc["grid"]), "descriptors,", len(set(doc["grid"])), "distinct values,", len(doc["conv"]), "conv cases")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--workspace-bytes":
        main_workspace(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else "(unnamed)")
    else:
        main()
