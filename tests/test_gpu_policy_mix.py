"""Cache-policy mix of the two streaming kernels of one tensor ("Cache-policy mix"): some blocks of
k_flat_fwd<OP_FWD, 512, nt, 0> (K1) and some units of k_row_stream<OP_BWD, 4, 512, 1, 2, TAIL> (K2) load with the default cache
policy, the others nontemporally, in two arms of a block-uniform branch.  The policy must change no bit: every descriptor here
holds blocks of both kinds in both kernels at the shipped constants (kMixK1: 3 of every 8 runs of 16 blocks of 2048 elements,
kMixK2: every 4th unit of 4096 elements), and

  out             bit for bit against the CPU oracle (oracle/lq_oracle.py fq_forward),
  ds and `parts`  against oracle/lq_oracle_f64.py under tests/_bounds.py, with the reference, the power-of-two scales and the
                  tolerance rule of tests/test_gpu_reverse_walk.py (whose _oracle this file calls).

The descriptors are the smallest that still take the two kernels -- both need 64 MiB (kNtBytes: 16 777 216 elements), K1 rows
with L % 4 == 0 -- in each form of launch_traverse's grid:

  (112, 3, 50176)   16.9 M elements, 3-D grid, rows of 12.25 units: a partly filled last unit per row
  (114, 3, 49152)   16.8 M elements, 3-D grid, rows of 12 full units
  (1, 65536, 2048)  65536 groups (> 65535): the 1-D grid with the division, one half-filled unit per row

A development build (liblq_hip_dev.so next to the product library, `make -C learned_quantization_amd/csrc dev`) adds one case per
pattern with a policy boundary inside a row: a contiguous tail of 0.3 of the tensor in both kernels (rows of 50176 elements:
16 859 136 * 0.7 is no multiple of 50176) and interleaved runs of 8 blocks (16384 elements, against rows of 50176) in K1 with
single units in K2, P and dy both."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _bounds import assert_within_terms, stable_seed
from oracle import lq_oracle as O32
from test_gpu_reverse_walk import _oracle

pytestmark = pytest.mark.gpu

CASES = [(112, 3, 50176), (114, 3, 49152), (1, 65536, 2048)]
LAMS = (1e-11, 1e-3)


def _inputs(outer, G, inner):
    dev = torch.device("cuda:0")
    n = outer * G * inner
    assert n * 4 >= 64 << 20, "streaming size: nontemporal k_flat_fwd and the two-float4 row stream"
    g = torch.Generator(device=dev).manual_seed(stable_seed("policy_mix", outer, G, inner) % (2 ** 31))
    P = torch.rand(n, device=dev, generator=g) * 255.0
    # ratios |dy| / |out| over nine decades: a third below lambda = 1e-11, all of them below 1e-3
    dy = torch.randn(n, device=dev, generator=g) * 1e-3 * torch.pow(10.0, torch.rand(n, device=dev, generator=g) * 9.0 - 9.0)
    s = torch.pow(2.0, torch.randint(-1, 2, (G,), device=dev, generator=g).float())
    return P, dy, s


def _check(lib, check, outer, G, inner, what):
    """Runs K1 and, for each lambda, K2 + K3 of `lib` on the descriptor and holds them to the oracles."""
    dev = torch.device("cuda:0")
    P, dy, s = _inputs(outer, G, inner)
    n = outer * G * inner
    out = torch.full((n,), float("nan"), device=dev)
    check(lib.lq_fq_forward(P.data_ptr(), s.data_ptr(), out.data_ptr(), None, 0, outer, G, inner, None), "lq_fq_forward")
    ws = torch.empty(lib.lq_workspace_bytes(outer, G, inner), dtype=torch.uint8, device=dev)
    got = {}
    for lam in LAMS:
        ds = torch.full((G,), float("nan"), device=dev)
        parts = torch.full((3 * G,), float("nan"), device=dev)
        check(lib.lq_fq_scale_grad(P.data_ptr(), s.data_ptr(), dy.data_ptr(), lam, ds.data_ptr(), parts.data_ptr(), ws.data_ptr(),
                                   ws.numel(), outer, G, inner, None), "lq_fq_scale_grad")
        torch.cuda.synchronize(dev)
        got[lam] = (ds.cpu().numpy(), parts.cpu().numpy().reshape(3, G))
    Pc, dyc, sc = P.cpu().numpy(), dy.cpu().numpy(), s.cpu().numpy()
    _, ref_out = O32.fq_forward(Pc.reshape(outer, G, inner), sc.reshape(1, G, 1))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref_out.reshape(-1).view(np.uint32), err_msg=f"{what}: out")
    del ref_out
    for lam in LAMS:
        got_ds, parts = got[lam]
        ds64, maxq64, mean64, below64, unsure = _oracle(Pc, sc, dyc, lam, outer, G, inner)
        w = f"{what} lam={lam:g}"
        print(f"{w}: max rel err ds {np.max(np.abs(got_ds - ds64) / np.abs(ds64)):.3e}, mean "
              f"{np.max(np.abs(parts[1] - mean64) / np.abs(mean64)):.3e}, count diff {np.max(np.abs(parts[2] - below64)):.0f}, "
              f"unsure {int(unsure.sum())}")
        assert below64.min() > 0, "every group has votes: the mean is a sum of terms"
        np.testing.assert_array_equal(parts[0], maxq64.astype(np.float32), err_msg=f"{w}: max|q|")
        assert_within_terms(got_ds, ds64, None, f"{w}: ds")
        assert_within_terms(parts[1], mean64, None, f"{w}: mean")
        tol = unsure + below64 * 2.0 ** -24
        assert np.all(np.abs(parts[2].astype(np.float64) - below64) <= tol), f"{w}: vote count"


@pytest.mark.parametrize("outer,G,inner", CASES)
def test_policy_mix_shipped_constants(outer, G, inner):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from learned_quantization_amd import _hip
    _check(_hip.load(), _hip.check, outer, G, inner, f"({outer}, {G}, {inner})")


def _word(mask_p, mask_dy, log2run, tail=0):
    return mask_p | (mask_dy << 8) | (log2run << 16) | (tail << 24)


# name -> (lq_dev_set_flags: K2's tail in bits 0xf00 as 1 + tenths, K1's mix word with its own tail in bits 24-27, K2's mix word)
DEV_POINTS = {"contiguous": (4 << 8, _word(0, 0, 0, tail=4), _word(0, 0, 0)),
              "interleaved": (1 << 8, _word(0x15, 0, 3, tail=1), _word(0x15, 0x11, 0))}


@pytest.mark.parametrize("pattern", sorted(DEV_POINTS))
def test_policy_mix_development_patterns(pattern):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from learned_quantization_amd import _hip
    path = os.path.join(os.path.dirname(_hip.LIB_PATH), "liblq_hip_dev.so")
    if not os.path.exists(path):
        pytest.skip("development build only: make -C learned_quantization_amd/csrc dev")
    dev = ctypes.CDLL(path)
    for name, (restype, argtypes) in _hip.SIGNATURES.items():
        fn = getattr(dev, name)
        fn.restype, fn.argtypes = restype, argtypes
    dev.lq_dev_set_policy_mix.argtypes = [ctypes.c_uint, ctypes.c_uint]

    def check(rc, what):
        assert rc == 0, f"{what}: {rc}"

    flags, w1, w2 = DEV_POINTS[pattern]
    check(dev.lq_dev_set_flags(flags), "lq_dev_set_flags")
    check(dev.lq_dev_set_policy_mix(w1, w2), "lq_dev_set_policy_mix")
    try:
        _check(dev, check, 112, 3, 50176, f"dev {pattern} (112, 3, 50176)")
    finally:
        dev.lq_dev_set_flags(0)
        dev.lq_dev_set_policy_mix(0xffffffff, 0xffffffff)
