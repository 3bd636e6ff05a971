"""The streaming scale gradient walks its units from the end of the tensor (k_row_stream<OP_BWD, 4, 512, 1, 2, TAIL>, kMallWalk in
csrc/lq_traverse.hpp) and loads the end of P with the default cache policy: which block takes which (row, chunk) changed, what a
unit sums and where its partial goes did not.  lq_fq_scale_grad with `parts` on row descriptors of streaming size against
oracle/lq_oracle_f64.py under the bounds of tests/_bounds.py, for both grid forms of launch_traverse:

  (256, 3, 50176)   3-D grid (chunk, group, outer), rows of 12.25 chunks of 4096: a partly filled last chunk
  (256, 3, 49152)   3-D grid, rows of 12 full chunks
  (70000, 1, 2048)  one scale: the plan takes G == 1 as ONE row of 143 M elements -- 35000 full chunks in the x dimension of a 3-D grid
  (1, 70000, 2048)  70000 groups (> 65535): the 1-D grid with the division, one half-filled chunk per row

Scales are powers of two, so P / s and q * s are exact in float32 and float64 alike and max|q| is compared bit for bit; the vote
sums are sums of terms of one sign, so |reference| is their sum|terms|.  An element whose float64 ratio lies within float32
rounding of lambda may fall on either side of the comparison: its term is below 1e-7 * lambda, and the count of such elements
(in practice none) is the tolerance of the vote count, next to the float32 rounding of the count itself."""
import numpy as np
import pytest
import torch

from _bounds import assert_within_terms, stable_seed
from oracle import lq_oracle_f64 as O64

pytestmark = pytest.mark.gpu

CASES = [(256, 3, 50176), (256, 3, 49152), (70000, 1, 2048), (1, 70000, 2048)]


def _oracle(P, s, dy, lam, outer, G, inner):
    """float64 reference: ds from O64.scale_grad; max|q| from O64.forward; the mean is ds / max|q| (the oracle's ds is their
    product); the vote count restated from its ratio test.  Many groups with outer == 1 are contiguous rows: the oracle, which
    selects every group from the whole tensor, is then called on slabs of ten rows."""
    if outer == 1 and G > 64:
        ds = np.concatenate([O64.scale_grad(P[a * inner:(a + 10) * inner], s[a:a + 10], lam, dy[a * inner:(a + 10) * inner],
                                            1, min(10, G - a), inner) for a in range(0, G, 10)])
    else:
        ds = O64.scale_grad(P, s, lam, dy, outer, G, inner)
    q, pr = O64.forward(P, s, outer, G, inner)
    maxq = np.abs(q).reshape(outer, G, inner).max(axis=(0, 2))
    del q
    r = np.abs(dy.astype(np.float64)) / np.abs(np.where(pr == 0.0, O64.EPS_F32, pr))
    del pr
    lam64 = float(np.float32(lam))
    below = (~(r >= lam64)).reshape(outer, G, inner).sum(axis=(0, 2))
    unsure = (np.abs(r - lam64) <= 2.0 ** -22 * lam64).reshape(outer, G, inner).sum(axis=(0, 2))
    return ds, maxq, ds / maxq, below, unsure


@pytest.mark.parametrize("lam", [1e-11, 1e-3])
@pytest.mark.parametrize("outer,G,inner", CASES)
def test_reverse_walk_scale_grad_against_f64(outer, G, inner, lam):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from learned_quantization_amd import _hip
    lib = _hip.load()
    dev = torch.device("cuda:0")
    n = outer * G * inner
    assert n * 4 >= 64 << 20, "streaming size: the nontemporal two-float4 row stream"
    g = torch.Generator(device=dev).manual_seed(stable_seed(outer, G, inner) % (2 ** 31))
    P = torch.rand(n, device=dev, generator=g) * 255.0
    # ratios |dy| / |out| over nine decades: a third below lambda = 1e-11, all of them below 1e-3
    dy = torch.randn(n, device=dev, generator=g) * 1e-3 * torch.pow(10.0, torch.rand(n, device=dev, generator=g) * 9.0 - 9.0)
    s = torch.pow(2.0, torch.randint(-1, 2, (G,), device=dev, generator=g).float())
    ds = torch.full((G,), float("nan"), device=dev)
    parts = torch.full((3 * G,), float("nan"), device=dev)
    ws = torch.empty(lib.lq_workspace_bytes(outer, G, inner), dtype=torch.uint8, device=dev)
    rc = lib.lq_fq_scale_grad(P.data_ptr(), s.data_ptr(), dy.data_ptr(), lam, ds.data_ptr(), parts.data_ptr(), ws.data_ptr(),
                              ws.numel(), outer, G, inner, None)
    _hip.check(rc, "lq_fq_scale_grad")
    torch.cuda.synchronize(dev)
    got_ds = ds.cpu().numpy()
    got = parts.cpu().numpy().reshape(3, G)
    ds64, maxq64, mean64, below64, unsure = _oracle(P.cpu().numpy(), s.cpu().numpy(), dy.cpu().numpy(), lam, outer, G, inner)
    what = f"({outer}, {G}, {inner}) lam={lam:g}"
    print(f"{what}: max rel err ds {np.max(np.abs(got_ds - ds64) / np.abs(ds64)):.3e}, mean "
          f"{np.max(np.abs(got[1] - mean64) / np.abs(mean64)):.3e}, count diff {np.max(np.abs(got[2] - below64)):.0f}, "
          f"unsure {int(unsure.sum())}")
    assert below64.min() > 0, "every group has votes: the mean is a sum of terms"
    np.testing.assert_array_equal(got[0], maxq64.astype(np.float32), err_msg=f"{what}: max|q|")
    assert_within_terms(got_ds, ds64, None, f"{what}: ds")
    assert_within_terms(got[1], mean64, None, f"{what}: mean")
    tol = unsure + below64 * 2.0 ** -24
    assert np.all(np.abs(got[2].astype(np.float64) - below64) <= tol), f"{what}: vote count"
