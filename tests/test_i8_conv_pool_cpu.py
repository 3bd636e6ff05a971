"""CPU tests of lq_i8_conv2d_quantize_pool: the binding, its refusals (every call fails in validation, no pointer is dereferenced), the
Python refusals, tests/_i8_conv_pool_reference.py against a window table written out by hand, and the data conditions of the GPU
cases, asserted on the reference alone so that no case of tests/test_gpu_i8_conv_pool.py passes vacuously."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_conv_pool_reference as PR                                                          # noqa: E402
from test_i8_conv_fused_cpu import REFUSALS as PARENT, _call as _parent                       # noqa: E402
from test_i8_direct_cpu import LQ_EINVAL, _g                                                  # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops                                   # noqa: E402

R = PR.R
_call = lambda pool=2, **kw: (lambda a: (*a[:11], pool, *a[11:]))(_parent(**kw))              # noqa: E731  `pool` stands before out_codes
REFUSALS = ([((*a[:11], 2, *a[11:]), rc, why) for a, rc, why in PARENT]                       # everything lq_i8_conv2d_quantize refuses
            + [(_call(pool=k), LQ_EINVAL, f"pool = {k}: only the non-overlapping 2 x 2 maximum") for k in (0, 1, 3, -2)]
            + [(_call(g=_g(H=1, KH=1, pads=(0, 1, 0, 1))), LQ_EINVAL, "(1 x 7) holds no 2 x 2 window"),
               (_call(g=_g(W=1, KW=1, pads=(1, 0, 1, 0))), LQ_EINVAL, "(5 x 1) holds no 2 x 2 window")])


def test_the_entry_point_is_declared_exported_and_bound():
    lib, header = _hip.load(), open(os.path.join(os.path.dirname(__file__), "..", "include", "lq_hip.h")).read()
    assert "int lq_i8_conv2d_quantize_pool(" in header and "lq_i8_conv2d_quantize_pool" in _hip.SIGNATURES
    assert lib.lq_i8_conv2d_quantize_pool.argtypes[11] is ctypes.c_int32 and len(lib.lq_i8_conv2d_quantize_pool.argtypes) == 15
    assert lib.lq_version() == 3                          # additions only


@pytest.mark.parametrize("args,rc,why", REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals_of_the_c_surface(args, rc, why):
    lib = _hip.load()
    assert lib.lq_i8_conv2d_quantize_pool(*args) == rc
    assert why in lib.lq_last_error().decode() and "lq_i8_conv2d_quantize_pool:" in lib.lq_last_error().decode()


def test_refusals_and_statements_of_the_python_surface():
    m = lq.build_model("cifar", mode="ste", value=0.0, bits=8, orientation="scalar").eval()
    chain, pools = m.i8_pooled_chain()
    assert chain == [(m.convs[k], "relu", m.bns[k], False) for k in range(5)] + [(m.convs[5], None, None, False)]
    assert pools == [None, 2, None, 2, None, None]
    assert m.i8_conv_chains() == [[(m.convs[k], "relu", m.bns[k], False), (m.convs[k + 1], None, None, False)] for k in (0, 2, 4)]
    affine, x = L.bn_affine(m.bns[0]), torch.zeros(1, 3, 8, 8)
    pair = [(m.convs[0], "relu", affine, False), (m.convs[1], None, None, False)]
    residual = ops.I8Pixels(torch.zeros(1, 8, 8, 32, dtype=torch.uint8), torch.zeros(1, 8, 8), (1, 32, 8, 8))
    for chain_, kw, why in ((pair, dict(pools=[3, None]), "pool=3"), (pair, dict(pools=[True, None]), "pool=True"), (pair, dict(pools=[2]), "1 entries for 2 steps"),
                            (pair, dict(pools=[None, 2]), "a pool on the last layer, which writes fp32"),
                            ([(*pair[0], residual), pair[1]], dict(pools=[2, None]), "a pool on a step with a residual"),
                            ([(*pair[0], None, None), pair[1]], dict(pools=[2, None]), "got 6 entries")):
        with pytest.raises(ValueError, match=why):
            L.i8_conv_chain(x, chain_, **kw)
    with pytest.raises(ValueError, match="pooled_convs=True needs fused_convs=True"):
        L.i8_hardware(m, convs=True, direct=True, pooled_convs=True)
    assert L.i8_hardware(m, convs=True, direct=True, fused_convs=True).pooled_convs is False


def test_the_reference_against_a_window_table():
    """One 2 x 2 window per channel, written out by hand, in a 3 x 3 image whose last row and column hold the largest values."""
    n, inf = np.nan, np.inf
    table = [((1, 2, 3, 4), 4), ((4, 3, 2, 1), 4), ((1, 5, 5, 2), 5), ((1, n, 3, 4), n), ((n, 1, 2, 3), n), ((1, 2, 3, n), n), ((-inf, -inf, -inf, -inf), -inf),
             ((-0.0, 0.0, -0.0, 0.0), -0.0), ((0.0, -0.0, -0.0, -0.0), 0.0), ((-3, -0.0, 0.0, -1), -0.0), ((-1, inf, n, 7), n)]
    v = np.full((1, 3, 3, len(table)), 99.0, np.float32)
    v[0, :2, :2] = np.array([t[0] for t in table], np.float32).T.reshape(2, 2, -1)
    got, want = PR.pool2(v), np.array([t[1] for t in table], np.float32)
    assert got.shape == (1, 1, 1, len(table)) and got.dtype == np.float32
    got, ok = np.ascontiguousarray(got.reshape(-1)), ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])      # bits: -0 is not +0
    assert PR.pool2(np.zeros((2, 5, 7, 3), np.float32)).shape == (2, 2, 3, 3)


@pytest.mark.parametrize("co", R.WAVE_CO + R.BLOCK_CO)
@pytest.mark.parametrize("gi", [0, 1, 2])
def test_data_conditions_of_the_gpu_cases(gi, co):
    """If a seed fails a condition, change the seed (PR.SEEDS), not the condition.  The conditions of tests/test_i8_conv_fused_cpu.py
    on the pooled p; the one over the four waves needs at least four pooled pixels, so geometry 2 (PM = 1) cannot carry it."""
    g, pix, q, sk, bias, affine = PR.case(gi, co)
    for name, (act, with_affine, first) in R.EPILOGUES.items():
        out, p, v = PR.pooled_reference(g, pix, q, sk, bias, act, affine if with_affine else None, first)
        codes, p2 = out["codes"].reshape(-1, out["codes"].shape[-1]), p.reshape(-1, co)
        assert out["scales"].shape == (g[0], *(d // 2 for d in R.out_hw(g))) and np.isfinite(out["scales"]).all() and not codes[:, co:].any()
        assert (out["scales"] > np.float32(2.0 ** -126)).all(), name
        if co > 128 and gi < 2:      # every wave's columns hold the absmax channel of some pooled pixel
            top = np.abs(p2).argmax(axis=1)
            assert all(((top >= lo) & (top < hi)).any() for lo, hi in R.wave_columns(co)), (name, np.bincount(top // 16))
        POH, POW = p.shape[1:3]
        members = np.stack([v[:, di:2 * POH:2, dj:2 * POW:2] for di in (0, 1) for dj in (0, 1)])
        assert set(np.unique(members.argmax(axis=0))) == {0, 1, 2, 3}, name      # each member is the first maximum of some window
        if act == "relu" and name != "relu_affine":      # relu last: a window of non-positive members gives +0 and code 0
            assert not codes[:, :co][p2 == 0].any() and (p2 > 0).any(), name
    if co in (33, 144) and gi == 0:       # the planted cases of the GPU file
        _, p, _ = PR.pooled_reference(*PR.case(gi, co, "dead")[:5], "relu")
        dead = (p == 0).all(axis=-1)
        assert dead[0, 0, 0] and not dead.all(), "the planted window is non-positive in every member and channel, and others are alive"
        assert int(np.isnan(PR.case(gi, co, "bad")[1]["scales"]).sum()) == 2
