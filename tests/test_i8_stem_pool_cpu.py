"""CPU tests of lq_i8_stem_conv2d_quantize_pool: the reference on a hand-written case, the refusals (nothing is launched), the new
keywords' defaults, and the data conditions of the GPU cases, on the reference alone."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i8_stem_pool_reference as R                                                           # noqa: E402
from test_i8_direct_cpu import LQ_EINVAL, P, _g                                               # noqa: E402

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402


def test_reference_on_a_hand_written_case():
    """4 x 4 under pads (0, 1, 0, 1): window (0, 0) holds a NaN, (0, 1) only -inf, (1, 0) ends on the padding, (1, 1) is one element."""
    inf, nan = np.inf, np.nan
    v = np.array([[1, 2, -inf, -inf], [3, nan, -inf, -inf], [5, 4, -inf, -inf], [9, 8, 7, -2]], np.float32).reshape(1, 4, 4, 1)
    p = R.pool3(v, (0, 1, 0, 1))[0, :, :, 0]
    assert np.isnan(p[0, 0]) and p[0, 1] == -inf and p[1, 0] == 9 and p[1, 1] == 7


_s = lambda **kw: _g(**{"C": 3, "xs": (105, 35, 7, 1), **kw})                                 # noqa: E731
_pool = lambda pads=(0, 1, 0, 1), g=None: (P, P, P, P, None, ctypes.byref(g or _s()), 10, None, None, 0, 0, *pads, P, P, None)  # noqa: E731


@pytest.mark.parametrize("args,why", [(_pool(pads=(2, 0, 0, 0)), "pool padding (2, 0, 0, 0): each of"), (_pool(pads=(0, 0, 0, -1)), "is 0 or 1"),
                                      (_pool(g=_s(H=2, W=7, KH=1, KW=1, pads=(0, 0, 0, 0)), pads=(0, 0, 1, 1)), "holds no 3 x 3 window")])
def test_refusals_of_the_c_surface(args, why):
    lib = _hip.load()
    assert len(lib.lq_i8_stem_conv2d_quantize_pool.argtypes) == 18 and lib.lq_i8_stem_conv2d_quantize_pool(*args) == LQ_EINVAL
    assert why in lib.lq_last_error().decode() and "lq_i8_stem_conv2d_quantize_pool:" in lib.lq_last_error().decode()


def test_python_refusals_and_defaults():
    m = lq.build_model("imagenette", mode="ste", value=0.0, bits=8, orientation="scalar", input_shape=(3, 32, 32)).eval()
    x, (chain, pools), hw = torch.zeros(1, 3, 8, 8), m.i8_stem_chain(), dict(convs=True, direct=True)
    for why, call in (("pool=2: only the 3 x 3 maximum of stride 2", lambda: ops.i8_stem_conv2d_quantize(None, None, pool=2)),
                      ("without pool=3", lambda: ops.i8_stem_conv2d_quantize(None, None, pool_padding=(0, 1, 0, 1))),
                      ("pool=3 without out_pixels=True", lambda: m.stem.call_i8_stem(x, pool=3)),
                      ("built in the stem convolution's epilogue only", lambda: m.blocks[0].conv1.call_i8_direct(torch.zeros(1, 64, 8, 8), out_pixels=True, pool=3)),
                      ("step 0: pool=3: only the non-overlapping 2 x 2 maximum", lambda: L.i8_conv_chain(x, chain, out_pixels=True, pools=[3])),
                      ("the stem epilogue takes no pool but 3", lambda: L.i8_conv_chain(x, chain, out_pixels=True, stem=True, pools=[2])),
                      ("stem_pool=True needs stem_convs=True and fused_convs=True", lambda: L.i8_hardware(m, **hw, stem_convs=True, stem_pool=True)),
                      ("emulate=True with stem_pool=True", lambda: L.i8_hardware(m, **hw, emulate=True, stem_pool=True))):
        with pytest.raises(ValueError, match=why):
            call()
    assert L.i8_hardware(m, **hw, stem_convs=True, fused_convs=True).stem_pool is False and pools == [3]
    for fn, name, default in ((ops.i8_stem_conv2d_quantize, "pool", None), (ops.i8_stem_conv2d_quantize, "pool_padding", (0, 0, 0, 0)),
                              (m.stem.call_i8_stem, "pool", None), (train.i8_eval, "stem_pool", False)):
        assert inspect.signature(fn).parameters[name].default == default and train.build_parser().parse_args([]).i8_eval_stem_pool is False


def test_data_conditions_of_the_gpu_cases():
    """A planted NaN spoils exactly the windows that cover it; the dead window is +0 in every channel; nine distinct argmax positions."""
    g, pads, rows, q, sk, bias, affine = R.case(0, 40, "bad")
    _, p, v = R.pooled_reference(g, pads, rows, q, sk, bias)
    covered = R.pool3(np.isnan(v).astype(np.float32), pads) > 0
    assert np.array_equal(np.isnan(p), covered) and 0 < np.isnan(p).sum() < p.size and np.isneginf(p).any() and np.isneginf(v).any()
    g, pads, rows, q, sk, bias, affine = R.case(1, 40, "dead")
    ref, p, _ = R.pooled_reference(g, pads, rows, q, sk, bias, "relu")
    assert not p[0, 0, 0].any() and ref["scales"][0, 0, 0] == np.float32(2.0 ** -126) and (p[0] > 0).any()
    g, pads, rows, q, sk = R.argmax_case()
    _, p, v = R.pooled_reference(g, pads, rows, q, sk, None)
    where = [int(np.argmax(v[k, :3, :3, 0])) for k in range(9)]
    assert where == list(range(9)) and all(p[k, 0, 0, 0] == v[k, k // 3, k % 3, 0] for k in range(9))
