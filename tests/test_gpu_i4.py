"""GPU tests of the packed 4-bit B operand of the int8 GEMM (include/lq_hip.h): bytes and bits only, no tolerance.  The packed buffers
against tests/_i4_reference.py, every product against the byte operands' definitions (tests/_i8_reference.py, _i8_affine_reference.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i4_reference as R4                                                                    # noqa: E402
import _i8_affine_reference as A                                                              # noqa: E402
import _i8_reference as G                                                                     # noqa: E402
from _arena import Arena                                                                      # noqa: E402
from test_gpu_i8_affine import _np, _t, _upload as _upload8, dev                              # noqa: E402,F401  (helpers and the fixture)

import learned_quantization_amd as lq                                                         # noqa: E402
from learned_quantization_amd import _hip, layers as L, ops, train                            # noqa: E402

pytestmark = pytest.mark.gpu
_ids = lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731
KEYS = [s + (0, 0) for s in [(16, 16, 64), (19, 21, 160), (37, 10, 784), (17, 129, 128), (129, 17, 128)]] + \
       [(37, 21, 320) + p for p in [(0, 0), (0, 64), (64, 128), (128, 64), (128, 128)]]


def _upload(op, dev, int4=False):
    """A reference operand as the device's byte operand or (``int4``) packed operand, through the NumPy packers."""
    if not int4:
        return _upload8(op, dev)
    cbuf, sbuf = R4.pack_layout(op)
    off = _t(A.offsets_layout(op), dev) if "offsets" in op else None
    return ops.I4Operand(_t(cbuf, dev), _t(sbuf, dev), *op["codes"].shape, op["block"], off)


_bits = lambda g, w: g.shape == w.shape and g.dtype == w.dtype and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes()      # noqa: E731,E501


_case = lambda key: (lambda a, b, bias: (a, R4.narrow(b), bias))(*G.gemm_case(*key))      # noqa: E731
_tbits = lambda x, y: x.shape == y.shape and _bits(_np(x), _np(y))      # noqa: E731


@pytest.mark.parametrize("affine", [False, True], ids=["sym", "affine"])
@pytest.mark.parametrize("qrange", [(-8, 7), (-7, 7)], ids=_ids)
@pytest.mark.parametrize("rounding", ["floor", "nearest"])
@pytest.mark.parametrize("case", G.PACK_CASES, ids=_ids)
def test_pack_is_the_numpy_packer_and_decode_is_the_byte_operands(dev, case, rounding, qrange, affine):
    R, C, axis, gs = case
    P, s = G.pack_case(R, C, axis, gs)
    off = np.random.default_rng(R).normal(0.0, 0.3, s.shape).astype(np.float32) if affine else None
    ref = A.operand_of_parameter_affine(P, s, off, *qrange, axis, gs, rounding) if affine else \
        G.operand_of_parameter(P, s, *qrange, axis, gs, rounding)
    args = (_t(P, dev), _t(s, dev), *qrange, gs, rounding, None if off is None else _t(off, dev))
    op, byte = ops.i4_operand_pack(*args), ops.i8_operand_pack(*args)
    assert (op.lines, op.K, op.block) == (byte.lines, byte.K, byte.block) == (*ref["codes"].shape, ref["block"])
    assert _bits(_np(op.codes), R4.pack_layout(ref)[0]), "the packed codes are not the NumPy packer's"
    assert _bits(_np(op.scales), _np(byte.scales)) and (not affine or _bits(_np(op.offsets), _np(byte.offsets)))
    assert G.buffers_mismatch(_np(byte.codes), _np(op.scales), ref) is None
    assert _bits(_np(ops.i8_operand_decode(op)), _np(ops.i8_operand_decode(byte))), "decode"


def test_nibble_to_k_map(dev):
    """Every k of two K steps singled out by a one-hot A; B puts every code into every nibble position (tests/test_i4_cpu.py)."""
    a, b = R4.nibble_sweep_case()
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev, int4=True)))
    want = np.concatenate([(np.arange(16)[:, None] + 1) * b["codes"][None, :, k].astype(np.int64) for k in range(128)])
    assert np.array_equal(y, want.astype(np.float32)) and _bits(y, G.gemm_reference(a, b))


@pytest.mark.parametrize("key", KEYS, ids=_ids)
def test_gemm_on_a_packed_b_is_the_definition(dev, key):
    a, b, bias = _case(key)
    (M, N), a_dev, b4 = key[:2], _upload(a, dev), _upload(b, dev, int4=True)
    assert _bits(_np(ops.i8_gemm(a_dev, b4)), G.gemm_reference(a, b))
    out = torch.full((M, N + 5), -7.0, device=dev)
    ops.i8_gemm(a_dev, b4, _t(bias, dev), out=out[:, :N])
    assert _bits(_np(out[:, :N]), G.gemm_reference(a, b, bias)) and bool((out[:, N:] == -7.0).all())
    bo = A.with_offsets(b)
    assert _bits(_np(ops.i8_gemm(a_dev, _upload(bo, dev, int4=True), _t(bias, dev))), A.gemm_affine_reference(a, bo, bias))
    assert _bits(_np(ops.i8_gemm(a_dev, _upload(A.with_offsets(b, zero=True), dev, int4=True))), G.gemm_reference(a, b))


def test_extreme_period_at_the_int32_bound(dev):
    """K = 65536 of (-128) * (-8): the accumulators hold 16 x the sum, 65536 * 128 * 128 = 2^30, the bound the byte operands have."""
    a, b = G.extreme_case(-8)
    y = _np(ops.i8_gemm(_upload(a, dev), _upload(b, dev, int4=True)))
    assert np.array_equal(y, np.full((16, 16), 65536.0 * 128 * 8, np.float32)) and _bits(y, G.gemm_reference(a, b))


@pytest.mark.parametrize("affine", [False, True], ids=["sym", "affine"])
@pytest.mark.parametrize("activation", [None, "relu"])
@pytest.mark.parametrize("key", [(17, 96, 128, 0, 64), (70, 160, 200, 64, 128), (33, 10, 784, 64, 0)], ids=_ids)
def test_gemm_quantize_on_a_packed_b_writes_the_byte_paths_buffers(dev, key, activation, affine):
    a, b, bias = _case(key)
    b = A.with_offsets(b) if affine else b
    a_dev, bias = _upload(a, dev), _t(bias * 0.01, dev)
    got, want = (ops.i8_gemm_quantize(a_dev, _upload(b, dev, int4=i4), bias, activation) for i4 in (True, False))
    assert isinstance(got, ops.I8Operand) and _bits(_np(got.codes), _np(want.codes)) and _bits(_np(got.scales), _np(want.scales))


def test_memory_contract_of_pack(dev):
    R, C, axis, gs = 33, 320, 1, 128
    P, s = G.pack_case(R, C, axis, gs)
    ref = G.operand_of_parameter(P, s, -8, 7, axis, gs, "nearest")
    cb, sb = ops.i4_operand_bytes(*ref["codes"].shape, ref["block"])
    ar = Arena(dev)
    ar.add("P", "in", data=P, residue=4, row_bytes=C * 4)
    ar.add("s", "in", data=s, residue=4)
    ar.add("codes", "out", nbytes=cb)
    ar.add("scales", "out", nbytes=sb)
    ar.build()
    _hip.check(_hip.load().lq_i4_operand_pack(ar.ptr("P"), ar.ptr("s"), -8, 7, 1, R, C, axis, gs, ar.ptr("codes"), ar.ptr("scales"),
                                              _hip.stream_ptr(dev)), "lq_i4_operand_pack")
    torch.cuda.synchronize()
    ar.check("i4 pack")
    assert _bits(ar.numpy("codes", np.uint8), R4.pack_layout(ref)[0])


@pytest.mark.parametrize("asymmetric", [False, True], ids=["sym", "affine"])
def test_dense_and_conv_layers_with_the_packed_operand(dev, asymmetric):
    kw = dict(scale_gradient="ste", initializer=lq.RandomNormal(seed=2), device=dev, bits=4, orientation="groupwise", group_size=64,
              asymmetric=asymmetric)
    dense = lq.CustomDenseLayer(units=21, input_shape=200, **kw)
    conv = lq.CustomConv2DLayer(filters=24, kernel_size=(3, 3), padding="same", input_shape=16, **kw)
    gen = torch.Generator(device=dev).manual_seed(1)
    for layer, x in ((dense, torch.randn(19, 200, device=dev, generator=gen)), (conv, torch.randn(2, 16, 9, 10, device=dev, generator=gen))):
        layer.init_scales("minmax" if asymmetric else "absmax")
        layer.eval()
        op = layer.i8_operand(offsets=asymmetric, int4=True)
        assert isinstance(op, ops.I4Operand) and (op.offsets is not None) == asymmetric and L.i8_int4_eligible(layer, asymmetric)
        want = layer.call_i8(x, 64, offsets=asymmetric)
        assert _tbits(layer.call_i8(x, 64, offsets=asymmetric, int4=True), want) and float(want.abs().max()) > 0


def test_mnist_fused_and_cifar_convs_under_i8_hardware(dev):
    mnist = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", bits=4, group_size=128).eval()
    x = torch.randn(5, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    with L.i8_hardware(mnist, act_block=64, fused=True) as hw:
        want = mnist(x).detach()
        assert hw.int4_layers == []
    with L.i8_hardware(mnist, act_block=64, fused=True, int4=True) as hw:
        assert hw.int4_layers == hw.layers and len(hw.fused_layers) == 2 and all(isinstance(m._i8_hw[0], ops.I4Operand) for m in hw.layers)
        assert _tbits(mnist(x).detach(), want)
    assert _tbits(*(L.i8_dense_chain(x.reshape(5, -1), mnist.i8_chain(), 64, int4=i4) for i4 in (True, False)))      # packs its own operands
    out = train.i8_eval(mnist, x, torch.arange(5, device=dev) % 10, act_block=64, int4=True)
    assert out["i8_eval_int4_layers"] == 2 and out["i8_eval_int4_max_logit_diff"] == 0.0
    cifar = lq.build_model("cifar", mode="ste", value=0.0, seed=3, device=dev, scale_init="absmax", kernel_storage="oihw", bits=4,
                           group_size=64).eval()
    xc = torch.rand(2, 3, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    with L.i8_hardware(cifar, convs=True) as hw:
        want, n = cifar(xc).detach(), len(hw.layers)
    with L.i8_hardware(cifar, convs=True, int4=True) as hw:
        assert len(hw.layers) == n and hw.int4_layers == hw.layers and sum(isinstance(m, L._ConvBase) for m in hw.int4_layers) == 6
        assert _tbits(cifar(xc).detach(), want) and bool(torch.isfinite(want).all())
