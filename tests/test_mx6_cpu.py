"""CPU tests of the fp6 MX operand (include/lq_hip.h: lq_mx6_*): sizes, the NumPy packer of the documented layout, the refusals of
the new C and Python surface with their messages, and that the old surface still refuses fp6 without the opt-in."""
import ctypes

import numpy as np
import pytest
import torch

import _mx6_reference as R

from learned_quantization_amd import _hip, layers as L, ops

FP4, FP6A, FP6B, E4M3, E5M2 = 0, 1, 2, 3, 4
_dense = lambda **kw: L.CustomDenseLayer(units=4, initializer=L.RandomNormal(seed=1), input_shape=70, orientation="groupwise", **kw)      # noqa: E731


@pytest.mark.parametrize("shape", [(1, 1), (16, 128), (17, 129), (40, 70), (33, 513)], ids=str)
@pytest.mark.parametrize("name", R.FORMATS6)
def test_sizes_and_the_packer(name, shape):
    """The packer round-trips; the live bits have distinct addresses inside the buffer and are exactly the bits an all-ones operand
    sets, so every byte is written once and the rest is code 0 / byte 127.  A whole tile (16, 128) has no padding."""
    (L_, K), LT, KT = shape, -(-shape[0] // 16), -(-shape[1] // 128)
    rng = np.random.default_rng(L_ * 1000 + K)
    codes, bytes_ = rng.integers(0, 64, size=(L_, K)), rng.integers(0, 256, size=(L_, -(-K // 32)))
    cbuf, sbuf = R.pack_layout(codes, bytes_)
    assert ops.mx6_operand_bytes(name, L_, K) == (LT * KT * 1536, LT * -(-KT // 4) * 256) == (cbuf.size, sbuf.size)
    got = R.unpack_layout(cbuf, sbuf, L_, K)
    assert np.array_equal(got[0], codes) and np.array_equal(got[1], bytes_)
    off, bit = R.bit_addresses(L_, K)
    live = np.unique(off * 8 + bit)
    assert live.size == 6 * L_ * K and live[0] >= 0 and live[-1] < cbuf.size * 8 and (shape != (16, 128) or live.size == cbuf.size * 8)
    ones, sones = R.pack_layout(np.full((L_, K), 63), np.zeros_like(bytes_))
    assert np.array_equal(np.flatnonzero(np.unpackbits(ones, bitorder="little")), live) and int((sones != 127).sum()) == bytes_.size


def test_refusals_of_the_c_surface():
    lib = _hip.load()
    buf, cb, sb = (ctypes.c_float * 64)(), ctypes.c_size_t(0), ctypes.c_size_t(0)
    p = (ctypes.addressof(buf) + 15) & ~15                # 16-byte aligned; never dereferenced: every call fails in validation
    refused = lambda rc, needle: rc == -1 and needle in lib.lq_last_error().decode()      # noqa: E731  (-1: LQ_EINVAL)
    for bad, needle in ((FP4, "is not an fp6 format"), (E4M3, "is not an fp6 format"), (5, "bad element format")):
        assert refused(lib.lq_mx6_operand_bytes(bad, 16, 128, ctypes.byref(cb), ctypes.byref(sb)), needle)
        assert refused(lib.lq_mx6_operand_pack(p, p, bad, 0, 70, 40, 0, 32, p, p, None), needle)
        assert refused(lib.lq_mx6_operand_quantize(p, bad, 0, 5, 100, p, p, None), needle)
        assert refused(lib.lq_mx6_operand_decode(p, p, bad, 5, 100, p, None), needle)
    gemm, gq = lib.lq_mx6_gemm, lib.lq_mx6_gemm_quantize   # (FP4, E5M2): a pair without an fp6 side
    assert refused(gemm(p, p, FP4, p, p, E5M2, None, p, 16, 16, 128, 16, None), "that product is lq_mx_gemm's")
    assert refused(gq(p, p, FP4, p, p, E5M2, None, 0, E4M3, 0, p, p, 16, 16, 128, None), "that product is lq_mx_gemm's")
    assert refused(gemm(p, p, FP6A, p, p, 5, None, p, 16, 16, 128, 16, None), "bad element format")
    assert refused(gq(p, p, FP6A, p, p, E4M3, None, 0, FP6B, 0, p, p, 16, 16, 128, None), "epilogue is not built")
    assert refused(lib.lq_mx6_operand_pack(p, p, FP6A, 0, 70, 40, 0, 16, p, p, None), "the instruction's block is 32")
    assert refused(lib.lq_mx6_operand_pack(p, p, FP6B, 1, 70, 40, 0, 32, p, p, None), "E8M0 scales only")
    assert refused(lib.lq_mx_operand_bytes(FP6A, 16, 128, ctypes.byref(cb), ctypes.byref(sb)), "fp6 operands are not supported")      # old


def test_refusals_of_the_python_surface_with_and_without_the_opt_in():
    u8, d, x = torch.zeros(16, dtype=torch.uint8), _dense(element_format="fp6_e2m3"), torch.zeros(3, 70)
    a6, b8, old6 = ops.Mx6Operand(u8, u8, "fp6_e2m3", 16, 128), ops.MxOperand(u8, u8, "fp8_e4m3", 16, 160), ops.MxOperand(u8, u8, "fp6_e2m3", 16, 160)
    assert L.mx_hardware_eligible(d, fp6=True) and not L.mx_hardware_eligible(_dense(element_format="fp6_e3m2", group_size=64), fp6=True)
    for call, needle in ((lambda: ops.mx_gemm(b8, ops.Mx6Operand(u8, u8, "fp4_e2m1", 16, 160)), "an Mx6Operand holds one of"),
                         (lambda: ops.mx_gemm(a6, b8), "different K: 128 and 160"),
                         (lambda: _dense(element_format="fp6_e2m3", scale_format="fp32").mx_operand(fp6=True), "E8M0"),
                         (lambda: _dense(element_format="fp6_e3m2", group_size=64).call_mx(x, fp6=True), "group_size=64"),
                         (lambda: ops.mx_gemm_quantize(a6, a6, out_format="fp6_e2m3"), "fp6 operands are not supported"),
                         (lambda: L.mx_hardware(d, act_format="fp6_e2m3", fp6=True), "fp6 operands are not supported"),
                         *((call, "fp6 operands are not supported") for call in      # without the opt-in: as before
                           (lambda: ops.mx_gemm(b8, old6), d.mx_operand, lambda: d.call_mx(x), lambda: L.mx_dense_chain(x, [(d, None)])))):
        with pytest.raises(ValueError, match=needle):
            call()
    assert not L.mx_hardware_eligible(d) and not L.mx_conv_eligible(d)
    with L.mx_hardware(d.eval()) as hw:
        assert hw.layers == [] and getattr(d, "_mx_hw", None) is None
