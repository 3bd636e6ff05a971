"""CPU tests of the packed 4-bit B operand (include/lq_hip.h): the NumPy packer on a fragment written out by hand, the sizes, the
refusals through C (validation comes before any launch) and Python, the data condition of tests/test_gpu_i4.py's nibble sweep."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _i4_reference as R4                                                                    # noqa: E402

from learned_quantization_amd import _hip, ops                                                # noqa: E402

def test_packer_on_a_fragment_written_out_by_hand():
    """Line 17 of a 40 x 130 operand (LT = 3, KT = 3), k = 80 .. 95: tile (1, 1), g = 1, so lane 16 + 1 and byte offset
    ((1 * 3 + 1) * 64 + 17) * 8 = 2184.  Codes -8 .. 7 in k order: byte 4 d + t = (low: code 8 d + t, high: code 8 d + 4 + t), i.e.
    d = 0: (-8, -4) (-7, -3) (-6, -2) (-5, -1) -> 0xC8 0xD9 0xEA 0xFB; d = 1: (0, 4) (1, 5) (2, 6) (3, 7) -> 0x40 0x51 0x62 0x73."""
    codes = np.zeros((40, 130), np.int8)
    codes[17, 80:96] = np.arange(-8, 8)
    cbuf, sbuf = R4.pack_layout(dict(codes=codes, scales=np.ones((40, 1), np.float32), block=0))
    assert cbuf.size == 3 * 3 * 512 and sbuf.size == 48
    assert cbuf[2184:2192].tolist() == [0xC8, 0xD9, 0xEA, 0xFB, 0x40, 0x51, 0x62, 0x73]
    assert np.flatnonzero(cbuf).tolist() == list(range(2184, 2192))
    assert np.array_equal(R4.unpack_codes(cbuf, 40, 130), codes)
    # the header's dword rule: (x_d << 4) & 0xF0F0F0F0 and x_d & 0xF0F0F0F0 are dwords 2 d and 2 d + 1 of the int8 fragment, times 16
    x = cbuf[2184:2192].view("<u4").astype(np.uint64)
    times16 = (codes[17, 80:96].astype(np.int16) * 16).astype(np.int8).view("<u4")
    mask = np.uint64(0xF0F0F0F0)
    assert [int((x[0] << np.uint64(4)) & mask), int(x[0] & mask), int((x[1] << np.uint64(4)) & mask), int(x[1] & mask)] == times16.tolist()


def test_bytes_are_half_the_codes_and_all_the_scales():
    for L_, K, block in [(1, 1, 0), (17, 65, 64), (10, 784, 128), (4096, 4096, 0), (33, 513, 192)]:
        cb, sb = ops.i8_operand_bytes(L_, K, block)
        assert ops.i4_operand_bytes(L_, K, block) == (cb // 2, sb) and cb % 2 == 0


def test_refusals():
    lib = _hip.load()
    err = lambda: lib.lq_last_error().decode()      # noqa: E731
    ok = [4096, 4096, -8, 7, 0, 128, 16, 0, 64, 4096, 4096, None]      # P, s, qmin, qmax, rounding, R, C, axis, gs, codes, scales, stream
    for qmin, qmax in ((-9, 7), (0, 15), (-8, 8)):
        assert lib.lq_i4_operand_pack(*ok[:2], qmin, qmax, *ok[4:]) == -1 and "not inside [-8, 7]" in err()
    assert lib.lq_i4_operand_pack(*ok[:8], 96, *ok[9:]) == -1 and "multiple of 64" in err()
    with pytest.raises(ValueError, match=r"\(-9, 7\) is not inside \[-8, 7\]"):
        ops.check_i4_operand_layer((-9, 7), "groupwise", 64)
    with pytest.raises(ValueError, match=r"\(0, 15\).*not built"):
        ops.check_i4_operand_layer((0, 15), "groupwise", 64)
    with pytest.raises(ValueError, match="group_size=96"):
        ops.check_i4_operand_layer((-8, 7), "groupwise", 96, fan_in=200)
    assert ops.check_i4_operand_layer((-8, 7), "groupwise", 64, asymmetric=True, offsets=True) == (-8, 7)
    assert ops.check_i4_operand_layer((-7, 7), "scalar", conv=True) == (-7, 7)
    # a packed operand is a B operand only
    z = torch.zeros(512, dtype=torch.uint8), torch.ones(16)
    a4, b8 = ops.I4Operand(*z, 16, 64, 0), ops.I8Operand(torch.zeros(1024, dtype=torch.uint8), z[1], 16, 64, 0)
    for product in (ops.i8_gemm, ops.i8_gemm_quantize):
        with pytest.raises(ValueError, match="B operand only"):
            product(a4, b8)
    with pytest.raises(ValueError, match="codes must be 512 uint8"):      # the byte operand's buffer under the packed type
        ops.i8_gemm(b8, ops.I4Operand(b8.codes, z[1], 16, 64, 0))


def test_nibble_sweep_covers_every_code_in_every_nibble_position():
    """B's packed buffer: every code in the low and high nibble of each byte position, 16 different nibbles per fragment; A: every k."""
    a, b = R4.nibble_sweep_case()
    frags = R4.pack_layout(b)[0].reshape(-1, 8)
    for byte in range(8):
        assert set(frags[:, byte] & 0xF) == set(range(16)) and set(frags[:, byte] >> 4) == set(range(16)), byte
    assert a["codes"].shape == (2048, 128) and all((np.flatnonzero(a["codes"][16 * k:16 * k + 16].any(0)) == [k]).all() for k in range(128))
    assert all(len(set((f & 0xF).tolist() + (f >> 4).tolist())) == 16 for f in frags)
