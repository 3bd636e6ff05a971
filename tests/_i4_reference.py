"""NumPy packer of the packed 4-bit B operand, from the layout text of include/lq_hip.h: codes [LT][KT][64 lanes][8 bytes]; fragment
`lane` of tile (lt, kt) holds line 16 lt + (lane & 15); with g = lane >> 4, byte 4 d + t holds code k = 64 kt + 16 g + 8 d + t in its low
nibble and k = 64 kt + 16 g + 8 d + 4 + t in its high nibble; nibble 0 past L and K; scales and offsets are the int8 operand's buffers.
An operand is tests/_i8_reference.py's dict with codes in [-8, 7]; every expected product comes from that module's references."""
import numpy as np

import _i8_reference as G


def _where(KT, line, k):
    """(byte offset, bit shift) of the nibble of (line, k)."""
    lane, j = 16 * ((k & 63) >> 4) + (line & 15), k & 15
    return (((line >> 4) * KT + (k >> 6)) * 64 + lane) * 8 + 4 * (j >> 3) + (j & 3), 4 * ((j >> 2) & 1)


def pack_layout(op):
    """(code buffer uint8 [LT * KT * 512], scale buffer) of an operand whose codes lie in [-8, 7], padding included."""
    codes = np.asarray(op["codes"], np.int8)
    assert codes.min() >= -8 and codes.max() <= 7
    L, K = codes.shape
    LT, KT, _ = G.layout_dims(L, K, op["block"])
    ln, k = np.meshgrid(np.arange(L), np.arange(K), indexing="ij")
    off, shift = _where(KT, ln, k)
    cbuf = np.zeros(LT * KT * 512, np.uint8)
    np.bitwise_or.at(cbuf, off, ((codes.view(np.uint8) & 0xF) << shift).astype(np.uint8))
    return cbuf, G.pack_layout(op)[1]


def unpack_codes(cbuf, L, K):
    """int8 [L][K]: the sign-extended nibbles of a packed code buffer."""
    KT = -(-K // 64)
    ln, k = np.meshgrid(np.arange(L), np.arange(K), indexing="ij")
    off, shift = _where(KT, ln, k)
    nib = (np.asarray(cbuf, np.uint8).reshape(-1)[off] >> shift) & 0xF
    return ((nib ^ 8).astype(np.int16) - 8).astype(np.int8)


def narrow(op):
    """``op`` with its byte codes folded into [-8, 7] (the low nibble, sign-extended)."""
    return dict(op, codes=(((op["codes"].astype(np.int16) & 0xF) ^ 8) - 8).astype(np.int8))


def nibble_sweep_case(K=128, N=16):
    """(A, B) for the nibble-to-k map: A stacks tests/_i8_reference.one_hot_case(k) for every k; B [N][K] holds code
    ((n + 5 (k & 15) + (k >> 4)) & 15) - 8: the 16 nibbles of every fragment are 16 different codes (5 is odd), so any exchange of
    nibbles inside a lane shows, and along the 16 lines every code meets every nibble position."""
    a = np.concatenate([G.one_hot_case(k, K)[0]["codes"] for k in range(K)])
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    b = (((n + 5 * (k & 15) + (k >> 4)) & 15) - 8).astype(np.int8)
    one = lambda L: np.ones((L, 1), np.float32)      # noqa: E731
    return dict(codes=a, scales=one(a.shape[0]), block=0), dict(codes=b, scales=one(N), block=0)
