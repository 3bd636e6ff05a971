"""NumPy packer / unpacker of the fp6 MX operand, written from the text of include/lq_hip.h ("packed fp6 MX operands").  Codes and
scale bytes are tests/_mx_gemm_reference.py's logical operands; the scale buffer is that file's, as the header says it is."""
import numpy as np

import _mx_gemm_reference as G

FORMATS6 = ("fp6_e2m3", "fp6_e3m2")
ALL_FORMATS = ("fp4_e2m1",) + FORMATS6 + ("fp8_e4m3", "fp8_e5m2")
PAIRS = [(a, b) for a in ALL_FORMATS for b in ALL_FORMATS if a in FORMATS6 or b in FORMATS6]      # the 16 with an fp6 side
_T = np.arange(6, dtype=np.int64)[:, None, None]


def bit_addresses(L, K):
    """(byte offset, bit in the byte) of bit t of code (line, k), each (6, L, K).  Fragment `lane` = 16 g + r of tile (lt, kt) holds line
    16 lt + r and k = 32 g + j: element j is its bits 6 j .. 6 j + 5; its bytes 0 .. 15 sit at [lane][16] of the tile, 16 .. 23 at 1024 + [lane][8]."""
    ln, k = np.arange(L, dtype=np.int64)[None, :, None], np.arange(K, dtype=np.int64)[None, None, :]
    lt, r, kt, kk = ln >> 4, ln & 15, k >> 7, k & 127
    lane, b = 16 * (kk >> 5) + r, 6 * (kk & 31) + _T
    off = (lt * G.layout_dims(L, K)[1] + kt) * 1536 + np.where(b < 128, lane * 16 + (b >> 3), 1024 + lane * 8 + (b >> 3) - 16)
    return off, (b & 7) + 0 * off


def pack_layout(codes, bytes_):
    """(code buffer, scale buffer), uint8, of codes (L, K) and E8M0 bytes (L, ceil(K / 32)): code 0, byte 127 where nothing lives."""
    codes = np.asarray(codes, np.int64)
    (LT, KT, _), (off, bit) = G.layout_dims(*codes.shape), bit_addresses(*codes.shape)
    cbuf = np.zeros(LT * KT * 1536, np.uint8)
    np.bitwise_or.at(cbuf, off.reshape(-1), ((((codes[None] >> _T) & 1) << bit).astype(np.uint8)).reshape(-1))
    return cbuf, G.pack_layout(np.zeros_like(codes), bytes_, "fp4_e2m1")[1]


def unpack_layout(cbuf, sbuf, L, K):
    """The inverse of pack_layout on the live part: (codes (L, K), bytes (L, ceil(K / 32))), int64."""
    off, bit = bit_addresses(L, K)
    codes = (((np.asarray(cbuf, np.uint8)[off].astype(np.int64) >> bit) & 1) << _T).sum(axis=0)
    return codes, G.unpack_layout(np.zeros(cbuf.size // 3 * 2, np.uint8), sbuf, "fp4_e2m1", L, K)[1]
