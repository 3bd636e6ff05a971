// lq_i4_operand.hpp -- 4-bit codes two to a byte, as the B operand of the int8 matrix instruction
// (lq_hip.h: lq_i4_operand_bytes / lq_i4_operand_pack / lq_i4_operand_decode and their _affine forms)
//
// An operand of L lines by K whose codes lie in [-8, 7], under the fp32 scales (and offsets) of lq_i8_operand.hpp in exactly its
// layout.  The codes are cut into the same tiles of 16 lines by 64 k, a fragment takes 8 bytes instead of 16:
//
//   codes   [LT][KT][64 lanes][8 bytes]       LT = ceil(L / 16), KT = ceil(K / 64)
//           fragment `lane` of tile (lt, kt) holds line 16 lt + (lane & 15); with g = lane >> 4, byte 4 d + t (d = 0, 1; t = 0 .. 3)
//           holds code k = 64 kt + 16 g + 8 d + t in its low nibble and code k = 64 kt + 16 g + 8 d + 4 + t in its high nibble,
//           each nibble the low four bits of the two's-complement code
//
// Read as two little-endian dwords x0, x1, (x_d << 4) & 0xF0F0F0F0 is dword 2 d of the int8 fragment with every byte multiplied
// by 16, and x_d & 0xF0F0F0F0 is dword 2 d + 1 of it with every byte multiplied by 16: a nibble moved to the top of its byte IS
// the signed byte 16 q, so the GEMM needs no per-byte sign extension (lq_i8_gemm.hpp: i8_b_operand).  The nibble order exists for
// that: bytes 4 apart in the int8 fragment share a packed byte, so one shift and two masks serve four codes each.
// Lines past L and k past K hold nibble 0; the scales of lines past L are 1.0f.
//
// pack: k_i8_pack itself (one thread per (line, 16 k), GroupStep's ctx / quant / view) with the store of this layout, 8 bytes.
#ifndef LQ_I4_OPERAND_HPP_
#define LQ_I4_OPERAND_HPP_
#include "lq_i8_operand.hpp"

namespace lq {

constexpr int kI4Min = -8, kI4Max = 7;      // what a nibble holds

// byte offset of the packed fragment that holds elements k0 .. k0 + 15 (k0 % 16 == 0) of line ln: 8 bytes
__host__ __device__ __forceinline__ int64_t i4_run_offset(int32_t KT, int32_t ln, int32_t k0) {
    const int64_t tile = (int64_t)(ln >> 4) * KT + (k0 >> 6);
    return (tile * 64 + (((k0 & 63) >> 4) << 4) + (ln & 15)) * 8;
}

// element j (0 .. 15) of a run sits in dword j >> 3 at this bit: byte j & 3, the high nibble for the second four of an eight
__host__ __device__ __forceinline__ int i4_nibble_shift(int j) { return 8 * (j & 3) + 4 * ((j >> 2) & 1); }

// the code of element k of line ln, sign-extended
__device__ __forceinline__ float i4_code(const uint8_t* codes, int32_t KT, int32_t ln, int32_t k) {
    const int j = k & 15;
    const uint32_t x = *reinterpret_cast<const uint32_t*>(codes + i4_run_offset(KT, ln, k & ~15) + 4 * (j >> 3));
    return (float)((int32_t)(x << (28 - i4_nibble_shift(j))) >> 28);
}

// k_i8_pack<.., I4RunStore>: where the 16 codes of a run go in this layout, a nibble each, 8 bytes; I8PackParams as they are
// (codes has half the bytes)
struct I4RunStore {
    static constexpr int kWords = 2;
    static __device__ __forceinline__ int word(int j) { return j >> 3; }
    static __device__ __forceinline__ uint32_t place(uint32_t byte, int j) { return (byte & 0xFu) << i4_nibble_shift(j); }
    static __device__ __forceinline__ void store(uint8_t* codes, int32_t KT, int32_t ln, int32_t k0, const uint32_t* x) {
        *reinterpret_cast<uint2*>(codes + i4_run_offset(KT, ln, k0)) = make_uint2(x[0], x[1]);
    }
};

// k_i8_decode / k_i8_decode_affine on a packed operand: the same products, bit for bit
__global__ __launch_bounds__(kBlock) void k_i4_decode(const I8DecodeParams dp) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)dp.L * dp.K) return;
    const int32_t ln = (int32_t)(i / dp.K), k = (int32_t)(i % dp.K);
    const int32_t blk = dp.block ? k / dp.block : 0;
    dp.out[i] = i4_code(dp.codes, dp.KT, ln, k) * dp.scales[(int64_t)blk * dp.LT * kI8TileLines + ln];
}

__global__ __launch_bounds__(kBlock) void k_i4_decode_affine(const I8DecodeAffineParams ap) {
    const I8DecodeParams& dp = ap.d;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)dp.L * dp.K) return;
    const int32_t ln = (int32_t)(i / dp.K), k = (int32_t)(i % dp.K);
    const int32_t blk = dp.block ? k / dp.block : 0;
    const int64_t si = (int64_t)blk * dp.LT * kI8TileLines + ln;
    dp.out[i] = __fadd_rn(__fmul_rn(i4_code(dp.codes, dp.KT, ln, k), dp.scales[si]), ap.offsets[si]);
}

}  // namespace lq

#endif
