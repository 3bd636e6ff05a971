// lq_mx_operand.hpp -- packed microscaling (MX) operands in the order the block-scaled matrix instruction consumes them
// (lq_hip.h: lq_mx_operand_bytes / lq_mx_operand_pack / lq_mx_operand_quantize / lq_mx_operand_decode)
//
// An operand is a matrix of L lines by K reduction elements: element codes at the instruction's width (8 bits for the fp8 formats,
// 4 bits for fp4) and one E8M0 byte per block of 32 along K.  It is cut into tiles of 16 lines by 128 K, the A (or B) operand of
// one v_mfma_scale_f32_16x16x128_f8f6f4.  Lane l of the wave holds line (l & 15); with g = l >> 4 (the map is pinned on the device
// by the exact GEMM tests of tests/test_gpu_mx_gemm.py):
//   fp4   the 32 consecutive k = 32 g + j of the step in its four operand registers: one MX block
//   fp8   k = 16 g + j in registers 0 .. 3 and k = 64 + 16 g + j in registers 4 .. 7 (j = 0 .. 15): halves of TWO blocks
//   scale the byte of block g (k = 32 g .. 32 g + 31) of its line, for every format: the instruction applies scales by k, not by
//         the lane that holds the data
//
//   codes   [LT][KT][64 lanes][FB bytes]      LT = ceil(L / 16), KT = ceil(K / 128), FB = 32 (fp8) or 16 (fp4)
//           an fp8 fragment holds one element per byte in the order above; an fp4 fragment holds element j in bits 4 (j & 1) .. + 3
//           of byte j >> 1 (the low nibble is the even element).  Read as little-endian dwords these are the operand registers.
//   scales  [LT][KG][64 lanes][4 bytes]       KG = ceil(KT / 4): byte u of a lane's dword is the scale of K step 4 kg + u, so a
//           lane loads one dword per four K steps and the instruction's op-sel picks the byte
//
// Lines past L and elements past K hold code 0 (+0 in every format) under byte 127 (2^0): the GEMM loads whole tiles without a
// bounds check and adds zeros.  Both kernels are one launch, one thread per (line, block): the thread holds the block's 32 values in
// registers, takes (quantize) or loads (pack) the block's scale, runs the element step of lq_mx.hpp -- GroupStep<.., GroupMxParams>,
// the step of lq_fq_forward_mx, not a restatement -- and stores the fragment with one or two 16-byte stores.  The dynamic scale is
// lq_scale_init.hpp's init_take / init_raw / init_final, the rule lq_scale_init_mx runs.
#ifndef LQ_MX_OPERAND_HPP_
#define LQ_MX_OPERAND_HPP_
#include "lq_mx.hpp"
#include "lq_scale_init.hpp"

namespace lq {

constexpr int kMxBlockLen = 32;       // elements of an MX block
constexpr int kMxTileLines = 16;      // lines of an operand tile
constexpr int kMxTileK = 128;         // K of an operand tile: four blocks

struct MxOperandParams {
    GroupMxParams mp;         // g.P, g.s (pack), g.lo / g.hi and the format; the geometry fields of g are not read
    InitParams ip;            // quantize: emax, mm_frac, min_value
    uint8_t* codes;
    uint8_t* scales;
    int64_t line_stride, k_stride;        // of P, in elements
    int64_t s_line_stride, s_blk_stride;  // of s (pack), in elements
    int32_t L, K, nbk;        // nbk = ceil(K / 32)
    int32_t LT, KT, KG;
};

// byte offset of the code of element k of line ln (fp4: of the byte that holds it); 16 consecutive k from a multiple of 16 are
// 16 (fp8) or 8 (fp4) consecutive bytes
__host__ __device__ __forceinline__ int64_t mx_code_offset(int32_t KT, bool fp4, int32_t ln, int32_t k) {
    const int64_t tile = (int64_t)(ln >> 4) * KT + (k >> 7);
    const int32_t kk = k & 127;
    if (fp4) return (tile * 64 + ((kk >> 5) << 4) + (ln & 15)) * 16 + ((kk & 31) >> 1);
    return (tile * 64 + (((kk & 63) >> 4) << 4) + (ln & 15)) * 32 + ((kk >> 6) << 4) + (kk & 15);
}
__host__ __device__ __forceinline__ int64_t mx_scale_offset(int32_t KG, int32_t ln, int32_t kb) {
    const int32_t kt = kb >> 2;
    const int64_t cell = (int64_t)(ln >> 4) * KG + (kt >> 2);
    return (cell * 64 + ((kb & 3) << 4) + (ln & 15)) * 4 + (kt & 3);
}

// DYN: the scale of a block is taken from the block (METHOD: kInitMxOcp / kInitMxCover); otherwise loaded from g.s.
// VEC: k_stride == 1 and every block starts on the 16-byte grid (K % 4 == 0 follows): float4 loads.
// LINE_FAST: neighbouring threads hold neighbouring lines (the parameter's contiguous axis under axis 0), else neighbouring blocks.
template <bool DYN, int METHOD, bool FP4, bool VEC, bool LINE_FAST>
__global__ __launch_bounds__(kBlock) void k_mx_operand(const MxOperandParams op) {
    using Step = GroupStep<true, GroupMxParams>;
    const int64_t lines = (int64_t)op.LT * kMxTileLines, blocks = (int64_t)op.KT * 4;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tid >= lines * blocks) return;
    const int32_t ln = (int32_t)(LINE_FAST ? tid % lines : tid / blocks);
    const int32_t kb = (int32_t)(LINE_FAST ? tid / lines : tid % blocks);
    const bool live = ln < op.L && kb < op.nbk;
    uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t byte = 127u;
    if (live) {
        const int n = min(kMxBlockLen, op.K - kb * kMxBlockLen);
        const float* src = op.mp.g.P + (int64_t)ln * op.line_stride + (int64_t)kb * kMxBlockLen * op.k_stride;
        float x[kMxBlockLen];
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < kMxBlockLen; j += 4) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j < n) v = *reinterpret_cast<const float4*>(src + j);
                x[j] = v.x; x[j + 1] = v.y; x[j + 2] = v.z; x[j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kMxBlockLen; ++j) x[j] = j < n ? src[(int64_t)j * op.k_stride] : 0.f;
        }
        float s;
        if constexpr (DYN) {
            InitAcc a{0.f, 0.f, 0.0, 0u};      // the zeros past n change neither maximum
#pragma unroll
            for (int j = 0; j < kMxBlockLen; ++j) init_take<METHOD>(x[j], a);
            s = init_final(op.ip, init_raw<METHOD>(op.ip, a, n), a.bad);
        } else {
            s = op.mp.g.s[(int64_t)ln * op.s_line_stride + (int64_t)kb * op.s_blk_stride];
        }
        const Ctx c = Step::ctx(op.mp, s);
        byte = (c.s != c.s) ? 255u : (__float_as_uint(c.s) >> 23);      // s_eff is a power of two in [2^-126, 2^127], or NaN
#pragma unroll
        for (int j = 0; j < kMxBlockLen; ++j) {
            const float q = Step::quant(op.mp, c, div_by_uniform(x[j], c));
            const uint32_t code = j < n ? mx_code_bits(q, op.mp.M, op.mp.emin, op.mp.bits) : 0u;
            if constexpr (FP4) w[j >> 3] |= code << (4 * (j & 7));
            else w[j >> 2] |= code << (8 * (j & 3));
        }
    }
    // fp4: the block is its lane's whole fragment; fp8: its two halves of 16 are halves of the fragments of two lanes
    *reinterpret_cast<uint4*>(op.codes + mx_code_offset(op.KT, FP4, ln, kb * kMxBlockLen)) = make_uint4(w[0], w[1], w[2], w[3]);
    if constexpr (!FP4)
        *reinterpret_cast<uint4*>(op.codes + mx_code_offset(op.KT, false, ln, kb * kMxBlockLen + 16)) = make_uint4(w[4], w[5], w[6], w[7]);
    op.scales[mx_scale_offset(op.KG, ln, kb)] = (uint8_t)byte;
    // the bytes of the K steps between KT and 4 KG, which no step reads: written so that the buffer is a function of the input
    if ((kb >> 2) == op.KT - 1)
        for (int32_t kt = op.KT; kt < 4 * op.KG; ++kt) op.scales[mx_scale_offset(op.KG, ln, kt * 4 + (kb & 3))] = 127u;
}

// value(code) of a format given by (M, emin, bits): OCP's NaN of fp8_e4m3 (S.1111.111) and Inf / NaN of fp8_e5m2 (the top exponent)
__device__ __forceinline__ float mx_code_value(uint32_t code, int M, int emin, int bits) {
    const uint32_t mag = code & ((1u << (bits - 1)) - 1u);
    const uint32_t ef = mag >> M, mf = mag & ((1u << M) - 1u);
    float v;
    if (ef == 0u) v = (float)mf * __uint_as_float((uint32_t)(127 + emin - M) << 23);
    else v = __uint_as_float(((ef - 1u + (uint32_t)(emin + 127)) << 23) | (mf << (23 - M)));
    if (bits == 8 && M == 3 && mag == 127u) v = __uint_as_float(0x7fc00000u);
    if (bits == 8 && M == 2 && ef == 31u) v = mf == 0u ? __builtin_inff() : __uint_as_float(0x7fc00000u);
    return (code >> (bits - 1)) ? -v : v;
}

// 2^(byte - 127); byte 255 is NaN, byte 0 the subnormal 2^-127
__device__ __forceinline__ float mx_scale_value(uint32_t byte) {
    return byte == 255u ? __uint_as_float(0x7fc00000u) : (byte == 0u ? __uint_as_float(0x00400000u) : __uint_as_float(byte << 23));
}

struct MxDecodeParams {
    const uint8_t* codes;
    const uint8_t* scales;
    float* out;
    int32_t L, K, KT, KG;
    int32_t M, emin, bits;
};

__global__ __launch_bounds__(kBlock) void k_mx_operand_decode(const MxDecodeParams dp) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)dp.L * dp.K) return;
    const int32_t ln = (int32_t)(i / dp.K), k = (int32_t)(i % dp.K);
    const int32_t kb = k >> 5, j = k & 31;
    uint32_t code;
    if (dp.bits == 4) code = (dp.codes[mx_code_offset(dp.KT, true, ln, k)] >> (4 * (j & 1))) & 15u;
    else code = dp.codes[mx_code_offset(dp.KT, false, ln, k)];
    dp.out[i] = mx_code_value(code, dp.M, dp.emin, dp.bits) * mx_scale_value(dp.scales[mx_scale_offset(dp.KG, ln, kb)]);
}

}  // namespace lq

#endif
