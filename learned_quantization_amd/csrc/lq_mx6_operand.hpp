// lq_mx6_operand.hpp -- packed fp6 microscaling operands (fp6_e2m3, fp6_e3m2) in the order the block-scaled matrix instruction
// consumes 6-bit data (lq_hip.h: lq_mx6_operand_bytes / lq_mx6_operand_pack / lq_mx6_operand_quantize / lq_mx6_operand_decode)
//
// The operand of lq_mx_operand.hpp with 6-bit codes: L lines by K, tiles of 16 lines by 128 K, one E8M0 byte per block of 32.  The
// scale buffer IS that file's, bit for bit (mx_scale_offset, byte 127 padding, the idle bytes).  Lane l of the wave holds line
// (l & 15) and, with g = l >> 4, the 32 consecutive k = 32 g + j of the step -- one MX block, as fp4 -- in a fragment of 192 bits:
// element j in bits 6 j .. 6 j + 5.  Read as little-endian dwords the 24 bytes are the operand registers 0 .. 5; registers 6 and 7
// are zero.  The scale byte of lane l applies to block g.
//
//   codes   [LT][KT][1536 bytes]   a tile is two planes, so that both loads of a wave are naturally aligned and contiguous:
//           bytes 0 .. 1023     [64 lanes][16]   bytes 0 .. 15 of each lane's fragment (registers 0 .. 3)
//           bytes 1024 .. 1535  [64 lanes][8]    bytes 16 .. 23 (registers 4, 5)
//   scales  [LT][KG][64 lanes][4 bytes]          lq_mx_operand.hpp's
//
// Lines past L and elements past K hold code 0 under byte 127.  One thread per (line, block), as k_mx_operand: the block's 32 values
// in registers, the scale taken (lq_scale_init.hpp's init_take / init_raw / init_final) or loaded, the element step of lq_mx.hpp and
// mx_code_bits -- called, not restated --, then six dwords assembled and stored as 16 + 8 bytes.
#ifndef LQ_MX6_OPERAND_HPP_
#define LQ_MX6_OPERAND_HPP_
#include "lq_mx_operand.hpp"

namespace lq {

constexpr int kMx6FragBytes = 24;                      // 32 codes of 6 bits
constexpr int kMx6PlaneLo = 64 * 16;                   // bytes of a tile's first plane
constexpr int kMx6TileBytes = 64 * kMx6FragBytes;      // 1536

// byte offset of the 16-byte word (HI: of the 8-byte word) of the fragment that holds block kb of line ln
template <bool HI>
__host__ __device__ __forceinline__ int64_t mx6_frag_offset(int32_t KT, int32_t ln, int32_t kb) {
    const int64_t tile = (int64_t)(ln >> 4) * KT + (kb >> 2);
    const int32_t lane = ((kb & 3) << 4) + (ln & 15);
    return tile * kMx6TileBytes + (HI ? kMx6PlaneLo + lane * 8 : lane * 16);
}
// byte offset of byte fb (0 .. 23) of that fragment
__host__ __device__ __forceinline__ int64_t mx6_byte_offset(int32_t KT, int32_t ln, int32_t kb, int32_t fb) {
    return fb < 16 ? mx6_frag_offset<false>(KT, ln, kb) + fb : mx6_frag_offset<true>(KT, ln, kb) + (fb - 16);
}

// The template parameters are k_mx_operand's: DYN takes the scale from the block (METHOD), VEC loads float4, LINE_FAST puts
// neighbouring lines on neighbouring threads (axis 0).
template <bool DYN, int METHOD, bool VEC, bool LINE_FAST>
__global__ __launch_bounds__(kBlock) void k_mx6_operand(const MxOperandParams op) {
    using Step = GroupStep<true, GroupMxParams>;
    const int64_t lines = (int64_t)op.LT * kMxTileLines, blocks = (int64_t)op.KT * 4;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tid >= lines * blocks) return;
    const int32_t ln = (int32_t)(LINE_FAST ? tid % lines : tid / blocks);
    const int32_t kb = (int32_t)(LINE_FAST ? tid / lines : tid % blocks);
    const bool live = ln < op.L && kb < op.nbk;
    uint32_t w[6] = {0u, 0u, 0u, 0u, 0u, 0u};
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
            // bits 6 j .. 6 j + 5 of the fragment: a code that starts above bit 26 of its dword continues in the next one
            constexpr int kBits = 6;
            const int dw = (kBits * j) >> 5, sh = (kBits * j) & 31;
            w[dw] |= code << sh;
            if (sh > 32 - kBits) w[dw + 1] |= code >> (32 - sh);
        }
    }
    *reinterpret_cast<uint4*>(op.codes + mx6_frag_offset<false>(op.KT, ln, kb)) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint2*>(op.codes + mx6_frag_offset<true>(op.KT, ln, kb)) = make_uint2(w[4], w[5]);
    op.scales[mx_scale_offset(op.KG, ln, kb)] = (uint8_t)byte;
    // the bytes of the K steps between KT and 4 KG, which no step reads: written so that the buffer is a function of the input
    if ((kb >> 2) == op.KT - 1)
        for (int32_t kt = op.KT; kt < 4 * op.KG; ++kt) op.scales[mx_scale_offset(op.KG, ln, kt * 4 + (kb & 3))] = 127u;
}

// one thread per element: the code's six bits lie in one or two bytes of its fragment
__global__ __launch_bounds__(kBlock) void k_mx6_operand_decode(const MxDecodeParams dp) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)dp.L * dp.K) return;
    const int32_t ln = (int32_t)(i / dp.K), k = (int32_t)(i % dp.K);
    const int32_t kb = k >> 5, bit = 6 * (k & 31);
    const int32_t fb = bit >> 3, sh = bit & 7;
    uint32_t v = dp.codes[mx6_byte_offset(dp.KT, ln, kb, fb)];
    if (sh > 2) v |= (uint32_t)dp.codes[mx6_byte_offset(dp.KT, ln, kb, fb + 1)] << 8;      // sh > 2 only below byte 23
    dp.out[i] = mx_code_value((v >> sh) & 63u, dp.M, dp.emin, dp.bits) * mx_scale_value(dp.scales[mx_scale_offset(dp.KG, ln, kb)]);
}

}  // namespace lq

#endif
