// lq_i8_gemm.hpp -- Y = A B^T (+ bias) of two packed int8 operands on the int8 matrix instruction (lq_hip.h: lq_i8_gemm)
//
// One v_mfma_i32_16x16x64_i8 multiplies a 16-line tile of A by a 16-line tile of B over 64 k into int32: lane l supplies line
// (l & 15) and the 16 bytes of its fragment (lq_i8_operand.hpp), one 16-byte load, no LDS.  The result tile has column (l & 15) on
// the lane and rows 4 (l >> 4) + r in its four registers, as every 16x16 form.
//
// The shape is k_mx_gemm's: a wave owns 2 x 2 result tiles (32 x 32 of Y), a block of four waves 64 x 64; per K step the wave
// loads two fragments of each operand and issues four instructions, each fragment used twice from registers; the fragments of step
// k + 1 are requested before the instructions of step k.  The operands are padded with zero codes to whole tiles, and a wave whose
// second tile lies past the operand's last one reads the last one again: no load is bounds-checked.  Only the store of Y is masked.
//
// The integer sums are exact, so the result has a bit-exact definition (lq_hip.h).  A PERIOD is a maximal run of k on which neither
// operand's scale changes: `ps` K steps, kernel-uniform.  At the end of a period (and of K) the four int32 accumulators are
// converted (v_cvt_f32_i32, nearest even), multiplied by t = RN(sa * sb) and added into four fp32 accumulators, three roundings
// stated with __fmul_rn / __fadd_rn so that no build contracts them, and zeroed.  The scales of a period are requested when it
// begins: a lane needs one float4 of A's scale row per tile (its four rows) and one float of B's (its column).
#ifndef LQ_I8_GEMM_HPP_
#define LQ_I8_GEMM_HPP_
#include "lq_i8_operand.hpp"

namespace lq {

typedef int i8_v4i __attribute__((ext_vector_type(4)));

struct I8GemmParams {
    const uint8_t* a_codes;
    const float* a_scales;    // [a_nbs][16 MT]
    const uint8_t* b_codes;
    const float* b_scales;    // [b_nbs][16 NT]
    const float* bias;        // [N] or NULL
    float* Y;
    int64_t ldy;
    int32_t M, N;
    int32_t MT, NT, KT;       // tiles of 16 lines, K steps of 64
    int32_t ps;               // K steps per period
    int32_t a_every, b_every; // periods per scale block of A / B (INT32_MAX: one scale per line)
};

__device__ __forceinline__ i8_v4i i8_load_frag(const uint8_t* codes, int32_t KT, int32_t lt, int32_t kt, int lane) {
    const uint4 v = *reinterpret_cast<const uint4*>(codes + (((int64_t)lt * KT + kt) * 64 + lane) * 16);
    i8_v4i f;
    f[0] = (int)v.x; f[1] = (int)v.y; f[2] = (int)v.z; f[3] = (int)v.w;
    return f;
}

// B with an offset per (line, scale block) (lq_hip.h: lq_i8_gemm_affine): W = q s + b adds, per period, RN(c_p * ob[n][p]) with
// c_p = RN((float)R_p * sa[m][p]) and R_p the exact row sum of A's codes over the period.
struct I8GemmAffineParams : I8GemmParams {
    const float* b_offsets;   // [b_nbs][16 NT], the layout of b_scales
};

// the B fragment whose 64 x 16 codes are all 1: the instruction then sums A's codes over the step, and the result tile holds that
// row sum for rows 4 (lane >> 4) + r in register r of every lane -- the layout of y[..][..][r], no cross-lane step
__device__ __forceinline__ i8_v4i i8_ones_frag() { return i8_v4i{0x01010101, 0x01010101, 0x01010101, 0x01010101}; }

// AFF false: the symmetric product.  AFF true: one more instruction per A tile and K step for the row sums (6 per step instead of
// 4), and at a period's end c once per row, then one product and one add per element, after the symmetric term.  B's offsets are
// loaded where its scales are, from the same index.
template <bool AFF>
__global__ __launch_bounds__(kBlock) void k_i8_gemm(const std::conditional_t<AFF, I8GemmAffineParams, I8GemmParams> p) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int32_t mt0 = ((int32_t)blockIdx.y * 2 + (wave & 1)) * 2;
    const int32_t nt0 = ((int32_t)blockIdx.x * 2 + (wave >> 1)) * 2;
    if (mt0 >= p.MT || nt0 >= p.NT) return;      // wave-uniform; the kernel has no barrier
    const int32_t mt[2] = {mt0, min(mt0 + 1, p.MT - 1)};
    const int32_t nt[2] = {nt0, min(nt0 + 1, p.NT - 1)};

    i8_v4i acc[2][2];
    float y[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc[i][j] = i8_v4i{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) y[i][j][r] = 0.f;
        }
    [[maybe_unused]] i8_v4i racc[2] = {i8_v4i{0, 0, 0, 0}, i8_v4i{0, 0, 0, 0}};      // AFF: the row sums of A's tiles
    [[maybe_unused]] const float* ob_base[2] = {nullptr, nullptr};
    [[maybe_unused]] float ob[2] = {0.f, 0.f};
    if constexpr (AFF) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            ob_base[j] = p.b_offsets + nt[j] * kI8TileLines + (lane & 15);
            ob[j] = ob_base[j][0];
        }
    }

    // the lane's scales of the running period: rows 4 (lane >> 4) + r of A's tiles, column (lane & 15) of B's
    const float* sa_base[2];
    const float* sb_base[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        sa_base[i] = p.a_scales + mt[i] * kI8TileLines + (lane >> 4) * 4;
        sb_base[i] = p.b_scales + nt[i] * kI8TileLines + (lane & 15);
    }
    const int64_t a_row = (int64_t)p.MT * kI8TileLines, b_row = (int64_t)p.NT * kI8TileLines;
    int32_t ia = 0, ib = 0, ca = 0, cb = 0;       // scale block of the running period and periods spent in it
    float4 sa[2];
    float sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        sa[i] = *reinterpret_cast<const float4*>(sa_base[i]);
        sb[i] = sb_base[i][0];
    }

    i8_v4i a[2], b[2], an[2], bn[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        an[i] = i8_load_frag(p.a_codes, p.KT, mt[i], 0, lane);
        bn[i] = i8_load_frag(p.b_codes, p.KT, nt[i], 0, lane);
    }
    int32_t left = p.ps;
    for (int32_t kt = 0; kt < p.KT; ++kt) {
        // take the fragments requested a step ago, request the next step's (the last step asks for itself again), multiply
        const int32_t ktn = min(kt + 1, p.KT - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = an[i];
            b[i] = bn[i];
            an[i] = i8_load_frag(p.a_codes, p.KT, mt[i], ktn, lane);
            bn[i] = i8_load_frag(p.b_codes, p.KT, nt[i], ktn, lane);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
        if constexpr (AFF) {
#pragma unroll
            for (int i = 0; i < 2; ++i) racc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], i8_ones_frag(), racc[i], 0, 0, 0);
        }
        if (--left == 0 || kt == p.KT - 1) {      // kernel-uniform: the period ends
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float sar[4] = {sa[i].x, sa[i].y, sa[i].z, sa[i].w};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float t = __fmul_rn(sar[r], sb[j]);
                        y[i][j][r] = __fadd_rn(y[i][j][r], __fmul_rn((float)acc[i][j][r], t));
                    }
                    acc[i][j] = i8_v4i{0, 0, 0, 0};
                }
                if constexpr (AFF) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float c = __fmul_rn((float)racc[i][r], sar[r]);
#pragma unroll
                        for (int j = 0; j < 2; ++j) y[i][j][r] = __fadd_rn(y[i][j][r], __fmul_rn(c, ob[j]));
                    }
                    racc[i] = i8_v4i{0, 0, 0, 0};
                }
            }
            left = p.ps;
            if (++ca == p.a_every) { ca = 0; ++ia; }
            if (++cb == p.b_every) { cb = 0; ++ib; }
            if (kt != p.KT - 1) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    sa[i] = *reinterpret_cast<const float4*>(sa_base[i] + ia * a_row);
                    sb[i] = sb_base[i][ib * b_row];
                    if constexpr (AFF) ob[i] = ob_base[i][ib * b_row];
                }
            }
        }
    }

    // result tile: column (lane & 15) on the lane, rows 4 (lane >> 4) + r in the registers
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int32_t n = (nt0 + j) * kI8TileLines + (lane & 15);
        if (n >= p.N) continue;
        const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int32_t m = (mt0 + i) * kI8TileLines + (lane >> 4) * 4 + r;
                if (m < p.M) p.Y[(int64_t)m * p.ldy + n] = p.bias ? __fadd_rn(y[i][j][r], bv) : y[i][j][r];
            }
    }
}

}  // namespace lq

#endif
