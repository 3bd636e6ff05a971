// lq_mx_gemm.hpp -- Y = A B^T (+ bias) of two packed MX operands on the block-scaled matrix instruction (lq_hip.h: lq_mx_gemm)
//
// One v_mfma_scale_f32_16x16x128_f8f6f4 multiplies a 16-line tile of A by a 16-line tile of B over 128 K: lane l supplies line
// (l & 15), 32 elements of the K step (which ones depends on the element width: lq_mx_operand.hpp) and the E8M0 byte of block
// (l >> 4) -- the fragment order lq_mx_operand.hpp stores, so a fragment is one (fp4) or two (fp8) 16-byte loads and no LDS is
// involved.  The result tile has column (l & 15) on the lane and rows 4 (l >> 4) + r in its four registers, as every 16x16 form.
//
// A wave owns 2 x 2 result tiles (32 x 32 of Y, four independent accumulators), a block of four waves 64 x 64.  Per K step the wave
// loads two fragments of each operand and issues four instructions, each fragment used twice from registers; the fragments of step
// k + 1 are requested before the instructions of step k.  A lane's scale dword covers four K steps; the op-sel immediates pick the
// byte, so the K loop is unrolled by four.  The element formats are the immediates cbsz / blgp: template parameters.
// The operands are padded with zero codes to whole tiles, and a wave whose second tile lies past the operand's last one reads the
// last one again: no load is bounds-checked.  Only the store of Y is masked.
#ifndef LQ_MX_GEMM_HPP_
#define LQ_MX_GEMM_HPP_
#include "lq_mx_operand.hpp"

namespace lq {

typedef int mx_v8i __attribute__((ext_vector_type(8)));
typedef float mx_v4f __attribute__((ext_vector_type(4)));

// the instruction's format immediates (cbsz for A, blgp for B): 0 fp8 e4m3, 1 fp8 e5m2, 4 fp4 e2m1
__host__ __device__ constexpr int mx_hw_format(int format) {
    return format == LQ_ELEM_FP8_E4M3 ? 0 : (format == LQ_ELEM_FP8_E5M2 ? 1 : 4);
}

struct MxGemmParams {
    const uint8_t* a_codes;
    const uint8_t* a_scales;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;        // [N] or NULL
    float* Y;
    int64_t ldy;
    int32_t M, N;
    int32_t MT, NT, KT, KG;   // tiles of 16 lines, K steps of 128, scale dwords per lane
};

// the fragment of `lane` in tile (lt, kt): an fp4 fragment fills the first four operand registers
template <int FORMAT>
__device__ __forceinline__ mx_v8i mx_load_frag(const uint8_t* codes, int32_t KT, int32_t lt, int32_t kt, int lane) {
    constexpr bool FP4 = FORMAT == LQ_ELEM_FP4_E2M1;
    const uint4* src = reinterpret_cast<const uint4*>(codes + (((int64_t)lt * KT + kt) * 64 + lane) * (FP4 ? 16 : 32));
    const uint4 lo = src[0];
    uint4 hi = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (!FP4) hi = src[1];
    mx_v8i f;
    f[0] = (int)lo.x; f[1] = (int)lo.y; f[2] = (int)lo.z; f[3] = (int)lo.w;
    f[4] = (int)hi.x; f[5] = (int)hi.y; f[6] = (int)hi.z; f[7] = (int)hi.w;
    return f;
}

__device__ __forceinline__ int mx_load_scale(const uint8_t* scales, int32_t KG, int32_t lt, int32_t kg, int lane) {
    return reinterpret_cast<const int*>(scales)[((int64_t)lt * KG + kg) * 64 + lane];
}

// the four instructions of one K step; U = K step mod 4 selects the byte of the scale dwords
template <int FA, int FB, int U>
__device__ __forceinline__ void mx_mfma_2x2(mx_v4f (&acc)[2][2], const mx_v8i (&a)[2], const mx_v8i (&b)[2], const int (&sa)[2],
                                            const int (&sb)[2]) {
    constexpr int CBSZ = mx_hw_format(FA), BLGP = mx_hw_format(FB);      // immediates of the instruction
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[i][j], CBSZ, BLGP, U, sa[i], U, sb[j]);
}

template <int FA, int FB>
__global__ __launch_bounds__(kBlock) void k_mx_gemm(const MxGemmParams p) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int32_t mt0 = ((int32_t)blockIdx.y * 2 + (wave & 1)) * 2;
    const int32_t nt0 = ((int32_t)blockIdx.x * 2 + (wave >> 1)) * 2;
    if (mt0 >= p.MT || nt0 >= p.NT) return;      // wave-uniform; the kernel has no barrier
    const int32_t mt[2] = {mt0, min(mt0 + 1, p.MT - 1)};
    const int32_t nt[2] = {nt0, min(nt0 + 1, p.NT - 1)};

    mx_v4f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mx_v4f{0.f, 0.f, 0.f, 0.f};

    mx_v8i a[2], b[2], an[2], bn[2];
    int sa[2], sb[2], san[2], sbn[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        an[i] = mx_load_frag<FA>(p.a_codes, p.KT, mt[i], 0, lane);
        bn[i] = mx_load_frag<FB>(p.b_codes, p.KT, nt[i], 0, lane);
        san[i] = mx_load_scale(p.a_scales, p.KG, mt[i], 0, lane);
        sbn[i] = mx_load_scale(p.b_scales, p.KG, nt[i], 0, lane);
    }
// one K step: take the fragments requested a step ago, request the next step's (the last step asks for itself again), multiply
#define LQ_MX_GEMM_STEP(U)                                                     \
    if (kg * 4 + (U) < p.KT) {                                                 \
        const int32_t ktn = min(kg * 4 + (U) + 1, p.KT - 1);                   \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                        \
            a[i] = an[i];                                                      \
            b[i] = bn[i];                                                      \
            an[i] = mx_load_frag<FA>(p.a_codes, p.KT, mt[i], ktn, lane);       \
            bn[i] = mx_load_frag<FB>(p.b_codes, p.KT, nt[i], ktn, lane);       \
        }                                                                      \
        mx_mfma_2x2<FA, FB, (U)>(acc, a, b, sa, sb);                           \
    }
    for (int32_t kg = 0; kg < p.KG; ++kg) {
        const int32_t kgn = min(kg + 1, p.KG - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            sa[i] = san[i];
            sb[i] = sbn[i];
            san[i] = mx_load_scale(p.a_scales, p.KG, mt[i], kgn, lane);
            sbn[i] = mx_load_scale(p.b_scales, p.KG, nt[i], kgn, lane);
        }
        LQ_MX_GEMM_STEP(0)
        LQ_MX_GEMM_STEP(1)
        LQ_MX_GEMM_STEP(2)
        LQ_MX_GEMM_STEP(3)
    }
#undef LQ_MX_GEMM_STEP

    // result tile: column (lane & 15) on the lane, rows 4 (lane >> 4) + r in the registers
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int32_t n = (nt0 + j) * kMxTileLines + (lane & 15);
        if (n >= p.N) continue;
        const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int32_t m = (mt0 + i) * kMxTileLines + (lane >> 4) * 4 + r;
                if (m < p.M) p.Y[(int64_t)m * p.ldy + n] = p.bias ? acc[i][j][r] + bv : acc[i][j][r];
            }
    }
}

}  // namespace lq

#endif
