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
// k_mx_gemm_quantize (lq_hip.h: lq_mx_gemm_quantize) is the same product with an operand-out epilogue: see the end of the file.
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

// k_mx_gemm's K loop for the kernel below: acc += A[mt[i]] B[nt[j]]^T, the same fragments, the same four instructions per step, in
// ascending K, so the accumulators are k_mx_gemm's bit for bit.  A copy, not a function both kernels call: with the loop moved into a
// function k_mx_gemm's nine instantiations compile to other instruction streams (up to 8 more VGPRs), so its text stays as it shipped
template <int FA, int FB>
__device__ __forceinline__ void mx_gemm_accumulate(const MxGemmParams& p, const int32_t (&mt)[2], const int32_t (&nt)[2], const int lane,
                                                   mx_v4f (&acc)[2][2]) {
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
}

// ---- operand-out epilogue (lq_hip.h: lq_mx_gemm_quantize) ----
// The same product, but what leaves the wave is the NEXT layer's operand: act(Y + bias) quantised per block of 32 along n, in the
// layout of lq_mx_operand.hpp for an operand of L = M lines over K' = N.  A wave's 32 x 32 of Y starts on an even tile, so for each
// of its 32 rows it holds exactly one block: the row's values sit in the 16 lanes that share (lane >> 4), two per lane.  The block's
// scale is lq_scale_init.hpp's rule (two maxima and an OR: order-free) merged over those 16 lanes by four DPP steps, the codes are
// the element step of lq_mx.hpp, and a quad's 4 x 4 bytes are transposed in registers so that a lane stores one dword (fp8) or one
// short (fp4) per tile.  No LDS, no fp32 Y.  The grid spans the whole padded operand (128 KT' columns): waves past B's last tile
// skip the K loop and write the padding, so the buffers are a function of the input without a memset.
struct MxGemmQuantParams {
    MxGemmParams g;           // Y and ldy are not read
    GroupMxParams mp;         // the output format: g.lo / g.hi, M, emin, bits, E8M0; nothing else of g is read
    InitParams ip;            // emax, mm_frac, min_value of the output format
    uint8_t* codes;
    uint8_t* scales;
    int32_t act;              // lq_mx_activation
    int32_t cover;            // LQ_MX_INIT_COVER
    int32_t OKT, OKG;         // K steps and scale dwords of the output operand (K' = N)
};

// lane l takes v of the lane a DPP control names: quad_perm (0x00 .. 0xff), row_half_mirror (0x141), row_mirror (0x140).  Every lane
// of the wave is active where this is called
template <int CTRL>
__device__ __forceinline__ uint32_t mx_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ void mx_merge_dpp(InitAcc& a) {
    init_merge<kInitMxOcp>(a, __uint_as_float(mx_dpp<CTRL>(__float_as_uint(a.f0))), __uint_as_float(mx_dpp<CTRL>(__float_as_uint(a.f1))),
                           0.0, mx_dpp<CTRL>(a.bad));
}
// byte q of the words of the quad's four lanes, lane u's in byte u: the 4 x 4 byte transpose, q = lane & 3
__device__ __forceinline__ uint32_t mx_quad_gather(uint32_t w, int q) {
    const int sh = 8 * q;
    return ((mx_dpp<0x00>(w) >> sh) & 0xffu) | (((mx_dpp<0x55>(w) >> sh) & 0xffu) << 8) | (((mx_dpp<0xaa>(w) >> sh) & 0xffu) << 16) |
           (((mx_dpp<0xff>(w) >> sh) & 0xffu) << 24);
}

template <int FA, int FB, bool OUT_FP4>
__global__ __launch_bounds__(kBlock) void k_mx_gemm_quantize(const MxGemmQuantParams p) {
    using Step = GroupStep<true, GroupMxParams>;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int32_t mt0 = ((int32_t)blockIdx.y * 2 + (wave & 1)) * 2;
    const int32_t nt0 = ((int32_t)blockIdx.x * 2 + (wave >> 1)) * 2;      // even: the wave's 32 columns are block nt0 / 2
    if (mt0 >= p.g.MT) return;                  // wave-uniform; the kernel has no barrier
    const bool has_k = nt0 < p.g.NT;            // wave-uniform: a wave past B's last tile writes padding only

    mx_v4f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mx_v4f{0.f, 0.f, 0.f, 0.f};
    if (has_k) {
        const int32_t mt[2] = {mt0, min(mt0 + 1, p.g.MT - 1)};
        const int32_t nt[2] = {nt0, min(nt0 + 1, p.g.NT - 1)};
        mx_gemm_accumulate<FA, FB>(p.g, mt, nt, lane, acc);
    }

    // bias, activation, and +0 for what lies past M or N (n from nt0 + j: a clamped second tile holds a copy of the last one)
    const int col = lane & 15, g4 = (lane >> 4) * 4, q = lane & 3;
    bool live_n[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int32_t n = (nt0 + j) * kMxTileLines + col;
        live_n[j] = n < p.g.N;
        const float bv = (p.g.bias && live_n[j]) ? p.g.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int32_t m = (mt0 + i) * kMxTileLines + g4 + r;
                float v = p.g.bias ? acc[i][j][r] + bv : acc[i][j][r];
                if (p.act == LQ_ACT_RELU) v = v > 0.f ? v : (v != v ? v : 0.f);
                acc[i][j][r] = (live_n[j] && m < p.g.M) ? v : 0.f;
            }
    }

    const int32_t kb = nt0 >> 1;                // the block of the output operand
    const bool idle = (kb >> 2) == p.OKT - 1;   // this wave also writes the scale bytes of the K steps OKT .. 4 OKG - 1
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (mt0 + i >= p.g.MT) break;           // wave-uniform: no such lines in the operand
        uint32_t w[2] = {0u, 0u};               // the lane's codes of tile (i, j), row r in byte r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int32_t m = (mt0 + i) * kMxTileLines + g4 + r;
            InitAcc a{0.f, 0.f, 0.0, 0u};
            init_take<kInitMxOcp>(acc[i][0][r], a);      // the two rules differ in init_raw only
            init_take<kInitMxOcp>(acc[i][1][r], a);
            mx_merge_dpp<0xb1>(a);              // lane ^ 1
            mx_merge_dpp<0x4e>(a);              // lane ^ 2
            mx_merge_dpp<0x141>(a);             // the other quad of the eight
            mx_merge_dpp<0x140>(a);             // the other eight of the sixteen
            const float raw = p.cover ? init_raw<kInitMxCover>(p.ip, a, kMxBlockLen) : init_raw<kInitMxOcp>(p.ip, a, kMxBlockLen);
            const Ctx c = Step::ctx(p.mp, init_final(p.ip, raw, a.bad));
            const bool live_m = m < p.g.M;
            const uint32_t byte = !(live_m && has_k) ? 127u : ((c.s != c.s) ? 255u : (__float_as_uint(c.s) >> 23));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float qv = Step::quant(p.mp, c, div_by_uniform(acc[i][j][r], c));
                const uint32_t code = (live_n[j] && live_m) ? mx_code_bits(qv, p.mp.M, p.mp.emin, p.mp.bits) : 0u;
                w[j] |= code << (8 * r);
            }
            if (col == r) {                     // one lane of the sixteen per row
                p.scales[mx_scale_offset(p.OKG, m, kb)] = (uint8_t)byte;
                if (idle)
                    for (int32_t kt = p.OKT; kt < 4 * p.OKG; ++kt) p.scales[mx_scale_offset(p.OKG, m, kt * 4 + (kb & 3))] = 127u;
            }
        }
        // lane q of a quad stores row g4 + q: the quad's four columns of it
        const int32_t ms = (mt0 + i) * kMxTileLines + g4 + q;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int32_t k0 = (nt0 + j) * kMxTileLines + (col & ~3);
            if constexpr (OUT_FP4) {
                const uint32_t wn = mx_dpp<0xb1>(w[j]);                                    // the neighbour's nibbles
                const uint32_t b = (lane & 1) ? (wn | (w[j] << 4)) : (w[j] | (wn << 4));   // the even column is the low nibble
                const uint32_t lo = (mx_dpp<0x00>(b) >> (8 * q)) & 0xffu, hi = (mx_dpp<0xaa>(b) >> (8 * q)) & 0xffu;
                *reinterpret_cast<uint16_t*>(p.codes + mx_code_offset(p.OKT, true, ms, k0)) = (uint16_t)(lo | (hi << 8));
            } else {
                *reinterpret_cast<uint32_t*>(p.codes + mx_code_offset(p.OKT, false, ms, k0)) = mx_quad_gather(w[j], q);
            }
        }
    }
}

}  // namespace lq

#endif
