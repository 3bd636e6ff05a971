// lq_i8_gemm_quant.hpp -- the int8 GEMM with an operand-out epilogue (lq_hip.h: lq_i8_gemm_quantize)
//
// The product of lq_i8_gemm.hpp, but what leaves the wave is the NEXT layer's operand: act(Y + bias) quantised per row and block of
// 64 along n, in the layout of lq_i8_operand.hpp for an operand of L = M lines over K' = N with scale blocks of 64.  lq_i8_gemm's Y
// is a function of the operands alone (exact int32 sums per period, then the stated fp32 roundings in ascending period order), so
// this kernel is free in its tiling and still computes that Y bit for bit.
//
// A wave owns 1 x 4 result tiles, 16 rows by 64 columns of Y: one K' step of the output operand, and one scale block of each of its
// rows.  A thread block is four such waves, 64 x 64 like k_i8_gemm's.  Per K step the wave loads one fragment of A and four of B
// (the four waves of a block ask for the same four, which the cache serves) and issues four instructions.  A row's 64 values then
// sit in the 16 lanes that share (lane >> 4), four per lane: its absmax partials (lq_scale_init.hpp: two maxima and an OR, exact in
// any order) merge by four DPP steps -- no LDS, no barrier, so a wave past the last row tile simply returns.  The scale and the
// element step are lq_i8_operand_quantize's own device functions; a quad's 4 x 4 bytes are transposed in registers
// (lq_mx_gemm.hpp: mx_quad_gather) so that a lane stores one dword per tile, and one lane of sixteen stores a row's scale.
// Along n the grid spans the padded operand, 64 ceil(N / 64) columns: a tile past B's last one reads the last one again (as
// k_i8_gemm's clamped second tile does) and what it holds is masked to +0, so the padding is written and no memset is needed.
#ifndef LQ_I8_GEMM_QUANT_HPP_
#define LQ_I8_GEMM_QUANT_HPP_
#include "lq_i8_gemm.hpp"
#include "lq_mx_gemm.hpp"

namespace lq {

struct I8GemmQuantParams {
    I8GemmParams g;           // Y and ldy are not read
    GroupParams gp;           // lo = -127, hi = 127; nothing else is read
    InitParams ip;            // lo, hi, min_value
    uint8_t* codes;
    float* scales;            // [OKT][16 MT]
    int32_t act;              // lq_mx_activation
    int32_t OKT;              // K steps of the output operand (K' = N), and its scale blocks
};

template <int CTRL>
__device__ __forceinline__ void i8_merge_dpp(InitAcc& a) {
    init_merge<LQ_INIT_ABSMAX>(a, __uint_as_float(mx_dpp<CTRL>(__float_as_uint(a.f0))), __uint_as_float(mx_dpp<CTRL>(__float_as_uint(a.f1))),
                               0.0, mx_dpp<CTRL>(a.bad));
}

struct I8GemmQuantAffineParams : I8GemmQuantParams {
    const float* b_offsets;   // [b_nbs][16 NT], the layout of b_scales
};

// AFF: k_i8_gemm<true>'s offset term in this kernel's tiling -- one more instruction per K step for the wave's one A tile (5 instead
// of 4), and at a period's end c once per row, then one product and one add per element
template <bool AFF>
__global__ __launch_bounds__(kBlock) void k_i8_gemm_quantize(const std::conditional_t<AFF, I8GemmQuantAffineParams, I8GemmQuantParams> p) {
    using Step = GroupStep<true, GroupParams>;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int32_t mt = (int32_t)blockIdx.y * 4 + wave;
    const int32_t nt0 = (int32_t)blockIdx.x * 4;       // below NT: the grid has ceil(N / 64) blocks along n
    if (mt >= p.g.MT) return;                          // wave-uniform; the kernel has no barrier
    int32_t nt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) nt[j] = min(nt0 + j, p.g.NT - 1);

    i8_v4i acc[4];
    float y[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = i8_v4i{0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) y[j][r] = 0.f;
    }

    // the lane's scales of the running period, as k_i8_gemm holds them: rows 4 (lane >> 4) + r of A's tile, column (lane & 15) of B's
    const float* sa_base = p.g.a_scales + mt * kI8TileLines + (lane >> 4) * 4;
    const float* sb_base[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sb_base[j] = p.g.b_scales + nt[j] * kI8TileLines + (lane & 15);
    const int64_t a_row = (int64_t)p.g.MT * kI8TileLines, b_row = (int64_t)p.g.NT * kI8TileLines;
    int32_t ia = 0, ib = 0, ca = 0, cb = 0;            // scale block of the running period and periods spent in it
    float4 sa = *reinterpret_cast<const float4*>(sa_base);
    float sb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sb[j] = sb_base[j][0];
    [[maybe_unused]] i8_v4i racc = i8_v4i{0, 0, 0, 0};      // AFF: the row sums of A's tile
    [[maybe_unused]] const float* ob_base[4] = {nullptr, nullptr, nullptr, nullptr};
    [[maybe_unused]] float ob[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (AFF) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ob_base[j] = p.b_offsets + nt[j] * kI8TileLines + (lane & 15);
            ob[j] = ob_base[j][0];
        }
    }

    i8_v4i a, an, b[4], bn[4];
    an = i8_load_frag(p.g.a_codes, p.g.KT, mt, 0, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j) bn[j] = i8_load_frag(p.g.b_codes, p.g.KT, nt[j], 0, lane);
    int32_t left = p.g.ps;
    for (int32_t kt = 0; kt < p.g.KT; ++kt) {
        // take the fragments requested a step ago, request the next step's (the last step asks for itself again), multiply
        const int32_t ktn = min(kt + 1, p.g.KT - 1);
        a = an;
        an = i8_load_frag(p.g.a_codes, p.g.KT, mt, ktn, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b[j] = bn[j];
            bn[j] = i8_load_frag(p.g.b_codes, p.g.KT, nt[j], ktn, lane);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[j], acc[j], 0, 0, 0);
        if constexpr (AFF) racc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, i8_ones_frag(), racc, 0, 0, 0);
        if (--left == 0 || kt == p.g.KT - 1) {         // kernel-uniform: the period ends; lq_i8_gemm's three roundings
            const float sar[4] = {sa.x, sa.y, sa.z, sa.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float t = __fmul_rn(sar[r], sb[j]);
                    y[j][r] = __fadd_rn(y[j][r], __fmul_rn((float)acc[j][r], t));
                }
                acc[j] = i8_v4i{0, 0, 0, 0};
            }
            if constexpr (AFF) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float c = __fmul_rn((float)racc[r], sar[r]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[j][r] = __fadd_rn(y[j][r], __fmul_rn(c, ob[j]));
                }
                racc = i8_v4i{0, 0, 0, 0};
            }
            left = p.g.ps;
            if (++ca == p.g.a_every) { ca = 0; ++ia; }
            if (++cb == p.g.b_every) { cb = 0; ++ib; }
            if (kt != p.g.KT - 1) {
                sa = *reinterpret_cast<const float4*>(sa_base + ia * a_row);
#pragma unroll
                for (int j = 0; j < 4; ++j) sb[j] = sb_base[j][ib * b_row];
                if constexpr (AFF) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) ob[j] = ob_base[j][ib * b_row];
                }
            }
        }
    }

    // bias, activation, and +0 for what lies past M or N (n from nt0 + j: a clamped tile holds a copy of the last one)
    const int col = lane & 15, g4 = (lane >> 4) * 4, q = lane & 3;
    bool live_n[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t n = (nt0 + j) * kI8TileLines + col;
        live_n[j] = n < p.g.N;
        const float bv = (p.g.bias && live_n[j]) ? p.g.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int32_t m = mt * kI8TileLines + g4 + r;
            float v = p.g.bias ? __fadd_rn(y[j][r], bv) : y[j][r];
            if (p.act == LQ_ACT_RELU) v = v > 0.f ? v : (v != v ? v : 0.f);
            y[j][r] = (live_n[j] && m < p.g.M) ? v : 0.f;
        }
    }

    const int32_t kb = (int32_t)blockIdx.x;            // the scale block, and the K step, of the output operand
    const int64_t lines = (int64_t)p.g.MT * kI8TileLines;
    uint32_t w[4] = {0u, 0u, 0u, 0u};                  // the lane's codes of tile j, row r in byte r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int32_t m = mt * kI8TileLines + g4 + r;
        const bool live_m = m < p.g.M;
        InitAcc a4{0.f, 0.f, 0.0, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) init_take<LQ_INIT_ABSMAX>(y[j][r], a4);      // a masked +0 changes neither maximum
        i8_merge_dpp<0xb1>(a4);                        // lane ^ 1
        i8_merge_dpp<0x4e>(a4);                        // lane ^ 2
        i8_merge_dpp<0x141>(a4);                       // the other quad of the eight
        i8_merge_dpp<0x140>(a4);                       // the other eight of the sixteen
        const float s = live_m ? init_final(p.ip, init_raw<LQ_INIT_ABSMAX>(p.ip, a4, kI8TileK), a4.bad) : 1.0f;
        const Ctx c = Step::ctx(p.gp, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float qv = Step::quant(p.gp, c, div_by_uniform(y[j][r], c));
            const uint32_t code = (live_n[j] && live_m) ? i8_view_byte(Step::view(p.gp, qv)) : 0u;
            w[j] |= code << (8 * r);
        }
        if (col == r) p.scales[(int64_t)kb * lines + m] = s;      // one lane of the sixteen per row
    }
    // lane q of a quad stores row g4 + q: the quad's four columns of it, four consecutive bytes of the fragment
    const int32_t ms = mt * kI8TileLines + g4 + q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t k0 = (nt0 + j) * kI8TileLines + (col & ~3);
        *reinterpret_cast<uint32_t*>(p.codes + i8_code_offset(p.OKT, ms, k0)) = mx_quad_gather(w[j], q);
    }
}

}  // namespace lq

#endif
