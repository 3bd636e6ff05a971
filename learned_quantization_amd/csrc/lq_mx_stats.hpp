// lq_mx_stats.hpp -- per-group statistics of the microscaling (MX) quantizer (lq_hip.h: lq_mx_stats)
//
// What lq_group_stats.hpp is for the integer grid, for the minifloat grids of lq_mx.hpp, read only: per group how many elements
// saturate on either side of +-mx, how many non-zero elements the grid turns into a zero of either sign (flushed below the smallest
// subnormal), the f64 sums of squared errors P - out and of squares P * P, and per tensor the histogram of the elements' encodings.
// Per element the arithmetic is lq_mx.hpp's forward: GroupStep<true, GroupMxParams>::ctx (s_eff and the division context), the
// group-wise quotient (fq_quot4c / fq_quot4 / div_by_uniform), mx_round, the comparison clamp, out = q * s_eff, and mx_code_bits for
// the bin -- the integer that mx_code converts for the forward's code view.
//
// Geometry, unit shapes, team widths, grid and merge order are lq_group_stats.hpp's (the host asks group_launch with no row split):
//
//   k_mx_stats_cols  (axis 0)  slot 0 adds err2 and below in slot order and emits them, slot 1 sig2 and above, slot 2 flushed, at
//                              the same time
//   k_mx_stats_rows  (axis 1)  the fixed xor butterfly carries the third count with the other four; lane 0 of the team emits
//
// Every f64 sum has one fixed order: two runs give the same bits.  No float atomics, no second stage, no workspace.  The histogram
// is the block-private array of lq_group_stats.hpp in dynamic LDS (2^bits words: 16 / 64 / 256; none when the caller wants no
// histogram), added to with LDS integer atomics and flushed bin by bin, non-zero bins only, with integer global atomics.
//
// The format enters as the kernel-uniform (M, emin, mx, bits, e8m0_mask) of GroupMxParams: the four kernels serve the five element
// formats and both scale formats.
#ifndef LQ_MX_STATS_HPP_
#define LQ_MX_STATS_HPP_
#include "lq_mx.hpp"
#include "lq_group_stats.hpp"

namespace lq {

struct MxStatsParams {
    GroupMxParams mp;      // g.P, g.s, g.lo = -mx, g.hi = mx, the geometry; M, emin, bits, e8m0_mask.  Nothing else of g is read
    uint32_t* below;
    uint32_t* above;
    uint32_t* flushed;
    double* err2;
    double* sig2;
    uint32_t* hist;        // may be NULL
    int32_t nbins;         // 2^bits where hist != NULL, else 0
};

// what one lane carries
struct MxStatsAcc {
    uint32_t below, above, flushed;
    double err2, sig2;
};

// one element: x = P, t its quotient by s_eff
__device__ __forceinline__ void mx_stats_take(const MxStatsParams& p, const Ctx& c, float x, float t, MxStatsAcc& a, const bool binned,
                                              uint32_t* sh_hist) {
    const float q0 = mx_round(t, p.mp);
    a.below += q0 < c.k0 ? 1u : 0u;      // a NaN q0 (a NaN element, or a NaN s_eff) is on neither side
    a.above += q0 > c.k1 ? 1u : 0u;
    const float q = ClipBase<true>::clampq(q0, c.k0, c.k1);
    a.flushed += ((x != 0.f) & (q == 0.f)) ? 1u : 0u;    // the grid made a zero of either sign out of a non-zero; a NaN q is not zero
    const float out = q * c.s;
    const double e = (double)x - (double)out;
    a.err2 += e * e;
    a.sig2 += (double)x * (double)x;
    if (binned && q == q) {      // q is a number: its NaN "code" 2^(E+M) - 1 is a value's code in the fp4 / fp6 formats
        const uint32_t bin = mx_code_bits(q, p.mp.M, p.mp.emin, p.mp.bits);
        if (bin < (uint32_t)p.nbins) atomicAdd(&sh_hist[bin], 1u);
    }
}

__device__ __forceinline__ void mx_stats_hist_clear(const MxStatsParams& p, const bool binned, uint32_t* sh_hist) {
    if (binned) {      // kernel-uniform
        for (int i = (int)threadIdx.x; i < p.nbins; i += kBlock) sh_hist[i] = 0u;
        __syncthreads();
    }
}

__device__ __forceinline__ void mx_stats_hist_flush(const MxStatsParams& p, const bool binned, uint32_t* sh_hist) {
    if (binned) {
        __syncthreads();
        for (int i = (int)threadIdx.x; i < p.nbins; i += kBlock) {
            const uint32_t n = sh_hist[i];
            if (n) atomicAdd(&p.hist[i], n);
        }
    }
}

template <int V, int TX>
__global__ __launch_bounds__(kBlock) void k_mx_stats_cols(const MxStatsParams p) {
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    static_assert(SLOTS >= 3, "slot 1 merges sig2 and above, slot 2 flushed");
    extern __shared__ uint32_t sh_hist[];      // p.nbins words where the caller wants the histogram, else none
    __shared__ double sh_err[SLOTS * COLS];
    __shared__ double sh_sig[SLOTS * COLS];
    __shared__ uint32_t sh_below[SLOTS * COLS];
    __shared__ uint32_t sh_above[SLOTS * COLS];
    __shared__ uint32_t sh_flushed[SLOTS * COLS];
    const GroupParams& gp = p.mp.g;
    const bool binned = p.hist != nullptr;      // kernel-uniform
    const int lx = (int)threadIdx.x % TX, slot = (int)threadIdx.x / TX;
    const int64_t c0 = ((int64_t)blockIdx.x * TX + lx) * V;
    const bool live = c0 < gp.C;      // V = 4 runs only with C % 4 == 0
    mx_stats_hist_clear(p, binned, sh_hist);
    // the trip count of the group loop is block-uniform: every thread meets every barrier
    for (int64_t g = blockIdx.y; g < gp.nb; g += gridDim.y) {
        const int64_t r0 = g * gp.gs;
        const int64_t r1 = (r0 + gp.gs < gp.R) ? r0 + gp.gs : gp.R;
        MxStatsAcc a[V];
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] = MxStatsAcc{0u, 0u, 0u, 0.0, 0.0};
        if (live) {
            Ctx c[V];
#pragma unroll
            for (int k = 0; k < V; ++k) c[k] = GroupStep<true, GroupMxParams>::ctx(p.mp, gp.s[g * gp.C + c0 + k]);
#pragma unroll 2
            for (int64_t r = r0 + slot; r < r1; r += SLOTS) {      // two rows in flight, as k_stats_cols
                const int64_t i = r * gp.C + c0;
                if constexpr (V == 4) {
                    const float4 x = *reinterpret_cast<const float4*>(gp.P + i);
                    const float4 t = fq_quot4c(x, c);
                    mx_stats_take(p, c[0], x.x, t.x, a[0], binned, sh_hist);
                    mx_stats_take(p, c[1], x.y, t.y, a[1], binned, sh_hist);
                    mx_stats_take(p, c[2], x.z, t.z, a[2], binned, sh_hist);
                    mx_stats_take(p, c[3], x.w, t.w, a[3], binned, sh_hist);
                } else {
                    const float x = gp.P[i];
                    mx_stats_take(p, c[0], x, div_by_uniform(x, c[0]), a[0], binned, sh_hist);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int j = slot * COLS + lx * V + k;
            sh_err[j] = a[k].err2;
            sh_sig[j] = a[k].sig2;
            sh_below[j] = a[k].below;
            sh_above[j] = a[k].above;
            sh_flushed[j] = a[k].flushed;
        }
        __syncthreads();
        if (slot < 2 && live) {      // slot 0: err2 and below; slot 1: sig2 and above, in the same slot order at the same time
            const double* const sh_d = slot == 0 ? sh_err : sh_sig;
            const uint32_t* const sh_u = slot == 0 ? sh_below : sh_above;
            double* const out_d = slot == 0 ? p.err2 : p.sig2;
            uint32_t* const out_u = slot == 0 ? p.below : p.above;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                double sum = sh_d[lx * V + k];
                uint32_t cnt = sh_u[lx * V + k];
#pragma unroll 2
                for (int w = 1; w < SLOTS; ++w) {      // fixed order: slot 0, 1, 2, ...
                    sum += sh_d[w * COLS + lx * V + k];
                    cnt += sh_u[w * COLS + lx * V + k];
                }
                out_d[g * gp.C + c0 + k] = sum;
                out_u[g * gp.C + c0 + k] = cnt;
            }
        } else if (slot == 2 && live) {      // slot 2: flushed
#pragma unroll
            for (int k = 0; k < V; ++k) {
                uint32_t cnt = sh_flushed[lx * V + k];
#pragma unroll 2
                for (int w = 1; w < SLOTS; ++w) cnt += sh_flushed[w * COLS + lx * V + k];
                p.flushed[g * gp.C + c0 + k] = cnt;
            }
        }
        __syncthreads();
    }
    mx_stats_hist_flush(p, binned, sh_hist);
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_mx_stats_rows(const MxStatsParams p, const int log_team) {
    extern __shared__ uint32_t sh_hist[];      // p.nbins words where the caller wants the histogram, else none
    const GroupParams& gp = p.mp.g;
    const bool binned = p.hist != nullptr;      // kernel-uniform
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const uint32_t pairs = (uint32_t)gp.R * (uint32_t)gp.nb;      // <= R * C < 2^31
    const uint32_t pair = blockIdx.x * (uint32_t)(kBlock >> log_team) + (threadIdx.x >> log_team);
    const bool live = pair < pairs;
    mx_stats_hist_clear(p, binned, sh_hist);
    MxStatsAcc a = MxStatsAcc{0u, 0u, 0u, 0.0, 0.0};
    if (live) {
        const uint32_t r = pair / (uint32_t)gp.nb, g = pair - r * (uint32_t)gp.nb;
        const int64_t base = (int64_t)r * gp.C;
        const int64_t c0 = (int64_t)g * gp.gs;
        const int64_t c1 = (c0 + gp.gs < gp.C) ? c0 + gp.gs : gp.C;
        const Ctx c = GroupStep<true, GroupMxParams>::ctx(p.mp, gp.s[pair]);
        for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {      // V = 4: gs % 4 == 0 and C % 4 == 0
            const int64_t i = base + col;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(gp.P + i);
                const float4 t = fq_quot4(x, c);
                mx_stats_take(p, c, x.x, t.x, a, binned, sh_hist);
                mx_stats_take(p, c, x.y, t.y, a, binned, sh_hist);
                mx_stats_take(p, c, x.z, t.z, a, binned, sh_hist);
                mx_stats_take(p, c, x.w, t.w, a, binned, sh_hist);
            } else {
                const float x = gp.P[i];
                mx_stats_take(p, c, x, div_by_uniform(x, c), a, binned, sh_hist);
            }
        }
    }
    for (int off = T >> 1; off > 0; off >>= 1) {      // fixed butterfly inside the aligned team; every lane of the wave takes part
        a.err2 += __shfl_xor(a.err2, off);
        a.sig2 += __shfl_xor(a.sig2, off);
        a.below += __shfl_xor(a.below, off);
        a.above += __shfl_xor(a.above, off);
        a.flushed += __shfl_xor(a.flushed, off);
    }
    if (live && lt == 0) {
        p.below[pair] = a.below;
        p.above[pair] = a.above;
        p.flushed[pair] = a.flushed;
        p.err2[pair] = a.err2;
        p.sig2[pair] = a.sig2;
    }
    mx_stats_hist_flush(p, binned, sh_hist);
}

}  // namespace lq

#endif
