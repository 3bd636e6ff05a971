// lq_group_stats.hpp -- per-group statistics of the group-wise quantizers (lq_hip.h: lq_group_stats, lq_mx_stats)
//
// What a quantizer does to a tensor under its present scales (and offsets), read only: per group how many elements the range cuts
// off below and above, the f64 sum of squared errors P - out and of squares P * P (their ratio is the group's SQNR), and per tensor
// the histogram of the clamped codes.  The microscaling grids (lq_mx_stats.hpp) count a third thing per group: the non-zero
// elements that the grid turns into a zero.
//
// There is ONE traversal body per axis, for the integer grid and the minifloat grids alike.  Geometry and unit shapes are those of
// lq_group.hpp's BACKWARD (the host asks group_launch with no row split), the bodies are siblings of lq_scale_init.hpp's:
//
//   stats_cols_body  (axis 0)  a lane keeps V fixed columns, TX lanes side by side, the 256 / TX row slots of the block split the
//                              rows of a group.  The slots' partials meet in LDS; slot 0 adds err2 and below in slot order and emits
//                              them, slot 1 does the same for sig2 and above at the same time, slot 2 for the third count.
//   stats_rows_body  (axis 1)  a team of T = 2^k <= 64 lanes per (row, group), a fixed xor butterfly (which carries the third count
//                              with the other four), lane 0 of the team emits.
//
// What depends on the grid the bodies ask of the parameter struct PT (StatsParams here, MxStatsParams in lq_mx_stats.hpp), through
// overloads in the manner of group_base:
//
//   stats_geom(p)        where P, s and R, C, gs, nb live: the struct itself, or the GroupParams inside it
//   stats_ctx(p, s)      the context of a group from its stored scale
//   stats_take(...)      one element: the grid's rounding, the counts, the two f64 terms and the bin
//   PT::kFlushed         whether the third count travels along.  What it adds (an LDS array, slot 2's merge, a fifth shuffle, a
//                        store to p.flushed) sits behind `if constexpr`
//
// and the output pointers, nbins and hist under the names both structs give them.  An offset (p.b, AFF) is the integer grid's alone.
// The kernels (k_stats_cols / k_stats_rows here, k_mx_stats_cols / k_mx_stats_rows) are wrappers that name the instantiation.
//
// Every f64 sum has one fixed order (the lane's own elements ascending, then slots 0, 1, ... or the butterfly): two runs give the
// same bits.  No float atomics, no second stage, no workspace.  The histogram is a block-private array in dynamic LDS (nbins
// words; none when the caller wants no histogram) that the lanes add to with LDS integer atomics; at the end of the block its
// non-zero bins go to the caller's with integer global atomics, which are exact in any order.
#ifndef LQ_GROUP_STATS_HPP_
#define LQ_GROUP_STATS_HPP_
#include "lq_group.hpp"

namespace lq {

constexpr int kStatsMaxBins = 4096;      // 16 KB of LDS

struct StatsParams {
    const float* P;
    const float* s;
    const float* b;        // AFF only
    float lo, hi;          // (float)qmin, (float)qmax
    int32_t qmin;
    int32_t nbins;         // qmax - qmin + 1 where hist != NULL, else 0
    uint32_t* below;
    uint32_t* above;
    double* err2;
    double* sig2;
    uint32_t* hist;        // may be NULL
    int32_t R, C, gs, nb;  // as GroupParams
    static constexpr bool kFlushed = false;
};

// what one lane carries; flushed: only where PT::kFlushed
struct StatsAcc {
    uint32_t below, above, flushed;
    double err2, sig2;
};

__device__ __forceinline__ const StatsParams& stats_geom(const StatsParams& p) { return p; }

__device__ __forceinline__ Ctx stats_ctx(const StatsParams& p, float s) {
    Ctx c;
    c.s = s;
    div_ctx(c);
    c.k0 = p.lo;
    c.k1 = p.hi;
    c.lam_hi = 0.f;
    c.sure_ok = 0;
    return c;
}

// one element: x = P, t its quotient (of x, or of x - b)
template <bool RNE, bool AFF>
__device__ __forceinline__ void stats_take(const StatsParams& p, const Ctx& c, float b, float x, float t, StatsAcc& a, const bool binned,
                                           uint32_t* sh_hist) {
    const float q0 = ClipBase<RNE>::rnd(t);
    a.below += q0 < c.k0 ? 1u : 0u;      // a NaN q0 is on neither side
    a.above += q0 > c.k1 ? 1u : 0u;
    const float q = ClipBase<RNE>::clampq(q0, c.k0, c.k1);
    float out = q * c.s;
    if constexpr (AFF) out = out + b;
    const double e = (double)x - (double)out;
    a.err2 += e * e;
    a.sig2 += (double)x * (double)x;
    if (binned && q == q) {      // q is a number: lo <= q <= hi after the clamp
        const uint32_t bin = (uint32_t)((int32_t)q - p.qmin);
        if (bin < (uint32_t)p.nbins) atomicAdd(&sh_hist[bin], 1u);
    }
}

template <class PT>
__device__ __forceinline__ void stats_hist_clear(const PT& p, const bool binned, uint32_t* sh_hist) {
    if (binned) {      // kernel-uniform
        for (int i = (int)threadIdx.x; i < p.nbins; i += kBlock) sh_hist[i] = 0u;
        __syncthreads();
    }
}

template <class PT>
__device__ __forceinline__ void stats_hist_flush(const PT& p, const bool binned, uint32_t* sh_hist) {
    if (binned) {
        __syncthreads();
        for (int i = (int)threadIdx.x; i < p.nbins; i += kBlock) {
            const uint32_t n = sh_hist[i];
            if (n) atomicAdd(&p.hist[i], n);
        }
    }
}

// The work of one block of a column kernel: every group that blockIdx.y strides to, of the column tile blockIdx.x.  RNE, AFF: the
// integer grid's rounding and offset (a minifloat grid passes true, false and reads neither)
template <bool RNE, bool AFF, int V, int TX, class PT>
__device__ __forceinline__ void stats_cols_body(const PT& p) {
    constexpr bool FL = PT::kFlushed;
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    static_assert(SLOTS >= (FL ? 3 : 2), "slot 1 merges sig2 and above, slot 2 flushed");
    extern __shared__ uint32_t sh_hist[];      // p.nbins words where the caller wants the histogram, else none
    __shared__ double sh_err[SLOTS * COLS];
    __shared__ double sh_sig[SLOTS * COLS];
    __shared__ uint32_t sh_below[SLOTS * COLS];
    __shared__ uint32_t sh_above[SLOTS * COLS];
    __shared__ uint32_t sh_flushed[FL ? SLOTS * COLS : 1];      // not referenced without the third count: no LDS
    const auto& gp = stats_geom(p);
    const bool binned = p.hist != nullptr;      // kernel-uniform
    const int lx = (int)threadIdx.x % TX, slot = (int)threadIdx.x / TX;
    const int64_t c0 = ((int64_t)blockIdx.x * TX + lx) * V;
    const bool live = c0 < gp.C;      // V = 4 runs only with C % 4 == 0
    stats_hist_clear(p, binned, sh_hist);
    // the trip count of the group loop is block-uniform: every thread meets every barrier
    for (int64_t g = blockIdx.y; g < gp.nb; g += gridDim.y) {
        const int64_t r0 = g * gp.gs;
        const int64_t r1 = (r0 + gp.gs < gp.R) ? r0 + gp.gs : gp.R;
        StatsAcc a[V];
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] = StatsAcc{0u, 0u, 0u, 0.0, 0.0};
        if (live) {
            Ctx c[V];
            float b[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                c[k] = stats_ctx(p, gp.s[g * gp.C + c0 + k]);
                if constexpr (AFF) b[k] = p.b[g * gp.C + c0 + k];
                else b[k] = 0.f;
            }
            // two rows in flight: the integer grid's V = 4 then holds 90 VGPRs (96 with an offset), 5 waves per SIMD with two loads
            // each.  (As a kernel of its own, before the bodies were shared, it held 92 (98) and 5 (4) waves; one row in flight held
            // 76 (83) and 6 (5) waves with one load)
#pragma unroll 2
            for (int64_t r = r0 + slot; r < r1; r += SLOTS) {
                const int64_t i = r * gp.C + c0;
                if constexpr (V == 4) {
                    const float4 x = *reinterpret_cast<const float4*>(gp.P + i);
                    float4 t;
                    if constexpr (AFF) t = fq_quot4c(make_float4(x.x - b[0], x.y - b[1], x.z - b[2], x.w - b[3]), c);
                    else t = fq_quot4c(x, c);
                    stats_take<RNE, AFF>(p, c[0], b[0], x.x, t.x, a[0], binned, sh_hist);
                    stats_take<RNE, AFF>(p, c[1], b[1], x.y, t.y, a[1], binned, sh_hist);
                    stats_take<RNE, AFF>(p, c[2], b[2], x.z, t.z, a[2], binned, sh_hist);
                    stats_take<RNE, AFF>(p, c[3], b[3], x.w, t.w, a[3], binned, sh_hist);
                } else {
                    const float x = gp.P[i];
                    float u = x;
                    if constexpr (AFF) u = u - b[0];
                    stats_take<RNE, AFF>(p, c[0], b[0], x, div_by_uniform(u, c[0]), a[0], binned, sh_hist);
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
            if constexpr (FL) sh_flushed[j] = a[k].flushed;
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
        } else if constexpr (FL) {
            if (slot == 2 && live) {      // slot 2: flushed
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    uint32_t cnt = sh_flushed[lx * V + k];
#pragma unroll 2
                    for (int w = 1; w < SLOTS; ++w) cnt += sh_flushed[w * COLS + lx * V + k];
                    p.flushed[g * gp.C + c0 + k] = cnt;
                }
            }
        }
        __syncthreads();
    }
    stats_hist_flush(p, binned, sh_hist);
}

// The work of one block of a row kernel: kBlock >> log_team (row, group) pairs
template <bool RNE, bool AFF, int V, class PT>
__device__ __forceinline__ void stats_rows_body(const PT& p, const int log_team) {
    extern __shared__ uint32_t sh_hist[];      // p.nbins words where the caller wants the histogram, else none
    const auto& gp = stats_geom(p);
    const bool binned = p.hist != nullptr;      // kernel-uniform
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const uint32_t pairs = (uint32_t)gp.R * (uint32_t)gp.nb;      // <= R * C < 2^31
    const uint32_t pair = blockIdx.x * (uint32_t)(kBlock >> log_team) + (threadIdx.x >> log_team);
    const bool live = pair < pairs;
    stats_hist_clear(p, binned, sh_hist);
    StatsAcc a = StatsAcc{0u, 0u, 0u, 0.0, 0.0};
    if (live) {
        const uint32_t r = pair / (uint32_t)gp.nb, g = pair - r * (uint32_t)gp.nb;
        const int64_t base = (int64_t)r * gp.C;
        const int64_t c0 = (int64_t)g * gp.gs;
        const int64_t c1 = (c0 + gp.gs < gp.C) ? c0 + gp.gs : gp.C;
        const Ctx c = stats_ctx(p, gp.s[pair]);
        float b = 0.f;
        if constexpr (AFF) b = p.b[pair];
        for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {      // V = 4: gs % 4 == 0 and C % 4 == 0
            const int64_t i = base + col;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(gp.P + i);
                float4 t;
                if constexpr (AFF) t = fq_quot4(make_float4(x.x - b, x.y - b, x.z - b, x.w - b), c);
                else t = fq_quot4(x, c);
                stats_take<RNE, AFF>(p, c, b, x.x, t.x, a, binned, sh_hist);
                stats_take<RNE, AFF>(p, c, b, x.y, t.y, a, binned, sh_hist);
                stats_take<RNE, AFF>(p, c, b, x.z, t.z, a, binned, sh_hist);
                stats_take<RNE, AFF>(p, c, b, x.w, t.w, a, binned, sh_hist);
            } else {
                const float x = gp.P[i];
                float u = x;
                if constexpr (AFF) u = u - b;
                stats_take<RNE, AFF>(p, c, b, x, div_by_uniform(u, c), a, binned, sh_hist);
            }
        }
    }
    for (int off = T >> 1; off > 0; off >>= 1) {      // fixed butterfly inside the aligned team; every lane of the wave takes part
        a.err2 += __shfl_xor(a.err2, off);
        a.sig2 += __shfl_xor(a.sig2, off);
        a.below += __shfl_xor(a.below, off);
        a.above += __shfl_xor(a.above, off);
        if constexpr (PT::kFlushed) a.flushed += __shfl_xor(a.flushed, off);
    }
    if (live && lt == 0) {
        p.below[pair] = a.below;
        p.above[pair] = a.above;
        if constexpr (PT::kFlushed) p.flushed[pair] = a.flushed;
        p.err2[pair] = a.err2;
        p.sig2[pair] = a.sig2;
    }
    stats_hist_flush(p, binned, sh_hist);
}

template <bool RNE, bool AFF, int V, int TX>
__global__ __launch_bounds__(kBlock) void k_stats_cols(const StatsParams p) {
    stats_cols_body<RNE, AFF, V, TX>(p);
}

template <bool RNE, bool AFF, int V>
__global__ __launch_bounds__(kBlock) void k_stats_rows(const StatsParams p, const int log_team) {
    stats_rows_body<RNE, AFF, V>(p, log_team);
}

}  // namespace lq

#endif

