// lq_mx_stats.hpp -- per-group statistics of the microscaling (MX) quantizer (lq_hip.h: lq_mx_stats)
//
// The minifloat grids of lq_mx.hpp on the traversal bodies of lq_group_stats.hpp, which states the design: geometry, unit shapes,
// team widths, grid, merge order and histogram are the bodies'.  This file supplies what the grid changes.  Per group: how many
// elements saturate on either side of +-mx, how many non-zero elements the grid turns into a zero of either sign (flushed below the
// smallest subnormal: the third count, kFlushed), the two f64 sums; per tensor the histogram of the elements' encodings (2^bits
// bins: 16 / 64 / 256).  Per element the arithmetic is lq_mx.hpp's forward: GroupStep<true, GroupMxParams>::ctx (s_eff and the
// division context), the group-wise quotient, mx_round, the comparison clamp, out = q * s_eff, and mx_code_bits for the bin -- the
// integer that mx_code converts for the forward's code view.
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
    static constexpr bool kFlushed = true;
};

__device__ __forceinline__ const GroupParams& stats_geom(const MxStatsParams& p) { return p.mp.g; }
__device__ __forceinline__ Ctx stats_ctx(const MxStatsParams& p, float s) { return GroupStep<true, GroupMxParams>::ctx(p.mp, s); }

// one element: x = P, t its quotient by s_eff.  There is one rounding and no offset: RNE, AFF and b are not read
template <bool RNE, bool AFF>
__device__ __forceinline__ void stats_take(const MxStatsParams& p, const Ctx& c, float, float x, float t, StatsAcc& a, const bool binned,
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

template <int V, int TX>
__global__ __launch_bounds__(kBlock) void k_mx_stats_cols(const MxStatsParams p) {
    stats_cols_body<true, false, V, TX>(p);
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_mx_stats_rows(const MxStatsParams p, const int log_team) {
    stats_rows_body<true, false, V>(p, log_team);
}

}  // namespace lq

#endif
