// lq_mx.hpp -- OCP microscaling (MX) element formats on the group-wise traversals
// (lq_hip.h: lq_fq_forward_mx / lq_fq_backward_mx / lq_scale_init_mx)
//
// Geometry, launch rule, traversal bodies, merge order and outputs are lq_group.hpp's; what differs is the element step, supplied
// to the bodies as GroupStep<RNE, GroupMxParams> (RNE is not read: a minifloat grid has one rounding, ties to even):
//
//   ctx    s_eff from the stored scale, once per group context: the nearest power of two in the log domain for an E8M0 scale (NaN
//          for a scale that is not positive, normal and finite, or that rounds past 2^127), the scale itself for an fp32 one; then
//          div_ctx(s_eff) -- a power of two inside 2^+-40 takes the uniform-divisor path like any other scale, and every step of it
//          is exact
//   quant  e = clamp(exponent field of |t|, emin, 127), u = 2^(e - M), q0 = copysign(rint(|t| * 2^(M - e)) * u, t), clamped to
//          +-mx by comparisons.  Both products are exact (a power of two times a value with room in the exponent); the upper clamp
//          of e only keeps 2^(M - e) a normal float for a non-finite t, which passes through unchanged either way.  The two powers
//          of two are formed in place, on the exponent field where it sits (and, med3, two subtractions against kernel-uniform
//          constants)
//   view   the element's encoding: sign, exponent and mantissa fields of q in the format
//   bwd    ClipBwdOp's term with q0 from `quant`'s rounding: inside = |q0| <= mx, r = inside ? q0 - t : q
//
// The format enters as the kernel-uniform values (M, emin, mx, bits) of GroupMxParams: one instantiation family (forward and
// backward of the four forms) serves the five formats and both scale formats.
#ifndef LQ_MX_HPP_
#define LQ_MX_HPP_
#include "lq_group.hpp"

namespace lq {

struct GroupMxParams {
    GroupParams g;        // P, s, dy, out / dP, q (the encodings), k, ds, clipped, geometry: as the integer pair; lo = -mx, hi = mx
    int32_t M;            // mantissa bits of the element format
    int32_t emin;         // exponent of its smallest normal
    int32_t bits;         // 1 + E + M
    uint32_t e8m0_mask;   // all ones: the stored scale is rounded to a power of two (LQ_SCALE_E8M0); 0: used as it is (LQ_SCALE_FP32)
};
__host__ __device__ __forceinline__ const GroupParams& group_base(const GroupMxParams& mp) { return mp.g; }
__device__ __forceinline__ float* group_db(const GroupMxParams&) { return nullptr; }

// the effective scale of a stored scale under LQ_SCALE_E8M0
__device__ __forceinline__ float mx_e8m0(float s) {
    const uint32_t sb = __float_as_uint(s);
    const bool valid = sb >= 0x00800000u && sb < 0x7f800000u;             // positive, normal, finite
    const uint32_t nb = (sb + 0x004afb0du) & 0x7f800000u;                 // mantissa >= sqrt(2) (fraction 0x3504f3) rounds up
    return (valid & (nb < 0x7f800000u)) ? __uint_as_float(nb) : __uint_as_float(0x7fc00000u);
}

// s_eff under either scale format, without a branch: the format is kernel-uniform, and as a branch it puts a wait between the
// scale loads of a lane's four contexts (four memory latencies in a row at the head of every group, measured: 19.2 us with the
// branch, 16.7 us without, for the forward of the (4224, 2048, 0, 32) matrix under E8M0)
__device__ __forceinline__ float mx_effective_scale(const GroupMxParams& mp, float s) {
    const uint32_t pow2 = __float_as_uint(mx_e8m0(s));
    return __uint_as_float((pow2 & mp.e8m0_mask) | (__float_as_uint(s) & ~mp.e8m0_mask));
}

// t on the element grid, unclamped
__device__ __forceinline__ float mx_round(float t, const GroupMxParams& mp) {
    const uint32_t e_lo = (uint32_t)(mp.emin + 127) << 23, m23 = (uint32_t)mp.M << 23;      // kernel-uniform: scalar registers
    const uint32_t field = __float_as_uint(t) & 0x7f800000u;              // 0 for a zero or subnormal |t|
    const uint32_t e = min(max(field, e_lo), 0x7f000000u);                // bits(2^e), e = clamp(exponent, emin, 127)
    const float to_int = __uint_as_float((0x7f000000u + m23) - e);        // 2^(M - e): |t| in units of u
    const float u = __uint_as_float(e - m23);                             // 2^(e - M)
    return copysignf(rintf(fabsf(t) * to_int) * u, t);
}

// the encoding of a clamped grid value q, as the integer it is (lq_mx_stats.hpp bins by it)
__device__ __forceinline__ uint32_t mx_code_bits(float q, int M, int emin, int bits) {
    const uint32_t qb = __float_as_uint(q);
    const uint32_t ab = qb & 0x7fffffffu;
    uint32_t mag;
    if (ab < ((uint32_t)(127 + emin) << 23)) {                            // below the smallest normal: a multiple of 2^(emin - M)
        mag = (uint32_t)(__uint_as_float(ab) * __uint_as_float((uint32_t)(127 + M - emin) << 23));
    } else {
        mag = (ab >> (23 - M)) - ((uint32_t)(126 + emin) << M);           // (e - emin + 1) * 2^M + the M mantissa bits
    }
    const uint32_t top = 1u << (bits - 1);
    return (q != q) ? top - 1u : ((qb >> 31) ? top : 0u) + mag;      // a NaN has no sign to keep: all ones below the sign bit
}

// the same as a float (the integer view's store converts it)
__device__ __forceinline__ float mx_code(float q, int M, int emin, int bits) { return (float)mx_code_bits(q, M, emin, bits); }

template <bool RNE>
struct GroupStep<RNE, GroupMxParams> {
    __device__ static __forceinline__ Ctx ctx(const GroupMxParams& mp, float s) {
        Ctx c;
        c.s = mx_effective_scale(mp, s);
        div_ctx(c);
        c.k0 = mp.g.lo;
        c.k1 = mp.g.hi;
        c.lam_hi = 0.f;
        c.sure_ok = 0;
        return c;
    }
    __device__ static __forceinline__ float quant(const GroupMxParams& mp, const Ctx& c, float t) {
        return ClipBase<true>::clampq(mx_round(t, mp), c.k0, c.k1);
    }
    __device__ static __forceinline__ float view(const GroupMxParams& mp, float q) { return mx_code(q, mp.M, mp.emin, mp.bits); }
    __device__ static __forceinline__ float bwd(const GroupMxParams& mp, const Ctx& c, float t, float dy, Acc& acc) {
        const float q0 = mx_round(t, mp);
        const bool inside = (q0 >= c.k0) & (q0 <= c.k1);                  // false for NaN
        const float r = inside ? q0 - t : ClipBase<true>::clampq(q0, c.k0, c.k1);
        acc.c += (double)dy * (double)r;
        acc.b += inside ? 0u : 1u;
        return inside ? dy : 0.f;
    }
};

template <bool BWD, int V, int TX>
__global__ __launch_bounds__(kBlock) void k_group_mx_cols(const GroupMxParams mp) {
    constexpr int N = BWD ? (kBlock / TX) * (TX * V) : 1;
    __shared__ double sh_sum[N];
    __shared__ uint32_t sh_cnt[N];
    const bool reduce = BWD && (mp.g.ds != nullptr || mp.g.clipped != nullptr);      // kernel-uniform
    for (int64_t g = blockIdx.y; g < mp.g.nb; g += gridDim.y)
        group_cols_body<true, BWD, V, TX>(mp, (int64_t)blockIdx.x, g, (int)blockIdx.z, (int)gridDim.z, reduce, sh_sum, nullptr, sh_cnt);
}

template <bool BWD, int V>
__global__ __launch_bounds__(kBlock) void k_group_mx_rows(const GroupMxParams mp, const int log_team) {
    group_rows_body<true, BWD, V>(mp, log_team, blockIdx.x);
}

}  // namespace lq

#endif
