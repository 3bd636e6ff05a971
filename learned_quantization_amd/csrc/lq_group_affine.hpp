// lq_group_affine.hpp -- asymmetric group-wise scales: a learned offset b per group next to the scale s
// (lq_hip.h: lq_fq_forward_group_affine / lq_fq_backward_group_affine / lq_scale_init_group_minmax)
//
//   u = P - b;  t = u / s;  q0 = rnd(t);  q = clamp(q0, lo, hi);  out = (q * s) + b      (every operation rounds on its own)
//   inside = lo <= q0 <= hi;  dP = inside ? dy : +0;  r = inside ? q0 - t : q
//   ds[g] = RN(k * sum dy * r);  db[g] = RN(kb * sum_{!inside} dy);  clipped[g] = #{!inside}      (sums in f64)
//
// Geometry, unit shapes and launch rule are lq_group.hpp's, taken from the same host helpers: k_group_affine_cols is k_group_cols
// (a lane keeps V columns, TX lanes side by side, 256 / TX row slots; the backward's partials meet in LDS and slot 0 adds them in
// slot order; the forward may split a group's rows over gridDim.z blocks), k_group_affine_rows is k_group_rows (a team of 2^k
// lanes per (row, group), xor butterfly, lane 0 emits).  What is added: per group one more context load (the offset, indexed like
// the scale), per element one subtraction ahead of K1's quotient and one addition behind the product, and in the backward a second
// f64 accumulator (sum of dy over the clipped elements) that travels with the first: a second LDS array merged in the same slot
// order (by the lanes of slot 1, while slot 0 merges the first), or the same butterfly.  The quotient is the symmetric pair's (div_by_uniform / fq_quot4 / fq_quot4c on u), the backward
// term is ClipBwdOp<RNE>::one itself: with b == +0 u is P bit for bit and dP, ds and clipped are the symmetric kernels' bits.
// The library is built without contraction: q * s + b is a product and a sum.
//
// k_minmax_cols / k_minmax_rows write s and b of a group from its minimum and maximum on the unit shapes of lq_scale_init.hpp
// (whole groups meet in one place; fminf / fmaxf are exact and order-free).
#ifndef LQ_GROUP_AFFINE_HPP_
#define LQ_GROUP_AFFINE_HPP_
#include "lq_group.hpp"
#include "lq_scale_init.hpp"

namespace lq {

struct GroupAffineParams {
    GroupParams g;        // P, s, dy, out / dP, q, range, k, ds, clipped, geometry: as the symmetric pair
    const float* b;       // offset, the scale's shape
    float* db;            // backward, may be NULL
    float kb;             // offset_grad_scale
};

// backward: ClipBwdOp's term on t, and dy of a clipped element into the offset's sum.  dP == dy (bitwise, or both NaN) exactly
// where the element is inside, except for dy == 0 and NaN dy, so `inside` is taken from q0 again: the compiler merges the two.
template <bool RNE>
__device__ __forceinline__ float affine_bwd_one(float t, float dy, float lo, float hi, Acc& acc, double& accb) {
    const float q0 = ClipBase<RNE>::rnd(t);
    const bool inside = (q0 >= lo) & (q0 <= hi);
    accb += inside ? 0.0 : (double)dy;
    return ClipBwdOp<RNE>::one(t, dy, lo, hi, acc);
}

template <bool RNE, bool BWD>
__device__ __forceinline__ float affine_elem(const GroupParams& p, const Ctx& c, float b, int64_t i, float t, float dy, Acc& acc, double& accb) {
    if constexpr (BWD) {
        return affine_bwd_one<RNE>(t, dy, c.k0, c.k1, acc, accb);
    } else {
        const float q = ClipBase<RNE>::clampq(ClipBase<RNE>::rnd(t), c.k0, c.k1);
        if (p.q) store_q(p.q, p.q_dtype, i, q);
        const float m = q * c.s;
        return m + b;
    }
}

// group_cols_body with an offset.  sh_sum / sh_sumb / sh_cnt: [256 / TX][TX * V] in LDS (backward only).
template <bool RNE, bool BWD, int V, int TX>
__device__ __forceinline__ void group_affine_cols_body(const GroupAffineParams& ap, const int64_t bx, const int64_t g, const int zi, const int nz,
                                                       const bool reduce, double* sh_sum, double* sh_sumb, uint32_t* sh_cnt) {
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    const GroupParams& p = ap.g;
    const int lx = (int)threadIdx.x % TX, slot = (int)threadIdx.x / TX;
    const int64_t c0 = (bx * TX + lx) * V;
    const bool live = c0 < p.C;      // V = 4 runs only with C % 4 == 0: the lane's four columns are inside together
    Acc acc[V];
    double accb[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        acc[k] = Acc{0u, 0u, 0.0};
        accb[k] = 0.0;
    }
    if (live) {
        const int64_t r0 = g * p.gs;
        const int64_t r1 = (r0 + p.gs < p.R) ? r0 + p.gs : p.R;
        Ctx c[V];
        float b[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            c[k] = group_ctx<RNE>(p, p.s[g * p.C + c0 + k]);
            b[k] = ap.b[g * p.C + c0 + k];
        }
        // the backward walks one row at a time: two rows in flight (the forward's and the symmetric backward's unroll) cost 106
        // VGPRs with the second f64 accumulator, 4 waves per SIMD instead of 6, and a second round of blocks on weight-sized tensors
#pragma unroll(BWD ? 1 : 2)
        for (int64_t r = r0 + zi * SLOTS + slot; r < r1; r += (int64_t)SLOTS * nz) {
            const int64_t i = r * p.C + c0;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (BWD) dy = *reinterpret_cast<const float4*>(p.dy + i);
                const float4 u = make_float4(x.x - b[0], x.y - b[1], x.z - b[2], x.w - b[3]);
                const float4 t = fq_quot4c(u, c);
                float4 o;
                o.x = affine_elem<RNE, BWD>(p, c[0], b[0], i + 0, t.x, dy.x, acc[0], accb[0]);
                o.y = affine_elem<RNE, BWD>(p, c[1], b[1], i + 1, t.y, dy.y, acc[1], accb[1]);
                o.z = affine_elem<RNE, BWD>(p, c[2], b[2], i + 2, t.z, dy.z, acc[2], accb[2]);
                o.w = affine_elem<RNE, BWD>(p, c[3], b[3], i + 3, t.w, dy.w, acc[3], accb[3]);
                *reinterpret_cast<float4*>(p.out + i) = o;
            } else {
                const float x = p.P[i];
                float dy = 0.f;
                if constexpr (BWD) dy = p.dy[i];
                p.out[i] = affine_elem<RNE, BWD>(p, c[0], b[0], i, div_by_uniform(x - b[0], c[0]), dy, acc[0], accb[0]);
            }
        }
    }
    if constexpr (BWD) {
        if (reduce) {      // block-uniform: every thread meets the barriers
#pragma unroll
            for (int k = 0; k < V; ++k) {
                sh_sum[slot * COLS + lx * V + k] = acc[k].c;
                sh_sumb[slot * COLS + lx * V + k] = accb[k];
                sh_cnt[slot * COLS + lx * V + k] = acc[k].b;
            }
            __syncthreads();
            // slot 0 merges the scale's sums and the counts as the symmetric kernel does; slot 1 (there are 4 slots at least) merges
            // the offset's sums at the same time, in the same slot order: the merge is no longer than the symmetric one
            if (slot == 0 && live) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    double sum = sh_sum[lx * V + k];
                    uint32_t cnt = sh_cnt[lx * V + k];
                    for (int w = 1; w < SLOTS; ++w) {      // fixed order: slot 0, 1, 2, ...
                        sum += sh_sum[w * COLS + lx * V + k];
                        cnt += sh_cnt[w * COLS + lx * V + k];
                    }
                    const int64_t j = g * p.C + c0 + k;
                    if (p.ds) p.ds[j] = (float)((double)p.k * sum);
                    if (p.clipped) p.clipped[j] = cnt;
                }
            } else if (slot == 1 && live && ap.db) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    double sumb = sh_sumb[lx * V + k];
                    for (int w = 1; w < SLOTS; ++w) sumb += sh_sumb[w * COLS + lx * V + k];      // the same fixed order
                    ap.db[g * p.C + c0 + k] = (float)((double)ap.kb * sumb);
                }
            }
            __syncthreads();
        }
    }
}

template <bool RNE, bool BWD, int V, int TX>
__global__ __launch_bounds__(kBlock) void k_group_affine_cols(const GroupAffineParams ap) {
    constexpr int SLOTS = kBlock / TX;
    static_assert(SLOTS >= 2, "slot 1 merges the offset's sums");
    constexpr int COLS = TX * V;
    __shared__ double sh_sum[BWD ? SLOTS * COLS : 1];
    __shared__ double sh_sumb[BWD ? SLOTS * COLS : 1];
    __shared__ uint32_t sh_cnt[BWD ? SLOTS * COLS : 1];
    const bool reduce = BWD && (ap.g.ds != nullptr || ap.db != nullptr || ap.g.clipped != nullptr);      // kernel-uniform
    // the trip count of the group loop is block-uniform
    for (int64_t g = blockIdx.y; g < ap.g.nb; g += gridDim.y)
        group_affine_cols_body<RNE, BWD, V, TX>(ap, (int64_t)blockIdx.x, g, (int)blockIdx.z, (int)gridDim.z, reduce, sh_sum, sh_sumb, sh_cnt);
}

// group_rows_body with an offset: [R][nb] like the scale, pair index == offset index.  No barrier.
template <bool RNE, bool BWD, int V>
__device__ __forceinline__ void group_affine_rows_body(const GroupAffineParams& ap, const int log_team, const uint32_t blk) {
    const GroupParams& p = ap.g;
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const uint32_t pairs = (uint32_t)p.R * (uint32_t)p.nb;      // <= R * C < 2^31
    const uint32_t pair = blk * (uint32_t)(kBlock >> log_team) + (threadIdx.x >> log_team);
    const bool live = pair < pairs;
    Acc acc = Acc{0u, 0u, 0.0};
    double accb = 0.0;
    if (live) {
        const uint32_t r = pair / (uint32_t)p.nb, g = pair - r * (uint32_t)p.nb;
        const int64_t base = (int64_t)r * p.C;
        const int64_t c0 = (int64_t)g * p.gs;
        const int64_t c1 = (c0 + p.gs < p.C) ? c0 + p.gs : p.C;
        const Ctx c = group_ctx<RNE>(p, p.s[pair]);
        const float b = ap.b[pair];
        for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {      // V = 4: gs % 4 == 0 and C % 4 == 0
            const int64_t i = base + col;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (BWD) dy = *reinterpret_cast<const float4*>(p.dy + i);
                const float4 u = make_float4(x.x - b, x.y - b, x.z - b, x.w - b);
                const float4 t = fq_quot4(u, c);
                float4 o;
                o.x = affine_elem<RNE, BWD>(p, c, b, i + 0, t.x, dy.x, acc, accb);
                o.y = affine_elem<RNE, BWD>(p, c, b, i + 1, t.y, dy.y, acc, accb);
                o.z = affine_elem<RNE, BWD>(p, c, b, i + 2, t.z, dy.z, acc, accb);
                o.w = affine_elem<RNE, BWD>(p, c, b, i + 3, t.w, dy.w, acc, accb);
                *reinterpret_cast<float4*>(p.out + i) = o;
            } else {
                const float x = p.P[i];
                float dy = 0.f;
                if constexpr (BWD) dy = p.dy[i];
                p.out[i] = affine_elem<RNE, BWD>(p, c, b, i, div_by_uniform(x - b, c), dy, acc, accb);
            }
        }
    }
    if constexpr (BWD) {
        if (p.ds != nullptr || ap.db != nullptr || p.clipped != nullptr) {      // block-uniform
            double sum = acc.c;
            double sumb = accb;
            uint32_t cnt = acc.b;
            for (int off = T >> 1; off > 0; off >>= 1) {      // fixed butterfly inside the aligned team; every lane of the wave takes part
                sum += __shfl_xor(sum, off);
                sumb += __shfl_xor(sumb, off);
                cnt += __shfl_xor(cnt, off);
            }
            if (live && lt == 0) {
                if (p.ds) p.ds[pair] = (float)((double)p.k * sum);
                if (ap.db) ap.db[pair] = (float)((double)ap.kb * sumb);
                if (p.clipped) p.clipped[pair] = cnt;
            }
        }
    }
}

template <bool RNE, bool BWD, int V>
__global__ __launch_bounds__(kBlock) void k_group_affine_rows(const GroupAffineParams ap, const int log_team) {
    group_affine_rows_body<RNE, BWD, V>(ap, log_team, blockIdx.x);
}

// ---- min-max initialisation ----
struct MinMaxParams {
    const float* P;
    float* s;
    float* b;
    float n;              // (float)(qmax - qmin), >= 1
    float c;              // (qmin + qmax) / 2 (+ 1/2 for floor), exact
    float min_value;      // > 0, finite
    int32_t R, C, gs, nb; // as GroupParams
};

struct MinMaxAcc {
    float mn, mx;
    uint32_t bad;         // the group holds a NaN or an Inf
};

__device__ __forceinline__ void minmax_take(float x, MinMaxAcc& a) {
    a.bad |= (fabsf(x) < __builtin_inff()) ? 0u : 1u;      // false for NaN and +-Inf
    a.mn = fminf(a.mn, x);                                 // fminf / fmaxf skip a NaN operand; `bad` has it
    a.mx = fmaxf(a.mx, x);
}

__device__ __forceinline__ void minmax_emit(const MinMaxParams& p, const MinMaxAcc& a, int64_t j) {
    const float nan = __uint_as_float(0x7fc00000u);
    const float d = a.mx - a.mn;
    const float w = d / p.n;
    const float s = fmaxf(w * kAbsmaxMargin, p.min_value);
    const float h0 = 0.5f * a.mn;
    const float h1 = 0.5f * a.mx;
    const float mid = h0 + h1;
    const float cs = p.c * s;
    const float b = mid - cs;
    p.s[j] = a.bad ? nan : s;
    p.b[j] = a.bad ? nan : b;
}

template <int V, int TX>
__global__ __launch_bounds__(kBlock) void k_minmax_cols(const MinMaxParams p) {
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    __shared__ float sh_mn[SLOTS * COLS];
    __shared__ float sh_mx[SLOTS * COLS];
    __shared__ uint32_t sh_u[SLOTS * COLS];
    const int lx = (int)threadIdx.x % TX, slot = (int)threadIdx.x / TX;
    const int64_t c0 = ((int64_t)blockIdx.x * TX + lx) * V;
    const bool live = c0 < p.C;      // V = 4 runs only with C % 4 == 0
    // the trip count of the group loop is block-uniform: every thread meets every barrier
    for (int64_t g = blockIdx.y; g < p.nb; g += gridDim.y) {
        const int64_t r0 = g * p.gs;
        const int64_t r1 = (r0 + p.gs < p.R) ? r0 + p.gs : p.R;
        MinMaxAcc a[V];
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] = MinMaxAcc{__builtin_inff(), -__builtin_inff(), 0u};
        if (live) {
#pragma unroll 4
            for (int64_t r = r0 + slot; r < r1; r += SLOTS) {
                const int64_t i = r * p.C + c0;
                if constexpr (V == 4) {
                    const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                    minmax_take(x.x, a[0]);
                    minmax_take(x.y, a[1]);
                    minmax_take(x.z, a[2]);
                    minmax_take(x.w, a[3]);
                } else {
                    minmax_take(p.P[i], a[0]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int j = slot * COLS + lx * V + k;
            sh_mn[j] = a[k].mn;
            sh_mx[j] = a[k].mx;
            sh_u[j] = a[k].bad;
        }
        __syncthreads();
        if (slot == 0 && live) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                MinMaxAcc t = MinMaxAcc{__builtin_inff(), -__builtin_inff(), 0u};
#pragma unroll 2
                for (int w = 0; w < SLOTS; ++w) {
                    const int j = w * COLS + lx * V + k;
                    t.mn = fminf(t.mn, sh_mn[j]);
                    t.mx = fmaxf(t.mx, sh_mx[j]);
                    t.bad |= sh_u[j];
                }
                minmax_emit(p, t, g * p.C + c0 + k);
            }
        }
        __syncthreads();
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_minmax_rows(const MinMaxParams p, const int log_team) {
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const uint32_t pairs = (uint32_t)p.R * (uint32_t)p.nb;      // <= R * C < 2^31
    const uint32_t pair = blockIdx.x * (uint32_t)(kBlock >> log_team) + (threadIdx.x >> log_team);
    const bool live = pair < pairs;
    MinMaxAcc a = MinMaxAcc{__builtin_inff(), -__builtin_inff(), 0u};
    if (live) {
        const uint32_t r = pair / (uint32_t)p.nb, g = pair - r * (uint32_t)p.nb;
        const int64_t base = (int64_t)r * p.C;
        const int64_t c0 = (int64_t)g * p.gs;
        const int64_t c1 = (c0 + p.gs < p.C) ? c0 + p.gs : p.C;
        for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {      // V = 4: gs % 4 == 0 and C % 4 == 0
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + base + col);
                minmax_take(x.x, a);
                minmax_take(x.y, a);
                minmax_take(x.z, a);
                minmax_take(x.w, a);
            } else {
                minmax_take(p.P[base + col], a);
            }
        }
    }
    for (int off = T >> 1; off > 0; off >>= 1) {      // fixed butterfly inside the aligned team; every lane of the wave takes part
        a.mn = fminf(a.mn, __shfl_xor(a.mn, off));
        a.mx = fmaxf(a.mx, __shfl_xor(a.mx, off));
        a.bad |= __shfl_xor(a.bad, off);
    }
    if (live && lt == 0) minmax_emit(p, a, pair);
}

}  // namespace lq

#endif
