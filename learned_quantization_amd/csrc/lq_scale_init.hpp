// lq_scale_init.hpp -- scales (and offsets) of the clipped b-bit quantizer from the weights themselves
// (lq_hip.h: lq_scale_init_group / lq_scale_init_group_minmax)
//
// Geometry and unit shapes are those of lq_group.hpp's BACKWARD, the ones in which a whole group meets in one place:
//
//   k_init_cols  (axis 0)  a lane keeps V fixed columns (V = 4: one float4; V = 1), TX lanes side by side, the 256 / TX row slots of
//                          the block split the rows of a group.  A block owns whole groups of its 64-column tile (blockIdx.y,
//                          grid-stride).  The slots' partials meet in LDS and are merged in slot order; slot 0 emits.
//   k_init_rows  (axis 1)  a team of T = 2^k <= 64 lanes per (row, group), a fixed xor butterfly, lane 0 of the team emits.
//
// The method is a compile-time parameter.  What a lane starts from and carries, how two partials merge and what the emitting lane
// writes are the method's init_start / init_take / init_merge / init_raw / init_final (and init_offset) below; the two kernels are
// the traversal around them.  LQ_INIT_ABSMAX carries two fp32 maxima; kInitMinMax (min-max: s and the offset b of the asymmetric
// quantizer) the minimum and the maximum (fminf / fmaxf: exact, order-free); LQ_INIT_LSQ one f64 sum of |P|; LQ_INIT_MSE runs the
// absmax reduction (phase 1: every lane of the group reads the result back), then walks the group's elements again and adds up, per candidate scale, the f64 squared error of the project's own clipped quantizer (phase 2), and the
// emitting lane takes the first smallest.  The row form holds all 28 error sums of its one scale (56 VGPRs); the column form with
// four columns per lane walks the candidates 7 at a time and re-reads the group per chunk.  Its partials pass through the same
// 12 KB of LDS the backward uses (one f64 and one 32-bit word per slot and column), one candidate at a time.
// Every sum has one fixed order (the lane's own elements ascending, then slots 0, 1, ... or the butterfly): two runs give the same
// bits.  No atomics, no second stage, no workspace.  The quotient is the IEEE `/` (the library is built with correctly rounded fp32
// division and without contraction: s0 * c_k is one multiply, d * d and the addition are two roundings).
#ifndef LQ_SCALE_INIT_HPP_
#define LQ_SCALE_INIT_HPP_
#include "lq_group.hpp"

namespace lq {

constexpr int kInitMinMax = 3;      // internal: lq_scale_init_group_minmax.  The public methods are lq_scale_init_method's
static_assert(kInitMinMax != LQ_INIT_ABSMAX && kInitMinMax != LQ_INIT_LSQ && kInitMinMax != LQ_INIT_MSE, "method constants collide");
// internal: lq_scale_init_mx's two rules (LQ_MX_INIT_OCP / LQ_MX_INIT_COVER).  They carry the absmax pair and differ in init_raw only
constexpr int kInitMxOcp = 4;
constexpr int kInitMxCover = 5;

// One layout for every method.  Min-max's n, c and b lie in unions on the fields it does not read (the host writes only the members
// of the method it launches): three more plain fields would grow the kernel argument, move log_team behind it and so change the
// argument loads and descriptors of the three methods that shipped before it.
struct InitParams {
    const float* P;
    float* s;
    union { float lo; float n; int32_t emax; };          // (float)qmin | min-max: (float)(qmax - qmin), >= 1 | MX: the format's emax
    union { float hi; float c; uint32_t mm_frac; };      // (float)qmax | min-max: (qmin + qmax) / 2 (+ 1/2 for floor), exact | MX: fraction bits of mx / 2^emax
    float min_value;      // > 0, finite
    union {
        double sqrt_qp;   // LQ_INIT_LSQ: sqrt((double)qp), taken on the host
        float* b;         // min-max: the offset, the scale's shape
    };
    int32_t R, C, gs, nb; // as GroupParams
};

constexpr int kInitCandidates = 28;                          // c_k = (32 - k) / 32, k = 0 .. 27: 1 down to 5/32
constexpr float kAbsmaxMargin = 1.0000002384185791015625f;   // 1 + 2^-22

// what one lane carries through phase 1
struct InitAcc {
    float f0, f1;      // absmax and mse: max(P, 0), max(-P, 0); min-max: min P, max P
    double sum;        // sum |P|: lsq
    uint32_t bad;      // the group holds a NaN or an Inf
};

// a lane starts from InitAcc{0, 0, 0.0, 0}, and min-max's extremes from +-Inf
template <int M>
__device__ __forceinline__ void init_start(InitAcc& a) {
    if constexpr (M == kInitMinMax) {
        a.f0 = __builtin_inff();
        a.f1 = -__builtin_inff();
    }
}

template <int M>
__device__ __forceinline__ void init_take(float x, InitAcc& a) {
    a.bad |= (fabsf(x) < __builtin_inff()) ? 0u : 1u;      // false for NaN and +-Inf
    if constexpr (M == LQ_INIT_LSQ) {
        a.sum += (double)fabsf(x);
    } else if constexpr (M == kInitMinMax) {
        a.f0 = fminf(a.f0, x);       // fminf / fmaxf skip a NaN operand; `bad` has it
        a.f1 = fmaxf(a.f1, x);
    } else {
        a.f0 = fmaxf(a.f0, x);
        a.f1 = fmaxf(a.f1, -x);
    }
}

// a += another lane's or slot's partial
template <int M>
__device__ __forceinline__ void init_merge(InitAcc& a, float f0, float f1, double sum, uint32_t bad) {
    if constexpr (M == LQ_INIT_LSQ) {
        a.sum += sum;
    } else {
        a.f0 = (M == kInitMinMax) ? fminf(a.f0, f0) : fmaxf(a.f0, f0);
        a.f1 = fmaxf(a.f1, f1);
    }
    a.bad |= bad;
}

// s_raw of a group of n elements from its merged accumulator
template <int M>
__device__ __forceinline__ float init_raw(const InitParams& p, const InitAcc& a, int64_t n) {
    if constexpr (M == LQ_INIT_LSQ) {
        return (float)(2.0 * a.sum / ((double)n * p.sqrt_qp));
    } else if constexpr (M == kInitMinMax) {
        return (a.f1 - a.f0) / p.n * kAbsmaxMargin;      // three roundings
    } else if constexpr (M == kInitMxOcp || M == kInitMxCover) {
        // A = m * 2^e, m in [1, 2): p = 2^(e - emax), one binade up under COVER when m exceeds the format's largest mantissa.
        // Integer exponent arithmetic throughout; a subnormal A is normalised first
        const uint32_t ab = __float_as_uint(fmaxf(a.f0, a.f1));
        if (ab == 0u) return 0.f;                        // a group of zeros: init_final raises it to min_value
        int e;
        uint32_t frac;
        if (ab < 0x00800000u) {
            const int top = 31 - __clz((int)ab);         // 0 .. 22
            e = top - 149;
            frac = (ab << (23 - top)) & 0x7fffffu;
        } else {
            e = (int)(ab >> 23) - 127;
            frac = ab & 0x7fffffu;
        }
        int pe = e - p.emax + ((M == kInitMxCover && frac > p.mm_frac) ? 1 : 0);
        pe = max(pe, -126);                              // at most 127 - 2 + 1: every format has emax >= 2
        return __uint_as_float((uint32_t)(pe + 127) << 23);
    } else {
        const float qa = p.hi > 0.f ? a.f0 / p.hi : 0.f;
        const float qb = p.lo < 0.f ? a.f1 / -p.lo : 0.f;
        return fmaxf(qa, qb) * kAbsmaxMargin;
    }
}

__device__ __forceinline__ float init_final(const InitParams& p, float raw, uint32_t bad) {
    return bad ? __uint_as_float(0x7fc00000u) : fmaxf(raw, p.min_value);
}

// min-max: the offset b = (min / 2 + max / 2) - c * s of a group next to its s = init_final(raw), one rounding per operation
__device__ __forceinline__ float init_offset(const InitParams& p, const InitAcc& a, float raw) {
    const float mid = 0.5f * a.f0 + 0.5f * a.f1;
    const float b = mid - p.c * fmaxf(raw, p.min_value);
    return a.bad ? __uint_as_float(0x7fc00000u) : b;
}

__device__ __forceinline__ float init_candidate(const InitParams& p, float s0, int k) {
    const float ck = (float)(32 - k) * 0.03125f;      // exact
    return fmaxf(s0 * ck, p.min_value);
}

// one element against candidates k0 .. k0 + CH - 1
template <bool RNE, int CH>
__device__ __forceinline__ void mse_take(const InitParams& p, float x, float s0, int k0, double* E) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        const float sk = init_candidate(p, s0, k0 + j);
        const float t = x / sk;
        const float q = ClipBase<RNE>::clampq(ClipBase<RNE>::rnd(t), p.lo, p.hi);
        const float out = q * sk;
        const double d = (double)x - (double)out;
        E[j] += d * d;
    }
}

template <int M, bool RNE, int V, int TX>
__global__ __launch_bounds__(kBlock) void k_init_cols(const InitParams p) {
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    constexpr int CH = kInitCandidates / V;      // V = 4: 7 candidates per walk (28 f64 sums per lane); V = 1: all 28
    static_assert(CH * V == kInitCandidates, "the chunks must tile the candidates");
    __shared__ double sh_d[SLOTS * COLS];        // lsq: the sums; mse phase 2: one candidate's sums; else f0 | f1 as floats
    __shared__ uint32_t sh_u[SLOTS * COLS];
    float* const sh_f = reinterpret_cast<float*>(sh_d);
    const int lx = (int)threadIdx.x % TX, slot = (int)threadIdx.x / TX;
    const int64_t c0 = ((int64_t)blockIdx.x * TX + lx) * V;
    const bool live = c0 < p.C;      // V = 4 runs only with C % 4 == 0
    // the trip count of the group loop is block-uniform: every thread meets every barrier
    for (int64_t g = blockIdx.y; g < p.nb; g += gridDim.y) {
        const int64_t r0 = g * p.gs;
        const int64_t r1 = (r0 + p.gs < p.R) ? r0 + p.gs : p.R;
        InitAcc a[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            a[k] = InitAcc{0.f, 0.f, 0.0, 0u};
            init_start<M>(a[k]);
        }
        if (live) {
#pragma unroll 4
            for (int64_t r = r0 + slot; r < r1; r += SLOTS) {
                const int64_t i = r * p.C + c0;
                if constexpr (V == 4) {
                    const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                    init_take<M>(x.x, a[0]);
                    init_take<M>(x.y, a[1]);
                    init_take<M>(x.z, a[2]);
                    init_take<M>(x.w, a[3]);
                } else {
                    init_take<M>(p.P[i], a[0]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int j = slot * COLS + lx * V + k;
            if constexpr (M == LQ_INIT_LSQ) {
                sh_d[j] = a[k].sum;
            } else {
                sh_f[j] = a[k].f0;
                sh_f[SLOTS * COLS + j] = a[k].f1;
            }
            sh_u[j] = a[k].bad;
        }
        __syncthreads();
        // mse: every lane merges (phase 2 needs s0 in all slots); otherwise slot 0 alone.  Min-max's live lanes of slot 0 also store
        // where they merge: with the two output addresses formed here, not ahead of the row loop, that loop keeps four loads in flight
        // (66 VGPRs) instead of three and one (64).  The older methods store below, in the form they shipped with.
        constexpr bool STORE_HERE = M == kInitMinMax;
        float raw[V];
        uint32_t bad[V];
        if ((M == LQ_INIT_MSE || slot == 0) && (!STORE_HERE || live)) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                InitAcc t = InitAcc{0.f, 0.f, 0.0, 0u};
                init_start<M>(t);
#pragma unroll 2
                for (int w = 0; w < SLOTS; ++w) {      // fixed order: slot 0, 1, 2, ...
                    const int j = w * COLS + lx * V + k;
                    if constexpr (M == LQ_INIT_LSQ) init_merge<M>(t, 0.f, 0.f, sh_d[j], sh_u[j]);
                    else init_merge<M>(t, sh_f[j], sh_f[SLOTS * COLS + j], 0.0, sh_u[j]);
                }
                raw[k] = init_raw<M>(p, t, r1 - r0);
                bad[k] = t.bad;
                if constexpr (STORE_HERE) {
                    p.s[g * p.C + c0 + k] = init_final(p, raw[k], bad[k]);
                    p.b[g * p.C + c0 + k] = init_offset(p, t, raw[k]);
                }
            }
        }
        if constexpr (M != LQ_INIT_MSE) {
            if (!STORE_HERE && slot == 0 && live) {
#pragma unroll
                for (int k = 0; k < V; ++k) p.s[g * p.C + c0 + k] = init_final(p, raw[k], bad[k]);
            }
            __syncthreads();
        } else {
            __syncthreads();      // phase 1's partials are read: the LDS is free for phase 2
            double best[V];
            float best_s[V];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                best[k] = 0.0;
                best_s[k] = 0.f;
            }
#pragma unroll 1
            for (int k0 = 0; k0 < kInitCandidates; k0 += CH) {
                double E[V][CH];
#pragma unroll
                for (int k = 0; k < V; ++k)
#pragma unroll
                    for (int j = 0; j < CH; ++j) E[k][j] = 0.0;
                if (live) {
                    for (int64_t r = r0 + slot; r < r1; r += SLOTS) {
                        const int64_t i = r * p.C + c0;
                        if constexpr (V == 4) {
                            const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                            mse_take<RNE, CH>(p, x.x, raw[0], k0, E[0]);
                            mse_take<RNE, CH>(p, x.y, raw[1], k0, E[1]);
                            mse_take<RNE, CH>(p, x.z, raw[2], k0, E[2]);
                            mse_take<RNE, CH>(p, x.w, raw[3], k0, E[3]);
                        } else {
                            mse_take<RNE, CH>(p, p.P[i], raw[0], k0, E[0]);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < CH; ++j) {
#pragma unroll
                    for (int k = 0; k < V; ++k) sh_d[slot * COLS + lx * V + k] = E[k][j];
                    __syncthreads();
                    if (slot == 0 && live) {
#pragma unroll
                        for (int k = 0; k < V; ++k) {
                            double tot = sh_d[lx * V + k];
#pragma unroll 2
                            for (int w = 1; w < SLOTS; ++w) tot += sh_d[w * COLS + lx * V + k];      // slot order
                            if (k0 + j == 0 || tot < best[k]) {      // strict <: on equal sums the smallest k stays
                                best[k] = tot;
                                best_s[k] = init_candidate(p, raw[k], k0 + j);
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            if (slot == 0 && live) {
#pragma unroll
                for (int k = 0; k < V; ++k) p.s[g * p.C + c0 + k] = init_final(p, best_s[k], bad[k]);
            }
        }
    }
}

template <int M, bool RNE, int V>
__global__ __launch_bounds__(kBlock) void k_init_rows(const InitParams p, const int log_team) {
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const uint32_t pairs = (uint32_t)p.R * (uint32_t)p.nb;      // <= R * C < 2^31
    const uint32_t pair = blockIdx.x * (uint32_t)(kBlock >> log_team) + (threadIdx.x >> log_team);
    const bool live = pair < pairs;
    int64_t base = 0, c0 = 0, c1 = 0;
    InitAcc a = InitAcc{0.f, 0.f, 0.0, 0u};
    init_start<M>(a);
    if (live) {
        const uint32_t r = pair / (uint32_t)p.nb, g = pair - r * (uint32_t)p.nb;
        base = (int64_t)r * p.C;
        c0 = (int64_t)g * p.gs;
        c1 = (c0 + p.gs < p.C) ? c0 + p.gs : p.C;
        for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {      // V = 4: gs % 4 == 0 and C % 4 == 0
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + base + col);
                init_take<M>(x.x, a);
                init_take<M>(x.y, a);
                init_take<M>(x.z, a);
                init_take<M>(x.w, a);
            } else {
                init_take<M>(p.P[base + col], a);
            }
        }
    }
    for (int off = T >> 1; off > 0; off >>= 1) {      // fixed butterfly inside the aligned team: every lane ends with the total
        if constexpr (M == LQ_INIT_LSQ) init_merge<M>(a, 0.f, 0.f, __shfl_xor(a.sum, off), __shfl_xor(a.bad, off));
        else init_merge<M>(a, __shfl_xor(a.f0, off), __shfl_xor(a.f1, off), 0.0, __shfl_xor(a.bad, off));
    }
    const float raw = init_raw<M>(p, a, live ? c1 - c0 : 1);
    if constexpr (M != LQ_INIT_MSE) {
        if (live && lt == 0) {
            p.s[pair] = init_final(p, raw, a.bad);
            if constexpr (M == kInitMinMax) p.b[pair] = init_offset(p, a, raw);
        }
    } else {
        double E[kInitCandidates];
#pragma unroll
        for (int j = 0; j < kInitCandidates; ++j) E[j] = 0.0;
        if (live) {
            for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {
                if constexpr (V == 4) {
                    const float4 x = *reinterpret_cast<const float4*>(p.P + base + col);
                    mse_take<RNE, kInitCandidates>(p, x.x, raw, 0, E);
                    mse_take<RNE, kInitCandidates>(p, x.y, raw, 0, E);
                    mse_take<RNE, kInitCandidates>(p, x.z, raw, 0, E);
                    mse_take<RNE, kInitCandidates>(p, x.w, raw, 0, E);
                } else {
                    mse_take<RNE, kInitCandidates>(p, p.P[base + col], raw, 0, E);
                }
            }
        }
        for (int off = T >> 1; off > 0; off >>= 1) {
#pragma unroll
            for (int j = 0; j < kInitCandidates; ++j) E[j] += __shfl_xor(E[j], off);
        }
        if (live && lt == 0) {
            double best = E[0];
            float best_s = init_candidate(p, raw, 0);
#pragma unroll
            for (int j = 1; j < kInitCandidates; ++j) {
                if (E[j] < best) {      // strict <: on equal sums the smallest k stays
                    best = E[j];
                    best_s = init_candidate(p, raw, j);
                }
            }
            p.s[pair] = init_final(p, best_s, a.bad);
        }
    }
}

}  // namespace lq

#endif
