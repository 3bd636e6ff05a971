// lq_group.hpp -- group-wise (block) scales of the clipped b-bit quantizer (lq_hip.h: lq_fq_forward_group / lq_fq_backward_group)
//
// The parameter is a matrix [R][C] in memory order, C contiguous.  axis 0: groups of `gs` rows per column, scale [nb][C];
// axis 1: groups of `gs` consecutive elements of a row, scale [R][nb]; nb = ceil(len / gs), the last group of a line may be short.
// Per element the arithmetic is the clipped pair's: K1's quotient (div_by_uniform / fq_quot4 / fq_quot4c of lq_math.hpp) and
// ClipBwdOp<RNE>::one / ClipBase<RNE>::clampq of lq_ops.hpp, the rounding a compile-time parameter.
//
//   k_group_cols  (axis 0)  a lane keeps V fixed columns (V = 4: one float4; V = 1: scalar columns), TX lanes lie side by side
//                           along a row and the 256 / TX row slots of the block split the rows of a group.  A block owns whole
//                           groups (blockIdx.y, grid-stride): the slots' f64 sums and counts meet in LDS, slot 0 adds them in
//                           slot order and emits ds and clipped itself.  The scale row changes every gs rows; the lane reloads
//                           its V contexts (one reciprocal each) there.  The forward has nothing to merge: where the grid is
//                           small it splits the rows of a group over up to 4 blocks (gridDim.z), two rows per lane at least.
//   k_group_rows  (axis 1)  a team of T = 2^k <= 64 lanes per (row, group): the lanes stride through the group's run (float4 where
//                           gs and C are multiples of 4 and the bases 16-byte aligned), a fixed xor butterfly inside the team adds
//                           the f64 sums and the counts, lane 0 of the team emits.  The scale is [R][nb]: pair index == scale index.
//
// Every sum has one fixed order (lane's own rows or elements in ascending order, then slots 0 .. or the butterfly): run-to-run
// bit-stable, no atomics, no second stage and therefore no workspace.  The forward is the same traversal without dy and sums.
// The work of one block is a __device__ function of the block's coordinates (group_cols_body, group_rows_body): the kernels here and
// the multi-tensor k_group_batch (lq_group_batch.hpp) both call it.
#ifndef LQ_GROUP_HPP_
#define LQ_GROUP_HPP_
#include "lq_ops.hpp"

namespace lq {

struct GroupParams {
    const float* P;
    const float* s;
    const float* dy;      // backward only
    float* out;           // forward: out; backward: dP
    void* q;              // forward: optional clamped integers
    int q_dtype;
    float lo, hi;         // (float)qmin, (float)qmax
    float k;              // grad_scale
    float* ds;            // backward, may be NULL
    uint32_t* clipped;    // backward, may be NULL
    int32_t R, C, gs, nb; // R * C < 2^31; gs is clamped to the line length by the host
};

template <bool RNE>
__device__ __forceinline__ Ctx group_ctx(const GroupParams& p, float s) {
    Ctx c;
    c.s = s;
    div_ctx(c);
    c.k0 = p.lo;
    c.k1 = p.hi;
    c.lam_hi = 0.f;
    c.sure_ok = 0;
    return c;
}

// one element: forward returns out and hands q to the integer view; backward returns dP and accumulates
template <bool RNE, bool BWD>
__device__ __forceinline__ float group_elem(const GroupParams& p, const Ctx& c, int64_t i, float t, float dy, Acc& acc) {
    if constexpr (BWD) {
        return ClipBwdOp<RNE>::one(t, dy, c.k0, c.k1, acc);
    } else {
        const float q = ClipBase<RNE>::clampq(ClipBase<RNE>::rnd(t), c.k0, c.k1);
        if (p.q) store_q(p.q, p.q_dtype, i, q);
        return q * c.s;
    }
}

constexpr int kGroupColsLanes4 = 16;      // V = 4: 16 lanes x float4 = 64 columns (256 bytes of a row), 16 row slots
constexpr int kGroupColsLanes1 = 64;      // V = 1: 64 lanes = 64 columns, 4 row slots (one wave each)

// The work of one block of k_group_cols on group g of column tile bx: the single-tensor kernel below and the multi-tensor batch
// (lq_group_batch.hpp) both run this body, so a tensor's bits do not depend on which launch carried it.  zi / nz: this block's
// share of the group's rows (forward only: nothing to merge).  sh_sum / sh_cnt: [256 / TX][TX * V] in LDS (backward only).
// Every thread of the block must call it (two barriers when `reduce`).
template <bool RNE, bool BWD, int V, int TX>
__device__ __forceinline__ void group_cols_body(const GroupParams& p, const int64_t bx, const int64_t g, const int zi, const int nz,
                                                const bool reduce, double* sh_sum, uint32_t* sh_cnt) {
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    const int lx = (int)threadIdx.x % TX, slot = (int)threadIdx.x / TX;
    const int64_t c0 = (bx * TX + lx) * V;
    const bool live = c0 < p.C;      // V = 4 runs only with C % 4 == 0: the lane's four columns are inside together
    Acc acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = Acc{0u, 0u, 0.0};
    if (live) {
        const int64_t r0 = g * p.gs;
        const int64_t r1 = (r0 + p.gs < p.R) ? r0 + p.gs : p.R;
        Ctx c[V];
#pragma unroll
        for (int k = 0; k < V; ++k) c[k] = group_ctx<RNE>(p, p.s[g * p.C + c0 + k]);
#pragma unroll 2
        // nz > 1 (forward only: nothing to merge) spreads the rows of a group over that many blocks
        for (int64_t r = r0 + zi * SLOTS + slot; r < r1; r += (int64_t)SLOTS * nz) {
            const int64_t i = r * p.C + c0;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (BWD) dy = *reinterpret_cast<const float4*>(p.dy + i);
                const float4 t = fq_quot4c(x, c);
                float4 o;
                o.x = group_elem<RNE, BWD>(p, c[0], i + 0, t.x, dy.x, acc[0]);
                o.y = group_elem<RNE, BWD>(p, c[1], i + 1, t.y, dy.y, acc[1]);
                o.z = group_elem<RNE, BWD>(p, c[2], i + 2, t.z, dy.z, acc[2]);
                o.w = group_elem<RNE, BWD>(p, c[3], i + 3, t.w, dy.w, acc[3]);
                *reinterpret_cast<float4*>(p.out + i) = o;
            } else {
                const float x = p.P[i];
                float dy = 0.f;
                if constexpr (BWD) dy = p.dy[i];
                p.out[i] = group_elem<RNE, BWD>(p, c[0], i, div_by_uniform(x, c[0]), dy, acc[0]);
            }
        }
    }
    if constexpr (BWD) {
        if (reduce) {      // block-uniform: every thread meets the barriers
#pragma unroll
            for (int k = 0; k < V; ++k) {
                sh_sum[slot * COLS + lx * V + k] = acc[k].c;
                sh_cnt[slot * COLS + lx * V + k] = acc[k].b;
            }
            __syncthreads();
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
            }
            __syncthreads();
        }
    }
}

template <bool RNE, bool BWD, int V, int TX>
__global__ __launch_bounds__(kBlock) void k_group_cols(const GroupParams p) {
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    __shared__ double sh_sum[BWD ? SLOTS * COLS : 1];
    __shared__ uint32_t sh_cnt[BWD ? SLOTS * COLS : 1];
    const bool reduce = BWD && (p.ds != nullptr || p.clipped != nullptr);      // kernel-uniform
    // the trip count of the group loop is block-uniform
    for (int64_t g = blockIdx.y; g < p.nb; g += gridDim.y)
        group_cols_body<RNE, BWD, V, TX>(p, (int64_t)blockIdx.x, g, (int)blockIdx.z, (int)gridDim.z, reduce, sh_sum, sh_cnt);
}

// The work of block `blk` of k_group_rows: kBlock >> log_team (row, group) pairs, a team of 1 << log_team lanes each.  No barrier.
template <bool RNE, bool BWD, int V>
__device__ __forceinline__ void group_rows_body(const GroupParams& p, const int log_team, const uint32_t blk) {
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const uint32_t pairs = (uint32_t)p.R * (uint32_t)p.nb;      // <= R * C < 2^31
    const uint32_t pair = blk * (uint32_t)(kBlock >> log_team) + (threadIdx.x >> log_team);
    const bool live = pair < pairs;
    Acc acc = Acc{0u, 0u, 0.0};
    if (live) {
        const uint32_t r = pair / (uint32_t)p.nb, g = pair - r * (uint32_t)p.nb;
        const int64_t base = (int64_t)r * p.C;
        const int64_t c0 = (int64_t)g * p.gs;
        const int64_t c1 = (c0 + p.gs < p.C) ? c0 + p.gs : p.C;
        const Ctx c = group_ctx<RNE>(p, p.s[pair]);
        for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {      // V = 4: gs % 4 == 0 and C % 4 == 0
            const int64_t i = base + col;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (BWD) dy = *reinterpret_cast<const float4*>(p.dy + i);
                const float4 t = fq_quot4(x, c);
                float4 o;
                o.x = group_elem<RNE, BWD>(p, c, i + 0, t.x, dy.x, acc);
                o.y = group_elem<RNE, BWD>(p, c, i + 1, t.y, dy.y, acc);
                o.z = group_elem<RNE, BWD>(p, c, i + 2, t.z, dy.z, acc);
                o.w = group_elem<RNE, BWD>(p, c, i + 3, t.w, dy.w, acc);
                *reinterpret_cast<float4*>(p.out + i) = o;
            } else {
                const float x = p.P[i];
                float dy = 0.f;
                if constexpr (BWD) dy = p.dy[i];
                p.out[i] = group_elem<RNE, BWD>(p, c, i, div_by_uniform(x, c), dy, acc);
            }
        }
    }
    if constexpr (BWD) {
        if (p.ds != nullptr || p.clipped != nullptr) {      // block-uniform
            double sum = acc.c;
            uint32_t cnt = acc.b;
            for (int off = T >> 1; off > 0; off >>= 1) {      // fixed butterfly inside the aligned team; every lane of the wave takes part
                sum += __shfl_xor(sum, off);
                cnt += __shfl_xor(cnt, off);
            }
            if (live && lt == 0) {
                if (p.ds) p.ds[pair] = (float)((double)p.k * sum);
                if (p.clipped) p.clipped[pair] = cnt;
            }
        }
    }
}

template <bool RNE, bool BWD, int V>
__global__ __launch_bounds__(kBlock) void k_group_rows(const GroupParams p, const int log_team) {
    group_rows_body<RNE, BWD, V>(p, log_team, blockIdx.x);
}

}  // namespace lq

#endif
