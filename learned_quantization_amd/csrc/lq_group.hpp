// lq_group.hpp -- group-wise (block) scales of the clipped b-bit quantizer, with or without a learned offset per group
// (lq_hip.h: lq_fq_forward_group / lq_fq_backward_group, lq_fq_forward_group_affine / lq_fq_backward_group_affine)
//
// The parameter is a matrix [R][C] in memory order, C contiguous.  axis 0: groups of `gs` rows per column, scale [nb][C];
// axis 1: groups of `gs` consecutive elements of a row, scale [R][nb]; nb = ceil(len / gs), the last group of a line may be short.
// Per element the arithmetic is the clipped pair's: K1's quotient (div_by_uniform / fq_quot4 / fq_quot4c of lq_math.hpp) and
// ClipBwdOp<RNE>::one / ClipBase<RNE>::clampq of lq_ops.hpp, the rounding a compile-time parameter.  With an offset b per group:
//
//   u = P - b;  t = u / s;  q0 = rnd(t);  q = clamp(q0, lo, hi);  out = (q * s) + b      (every operation rounds on its own)
//   inside = lo <= q0 <= hi;  dP = inside ? dy : +0;  r = inside ? q0 - t : q
//   ds[g] = RN(k * sum dy * r);  db[g] = RN(kb * sum_{!inside} dy);  clipped[g] = #{!inside}      (sums in f64)
//
// The symmetric pair is the same without b, db and the second sum (with b == +0 u is P bit for bit, and dP, ds and clipped are
// its bits).  The library is built without contraction: q * s + b is a product and a sum.
//
// There is ONE traversal body per axis.  Whether an offset travels along is a compile-time property of the parameter struct the
// body is called with (GroupParams / GroupAffineParams); what the offset adds sits behind `if constexpr`:
//
//   group_cols_body  (axis 0)  a lane keeps V fixed columns (V = 4: one float4; V = 1: scalar columns), TX lanes lie side by side
//                              along a row and the 256 / TX row slots of the block split the rows of a group.  A block owns whole
//                              groups: the slots' f64 sums and counts meet in LDS, slot 0 adds them in slot order and emits ds and
//                              clipped itself; the offset's sums lie in a second array that slot 1 adds in the same order at the
//                              same time and emits as db.  The scale row changes every gs rows; the lane reloads its V contexts
//                              (one reciprocal each; the offset is indexed like the scale) there.  The forward has nothing to merge:
//                              where the grid is small it splits the rows of a group over up to 4 blocks, two rows per lane at least.
//   group_rows_body  (axis 1)  a team of T = 2^k <= 64 lanes per (row, group): the lanes stride through the group's run (float4 where
//                              gs and C are multiples of 4 and the bases 16-byte aligned), a fixed xor butterfly inside the team adds
//                              the f64 sums and the counts, lane 0 of the team emits.  Scale and offset are [R][nb]: pair index ==
//                              scale index.
//
// Every sum has one fixed order (lane's own rows or elements in ascending order, then slots 0 .. or the butterfly): run-to-run
// bit-stable, no atomics, no second stage and therefore no workspace.  The forward is the same traversal without dy and sums.
// What depends on the element grid -- the context of a group from its stored scale, the clamped grid value of a quotient, what the
// integer view holds, the backward's term -- the bodies ask of GroupStep<RNE, PT>: the integer grid here, the minifloat grids of
// the microscaling formats in lq_mx.hpp (k_group_mx_cols / k_group_mx_rows).
// The kernels are wrappers that own the LDS and hand the body its block's coordinates: k_group_cols / k_group_rows and
// k_group_affine_cols / k_group_affine_rows here (blockIdx.y strides over the groups, blockIdx.z shares a group's rows in the
// forward) and the multi-tensor k_group_batch (lq_group_batch.hpp), so a tensor's bits do not depend on which launch carried it.
#ifndef LQ_GROUP_HPP_
#define LQ_GROUP_HPP_
#include <type_traits>
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

struct GroupAffineParams {
    GroupParams g;        // P, s, dy, out / dP, q, range, k, ds, clipped, geometry: as the symmetric pair
    const float* b;       // offset, the scale's shape
    float* db;            // backward, may be NULL
    float kb;             // offset_grad_scale
};

template <class PT>      // GroupAffineParams, or a struct derived from it (the batch's: lq_group_batch.hpp)
constexpr bool kGroupHasOffset = std::is_base_of_v<GroupAffineParams, PT>;
__host__ __device__ __forceinline__ const GroupParams& group_base(const GroupParams& p) { return p; }
__host__ __device__ __forceinline__ const GroupParams& group_base(const GroupAffineParams& ap) { return ap.g; }

__device__ __forceinline__ float* group_db(const GroupParams&) { return nullptr; }      // no offset: no db
__device__ __forceinline__ float* group_db(const GroupAffineParams& ap) { return ap.db; }

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

// backward with an offset: ClipBwdOp's term on t, and dy of a clipped element into the offset's sum.  dP == dy (bitwise, or both
// NaN) exactly where the element is inside, except for dy == 0 and NaN dy, so `inside` is taken from q0 again: the compiler merges the two.
template <bool RNE>
__device__ __forceinline__ float affine_bwd_one(float t, float dy, float lo, float hi, Acc& acc, double& accb) {
    const float q0 = ClipBase<RNE>::rnd(t);
    const bool inside = (q0 >= lo) & (q0 <= hi);
    accb += inside ? 0.0 : (double)dy;
    return ClipBwdOp<RNE>::one(t, dy, lo, hi, acc);
}

// The element step of a parameter struct: the context of a group from its stored scale, the clamped grid value of a quotient, what
// the integer view holds for it, and the backward's term.  This one is the integer grid (GroupParams, GroupAffineParams and what
// derives from them); lq_mx.hpp specialises it for the minifloat grids under a power-of-two scale.
template <bool RNE, class PT>
struct GroupStep {
    __device__ static __forceinline__ Ctx ctx(const PT& pp, float s) { return group_ctx<RNE>(group_base(pp), s); }
    __device__ static __forceinline__ float quant(const PT&, const Ctx& c, float t) { return ClipBase<RNE>::clampq(ClipBase<RNE>::rnd(t), c.k0, c.k1); }
    __device__ static __forceinline__ float view(const PT&, float q) { return q; }
    __device__ static __forceinline__ float bwd(const PT&, const Ctx& c, float t, float dy, Acc& acc) { return ClipBwdOp<RNE>::one(t, dy, c.k0, c.k1, acc); }
};

// one element: forward returns out and hands q to the integer view; backward returns dP and accumulates.  b, accb: AFF only
template <bool RNE, bool BWD, class PT>
__device__ __forceinline__ float group_elem(const PT& pp, const Ctx& c, float b, int64_t i, float t, float dy, Acc& acc, double& accb) {
    constexpr bool AFF = kGroupHasOffset<PT>;
    using Step = GroupStep<RNE, PT>;
    const GroupParams& p = group_base(pp);
    if constexpr (BWD) {
        if constexpr (AFF) return affine_bwd_one<RNE>(t, dy, c.k0, c.k1, acc, accb);
        else return Step::bwd(pp, c, t, dy, acc);
    } else {
        const float q = Step::quant(pp, c, t);
        if (p.q) store_q(p.q, p.q_dtype, i, Step::view(pp, q));
        const float m = q * c.s;
        if constexpr (AFF) return m + b;
        else return m;
    }
}

constexpr int kGroupColsLanes4 = 16;      // V = 4: 16 lanes x float4 = 64 columns (256 bytes of a row), 16 row slots
constexpr int kGroupColsLanes1 = 64;      // V = 1: 64 lanes = 64 columns, 4 row slots (one wave each)

// The work of one block of a column kernel on group g of column tile bx.  zi / nz: this block's share of the group's rows (forward
// only: nothing to merge).  sh_sum / sh_sumb / sh_cnt: [256 / TX][TX * V] in LDS (backward only; sh_sumb with an offset only, else
// NULL).  Every thread of the block must call it (two barriers when `reduce`, which is block-uniform).
template <bool RNE, bool BWD, int V, int TX, class PT>
__device__ __forceinline__ void group_cols_body(const PT& pp, const int64_t bx, const int64_t g, const int zi, const int nz,
                                                const bool reduce, double* sh_sum, double* sh_sumb, uint32_t* sh_cnt) {
    constexpr bool AFF = kGroupHasOffset<PT>;
    constexpr int SLOTS = kBlock / TX;
    constexpr int COLS = TX * V;
    static_assert(!AFF || SLOTS >= 2, "slot 1 merges the offset's sums");
    const GroupParams& p = group_base(pp);
    const int lx = (int)threadIdx.x % TX, slot = (int)threadIdx.x / TX;
    const int64_t c0 = (bx * TX + lx) * V;
    const bool live = c0 < p.C;      // V = 4 runs only with C % 4 == 0: the lane's four columns are inside together
    Acc acc[V];
    double accb[V];                  // AFF: sum of dy over the lane's clipped elements
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
            c[k] = GroupStep<RNE, PT>::ctx(pp, p.s[g * p.C + c0 + k]);
            if constexpr (AFF) b[k] = pp.b[g * p.C + c0 + k];
            else b[k] = 0.f;
        }
        // Two rows in flight, except in the backward with an offset: there they cost 106 VGPRs with the second f64 accumulator, 4
        // waves per SIMD instead of 6, and a second round of blocks on weight-sized tensors.
        // nz > 1 (forward only: nothing to merge) spreads the rows of a group over that many blocks
        constexpr int kRowsInFlight = AFF && BWD ? 1 : 2;
#pragma unroll kRowsInFlight
        for (int64_t r = r0 + zi * SLOTS + slot; r < r1; r += (int64_t)SLOTS * nz) {
            const int64_t i = r * p.C + c0;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (BWD) dy = *reinterpret_cast<const float4*>(p.dy + i);
                float4 t;
                if constexpr (AFF) t = fq_quot4c(make_float4(x.x - b[0], x.y - b[1], x.z - b[2], x.w - b[3]), c);
                else t = fq_quot4c(x, c);
                float4 o;
                o.x = group_elem<RNE, BWD>(pp, c[0], b[0], i + 0, t.x, dy.x, acc[0], accb[0]);
                o.y = group_elem<RNE, BWD>(pp, c[1], b[1], i + 1, t.y, dy.y, acc[1], accb[1]);
                o.z = group_elem<RNE, BWD>(pp, c[2], b[2], i + 2, t.z, dy.z, acc[2], accb[2]);
                o.w = group_elem<RNE, BWD>(pp, c[3], b[3], i + 3, t.w, dy.w, acc[3], accb[3]);
                *reinterpret_cast<float4*>(p.out + i) = o;
            } else {
                float u = p.P[i];
                float dy = 0.f;
                if constexpr (BWD) dy = p.dy[i];
                if constexpr (AFF) u = u - b[0];
                p.out[i] = group_elem<RNE, BWD>(pp, c[0], b[0], i, div_by_uniform(u, c[0]), dy, acc[0], accb[0]);
            }
        }
    }
    if constexpr (BWD) {
        if (reduce) {      // block-uniform: every thread meets the barriers
#pragma unroll
            for (int k = 0; k < V; ++k) {
                sh_sum[slot * COLS + lx * V + k] = acc[k].c;
                if constexpr (AFF) sh_sumb[slot * COLS + lx * V + k] = accb[k];
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
            } else if (AFF && slot == 1 && live && group_db(pp)) {
                // Slot 1 adds the offset's sums in the same slot order while slot 0 adds the scale's: the merge takes no longer with an
                // offset than without.  `AFF &&` is a compile-time constant (without an offset the branch folds away; group_db's
                // GroupParams overload exists so that the condition compiles) and the branch stays an `else` of slot 0's: as a
                // separate `if constexpr { if ... }` the affine backward kernels get another instruction stream than they shipped with.
                if constexpr (AFF) {
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        double sumb = sh_sumb[lx * V + k];
                        for (int w = 1; w < SLOTS; ++w) sumb += sh_sumb[w * COLS + lx * V + k];
                        pp.db[g * p.C + c0 + k] = (float)((double)pp.kb * sumb);
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <bool RNE, bool BWD, int V, int TX>
__global__ __launch_bounds__(kBlock) void k_group_cols(const GroupParams p) {
    constexpr int N = BWD ? (kBlock / TX) * (TX * V) : 1;
    __shared__ double sh_sum[N];
    __shared__ uint32_t sh_cnt[N];
    const bool reduce = BWD && (p.ds != nullptr || p.clipped != nullptr);      // kernel-uniform
    // the trip count of the group loop is block-uniform
    for (int64_t g = blockIdx.y; g < p.nb; g += gridDim.y)
        group_cols_body<RNE, BWD, V, TX>(p, (int64_t)blockIdx.x, g, (int)blockIdx.z, (int)gridDim.z, reduce, sh_sum, nullptr, sh_cnt);
}

template <bool RNE, bool BWD, int V, int TX>
__global__ __launch_bounds__(kBlock) void k_group_affine_cols(const GroupAffineParams ap) {
    constexpr int N = BWD ? (kBlock / TX) * (TX * V) : 1;
    __shared__ double sh_sum[N];
    __shared__ double sh_sumb[N];
    __shared__ uint32_t sh_cnt[N];
    const bool reduce = BWD && (ap.g.ds != nullptr || ap.db != nullptr || ap.g.clipped != nullptr);      // kernel-uniform
    for (int64_t g = blockIdx.y; g < ap.g.nb; g += gridDim.y)
        group_cols_body<RNE, BWD, V, TX>(ap, (int64_t)blockIdx.x, g, (int)blockIdx.z, (int)gridDim.z, reduce, sh_sum, sh_sumb, sh_cnt);
}

// The work of block `blk` of a row kernel: kBlock >> log_team (row, group) pairs, a team of 1 << log_team lanes each.  No barrier.
template <bool RNE, bool BWD, int V, class PT>
__device__ __forceinline__ void group_rows_body(const PT& pp, const int log_team, const uint32_t blk) {
    constexpr bool AFF = kGroupHasOffset<PT>;
    const GroupParams& p = group_base(pp);
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const uint32_t pairs = (uint32_t)p.R * (uint32_t)p.nb;      // <= R * C < 2^31
    const uint32_t pair = blk * (uint32_t)(kBlock >> log_team) + (threadIdx.x >> log_team);
    const bool live = pair < pairs;
    Acc acc = Acc{0u, 0u, 0.0};
    double accb = 0.0;               // AFF: sum of dy over the lane's clipped elements
    if (live) {
        const uint32_t r = pair / (uint32_t)p.nb, g = pair - r * (uint32_t)p.nb;
        const int64_t base = (int64_t)r * p.C;
        const int64_t c0 = (int64_t)g * p.gs;
        const int64_t c1 = (c0 + p.gs < p.C) ? c0 + p.gs : p.C;
        const Ctx c = GroupStep<RNE, PT>::ctx(pp, p.s[pair]);
        float b = 0.f;
        if constexpr (AFF) b = pp.b[pair];
        for (int64_t col = c0 + (int64_t)lt * V; col < c1; col += (int64_t)T * V) {      // V = 4: gs % 4 == 0 and C % 4 == 0
            const int64_t i = base + col;
            if constexpr (V == 4) {
                const float4 x = *reinterpret_cast<const float4*>(p.P + i);
                float4 dy = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (BWD) dy = *reinterpret_cast<const float4*>(p.dy + i);
                float4 t;
                if constexpr (AFF) t = fq_quot4(make_float4(x.x - b, x.y - b, x.z - b, x.w - b), c);
                else t = fq_quot4(x, c);
                float4 o;
                o.x = group_elem<RNE, BWD>(pp, c, b, i + 0, t.x, dy.x, acc, accb);
                o.y = group_elem<RNE, BWD>(pp, c, b, i + 1, t.y, dy.y, acc, accb);
                o.z = group_elem<RNE, BWD>(pp, c, b, i + 2, t.z, dy.z, acc, accb);
                o.w = group_elem<RNE, BWD>(pp, c, b, i + 3, t.w, dy.w, acc, accb);
                *reinterpret_cast<float4*>(p.out + i) = o;
            } else {
                float u = p.P[i];
                float dy = 0.f;
                if constexpr (BWD) dy = p.dy[i];
                if constexpr (AFF) u = u - b;
                p.out[i] = group_elem<RNE, BWD>(pp, c, b, i, div_by_uniform(u, c), dy, acc, accb);
            }
        }
    }
    if constexpr (BWD) {
        if (p.ds != nullptr || group_db(pp) != nullptr || p.clipped != nullptr) {      // block-uniform
            double sum = acc.c;
            double sumb = accb;
            uint32_t cnt = acc.b;
            for (int off = T >> 1; off > 0; off >>= 1) {      // fixed butterfly inside the aligned team; every lane of the wave takes part
                sum += __shfl_xor(sum, off);
                if constexpr (AFF) sumb += __shfl_xor(sumb, off);
                cnt += __shfl_xor(cnt, off);
            }
            if (live && lt == 0) {
                if (p.ds) p.ds[pair] = (float)((double)p.k * sum);
                if constexpr (AFF) {
                    if (pp.db) pp.db[pair] = (float)((double)pp.kb * sumb);
                }
                if (p.clipped) p.clipped[pair] = cnt;
            }
        }
    }
}

template <bool RNE, bool BWD, int V>
__global__ __launch_bounds__(kBlock) void k_group_rows(const GroupParams p, const int log_team) {
    group_rows_body<RNE, BWD, V>(p, log_team, blockIdx.x);
}

template <bool RNE, bool BWD, int V>
__global__ __launch_bounds__(kBlock) void k_group_affine_rows(const GroupAffineParams ap, const int log_team) {
    group_rows_body<RNE, BWD, V>(ap, log_team, blockIdx.x);
}

}  // namespace lq

#endif
