// lq_group_batch.hpp -- group-wise tensors in one launch per pass (lq_hip.h: lq_group_batch_*)
//
// A table of tasks built at create time, one per tensor: the tensor's GroupParams, the single-tensor form that
// lq_fq_*_group picks for the same geometry and alignment, and the first block of the task.  A block reads its task from a
// per-block table (block_task, as k_batch_traverse of lq_batch.hpp), finds its unit inside the task and runs the body of that
// form -- the same __device__ function the single-tensor kernel runs (lq_group.hpp), so out, dP, the counts AND ds are the
// single-tensor call's bit for bit: the form, V, the slot count, the butterfly and the order of a lane's own elements are the same.
//
//   column forms (axis 0)   one unit per (column tile, group); the forward keeps the single-tensor row split (nz blocks per group),
//                           the backward is one block per group: the LDS merge in slot order needs the whole group in one block
//   row forms (axis 1)      one unit per kBlock >> log_team (row, group) pairs, log_team by group_launch's rule
//
// No partials, no finalize, no workspace: the whole backward of a model (masked dP, ds, clip counts) is ONE launch.
// Upstream gradients and grad_scale travel by value in the kernel arguments (PtrPack 2 KB + CoefPack 1 KB + three words: below
// the 4 KB limit of the argument block).  The form branch is block-uniform; only the backward column forms have barriers and every
// thread of such a block reaches both.  The backward's static LDS is the float4 column form's 12 KB for every form: 13 blocks per
// CU by LDS, above the 8 blocks of 256 threads a CU holds, so it never bounds occupancy.  The forward uses no LDS.
//
// Tensors with a learned offset per group (lq_group_batch_create_affine) run k_group_batch_affine on a table of GroupAffineTask:
// a GroupTask followed by the offset b, its gradient db and the gradient's factor kb.  kb lives in the table, fixed at create
// time, because the argument block has no room for a second 1 KB coefficient pack.  A task with b == NULL (a bias of an asymmetric
// model) calls the bodies with GroupParams, literally what k_group_batch does, so it keeps the symmetric bits, -0.0 included; a
// task with b calls them with GroupAffineParams, as k_group_affine_cols / k_group_affine_rows do.  That branch is block-uniform
// too.  k_group_batch and the GroupTask table of a batch without offsets are untouched.
// Resources of k_group_batch_affine on gfx950 (compiler's report, profiles/group_affine_batch/kernel_resources.txt):
//   forward   44 VGPRs, 68 SGPRs, no LDS, no scratch, 8 waves per SIMD      (k_group_batch: 39 VGPRs, 8 waves)
//   backward  72 VGPRs, 94 SGPRs, 20480 bytes of LDS, no scratch, 7 waves per SIMD      (k_group_batch: 66 VGPRs, 12288 bytes, 7 waves)
// The backward's static LDS is 8 KB sh_sum + 8 KB sh_sumb + 4 KB sh_cnt = 20 KB for every form: 8 blocks x 20 KB are the CU's
// 160 KB, exactly the 8 blocks of 256 threads a CU holds, so the 72 registers bound occupancy (7 waves) before LDS does.  The
// float4 column body keeps its one row in flight (lq_group.hpp, unroll(1) with an offset in the backward).
//
// Microscaling tensors (lq_group_batch_create_mx) run k_group_batch_mx on a table of GroupMxTask: a GroupTask followed by the
// values of the tensor's element format and scale format (M, emin, bits, e8m0_mask; lo / hi of the GroupParams are the format's
// -max / +max).  The format is the task's own: one batch holds tensors of different formats.  A block builds the MX parameter
// struct from its task and runs the bodies with the element step of lq_mx.hpp, what k_group_mx_cols / k_group_mx_rows run, so
// out, dP, the saturation counts and ds are lq_fq_*_mx's bit for bit, a bias (the one-group line) included.  The format values are
// block-uniform where the single-tensor kernels have them kernel-uniform: the table is read at a uniform index with scalar loads
// (the four words after the GroupTask come by one s_load_dwordx4 in the forward, s_load_dwordx2 + 2 x s_load_dword in the
// backward) and they stay in scalar registers.
// Resources of k_group_batch_mx on gfx950 (compiler's report, profiles/mx_batch/kernel_resources.txt):
//   forward   39 VGPRs, 70 SGPRs, no LDS, no scratch, 8 waves per SIMD      (k_group_batch: 39 VGPRs, 8 waves)
//   backward  64 VGPRs, 78 SGPRs, 12288 bytes of LDS, no scratch, 8 waves per SIMD
//             (k_group_batch: 66 VGPRs, 12288 bytes, 7 waves; k_group_mx_cols<true, 4, 16>: 76 VGPRs, 12288 bytes, 6 waves)
// The backward's static LDS is the symmetric batch's (8 KB sh_sum + 4 KB sh_cnt; there is no sh_sumb).
#ifndef LQ_GROUP_BATCH_HPP_
#define LQ_GROUP_BATCH_HPP_
#include "lq_group.hpp"
#include "lq_batch.hpp"
#include "lq_mx.hpp"

namespace lq {

enum : int32_t { GROUP_COLS4 = 0, GROUP_COLS1 = 1, GROUP_ROWS4 = 2, GROUP_ROWS1 = 3 };

struct GroupTask {
    GroupParams p;            // forward table: out; backward table: out = dp, ds, clipped = the batch-owned counts
    int32_t form;             // GROUP_*
    int32_t log_team;         // row forms
    uint32_t first_block;     // prefix over the blocks of the launch
    uint32_t nbx;             // column forms: column tiles
    uint32_t nz;              // column forms, forward: blocks per (column tile, group)
    uint32_t pad;
};

constexpr int kGroupBatchLdsSum = (kBlock / kGroupColsLanes4) * (kGroupColsLanes4 * 4);      // 16 slots x 64 columns

template <bool RNE, bool BWD>
__global__ __launch_bounds__(kBlock) void k_group_batch(const GroupTask* __restrict__ tasks, const uint32_t* __restrict__ block_task,
                                                        PtrPack pk, CoefPack cf, int mask_only) {
    __shared__ double sh_sum[BWD ? kGroupBatchLdsSum : 1];
    __shared__ uint32_t sh_cnt[BWD ? kGroupBatchLdsSum : 1];
    const int ti = (int)block_task[blockIdx.x];
    const GroupTask& t = tasks[ti];
    GroupParams p = t.p;
    if constexpr (BWD) {
        p.dy = pk.dy[ti];
        p.k = cf.c[ti];
        if (mask_only) p.ds = nullptr;
    }
    const uint32_t b = blockIdx.x - t.first_block;
    if (t.form <= GROUP_COLS1) {       // block-uniform
        const uint32_t bx = b % t.nbx, rest = b / t.nbx;
        const uint32_t g = rest % (uint32_t)p.nb, z = rest / (uint32_t)p.nb;      // backward: nz == 1, z == 0
        if (t.form == GROUP_COLS4) group_cols_body<RNE, BWD, 4, kGroupColsLanes4>(p, (int64_t)bx, (int64_t)g, (int)z, (int)t.nz, BWD, sh_sum, nullptr, sh_cnt);
        else group_cols_body<RNE, BWD, 1, kGroupColsLanes1>(p, (int64_t)bx, (int64_t)g, (int)z, (int)t.nz, BWD, sh_sum, nullptr, sh_cnt);
    } else if (t.form == GROUP_ROWS4) {
        group_rows_body<RNE, BWD, 4>(p, t.log_team, b);
    } else {
        group_rows_body<RNE, BWD, 1>(p, t.log_team, b);
    }
}

// A GroupTask that may carry an offset: the affine table's entry.  b == NULL: a symmetric tensor, db and kb unused.
struct GroupAffineTask {
    GroupTask t;
    const float* b;           // offset, the scale's shape, or NULL
    float* db;                // backward table: offset gradient or NULL; forward table: NULL
    float kb;                 // offset_grad_scale, fixed at create time
    uint32_t pad;
};

// The batch's own name for GroupAffineParams (kGroupHasOffset holds for it): the bodies are instantiated apart from the
// single-tensor kernels' copies.  With the shared instantiation the compiler built k_group_affine_cols<*, true, *, *> differently
// once it had a second caller (float4 form: 170 VGPRs and 2 waves per SIMD instead of 76 and 6); with a type of its own every
// kernel the library had keeps its instruction stream (tools/asm_compare.py) and the source of the bodies is still one.
struct GroupBatchAffineParams : GroupAffineParams {};

// The work of one block on its task's unit: the form branch of k_group_batch for either parameter struct
template <bool RNE, bool BWD, class PT>
__device__ __forceinline__ void group_batch_unit(const PT& pp, const GroupTask& t, const uint32_t b, double* sh_sum, double* sh_sumb,
                                                 uint32_t* sh_cnt) {
    const GroupParams& p = group_base(pp);
    if (t.form <= GROUP_COLS1) {       // block-uniform
        const uint32_t bx = b % t.nbx, rest = b / t.nbx;
        const uint32_t g = rest % (uint32_t)p.nb, z = rest / (uint32_t)p.nb;      // backward: nz == 1, z == 0
        if (t.form == GROUP_COLS4) group_cols_body<RNE, BWD, 4, kGroupColsLanes4>(pp, (int64_t)bx, (int64_t)g, (int)z, (int)t.nz, BWD, sh_sum, sh_sumb, sh_cnt);
        else group_cols_body<RNE, BWD, 1, kGroupColsLanes1>(pp, (int64_t)bx, (int64_t)g, (int)z, (int)t.nz, BWD, sh_sum, sh_sumb, sh_cnt);
    } else if (t.form == GROUP_ROWS4) {
        group_rows_body<RNE, BWD, 4>(pp, t.log_team, b);
    } else {
        group_rows_body<RNE, BWD, 1>(pp, t.log_team, b);
    }
}

template <bool RNE, bool BWD>
__global__ __launch_bounds__(kBlock) void k_group_batch_affine(const GroupAffineTask* __restrict__ tasks, const uint32_t* __restrict__ block_task,
                                                               PtrPack pk, CoefPack cf, int mask_only) {
    __shared__ double sh_sum[BWD ? kGroupBatchLdsSum : 1];
    __shared__ double sh_sumb[BWD ? kGroupBatchLdsSum : 1];
    __shared__ uint32_t sh_cnt[BWD ? kGroupBatchLdsSum : 1];
    const int ti = (int)block_task[blockIdx.x];
    const GroupAffineTask& at = tasks[ti];
    const GroupTask& t = at.t;
    GroupBatchAffineParams ap;
    ap.g = t.p;
    ap.b = at.b;
    ap.db = nullptr;
    ap.kb = at.kb;
    if constexpr (BWD) {
        ap.g.dy = pk.dy[ti];
        ap.g.k = cf.c[ti];
        ap.db = at.db;
        if (mask_only) {
            ap.g.ds = nullptr;
            ap.db = nullptr;
        }
    }
    const uint32_t b = blockIdx.x - t.first_block;
    // block-uniform: every thread of a block takes the same side, and a column form's two barriers with it
    if (ap.b != nullptr) group_batch_unit<RNE, BWD>(ap, t, b, sh_sum, sh_sumb, sh_cnt);
    else group_batch_unit<RNE, BWD>(ap.g, t, b, sh_sum, nullptr, sh_cnt);
}

// A GroupTask of a microscaling tensor: the mx table's entry (lq_group_batch_create_mx).  The format is the task's own, so one
// batch holds tensors of different element formats and scale formats; t.p.lo / hi are the format's -max / +max.
struct GroupMxTask {
    GroupTask t;
    int32_t M, emin, bits;    // as GroupMxParams
    uint32_t e8m0_mask;
};

// The batch's own name for GroupMxParams, for the reason GroupBatchAffineParams has one: the bodies are instantiated apart from
// k_group_mx_cols / k_group_mx_rows, which keep their instruction streams.  The element step is GroupMxParams' own.
struct GroupBatchMxParams : GroupMxParams {};
template <bool RNE>
struct GroupStep<RNE, GroupBatchMxParams> : GroupStep<RNE, GroupMxParams> {};

// The format values (M, emin, bits, the scale-format mask, lo / hi) are block-uniform here where the single-tensor kernels have
// them kernel-uniform: they are read from the table at a uniform index, by scalar loads into scalar registers.
template <bool BWD>
__global__ __launch_bounds__(kBlock) void k_group_batch_mx(const GroupMxTask* __restrict__ tasks, const uint32_t* __restrict__ block_task,
                                                           PtrPack pk, CoefPack cf, int mask_only) {
    __shared__ double sh_sum[BWD ? kGroupBatchLdsSum : 1];
    __shared__ uint32_t sh_cnt[BWD ? kGroupBatchLdsSum : 1];
    const int ti = (int)block_task[blockIdx.x];
    const GroupMxTask& mt = tasks[ti];
    const GroupTask& t = mt.t;
    GroupBatchMxParams mp;
    mp.g = t.p;
    mp.M = mt.M;
    mp.emin = mt.emin;
    mp.bits = mt.bits;
    mp.e8m0_mask = mt.e8m0_mask;
    if constexpr (BWD) {
        mp.g.dy = pk.dy[ti];
        mp.g.k = cf.c[ti];
        if (mask_only) mp.g.ds = nullptr;
    }
    group_batch_unit<true, BWD>(mp, t, blockIdx.x - t.first_block, sh_sum, nullptr, sh_cnt);
}

}  // namespace lq

#endif
