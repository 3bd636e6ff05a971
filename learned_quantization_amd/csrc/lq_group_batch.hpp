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
#ifndef LQ_GROUP_BATCH_HPP_
#define LQ_GROUP_BATCH_HPP_
#include "lq_group.hpp"
#include "lq_batch.hpp"

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

}  // namespace lq

#endif
