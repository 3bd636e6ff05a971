// lq_kernels.hip -- hand-written gfx950 (MI355X / CDNA4) kernels for the learned-quantization
// hot path, and the C ABI of include/lq_hip.h on top of them.  One translation unit:
//
//   lq_common.hpp       constants, kernel parameter block, accumulator types
//   lq_math.hpp         exact fp32 arithmetic: uniform-divisor division, in-window ratio division, |tanh|, vote
//   lq_ops.hpp          per-operation traits (K1 fwd, K2 bwd, K4 fused, K5 penalties, integer view, STE scale gradient, clipped pairs: floor / nearest)
//   lq_reduce.hpp       wave/block reductions (DPP for the standard accumulator, shuffles for custom merges)
//   lq_traverse.hpp     traversal modes (row stream / row small / column) + finalize kernels
//   lq_stream2.hpp      streaming-size forms of the column and tiny-row modes (round 2): flat K1, pipelined column tile, ...
//   lq_aux_kernels.hpp  scale-sized kernels (K5c, K6), integer statistics, device self-test
//   lq_batch.hpp        device side of the multi-tensor batch
//   lq_pack.hpp         bit-packed integer view: lossless export and exact restore
//   lq_group.hpp        group-wise (block) scales, symmetric and with an offset: one traversal body per axis
//   lq_group_batch.hpp  group-wise tensors in one launch per pass
//   lq_scale_init.hpp   scales and offsets from the weights: absmax / LSQ / MSE / min-max on the group-wise unit shapes
//   lq_mx.hpp           OCP microscaling element formats: the group-wise traversal bodies with a minifloat element step
//   lq_mx_operand.hpp   packed MX operands in the block-scaled matrix instruction's fragment order: pack, dynamic quantize, decode
//   lq_mx_gemm.hpp      the GEMM of two packed operands on v_mfma_scale_f32_16x16x128_f8f6f4
//   lq_i8_operand.hpp   packed int8 operands with fp32 scales per line and scale block: pack, dynamic quantize, decode
//   lq_i8_gemm.hpp      the GEMM of two packed int8 operands on v_mfma_i32_16x16x64_i8
//   lq_i8_gemm_quant.hpp  the same product with an operand-out epilogue: it writes the next layer's int8 operand
//   lq_im2col.hpp       a convolution's im2col matrix without the matrix: geometry, a line's window, the predicated gather
//   lq_mx_conv.hpp      the MX operand of that matrix, gathered from the input in one launch
//   lq_i8_conv.hpp      the int8 operand of the same matrix: absmax scales per (line, scale block), two passes over the gather
//   this file           host side: traversal plan, launchers, the extern "C" entry points
//
// The path is elementwise + per-group reductions: HBM-bound, no MFMA.  Design rules
// (cdna_hip_programming.md G2/G11/G12/G13, MI355X_MICROARCH.md HBM), each settled by measurement on the
// device (tools/membench.hip, tools/bench_shapes.py):
//   * one 16-byte coalesced access per lane and stream (float4), nontemporal for tensors >= 64 MiB; blocks of
//     512 threads for streaming-size tensors; loads issued before the per-group context is computed;
//   * the per-group scale is block-uniform in the streaming kernels (one scalar load, SGPR broadcast) -- the
//     group index never costs per-element integer division (3-D grid / loop-invariant lane->column maps);
//   * reductions: DPP inside the 64-lane wave -> LDS across the block's waves -> one partial per block in a
//     caller-provided workspace -> a finalize kernel.  No float atomics: every sum is taken in a fixed
//     order, results are run-to-run bit-stable;
//   * max|q| is reduced on the uint32 bit pattern of |q| (order-independent, exact);
//   * the integers must match the reference bit for bit: IEEE-754 correctly rounded fp32 division followed
//     by floor (never a reciprocal multiply; the fast forms are proven/validated exact), -ffp-contract=off,
//     no fast-math.
//
// Reference semantics restated here (file:line relative to /root/reference):
//   forward           MNIST/nested_quantization_layer/custom_components/custom_layers.py:55-60
//   NQ backward       custom_layers.py:62-118
//   penalties         CIFAR-10/custom_loss_terms/custom_components/custom_loss_functions.py:75-116,161-195,240-275
//   constraint        custom_layers.py:35-46
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <algorithm>
#include <vector>

#include "lq_hip.h"

#include "lq_batch.hpp"
#include "lq_stream2.hpp"
#include "lq_pack.hpp"
#include "lq_group.hpp"
#include "lq_group_batch.hpp"
#include "lq_scale_init.hpp"
#include "lq_mx.hpp"
#include "lq_group_stats.hpp"
#include "lq_mx_stats.hpp"
#include "lq_mx_operand.hpp"
#include "lq_mx_gemm.hpp"
#include "lq_mx_conv.hpp"
#include "lq_i8_operand.hpp"
#include "lq_i8_gemm.hpp"
#include "lq_i8_conv.hpp"
#include "lq_i8_gemm_quant.hpp"

namespace lq {

// ------------------------------------------------------------------------------------------
//  Host side: plan, launchers, C ABI.
// ------------------------------------------------------------------------------------------
enum Mode { MODE_ROW_BIG = 0, MODE_ROW_SMALL = 1, MODE_COL = 2 };

// Rows per block of the pipelined column tile, by operation (MI355X sweep, profiles/r02/column_tile_rows_per_block.txt):
// the read-only scale-gradient traversal wants long blocks (128 rows: 5.7-5.9 TB/s; 32 rows: 4.5), the kernels that
// also store want short ones (48 rows: K4 5.6-5.8 TB/s; 128 rows: 5.3-5.5)
constexpr int64_t kColRbFused = 48;
constexpr int64_t kColRbBwd = 128;

// Where a traversal leaves its partial triples and how the finalize walks them (host only: FinGeom and Task carry copies).
struct PartialLayout {
    int64_t np;                             // partial triples the traversal writes
    int64_t gstride, n1, stride1, n2;       // finalize geometry: group g's partials at g * gstride + i1 * stride1 + i2
};

struct Plan {
    int mode;
    int64_t R, L;       // row modes
    int bs;             // threads per block in the streaming traversal (unit = bs*4 elements)
    int CH;
    int64_t nc;
    int lpr_log2;
    int64_t C, rps, ysplit;   // column mode
    int per4;           // column mode, C <= 64: geometry admits the float4 grid-stride variant (ysplit % C == 0)
    PartialLayout lay;  // the partials of the form the plan describes; a launch that runs another form replaces it
    int64_t np_bound;   // workspace bound: the largest partial count of any form the launch may choose (>= lay.np)
};

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The three layouts, and the only code that writes one (the batch's group fragments and the conv tile have one each further
// down: layout_frags, conv_tile_layout).  Partial p of group g, outer index o:
// one per (row, chunk): row o * G + g, chunk c at (o * G + g) * nc + c
static PartialLayout layout_row_chunks(int64_t R, int64_t nc, int64_t f_outer, int64_t G) { return {R * nc, nc, f_outer, G * nc, nc}; }
// one per row, stored group-major: g * f_outer + o
static PartialLayout layout_rows(int64_t R, int64_t f_outer) { return {R, f_outer, f_outer, 1, 1}; }
// one per (row block, column): block y, column g * inner + i at y * C + g * inner + i
static PartialLayout layout_cols(int64_t nby, int64_t C, int64_t inner) { return {nby * C, inner, nby, C, inner}; }
// a plan that carries nothing but a layout (the conv tile's: its launch has a geometry of its own, ConvTile)
static Plan plan_of_layout(const PartialLayout& lay) {
    Plan pl;
    memset(&pl, 0, sizeof(pl));
    pl.lay = lay;
    pl.np_bound = lay.np;
    return pl;
}

// Development knobs.  The shipped library reads NO environment variable: the traversal plan, the partial layout and with
// them the workspace size are pure functions of the descriptor and the pointers' alignment.  `make dev` (-DLQ_DEV_KNOBS,
// tools/ only) turns LQ_KNOB into a getenv lookup and compiles the alternative launches the tuning sweeps of profiles/r02
// were made with; every use is marked.
#ifdef LQ_DEV_KNOBS
static int knob_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
#define LQ_KNOB(var, name, dflt) static const int var = knob_env(name, dflt)
#else
#define LQ_KNOB(var, name, dflt) constexpr int var = (dflt)
#endif

#ifdef LQ_DEV_KNOBS
static int g_dev_flags_host = 0;       // the host's copy of lq_dev_set_flags(bits)
#endif
// First element of the tail of a streaming tensor that K1 and K2 load with the default cache policy whatever the mix word says
// (kMallKeepBytes: none in the shipped build; DESIGN.md section 3 "Infinity Cache reuse", "Cache-policy mix").  Development
// builds: LQ_TUNE_MALL_T or bits 0xf00 of lq_dev_set_flags hold 1 + the fraction of the tensor in tenths (1 = nothing kept), 0 =
// the shipped rule.
#ifdef LQ_DEV_KNOBS
// lq_dev_set_policy_mix(k1, k2): the mix words of K1 and K2 (mix_word, lq_common.hpp; 0xffffffff = the shipped constant).  Bits
// 24-27 of k1, when set, hold a tail fraction for K1 ALONE, coded like bits 0xf00 of lq_dev_set_flags (K2 keeps its own).
static uint32_t g_dev_mix_k1 = 0xffffffffu, g_dev_mix_k2 = 0xffffffffu;
#endif
static uint32_t mix_k1() {
#ifdef LQ_DEV_KNOBS
    if (g_dev_mix_k1 != 0xffffffffu) return g_dev_mix_k1 & 0x1fffffu;
#endif
    return kMixK1;
}
static uint32_t mix_k2() {
#ifdef LQ_DEV_KNOBS
    if (g_dev_mix_k2 != 0xffffffffu) return g_dev_mix_k2 & 0x1fffffu;
#endif
    return kMixK2;
}
static int64_t mall_keep_from(int64_t numel, bool k1 = false) {
    int64_t keep = kMallKeepBytes / 4;
    LQ_KNOB(t_env, "LQ_TUNE_MALL_T", 0);
    int t = t_env;
#ifdef LQ_DEV_KNOBS
    if (g_dev_flags_host & 0xf00) t = (g_dev_flags_host >> 8) & 15;
    if (k1 && g_dev_mix_k1 != 0xffffffffu && (g_dev_mix_k1 >> 24 & 15)) t = g_dev_mix_k1 >> 24 & 15;
#endif
    if (t > 0) keep = (int64_t)((double)numel * (t - 1) / 10.0);
    return keep >= numel ? 0 : numel - keep;
}

static bool flat_cols_ok(int64_t C) { return C == 8 || C == 16 || C == 32 || C == 64; }
static int64_t colx_max_inner() {        // rows shorter than this may run in column mode (see make_plan)
    LQ_KNOB(v, "LQ_TUNE_COLX_INNER", 200);
    return v;
}
static int64_t periodic_target() {      // block count of the periodic column form
    LQ_KNOB(v, "LQ_TUNE_PER_NB", 2048);
    return v > 0 ? v : 2048;
}
static int64_t periodic_blocks(int64_t C) { return C * ((periodic_target() + C / 2) / C); }      // ~2048 blocks, a multiple of C

// Chunks of CH elements per row of length L.  A tail of at most CH/8 elements is folded into the previous chunk (the
// traversal's last chunk takes whatever remains) instead of getting a block of its own.
static int64_t row_chunks(int64_t L, int64_t CH) {
    int64_t nc = ceil_div(L, CH);
    const int64_t r = L % CH;
    if (nc > 1 && r != 0 && r * 8 <= CH) nc -= 1;
    return nc;
}

static Plan make_plan(int64_t outer, int64_t G, int64_t inner, int force_bs = 0) {
    Plan pl;
    memset(&pl, 0, sizeof(pl));
    const int64_t N = outer * G * inner;
    int64_t R, L, f_outer;
    bool col = false;
    if (G == 1) {
        R = 1;
        L = N;
        f_outer = 1;
    } else {
        R = outer * G;
        L = inner;
        f_outer = outer;
        // Short rows that come in many layers (outer >= 32: per-channel scales of NCHW activations with small planes, e.g.
        // (256, 2048, 7 x 7)) are instruction-bound as rows -- per-row context, team reduction and emit every 100-400 bytes --
        // but as the matrix [outer][G * inner] a lane keeps its four columns, contexts and accumulators across all layers:
        // column mode for them too, at streaming size and when the matrix rows are whole 128-byte lines.
        LQ_KNOB(colx, "LQ_TUNE_COLX", 1);      // 0 = rows
        const bool short_rows_many_layers = colx && inner >= 16 && inner < colx_max_inner() && outer >= 32 && (G * inner) % 32 == 0 &&
                                            G * inner > 64 && (double)N >= (double)kPeriodic4Min && !(inner % 4 == 0 && (inner & (inner - 1)) == 0);
        if ((inner < 16 && outer > 1) || short_rows_many_layers) {
            // column mode unless thread-per-row yields fewer partials
            const int64_t C = G * inner;
            // rows per block: ~16 K elements per block for narrow matrices, 128 rows for wide ones
            int64_t RB;
            int64_t nby = 0;
            int per4 = 0;
            if (C <= 64 && (double)outer * (double)C >= (double)kPeriodic4Min) {
                per4 = 1;
                // streaming size: a block count that is a multiple of C (what the float4 grid-stride variant needs);
                // the scalar periodic variant runs on the same geometry (trailing blocks may own no rows)
                nby = periodic_blocks(C);
                const int64_t k = 64 / C;
                RB = ceil_div(ceil_div(outer, nby), 4 * k) * 4 * k;
            } else if (C <= 64) {
                // ~16 K elements per block, but at least ~1024 blocks' worth of parallelism for small matrices: a block whose
                // waves walk 1656 rows of 10 columns needs 17 dependent load rounds (12 us for 64 K elements)
                const int64_t k = 64 / C;
                RB = ceil_div(ceil_div(16384, C), 4 * k) * 4 * k;
                const int64_t rb_par = ceil_div(ceil_div(outer, 1024), 4 * k) * 4 * k;
                if (rb_par < RB) RB = rb_par;
            } else {
                // 128 rows per block for streaming sizes; small matrices get shorter row blocks (about 512 blocks in all) so
                // that a wave walks its rows in one or two dependent load rounds instead of eight (784 x 128 Dense, column-wise:
                // scale-gradient traversal 12.5 -> 5.9 us, forward 9.4 -> 4.3 us)
                RB = ceil_div(outer * ceil_div(C, 256), 512);
                RB = ceil_div(RB, 16) * 16;
                if (RB > 128) RB = 128;
                // streaming sizes with float4 columns: the round-2 pipelined tile (lq_stream2.hpp) picks its rows per block per
                // operation at launch (kColRbFused / kColRbBwd); the plan carries the smaller one, i.e. the larger partial
                // count, so the workspace bound holds for both
                // (C % 4 != 0: the same tile with dword-aligned float4 access, k_col_pipe<..., UA = 1>)
                if ((double)outer * (double)C >= (double)kPeriodic4Min) RB = kColRbFused;
                // short rows in many layers (see above): one partial per column and 128 layers keeps the partial count near the
                // row count (a partial per column and 48 layers would be 5-10 % of the traffic for rows of 100+ elements)
                // -- only when 48 layers per block would not fit the partial budget below (K4 prefers 48: 7 x 7 planes 5.4 against 5.2)
                if (short_rows_many_layers && ceil_div(outer, kColRbFused) * C > 2 * R) RB = kColRbBwd;
            }
            if (RB > outer) RB = outer;
            if (!nby) nby = ceil_div(outer, RB);
            if (nby * C <= R || (short_rows_many_layers && nby * C <= 2 * R)) {
                col = true;
                pl.mode = MODE_COL;
                pl.C = C;
                pl.rps = RB;
                pl.ysplit = nby;
                pl.per4 = per4;
                pl.lay = layout_cols(nby, C, inner);
                pl.np_bound = pl.lay.np;
                // the one-shot flat column kernel (lq_stream2.hpp k_flat_cols: C <= 4 or C = 8, 16, 32, 64 at streaming sizes)
                // writes one partial per (block of 1024 float4, column): size the workspace for it
                if (per4 && flat_cols_ok(C)) {
                    const int64_t fb = ceil_div(ceil_div(outer * C, 4) + 1, (int64_t)kFlatColsBlock * 2);
                    if (fb * C > pl.np_bound) pl.np_bound = fb * C;
                }
                // 64 < C <= 256 at streaming size may run the periodic form (a column tile narrower than 256 columns leaves
                // lanes idle): one partial per (block, column) for periodic_blocks(C) blocks
                if (C > 64 && C <= 256 && (double)outer * (double)C >= (double)kPeriodic4Min && periodic_blocks(C) * C > pl.np_bound)
                    pl.np_bound = periodic_blocks(C) * C;
            }
        }
    }
    if (!col) {
        pl.R = R;
        pl.L = L;
        if (L >= 1024) {
            pl.mode = MODE_ROW_BIG;
            // 512 threads: measured best on MI355X (BENCH bwd 44.9 us vs 53.6 us at 1024 -- fewer waves held at the
            // closing barrier -- and vs 48.4 us at 256; the forward is insensitive)
            // Below 4 M elements a tensor is latency-bound and keeps 256-thread units, the geometry the
            // multi-tensor batch kernels use -- so batched and single-tensor results are bit-identical there.
            pl.bs = (L >= 2048 && (double)R * (double)L >= 4194304.0) ? 512 : 256;
            if (force_bs) pl.bs = force_bs;
#ifdef LQ_DEV_KNOBS
            else {                                             // force the streaming block size
                LQ_KNOB(v, "LQ_TUNE_BS", 0);
                if ((v == 256 || v == 512 || v == 1024) && L >= v * 4) pl.bs = v;
            }
#endif
            pl.CH = pl.bs * 4;
            pl.nc = row_chunks(L, pl.CH);
        } else {
            pl.mode = MODE_ROW_SMALL;
            pl.CH = (int)L;
            pl.nc = 1;
            int lpr = 1, lg = 0;   // lanes per row = pow2floor(max(L/2, 1)) clipped to one wave
            const int64_t half = L / 2 > 1 ? L / 2 : 1;
            while (lpr * 2 <= half && lpr < 64) {
                lpr *= 2;
                ++lg;
            }
            pl.lpr_log2 = lg;
        }
        pl.lay = pl.mode == MODE_ROW_SMALL ? layout_rows(R, f_outer) : layout_row_chunks(R, pl.nc, f_outer, G);
        pl.np_bound = pl.lay.np;
        // launch_traverse may cut the rows of 512-thread units into 1024-element chunks
        if (pl.mode == MODE_ROW_BIG && pl.bs == 512 && R * row_chunks(L, 1024) > pl.np_bound) pl.np_bound = R * row_chunks(L, 1024);
    }
    return pl;
}

static thread_local char g_err[512] = "";
static thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;      // lq_profile_events

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int check_hip(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LQ_EHIP, "%s: %s", what, hipGetErrorString(e));
    return LQ_OK;
}

static bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// the optional integer view of a forward: q and q_dtype come together or not at all
static int check_q_view(const char* fn, const void* q, int q_dtype) {
    if (q_dtype < LQ_Q_NONE || q_dtype > LQ_Q_I8) return fail(LQ_EINVAL, "%s: bad q_dtype %d", fn, q_dtype);
    if ((q != nullptr) != (q_dtype != LQ_Q_NONE)) return fail(LQ_EINVAL, "%s: q and q_dtype disagree", fn);
    return LQ_OK;
}

static int check_desc(int64_t outer, int64_t G, int64_t inner) {
    if (outer <= 0 || G <= 0 || inner <= 0) return fail(LQ_EINVAL, "descriptor extents must be positive (outer=%lld G=%lld inner=%lld)", (long long)outer, (long long)G, (long long)inner);
    const double n = (double)outer * (double)G * (double)inner;
    if (n > 9.0e15) return fail(LQ_EINVAL, "tensor too large");
    return LQ_OK;
}

static size_t ws_partials(const Plan& pl) { return ((size_t)pl.np_bound + 63) / 64 * 64; }      // per accumulator array
static size_t ws_bytes_for(const Plan& pl) { return ws_partials(pl) * 16 + 256; }

static int bind_ws(Params& p, const Plan& pl, void* ws, size_t ws_bytes) {
    if (!ws) return fail(LQ_EWORKSPACE, "workspace is NULL (need %zu bytes)", ws_bytes_for(pl));
    if (!aligned(ws, 16)) return fail(LQ_EALIGN, "workspace must be 16-byte aligned");
    if (ws_bytes < ws_bytes_for(pl)) return fail(LQ_EWORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, ws_bytes_for(pl));
    const size_t np = ws_partials(pl);
    p.pa = reinterpret_cast<uint32_t*>(ws);
    p.pb = p.pa + np;
    p.pc = reinterpret_cast<double*>(p.pb + np);
    return LQ_OK;
}

// row-small: lanes per row.  Scalar form: pow2floor(max(L/2,1)) (plan); float4 form: pow2ceil(L/4), both <= 64.
static int row_small_lpr_log2_vec(int64_t L) {
    const int64_t l4 = L / 4;
    int lg = 0;
    while ((1 << lg) < l4 && lg < 6) ++lg;
    return lg;
}
static bool row_small_vec(const Plan& pl, const void* P, const void* dy, const void* out) {
    return pl.L % 4 == 0 && pl.L >= 8 && aligned(P, 16) && (!dy || aligned(dy, 16)) && (!out || aligned(out, 16));
}

// column-mode kernel variant and blocks along the columns: 0 = periodic (C <= 64), 4 = float4 tile, 1 = scalar tile
static void col_variant(const Plan& pl, const void* P, const void* dy, const void* out, int& variant, int64_t& nbx,
                        bool allow_periodic4 = true) {
    const bool al16 = aligned(P, 16) && (!dy || aligned(dy, 16)) && (!out || aligned(out, 16));
    const double bytes = (double)pl.C * (double)pl.ysplit * (double)pl.rps * 4.0;
    if (pl.C <= 64) {
        variant = (allow_periodic4 && pl.per4 && al16) ? (bytes >= (double)kNtBytes ? 7 : 6) : 0;
        nbx = 1;
    } else if (pl.C % 4 == 0 && al16) {
        variant = (bytes >= (double)kNtBytes) ? 5 : 4;
        nbx = ceil_div(pl.C, 256);
    } else {
        variant = 1;
        nbx = ceil_div(pl.C, 64);
    }
}

// development knobs of the streaming forms: LQ_TUNE_S2 = bit mask of forms to DISABLE (1 flat K1, 2 pipelined column tile,
// 4 pipelined periodic columns, 8 tiny-row passes, ...); LQ_TUNE_PIPE = U*10 + NW of the column tile; LQ_TUNE_TINY_U = passes

#ifdef LQ_DEV_KNOBS
constexpr bool kDevKnobs = true;       // tools/ builds: the LQ_TUNE_* switches can route a descriptor to any form
#else
constexpr bool kDevKnobs = false;
#endif

// The streaming geometry of long rows (512-thread units, nontemporal accesses, two float4 per thread) exists for K1, K2 and K4 --
// the operations that run on activation-sized tensors.  The penalty terms, the integer view and the element-wise OIHW
// companion work on weight-sized tensors: they keep the 256-thread units at every size (their entry points plan with
// make_plan(..., kBlock)), which is a third of the row-stream instantiations and none that a parity test could not reach.
template <int OP>
constexpr bool kStreamOp = OP == OP_FWD || OP == OP_BWD || OP == OP_FUSED;

template <int NT, int GM>
static void launch_flat_fwd_as(const Params& p, const FlatIdx& fx, int64_t nv, int rem, int64_t blocks, bool events, hipStream_t st) {
    // hipExtLaunchKernelGGL: with lq_profile_events() set, the events take the kernel's own begin / end timestamps
    if (events) hipExtLaunchKernelGGL((k_flat_fwd<OP_FWD, 512, NT, GM>), dim3((unsigned)blocks), dim3(512), 0, st, g_prof_start, g_prof_stop, 0, p, fx, nv, rem);
    else hipLaunchKernelGGL((k_flat_fwd<OP_FWD, 512, NT, GM>), dim3((unsigned)blocks), dim3(512), 0, st, p, fx, nv, rem);
}

// K1 as the flat one-shot stream (lq_stream2.hpp k_flat_fwd): the `n` elements as float4, 512 per block, and with `with_rem` a
// last block for the n % 4 elements that remain.  gm: the kernel's group mode; gm_wide: its 64-bit form for 2^32 or more
// elements (< 0: there is none and the caller keeps such tensors away; 2^32 elements are 16 GiB, so `wide` implies `nt`).
// events: the launch lq_profile_events() stamps.  Returns 1 when it launched, < 0 on error, 0 when the grid would be too large.
static int launch_flat_fwd(const Params& p, const FlatIdx& fx, int64_t n, int gm, int gm_wide, bool with_rem, bool nt, bool events,
                           hipStream_t st) {
    const int64_t nv = n >> 2;
    const int rem = with_rem ? (int)(n & 3) : 0;
    const int64_t blocks = ceil_div(nv + (rem ? 1 : 0), 512);
    if (blocks > 2147483647ll) return 0;
    const bool wide = nt && gm_wide >= 0 && n >= 4294967296ll;
    switch ((wide ? gm_wide : gm) * 2 + (nt ? 1 : 0)) {      // every (NT, GM) pair that is compiled
        case 0 * 2 + 0: launch_flat_fwd_as<0, 0>(p, fx, nv, rem, blocks, events, st); break;
        case 0 * 2 + 1: launch_flat_fwd_as<1, 0>(p, fx, nv, rem, blocks, events, st); break;
        case 2 * 2 + 1: launch_flat_fwd_as<1, 2>(p, fx, nv, rem, blocks, events, st); break;
        case 4 * 2 + 0: launch_flat_fwd_as<0, 4>(p, fx, nv, rem, blocks, events, st); break;
        case 4 * 2 + 1: launch_flat_fwd_as<1, 4>(p, fx, nv, rem, blocks, events, st); break;
        case 5 * 2 + 1: launch_flat_fwd_as<1, 5>(p, fx, nv, rem, blocks, events, st); break;
        case 6 * 2 + 0: launch_flat_fwd_as<0, 6>(p, fx, nv, rem, blocks, events, st); break;
        case 6 * 2 + 1: launch_flat_fwd_as<1, 6>(p, fx, nv, rem, blocks, events, st); break;
        case 7 * 2 + 1: launch_flat_fwd_as<1, 7>(p, fx, nv, rem, blocks, events, st); break;
        case 8 * 2 + 0: launch_flat_fwd_as<0, 8>(p, fx, nv, rem, blocks, events, st); break;
        case 8 * 2 + 1: launch_flat_fwd_as<1, 8>(p, fx, nv, rem, blocks, events, st); break;
        case 9 * 2 + 1: launch_flat_fwd_as<1, 9>(p, fx, nv, rem, blocks, events, st); break;
        case 10 * 2 + 0: launch_flat_fwd_as<0, 10>(p, fx, nv, rem, blocks, events, st); break;
        case 10 * 2 + 1: launch_flat_fwd_as<1, 10>(p, fx, nv, rem, blocks, events, st); break;
        case 11 * 2 + 0: launch_flat_fwd_as<0, 11>(p, fx, nv, rem, blocks, events, st); break;
        case 11 * 2 + 1: launch_flat_fwd_as<1, 11>(p, fx, nv, rem, blocks, events, st); break;
        default: fail(LQ_EINVAL, "internal: flat forward has no group mode %d (nt %d)", wide ? gm_wide : gm, (int)nt); return -1;
    }
    return check_hip("flat forward launch") ? -1 : 1;
}

// Streaming-size (>= 4 M elements) forms of lq_stream2.hpp.  Returns 1 when it launched the traversal, 0 when the
// round-1 traversal should run, < 0 on error.
template <int OP>
static int launch_stream2(Plan& pl, const Params& p, hipStream_t st) {
    if constexpr (!kStreamOp<OP>) {
        return 0;
    } else {
    using O = OpT<OP>;
    const double numel = (double)p.outer * (double)p.G * (double)p.inner;
    if (numel < (double)kPeriodic4Min) return 0;
    if (p.out_perm || p.dy_perm) return 0;
    FlatIdx fx;              // 32-bit forms only (numel < 2^32); the wide forms divide in 64 bits
    fx.inner = make_fastdiv((uint32_t)(p.inner < 4294967296ll ? p.inner : 1));
    fx.G = make_fastdiv((uint32_t)(p.G < 4294967296ll ? p.G : 1));
    fx.keep_from = 0xffffffffu;      // no block keeps its lines (set below for the streaming forward of long aligned rows)
    fx.keep_mix = 0;
    (void)fx;
    if (pl.mode == MODE_ROW_BIG) {
        // long rows off the 16-byte grid: K1 as a line-aligned flat stream (lq_stream2.hpp k_flat_fwd, group mode 6 / 7)
        if constexpr (OP == OP_FWD) {
            LQ_KNOB(off_rb, "LQ_TUNE_S2", 0);
            const int64_t nn = p.outer * p.G * p.inner;
            // K1 of long rows as the flat one-shot stream too: one group per float4 when L % 4 == 0 (group mode 0 / 2) -- rows that
            // are not whole 128-byte lines (4100: 5.4 -> 6.3 TB/s), rows that fill their chunks poorly (1600 = 1024 + 576: 5.65 ->
            // 6.3) and, by 2 %, the well-filled aligned rows as well (BENCH tensor, K1 alone on four buffer sets, three interleaved
            // runs: 48.6-48.9 us against 49.8-49.9 for the row stream; profiles/r02/bench_k1_row_stream_vs_flat.txt; development
            // knob 32768 restores the row stream for them).  L % 4 != 0: a float4 may straddle a row end (6 / 7), see below.
            const bool poor_fill = (double)pl.L / (double)(pl.nc * pl.CH) < 0.95;
            if (!(off_rb & 256) && (pl.L % 32 != 0 || poor_fill || !(off_rb & 32768)) && aligned(p.P, 16) && aligned(p.out, 16)) {
                const bool ntb = numel * 4.0 >= (double)kNtBytes;
                int r;
                if (pl.L % 4 == 0) {
                    if (ntb) {
                        fx.keep_from = (uint32_t)ceil_div(mall_keep_from(nn, true), 2048);      // 512 float4 per block
                        fx.keep_mix = mix_k1();
                    }
                    r = launch_flat_fwd(p, fx, nn, 0, 2, true, ntb, true, st);
                } else if (!(off_rb & 512) && (double)pl.L / (double)(pl.nc * pl.CH) >= 0.8) {
                    // long rows with L % 4 != 0 keep the row stream (TAIL instantiation): K1 5.8-6.0 TB/s on rows of 1025,
                    // 2047, 4099, 50177 against 5.4-5.9 for the straddling flat form (development knob 512 selects the latter)
                    // -- unless their chunks are poorly filled (rows of 1225 = 1024 + 201 elements: 4.3 TB/s)
                    return 0;
                } else {
                    r = launch_flat_fwd(p, fx, nn, 6, 7, true, ntb, true, st);
                }
                if (r) return r;
            }
        } else {
            // Rows of 1153..1533 elements are two 1024-chunks, the second one 13-50 % full (35 x 35 planes: 1225 = 1024 + 201) --
            // too few bytes in flight per resident thread: K2 / K4 4.0 / 3.9 TB/s.  One wave per row through the row-window
            // kernel instead (5 or 6 float4 per lane: 80-100 % of the lanes carry data); partials as in the row-small mode.
            LQ_KNOB(off_rb, "LQ_TUNE_S2", 0);
            const int nwin = (int)(pl.L % 4 ? (pl.L + 6) / 4 : pl.L / 4);
            const bool al = aligned(p.P, 16) && aligned(p.dy, 16) && (!O::kStore || aligned(p.out, 16));
            // (rows of 1534..2047 elements: two chunks that fill >= 75 % -- the row stream is as good or better (1800: K2 / K4 6.4 / 5.8
            // against 6.0 / 5.5 with 8 float4 per lane) unless the rows are off the 16-byte grid (1535, 1537: 5.0 / 4.7 -> 6.1 / 5.6))
            LQ_KNOB(win_max, "LQ_TUNE_WIN_MAX", 384);      // development knob: widest window (float4) for rows ON the grid
            const bool wide_ok = pl.L % 4 != 0 && (double)pl.L / 2048.0 < 0.95;
            if (!(off_rb & 128) && pl.bs == 256 && pl.nc == 2 && (nwin <= win_max || wide_ok) && nwin <= 512 && al && !p.direct && pl.R < 4294967296ll) {
                const int64_t blocks = ceil_div(pl.R, (int64_t)kWavesPerBlock);
                if (blocks <= 2147483647ll) {
                    const int64_t n = p.outer * p.G * p.inner;
                    const bool ntb = numel * 4.0 >= (double)kNtBytes;
                    const FastDiv fG = make_fastdiv((uint32_t)p.G);
                    pl.nc = 1;                 // the finalize that follows must walk the partial layout this launch produces:
                    pl.lay = layout_rows(pl.R, pl.R / p.G);      // one partial per row, as in the row-small mode
#define LQ_WINB(NT_, V_) hipLaunchKernelGGL((k_row_win<OP, NT_, 6, V_, 1>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, fG, pl.R, (int)pl.L, n)
                    if (nwin <= 320) { if (ntb) LQ_WINB(1, 5); else LQ_WINB(0, 5); }
                    else if (nwin <= 384) { if (ntb) LQ_WINB(1, 6); else LQ_WINB(0, 6); }
                    else if (nwin <= 448) { if (ntb) LQ_WINB(1, 7); else LQ_WINB(0, 7); }
                    else { if (ntb) LQ_WINB(1, 8); else LQ_WINB(0, 8); }
#undef LQ_WINB
                    return check_hip("row-window launch") ? -1 : 1;
                }
            }
        }
        return 0;
    }
    const bool al16 = aligned(p.P, 16) && (!O::kDy || aligned(p.dy, 16)) && (!O::kStore || aligned(p.out, 16));
    if (!al16) return 0;
    LQ_KNOB(off, "LQ_TUNE_S2", 0);
    const bool nt = numel * 4.0 >= (double)kNtBytes;
    const int64_t n = p.outer * p.G * p.inner;
    // ---- K1 as a flat stream: whenever a float4 has one group (inner % 4 == 0) -- tiny rows, rows of 8..1020 elements,
    // column matrices with inner = 4, 8, 12
    if constexpr (OP == OP_FWD) {
        const bool one_group = p.inner % 4 == 0;                                             // a float4 never straddles groups
        const bool scale4 = p.inner == 1 && p.G % 4 == 0 && aligned(p.s, 16) && !(off & 32);   // its 4 scales are one float4
        const bool scale4u = p.inner == 1 && p.G % 4 != 0 && p.G > 64 && !(off & 8192);       // the same, dword-aligned, may wrap
        const bool cols_pow2 = pl.mode == MODE_COL && pl.per4 && flat_cols_ok(pl.C) && !(off & 64);   // k_flat_cols below: 1-2 % faster
        // rows of 4..1023 elements off the 16-byte grid (row-small mode, L % 4 != 0): a float4 straddles at most one row end
        const bool straddle = pl.mode == MODE_ROW_SMALL && pl.L >= 4 && pl.L % 4 != 0 && !(off & 256);
        if (straddle) {
            if (const int r = launch_flat_fwd(p, fx, n, 6, 7, true, nt, false, st)) return r;
        }
        if (scale4u && !(off & 1)) {
            if (const int r = launch_flat_fwd(p, fx, n, 8, 9, true, nt, false, st)) return r;
        }
        // every other column-mode forward (several groups inside a float4: C = 3, 5, 10, 30; inner = 2, 3, 5, 15): gathered scales
        LQ_KNOB(gather_on, "LQ_TUNE_GATHER", 1);
        if (gather_on && !(off & 1) && pl.mode == MODE_COL && !one_group && !scale4 && !scale4u && !cols_pow2 && n < 4294967296ll) {
            if (const int r = launch_flat_fwd(p, fx, n, p.inner == 1 ? 10 : 11, -1, true, nt, false, st)) return r;
        }
        if (!(off & 1) && (one_group || scale4) && !cols_pow2) {      // n % 4 == 0: no remainder block
            if (const int r = launch_flat_fwd(p, fx, n, one_group ? 0 : 4, one_group ? 2 : 5, false, nt, false, st)) return r;
        }
    }
    if (pl.mode == MODE_COL) {
        // K1 reaches this point only with 2^32 or more elements (every smaller column-mode forward is one of the flat forms
        // above): the round-1 column kernel serves it -- no pipelined column instantiation exists for the forward
        if constexpr (OP == OP_FWD) {
            return 0;
        } else {
        constexpr int kUp = 2;                                 // float4 per stream in flight (two streams)
        // K2 of C = 8, 16, 32, 64 as a one-shot stream with FOUR float4 per thread and stream: with two, nothing hid the shuffle
        // tree and the barrier at the end of so short a wave (4.3-5.4 TB/s); with four the epilogue is paid once per 8 KB of each
        // stream: 6.0-6.2 TB/s against 5.5-5.6 for the periodic form.  (K4 with four: 5.6-5.9 against 5.7-6.1 with two.)
        if constexpr (OP == OP_BWD) {
            LQ_KNOB(fc_k2, "LQ_TUNE_FC_K2", 4);      // development knob: 0 = the periodic form
            if (fc_k2 == 4 && pl.C <= 64 && pl.per4 && flat_cols_ok(pl.C) && nt && !(off & 64)) {
                const int64_t nv = n >> 2;
                const int64_t fb = ceil_div(nv, (int64_t)kFlatColsBlock * 4);
                if (fb <= 2147483647ll && fb * pl.C <= pl.np_bound) {
                    pl.ysplit = fb;           // the finalize that follows must walk the partial layout this launch produces
                    pl.lay = layout_cols(fb, pl.C, p.inner);
                    hipLaunchKernelGGL((k_flat_cols<OP, 1, 4>), dim3((unsigned)fb), dim3(kFlatColsBlock), 0, st, p, (int)pl.C, nv);
                    return check_hip("flat column launch") ? -1 : 1;
                }
            }
        }
        if constexpr (OP != OP_BWD) if (pl.C <= 64 && pl.per4 && flat_cols_ok(pl.C) && !(off & 64)) {
            // C = 8, 16, 32, 64 as a flat one-shot stream: K1 and K4 (the read-only K2 is faster in the periodic form)
            const int64_t nv = n >> 2;                        // numel = outer * C is a multiple of 8
            constexpr int kU = 2;
            const int64_t fb = ceil_div(nv, (int64_t)kFlatColsBlock * kU);
            if (fb <= 2147483647ll && (OP == OP_FWD || fb * pl.C <= pl.np_bound)) {
                if (OP != OP_FWD) {
                    pl.ysplit = fb;           // the finalize that follows must walk the partial layout this launch produces
                    pl.lay = layout_cols(fb, pl.C, p.inner);
                }
                if (nt) hipLaunchKernelGGL((k_flat_cols<OP, 1, kU>), dim3((unsigned)fb), dim3(kFlatColsBlock), 0, st, p, (int)pl.C, nv);
                else hipLaunchKernelGGL((k_flat_cols<OP, 0, kU>), dim3((unsigned)fb), dim3(kFlatColsBlock), 0, st, p, (int)pl.C, nv);
                return check_hip("flat column launch") ? -1 : 1;
            }
        }
        if (pl.C <= 64) {
            if ((off & 4) || !pl.per4) return 0;
#ifdef LQ_DEV_KNOBS
            LQ_KNOB(per, "LQ_TUNE_PERIODIC", 0);      // U*10 + (block size / 256)
            if (nt && (per == 12 || per == 22)) {
                // 512-thread blocks, half as many: the finalize that follows must walk the partial layout this launch produces
                const int64_t nb2 = ((pl.ysplit / 2) / pl.C) * pl.C;
                if (nb2 >= pl.C) {
                    pl.ysplit = nb2;
                    pl.lay = layout_cols(nb2, pl.C, p.inner);
                    if (per == 12) hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 1, 512>), dim3((unsigned)nb2), dim3(512), 0, st, p, (int)pl.C, nb2);
                    else hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 2, 512>), dim3((unsigned)nb2), dim3(512), 0, st, p, (int)pl.C, nb2);
                    return check_hip("periodic column launch") ? -1 : 1;
                }
            }
            if (nt && (per == 11 || per == 21 || per == 41)) {
                if (per == 11) hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 1, 256>), dim3((unsigned)pl.ysplit), dim3(256), 0, st, p, (int)pl.C, pl.ysplit);
                else if (per == 21) hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 2, 256>), dim3((unsigned)pl.ysplit), dim3(256), 0, st, p, (int)pl.C, pl.ysplit);
                else hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 4, 256>), dim3((unsigned)pl.ysplit), dim3(256), 0, st, p, (int)pl.C, pl.ysplit);
                return check_hip("periodic column launch") ? -1 : 1;
            }
#endif
            // K4 with C >= 16: one float4 per stream in flight (98 VGPRs, 5 waves per SIMD) measured 5.67-5.75 TB/s at C = 64 against
            // 5.30-5.49 with two (128 VGPRs); at C = 3 the other way round (5.57 against 5.24)
            if constexpr (OP == OP_FUSED) {
                if (nt && pl.C >= 16) {
                    hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 1>), dim3((unsigned)pl.ysplit), dim3(kBlock), 0, st, p, (int)pl.C, pl.ysplit);
                    return check_hip("periodic column launch") ? -1 : 1;
                }
            }
            if (nt) hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, kUp>), dim3((unsigned)pl.ysplit), dim3(kBlock), 0, st, p, (int)pl.C, pl.ysplit);
            else hipLaunchKernelGGL((k_col_periodic_pipe<OP, 0, kUp>), dim3((unsigned)pl.ysplit), dim3(kBlock), 0, st, p, (int)pl.C, pl.ysplit);
            return check_hip("periodic column launch") ? -1 : 1;
        }
        LQ_KNOB(per_cmax, "LQ_TUNE_PER_CMAX", 256);      // development knob: 0 = always the tile
        if (pl.C <= per_cmax && pl.C <= 256 && (pl.C < 192 || pl.C % 32 != 0) && periodic_blocks(pl.C) * pl.C <= pl.np_bound) {
            // 64 < C <= 256: a tile narrower than 256 columns leaves lanes idle and, when C % 32 != 0, starts every row in the
            // middle of a 128-byte line; the periodic form is a flat line-aligned stream for any C.  Measured (K2 / K4 TB/s,
            // tile -> periodic): C = 68: 3.2 / 2.9 -> 5.6 / 5.7; 100: 4.3 / 4.0 -> 5.7 / 5.6; 130: 5.0 / 4.3 -> 5.4 / 5.1;
            // 99 (inner 3): 3.9 / 3.6 -> 5.5 / 5.0; 200, 250: +-3 %; 192 (3 full lines per row): 5.5 / 5.6 -> 5.1 / 5.1, keeps the tile
            const int64_t nb = periodic_blocks(pl.C);
            pl.ysplit = nb;               // the finalize that follows must walk the partial layout this launch produces
            pl.lay = layout_cols(nb, pl.C, p.inner);
            if constexpr (OP == OP_FUSED) {
                if (nt) hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 1>), dim3((unsigned)nb), dim3(kBlock), 0, st, p, (int)pl.C, nb);
                else hipLaunchKernelGGL((k_col_periodic_pipe<OP, 0, kUp>), dim3((unsigned)nb), dim3(kBlock), 0, st, p, (int)pl.C, nb);
            } else {
                if (nt) hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, kUp>), dim3((unsigned)nb), dim3(kBlock), 0, st, p, (int)pl.C, nb);
                else hipLaunchKernelGGL((k_col_periodic_pipe<OP, 0, kUp>), dim3((unsigned)nb), dim3(kBlock), 0, st, p, (int)pl.C, nb);
            }
            return check_hip("periodic column launch") ? -1 : 1;
        }
        // 256 < C <= 512 whose second column block is mostly empty (C = 320: 16 of 64 lanes in half the blocks, K2 / K4 4.7 / 4.5 TB/s)
        // or whose rows start inside a 128-byte line: the periodic form with 512-thread blocks (its LDS combine needs C <= block
        // size): C = 300: 4.2 / 4.0 -> 5.5 / 5.4; 320: -> 5.6 / 5.5; 450: 4.8 / 4.5 -> 5.4 / 5.4; 500: 5.3 / 4.9 -> 5.5 / 5.6
        if (nt && pl.C > 256 && pl.C <= 512 && pl.C <= per_cmax * 2 && ((double)pl.C / 512.0 < 0.8 || pl.C % 32 != 0)) {
            const int64_t nb = pl.C * ((1024 + pl.C / 2) / pl.C);          // ~1024 blocks of 512 threads, a multiple of C
            if (nb * pl.C <= pl.np_bound) {
                pl.ysplit = nb;               // the finalize that follows must walk the partial layout this launch produces
                pl.lay = layout_cols(nb, pl.C, p.inner);
                if constexpr (OP == OP_FUSED) hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 1, 512>), dim3((unsigned)nb), dim3(512), 0, st, p, (int)pl.C, nb);
                else hipLaunchKernelGGL((k_col_periodic_pipe<OP, 1, 2, 512>), dim3((unsigned)nb), dim3(512), 0, st, p, (int)pl.C, nb);
                return check_hip("periodic column launch") ? -1 : 1;
            }
        }
        const bool ua = pl.C % 4 != 0;
        if ((off & 2) || (ua && (off & 2048))) return 0;
        const int64_t nbx = ceil_div(pl.C, 256);
        {
            // rows per block by operation; never fewer than the plan's (the workspace was sized for the plan's partial count)
            LQ_KNOB(rb_bwd, "LQ_TUNE_COL_RB_K2", (int)kColRbBwd);
            LQ_KNOB(rb_st, "LQ_TUNE_COL_RB_K4", (int)kColRbFused);
            int64_t rb = (OP == OP_BWD) ? rb_bwd : rb_st;
            if (rb < pl.rps) rb = pl.rps;
            if (rb > p.outer) rb = p.outer;
            const int64_t nby = ceil_div(p.outer, rb);
            pl.rps = rb;                      // the finalize that follows must walk the partial layout this launch produces
            pl.ysplit = nby;
            pl.lay = layout_cols(nby, pl.C, p.inner);
        }
        const int64_t blocks = nbx * pl.ysplit;
        if (blocks > 2147483647ll) return 0;
        LQ_KNOB(pipe_r, "LQ_TUNE_PIPE", 28);      // U*10 + NW (scale-gradient ops)
        const int pipe = pipe_r;
#define LQ_PIPE(NT_, U_, NW_) hipLaunchKernelGGL((k_col_pipe<OP, NT_, U_, NW_>), dim3((unsigned)blocks), dim3(NW_ * 64), 0, st, p, pl.C, pl.rps, nbx)
        LQ_KNOB(xcd_remap, "LQ_TUNE_XCD", 1);      // development knob: 0 = natural block order for C % 32 != 0
        if (ua) {
            if (nt) hipLaunchKernelGGL((k_col_pipe<OP, 1, 2, 8, 1>), dim3((unsigned)blocks), dim3(512), 0, st, p, pl.C, pl.rps, nbx);
            else hipLaunchKernelGGL((k_col_pipe<OP, 0, 2, 8, 1>), dim3((unsigned)blocks), dim3(512), 0, st, p, pl.C, pl.rps, nbx);
        } else if (OP == OP_BWD && nt && pl.C % 32 != 0 && nbx > 1 && xcd_remap && pipe == 28) {
            // rows that are not whole lines: neighbouring column blocks share a line -- keep them on one XCD (lq_stream2.hpp)
            if constexpr (OP == OP_BWD) hipLaunchKernelGGL((k_col_pipe<OP, 1, 2, 8, 2>), dim3((unsigned)blocks), dim3(512), 0, st, p, pl.C, pl.rps, nbx);
        } else if (nt) {
#ifdef LQ_DEV_KNOBS
            if (pipe == 14) LQ_PIPE(1, 1, 4); else if (pipe == 44) LQ_PIPE(1, 4, 4); else if (pipe == 18) LQ_PIPE(1, 1, 8);
            else if (pipe == 48) LQ_PIPE(1, 4, 8); else if (pipe == 24) LQ_PIPE(1, 2, 4); else
#endif
            LQ_PIPE(1, 2, 8);
        } else {
            LQ_PIPE(0, 2, 8);
        }
#undef LQ_PIPE
        return check_hip("pipelined column launch") ? -1 : 1;
        }      // OP != OP_FWD
    }
    if constexpr (OP == OP_FWD) {
        return 0;                                      // a forward none of the flat forms above took (e.g. 2^32 or more elements in column mode)
    } else {
        // MODE_ROW_SMALL, scale-gradient ops.  Rows off the 16-byte grid (or, development knob 1024, any row of 68..1020
        // elements): aligned float4 windows (lq_stream2.hpp k_row_win)
        // short rows off the 16-byte grid: one flat window per block (lq_stream2.hpp k_row_seg)
        // -- when the team-per-row form below would leave too many lanes idle (widest window of a row / team size): measured
        // K2 / K4 TB/s, team -> block: L = 63 (17 of 32 lanes): 3.6 / 3.8 -> 4.2 / 4.9; 30: 3.5 / 3.9 -> 4.2 / 4.8; 17: 3.9 / 3.9 ->
        // 4.1 / 4.7; 49 (13 of 16): 4.8 / 4.6 -> 3.5 / 4.3 (keeps the team); 9 with outer = 4: 3.0 / 3.2 -> 2.8 / 3.5
        bool seg = false;
        if (pl.L >= 5 && pl.L <= 64 && pl.L % 4 != 0) {
            const int nw = (int)(pl.L + 6) / 4;
            int tl = 1;
            while ((1 << tl) < nw) ++tl;
            const double eff = (double)nw / (double)(1 << tl);
            seg = eff < (OP == OP_FUSED ? 0.8 : 0.7);
        }
        if (!(off & 16384) && seg && pl.R < 4294967296ll) {
            constexpr int kSegU = 2;
            const int rpb = (kBlock * kSegU * 4 - 3) / (int)pl.L;
            const int64_t blocks = ceil_div(pl.R, (int64_t)rpb);
            if (blocks <= 2147483647ll) {
                const FastDiv fL = make_fastdiv((uint32_t)pl.L), fG = make_fastdiv((uint32_t)p.G);
                if (nt) hipLaunchKernelGGL((k_row_seg<OP, 1, kSegU>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, fL, fG, pl.R, (int)pl.L, rpb, n);
                else hipLaunchKernelGGL((k_row_seg<OP, 0, kSegU>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, fL, fG, pl.R, (int)pl.L, rpb, n);
                return check_hip("row-segment launch") ? -1 : 1;
            }
        }
        LQ_KNOB(win_all, "LQ_TUNE_WIN", 1);      // 0: rows with L % 4 == 0 and L > 64 keep the round-1 row-small kernel
        if (!(off & 128) && pl.L >= 5 && pl.R < 4294967296ll && (pl.L % 4 != 0 || (win_all && pl.L > 64))) {
            const int nwin = (int)(pl.L % 4 ? (pl.L + 3 + 3) / 4 : pl.L / 4);     // float4s of the widest window of a row
            int lg = 1;
            while ((1 << lg) < nwin && lg < 6) ++lg;
            int V = lg == 6 ? (nwin + 63) / 64 : 1;
            // Round 3: rows of 65..340 elements.  The smallest power-of-two team with one float4 per lane leaves half the lanes
            // idle just above a power of two (rows of 68: 17 of 32 lanes) -- and, what costs more, pays the per-row work (context,
            // team reduction, emit) once per 32 or 64 lanes.  Teams of 16 / 32 lanes with 2-3 float4 per lane put two to four times
            // as many rows into a wave at 256- / 512-byte pieces per team and load.  Measured on 33.5 M elements, outer == 1
            // (tools/r03_win_geom.sh, profiles/r03/short_rows/): K2 rows of 68: 4.0 -> 5.0 TB/s, 88: 5.0 -> 6.0, 131: 3.7 -> 5.7,
            // 160: 4.9 -> 6.3, 260: 5.4 -> 6.1; K4 keeps the wider team where its stores want it (rows of 84..124 unless they are
            // whole 64-byte multiples): 68: 4.5 -> 4.9, 132: 4.5 -> 5.0, 160: 5.2 -> 6.0, 200: 5.5 -> 5.8.  (Teams of 8 lanes --
            // 128-byte pieces -- and two rows per team next to several float4 per lane both measured worse.)
            if constexpr (OP == OP_BWD) {
                if (nwin >= 17 && nwin <= 32) { lg = 4; V = 2; }
                else if (nwin >= 33 && nwin <= 48) { lg = 4; V = 3; }
                else if (nwin >= 49 && nwin <= 55) { lg = 5; V = 2; }
                else if (nwin >= 65 && nwin <= 84) { lg = 5; V = 3; }
            } else {
                if (nwin >= 17 && nwin <= 32 && (nwin <= 19 || pl.L % 16 == 0)) { lg = 4; V = 2; }
                else if (nwin >= 33 && nwin <= 64) { lg = 5; V = 2; }
            }
            const int U = V == 1 ? 2 : 1;
            const int64_t rows_per_block = (int64_t)kWavesPerBlock * (64 >> lg) * U;
            const int64_t blocks = ceil_div(pl.R, rows_per_block);
            if (blocks <= 2147483647ll && V <= 5) {
                const FastDiv fG = make_fastdiv((uint32_t)p.G);
#define LQ_WIN(NT_, LG_, V_, U_) hipLaunchKernelGGL((k_row_win<OP, NT_, LG_, V_, U_>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, fG, pl.R, (int)pl.L, n)
                // (only the combinations the rules above can produce are compiled: K2 never runs 32 lanes x 1, K4 never 64 x 1)
#define LQ_WIN2(NT_) do { \
                switch (lg * 8 + V) { \
                    case 1 * 8 + 1: LQ_WIN(NT_, 1, 1, 2); break; \
                    case 2 * 8 + 1: LQ_WIN(NT_, 2, 1, 2); break; \
                    case 3 * 8 + 1: LQ_WIN(NT_, 3, 1, 2); break; \
                    case 4 * 8 + 1: LQ_WIN(NT_, 4, 1, 2); break; \
                    case 4 * 8 + 2: LQ_WIN(NT_, 4, 2, 1); break; \
                    case 4 * 8 + 3: if constexpr (OP == OP_BWD || kDevKnobs) LQ_WIN(NT_, 4, 3, 1); break; \
                    case 5 * 8 + 1: if constexpr (OP != OP_BWD || kDevKnobs) LQ_WIN(NT_, 5, 1, 2); break; \
                    case 5 * 8 + 2: LQ_WIN(NT_, 5, 2, 1); break; \
                    case 5 * 8 + 3: if constexpr (OP == OP_BWD || kDevKnobs) LQ_WIN(NT_, 5, 3, 1); break; \
                    case 6 * 8 + 1: if constexpr (OP == OP_BWD || kDevKnobs) LQ_WIN(NT_, 6, 1, 2); break; \
                    case 6 * 8 + 2: LQ_WIN(NT_, 6, 2, 1); break; \
                    case 6 * 8 + 3: LQ_WIN(NT_, 6, 3, 1); break; \
                    case 6 * 8 + 4: LQ_WIN(NT_, 6, 4, 1); break; \
                    default: LQ_WIN(NT_, 6, 5, 1); break; \
                } } while (0)
#ifdef LQ_DEV_KNOBS
                // development: LQ_TUNE_WIN_GEOM = LG * 100 + V * 10 + U forces the team geometry (teams of 2^LG lanes, V float4 per lane,
                // U rows per team and wave)
                LQ_KNOB(geom, "LQ_TUNE_WIN_GEOM", 0);
                if (geom >= 100 && nt && ((geom / 10) % 10) * (1 << (geom / 100)) >= nwin) {
                    const int glg = geom / 100, gu = geom % 10;
                    const int64_t gblocks = ceil_div(pl.R, (int64_t)kWavesPerBlock * (64 >> glg) * gu);
                    bool done = true;
#define LQ_WING(LG_, V_, U_) hipLaunchKernelGGL((k_row_win<OP, 1, LG_, V_, U_>), dim3((unsigned)gblocks), dim3(kBlock), 0, st, p, fG, pl.R, (int)pl.L, n)
                    switch (geom) {
                        case 421: LQ_WING(4, 2, 1); break;
                        case 422: LQ_WING(4, 2, 2); break;
                        case 431: LQ_WING(4, 3, 1); break;
                        case 432: LQ_WING(4, 3, 2); break;
                        case 521: LQ_WING(5, 2, 1); break;
                        case 522: LQ_WING(5, 2, 2); break;
                        case 531: LQ_WING(5, 3, 1); break;
                        case 532: LQ_WING(5, 3, 2); break;
                        case 541: LQ_WING(5, 4, 1); break;
                        case 414: LQ_WING(4, 1, 4); break;
                        case 514: LQ_WING(5, 1, 4); break;
                        default: done = false;
                    }
#undef LQ_WING
                    if (done) return check_hip("row-window launch") ? -1 : 1;
                }
#endif
                if (nt) LQ_WIN2(1); else LQ_WIN2(0);
#undef LQ_WIN2
#undef LQ_WIN
                return check_hip("row-window launch") ? -1 : 1;
            }
        }
        if ((off & 8) || pl.L > 64 || pl.L < 8 || pl.L % 4 != 0) return 0;
        const int lg = row_small_lpr_log2_vec(pl.L);         // 1..4
        LQ_KNOB(tiny_u, "LQ_TUNE_TINY_U", 2);
        int U = (1 << lg) < tiny_u ? (1 << lg) : tiny_u;
        if (U != 2 && U != 4) U = 2;
        const int64_t rows_per_block = (int64_t)kWavesPerBlock * (64 >> lg) * U;
        const int64_t blocks = ceil_div(pl.R, rows_per_block);
        if (blocks > 2147483647ll) return 0;
        // (2^32 or more rows -- 128 GiB per stream at 8 elements a row -- keep the round-1 kernel: a 64-bit row modulo form of
        // this kernel could not be exercised by any test)
        if (pl.R >= 4294967296ll) return 0;
        const int gm = (p.outer == 1) ? 0 : 1;
#define LQ_TINY3(NT_, U_, LG_) do { \
            if (gm == 0) hipLaunchKernelGGL((k_row_tiny<OP, NT_, U_, LG_, 0>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, pl.R, (int)pl.L); \
            else hipLaunchKernelGGL((k_row_tiny<OP, NT_, U_, LG_, 1>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, pl.R, (int)pl.L); } while (0)
#ifdef LQ_DEV_KNOBS
#define LQ_TINY2(NT_) do { \
            if (lg == 1) LQ_TINY3(NT_, 2, 1); \
            else if (lg == 2) { if (U == 2) LQ_TINY3(NT_, 2, 2); else LQ_TINY3(NT_, 4, 2); } \
            else if (lg == 3) { if (U == 2) LQ_TINY3(NT_, 2, 3); else LQ_TINY3(NT_, 4, 3); } \
            else { if (U == 2) LQ_TINY3(NT_, 2, 4); else LQ_TINY3(NT_, 4, 4); } } while (0)
#else       // two passes of rows per wave (four measured no better: profiles/r02/tuning_sweeps.txt)
#define LQ_TINY2(NT_) do { \
            if (lg == 1) LQ_TINY3(NT_, 2, 1); \
            else if (lg == 2) LQ_TINY3(NT_, 2, 2); \
            else if (lg == 3) LQ_TINY3(NT_, 2, 3); \
            else LQ_TINY3(NT_, 2, 4); } while (0)
#endif
        if (nt) LQ_TINY2(1); else LQ_TINY2(0);
#undef LQ_TINY2
#undef LQ_TINY3
        return check_hip("tiny-row launch") ? -1 : 1;
    }
    }      // kStreamOp<OP>
}

template <int OP>
static int launch_traverse(Plan& pl, const Params& p, hipStream_t st) {
    using O = OpT<OP>;
    if (!kStreamOp<OP> && pl.mode == MODE_ROW_BIG && pl.bs != kBlock) return fail(LQ_EINVAL, "internal: operation %d planned with %d-thread units", OP, pl.bs);
    {
        const int r2 = launch_stream2<OP>(pl, p, st);
        if (r2 < 0) return LQ_EHIP;
        if (r2 > 0) return LQ_OK;
    }
    if (pl.mode == MODE_ROW_BIG) {
        // float4 path: 16-byte aligned bases; rows of any length (a scalar head/tail of <= 3 elements re-aligns each chunk)
        const bool vec = aligned(p.P, 16) && (!O::kDy || aligned(p.dy, 16)) && (!O::kStore || aligned(p.out, 16));
        // Chunk size by row length (streaming sizes, where the plan says 512 threads).  A row is cut into chunks of CH
        // elements and its last chunk is whatever remains: rows of 2500 elements fill 61 % of two 2048-chunks but 81 % of
        // three 1024-chunks.  Measured, K4 at 512 -> 256 threads: rows of 2500: 4.4 -> 6.0 TB/s, 3000: 5.1 -> 6.1, 5000: 5.8 ->
        // 6.3, 6000 (same fill): 6.2 = 6.2; K2 (two float4 per thread, CH = 4096): 5000: 5.7 -> 6.5, 6000: 5.9 -> 6.6, but a
        // row that is ONE chunk keeps it (2500: 6.8 against 6.3).  The BENCH rows (50176 = 24.5 x 2048) keep 512 threads.
        LQ_KNOB(tune_chunk, "LQ_TUNE_CHUNK", 1);     // development knob: 0 = always the plan's block size
        LQ_KNOB(forced_bs, "LQ_TUNE_BS", 0);
        if (pl.bs == 512 && vec && tune_chunk && !p.direct && !forced_bs && pl.np_bound >= pl.R * row_chunks(pl.L, 1024)) {
            auto fill = [&](int64_t CH) { return (double)pl.L / (double)(row_chunks(pl.L, CH) * CH); };
            const bool k2_form = (OP == OP_BWD || (OP == OP_FUSED && p.tmode >= 1)) && (double)pl.R * (double)pl.L * 4.0 >= (double)kNtBytes;
            const bool small = k2_form ? (row_chunks(pl.L, 4096) > 1 && fill(1024) > fill(4096) + 0.1) : (fill(1024) > fill(2048) + 0.05);
            if (small) {
                pl.bs = 256;
                pl.CH = 1024;
                pl.nc = row_chunks(pl.L, 1024);
                pl.lay = layout_row_chunks(pl.R, pl.nc, pl.R / p.G, p.G);      // the finalize that follows must walk the partial layout this launch produces
            }
        }
        const int64_t units = pl.R * pl.nc;
        if (units > 2147483647ll) return fail(LQ_EINVAL, "too many work units (%lld)", (long long)units);
        const int64_t outer_f = pl.R / p.G;
        const int grid3d = (p.G <= 65535 && outer_f <= 65535 && pl.R == outer_f * p.G) ? 1 : 0;
        const dim3 grid = grid3d ? dim3((unsigned)pl.nc, (unsigned)p.G, (unsigned)outer_f) : dim3((unsigned)units);
        const bool nt = kStreamOp<OP> && vec && (double)pl.R * (double)pl.L * 4.0 >= (double)kNtBytes;
        // Two float4 per thread and stream (see row_stream_body): the backward always (measured 100.3 vs 101.4 us per
        // BENCH step, and 105 vs 116 us at lambda = 1e-3 where every element takes the exact-ratio + tanh branch; it
        // also halves the partials the finalize walks); the fused kernel only when lambda >= 4e-4 (77.4 vs 81.7 us
        // there, but 77.7 vs 75.4 us at small lambda).  The unit doubles, so the chunk count halves; the workspace
        // bound (computed for one float4 per thread) still holds.  Four float4 per thread in K2 were measured in round 2:
        // 49.5 against 48.0 us on the BENCH tensor -- not better.
        LQ_KNOB(tune_u2, "LQ_TUNE_U2", -1);   // force 0/1
        const bool want_u2 = tune_u2 >= 0 ? tune_u2 == 1 : (OP == OP_BWD || p.tmode >= 1);
        const bool u2 = (OP == OP_BWD || OP == OP_FUSED) && want_u2 && vec && nt && pl.bs == 512;
        // rows with a folded tail or with chunks off the 16-byte grid take the TAIL instantiation (see row_stream_body)
        auto needs_tail = [&](int64_t CH) {
            const int64_t r = pl.L % CH;
            return pl.L % 4 != 0 || (pl.L > CH && r != 0 && r * 8 <= CH);
        };
        if constexpr (OP == OP_BWD || OP == OP_FUSED) if (u2) {
            const int64_t nc2 = row_chunks(pl.L, (int64_t)pl.bs * 8);
            const dim3 grid2 = grid3d ? dim3((unsigned)nc2, (unsigned)p.G, (unsigned)outer_f) : dim3((unsigned)(pl.R * nc2));
            // the scale gradient walks these units backwards, with the cache-policy mix of kMixK2 (kMallWalk)
            int64_t keep_from = OP == OP_BWD ? mall_keep_from(pl.R * pl.L) : 0;
            const uint32_t mix = OP == OP_BWD ? mix_k2() : 0u;
#ifdef LQ_DEV_KNOBS
            if (g_dev_flags_host & 0x1000) keep_from = -1 - keep_from;      // the forward walk
#endif
            if (needs_tail((int64_t)pl.bs * 8))
                hipExtLaunchKernelGGL((k_row_stream<OP, 4, 512, 1, 2, 1>), grid2, dim3(512), 0, st, g_prof_start, g_prof_stop, 0, p, pl.L, nc2, grid3d, mix, keep_from);
            else
                hipExtLaunchKernelGGL((k_row_stream<OP, 4, 512, 1, 2, 0>), grid2, dim3(512), 0, st, g_prof_start, g_prof_stop, 0, p, pl.L, nc2, grid3d, mix, keep_from);
            // the finalize that follows must walk the partial layout this launch produced
            pl.CH = pl.bs * 8;
            pl.nc = nc2;
            pl.lay = layout_row_chunks(pl.R, nc2, outer_f, p.G);
            return check_hip("traversal launch");
        }
        // hipExtLaunchKernelGGL with NULL events is a plain launch; with lq_profile_events() set, the events take the kernel's own
        // begin / end timestamps (what rocprofv3 reports as its duration)
        const bool tail1 = needs_tail((int64_t)pl.CH);
        // (TAIL = 0 forms that no descriptor reaches are not compiled: K1 beyond 256-thread default-policy units, K2 with
        // nontemporal 512-thread units -- see the two internal errors below)
#define LQ_LAUNCH_STREAM(VEC_, BS_, NT_) do { \
        constexpr bool kTail0 = kDevKnobs || (VEC_ == 4 && !(OP == OP_FWD && (BS_ != kBlock || NT_ != 0)) && !(OP == OP_BWD && BS_ == 512 && NT_ == 1)); \
        constexpr bool kTail1 = kDevKnobs || !(OP == OP_BWD && VEC_ == 4 && BS_ == 512 && NT_ == 1); \
        if (VEC_ == 1 || tail1) { if constexpr (kTail1) hipExtLaunchKernelGGL((k_row_stream<OP, VEC_, BS_, NT_, 1, 1>), grid, dim3(BS_), 0, st, g_prof_start, g_prof_stop, 0, p, pl.L, pl.nc, grid3d, 0u, (int64_t)0); } \
        else { if constexpr (kTail0) hipExtLaunchKernelGGL((k_row_stream<OP, VEC_, BS_, NT_, 1, 0>), grid, dim3(BS_), 0, st, g_prof_start, g_prof_stop, 0, p, pl.L, pl.nc, grid3d, 0u, (int64_t)0); } } while (0)
        if constexpr (!kStreamOp<OP>) {
            if (vec) LQ_LAUNCH_STREAM(4, 256, 0);
            else LQ_LAUNCH_STREAM(1, 256, 0);
        } else if (!kDevKnobs && OP == OP_FWD && vec && !tail1 && (pl.bs != kBlock || nt)) {
            // K1 of aligned rows with L % 4 == 0 at streaming size is the flat one-shot stream (launch_stream2): no row-stream
            // instantiation exists for it
            return fail(LQ_EINVAL, "internal: streaming-size forward of aligned rows reached the row stream");
        } else if (!kDevKnobs && OP == OP_BWD && vec && nt && pl.bs == 512) {
            // K2 with nontemporal 512-thread units always takes two float4 per thread (u2 above)
            return fail(LQ_EINVAL, "internal: streaming-size scale gradient reached the one-float4 row stream");
        } else if (vec) {
#ifdef LQ_DEV_KNOBS
            if (pl.bs == 1024) {
                if (nt) LQ_LAUNCH_STREAM(4, 1024, 1);
                else LQ_LAUNCH_STREAM(4, 1024, 0);
            } else
#endif
            if (pl.bs == 512) {
                if (nt) LQ_LAUNCH_STREAM(4, 512, 1);
                else LQ_LAUNCH_STREAM(4, 512, 0);
            } else {
                if (nt) LQ_LAUNCH_STREAM(4, 256, 1);
                else LQ_LAUNCH_STREAM(4, 256, 0);
            }
        } else {
#ifdef LQ_DEV_KNOBS
            if (pl.bs == 1024) LQ_LAUNCH_STREAM(1, 1024, 0);
            else
#endif
            if (pl.bs == 512) LQ_LAUNCH_STREAM(1, 512, 0);
            else LQ_LAUNCH_STREAM(1, 256, 0);
        }
#undef LQ_LAUNCH_STREAM
    } else if (pl.mode == MODE_ROW_SMALL) {
        const bool vec = row_small_vec(pl, p.P, O::kDy ? p.dy : nullptr, O::kStore ? p.out : nullptr);
        const int lg = vec ? row_small_lpr_log2_vec(pl.L) : pl.lpr_log2;
        const int64_t blocks = ceil_div(pl.R, kBlock >> lg);
        if (blocks > 2147483647ll) return fail(LQ_EINVAL, "too many blocks (%lld)", (long long)blocks);
        if (vec) hipLaunchKernelGGL((k_row_small<OP, 4>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, pl.R, (int)pl.L, lg);
        else hipLaunchKernelGGL((k_row_small<OP, 1>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, pl.R, (int)pl.L, lg);
    } else {
        int variant;
        int64_t nbx;
        col_variant(pl, p.P, O::kDy ? p.dy : nullptr, O::kStore ? p.out : nullptr, variant, nbx);
        const int64_t blocks = nbx * pl.ysplit;
        if (blocks > 2147483647ll) return fail(LQ_EINVAL, "too many blocks (%lld)", (long long)blocks);
        hipLaunchKernelGGL((k_col<OP>), dim3((unsigned)blocks), dim3(kBlock), 0, st, p, pl.C, pl.rps, nbx, variant, pl.ysplit);
    }
    return check_hip("traversal launch");
}

// The column form (lq_traverse.hpp) of a single launch pays four waves per 64 columns walking n1 rows eight at a time: it wins
// where the other forms gather megabytes of scattered words (6144 x 6144 column-wise: 8.7 -> 5.6 us; 4096 x 4096, whose 32
// partials per group used to go to the thread form: 10.3 -> 4.8 us) and loses on small partial sets or many rows per column
// (16384 x 1001: 4.9 -> 8.4 us, eleven dependent rounds in 16 blocks).  The multi-tensor batch uses it wherever the geometry
// allows (its tasks share one launch, the amplified gathers add up: lq_batch.hpp).
static bool finalize_cols_single(const FinGeom& f) {
    return finalize_cols_ok(f.groups, f.gstride, f.n1, f.stride1, f.n2) && f.n1 <= 64 && f.n1 * f.groups * f.n2 >= 131072;
}

template <int OP, bool COLS = true>      // COLS = false: global reductions (one group) never take the column form
static int launch_finalize(const Params& p, FinGeom f, hipStream_t st) {
    const int form = finalize_form(f.groups, f.n1, f.stride1, f.n2);       // lq_traverse.hpp
    if (COLS && finalize_cols_single(f)) {
        if constexpr (COLS) hipLaunchKernelGGL((k_finalize_cols<OP>), dim3((unsigned)ceil_div(f.groups, 64 / f.n2)), dim3(kBlock), 0, st, p, f);
    } else if (form == 0) {
        hipLaunchKernelGGL((k_finalize_thread<OP>), dim3((unsigned)ceil_div(f.groups, kBlock)), dim3(kBlock), 0, st, p, f);
    } else if (form == 1) {
        hipLaunchKernelGGL((k_finalize_block<OP, 64>), dim3((unsigned)f.groups), dim3(64), 0, st, p, f);
    } else if (form == 2) {
        hipLaunchKernelGGL((k_finalize_block<OP, 256>), dim3((unsigned)f.groups), dim3(256), 0, st, p, f);
    } else {
        hipLaunchKernelGGL((k_finalize_block<OP, 1024>), dim3((unsigned)f.groups), dim3(1024), 0, st, p, f);
    }
    return check_hip("finalize launch");
}

static FinGeom group_geom(const Plan& pl, int64_t outer, int64_t G, int64_t inner) {
    FinGeom f;
    memset(&f, 0, sizeof(f));
    f.groups = G;
    f.gstride = pl.lay.gstride;
    f.n1 = pl.lay.n1;
    f.stride1 = pl.lay.stride1;
    f.n2 = pl.lay.n2;
    f.count = (double)outer * (double)inner;
    return f;
}

static FinGeom global_geom(const Plan& pl, int64_t outer, int64_t G, int64_t inner) {
    FinGeom f;
    memset(&f, 0, sizeof(f));
    f.groups = 1;
    f.gstride = 0;
    f.n1 = 1;
    f.stride1 = 0;
    f.n2 = pl.lay.np;
    f.count = (double)outer * (double)G * (double)inner;
    return f;
}

static Params base_params(const float* P, const float* s, int64_t outer, int64_t G, int64_t inner) {
    Params p;
    memset(&p, 0, sizeof(p));
    p.P = P;
    p.s = s;
    p.outer = outer;
    p.G = G;
    p.inner = inner;
    return p;
}

// The vote's branch of the scale gradient by lambda (lq_ops.hpp).  A NaN lambda fails both comparisons: 2.
static int tmode_of(float lambda) { return (lambda < 4.0e-4f) ? 0 : ((lambda <= 0.25f) ? 1 : 2); }

// The tail of the per-group reductions: the traversal OP into the bound workspace, then the finalize FIN_OP into o0 / o1 / o2
// (FinGeom's outputs; NULL = not wanted).  With `allow_direct` and one partial per group the traversal emits the outputs itself
// and no finalize is launched: o0 and, as the second pointer, o1 or else o2 (emit_direct of the clipped ops hands it on as
// FinGeom::o2).  No finalize either when no output is wanted (a clipped backward called for dP alone).
template <int OP, int FIN_OP = OP>
static int traverse_and_finalize(Plan& pl, Params& p, float* o0, float* o1, uint32_t* o2, bool allow_direct, hipStream_t st) {
    const bool direct = allow_direct && pl.lay.n1 * pl.lay.n2 == 1;
    if (direct) {
        p.direct = 1;
        p.e0 = o0;
        p.e1 = o1 ? o1 : reinterpret_cast<float*>(o2);
        p.ecount = (double)p.outer * (double)p.inner;
    }
    if (int rc = launch_traverse<OP>(pl, p, st)) return rc;
    if (direct || (!o0 && !o1 && !o2)) return LQ_OK;
    FinGeom f = group_geom(pl, p.outer, p.G, p.inner);
    f.o0 = o0;
    f.o1 = o1;
    f.o2 = o2;
    return launch_finalize<FIN_OP>(p, f, st);
}

static bool make_conv_tile(ConvTile& ct, int64_t hw, int64_t ci, int64_t co, int64_t outer, int64_t G, int64_t inner);
static PartialLayout conv_tile_layout(const ConvTile& ct, int64_t G);

}  // namespace lq

using namespace lq;

// fn: the entry point's name as the caller spelled it (it opens every message); bodies shared by two entry points pass it on
#define LQ_REQUIRE_PTR_FN(fn, x)                                               \
    do {                                                                       \
        if (!(x)) return fail(LQ_EINVAL, "%s: argument '%s' is NULL", fn, #x); \
        if (!aligned((x), 4)) return fail(LQ_EALIGN, "%s: argument '%s' is not 4-byte aligned", fn, #x); \
    } while (0)
#define LQ_REQUIRE_PTR(x) LQ_REQUIRE_PTR_FN(__func__, x)

extern "C" {

int lq_version(void) { return LQ_ABI_VERSION; }

#ifdef LQ_DEV_KNOBS
int lq_dev_set_ablate(int mask) {      // development builds only (see lq_conv_tile.hpp)
    return hipMemcpyToSymbol(HIP_SYMBOL(lq::g_ablate), &mask, sizeof(int)) == hipSuccess ? LQ_OK : LQ_EHIP;
}
#endif

#ifdef LQ_DEV_KNOBS
int lq_dev_set_flags(int bits) {       // development builds only (see lq_stream2.hpp)
    g_dev_flags_host = bits;
    return hipMemcpyToSymbol(HIP_SYMBOL(lq::g_dev_flags), &bits, sizeof(int)) == hipSuccess ? LQ_OK : LQ_EHIP;
}
#endif

#ifdef LQ_DEV_KNOBS
int lq_dev_set_policy_mix(unsigned k1, unsigned k2) {      // development builds only (see mix_k1 / mix_k2 above)
    g_dev_mix_k1 = k1;
    g_dev_mix_k2 = k2;
    return LQ_OK;
}
#endif

#ifdef LQ_DEV_KNOBS
int lq_dev_set_trace(void* buf) {      // development builds only: block timeline of the batch traversals (lq_conv_tile.hpp)
    unsigned long long* b = (unsigned long long*)buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(lq::g_trace), &b, sizeof(b)) == hipSuccess ? LQ_OK : LQ_EHIP;
}
#endif

int lq_profile_events(void* start, void* stop) {
    g_prof_start = (hipEvent_t)start;
    g_prof_stop = (hipEvent_t)stop;
    return LQ_OK;
}

const char* lq_last_error(void) { return g_err; }

const char* lq_status_string(int status) {
    switch (status) {
        case LQ_OK: return "LQ_OK";
        case LQ_EINVAL: return "LQ_EINVAL";
        case LQ_EHIP: return "LQ_EHIP";
        case LQ_EWORKSPACE: return "LQ_EWORKSPACE";
        case LQ_EALIGN: return "LQ_EALIGN";
        default: return "LQ_UNKNOWN";
    }
}

size_t lq_workspace_bytes(int64_t outer, int64_t G, int64_t inner) {
    if (outer <= 0 || G <= 0 || inner <= 0) return 0;
    return ws_bytes_for(make_plan(outer, G, inner));
}

int lq_fq_forward(const float* P, const float* s, float* out, void* q, int q_dtype, int64_t outer, int64_t G,
                  int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    if (!out && !q) return fail(LQ_EINVAL, "lq_fq_forward: both out and q are NULL");
    if ((rc = check_q_view(__func__, q, q_dtype))) return rc;
    Plan pl = make_plan(outer, G, inner);
    Params p = base_params(P, s, outer, G, inner);
    p.q = q;
    p.q_dtype = q_dtype;
    if (out) {
        if (!aligned(out, 4)) return fail(LQ_EALIGN, "lq_fq_forward: out is not 4-byte aligned");
        p.out = out;
        return launch_traverse<OP_FWD>(pl, p, (hipStream_t)stream);
    }
    pl = make_plan(outer, G, inner, kBlock);      // the integer view alone (callbacks / export): 256-thread units (kStreamOp)
    return launch_traverse<OP_QONLY>(pl, p, (hipStream_t)stream);
}

static int check_conv(const char* fn, int64_t hw, int64_t ci, int64_t co, int64_t outer, int64_t G, int64_t inner) {
    if (hw <= 0 || ci <= 0 || co <= 0) return fail(LQ_EINVAL, "%s: hw, ci, co must be positive", fn);
    const double n = (double)hw * (double)ci * (double)co;
    if (n != (double)outer * (double)G * (double)inner) return fail(LQ_EINVAL, "%s: hw*ci*co does not match the tensor", fn);
    if (n >= 4294967296.0) return fail(LQ_EINVAL, "%s: conv kernels must have fewer than 2^32 elements", fn);
    return LQ_OK;
}

int lq_fq_forward_oihw(const float* P, const float* s, float* out, float* out_oihw, int64_t hw, int64_t ci, int64_t co,
                       int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    if ((rc = check_conv("lq_fq_forward_oihw", hw, ci, co, outer, G, inner))) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(out_oihw);
    if (!out && !(aligned(P, 16) && lq_conv_tile_supported(hw, ci, co, outer, G, inner)))
        return fail(LQ_EINVAL, "lq_fq_forward_oihw: out may be NULL only for kernels the LDS-tile path takes (lq_conv_tile_supported) with P 16-byte aligned");
    Plan pl = make_plan(outer, G, inner, kBlock);      // weight-sized operation: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    p.out = out;
    p.out_perm = out_oihw;
    p.perm_hw = (uint32_t)hw;
    p.perm_ci = (uint32_t)ci;
    p.perm_co = (uint32_t)co;
    ConvTile ct;
    if (aligned(P, 16) && aligned(out, 16) && make_conv_tile(ct, hw, ci, co, outer, G, inner)) {      // LDS tiles (lq_conv_tile.hpp)
        hipLaunchKernelGGL(k_conv_tile_fwd, dim3(ct.ntc * ct.nto), dim3(kBlock), 0, (hipStream_t)stream, p, ct);
        return check_hip("conv tile forward launch");
    }
    return launch_traverse<OP_FWD_PERM>(pl, p, (hipStream_t)stream);      // element-wise companion (kernels with > 9 taps, co % 4 != 0, ...)
}

int lq_conv_tile_supported(int64_t hw, int64_t ci, int64_t co, int64_t outer, int64_t G, int64_t inner) {
    if (outer <= 0 || G <= 0 || inner <= 0 || hw <= 0 || ci <= 0 || co <= 0) return 0;
    if ((double)hw * (double)ci * (double)co != (double)outer * (double)G * (double)inner) return 0;
    ConvTile ct;
    return make_conv_tile(ct, hw, ci, co, outer, G, inner) ? 1 : 0;
}

size_t lq_conv_workspace_bytes(int64_t hw, int64_t ci, int64_t co, int64_t outer, int64_t G, int64_t inner) {
    if (outer <= 0 || G <= 0 || inner <= 0) return 0;
    size_t need = ws_bytes_for(make_plan(outer, G, inner));
    ConvTile ct;
    if (hw > 0 && ci > 0 && co > 0 && make_conv_tile(ct, hw, ci, co, outer, G, inner)) {
        const size_t t = ws_bytes_for(plan_of_layout(conv_tile_layout(ct, G)));
        if (t > need) need = t;
    }
    return need;
}

int lq_fq_scale_grad_oihw(const float* P, const float* s, const float* dy_oihw, float lambda, float* ds, float* dP,
                          void* ws, size_t ws_bytes, int64_t hw, int64_t ci, int64_t co,
                          int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    if ((rc = check_conv("lq_fq_scale_grad_oihw", hw, ci, co, outer, G, inner))) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(dy_oihw);
    LQ_REQUIRE_PTR(ds);
    LQ_REQUIRE_PTR(dP);
    Plan pl = make_plan(outer, G, inner, kBlock);      // weight-sized operation: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    p.dy = P;                     // valid dummy for the traversals' dy loads; the op gathers from dy_perm
    p.dy_perm = dy_oihw;
    p.dp_out = dP;
    p.perm_hw = (uint32_t)hw;
    p.perm_ci = (uint32_t)ci;
    p.perm_co = (uint32_t)co;
    p.lam = lambda;
    p.tmode = tmode_of(lambda);
    ConvTile ct;
    if (aligned(P, 16) && aligned(dP, 16) && make_conv_tile(ct, hw, ci, co, outer, G, inner)) {       // LDS tiles (lq_conv_tile.hpp)
        const Plan tp = plan_of_layout(conv_tile_layout(ct, G));
        if (ws && ws_bytes < ws_bytes_for(tp))
            return fail(LQ_EWORKSPACE, "lq_fq_scale_grad_oihw: workspace too small: %zu < %zu bytes (size it with lq_conv_workspace_bytes)",
                        ws_bytes, ws_bytes_for(tp));
        if ((rc = bind_ws(p, tp, ws, ws_bytes))) return rc;
        hipLaunchKernelGGL(k_conv_tile_bwd, dim3(ct.ntc * ct.nto), dim3(kBlock), 0, (hipStream_t)stream, p, ct);
        if ((rc = check_hip("conv tile backward launch"))) return rc;
        FinGeom f = group_geom(tp, outer, G, inner);
        f.o0 = ds;
        return launch_finalize<OP_BWD>(p, f, (hipStream_t)stream);
    }
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    return traverse_and_finalize<OP_BWD_PERM, OP_BWD>(pl, p, ds, nullptr, nullptr, true, (hipStream_t)stream);
}

int lq_fq_scale_grad(const float* P, const float* s, const float* dy, float lambda, float* ds, float* parts, void* ws,
                     size_t ws_bytes, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(dy);
    LQ_REQUIRE_PTR(ds);
    Plan pl = make_plan(outer, G, inner);
    Params p = base_params(P, s, outer, G, inner);
    p.dy = dy;
    p.lam = lambda;
    p.tmode = tmode_of(lambda);
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    return traverse_and_finalize<OP_BWD>(pl, p, ds, parts, nullptr, true, (hipStream_t)stream);
}

int lq_fq_scale_grad_ste(const float* P, const float* s, const float* dy, float grad_scale, float* ds, void* ws, size_t ws_bytes,
                         int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(dy);
    LQ_REQUIRE_PTR(ds);
    Plan pl = make_plan(outer, G, inner, kBlock);      // generic traversal bodies: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    p.dy = dy;
    p.c_scale = grad_scale;
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    return traverse_and_finalize<OP_STE_SCALE>(pl, p, ds, nullptr, nullptr, true, (hipStream_t)stream);
}

static int check_clip_range(const char* fn, int32_t qmin, int32_t qmax) {
    constexpr int32_t kLim = 1 << 24;      // integers up to 2^24 in magnitude are exact in fp32
    if (qmin > qmax) return fail(LQ_EINVAL, "%s: qmin %d > qmax %d", fn, (int)qmin, (int)qmax);
    if (qmin < -kLim || qmax > kLim) return fail(LQ_EINVAL, "%s: range [%d, %d] is outside +-2^24", fn, (int)qmin, (int)qmax);
    return LQ_OK;
}

static int check_rounding(const char* fn, int rounding) {
    if (rounding != LQ_ROUND_FLOOR && rounding != LQ_ROUND_NEAREST_EVEN) return fail(LQ_EINVAL, "%s: bad rounding %d", fn, rounding);
    return LQ_OK;
}

// One body per direction behind both spellings of the entry point; `fn` is the name the caller used.
static int clip_forward(const char* fn, const float* P, const float* s, float* out, void* q, int q_dtype, int32_t qmin, int32_t qmax,
                        int rounding, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    LQ_REQUIRE_PTR_FN(fn, out);
    if ((rc = check_clip_range(fn, qmin, qmax))) return rc;
    if ((rc = check_rounding(fn, rounding))) return rc;
    if ((rc = check_q_view(fn, q, q_dtype))) return rc;
    Plan pl = make_plan(outer, G, inner, kBlock);      // generic traversal bodies: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    p.out = out;
    p.q = q;
    p.q_dtype = q_dtype;
    p.clip_lo = (float)qmin;
    p.clip_hi = (float)qmax;
    // the rounding is a template parameter of the op trait: each pair has its own kernels, none tests a flag
    if (rounding == LQ_ROUND_NEAREST_EVEN) return launch_traverse<OP_CLIP_FWD_RNE>(pl, p, (hipStream_t)stream);
    return launch_traverse<OP_CLIP_FWD>(pl, p, (hipStream_t)stream);
}

int lq_fq_forward_clip_r(const float* P, const float* s, float* out, void* q, int q_dtype, int32_t qmin, int32_t qmax, int rounding,
                         int64_t outer, int64_t G, int64_t inner, void* stream) {
    return clip_forward(__func__, P, s, out, q, q_dtype, qmin, qmax, rounding, outer, G, inner, stream);
}

int lq_fq_forward_clip(const float* P, const float* s, float* out, void* q, int q_dtype, int32_t qmin, int32_t qmax, int64_t outer,
                       int64_t G, int64_t inner, void* stream) {
    return clip_forward(__func__, P, s, out, q, q_dtype, qmin, qmax, LQ_ROUND_FLOOR, outer, G, inner, stream);
}

static int clip_backward(const char* fn, const float* P, const float* s, const float* dy, int32_t qmin, int32_t qmax, int rounding,
                         float grad_scale, float* dP, float* ds, uint32_t* clipped, void* ws, size_t ws_bytes, int64_t outer, int64_t G,
                         int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    LQ_REQUIRE_PTR_FN(fn, dy);
    LQ_REQUIRE_PTR_FN(fn, dP);
    if (ds && !aligned(ds, 4)) return fail(LQ_EALIGN, "%s: ds is not 4-byte aligned", fn);
    if (clipped && !aligned(clipped, 4)) return fail(LQ_EALIGN, "%s: clipped is not 4-byte aligned", fn);
    if ((rc = check_clip_range(fn, qmin, qmax))) return rc;
    if ((rc = check_rounding(fn, rounding))) return rc;
    Plan pl = make_plan(outer, G, inner, kBlock);      // generic traversal bodies, as lq_fq_scale_grad_ste
    Params p = base_params(P, s, outer, G, inner);
    p.dy = dy;
    p.out = dP;
    p.c_scale = grad_scale;
    p.clip_lo = (float)qmin;
    p.clip_hi = (float)qmax;
    // the workspace is required, and checked, also for "mask only" calls: one kernel serves both, the sum is dropped at the emit
    if (!ws || ws_bytes < ws_bytes_for(pl)) return fail(LQ_EINVAL, "%s: workspace %s (%zu bytes given, %zu needed)", fn,
                                                        ws ? "too small" : "is NULL", ws ? ws_bytes : (size_t)0, ws_bytes_for(pl));
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    // the rounding is a template parameter of the op trait: each pair has its own kernels, none tests a flag
    if (rounding == LQ_ROUND_NEAREST_EVEN) return traverse_and_finalize<OP_CLIP_BWD_RNE>(pl, p, ds, nullptr, clipped, true, (hipStream_t)stream);
    return traverse_and_finalize<OP_CLIP_BWD>(pl, p, ds, nullptr, clipped, true, (hipStream_t)stream);
}

int lq_fq_backward_clip_r(const float* P, const float* s, const float* dy, int32_t qmin, int32_t qmax, int rounding, float grad_scale,
                          float* dP, float* ds, uint32_t* clipped, void* ws, size_t ws_bytes, int64_t outer, int64_t G, int64_t inner,
                          void* stream) {
    return clip_backward(__func__, P, s, dy, qmin, qmax, rounding, grad_scale, dP, ds, clipped, ws, ws_bytes, outer, G, inner, stream);
}

int lq_fq_backward_clip(const float* P, const float* s, const float* dy, int32_t qmin, int32_t qmax, float grad_scale, float* dP,
                        float* ds, uint32_t* clipped, void* ws, size_t ws_bytes, int64_t outer, int64_t G, int64_t inner, void* stream) {
    return clip_backward(__func__, P, s, dy, qmin, qmax, LQ_ROUND_FLOOR, grad_scale, dP, ds, clipped, ws, ws_bytes, outer, G, inner, stream);
}

// ---- group-wise (block) scales of the clipped pair, symmetric and with an offset, and their initialisation ----
// (lq_group.hpp, lq_scale_init.hpp)
// Dispatch is a pure function of the arguments: axis picks the traversal, V = 4 (float4) needs C % 4 == 0 (and gs % 4 == 0 on
// axis 1) and every dense base 16-byte aligned, anything else that is 4-byte aligned runs the scalar form.  Neither form has a
// second stage: the workspace size is 0 for every shape.  Scale, offset, ds and db are read and written one element at a time.
static int check_group(const char* fn, int64_t R, int64_t C, int axis, int64_t gs) {
    if (R <= 0 || C <= 0) return fail(LQ_EINVAL, "%s: extents must be positive (R=%lld C=%lld)", fn, (long long)R, (long long)C);
    if ((double)R * (double)C >= 2147483648.0) return fail(LQ_EINVAL, "%s: R * C = %lld * %lld is not below 2^31", fn, (long long)R, (long long)C);
    if (axis != 0 && axis != 1) return fail(LQ_EINVAL, "%s: bad axis %d (0: groups along R, 1: groups along C)", fn, axis);
    if (gs < 1) return fail(LQ_EINVAL, "%s: group size %lld < 1", fn, (long long)gs);
    return LQ_OK;
}

static GroupParams group_params(const float* P, const float* s, int32_t qmin, int32_t qmax, int64_t R, int64_t C, int axis, int64_t gs) {
    GroupParams p{};
    const int64_t len = axis == 0 ? R : C;
    if (gs > len) gs = len;      // gs >= len: one group per line
    p.P = P;
    p.s = s;
    p.lo = (float)qmin;
    p.hi = (float)qmax;
    p.k = 1.0f;
    p.R = (int32_t)R;
    p.C = (int32_t)C;
    p.gs = (int32_t)gs;
    p.nb = (int32_t)((len + gs - 1) / gs);
    return p;
}

static bool group_vec_ok(const GroupParams& p, int axis) { return p.C % 4 == 0 && (axis == 0 || p.gs % 4 == 0); }

// The launch shape of a group-wise tensor.  This is the ONE statement of the rule: the forward and backward pairs (symmetric and
// with an offset), both scale initialisations and the batch's task table (fill_group_task) all ask here, which keeps a tensor's
// form, team width and row split the same on every path.
struct GroupLaunch {
    int32_t form;         // GROUP_* of lq_group_batch.hpp: axis picks columns / rows, `vec` V = 4 / V = 1
    dim3 grid;
    int log_team;         // row forms: log2 of the lanes per (row, group) pair
    uint32_t nbx, nz;     // column forms: column tiles (grid.x) and blocks that share the rows of a group (grid.z)
    uint32_t blocks;      // of the grid
};
// `max_groups_y`, the group extent of a column grid.  A single-tensor kernel strides over the groups from kGroupGridY on; the batch
// has one block per (tile, group, z) and passes kGroupEveryGroup.  The two differ only above 32768 groups, where the row split
// (the one thing that reads the extent) is past its 2048-block cap on either path.
constexpr int64_t kGroupGridY = 32768;
constexpr int64_t kGroupEveryGroup = INT32_MAX;

// row_split: the forward of the column forms, which has nothing to merge, may share the rows of a group among up to 4 blocks (a
// block per (column tile, group) leaves the chip half empty on weight-sized tensors); whoever needs a whole group in one block
// (backward, scale initialisation) passes false.
static GroupLaunch group_launch(const GroupParams& p, int axis, bool vec, bool row_split, int64_t max_groups_y) {
    GroupLaunch L{};
    L.nbx = L.nz = 1;
    if (axis == 0) {
        const int lanes = vec ? kGroupColsLanes4 : kGroupColsLanes1, cols = lanes * (vec ? 4 : 1), slots = kBlock / lanes;
        const int64_t groups_y = std::min<int64_t>(p.nb, max_groups_y);
        L.form = vec ? GROUP_COLS4 : GROUP_COLS1;
        L.nbx = (uint32_t)((p.C + cols - 1) / cols);
        while (row_split && L.nz < 4 && (int64_t)L.nbx * groups_y * L.nz < 2048 && (int64_t)slots * L.nz * 4 <= p.gs) L.nz *= 2;
        L.grid = dim3(L.nbx, (unsigned)groups_y, L.nz);
    } else {
        const int64_t items = (p.gs + (vec ? 3 : 0)) / (vec ? 4 : 1);      // about four accesses per lane
        while (L.log_team < 6 && ((int64_t)4 << L.log_team) < items) ++L.log_team;
        const int64_t pairs = (int64_t)p.R * p.nb, per_block = kBlock >> L.log_team;
        L.form = vec ? GROUP_ROWS4 : GROUP_ROWS1;
        L.grid = dim3((unsigned)((pairs + per_block - 1) / per_block));
    }
    L.blocks = L.grid.x * L.grid.y * L.grid.z;
    return L;
}

extern "C++" {      // templates inside the C-linkage block
// The four instantiations of a kernel family, in launch_group_form's order: columns V = 4, V = 1, rows V = 4, V = 1
#define LQ_GROUP_FAMILY(COLS, ROWS, ...) \
    COLS<__VA_ARGS__, 4, kGroupColsLanes4>, COLS<__VA_ARGS__, 1, kGroupColsLanes1>, ROWS<__VA_ARGS__, 4>, ROWS<__VA_ARGS__, 1>
// the same of a family with no template arguments ahead of V
#define LQ_GROUP_FAMILY0(COLS, ROWS) COLS<4, kGroupColsLanes4>, COLS<1, kGroupColsLanes1>, ROWS<4>, ROWS<1>

// Launches the member of a family that the form names; `family` opens the message of a failed launch, `lds` is dynamic LDS in bytes
template <class Args>
static int launch_group_form(const GroupLaunch& L, void (*cols4)(Args), void (*cols1)(Args), void (*rows4)(Args, int),
                             void (*rows1)(Args, int), const Args& a, const char* family, hipStream_t st, size_t lds = 0) {
    const bool cols = L.form <= GROUP_COLS1;
    if (cols) hipLaunchKernelGGL(L.form == GROUP_COLS4 ? cols4 : cols1, L.grid, dim3(kBlock), lds, st, a);
    else hipLaunchKernelGGL(L.form == GROUP_ROWS4 ? rows4 : rows1, L.grid, dim3(kBlock), lds, st, a, L.log_team);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LQ_EHIP, "%s %s launch: %s", family, cols ? "column" : "row", hipGetErrorString(e));
    return LQ_OK;
}

// PT: GroupParams, GroupAffineParams or GroupMxParams.  The rounding is a template parameter of the kernels: none tests a flag
// (a minifloat grid has one rounding: `rounding` is not read for GroupMxParams)
template <bool BWD, class PT>
static int launch_group(const PT& pp, int axis, bool vec, int rounding, void* stream) {
    const GroupLaunch L = group_launch(group_base(pp), axis, vec, !BWD, kGroupGridY);
    const bool rne = rounding == LQ_ROUND_NEAREST_EVEN;
    hipStream_t st = (hipStream_t)stream;
    if constexpr (std::is_same_v<PT, GroupMxParams>) {
        return launch_group_form(L, LQ_GROUP_FAMILY(k_group_mx_cols, k_group_mx_rows, BWD), pp, "microscaling", st);
    } else if constexpr (kGroupHasOffset<PT>) {
        if (rne) return launch_group_form(L, LQ_GROUP_FAMILY(k_group_affine_cols, k_group_affine_rows, true, BWD), pp, "affine group-wise", st);
        return launch_group_form(L, LQ_GROUP_FAMILY(k_group_affine_cols, k_group_affine_rows, false, BWD), pp, "affine group-wise", st);
    } else {
        if (rne) return launch_group_form(L, LQ_GROUP_FAMILY(k_group_cols, k_group_rows, true, BWD), pp, "group-wise", st);
        return launch_group_form(L, LQ_GROUP_FAMILY(k_group_cols, k_group_rows, false, BWD), pp, "group-wise", st);
    }
}

// Scale initialisation takes the group-wise BACKWARD's shape (no row split: a block owns whole groups), so alignment handling and
// dead lanes / teams are the code that pair already runs.
template <int M, bool RNE>
static int launch_scale_init(const InitParams& ip, const GroupParams& gp, int axis, bool vec, const char* family, void* stream) {
    return launch_group_form(group_launch(gp, axis, vec, false, kGroupGridY), LQ_GROUP_FAMILY(k_init_cols, k_init_rows, M, RNE), ip,
                             family, (hipStream_t)stream);
}
}  // extern "C++"

// What the group forward entry points check and fill in common; affine: the offset b is an argument
static int group_forward_setup(const char* fn, const float* P, const float* s, bool affine, const float* b, float* out, void* q,
                               int q_dtype, int32_t qmin, int32_t qmax, int rounding, int64_t R, int64_t C, int axis, int64_t gs,
                               GroupParams& p, bool& vec) {
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if (affine) LQ_REQUIRE_PTR_FN(fn, b);
    LQ_REQUIRE_PTR_FN(fn, out);
    if ((rc = check_clip_range(fn, qmin, qmax))) return rc;
    if ((rc = check_rounding(fn, rounding))) return rc;
    if ((rc = check_q_view(fn, q, q_dtype))) return rc;
    if (q && q_dtype != LQ_Q_I8 && !aligned(q, 4)) return fail(LQ_EALIGN, "%s: q is not 4-byte aligned", fn);
    p = group_params(P, s, qmin, qmax, R, C, axis, gs);
    p.out = out;
    p.q = q;
    p.q_dtype = q_dtype;
    vec = group_vec_ok(p, axis) && aligned(P, 16) && aligned(out, 16);
    return LQ_OK;
}

// The same for the backward entry points; affine: b and the optional db are arguments
static int group_backward_setup(const char* fn, const float* P, const float* s, bool affine, const float* b, const float* dy,
                                int32_t qmin, int32_t qmax, int rounding, float grad_scale, float* dP, float* ds, float* db,
                                uint32_t* clipped, int64_t R, int64_t C, int axis, int64_t gs, GroupParams& p, bool& vec) {
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if (affine) LQ_REQUIRE_PTR_FN(fn, b);
    LQ_REQUIRE_PTR_FN(fn, dy);
    LQ_REQUIRE_PTR_FN(fn, dP);
    if (ds && !aligned(ds, 4)) return fail(LQ_EALIGN, "%s: ds is not 4-byte aligned", fn);
    if (affine && db && !aligned(db, 4)) return fail(LQ_EALIGN, "%s: db is not 4-byte aligned", fn);
    if (clipped && !aligned(clipped, 4)) return fail(LQ_EALIGN, "%s: clipped is not 4-byte aligned", fn);
    if ((rc = check_clip_range(fn, qmin, qmax))) return rc;
    if ((rc = check_rounding(fn, rounding))) return rc;
    p = group_params(P, s, qmin, qmax, R, C, axis, gs);
    p.dy = dy;
    p.out = dP;
    p.k = grad_scale;
    p.ds = ds;
    p.clipped = clipped;
    vec = group_vec_ok(p, axis) && aligned(P, 16) && aligned(dy, 16) && aligned(dP, 16);
    return LQ_OK;
}

size_t lq_group_workspace_bytes(int64_t R, int64_t C, int axis, int64_t gs) {
    (void)R; (void)C; (void)axis; (void)gs;
    return 0;      // every form is single-stage (lq_group.hpp)
}

int lq_fq_forward_group(const float* P, const float* s, float* out, void* q, int q_dtype, int32_t qmin, int32_t qmax, int rounding,
                        int64_t R, int64_t C, int axis, int64_t gs, void* stream) {
    GroupParams p;
    bool vec;
    const int rc = group_forward_setup(__func__, P, s, false, nullptr, out, q, q_dtype, qmin, qmax, rounding, R, C, axis, gs, p, vec);
    return rc ? rc : launch_group<false>(p, axis, vec, rounding, stream);
}

int lq_fq_backward_group(const float* P, const float* s, const float* dy, int32_t qmin, int32_t qmax, int rounding, float grad_scale,
                         float* dP, float* ds, uint32_t* clipped, void* ws, size_t ws_bytes, int64_t R, int64_t C, int axis,
                         int64_t gs, void* stream) {
    (void)ws; (void)ws_bytes;      // lq_group_workspace_bytes() == 0: ws may be NULL and is never touched
    GroupParams p;
    bool vec;
    const int rc = group_backward_setup(__func__, P, s, false, nullptr, dy, qmin, qmax, rounding, grad_scale, dP, ds, nullptr, clipped,
                                        R, C, axis, gs, p, vec);
    return rc ? rc : launch_group<true>(p, axis, vec, rounding, stream);
}

int lq_fq_forward_group_affine(const float* P, const float* s, const float* b, float* out, void* q, int q_dtype, int32_t qmin,
                               int32_t qmax, int rounding, int64_t R, int64_t C, int axis, int64_t gs, void* stream) {
    GroupAffineParams ap{};
    bool vec;
    const int rc = group_forward_setup(__func__, P, s, true, b, out, q, q_dtype, qmin, qmax, rounding, R, C, axis, gs, ap.g, vec);
    ap.b = b;
    return rc ? rc : launch_group<false>(ap, axis, vec, rounding, stream);
}

int lq_fq_backward_group_affine(const float* P, const float* s, const float* b, const float* dy, int32_t qmin, int32_t qmax,
                                int rounding, float grad_scale, float offset_grad_scale, float* dP, float* ds, float* db,
                                uint32_t* clipped, void* ws, size_t ws_bytes, int64_t R, int64_t C, int axis, int64_t gs,
                                void* stream) {
    (void)ws; (void)ws_bytes;      // lq_group_workspace_bytes() == 0: ws may be NULL and is never touched
    GroupAffineParams ap{};
    bool vec;
    const int rc = group_backward_setup(__func__, P, s, true, b, dy, qmin, qmax, rounding, grad_scale, dP, ds, db, clipped, R, C, axis,
                                        gs, ap.g, vec);
    ap.b = b;
    ap.db = db;
    ap.kb = offset_grad_scale;
    return rc ? rc : launch_group<true>(ap, axis, vec, rounding, stream);
}

// ---- scale initialisation (lq_scale_init.hpp) ----
static int check_init_min_value(const char* fn, float min_value) {
    if (!(min_value > 0.0f) || !(min_value <= 3.4028234663852886e+38f)) return fail(LQ_EINVAL, "%s: min_value %g is not a positive finite number", fn, (double)min_value);
    return LQ_OK;
}

// the fields every method reads; lo / hi / sqrt_qp or n / c / b are the caller's
static InitParams init_params(const GroupParams& gp, float* s, float min_value) {
    InitParams ip{};
    ip.P = gp.P;
    ip.s = s;
    ip.min_value = min_value;
    ip.R = gp.R;
    ip.C = gp.C;
    ip.gs = gp.gs;
    ip.nb = gp.nb;
    return ip;
}

int lq_scale_init_group(const float* P, float* s, int32_t qmin, int32_t qmax, int rounding, int method, float min_value,
                        int64_t R, int64_t C, int axis, int64_t gs, void* stream) {
    const char* fn = __func__;
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if ((rc = check_clip_range(fn, qmin, qmax))) return rc;
    if ((rc = check_rounding(fn, rounding))) return rc;
    if (method != LQ_INIT_ABSMAX && method != LQ_INIT_LSQ && method != LQ_INIT_MSE) return fail(LQ_EINVAL, "%s: bad method %d", fn, method);
    if ((rc = check_init_min_value(fn, min_value))) return rc;
    const GroupParams gp = group_params(P, s, qmin, qmax, R, C, axis, gs);
    InitParams ip = init_params(gp, s, min_value);
    ip.lo = gp.lo;
    ip.hi = gp.hi;
    ip.sqrt_qp = sqrt((double)(qmax > 0 ? qmax : -(int64_t)qmin));
    const bool vec = group_vec_ok(gp, axis) && aligned(P, 16);
    if (method == LQ_INIT_ABSMAX) return launch_scale_init<LQ_INIT_ABSMAX, false>(ip, gp, axis, vec, "scale-init", stream);
    if (method == LQ_INIT_LSQ) return launch_scale_init<LQ_INIT_LSQ, false>(ip, gp, axis, vec, "scale-init", stream);
    if (rounding == LQ_ROUND_NEAREST_EVEN) return launch_scale_init<LQ_INIT_MSE, true>(ip, gp, axis, vec, "scale-init", stream);
    return launch_scale_init<LQ_INIT_MSE, false>(ip, gp, axis, vec, "scale-init", stream);
}

int lq_scale_init_group_minmax(const float* P, float* s, float* b, int32_t qmin, int32_t qmax, int rounding, float min_value,
                               int64_t R, int64_t C, int axis, int64_t gs, void* stream) {
    const char* fn = __func__;
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    LQ_REQUIRE_PTR_FN(fn, b);
    constexpr int32_t kLim = 1 << 22;      // c = (qmin + qmax) / 2 (+ 1/2) and n = qmax - qmin are exact floats
    if (qmin >= qmax) return fail(LQ_EINVAL, "%s: min-max needs qmax > qmin (got [%d, %d])", fn, (int)qmin, (int)qmax);
    if (qmin < -kLim || qmax > kLim) return fail(LQ_EINVAL, "%s: range [%d, %d] is outside +-2^22", fn, (int)qmin, (int)qmax);
    if ((rc = check_rounding(fn, rounding))) return rc;
    if ((rc = check_init_min_value(fn, min_value))) return rc;
    const GroupParams gp = group_params(P, s, qmin, qmax, R, C, axis, gs);
    InitParams ip = init_params(gp, s, min_value);
    ip.n = (float)((int64_t)qmax - (int64_t)qmin);
    ip.c = (float)(((double)qmin + (double)qmax) * 0.5 + (rounding == LQ_ROUND_FLOOR ? 0.5 : 0.0));
    ip.b = b;
    const bool vec = group_vec_ok(gp, axis) && aligned(P, 16);
    return launch_scale_init<kInitMinMax, false>(ip, gp, axis, vec, "min-max", stream);
}

// ---- OCP microscaling element formats under a power-of-two (or fp32) scale per group (lq_mx.hpp) ----
struct MxFormat {
    int32_t bits, M, emin, emax;
    float mx;
    uint32_t mm_frac;      // fraction bits of mx / 2^emax
};
static const MxFormat kMxFormats[] = {
    {4, 1, 0, 2, 6.0f, 0x400000u},            // LQ_ELEM_FP4_E2M1
    {6, 3, 0, 2, 7.5f, 0x700000u},            // LQ_ELEM_FP6_E2M3
    {6, 2, -2, 4, 28.0f, 0x600000u},          // LQ_ELEM_FP6_E3M2
    {8, 3, -6, 8, 448.0f, 0x600000u},         // LQ_ELEM_FP8_E4M3
    {8, 2, -14, 15, 57344.0f, 0x600000u},     // LQ_ELEM_FP8_E5M2
};

static int check_mx(const char* fn, int format, int scale_format) {
    if (format < LQ_ELEM_FP4_E2M1 || format > LQ_ELEM_FP8_E5M2) return fail(LQ_EINVAL, "%s: bad element format %d", fn, format);
    if (scale_format != LQ_SCALE_E8M0 && scale_format != LQ_SCALE_FP32) return fail(LQ_EINVAL, "%s: bad scale format %d", fn, scale_format);
    return LQ_OK;
}

static void mx_fill(GroupMxParams& mp, int format, int scale_format) {
    const MxFormat& f = kMxFormats[format];
    mp.g.lo = -f.mx;
    mp.g.hi = f.mx;
    mp.M = f.M;
    mp.emin = f.emin;
    mp.bits = f.bits;
    mp.e8m0_mask = scale_format == LQ_SCALE_E8M0 ? ~0u : 0u;
}

int lq_fq_forward_mx(const float* P, const float* s, float* out, void* code, int code_dtype, int format, int scale_format,
                     int64_t R, int64_t C, int axis, int64_t gs, void* stream) {
    GroupMxParams mp{};
    bool vec;
    int rc = group_forward_setup(__func__, P, s, false, nullptr, out, code, code_dtype, 0, 0, LQ_ROUND_NEAREST_EVEN, R, C, axis, gs, mp.g, vec);
    if (rc || (rc = check_mx(__func__, format, scale_format))) return rc;
    mx_fill(mp, format, scale_format);
    return launch_group<false>(mp, axis, vec, LQ_ROUND_NEAREST_EVEN, stream);
}

int lq_fq_backward_mx(const float* P, const float* s, const float* dy, int format, int scale_format, float grad_scale, float* dP,
                      float* ds, uint32_t* clipped, int64_t R, int64_t C, int axis, int64_t gs, void* stream) {
    GroupMxParams mp{};
    bool vec;
    int rc = group_backward_setup(__func__, P, s, false, nullptr, dy, 0, 0, LQ_ROUND_NEAREST_EVEN, grad_scale, dP, ds, nullptr, clipped,
                                  R, C, axis, gs, mp.g, vec);
    if (rc || (rc = check_mx(__func__, format, scale_format))) return rc;
    mx_fill(mp, format, scale_format);
    return launch_group<true>(mp, axis, vec, LQ_ROUND_NEAREST_EVEN, stream);
}

int lq_scale_init_mx(const float* P, float* s, int format, int method, float min_value, int64_t R, int64_t C, int axis, int64_t gs,
                     void* stream) {
    const char* fn = __func__;
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if ((rc = check_mx(fn, format, LQ_SCALE_E8M0))) return rc;
    if (method != LQ_MX_INIT_OCP && method != LQ_MX_INIT_COVER) return fail(LQ_EINVAL, "%s: bad method %d", fn, method);
    if ((rc = check_init_min_value(fn, min_value))) return rc;
    const GroupParams gp = group_params(P, s, 0, 0, R, C, axis, gs);
    InitParams ip = init_params(gp, s, min_value);
    ip.emax = kMxFormats[format].emax;
    ip.mm_frac = kMxFormats[format].mm_frac;
    const bool vec = group_vec_ok(gp, axis) && aligned(P, 16);
    if (method == LQ_MX_INIT_OCP) return launch_scale_init<kInitMxOcp, false>(ip, gp, axis, vec, "microscaling scale-init", stream);
    return launch_scale_init<kInitMxCover, false>(ip, gp, axis, vec, "microscaling scale-init", stream);
}

// ---- per-group statistics (lq_group_stats.hpp, lq_mx_stats.hpp) ----
// The output pointers of both entry points; `flushed` is checked where the quantizer has the third count
static int check_stats_outputs(const char* fn, const uint32_t* below, const uint32_t* above, bool has_flushed, const uint32_t* flushed,
                               const double* err2, const double* sig2, const uint32_t* hist) {
    LQ_REQUIRE_PTR_FN(fn, below);
    LQ_REQUIRE_PTR_FN(fn, above);
    if (has_flushed) LQ_REQUIRE_PTR_FN(fn, flushed);
    if (!err2 || !sig2) return fail(LQ_EINVAL, "%s: argument '%s' is NULL", fn, err2 ? "sig2" : "err2");
    if (!aligned(err2, 8) || !aligned(sig2, 8)) return fail(LQ_EALIGN, "%s: err2 and sig2 must be 8-byte aligned", fn);
    if (hist && !aligned(hist, 4)) return fail(LQ_EALIGN, "%s: hist is not 4-byte aligned", fn);
    return LQ_OK;
}

// Both launch in the backward's shape (group_launch without a row split) with the block's histogram, nbins words, in dynamic LDS
int lq_group_stats(const float* P, const float* s, const float* b, int32_t qmin, int32_t qmax, int rounding, uint32_t* below,
                   uint32_t* above, double* err2, double* sig2, uint32_t* hist, int64_t R, int64_t C, int axis, int64_t gs,
                   void* stream) {
    const char* fn = __func__;
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if (b && !aligned(b, 4)) return fail(LQ_EALIGN, "%s: b is not 4-byte aligned", fn);
    if ((rc = check_stats_outputs(fn, below, above, false, nullptr, err2, sig2, hist))) return rc;
    if ((rc = check_clip_range(fn, qmin, qmax))) return rc;
    if ((rc = check_rounding(fn, rounding))) return rc;
    const int64_t codes = (int64_t)qmax - (int64_t)qmin + 1;
    if (hist && codes > kStatsMaxBins)
        return fail(LQ_EINVAL, "%s: a histogram of %lld codes exceeds the limit of %d (pass hist = NULL)", fn, (long long)codes, kStatsMaxBins);
    const GroupParams gp = group_params(P, s, qmin, qmax, R, C, axis, gs);
    StatsParams sp{};
    sp.P = P;
    sp.s = s;
    sp.b = b;
    sp.lo = gp.lo;
    sp.hi = gp.hi;
    sp.qmin = qmin;
    sp.nbins = hist ? (int32_t)codes : 0;
    sp.below = below;
    sp.above = above;
    sp.err2 = err2;
    sp.sig2 = sig2;
    sp.hist = hist;
    sp.R = gp.R;
    sp.C = gp.C;
    sp.gs = gp.gs;
    sp.nb = gp.nb;
    const bool vec = group_vec_ok(gp, axis) && aligned(P, 16);
    const GroupLaunch L = group_launch(gp, axis, vec, false, kGroupGridY);
    const size_t lds = (size_t)sp.nbins * sizeof(uint32_t);
    hipStream_t st = (hipStream_t)stream;
    const char* family = "group statistics";
    const bool rne = rounding == LQ_ROUND_NEAREST_EVEN;
    if (b && rne) return launch_group_form(L, LQ_GROUP_FAMILY(k_stats_cols, k_stats_rows, true, true), sp, family, st, lds);
    if (b) return launch_group_form(L, LQ_GROUP_FAMILY(k_stats_cols, k_stats_rows, false, true), sp, family, st, lds);
    if (rne) return launch_group_form(L, LQ_GROUP_FAMILY(k_stats_cols, k_stats_rows, true, false), sp, family, st, lds);
    return launch_group_form(L, LQ_GROUP_FAMILY(k_stats_cols, k_stats_rows, false, false), sp, family, st, lds);
}

int lq_mx_stats(const float* P, const float* s, int format, int scale_format, uint32_t* below, uint32_t* above, uint32_t* flushed,
                double* err2, double* sig2, uint32_t* hist, int64_t R, int64_t C, int axis, int64_t gs, void* stream) {
    const char* fn = __func__;
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if ((rc = check_stats_outputs(fn, below, above, true, flushed, err2, sig2, hist))) return rc;
    if ((rc = check_mx(fn, format, scale_format))) return rc;
    MxStatsParams sp{};
    sp.mp.g = group_params(P, s, 0, 0, R, C, axis, gs);
    mx_fill(sp.mp, format, scale_format);
    sp.below = below;
    sp.above = above;
    sp.flushed = flushed;
    sp.err2 = err2;
    sp.sig2 = sig2;
    sp.hist = hist;
    sp.nbins = hist ? (int32_t)1 << sp.mp.bits : 0;
    const bool vec = group_vec_ok(sp.mp.g, axis) && aligned(P, 16);
    const GroupLaunch L = group_launch(sp.mp.g, axis, vec, false, kGroupGridY);
    return launch_group_form(L, LQ_GROUP_FAMILY0(k_mx_stats_cols, k_mx_stats_rows), sp, "microscaling statistics", (hipStream_t)stream,
                             (size_t)sp.nbins * sizeof(uint32_t));
}

// ---- the matrix path: what the MX and the int8 family share on the host ----
// 2^-126, the floor of every scale an operand quantizer takes from its data: the smallest an E8M0 byte of s_eff can hold
constexpr float kOperandMinScale = 1.17549435082228750797e-38f;
// what the GEMMs read the scales as: an MX operand's bytes as words, an int8 operand's floats as float4
constexpr int kMxScaleAlign = 4, kI8ScaleAlign = 16;

static int check_operand_buffers(const char* fn, const void* codes, const void* scales, int scale_align) {
    if (!codes || !scales) return fail(LQ_EINVAL, "%s: argument '%s' is NULL", fn, codes ? "scales" : "codes");
    if (!aligned(codes, 16)) return fail(LQ_EALIGN, "%s: codes is not 16-byte aligned", fn);
    if (!aligned(scales, scale_align)) return fail(LQ_EALIGN, "%s: scales is not %d-byte aligned", fn, scale_align);
    return LQ_OK;
}

static int check_gemm_bias(const char* fn, const float* bias) {
    return bias && !aligned(bias, 4) ? fail(LQ_EALIGN, "%s: bias is not 4-byte aligned", fn) : LQ_OK;
}

// Y (M, N) in fp32 with leading dimension ldy, and the optional bias
static int check_gemm_output(const char* fn, const float* bias, const float* Y, int64_t ldy, int64_t M, int64_t N) {
    LQ_REQUIRE_PTR_FN(fn, Y);
    if (int rc = check_gemm_bias(fn, bias)) return rc;
    if (ldy < N) return fail(LQ_EINVAL, "%s: ldy = %lld is below N = %lld", fn, (long long)ldy, (long long)N);
    if ((double)M * (double)ldy >= 9.0e15) return fail(LQ_EINVAL, "%s: Y is too large", fn);
    return LQ_OK;
}

// a thread block is 4 x 4 tiles, 64 x 64 of Y: gx blocks along n, the MT tiles of 16 lines along m in grid.y, which takes 65535
static int gemm_grid(const char* fn, int64_t gx, int64_t MT, int64_t M, dim3& grid) {
    const int64_t gy = (MT + 3) / 4;
    if (gy > 65535) return fail(LQ_EINVAL, "%s: M = %lld is above 65535 * 64", fn, (long long)M);
    grid = dim3((unsigned)gx, (unsigned)gy);
    return LQ_OK;
}

// ---- packed MX operands and the block-scaled GEMM (lq_mx_operand.hpp, lq_mx_gemm.hpp) ----
// the three element formats whose fragments are built: the 6-bit formats need a 96-byte fragment packing of their own
static int check_mx_operand_format(const char* fn, int format) {
    if (format == LQ_ELEM_FP6_E2M3 || format == LQ_ELEM_FP6_E3M2)
        return fail(LQ_EINVAL, "%s: fp6 operands are not supported (element format %d): 6-bit lanes need their own fragment packing", fn, format);
    if (format != LQ_ELEM_FP4_E2M1 && format != LQ_ELEM_FP8_E4M3 && format != LQ_ELEM_FP8_E5M2)
        return fail(LQ_EINVAL, "%s: bad element format %d", fn, format);
    return LQ_OK;
}

struct MxOperandDims {
    int64_t LT, KT, KG, fb;
    size_t code_bytes, scale_bytes;
};

static int mx_operand_dims(const char* fn, int format, int64_t L, int64_t K, MxOperandDims& d) {
    int rc = check_mx_operand_format(fn, format);
    if (rc) return rc;
    if (L <= 0 || K <= 0) return fail(LQ_EINVAL, "%s: extents must be positive (L=%lld K=%lld)", fn, (long long)L, (long long)K);
    if ((double)L * (double)K >= 2147483648.0) return fail(LQ_EINVAL, "%s: L * K = %lld * %lld is not below 2^31", fn, (long long)L, (long long)K);
    d.LT = (L + kMxTileLines - 1) / kMxTileLines;
    d.KT = (K + kMxTileK - 1) / kMxTileK;
    d.KG = (d.KT + 3) / 4;
    d.fb = format == LQ_ELEM_FP4_E2M1 ? 16 : 32;
    d.code_bytes = (size_t)(d.LT * d.KT * 64 * d.fb);
    d.scale_bytes = (size_t)(d.LT * d.KG * 256);
    return LQ_OK;
}

int lq_mx_operand_bytes(int format, int64_t L, int64_t K, size_t* code_bytes, size_t* scale_bytes) {
    const char* fn = __func__;
    if (!code_bytes || !scale_bytes) return fail(LQ_EINVAL, "%s: code_bytes or scale_bytes is NULL", fn);
    MxOperandDims d;
    int rc = mx_operand_dims(fn, format, L, K, d);
    if (rc) return rc;
    *code_bytes = d.code_bytes;
    *scale_bytes = d.scale_bytes;
    return LQ_OK;
}

extern "C++" {      // templates inside the C-linkage block
template <bool DYN, int METHOD, bool LINE_FAST>
static int launch_mx_operand(const MxOperandParams& op, bool fp4, bool vec, const char* what, void* stream) {
    const int64_t threads = (int64_t)op.LT * kMxTileLines * op.KT * 4;
    const dim3 grid((unsigned)((threads + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    constexpr bool kVecForm = !LINE_FAST;      // float4 loads need the blocks along the contiguous axis: axis 1 and quantize
    if (fp4) {
        if (kVecForm && vec) hipLaunchKernelGGL((k_mx_operand<DYN, METHOD, true, kVecForm, LINE_FAST>), grid, block, 0, st, op);
        else hipLaunchKernelGGL((k_mx_operand<DYN, METHOD, true, false, LINE_FAST>), grid, block, 0, st, op);
    } else {
        if (kVecForm && vec) hipLaunchKernelGGL((k_mx_operand<DYN, METHOD, false, kVecForm, LINE_FAST>), grid, block, 0, st, op);
        else hipLaunchKernelGGL((k_mx_operand<DYN, METHOD, false, false, LINE_FAST>), grid, block, 0, st, op);
    }
    return check_hip(what);
}

template <int FA>
static void launch_mx_gemm_b(const MxGemmParams& p, int b_format, dim3 grid, hipStream_t st) {
    if (b_format == LQ_ELEM_FP4_E2M1) hipLaunchKernelGGL((k_mx_gemm<FA, LQ_ELEM_FP4_E2M1>), grid, dim3(kBlock), 0, st, p);
    else if (b_format == LQ_ELEM_FP8_E4M3) hipLaunchKernelGGL((k_mx_gemm<FA, LQ_ELEM_FP8_E4M3>), grid, dim3(kBlock), 0, st, p);
    else hipLaunchKernelGGL((k_mx_gemm<FA, LQ_ELEM_FP8_E5M2>), grid, dim3(kBlock), 0, st, p);
}

// 3 x 3 x 2 instantiations: the input formats are immediates of the instruction, of the output format only the width is compile-time
template <int FA, int FB>
static void launch_mx_gemm_quantize_o(const MxGemmQuantParams& p, bool out_fp4, dim3 grid, hipStream_t st) {
    if (out_fp4) hipLaunchKernelGGL((k_mx_gemm_quantize<FA, FB, true>), grid, dim3(kBlock), 0, st, p);
    else hipLaunchKernelGGL((k_mx_gemm_quantize<FA, FB, false>), grid, dim3(kBlock), 0, st, p);
}
template <int FA>
static void launch_mx_gemm_quantize_b(const MxGemmQuantParams& p, int b_format, bool out_fp4, dim3 grid, hipStream_t st) {
    if (b_format == LQ_ELEM_FP4_E2M1) launch_mx_gemm_quantize_o<FA, LQ_ELEM_FP4_E2M1>(p, out_fp4, grid, st);
    else if (b_format == LQ_ELEM_FP8_E4M3) launch_mx_gemm_quantize_o<FA, LQ_ELEM_FP8_E4M3>(p, out_fp4, grid, st);
    else launch_mx_gemm_quantize_o<FA, LQ_ELEM_FP8_E5M2>(p, out_fp4, grid, st);
}
}  // extern "C++"

static void mx_operand_fill(MxOperandParams& op, const MxOperandDims& d, int format, int64_t L, int64_t K, void* codes, void* scales) {
    mx_fill(op.mp, format, LQ_SCALE_E8M0);
    op.codes = (uint8_t*)codes;
    op.scales = (uint8_t*)scales;
    op.L = (int32_t)L;
    op.K = (int32_t)K;
    op.nbk = (int32_t)((K + kMxBlockLen - 1) / kMxBlockLen);
    op.LT = (int32_t)d.LT;
    op.KT = (int32_t)d.KT;
    op.KG = (int32_t)d.KG;
}

int lq_mx_operand_pack(const float* P, const float* s, int format, int scale_format, int64_t R, int64_t C, int axis, int64_t gs,
                       void* codes, void* scales, void* stream) {
    const char* fn = __func__;
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if ((rc = check_mx(fn, format, scale_format))) return rc;
    if (scale_format != LQ_SCALE_E8M0)
        return fail(LQ_EINVAL, "%s: fp32 scales cannot be packed: the block-scaled matrix instruction takes E8M0 scales only", fn);
    if (gs != kMxBlockLen) return fail(LQ_EINVAL, "%s: group size %lld: the instruction's block is %d", fn, (long long)gs, kMxBlockLen);
    const int64_t L = axis == 0 ? C : R, K = axis == 0 ? R : C;
    MxOperandDims d;
    if ((rc = mx_operand_dims(fn, format, L, K, d))) return rc;
    if ((rc = check_operand_buffers(fn, codes, scales, kMxScaleAlign))) return rc;
    MxOperandParams op{};
    mx_operand_fill(op, d, format, L, K, codes, scales);
    op.mp.g.P = P;
    op.mp.g.s = s;
    op.line_stride = axis == 0 ? 1 : C;
    op.k_stride = axis == 0 ? C : 1;
    op.s_line_stride = axis == 0 ? 1 : op.nbk;      // [nb][C] | [R][nb]
    op.s_blk_stride = axis == 0 ? C : 1;
    const bool fp4 = format == LQ_ELEM_FP4_E2M1;
    if (axis == 0) return launch_mx_operand<false, kInitMxOcp, true>(op, fp4, false, "microscaling operand pack", stream);
    return launch_mx_operand<false, kInitMxOcp, false>(op, fp4, C % 4 == 0 && aligned(P, 16), "microscaling operand pack", stream);
}

int lq_mx_operand_quantize(const float* X, int format, int method, int64_t M, int64_t K, void* codes, void* scales, void* stream) {
    const char* fn = __func__;
    LQ_REQUIRE_PTR_FN(fn, X);
    if (method != LQ_MX_INIT_OCP && method != LQ_MX_INIT_COVER) return fail(LQ_EINVAL, "%s: bad method %d", fn, method);
    MxOperandDims d;
    int rc = mx_operand_dims(fn, format, M, K, d);
    if (rc) return rc;
    if ((rc = check_operand_buffers(fn, codes, scales, kMxScaleAlign))) return rc;
    MxOperandParams op{};
    mx_operand_fill(op, d, format, M, K, codes, scales);
    op.mp.g.P = X;
    op.line_stride = K;
    op.k_stride = 1;
    op.ip.emax = kMxFormats[format].emax;
    op.ip.mm_frac = kMxFormats[format].mm_frac;
    op.ip.min_value = kOperandMinScale;
    const bool fp4 = format == LQ_ELEM_FP4_E2M1;
    const bool vec = K % 4 == 0 && aligned(X, 16);
    if (method == LQ_MX_INIT_OCP) return launch_mx_operand<true, kInitMxOcp, false>(op, fp4, vec, "microscaling operand quantize", stream);
    return launch_mx_operand<true, kInitMxCover, false>(op, fp4, vec, "microscaling operand quantize", stream);
}

int lq_mx_operand_decode(const void* codes, const void* scales, int format, int64_t L, int64_t K, float* out, void* stream) {
    const char* fn = __func__;
    MxOperandDims d;
    int rc = mx_operand_dims(fn, format, L, K, d);
    if (rc) return rc;
    if ((rc = check_operand_buffers(fn, codes, scales, kMxScaleAlign))) return rc;
    LQ_REQUIRE_PTR_FN(fn, out);
    MxDecodeParams dp{};
    dp.codes = (const uint8_t*)codes;
    dp.scales = (const uint8_t*)scales;
    dp.out = out;
    dp.L = (int32_t)L;
    dp.K = (int32_t)K;
    dp.KT = (int32_t)d.KT;
    dp.KG = (int32_t)d.KG;
    dp.M = kMxFormats[format].M;
    dp.emin = kMxFormats[format].emin;
    dp.bits = kMxFormats[format].bits;
    const int64_t n = L * K;
    hipLaunchKernelGGL(k_mx_operand_decode, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, dp);
    return check_hip("microscaling operand decode");
}

int lq_mx_gemm(const void* a_codes, const void* a_scales, int a_format, const void* b_codes, const void* b_scales, int b_format,
               const float* bias, float* Y, int64_t M, int64_t N, int64_t K, int64_t ldy, void* stream) {
    const char* fn = __func__;
    MxOperandDims da, db;
    int rc = mx_operand_dims(fn, a_format, M, K, da);
    if (rc || (rc = mx_operand_dims(fn, b_format, N, K, db))) return rc;
    if ((rc = check_operand_buffers(fn, a_codes, a_scales, kMxScaleAlign))) return rc;
    if ((rc = check_operand_buffers(fn, b_codes, b_scales, kMxScaleAlign))) return rc;
    if ((rc = check_gemm_output(fn, bias, Y, ldy, M, N))) return rc;
    MxGemmParams p{};
    p.a_codes = (const uint8_t*)a_codes;
    p.a_scales = (const uint8_t*)a_scales;
    p.b_codes = (const uint8_t*)b_codes;
    p.b_scales = (const uint8_t*)b_scales;
    p.bias = bias;
    p.Y = Y;
    p.ldy = ldy;
    p.M = (int32_t)M;
    p.N = (int32_t)N;
    p.MT = (int32_t)da.LT;
    p.NT = (int32_t)db.LT;
    p.KT = (int32_t)da.KT;
    p.KG = (int32_t)da.KG;
    dim3 grid;
    if ((rc = gemm_grid(fn, (db.LT + 3) / 4, da.LT, M, grid))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a_format == LQ_ELEM_FP4_E2M1) launch_mx_gemm_b<LQ_ELEM_FP4_E2M1>(p, b_format, grid, st);
    else if (a_format == LQ_ELEM_FP8_E4M3) launch_mx_gemm_b<LQ_ELEM_FP8_E4M3>(p, b_format, grid, st);
    else launch_mx_gemm_b<LQ_ELEM_FP8_E5M2>(p, b_format, grid, st);
    return check_hip("microscaling GEMM");
}

int lq_mx_gemm_quantize(const void* a_codes, const void* a_scales, int a_format, const void* b_codes, const void* b_scales, int b_format,
                        const float* bias, int activation, int out_format, int method, void* out_codes, void* out_scales, int64_t M,
                        int64_t N, int64_t K, void* stream) {
    const char* fn = __func__;
    MxOperandDims da, db, dout;
    int rc = mx_operand_dims(fn, a_format, M, K, da);
    if (rc || (rc = mx_operand_dims(fn, b_format, N, K, db)) || (rc = mx_operand_dims(fn, out_format, M, N, dout))) return rc;
    if (method != LQ_MX_INIT_OCP && method != LQ_MX_INIT_COVER) return fail(LQ_EINVAL, "%s: bad method %d", fn, method);
    if (activation != LQ_ACT_NONE && activation != LQ_ACT_RELU) return fail(LQ_EINVAL, "%s: bad activation %d", fn, activation);
    if ((rc = check_operand_buffers(fn, a_codes, a_scales, kMxScaleAlign))) return rc;
    if ((rc = check_operand_buffers(fn, b_codes, b_scales, kMxScaleAlign))) return rc;
    if ((rc = check_operand_buffers(fn, out_codes, out_scales, kMxScaleAlign))) return rc;
    if ((rc = check_gemm_bias(fn, bias))) return rc;
    MxGemmQuantParams p{};
    p.g.a_codes = (const uint8_t*)a_codes;
    p.g.a_scales = (const uint8_t*)a_scales;
    p.g.b_codes = (const uint8_t*)b_codes;
    p.g.b_scales = (const uint8_t*)b_scales;
    p.g.bias = bias;
    p.g.M = (int32_t)M;
    p.g.N = (int32_t)N;
    p.g.MT = (int32_t)da.LT;
    p.g.NT = (int32_t)db.LT;
    p.g.KT = (int32_t)da.KT;
    p.g.KG = (int32_t)da.KG;
    mx_fill(p.mp, out_format, LQ_SCALE_E8M0);
    p.ip.emax = kMxFormats[out_format].emax;
    p.ip.mm_frac = kMxFormats[out_format].mm_frac;
    p.ip.min_value = kOperandMinScale;
    p.codes = (uint8_t*)out_codes;
    p.scales = (uint8_t*)out_scales;
    p.act = activation;
    p.cover = method == LQ_MX_INIT_COVER ? 1 : 0;
    p.OKT = (int32_t)dout.KT;
    p.OKG = (int32_t)dout.KG;
    // along n the grid spans the padded operand, 128 OKT columns, so that its padding is written too
    dim3 grid;
    if ((rc = gemm_grid(fn, 2 * dout.KT, da.LT, M, grid))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool out_fp4 = out_format == LQ_ELEM_FP4_E2M1;
    if (a_format == LQ_ELEM_FP4_E2M1) launch_mx_gemm_quantize_b<LQ_ELEM_FP4_E2M1>(p, b_format, out_fp4, grid, st);
    else if (a_format == LQ_ELEM_FP8_E4M3) launch_mx_gemm_quantize_b<LQ_ELEM_FP8_E4M3>(p, b_format, out_fp4, grid, st);
    else launch_mx_gemm_quantize_b<LQ_ELEM_FP8_E5M2>(p, b_format, out_fp4, grid, st);
    return check_hip("microscaling GEMM with operand-out epilogue");
}

// ---- the operand of a convolution's im2col matrix (lq_mx_conv.hpp) ----
struct ConvDims {
    int64_t M, K, OH, OW;
};

// the geometry alone: what lq_mx_im2col_dims answers.  M and K are formed in double first, so that no int64 product overflows
static int conv_geom_dims(const char* fn, const lq_conv_geom* g, ConvDims& d) {
    if (!g) return fail(LQ_EINVAL, "%s: argument 'g' is NULL", fn);
    if (g->B <= 0 || g->C <= 0 || g->H <= 0 || g->W <= 0)
        return fail(LQ_EINVAL, "%s: extents must be positive (B=%lld C=%lld H=%lld W=%lld)", fn, (long long)g->B, (long long)g->C,
                    (long long)g->H, (long long)g->W);
    if (g->KH <= 0 || g->KW <= 0) return fail(LQ_EINVAL, "%s: kernel size must be positive (KH=%d KW=%d)", fn, g->KH, g->KW);
    if (g->stride_h <= 0 || g->stride_w <= 0)
        return fail(LQ_EINVAL, "%s: strides must be positive (stride_h=%d stride_w=%d)", fn, g->stride_h, g->stride_w);
    if (g->pad_top < 0 || g->pad_left < 0 || g->pad_bottom < 0 || g->pad_right < 0)
        return fail(LQ_EINVAL, "%s: padding must not be negative (top=%d left=%d bottom=%d right=%d)", fn, g->pad_top, g->pad_left,
                    g->pad_bottom, g->pad_right);
    if (g->H > (INT64_MAX >> 1) || g->W > (INT64_MAX >> 1))
        return fail(LQ_EINVAL, "%s: H=%lld or W=%lld does not leave room for the padding", fn, (long long)g->H, (long long)g->W);
    const int64_t span_h = g->H + g->pad_top + g->pad_bottom - g->KH, span_w = g->W + g->pad_left + g->pad_right - g->KW;
    d.OH = span_h < 0 ? 0 : span_h / g->stride_h + 1;
    d.OW = span_w < 0 ? 0 : span_w / g->stride_w + 1;
    if (d.OH < 1 || d.OW < 1)
        return fail(LQ_EINVAL, "%s: the kernel does not fit the padded input (OH=%lld OW=%lld)", fn, (long long)d.OH, (long long)d.OW);
    const double m = (double)g->B * (double)d.OH * (double)d.OW, k = (double)g->C * (double)g->KH * (double)g->KW;
    if (m >= 4611686018427387904.0 || k >= 4611686018427387904.0)
        return fail(LQ_EINVAL, "%s: M = B * OH * OW or K = C * KH * KW is not below 2^62", fn);
    d.M = g->B * d.OH * d.OW;
    d.K = g->C * g->KH * g->KW;
    return LQ_OK;
}

int lq_mx_im2col_dims(const lq_conv_geom* g, int64_t* M, int64_t* K, int64_t* OH, int64_t* OW) {
    const char* fn = __func__;
    if (!M || !K || !OH || !OW) return fail(LQ_EINVAL, "%s: argument '%s' is NULL", fn, !M ? "M" : !K ? "K" : !OH ? "OH" : "OW");
    ConvDims d;
    int rc = conv_geom_dims(fn, g, d);
    if (rc) return rc;
    *M = d.M;
    *K = d.K;
    *OH = d.OH;
    *OW = d.OW;
    return LQ_OK;
}

// the geometry with the strides of X, as both im2col operands take it
static int conv_geom_dims_strided(const char* fn, const lq_conv_geom* g, ConvDims& d) {
    int rc = conv_geom_dims(fn, g, d);
    if (rc) return rc;
    if (g->xs_b < 0 || g->xs_c < 0 || g->xs_h < 0 || g->xs_w < 0)
        return fail(LQ_EINVAL, "%s: strides of X must not be negative (xs_b=%lld xs_c=%lld xs_h=%lld xs_w=%lld)", fn, (long long)g->xs_b,
                    (long long)g->xs_c, (long long)g->xs_h, (long long)g->xs_w);
    return LQ_OK;
}

// all of the device's geometry but `chunks`, which is the kernel's own cut of its grid.  Call once M * K < 2^31 is known: that
// bounds OH * OW, OW, KH * KW and KW, so every divisor and dividend is a 32-bit number
static void fill_im2col_geom(Im2colGeom& ig, const lq_conv_geom* g, const ConvDims& cd) {
    ig.xs_b = g->xs_b;
    ig.xs_c = g->xs_c;
    ig.xs_h = g->xs_h;
    ig.xs_w = g->xs_w;
    ig.H = g->H;
    ig.W = g->W;
    ig.ohow = make_fastdiv((uint32_t)(cd.OH * cd.OW));
    ig.ow = make_fastdiv((uint32_t)cd.OW);
    ig.khkw = make_fastdiv((uint32_t)((int64_t)g->KH * g->KW));
    ig.kw = make_fastdiv((uint32_t)g->KW);
    ig.KH = g->KH;
    ig.stride_h = g->stride_h;
    ig.stride_w = g->stride_w;
    ig.pad_top = g->pad_top;
    ig.pad_left = g->pad_left;
    ig.M = (int32_t)cd.M;
}

int lq_mx_operand_im2col(const float* X, const lq_conv_geom* g, int format, int method, void* codes, void* scales, void* stream) {
    const char* fn = __func__;
    LQ_REQUIRE_PTR_FN(fn, X);
    if (method != LQ_MX_INIT_OCP && method != LQ_MX_INIT_COVER) return fail(LQ_EINVAL, "%s: bad method %d", fn, method);
    ConvDims cd;
    int rc = conv_geom_dims_strided(fn, g, cd);
    if (rc) return rc;
    MxOperandDims d;
    if ((rc = mx_operand_dims(fn, format, cd.M, cd.K, d))) return rc;      // the format, M * K < 2^31
    if ((rc = check_operand_buffers(fn, codes, scales, kMxScaleAlign))) return rc;
    MxIm2colParams op{};
    mx_fill(op.mp, format, LQ_SCALE_E8M0);
    op.mp.g.P = X;
    op.ip.emax = kMxFormats[format].emax;
    op.ip.mm_frac = kMxFormats[format].mm_frac;
    op.ip.min_value = kOperandMinScale;
    op.codes = (uint8_t*)codes;
    op.scales = (uint8_t*)scales;
    fill_im2col_geom(op.geom, g, cd);
    op.K = (int32_t)cd.K;
    op.nbk = (int32_t)((cd.K + kMxBlockLen - 1) / kMxBlockLen);
    op.LT = (int32_t)d.LT;
    op.KT = (int32_t)d.KT;
    op.KG = (int32_t)d.KG;
    // a thread block is kBlock consecutive lines of one k block: chunks per k block, k blocks slowest
    const int64_t chunks = (d.LT * kMxTileLines + kBlock - 1) / kBlock;
    op.geom.chunks = make_fastdiv((uint32_t)chunks);
    const dim3 grid((unsigned)(chunks * d.KT * 4)), block(kBlock);     // below 2^31: at most M K / 8192 + M / 64 + K / 32 + 4
    hipStream_t st = (hipStream_t)stream;
    const bool fp4 = format == LQ_ELEM_FP4_E2M1;
    if (method == LQ_MX_INIT_OCP) {
        if (fp4) hipLaunchKernelGGL((k_mx_im2col<kInitMxOcp, true>), grid, block, 0, st, op);
        else hipLaunchKernelGGL((k_mx_im2col<kInitMxOcp, false>), grid, block, 0, st, op);
    } else {
        if (fp4) hipLaunchKernelGGL((k_mx_im2col<kInitMxCover, true>), grid, block, 0, st, op);
        else hipLaunchKernelGGL((k_mx_im2col<kInitMxCover, false>), grid, block, 0, st, op);
    }
    return check_hip("microscaling im2col operand");
}

// ---- packed int8 operands and the int8 GEMM (lq_i8_operand.hpp, lq_i8_gemm.hpp) ----
struct I8OperandDims {
    int64_t LT, KT, nbs;
    size_t code_bytes, scale_bytes;
};

static int i8_operand_dims(const char* fn, int64_t L, int64_t K, int64_t block, I8OperandDims& d) {
    if (L <= 0 || K <= 0) return fail(LQ_EINVAL, "%s: extents must be positive (L=%lld K=%lld)", fn, (long long)L, (long long)K);
    if ((double)L * (double)K >= 2147483648.0 || K > 2147483647 - kI8TileK)
        return fail(LQ_EINVAL, "%s: L * K = %lld * %lld is not below 2^31", fn, (long long)L, (long long)K);
    if (block < 0 || block % kI8TileK != 0 || block > (1 << 30))
        return fail(LQ_EINVAL, "%s: scale block %lld is neither 0 (one scale per line) nor a multiple of %d up to 2^30: a scale "
                    "must not change inside a step of the instruction", fn, (long long)block, kI8TileK);
    d.LT = (L + kI8TileLines - 1) / kI8TileLines;
    d.KT = (K + kI8TileK - 1) / kI8TileK;
    d.nbs = block ? (K + block - 1) / block : 1;
    d.code_bytes = (size_t)(d.LT * d.KT * 1024);
    d.scale_bytes = (size_t)(d.nbs * d.LT * kI8TileLines * 4);
    return LQ_OK;
}

int lq_i8_operand_bytes(int64_t L, int64_t K, int64_t block, size_t* code_bytes, size_t* scale_bytes) {
    const char* fn = __func__;
    if (!code_bytes || !scale_bytes) return fail(LQ_EINVAL, "%s: code_bytes or scale_bytes is NULL", fn);
    I8OperandDims d;
    int rc = i8_operand_dims(fn, L, K, block, d);
    if (rc) return rc;
    *code_bytes = d.code_bytes;
    *scale_bytes = d.scale_bytes;
    return LQ_OK;
}

// an operand's offsets (the affine entry points): a buffer in the layout of its scales, on the same grid
static int check_operand_offsets(const char* fn, const void* offsets) {
    if (!offsets) return fail(LQ_EINVAL, "%s: argument 'offsets' is NULL", fn);
    if (!aligned(offsets, kI8ScaleAlign)) return fail(LQ_EALIGN, "%s: offsets is not %d-byte aligned", fn, kI8ScaleAlign);
    return LQ_OK;
}

// lq_i8_operand_pack (b == NULL, offsets == NULL, affine false) and lq_i8_operand_pack_affine: one geometry, one set of refusals
static int i8_operand_pack(const char* fn, bool affine, const float* P, const float* s, const float* b, int32_t qmin, int32_t qmax,
                           int rounding, int64_t R, int64_t C, int axis, int64_t gs, void* codes, void* scales, void* offsets,
                           void* stream) {
    int rc = check_group(fn, R, C, axis, gs);
    if (rc) return rc;
    LQ_REQUIRE_PTR_FN(fn, P);
    LQ_REQUIRE_PTR_FN(fn, s);
    if (affine) {
        LQ_REQUIRE_PTR_FN(fn, b);
    }
    if ((rc = check_clip_range(fn, qmin, qmax))) return rc;
    if ((rc = check_rounding(fn, rounding))) return rc;
    if (qmin < -128 || qmax > 127)
        return fail(LQ_EINVAL, "%s: range [%d, %d] is not inside [-128, 127], the operands of the int8 matrix instruction", fn, (int)qmin,
                    (int)qmax);
    const int64_t L = axis == 0 ? C : R, K = axis == 0 ? R : C;
    if (gs < K && gs % kI8TileK != 0)
        return fail(LQ_EINVAL, "%s: group size %lld is neither the whole line (%lld) nor a multiple of %d: a scale must not change "
                    "inside a step of the instruction", fn, (long long)gs, (long long)K, kI8TileK);
    const int64_t block = gs >= K ? 0 : gs;
    I8OperandDims d;
    if ((rc = i8_operand_dims(fn, L, K, block, d))) return rc;
    if ((rc = check_operand_buffers(fn, codes, scales, kI8ScaleAlign))) return rc;
    if (affine && (rc = check_operand_offsets(fn, offsets))) return rc;
    I8PackParams op{};
    op.g = group_params(P, s, qmin, qmax, R, C, axis, gs);
    op.codes = (uint8_t*)codes;
    op.scales = (float*)scales;
    op.line_stride = axis == 0 ? 1 : C;
    op.k_stride = axis == 0 ? C : 1;
    op.s_line_stride = axis == 0 ? 1 : d.nbs;      // [nb][C] | [R][nb]
    op.s_blk_stride = axis == 0 ? C : 1;
    op.L = (int32_t)L;
    op.K = (int32_t)K;
    op.block = (int32_t)block;
    op.LT = (int32_t)d.LT;
    op.KT = (int32_t)d.KT;
    const int64_t threads = d.LT * kI8TileLines * d.KT * 4;
    const dim3 grid((unsigned)((threads + kBlock - 1) / kBlock)), blk(kBlock);
    hipStream_t st = (hipStream_t)stream;
    const bool rne = rounding == LQ_ROUND_NEAREST_EVEN;
    if (affine) {
        I8PackAffineParams ap{};
        static_cast<I8PackParams&>(ap) = op;
        ap.b = b;
        ap.offsets = (float*)offsets;
        if (axis == 0) {
            if (rne) hipLaunchKernelGGL((k_i8_pack<true, true, true>), grid, blk, 0, st, ap);
            else hipLaunchKernelGGL((k_i8_pack<false, true, true>), grid, blk, 0, st, ap);
        } else {
            if (rne) hipLaunchKernelGGL((k_i8_pack<true, false, true>), grid, blk, 0, st, ap);
            else hipLaunchKernelGGL((k_i8_pack<false, false, true>), grid, blk, 0, st, ap);
        }
        return check_hip("int8 operand pack with offsets");
    }
    if (axis == 0) {
        if (rne) hipLaunchKernelGGL((k_i8_pack<true, true>), grid, blk, 0, st, op);
        else hipLaunchKernelGGL((k_i8_pack<false, true>), grid, blk, 0, st, op);
    } else {
        if (rne) hipLaunchKernelGGL((k_i8_pack<true, false>), grid, blk, 0, st, op);
        else hipLaunchKernelGGL((k_i8_pack<false, false>), grid, blk, 0, st, op);
    }
    return check_hip("int8 operand pack");
}

int lq_i8_operand_pack(const float* P, const float* s, int32_t qmin, int32_t qmax, int rounding, int64_t R, int64_t C, int axis,
                       int64_t gs, void* codes, void* scales, void* stream) {
    return i8_operand_pack(__func__, false, P, s, nullptr, qmin, qmax, rounding, R, C, axis, gs, codes, scales, nullptr, stream);
}

int lq_i8_operand_pack_affine(const float* P, const float* s, const float* b, int32_t qmin, int32_t qmax, int rounding, int64_t R,
                              int64_t C, int axis, int64_t gs, void* codes, void* scales, void* offsets, void* stream) {
    return i8_operand_pack(__func__, true, P, s, b, qmin, qmax, rounding, R, C, axis, gs, codes, scales, offsets, stream);
}

int lq_i8_operand_quantize(const float* X, int64_t M, int64_t K, int64_t block, void* codes, void* scales, void* stream) {
    const char* fn = __func__;
    LQ_REQUIRE_PTR_FN(fn, X);
    I8OperandDims d;
    int rc = i8_operand_dims(fn, M, K, block, d);
    if (rc) return rc;
    if ((rc = check_operand_buffers(fn, codes, scales, kI8ScaleAlign))) return rc;
    I8QuantParams op{};
    op.g.P = X;
    op.g.lo = op.ip.lo = -127.0f;
    op.g.hi = op.ip.hi = 127.0f;
    op.ip.min_value = kOperandMinScale;
    op.codes = (uint8_t*)codes;
    op.scales = (float*)scales;
    op.M = (int32_t)M;
    op.K = (int32_t)K;
    op.block = (int32_t)block;
    op.nbs = (int32_t)d.nbs;
    op.LT = (int32_t)d.LT;
    op.KT = (int32_t)d.KT;
    // the team covers its scale block (or row) in one access per lane where 64 lanes can
    const int v = (K % 4 == 0 && aligned(X, 16)) ? 4 : 1;
    const int64_t span = std::min<int64_t>(block ? block : d.KT * kI8TileK, 64 * v);
    int log_team = 0;
    while (log_team < 6 && ((int64_t)v << log_team) < span) ++log_team;
    const int64_t pairs = d.LT * kI8TileLines * d.nbs, per_block = kBlock >> log_team;
    const dim3 grid((unsigned)((pairs + per_block - 1) / per_block)), blk(kBlock);
    if (v == 4) hipLaunchKernelGGL(k_i8_quantize<4>, grid, blk, 0, (hipStream_t)stream, op, log_team);
    else hipLaunchKernelGGL(k_i8_quantize<1>, grid, blk, 0, (hipStream_t)stream, op, log_team);
    return check_hip("int8 operand quantize");
}

// the launch form of lq_i8_operand_im2col (tests/_i8_conv_forms.py restates it): a span that one thread's registers hold takes the
// plain form, a longer one is split over kI8ConvSlices slices -- whatever the number of lines: measured, the split form is never
// slower and up to 2.4 times faster where the plain form had filled the device too
static int i8_conv_slices(int64_t units) { return units > kI8ConvCache ? kI8ConvSlices : 1; }

int lq_i8_operand_im2col(const float* X, const lq_conv_geom* g, int64_t block, void* codes, void* scales, void* stream) {
    const char* fn = __func__;
    LQ_REQUIRE_PTR_FN(fn, X);
    ConvDims cd;
    int rc = conv_geom_dims_strided(fn, g, cd);
    if (rc) return rc;
    I8OperandDims d;
    if ((rc = i8_operand_dims(fn, cd.M, cd.K, block, d))) return rc;      // M * K < 2^31, the block
    if ((rc = check_operand_buffers(fn, codes, scales, kI8ScaleAlign))) return rc;
    I8Im2colParams op{};
    op.g.P = X;
    op.g.lo = op.ip.lo = -127.0f;
    op.g.hi = op.ip.hi = 127.0f;
    op.ip.min_value = kOperandMinScale;
    op.codes = (uint8_t*)codes;
    op.scales = (float*)scales;
    fill_im2col_geom(op.geom, g, cd);
    op.K = (int32_t)cd.K;
    op.block = (int32_t)block;
    op.nbs = (int32_t)d.nbs;
    op.LT = (int32_t)d.LT;
    op.KT = (int32_t)d.KT;
    // the longest span in units: the first scale block, or the padded row
    const int64_t lines = d.LT * kI8TileLines;
    const int64_t units = (d.nbs > 1 ? block : d.KT * kI8TileK) / kI8ConvUnit;
    const int slices = i8_conv_slices(units);
    // a thread block is kBlock / slices consecutive lines of one scale block: chunks per scale block, scale blocks slowest
    const int64_t per = kBlock / slices, chunks = (lines + per - 1) / per;
    op.geom.chunks = make_fastdiv((uint32_t)chunks);
    const dim3 grid((unsigned)(chunks * d.nbs)), blk(kBlock);      // below 2^31: at most M K / 4096 + M / 64 + K / 64 + 1
    hipStream_t st = (hipStream_t)stream;
    if (slices == 1) hipLaunchKernelGGL(k_i8_im2col<1>, grid, blk, 0, st, op);
    else hipLaunchKernelGGL(k_i8_im2col<kI8ConvSlices>, grid, blk, 0, st, op);
    return check_hip("int8 im2col operand");
}

static int i8_operand_decode(const char* fn, bool affine, const void* codes, const void* scales, const void* offsets, int64_t L,
                             int64_t K, int64_t block, float* out, void* stream) {
    I8OperandDims d;
    int rc = i8_operand_dims(fn, L, K, block, d);
    if (rc) return rc;
    if ((rc = check_operand_buffers(fn, codes, scales, kI8ScaleAlign))) return rc;
    if (affine && (rc = check_operand_offsets(fn, offsets))) return rc;
    LQ_REQUIRE_PTR_FN(fn, out);
    I8DecodeParams dp{};
    dp.codes = (const uint8_t*)codes;
    dp.scales = (const float*)scales;
    dp.out = out;
    dp.L = (int32_t)L;
    dp.K = (int32_t)K;
    dp.block = (int32_t)block;
    dp.LT = (int32_t)d.LT;
    dp.KT = (int32_t)d.KT;
    const int64_t n = L * K;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (affine) {
        I8DecodeAffineParams ap{};
        ap.d = dp;
        ap.offsets = (const float*)offsets;
        hipLaunchKernelGGL(k_i8_decode_affine, grid, dim3(kBlock), 0, (hipStream_t)stream, ap);
        return check_hip("int8 operand decode with offsets");
    }
    hipLaunchKernelGGL(k_i8_decode, grid, dim3(kBlock), 0, (hipStream_t)stream, dp);
    return check_hip("int8 operand decode");
}

int lq_i8_operand_decode(const void* codes, const void* scales, int64_t L, int64_t K, int64_t block, float* out, void* stream) {
    return i8_operand_decode(__func__, false, codes, scales, nullptr, L, K, block, out, stream);
}

int lq_i8_operand_decode_affine(const void* codes, const void* scales, const void* offsets, int64_t L, int64_t K, int64_t block,
                                float* out, void* stream) {
    return i8_operand_decode(__func__, true, codes, scales, offsets, L, K, block, out, stream);
}

// lq_i8_gemm (b_offsets == NULL, affine false) and lq_i8_gemm_affine: one set of refusals, one period rule, one grid
static int i8_gemm(const char* fn, bool affine, const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes,
                   const void* b_scales, const void* b_offsets, int64_t b_block, const float* bias, float* Y, int64_t ldy, int64_t M,
                   int64_t N, int64_t K, void* stream) {
    I8OperandDims da, db;
    int rc = i8_operand_dims(fn, M, K, a_block, da);
    if (rc || (rc = i8_operand_dims(fn, N, K, b_block, db))) return rc;
    const int64_t lo = std::min(a_block, b_block), hi = std::max(a_block, b_block);
    if (lo > 0 && hi % lo != 0)
        return fail(LQ_EINVAL, "%s: scale blocks %lld and %lld: the larger must be a multiple of the smaller", fn, (long long)a_block,
                    (long long)b_block);
    const int64_t F = lo > 0 ? lo : hi;            // the period: the smaller non-zero block, or 0 for the whole K
    const int64_t period = F > 0 ? std::min(F, K) : K;
    if (period > 65536)
        return fail(LQ_EINVAL, "%s: a period of %lld k between two scale changes is above 65536: the int32 sum of that many products of "
                    "magnitude up to 2^14 could overflow", fn, (long long)period);
    if ((rc = check_operand_buffers(fn, a_codes, a_scales, kI8ScaleAlign))) return rc;
    if ((rc = check_operand_buffers(fn, b_codes, b_scales, kI8ScaleAlign))) return rc;
    if (affine && (rc = check_operand_offsets(fn, b_offsets))) return rc;
    if ((rc = check_gemm_output(fn, bias, Y, ldy, M, N))) return rc;
    I8GemmParams p{};
    p.a_codes = (const uint8_t*)a_codes;
    p.a_scales = (const float*)a_scales;
    p.b_codes = (const uint8_t*)b_codes;
    p.b_scales = (const float*)b_scales;
    p.bias = bias;
    p.Y = Y;
    p.ldy = ldy;
    p.M = (int32_t)M;
    p.N = (int32_t)N;
    p.MT = (int32_t)da.LT;
    p.NT = (int32_t)db.LT;
    p.KT = (int32_t)da.KT;
    p.ps = (int32_t)(F > 0 ? std::min(F / kI8TileK, da.KT) : da.KT);
    p.a_every = a_block > 0 ? (int32_t)(a_block / F) : INT32_MAX;
    p.b_every = b_block > 0 ? (int32_t)(b_block / F) : INT32_MAX;
    dim3 grid;
    if ((rc = gemm_grid(fn, (db.LT + 3) / 4, da.LT, M, grid))) return rc;
    if (affine) {
        I8GemmAffineParams ap{};
        static_cast<I8GemmParams&>(ap) = p;
        ap.b_offsets = (const float*)b_offsets;
        hipLaunchKernelGGL(k_i8_gemm<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, ap);
        return check_hip("int8 GEMM with offsets");
    }
    hipLaunchKernelGGL(k_i8_gemm<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, p);
    return check_hip("int8 GEMM");
}

int lq_i8_gemm(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales, int64_t b_block,
               const float* bias, float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, void* stream) {
    return i8_gemm(__func__, false, a_codes, a_scales, a_block, b_codes, b_scales, nullptr, b_block, bias, Y, ldy, M, N, K, stream);
}

int lq_i8_gemm_affine(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales,
                      const void* b_offsets, int64_t b_block, const float* bias, float* Y, int64_t ldy, int64_t M, int64_t N,
                      int64_t K, void* stream) {
    return i8_gemm(__func__, true, a_codes, a_scales, a_block, b_codes, b_scales, b_offsets, b_block, bias, Y, ldy, M, N, K, stream);
}

static int i8_gemm_quantize(const char* fn, bool affine, const void* a_codes, const void* a_scales, int64_t a_block,
                            const void* b_codes, const void* b_scales, const void* b_offsets, int64_t b_block, const float* bias,
                            int activation, int64_t out_block, void* out_codes, void* out_scales, int64_t M, int64_t N, int64_t K,
                            void* stream) {
    I8OperandDims da, db, dout;
    int rc = i8_operand_dims(fn, M, K, a_block, da);
    if (rc || (rc = i8_operand_dims(fn, N, K, b_block, db))) return rc;
    const int64_t lo = std::min(a_block, b_block), hi = std::max(a_block, b_block);
    if (lo > 0 && hi % lo != 0)
        return fail(LQ_EINVAL, "%s: scale blocks %lld and %lld: the larger must be a multiple of the smaller", fn, (long long)a_block,
                    (long long)b_block);
    const int64_t F = lo > 0 ? lo : hi;            // the period, as lq_i8_gemm takes it
    const int64_t period = F > 0 ? std::min(F, K) : K;
    if (period > 65536)
        return fail(LQ_EINVAL, "%s: a period of %lld k between two scale changes is above 65536: the int32 sum of that many products of "
                    "magnitude up to 2^14 could overflow", fn, (long long)period);
    if (out_block != kI8TileK)
        return fail(LQ_EINVAL, "%s: out_block = %lld: the epilogue writes scale blocks of %d, the columns of one thread block; one "
                    "scale per row (0) or a larger block needs every column tile of the row before the first code", fn,
                    (long long)out_block, kI8TileK);
    if (activation != LQ_ACT_NONE && activation != LQ_ACT_RELU) return fail(LQ_EINVAL, "%s: bad activation %d", fn, activation);
    if ((rc = i8_operand_dims(fn, M, N, out_block, dout))) return rc;      // M * N < 2^31
    if ((rc = check_operand_buffers(fn, a_codes, a_scales, kI8ScaleAlign))) return rc;
    if ((rc = check_operand_buffers(fn, b_codes, b_scales, kI8ScaleAlign))) return rc;
    if (affine && (rc = check_operand_offsets(fn, b_offsets))) return rc;
    if ((rc = check_operand_buffers(fn, out_codes, out_scales, kI8ScaleAlign))) return rc;
    if ((rc = check_gemm_bias(fn, bias))) return rc;
    I8GemmQuantParams p{};
    p.g.a_codes = (const uint8_t*)a_codes;
    p.g.a_scales = (const float*)a_scales;
    p.g.b_codes = (const uint8_t*)b_codes;
    p.g.b_scales = (const float*)b_scales;
    p.g.bias = bias;
    p.g.M = (int32_t)M;
    p.g.N = (int32_t)N;
    p.g.MT = (int32_t)da.LT;
    p.g.NT = (int32_t)db.LT;
    p.g.KT = (int32_t)da.KT;
    p.g.ps = (int32_t)(F > 0 ? std::min(F / kI8TileK, da.KT) : da.KT);
    p.g.a_every = a_block > 0 ? (int32_t)(a_block / F) : INT32_MAX;
    p.g.b_every = b_block > 0 ? (int32_t)(b_block / F) : INT32_MAX;
    p.gp.lo = p.ip.lo = -127.0f;
    p.gp.hi = p.ip.hi = 127.0f;
    p.ip.min_value = kOperandMinScale;
    p.codes = (uint8_t*)out_codes;
    p.scales = (float*)out_scales;
    p.act = activation;
    p.OKT = (int32_t)dout.KT;
    // along n the grid spans the padded operand, 64 OKT columns, so that its padding is written too
    dim3 grid;
    if ((rc = gemm_grid(fn, dout.KT, da.LT, M, grid))) return rc;
    if (affine) {
        I8GemmQuantAffineParams ap{};
        static_cast<I8GemmQuantParams&>(ap) = p;
        ap.b_offsets = (const float*)b_offsets;
        hipLaunchKernelGGL(k_i8_gemm_quantize<true>, grid, dim3(kBlock), 0, (hipStream_t)stream, ap);
        return check_hip("int8 GEMM with offsets and operand-out epilogue");
    }
    hipLaunchKernelGGL(k_i8_gemm_quantize<false>, grid, dim3(kBlock), 0, (hipStream_t)stream, p);
    return check_hip("int8 GEMM with operand-out epilogue");
}

int lq_i8_gemm_quantize(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales,
                        int64_t b_block, const float* bias, int activation, int64_t out_block, void* out_codes, void* out_scales,
                        int64_t M, int64_t N, int64_t K, void* stream) {
    return i8_gemm_quantize(__func__, false, a_codes, a_scales, a_block, b_codes, b_scales, nullptr, b_block, bias, activation,
                            out_block, out_codes, out_scales, M, N, K, stream);
}

int lq_i8_gemm_quantize_affine(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales,
                               const void* b_offsets, int64_t b_block, const float* bias, int activation, int64_t out_block,
                               void* out_codes, void* out_scales, int64_t M, int64_t N, int64_t K, void* stream) {
    return i8_gemm_quantize(__func__, true, a_codes, a_scales, a_block, b_codes, b_scales, b_offsets, b_block, bias, activation,
                            out_block, out_codes, out_scales, M, N, K, stream);
}

int lq_fq_fwd_bwd_fused(const float* P, const float* s, const float* dy, float lambda, float* out, float* ds, void* ws,
                        size_t ws_bytes, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(dy);
    LQ_REQUIRE_PTR(out);
    LQ_REQUIRE_PTR(ds);
    Plan pl = make_plan(outer, G, inner);
    Params p = base_params(P, s, outer, G, inner);
    p.dy = dy;
    p.lam = lambda;
    p.tmode = tmode_of(lambda);
    p.out = out;
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    return traverse_and_finalize<OP_FUSED>(pl, p, ds, nullptr, nullptr, true, (hipStream_t)stream);
}

int lq_penalty_maxbin_fwd(const float* P, const float* s, float* mb, uint32_t* ties, float* term, void* ws,
                          size_t ws_bytes, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(mb);
    LQ_REQUIRE_PTR(ties);
    LQ_REQUIRE_PTR(term);
    Plan pl = make_plan(outer, G, inner, kBlock);      // weight-sized operation: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    if ((rc = launch_traverse<OP_MAXBIN_FWD>(pl, p, (hipStream_t)stream))) return rc;
    FinGeom f = group_geom(pl, outer, G, inner);
    f.o0 = mb;
    f.o2 = ties;
    if ((rc = launch_finalize<OP_MAXBIN_FWD>(p, f, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL((k_vec_mean<0>), dim3(1), dim3(kBlock), 0, (hipStream_t)stream, mb, G, term);   // :110 reduce_mean(maxbin)
    return check_hip("maxbin mean launch");
}

int lq_penalty_maxbin_bwd(const float* P, const float* s, const float* mb, const uint32_t* ties, const float* c_dev,
                          float c_scale, float* dP, float* ds, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(mb);
    LQ_REQUIRE_PTR(ties);
    LQ_REQUIRE_PTR(c_dev);
    LQ_REQUIRE_PTR(dP);
    LQ_REQUIRE_PTR(ds);
    Plan pl = make_plan(outer, G, inner, kBlock);      // weight-sized operation: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    p.mb = mb;
    p.ties = ties;
    p.c_dev = c_dev;
    p.c_scale = c_scale;
    p.out = dP;
    if ((rc = launch_traverse<OP_MAXBIN_BWD>(pl, p, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL(k_maxbin_ds, dim3((unsigned)ceil_div(G, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, s, mb, c_dev, c_scale, ds, G);
    return check_hip("maxbin ds launch");
}

int lq_penalty_difference_fwd(const float* P, const float* s, float* term, void* ws, size_t ws_bytes, int64_t outer,
                              int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(term);
    Plan pl = make_plan(outer, G, inner, kBlock);      // weight-sized operation: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    if ((rc = launch_traverse<OP_DIFF_FWD>(pl, p, (hipStream_t)stream))) return rc;
    FinGeom f = global_geom(pl, outer, G, inner);
    f.o0 = term;
    return launch_finalize<OP_DIFF_FWD, false>(p, f, (hipStream_t)stream);
}

int lq_penalty_difference_bwd(const float* P, const float* s, const float* c_dev, float c_scale, float* dP, float* ds,
                              void* ws, size_t ws_bytes, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(c_dev);
    LQ_REQUIRE_PTR(dP);
    LQ_REQUIRE_PTR(ds);
    Plan pl = make_plan(outer, G, inner, kBlock);      // weight-sized operation: 256-thread units at every size (kStreamOp)
    Params p = base_params(P, s, outer, G, inner);
    p.c_dev = c_dev;
    p.c_scale = c_scale;
    p.out = dP;
    if ((rc = bind_ws(p, pl, ws, ws_bytes))) return rc;
    return traverse_and_finalize<OP_DIFF_BWD>(pl, p, ds, nullptr, nullptr, false, (hipStream_t)stream);
}

int lq_penalty_inverse_fwd(const float* s, float* term, int64_t G, void* stream) {
    if (G <= 0) return fail(LQ_EINVAL, "lq_penalty_inverse_fwd: G must be positive");
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(term);
    hipLaunchKernelGGL((k_vec_mean<1>), dim3(1), dim3(kBlock), 0, (hipStream_t)stream, s, G, term);
    return check_hip("inverse fwd launch");
}

int lq_penalty_inverse_bwd(const float* s, const float* c_dev, float c_scale, float* ds, int64_t G, void* stream) {
    if (G <= 0) return fail(LQ_EINVAL, "lq_penalty_inverse_bwd: G must be positive");
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(c_dev);
    LQ_REQUIRE_PTR(ds);
    hipLaunchKernelGGL(k_inverse_bwd, dim3((unsigned)ceil_div(G, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, s, c_dev, c_scale, ds, G);
    return check_hip("inverse bwd launch");
}

int lq_scale_adam_step(float* s, const float* ds, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                       double eps, int64_t step, float min_value, int mode, void* stream) {
    if (n <= 0) return fail(LQ_EINVAL, "lq_scale_adam_step: n must be positive");
    if (step < 1) return fail(LQ_EINVAL, "lq_scale_adam_step: step is 1-based");
    if (mode != LQ_ADAM_KERAS && mode != LQ_ADAM_TORCH) return fail(LQ_EINVAL, "lq_scale_adam_step: bad mode %d", mode);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(ds);
    LQ_REQUIRE_PTR(m);
    LQ_REQUIRE_PTR(v);
    // the bias corrections are formed on the device from `step` with the arithmetic of lq_scale_adam_step_dev (Keras 2.11: beta
    // powers and alpha in fp32, tf.pow on the cast hyper-parameter; torch: python doubles), so that a step replayed from a
    // hipGraph (device-side counter) and an eager step give the same bits -- the thresholded scale gradient amplifies a
    // last-bit difference of a scale into visibly different trajectories
    hipLaunchKernelGGL(k_adam_dev, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, s, ds, m, v, n,
                       (float)lr, (float)beta1, (float)beta2, lr, beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                       (float)eps, (const int64_t*)nullptr, step, min_value, mode);
    return check_hip("adam launch");
}

int lq_scale_adam_step_dev(float* s, const float* ds, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                           double eps, const int64_t* step_dev, float min_value, int mode, void* stream) {
    if (n <= 0) return fail(LQ_EINVAL, "lq_scale_adam_step_dev: n must be positive");
    if (mode != LQ_ADAM_KERAS && mode != LQ_ADAM_TORCH) return fail(LQ_EINVAL, "lq_scale_adam_step_dev: bad mode %d", mode);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(ds);
    LQ_REQUIRE_PTR(m);
    LQ_REQUIRE_PTR(v);
    if (!step_dev || !aligned(step_dev, 8)) return fail(LQ_EINVAL, "lq_scale_adam_step_dev: step_dev must be an 8-byte aligned device pointer");
    hipLaunchKernelGGL(k_adam_dev, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, s, ds, m, v, n,
                       (float)lr, (float)beta1, (float)beta2, lr, beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                       (float)eps, step_dev, (int64_t)0, min_value, mode);
    return check_hip("adam (device step) launch");
}

int lq_min_value_project(float* w, int64_t n, float min_value, void* stream) {
    if (n <= 0) return fail(LQ_EINVAL, "lq_min_value_project: n must be positive");
    LQ_REQUIRE_PTR(w);
    hipLaunchKernelGGL(k_min_project, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, w, n, min_value);
    return check_hip("min project launch");
}

int lq_q_absmax_over_axis(const float* P, const float* s, float* result, int64_t pre, int64_t n_axis, int64_t post,
                          int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    if (pre <= 0 || n_axis <= 0 || post <= 0 || pre * n_axis * post != outer * G * inner)
        return fail(LQ_EINVAL, "lq_q_absmax_over_axis: (pre,n_axis,post) does not match the tensor");
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(result);
    const int64_t n = pre * n_axis * post;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(result, 0, (size_t)(pre * post) * sizeof(float), st) != hipSuccess) return check_hip("absmax axis memset");
    const int64_t blocks = ceil_div(n, (int64_t)kAbsChunk);
    if (blocks > 2147483647ll) return fail(LQ_EINVAL, "lq_q_absmax_over_axis: tensor too large");
    // outputs one chunk can touch: (chunks of slices it overlaps) * post entries, starting at its first slice
    const int64_t slice = n_axis * post;
    int64_t span = (ceil_div((int64_t)kAbsChunk, slice) + 1) * post;
    if (span > pre * post) span = pre * post;
    const int use_lds = span <= kAbsTab ? 1 : 0;
    if (n < 4294967296ll)
        hipLaunchKernelGGL(k_q_absmax_axis<uint32_t>, dim3((unsigned)blocks), dim3(kBlock), 0, st, P, s, reinterpret_cast<uint32_t*>(result),
                           (uint32_t)n, (uint32_t)n_axis, (uint32_t)post, (uint32_t)G, (uint32_t)inner, use_lds, (int)(use_lds ? span : 0));
    else
        hipLaunchKernelGGL(k_q_absmax_axis<int64_t>, dim3((unsigned)blocks), dim3(kBlock), 0, st, P, s, reinterpret_cast<uint32_t*>(result),
                           n, n_axis, post, G, inner, use_lds, (int)(use_lds ? span : 0));
    return check_hip("absmax axis launch");
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
//  lq_batch: host object + C ABI
// ------------------------------------------------------------------------------------------
struct lq_task_table {                    // one device-resident task table
    std::vector<lq::Task> h;
    std::vector<int> index;               // table position -> descriptor index (tasks are ordered by work per block)
    lq::Task* d = nullptr;
    uint32_t* prefix_d = nullptr;         // [n] first block of every task, then [n] first group
    uint32_t* block_task_d = nullptr;     // [blocks] task of every traversal block (a DWORD each: one scalar load; sub-dword entries are fetched with vector loads)
    lq::FinRec* fin_blocks_d = nullptr;   // [fin_blocks] one self-contained record per finalize block (scale-gradient tables)
    std::vector<lq::FinRec> fin_h;        // host copy: the Adam-state pointers are filled in by lq_batch_create before the upload
    uint32_t fin_blocks = 0;
    uint32_t blocks = 0, groups = 0;
    bool has_tile = false;                // some task runs the conv tile (needs the tile kernel's LDS)
    int64_t ws_words = 0;
};

struct lq_batch {
    int n = 0;
    lq_task_table fwd, bwd, bwd_o, pen;   // bwd: HWIO gradients (generic traversals); bwd_o: OIHW gradients of the conv kernels (tiles);
                                          // pen: every tensor, with workspace slices and mb/ties buffers (penalty passes)
    std::vector<lq::AdamTask> adam_h;
    float* mb_d = nullptr;
    uint32_t* ties_d = nullptr;
    lq::AdamTask* adam_d = nullptr;
    size_t ws_bytes = 256;
    bool has_perm = false;               // some conv kernel has an OIHW companion
    // clipped pair (lq_batch_set_clip): tables of their own, planned for the generic traversal bodies with the stored destination's
    // alignment taken into account (cfwd: out; cbwd: dp), Params::clip_lo / clip_hi per task
    std::vector<lq_tensor_desc> descs;   // the descriptors as given to lq_batch_create
    lq_task_table cfwd, cbwd;
    uint32_t* clip_d = nullptr;          // per-group clip counts, in the order of cbwd's groups
    bool has_clip = false;
    int clip_rounding = 0;
};

namespace lq {

// Conv-tile geometry of an HWIO kernel (lq_conv_tile.hpp), or false when the tensor keeps the generic traversal: kernels
// with more than 9 taps, co % 4 != 0, or a descriptor whose groups are not a function of (h, c) the tile knows.
static bool make_conv_tile(ConvTile& ct, int64_t hw, int64_t ci, int64_t co, int64_t outer, int64_t G, int64_t inner) {
    memset(&ct, 0, sizeof(ct));
    if (hw < 1 || hw > kCtPass || co % 4 != 0 || ci < 1) return false;
    if ((double)hw * (double)ci * (double)co >= 4294967296.0) return false;
    int kind;
    int64_t A = 1;
    if (G == 1) {
        kind = 1;
        A = hw;
    } else if (inner == co && G == ci) {
        kind = 0;
    } else if (inner % (ci * co) == 0 && G <= 255) {
        kind = 1;
        A = inner / (ci * co);
        if (outer * G * A != hw) return false;
    } else {
        return false;
    }
    int64_t m = kCtPass / hw;
    const int64_t mc = ceil_div(ci, 32);
    if (m > mc) m = mc;
    if (m < 1) m = 1;
    ct.hw = (uint32_t)hw;
    ct.ci = (uint32_t)ci;
    ct.co = (uint32_t)co;
    ct.tc = (uint32_t)(32 * m);
    ct.ntc = (uint32_t)ceil_div(ci, 32 * m);
    ct.nto = (uint32_t)ceil_div(co, kCtO);
    if ((double)ct.ntc * (double)ct.nto > 2147483647.0) return false;
    ct.npass = (uint32_t)(m * hw);
    ct.kind = (uint32_t)kind;
    ct.fnto = make_fastdiv(ct.nto);
    // pass order: kind 0 by channel block, kind 1 group by group (one accumulator flush per group)
    struct PassKey { int g, j, h; };
    std::vector<PassKey> ps;
    for (int64_t j = 0; j < m; ++j)
        for (int64_t h = 0; h < hw; ++h) ps.push_back({kind == 0 ? (int)j : (int)((h / A) % G), (int)j, (int)h});
    std::stable_sort(ps.begin(), ps.end(), [](const PassKey& a, const PassKey& b) { return a.g < b.g; });
    for (size_t q = 0; q < ps.size(); ++q) {
        const uint32_t is_new = (q > 0 && ps[q].g != ps[q - 1].g) ? 1u : 0u;
        ct.pass_info[q] = (uint32_t)(8 * ps[q].j) | ((uint32_t)ps[q].h << 8) | ((uint32_t)(kind == 0 ? 0 : ps[q].g) << 16) | (is_new << 24);
        ct.pass_off[q] = (uint32_t)(((int64_t)ps[q].h * ci + 8 * ps[q].j) * co);
    }
    return true;
}

// the tile's partials (see ct_flush): per group one run of a partial per column tile (kind 0), or per (tile, wave) (kind 1)
static PartialLayout conv_tile_layout(const ConvTile& ct, int64_t G) {
    const int64_t per_group = ct.kind == 0 ? (int64_t)ct.nto : (int64_t)ct.nto * ct.ntc * kWavesPerBlock;
    return {(ct.kind == 0 ? (int64_t)ct.ci : G) * per_group, per_group, 1, 0, per_group};
}

// the batch's group fragments (lq_batch_cols.hpp): one partial per (row block, fragment); finalize_frag_body walks them through
// Task::fg, the geometry here is kept consistent for the workspace bound
static PartialLayout layout_frags(int64_t nby, int64_t F) { return {nby * F, 0, nby, F, 1}; }

// Row blocks of the batch's scale-gradient column tiles are sized by the BATCH, not per tensor: make_plan aims at about 512 blocks
// per tensor (right for a launch of its own); 40 or 108 tensors in one launch then make 2000-5300 blocks of 2-8 K elements, more than
// the chip holds at once -- the second round of blocks ran on a nearly idle chip (profiles/r03/timelines/) -- and 4-8 times the
// partials the launch needs.  Every float4 column tile of the scale-gradient table gets about `w` elements per block instead, with
// `w` chosen so that the whole launch is one resident round.
static double batch_block_elements(double total_elements) {
    LQ_KNOB(w, "LQ_TUNE_BATCH_W", 0);                  // development: force the elements per block
    if (w > 0) return (double)w;
    LQ_KNOB(nb, "LQ_TUNE_BATCH_NB", 1280);             // blocks the chip holds at once: 256 CUs x 5 (k_batch_traverse<OP_BWD>: 5 waves per SIMD)
    const double per = total_elements / (double)nb;
    return per < 8192.0 ? 8192.0 : per;
}

static void batch_rows_per_block(Plan& pl, int64_t outer, double w) {
    const int64_t tilew = pl.C < 256 ? pl.C : 256;
    int64_t rb = ceil_div((int64_t)w, tilew);
    rb = ceil_div(rb, 16) * 16;                        // whole rounds of four waves x four rows
    if (rb > outer) rb = outer;
    const int64_t nby = ceil_div(outer, rb);
    rb = ceil_div(ceil_div(outer, nby), 4) * 4;        // even out the row blocks
    if (rb > outer) rb = outer;
    pl.rps = rb;
    pl.ysplit = ceil_div(outer, rb);
}

// Narrow column matrices (C <= 64: row-wise / column-wise scales of a conv kernel stored OIHW are [co ci][kh kw] and [co ci kh][kw],
// groups of period 9 and 3) as a periodic float4 stream (lq_traverse.hpp col_periodic4_body): `nblk` blocks, a multiple of C, so that
// a thread's four columns never change; about `w` elements per block.  The scalar form it replaces in the batch reads 4 bytes per
// lane (col_small_body: 252 bytes per wave and load for C = 9).
static int64_t batch_periodic_blocks(int64_t C, double elements, double w) {
    int64_t k = (int64_t)(elements / w / (double)C + 0.5);
    if (k < 1) k = 1;
    return C * k;
}
constexpr double kBatchPeriodicMin = 32768.0;      // elements from which a C <= 64 task of the batch takes the periodic form

static int fill_task(Task& t, const lq_tensor_desc& d, bool bwd, bool allow_tile, lq_task_table& tb, double batch_w = 0.0) {
    memset(&t, 0, sizeof(t));
    Plan pl = make_plan(d.outer, d.G, d.inner, kBlock);
    // a task runs one form, chosen here: where that is not the plan's, its partial count is the bound of the task's workspace slice too
    auto relayout = [&pl](const PartialLayout& lay) {
        pl.lay = lay;
        pl.np_bound = lay.np;
    };
    t.p = base_params(d.P, d.s, d.outer, d.G, d.inner);
    t.p.out = d.out;
    t.p.dy = d.dy;
    t.p.lam = d.lambda;
    t.p.tmode = tmode_of(d.lambda);
    bool tile = false;
    if (d.conv_co > 0) {
        t.p.out_perm = bwd ? nullptr : d.out_oihw;
        t.p.perm_hw = (uint32_t)d.conv_hw;
        t.p.perm_ci = (uint32_t)d.conv_ci;
        t.p.perm_co = (uint32_t)d.conv_co;
        t.dp = d.dp;
        tile = allow_tile && aligned(d.P, 16) && aligned(bwd ? (const void*)d.dp : (const void*)d.out, 16) &&
               make_conv_tile(t.ct, d.conv_hw, d.conv_ci, d.conv_co, d.outer, d.G, d.inner);
    }
    t.ds = d.ds;
    t.mode = tile ? MODE_CONV_TILE : pl.mode;
    t.lpr_log2 = pl.lpr_log2;
    t.R = pl.R;
    t.L = pl.L;
    t.nc = pl.nc;
    t.C = pl.C;
    t.nbx = 0;
    if (!tile && pl.mode == MODE_COL) {
        col_variant(pl, d.P, nullptr, bwd ? nullptr : d.out, t.col_variant, t.nbx, false);
        // scale-gradient table of the plain (non-companion) pass: float4 tiles run lq_batch_cols.hpp -- batch-sized row blocks, one
        // partial per (row block, group fragment)
        if (bwd && batch_w > 0.0 && t.col_variant >= 4 && pl.C < (1ll << 30) && d.outer < (1ll << 31)) {
            batch_rows_per_block(pl, d.outer, batch_w);
            LQ_KNOB(frag, "LQ_TUNE_BATCH_FRAG", 1);    // development: 0 = a partial per column (the generic layout)
            const bool grouped = frag && d.inner > 1 && d.inner <= 64;
            t.fg = make_frag_geom(d.G, d.inner, pl.C, grouped);
            if (grouped) {
                relayout(layout_frags(pl.ysplit, (int64_t)t.fg.F));
            } else {
                t.fg.F = (uint32_t)pl.C;
                t.fg.gpb = 0;
                relayout(layout_cols(pl.ysplit, pl.C, d.inner));
            }
        } else if (!bwd && batch_w > 0.0 && t.col_variant >= 4) {
            // forward tiles keep make_plan's row blocks (16-32 rows: 1968 blocks for the ResNet-18-like set, all resident at 62 VGPRs)
            LQ_KNOB(fw, "LQ_TUNE_BATCH_FWD_W", 0);     // development: elements per block of the forward's tiles
            if (fw > 0) batch_rows_per_block(pl, d.outer, (double)fw);
        } else if (bwd && batch_w > 0.0 && t.col_variant >= 4) {
            // a matrix beyond the 32-bit extents of that form (2^30 columns): the scalar column tile, generic layout
            t.col_variant = 1;
            t.nbx = ceil_div(pl.C, 64);
        } else if (batch_w > 0.0 && t.col_variant == 0 && (double)d.outer * (double)pl.C >= kBatchPeriodicMin && aligned(d.P, 16) &&
                   (bwd || aligned(d.out, 16))) {
            t.col_variant = 6;
            pl.ysplit = batch_periodic_blocks(pl.C, (double)d.outer * (double)pl.C, batch_w);
            pl.rps = pl.ysplit;                        // variant 6: the block count travels in `rps`
            t.nbx = 1;
            relayout(layout_cols(pl.ysplit, pl.C, d.inner));      // one partial per (block, column)
        }
    }
    t.rps = pl.rps;
    int64_t blocks;
    if (tile) {
        blocks = (int64_t)t.ct.ntc * t.ct.nto;
        t.vec = 1;
    } else if (pl.mode == MODE_ROW_BIG) {
        // float4 path: forward needs P and out 16-byte aligned; backward needs P (dy is checked at every launch)
        t.vec = (aligned(d.P, 16) && (bwd || aligned(d.out, 16))) ? 1 : 0;
        t.ru = 1;
        if (batch_w > 0.0 && t.vec && d.conv_co == 0) {
            // batch-sized units for long rows (forward and scale-gradient tables): 4096 elements where a row has at least two of them
            const int ru = pl.L >= 8192 ? 4 : (pl.L >= 4096 ? 2 : 1);
            if (ru > 1) {
                t.ru = ru;
                pl.nc = row_chunks(pl.L, (int64_t)kBlock * 4 * ru);
                relayout(layout_row_chunks(pl.R, pl.nc, pl.R / d.G, d.G));
                t.nc = pl.nc;
            }
        }
        blocks = pl.R * pl.nc;
    } else if (pl.mode == MODE_ROW_SMALL) {
        t.vec = row_small_vec(pl, d.P, nullptr, bwd ? nullptr : d.out) ? 1 : 0;
        if (t.vec) t.lpr_log2 = row_small_lpr_log2_vec(pl.L);
        blocks = ceil_div(pl.R, kBlock >> t.lpr_log2);
    } else {
        blocks = t.nbx * pl.ysplit;
    }
    if (blocks <= 0 || blocks > 0x7fffffffll) return fail(LQ_EINVAL, "lq_batch_create: too many blocks");
    t.first_block = (uint32_t)blocks;            // block COUNT until finish_table() turns it into a prefix
    if (bwd) {
        t.first_group = (uint32_t)d.G;           // likewise
        if (tile) relayout(conv_tile_layout(t.ct, d.G));
        t.gstride = pl.lay.gstride;
        t.n1 = pl.lay.n1;
        t.stride1 = pl.lay.stride1;
        t.n2 = pl.lay.n2;
        t.np_pad = (int64_t)ws_partials(pl);
        t.count = (double)d.outer * (double)d.inner;
    }
    if (tile) tb.has_tile = true;
    return LQ_OK;
}

// Orders the table by decreasing work per block (tiles first), assigns block / group prefixes and workspace slices, uploads.
static int finish_table(lq_task_table& tb, bool bwd, int slices = 1) {     // slices: partial slices per task (2: an op with a second accumulator)
    const size_t n = tb.h.size();
    if (!n) return LQ_OK;
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    auto weight = [&](size_t i) {
        const Task& t = tb.h[i];
        const double el = (double)t.p.outer * (double)t.p.G * (double)t.p.inner;
        return el / (double)t.first_block;                     // elements per block
    };
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weight(a) > weight(b); });
    std::vector<Task> h2(n);
    std::vector<int> idx2(n);
    std::vector<uint32_t> prefix(2 * n);
    uint64_t bp = 0, gp = 0;
    int64_t words = 0;
    for (size_t k = 0; k < n; ++k) {
        Task t = tb.h[order[k]];
        const uint32_t nb = t.first_block, ng = bwd ? t.first_group : 0u;
        if (bp + nb > 0xffffffffull || gp + ng > 0xffffffffull) return fail(LQ_EINVAL, "lq_batch_create: too many blocks or groups");
        t.first_block = (uint32_t)bp;
        t.first_group = (uint32_t)gp;
        prefix[k] = (uint32_t)bp;
        prefix[n + k] = (uint32_t)gp;
        bp += nb;
        gp += ng;
        if (bwd) {
            t.ws_off = words;
            words += 4 * t.np_pad * slices;
        }
        h2[k] = t;
        idx2[k] = tb.index[order[k]];
    }
    tb.h.swap(h2);
    tb.index.swap(idx2);
    tb.blocks = (uint32_t)bp;
    tb.groups = (uint32_t)gp;
    tb.ws_words = words;
    std::vector<uint32_t> bt((size_t)bp);
    for (size_t k = 0; k < n; ++k) {
        const uint64_t end = k + 1 < n ? prefix[k + 1] : bp;
        for (uint64_t b = prefix[k]; b < end; ++b) bt[b] = (uint32_t)k;
    }
    hipError_t e = hipMalloc(&tb.prefix_d, 2 * n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(tb.prefix_d, prefix.data(), 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&tb.block_task_d, bt.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(tb.block_task_d, bt.data(), bt.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && bwd && gp > 0) {
        // finalize blocks: column traversals (one partial per (row block, column), a group's partials `C` words apart) get a
        // block per floor(64 / inner) groups that reads contiguous runs of the rows of partials; otherwise four groups per block (a wave each)
        // where a group has at most 256 partials, else a block per group
        std::vector<FinRec>& fb = tb.fin_h;
        fb.clear();
        for (size_t k = 0; k < n; ++k) {
            const Task& t = tb.h[k];
            const bool frag = t.fg.gpb != 0;                                                  // lq_batch_cols.hpp: fragments of fg.gpb groups per block
            const bool cols = !frag && finalize_cols_ok(t.p.G, t.gstride, t.n1, t.stride1, t.n2);      // the rule of the single-tensor finalize
            const bool wide = !frag && !cols && t.n1 * t.n2 > 256;
            const int64_t per = frag ? (int64_t)t.fg.gpb : (cols ? 64 / t.n2 : (wide ? 1 : 4));
            FinRec r;
            memset(&r, 0, sizeof(r));
            r.form = frag ? 3u : (cols ? 2u : (wide ? 1u : 0u));
            r.G = (uint32_t)t.p.G;
            r.lam = t.p.lam;
            r.ws_off = t.ws_off;
            r.np_pad = t.np_pad;
            r.gstride = t.gstride;
            r.n1 = t.n1;
            r.stride1 = t.stride1;
            r.n2 = t.n2;
            r.fg = t.fg;
            r.count = t.count;
            r.ds = t.ds;
            r.s = const_cast<float*>(t.p.s);
            r.pad = (uint32_t)k;                       // table position of the task: fill_fin_state() finds its Adam state through it
            for (int64_t g = 0; g < t.p.G; g += per) {
                r.g0 = (uint32_t)g;
                fb.push_back(r);
            }
        }
        if (fb.size() > 0x7fffffffull) return fail(LQ_EINVAL, "lq_batch_create: too many groups");
        tb.fin_blocks = (uint32_t)fb.size();
        e = hipMalloc(&tb.fin_blocks_d, fb.size() * sizeof(FinRec));
    }
    if (e == hipSuccess) e = hipMalloc(&tb.d, n * sizeof(Task));
    if (e != hipSuccess) return fail(LQ_EHIP, "lq_batch_create: %s", hipGetErrorString(e));
    return LQ_OK;
}

static int upload_table(lq_task_table& tb) {
    if (tb.h.empty()) return LQ_OK;
    hipError_t e = hipMemcpy(tb.d, tb.h.data(), tb.h.size() * sizeof(Task), hipMemcpyHostToDevice);
    if (e == hipSuccess && !tb.fin_h.empty()) {
        for (FinRec& r : tb.fin_h) {                   // Adam state of the task (set after finish_table ordered the tasks)
            const Task& t = tb.h[r.pad];
            r.am = t.am;
            r.av = t.av;
            r.amin = t.amin;
        }
        e = hipMemcpy(tb.fin_blocks_d, tb.fin_h.data(), tb.fin_h.size() * sizeof(FinRec), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return fail(LQ_EHIP, "lq_batch_create: %s", hipGetErrorString(e));
    return LQ_OK;
}

static void free_table(lq_task_table& tb) {
    if (tb.d) (void)hipFree(tb.d);
    if (tb.prefix_d) (void)hipFree(tb.prefix_d);
    if (tb.block_task_d) (void)hipFree(tb.block_task_d);
    if (tb.fin_blocks_d) (void)hipFree(tb.fin_blocks_d);
    tb.block_task_d = nullptr;
    tb.fin_blocks_d = nullptr;
    tb.d = nullptr;
    tb.prefix_d = nullptr;
}

}  // namespace lq

extern "C" {

int lq_batch_create(const lq_tensor_desc* descs, int n, lq_batch** out) {
    if (!descs || !out) return fail(LQ_EINVAL, "lq_batch_create: NULL argument");
    if (n <= 0 || n > kBatchMax) return fail(LQ_EINVAL, "lq_batch_create: n must be in 1..%d", kBatchMax);
    lq_batch* b = new (std::nothrow) lq_batch();
    if (!b) return fail(LQ_EHIP, "lq_batch_create: out of host memory");
    b->n = n;
    b->descs.assign(descs, descs + n);
    int rc = LQ_OK;
    double bwd_elements = 0.0;             // elements the scale-gradient pass traverses: sizes its row blocks (batch_block_elements)
    for (int i = 0; i < n; ++i)
        if (descs[i].lambda == descs[i].lambda && descs[i].outer > 0 && descs[i].G > 0 && descs[i].inner > 0)
            bwd_elements += (double)descs[i].outer * (double)descs[i].G * (double)descs[i].inner;
    const double batch_w = batch_block_elements(bwd_elements);
    // the forward table keeps make_plan's float4 tiles (its blocks are all resident: 61 VGPRs); `b_fwd_w` only sizes the periodic
    // streams of narrow column matrices -- and only where no OIHW companion is emitted (OP_FWD; OP_FWD_PERM has no float4 element path)
    bool any_perm = false;
    for (int i = 0; i < n; ++i) any_perm = any_perm || descs[i].conv_co > 0;
    const double b_fwd_w = any_perm ? 0.0 : 8192.0;
    for (int i = 0; i < n && !rc; ++i) {
        const lq_tensor_desc& d = descs[i];
        rc = check_desc(d.outer, d.G, d.inner);
        // `out` (HWIO) is optional for a conv kernel whose OIHW companion is the only consumer, where the LDS tile serves it
        const bool out_optional = !rc && d.conv_co > 0 && d.out_oihw && aligned(d.P, 16) &&
                                  lq_conv_tile_supported(d.conv_hw, d.conv_ci, d.conv_co, d.outer, d.G, d.inner);
        if (!rc && (!d.P || !d.s || (!d.out && !out_optional)))
            rc = fail(LQ_EINVAL, "lq_batch_create: tensor %d has a NULL P/s/out (out may be NULL only next to an out_oihw the LDS-tile path writes)", i);
        if (!rc && (!aligned(d.P, 4) || !aligned(d.s, 4) || !aligned(d.out, 4))) rc = fail(LQ_EALIGN, "lq_batch_create: tensor %d misaligned", i);
        if (!rc && d.conv_co > 0) {
            rc = check_conv("lq_batch_create", d.conv_hw, d.conv_ci, d.conv_co, d.outer, d.G, d.inner);
            if (!rc && (!d.out_oihw || !d.dp || !aligned(d.out_oihw, 4) || !aligned(d.dp, 4)))
                rc = fail(LQ_EINVAL, "lq_batch_create: tensor %d has conv extents but no out_oihw / dp buffer", i);
            if (!rc) b->has_perm = true;
        }
        Task t;
        if (!rc) rc = fill_task(t, d, false, true, b->fwd, b_fwd_w);
        if (rc) break;
        b->fwd.h.push_back(t);
        b->fwd.index.push_back(i);
        if (d.ds) {                   // penalty passes need a scale-gradient destination
            Task tp;
            if ((rc = fill_task(tp, d, true, false, b->pen))) break;
            b->pen.h.push_back(tp);
            b->pen.index.push_back(i);
        }
        if (d.lambda == d.lambda) {   // not NaN: nested-quantization tensor with a scale gradient
            if (!d.ds) {
                rc = fail(LQ_EINVAL, "lq_batch_create: tensor %d has lambda but no ds", i);
                break;
            }
            Task tb;
            if ((rc = fill_task(tb, d, true, false, b->bwd, batch_w))) break;
            if (d.m && d.v) {           // the finalize can apply the scale's Adam step itself (lq_batch_scale_grad_step)
                tb.am = d.m;
                tb.av = d.v;
                tb.amin = d.min_value;
            }
            b->bwd.h.push_back(tb);
            b->bwd.index.push_back(i);
            if ((rc = fill_task(tb, d, true, true, b->bwd_o))) break;
            if (d.m && d.v) {
                tb.am = d.m;
                tb.av = d.v;
                tb.amin = d.min_value;
            }
            b->bwd_o.h.push_back(tb);
            b->bwd_o.index.push_back(i);
        }
        if (d.m && d.v) {
            AdamTask a;
            memset(&a, 0, sizeof(a));
            a.s = const_cast<float*>(d.s);
            a.ds = d.ds;
            a.m = d.m;
            a.v = d.v;
            a.n = d.G;
            a.min_value = d.min_value;
            if (!d.ds) {
                rc = fail(LQ_EINVAL, "lq_batch_create: tensor %d has Adam state but no ds", i);
                break;
            }
            b->adam_h.push_back(a);
        }
    }
    if (!rc) rc = finish_table(b->fwd, false);
    if (!rc) rc = finish_table(b->bwd, true);
    if (!rc) rc = finish_table(b->bwd_o, true);
    if (!rc) rc = finish_table(b->pen, true, 2);      // OP_DIFF_BWD_V writes a second partial per work unit
    if (!rc && !b->pen.h.empty()) {
        hipError_t e = hipMalloc(&b->mb_d, (size_t)b->pen.groups * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&b->ties_d, (size_t)b->pen.groups * sizeof(uint32_t));
        if (e != hipSuccess) rc = fail(LQ_EHIP, "lq_batch_create: %s", hipGetErrorString(e));
        for (auto& tp : b->pen.h) {
            tp.mb = b->mb_d + tp.first_group;
            tp.ties = b->ties_d + tp.first_group;
        }
    }
    if (!rc) rc = upload_table(b->fwd);
    if (!rc) rc = upload_table(b->bwd);
    if (!rc) rc = upload_table(b->bwd_o);
    if (!rc) rc = upload_table(b->pen);
    if (!rc && !b->adam_h.empty()) {
        hipError_t e = hipMalloc(&b->adam_d, b->adam_h.size() * sizeof(AdamTask));
        if (e == hipSuccess) e = hipMemcpy(b->adam_d, b->adam_h.data(), b->adam_h.size() * sizeof(AdamTask), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail(LQ_EHIP, "lq_batch_create: %s", hipGetErrorString(e));
    }
    if (rc) {
        char keep[sizeof(g_err)];
        memcpy(keep, g_err, sizeof(keep));
        lq_batch_destroy(b);
        memcpy(g_err, keep, sizeof(keep));
        return rc;
    }
    int64_t words = b->bwd.ws_words > b->pen.ws_words ? b->bwd.ws_words : b->pen.ws_words;
    if (b->bwd_o.ws_words > words) words = b->bwd_o.ws_words;
    b->ws_bytes = (size_t)words * 4 + 256;
    *out = b;
    return LQ_OK;
}

int lq_batch_destroy(lq_batch* b) {
    if (!b) return LQ_OK;
    free_table(b->fwd);
    free_table(b->bwd);
    free_table(b->bwd_o);
    free_table(b->pen);
    free_table(b->cfwd);
    free_table(b->cbwd);
    if (b->clip_d) (void)hipFree(b->clip_d);
    if (b->adam_d) (void)hipFree(b->adam_d);
    if (b->mb_d) (void)hipFree(b->mb_d);
    if (b->ties_d) (void)hipFree(b->ties_d);
    delete b;
    return LQ_OK;
}

size_t lq_batch_workspace_bytes(const lq_batch* b) { return b ? b->ws_bytes : 0; }

int lq_batch_forward(const lq_batch* b, void* stream) {
    if (!b) return fail(LQ_EINVAL, "lq_batch_forward: NULL batch");
    PtrPack pk;
    CoefPack cf;
    const lq_task_table& tb = b->fwd;
    const int nt = (int)tb.h.size();
    if (b->has_perm)
        hipLaunchKernelGGL((k_batch_traverse<OP_FWD_PERM>), dim3(tb.blocks), dim3(kBlock), 0, (hipStream_t)stream, tb.d, tb.block_task_d, nt,
                           (uint32_t*)nullptr, pk, 0, cf);
    else
        hipLaunchKernelGGL((k_batch_traverse<OP_FWD>), dim3(tb.blocks), dim3(kBlock), 0, (hipStream_t)stream, tb.d, tb.block_task_d, nt,
                           (uint32_t*)nullptr, pk, 0, cf);
    return check_hip("batch forward launch");
}

}  // extern "C"

// ---- checks the batch entry points share ----
// Does the traversal the task was planned for touch its streams with 16-byte accesses?
static bool task_wants16(const lq::Task& t) {
    return t.mode == MODE_CONV_TILE || (t.mode != MODE_COL && t.vec) || (t.mode == MODE_COL && t.col_variant >= 4);
}

static int check_batch_workspace(const char* fn, const lq_batch* b, const void* ws, size_t ws_bytes) {
    if (!ws) return fail(LQ_EWORKSPACE, "%s: workspace is NULL (need %zu bytes)", fn, b->ws_bytes);
    if (!aligned(ws, 16)) return fail(LQ_EALIGN, "%s: workspace must be 16-byte aligned", fn);
    if (ws_bytes < b->ws_bytes) return fail(LQ_EWORKSPACE, "%s: workspace too small: %zu < %zu bytes", fn, ws_bytes, b->ws_bytes);
    return LQ_OK;
}

// The upstream gradient of every task of `tb` into pk.dy: the caller's dy[tensor] or else the descriptor's.  oihw: gradients of
// conv kernels are read through the permutation (LDS tile or element-wise), never with vector loads.  A dy off the 16-byte grid
// of a task that wants it there fails at that tensor, or with `report16_last` after every dy was looked at, without an index.
// per_task(i, task): what else the caller checks or collects per task, after the task's dy passed.
template <class F>
static int gather_dy(const char* fn, const lq_task_table& tb, const float* const* dy, bool oihw, PtrPack& pk, bool report16_last, F&& per_task) {
    bool all_aligned = true;
    for (size_t i = 0; i < tb.h.size(); ++i) {
        const lq::Task& t = tb.h[i];
        const float* d = dy ? dy[tb.index[i]] : t.p.dy;
        if (!d) return fail(LQ_EINVAL, "%s: no upstream gradient for tensor %d", fn, tb.index[i]);
        if (!aligned(d, 4)) return fail(LQ_EALIGN, "%s: dy of tensor %d misaligned", fn, tb.index[i]);
        const bool gathered = oihw && t.p.perm_co != 0;
        if (!gathered && task_wants16(t) && !aligned(d, 16)) {
            if (!report16_last) return fail(LQ_EALIGN, "%s: dy of the 16-byte aligned tensor %d is not 16-byte aligned", fn, tb.index[i]);
            all_aligned = false;
        }
        if (int rc = per_task(i, t)) return rc;
        pk.dy[i] = d;
    }
    if (!all_aligned) return fail(LQ_EALIGN, "%s: a 16-byte aligned tensor got a dy that is not 16-byte aligned", fn);
    return LQ_OK;
}

static AdamHyper adam_hyper(double lr, double beta1, double beta2, double eps, int64_t step, const int64_t* step_dev, int mode, int on) {
    AdamHyper h;
    memset(&h, 0, sizeof(h));
    h.lr_d = lr;
    h.b1_d = beta1;
    h.b2_d = beta2;
    h.step_dev = step_dev;
    h.step_host = step;
    h.lr = (float)lr;
    h.b1 = (float)beta1;
    h.b2 = (float)beta2;
    h.f0 = (float)(1.0 - beta1);
    h.f1 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.mode = mode;
    h.on = on;
    return h;
}

static int batch_scale_grad(const lq_batch* b, const float* const* dy, void* ws, size_t ws_bytes, void* stream, bool oihw, const AdamHyper& ah) {
    const char* fn = "lq_batch_scale_grad";
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    const lq_task_table& tb = oihw ? b->bwd_o : b->bwd;
    if (tb.h.empty()) return LQ_OK;
    int rc = check_batch_workspace(fn, b, ws, ws_bytes);
    if (rc) return rc;
    PtrPack pk;
    memset(&pk, 0, sizeof(pk));
    if ((rc = gather_dy(fn, tb, dy, oihw, pk, true, [](size_t, const lq::Task&) { return LQ_OK; }))) return rc;
    CoefPack cf;
    const int nt = (int)tb.h.size();
    if (oihw)
        hipLaunchKernelGGL((k_batch_traverse<OP_BWD_PERM>), dim3(tb.blocks), dim3(kBlock), 0, (hipStream_t)stream, tb.d, tb.block_task_d, nt,
                           (uint32_t*)ws, pk, oihw ? 3 : 1, cf);
    else
        hipLaunchKernelGGL((k_batch_traverse<OP_BWD>), dim3(tb.blocks), dim3(kBlock), 0, (hipStream_t)stream, tb.d, tb.block_task_d, nt,
                           (uint32_t*)ws, pk, 1, cf);
    if ((rc = check_hip("batch scale-grad launch"))) return rc;
    hipLaunchKernelGGL((k_batch_finalize_t<OP_BWD>), dim3(tb.fin_blocks), dim3(256), 0, (hipStream_t)stream, tb.fin_blocks_d, (uint32_t*)ws, ah);
    return check_hip("batch finalize launch");
}

extern "C" {

int lq_batch_scale_grad(const lq_batch* b, const float* const* dy, void* ws, size_t ws_bytes, void* stream) {
    return batch_scale_grad(b, dy, ws, ws_bytes, stream, false, adam_hyper(0, 0, 0, 0, 1, nullptr, LQ_ADAM_KERAS, 0));
}

int lq_batch_scale_grad_oihw(const lq_batch* b, const float* const* dy, void* ws, size_t ws_bytes, void* stream) {
    return batch_scale_grad(b, dy, ws, ws_bytes, stream, b && b->has_perm, adam_hyper(0, 0, 0, 0, 1, nullptr, LQ_ADAM_KERAS, 0));
}

int lq_batch_scale_grad_step(const lq_batch* b, const float* const* dy, int dy_oihw, void* ws, size_t ws_bytes, double lr, double beta1,
                             double beta2, double eps, int64_t step, const int64_t* step_dev, int mode, void* stream) {
    if (!b) return fail(LQ_EINVAL, "lq_batch_scale_grad_step: NULL batch");
    if (!step_dev && step < 1) return fail(LQ_EINVAL, "lq_batch_scale_grad_step: step is 1-based");
    if (mode != LQ_ADAM_KERAS && mode != LQ_ADAM_TORCH) return fail(LQ_EINVAL, "lq_batch_scale_grad_step: bad mode %d", mode);
    // every scale the separate Adam launch would update must be one whose gradient this pass computes
    size_t with_state = 0;
    for (const lq::Task& t : b->bwd.h) with_state += t.am ? 1 : 0;
    if (with_state != b->adam_h.size() || with_state != b->bwd.h.size())
        return fail(LQ_EINVAL, "lq_batch_scale_grad_step: every tensor of the batch needs lambda, ds and Adam state (%zu of %zu have them)",
                    with_state, b->adam_h.size() > b->bwd.h.size() ? b->adam_h.size() : b->bwd.h.size());
    return batch_scale_grad(b, dy, ws, ws_bytes, stream, dy_oihw && b->has_perm, adam_hyper(lr, beta1, beta2, eps, step, step_dev, mode, 1));
}

}  // extern "C"

// Value outputs of the penalty entry points (lq_hip.h: lq_batch_penalty_values, lq_batch_penalty_grads_values).
struct PenaltyValueArgs {
    const float* dims;
    const uint8_t* layer_start;
    float* terms;
    float* penalty;
};

// everything that can be said about the arguments without the batch: kind first, then the outputs
static int check_penalty_value_args(const char* fn, int kind, const PenaltyValueArgs& va) {
    if (kind < LQ_PENALTY_MAXBIN || kind > LQ_PENALTY_INVERSE) return fail(LQ_EINVAL, "%s: bad kind %d", fn, kind);
    if (!va.terms) return fail(LQ_EINVAL, "%s: terms_dev is NULL", fn);
    if (!va.penalty) return fail(LQ_EINVAL, "%s: penalty_dev is NULL", fn);
    if (!aligned(va.terms, 4) || !aligned(va.penalty, 4)) return fail(LQ_EALIGN, "%s: terms_dev / penalty_dev must be 4-byte aligned", fn);
    if (!va.dims) return fail(LQ_EINVAL, "%s: dims is NULL", fn);
    if (!va.layer_start) return fail(LQ_EINVAL, "%s: layer_start is NULL", fn);
    return LQ_OK;
}

// The value launches.  `have_mb`: the gradient launches of this call have just left, for every group, mb[g] (MaxBin) or the mean
// |P - P/s| (Difference, co-emitted by OP_DIFF_BWD_V) in the batch's buffer.  Without them (values only) a forward traversal of
// the batch and its finalize produce the same numbers first.
static int launch_penalty_values(const char* fn, const lq_batch* b, int kind, const PenaltyValueArgs& va, void* ws, bool have_mb, hipStream_t st) {
    const lq_task_table& tb = b->pen;
    const int nt = (int)tb.h.size();
    const uint32_t* gpre = tb.prefix_d + nt;
    CoefPack cf;
    PtrPack none;
    memset(&cf, 0, sizeof(cf));
    memset(&none, 0, sizeof(none));
    if (kind == LQ_PENALTY_MAXBIN && !have_mb) {
        hipLaunchKernelGGL((k_batch_traverse<OP_MAXBIN_FWD>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, none, 0, cf);
        hipLaunchKernelGGL((k_batch_finalize<OP_MAXBIN_FWD>), dim3(tb.groups), dim3(64), 0, st, tb.d, gpre, nt, (uint32_t*)ws, 0);
    } else if (kind == LQ_PENALTY_DIFFERENCE && !have_mb) {
        hipLaunchKernelGGL((k_batch_traverse<OP_DIFF_FWD>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, none, 0, cf);
        hipLaunchKernelGGL((k_batch_finalize<OP_DIFF_FWD>), dim3(tb.groups), dim3(64), 0, st, tb.d, gpre, nt, (uint32_t*)ws, 0);
    }
    TermPack tp;
    CombinePack cp;
    memset(&tp, 0, sizeof(tp));
    memset(&cp, 0, sizeof(cp));
    double normalizer = 0.0;                                    // custom_loss_functions.py:114, a Python float
    for (int i = 0; i < nt; ++i) {
        tp.index[i] = (uint16_t)tb.index[i];
        cp.dim[i] = va.dims[i];
        cp.start[i] = va.layer_start[i] ? 1 : 0;
        normalizer += (double)va.dims[i];
    }
    hipLaunchKernelGGL(k_batch_penalty_terms, dim3(nt), dim3(kBlock), 0, st, tb.d, kind, tp, va.terms);
    hipLaunchKernelGGL(k_batch_penalty_combine, dim3(1), dim3(kBatchMax), 0, st, va.terms, nt, cp, (float)normalizer, va.penalty);
    return check_hip(fn);
}

static int batch_penalty_grads(const char* fn, const lq_batch* b, int kind, const float* coeff, float* const* grad, void* ws, size_t ws_bytes,
                               void* stream, const PenaltyValueArgs* va) {
    if (va) {
        const int rc = check_penalty_value_args(fn, kind & ~LQ_PENALTY_ACCUMULATE_DS, *va);
        if (rc) return rc;
    }
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    const int accum = (kind & LQ_PENALTY_ACCUMULATE_DS) ? 1 : 0;
    kind &= ~LQ_PENALTY_ACCUMULATE_DS;
    if (kind < LQ_PENALTY_MAXBIN || kind > LQ_PENALTY_INVERSE) return fail(LQ_EINVAL, "%s: bad kind %d", fn, kind);
    if (!coeff) return fail(LQ_EINVAL, "%s: coeff is NULL", fn);
    const lq_task_table& tb = b->pen;
    if (tb.h.size() != (size_t)b->n) return fail(LQ_EINVAL, "%s: every tensor of the batch needs a ds buffer", fn);
    CoefPack cf;
    PtrPack pk;
    memset(&pk, 0, sizeof(pk));
    memset(&cf, 0, sizeof(cf));
    const int nt = (int)tb.h.size();
    for (int i = 0; i < nt; ++i) cf.c[i] = coeff[tb.index[i]];
    hipStream_t st = (hipStream_t)stream;
    if (kind != LQ_PENALTY_INVERSE) {
        if (!grad) return fail(LQ_EINVAL, "%s: grad pointers are NULL", fn);
        if (const int rc = check_batch_workspace(fn, b, ws, ws_bytes)) return rc;
        for (int i = 0; i < nt; ++i) {
            float* gi = grad[tb.index[i]];
            if (!gi || !aligned(gi, 4)) return fail(LQ_EINVAL, "%s: gradient buffer of tensor %d missing", fn, tb.index[i]);
            if (task_wants16(tb.h[i]) && !aligned(gi, 16)) return fail(LQ_EALIGN, "%s: gradient buffer of tensor %d is not 16-byte aligned", fn, tb.index[i]);
            pk.dy[i] = gi;
        }
    }
    const uint32_t* gpre = tb.prefix_d + nt;
    if (kind == LQ_PENALTY_MAXBIN) {
        PtrPack none;
        memset(&none, 0, sizeof(none));
        hipLaunchKernelGGL((k_batch_traverse<OP_MAXBIN_FWD>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, none, 0, cf);
        hipLaunchKernelGGL((k_batch_finalize<OP_MAXBIN_FWD>), dim3(tb.groups), dim3(64), 0, st, tb.d, gpre, nt, (uint32_t*)ws, 0);
        hipLaunchKernelGGL((k_batch_traverse<OP_MAXBIN_BWD>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, pk, 2, cf);
        hipLaunchKernelGGL(k_batch_penalty_ds, dim3((unsigned)ceil_div(tb.groups, kBlock)), dim3(kBlock), 0, st, tb.d, gpre, nt, tb.groups, 0, cf, accum);
    } else if (kind == LQ_PENALTY_DIFFERENCE) {
        if (va) {
            // the same traversal with a second accumulator (sum |u| next to sum gi * (P/s) / s: OP_DIFF_BWD_V, lq_ops.hpp); its
            // partials go to the second slice of every task; one finalize launch emits ds and, into the mb buffer, the groups' mean |u|
            if (tb.groups > 0x3fffffffu) return fail(LQ_EINVAL, "%s: too many groups for the two-slice finalize (%u)", fn, tb.groups);
            hipLaunchKernelGGL((k_batch_traverse<OP_DIFF_BWD_V>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, pk, 2, cf);
            hipLaunchKernelGGL(k_batch_finalize_diff_v, dim3(2 * tb.groups), dim3(64), 0, st, tb.d, gpre, nt, (uint32_t*)ws, accum, tb.groups);
        } else {
            hipLaunchKernelGGL((k_batch_traverse<OP_DIFF_BWD>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, pk, 2, cf);
            hipLaunchKernelGGL((k_batch_finalize<OP_DIFF_BWD>), dim3(tb.groups), dim3(64), 0, st, tb.d, gpre, nt, (uint32_t*)ws, accum);
        }
    } else {
        hipLaunchKernelGGL(k_batch_penalty_ds, dim3((unsigned)ceil_div(tb.groups, kBlock)), dim3(kBlock), 0, st, tb.d, gpre, nt, tb.groups, 2, cf, accum);
    }
    int rc = check_hip("batch penalty launch");
    if (rc || !va) return rc;
    return launch_penalty_values(fn, b, kind, *va, ws, kind != LQ_PENALTY_INVERSE, st);
}

extern "C" {

int lq_batch_penalty_grads(const lq_batch* b, int kind, const float* coeff, float* const* grad, void* ws, size_t ws_bytes,
                           void* stream) {
    return batch_penalty_grads("lq_batch_penalty_grads", b, kind, coeff, grad, ws, ws_bytes, stream, nullptr);
}

int lq_batch_penalty_grads_values(const lq_batch* b, int kind, const float* coeff, float* const* grad, const float* dims,
                                  const uint8_t* layer_start, float* terms_dev, float* penalty_dev, void* ws, size_t ws_bytes,
                                  void* stream) {
    const PenaltyValueArgs va = {dims, layer_start, terms_dev, penalty_dev};
    return batch_penalty_grads("lq_batch_penalty_grads_values", b, kind, coeff, grad, ws, ws_bytes, stream, &va);
}

int lq_batch_penalty_values(const lq_batch* b, int kind, const float* dims, const uint8_t* layer_start, float* terms_dev,
                            float* penalty_dev, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "lq_batch_penalty_values";
    const PenaltyValueArgs va = {dims, layer_start, terms_dev, penalty_dev};
    int rc = check_penalty_value_args(fn, kind, va);
    if (rc) return rc;
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    if (b->pen.h.size() != (size_t)b->n) return fail(LQ_EINVAL, "%s: every tensor of the batch needs a ds buffer", fn);
    if (kind != LQ_PENALTY_INVERSE && (rc = check_batch_workspace(fn, b, ws, ws_bytes))) return rc;
    return launch_penalty_values(fn, b, kind, va, ws, false, (hipStream_t)stream);
}

// Runs on the `pen` table: every tensor with a ds buffer, generic traversal bodies and partial layout, whatever its lambda.
int lq_batch_scale_grad_ste(const lq_batch* b, const float* const* dy, const float* grad_scale, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "lq_batch_scale_grad_ste";
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    const lq_task_table& tb = b->pen;
    if (tb.h.empty()) return LQ_OK;
    int rc = check_batch_workspace(fn, b, ws, ws_bytes);
    if (rc) return rc;
    PtrPack pk;
    CoefPack cf;
    memset(&pk, 0, sizeof(pk));
    memset(&cf, 0, sizeof(cf));
    const int nt = (int)tb.h.size();
    rc = gather_dy(fn, tb, dy, false, pk, false, [&](size_t i, const Task&) {
        cf.c[i] = grad_scale ? grad_scale[tb.index[i]] : 1.0f;
        return LQ_OK;
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((k_batch_traverse<OP_STE_SCALE>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, pk, 1, cf);
    if ((rc = check_hip("batch STE scale-grad launch"))) return rc;
    hipLaunchKernelGGL(k_batch_finalize_ste, dim3(tb.groups), dim3(64), 0, st, tb.d, tb.prefix_d + nt, nt, (uint32_t*)ws, cf);
    return check_hip("batch STE finalize launch");
}

// ---- clipped b-bit tensors in the batch (lq_hip.h: lq_batch_set_clip) ----

int lq_batch_set_clip(lq_batch* b, const int32_t* qmin, const int32_t* qmax, int n, int rounding) {
    const char* fn = "lq_batch_set_clip";
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    if (!qmin || !qmax) return fail(LQ_EINVAL, "%s: qmin / qmax is NULL", fn);
    if (n != b->n) return fail(LQ_EINVAL, "%s: %d ranges for a batch of %d tensors", fn, n, b->n);
    int rc = check_rounding(fn, rounding);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        const lq_tensor_desc& d = b->descs[i];
        if ((rc = check_clip_range(fn, qmin[i], qmax[i]))) return rc;
        if (d.conv_co != 0) return fail(LQ_EINVAL, "%s: tensor %d has an OIHW companion (conv extents); the clipped pair takes conv kernels stored OIHW", fn, i);
        if (!d.out) return fail(LQ_EINVAL, "%s: tensor %d has no out buffer", fn, i);
        if (!d.dp) return fail(LQ_EINVAL, "%s: tensor %d has no dp buffer", fn, i);
        if (!aligned(d.dp, 4)) return fail(LQ_EALIGN, "%s: dp of tensor %d is not 4-byte aligned", fn, i);
        if (d.ds && !aligned(d.ds, 4)) return fail(LQ_EALIGN, "%s: ds of tensor %d is not 4-byte aligned", fn, i);
    }
    // tables of their own, sized per tensor (batch_w = 0: no batch-sized units, no periodic stream, no fragment layout): the forms
    // of the single-tensor clipped pair.  The forward table's plan looks at `out`; the backward's looks at P only, so the stored
    // destination is checked here: never a misaligned vector store.
    lq_task_table cf, cb;
    uint32_t* counts = nullptr;
    for (int i = 0; i < n && !rc; ++i) {
        const lq_tensor_desc& d = b->descs[i];
        Task t;
        if ((rc = fill_task(t, d, false, false, cf))) break;
        t.p.clip_lo = (float)qmin[i];
        t.p.clip_hi = (float)qmax[i];
        cf.h.push_back(t);
        cf.index.push_back(i);
        if ((rc = fill_task(t, d, true, false, cb))) break;
        t.p.clip_lo = (float)qmin[i];
        t.p.clip_hi = (float)qmax[i];
        t.dp = d.dp;
        if (task_wants16(t) && !aligned(d.dp, 16)) {
            rc = fail(LQ_EALIGN, "%s: tensor %d is traversed with 16-byte accesses but its dp is not 16-byte aligned", fn, i);
            break;
        }
        cb.h.push_back(t);
        cb.index.push_back(i);
    }
    if (!rc) rc = finish_table(cf, false);
    if (!rc) rc = finish_table(cb, true);
    if (!rc) {
        if (hipMalloc(&counts, (size_t)cb.groups * sizeof(uint32_t)) != hipSuccess) rc = fail(LQ_EHIP, "%s: out of device memory", fn);
        else if (hipMemset(counts, 0, (size_t)cb.groups * sizeof(uint32_t)) != hipSuccess) rc = fail(LQ_EHIP, "%s: hipMemset failed", fn);
    }
    if (!rc) {
        for (Task& t : cb.h) t.ties = counts + t.first_group;      // the finalize's count output (batch_finalize_body)
        rc = upload_table(cf);
    }
    if (!rc) rc = upload_table(cb);
    if (rc) {
        free_table(cf);
        free_table(cb);
        if (counts) (void)hipFree(counts);
        return rc;
    }
    free_table(b->cfwd);            // a repeated call replaces the ranges (hipFree waits for the device)
    free_table(b->cbwd);
    if (b->clip_d) (void)hipFree(b->clip_d);
    b->cfwd = cf;
    b->cbwd = cb;
    b->clip_d = counts;
    b->clip_rounding = rounding;
    b->has_clip = true;
    const size_t need = (size_t)cb.ws_words * 4 + 256;
    if (need > b->ws_bytes) b->ws_bytes = need;
    return LQ_OK;
}

int lq_batch_forward_clip(const lq_batch* b, void* stream) {
    const char* fn = "lq_batch_forward_clip";
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    if (!b->has_clip) return fail(LQ_EINVAL, "%s: the batch has no ranges (lq_batch_set_clip)", fn);
    PtrPack pk;
    CoefPack cf;
    memset(&pk, 0, sizeof(pk));
    memset(&cf, 0, sizeof(cf));
    const lq_task_table& tb = b->cfwd;
    const int nt = (int)tb.h.size();
    hipStream_t st = (hipStream_t)stream;
    if (b->clip_rounding == LQ_ROUND_NEAREST_EVEN)
        hipLaunchKernelGGL((k_batch_traverse<OP_CLIP_FWD_RNE>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)nullptr, pk, 0, cf);
    else
        hipLaunchKernelGGL((k_batch_traverse<OP_CLIP_FWD>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)nullptr, pk, 0, cf);
    return check_hip("batch clipped forward launch");
}

int lq_batch_backward_clip(const lq_batch* b, const float* const* dy, const float* grad_scale, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "lq_batch_backward_clip";
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    if (!b->has_clip) return fail(LQ_EINVAL, "%s: the batch has no ranges (lq_batch_set_clip)", fn);
    const lq_task_table& tb = b->cbwd;
    int rc = check_batch_workspace(fn, b, ws, ws_bytes);
    if (rc) return rc;
    PtrPack pk;
    CoefPack cf;
    memset(&pk, 0, sizeof(pk));
    memset(&cf, 0, sizeof(cf));
    const int nt = (int)tb.h.size();
    rc = gather_dy(fn, tb, dy, false, pk, false, [&](size_t i, const Task& t) {
        if (grad_scale && !t.ds) return fail(LQ_EINVAL, "%s: tensor %d has no ds buffer (pass grad_scale = NULL for the mask alone)", fn, tb.index[i]);
        cf.c[i] = grad_scale ? grad_scale[tb.index[i]] : 0.0f;
        return (int)LQ_OK;
    });
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (b->clip_rounding == LQ_ROUND_NEAREST_EVEN)
        hipLaunchKernelGGL((k_batch_traverse<OP_CLIP_BWD_RNE>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, pk, 0, cf);
    else
        hipLaunchKernelGGL((k_batch_traverse<OP_CLIP_BWD>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, nt, (uint32_t*)ws, pk, 0, cf);
    if ((rc = check_hip("batch clipped backward launch"))) return rc;
    hipLaunchKernelGGL(k_batch_finalize_clip, dim3(tb.groups), dim3(64), 0, st, tb.d, tb.prefix_d + nt, nt, (uint32_t*)ws, cf, grad_scale ? 0 : 1);
    return check_hip("batch clipped finalize launch");
}

int lq_batch_clip_counts(const lq_batch* b, int tensor, const uint32_t** dev, int64_t* groups) {
    const char* fn = "lq_batch_clip_counts";
    if (!b || !dev || !groups) return fail(LQ_EINVAL, "%s: NULL argument", fn);
    if (!b->has_clip) return fail(LQ_EINVAL, "%s: the batch has no ranges (lq_batch_set_clip)", fn);
    if (tensor < 0 || tensor >= b->n) return fail(LQ_EINVAL, "%s: tensor %d of %d", fn, tensor, b->n);
    const lq_task_table& tb = b->cbwd;
    for (size_t k = 0; k < tb.h.size(); ++k) {
        if (tb.index[k] != tensor) continue;
        *dev = tb.h[k].ties;
        *groups = tb.h[k].p.G;
        return LQ_OK;
    }
    return fail(LQ_EINVAL, "%s: tensor %d is not in the clipped tables", fn, tensor);
}

// ------------------------------------------------------------------------------------------
//  lq_group_batch: group-wise tensors, one launch per pass (lq_group_batch.hpp)
// ------------------------------------------------------------------------------------------
}  // extern "C"

struct lq_group_table {
    std::vector<lq::GroupTask> h;
    std::vector<int> index;               // table position -> descriptor index (tasks are ordered by work per block)
    lq::GroupTask* d = nullptr;           // a batch without offsets
    lq::GroupAffineTask* da = nullptr;    // a batch with offsets: the same tasks, each with its b, db and kb
    lq::GroupMxTask* dm = nullptr;        // a microscaling batch: the same tasks, each with its format
    uint32_t* block_task_d = nullptr;     // [blocks] task of every block
    uint32_t blocks = 0;
};

struct lq_group_batch {
    int n = 0;
    int rounding = 0;
    bool affine = false;                  // some tensor has an offset: the tables are GroupAffineTask, the kernel k_group_batch_affine
    std::vector<lq_group_offset> offs;    // per descriptor; empty without offsets
    bool mx = false;                      // lq_group_batch_create_mx: the tables are GroupMxTask, the kernel k_group_batch_mx
    std::vector<lq_group_mx_format> fmts; // per descriptor; empty unless mx
    lq_group_table fwd, bwd;
    std::vector<const uint32_t*> counts;  // per descriptor: its slice of counts_d
    std::vector<int64_t> groups;          // per descriptor: scale elements
    uint32_t* counts_d = nullptr;
};

namespace lq {

// One task: the form lq_fq_*_group picks for this geometry and alignment (group_launch), and its blocks (left in first_block until
// the table is ordered): tiles * groups <= R * C < 2^31 elements, nz <= 4 only below 2048 blocks
static void fill_group_task(GroupTask& t, const GroupParams& p, int axis, bool vec, bool bwd) {
    const GroupLaunch L = group_launch(p, axis, vec, !bwd, kGroupEveryGroup);
    memset(&t, 0, sizeof(t));
    t.p = p;
    t.form = L.form;
    t.log_team = L.log_team;
    t.nbx = L.nbx;
    t.nz = L.nz;
    t.first_block = L.blocks;
}

// Orders the table so that the heaviest units start first (as finish_table), assigns the block prefix, uploads the block table and
// allocates the task table; affine: its entries are GroupAffineTask (a batch with offsets), mx: GroupMxTask, else GroupTask
static int finish_group_table(lq_group_table& tb, bool affine, bool mx) {
    const size_t n = tb.h.size();
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    auto weight = [&](size_t i) { return (double)tb.h[i].p.R * (double)tb.h[i].p.C / (double)tb.h[i].first_block; };      // elements per block
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weight(a) > weight(b); });
    std::vector<GroupTask> h2(n);
    std::vector<int> idx2(n);
    uint64_t bp = 0;
    for (size_t k = 0; k < n; ++k) {
        h2[k] = tb.h[order[k]];
        idx2[k] = tb.index[order[k]];
        const uint32_t nb = h2[k].first_block;
        h2[k].first_block = (uint32_t)bp;
        bp += nb;
        if (bp > 0x7fffffffull) return fail(LQ_EINVAL, "lq_group_batch_create: too many blocks");
    }
    tb.h.swap(h2);
    tb.index.swap(idx2);
    tb.blocks = (uint32_t)bp;
    std::vector<uint32_t> bt((size_t)bp);
    for (size_t k = 0; k < n; ++k) {
        const uint64_t end = k + 1 < n ? tb.h[k + 1].first_block : bp;
        for (uint64_t b = tb.h[k].first_block; b < end; ++b) bt[b] = (uint32_t)k;
    }
    hipError_t e = hipMalloc(&tb.block_task_d, bt.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(tb.block_task_d, bt.data(), bt.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = affine ? hipMalloc(&tb.da, n * sizeof(GroupAffineTask)) : (mx ? hipMalloc(&tb.dm, n * sizeof(GroupMxTask)) : hipMalloc(&tb.d, n * sizeof(GroupTask)));
    if (e != hipSuccess) return fail(LQ_EHIP, "lq_group_batch_create: %s", hipGetErrorString(e));
    return LQ_OK;
}

static void free_group_table(lq_group_table& tb) {
    if (tb.d) (void)hipFree(tb.d);
    if (tb.da) (void)hipFree(tb.da);
    if (tb.dm) (void)hipFree(tb.dm);
    if (tb.block_task_d) (void)hipFree(tb.block_task_d);
    tb.d = nullptr;
    tb.da = nullptr;
    tb.dm = nullptr;
    tb.block_task_d = nullptr;
}

}  // namespace lq

extern "C" {

// lq_group_batch_create, lq_group_batch_create_affine and lq_group_batch_create_mx.  offs == NULL, or no tensor with a b: the
// tables and the kernel of a batch without offsets.  mx: fmts holds every tensor's format, the range is the format's and the
// descriptor's qmin / qmax are not read
static int group_batch_create(const char* fn, const lq_group_desc* descs, const lq_group_offset* offs, const lq_group_mx_format* fmts,
                              bool mx, int n, int rounding, lq_group_batch** out) {
    if (!out) return fail(LQ_EINVAL, "%s: out is NULL", fn);
    *out = nullptr;
    if (!descs) return fail(LQ_EINVAL, "%s: descs is NULL", fn);
    if (mx && !fmts) return fail(LQ_EINVAL, "%s: fmts is NULL", fn);
    if (n < 1 || n > kBatchMax) return fail(LQ_EINVAL, "%s: %d tensors (1 .. %d)", fn, n, kBatchMax);
    int rc = check_rounding(fn, rounding);
    if (rc) return rc;
    // everything is validated before the first HIP call
    for (int i = 0; i < n; ++i) {
        const lq_group_desc& d = descs[i];
        char who[64];
        snprintf(who, sizeof(who), "%s: tensor %d", fn, i);
        if (!d.P || !d.s || !d.out || !d.dp)
            return fail(LQ_EINVAL, "%s: %s is NULL", who, !d.P ? "P" : (!d.s ? "s" : (!d.out ? "out" : "dp")));
        if (!aligned(d.P, 4) || !aligned(d.s, 4) || !aligned(d.out, 4) || !aligned(d.dp, 4) || (d.ds && !aligned(d.ds, 4)))
            return fail(LQ_EALIGN, "%s: P, s, out, dp and ds must be 4-byte aligned", who);
        if ((rc = check_group(who, d.R, d.C, d.axis, d.gs))) return rc;
        rc = mx ? check_mx(who, fmts[i].format, fmts[i].scale_format) : check_clip_range(who, d.qmin, d.qmax);
        if (rc) return rc;
    }
    bool affine = false;
    for (int i = 0; offs && i < n; ++i) {
        const lq_group_offset& o = offs[i];
        if (o.db && !o.b) return fail(LQ_EINVAL, "%s: tensor %d has a db but no offset b", fn, i);
        if (o.b && !std::isfinite(o.offset_grad_scale))
            return fail(LQ_EINVAL, "%s: tensor %d: offset_grad_scale %g is not finite", fn, i, (double)o.offset_grad_scale);
        if ((o.b && !aligned(o.b, 4)) || (o.db && !aligned(o.db, 4)))
            return fail(LQ_EALIGN, "%s: tensor %d: b and db must be 4-byte aligned", fn, i);
        affine = affine || o.b != nullptr;
    }
    lq_group_batch* b = new (std::nothrow) lq_group_batch();
    if (!b) return fail(LQ_EHIP, "%s: out of host memory", fn);
    b->n = n;
    b->rounding = rounding;
    b->affine = affine;
    if (affine) b->offs.assign(offs, offs + n);
    b->mx = mx;
    if (mx) b->fmts.assign(fmts, fmts + n);
    b->counts.resize(n);
    b->groups.resize(n);
    int64_t total = 0;
    std::vector<int64_t> first(n);
    for (int i = 0; i < n; ++i) {
        const lq_group_desc& d = descs[i];
        const GroupParams p = group_params(d.P, d.s, 0, 0, d.R, d.C, d.axis, d.gs);      // the geometry alone
        first[i] = total;
        b->groups[i] = d.axis == 0 ? (int64_t)p.nb * p.C : (int64_t)p.R * p.nb;
        total += b->groups[i];
    }
    if (hipMalloc(&b->counts_d, (size_t)total * sizeof(uint32_t)) != hipSuccess) rc = fail(LQ_EHIP, "%s: out of device memory", fn);
    else if (hipMemset(b->counts_d, 0, (size_t)total * sizeof(uint32_t)) != hipSuccess) rc = fail(LQ_EHIP, "%s: hipMemset failed", fn);
    for (int i = 0; i < n && !rc; ++i) {
        const lq_group_desc& d = descs[i];
        b->counts[i] = b->counts_d + first[i];
        GroupParams p = group_params(d.P, d.s, mx ? 0 : d.qmin, mx ? 0 : d.qmax, d.R, d.C, d.axis, d.gs);
        if (mx) {      // lo = -max, hi = +max of the tensor's format, as lq_fq_*_mx
            p.lo = -kMxFormats[fmts[i].format].mx;
            p.hi = kMxFormats[fmts[i].format].mx;
        }
        GroupTask t;
        p.out = d.out;
        fill_group_task(t, p, d.axis, group_vec_ok(p, d.axis) && aligned(d.P, 16) && aligned(d.out, 16), false);
        b->fwd.h.push_back(t);
        b->fwd.index.push_back(i);
        p.out = d.dp;            // dy and grad_scale arrive with the call
        p.ds = d.ds;
        p.clipped = b->counts_d + first[i];
        fill_group_task(t, p, d.axis, group_vec_ok(p, d.axis) && aligned(d.P, 16) && aligned(d.dp, 16), true);
        b->bwd.h.push_back(t);
        b->bwd.index.push_back(i);
    }
    for (lq_group_table* tb : {&b->fwd, &b->bwd}) {
        if (!rc) rc = finish_group_table(*tb, affine, mx);
        if (rc) break;
        hipError_t e;
        if (affine) {      // the ordered tasks, each with its descriptor's offset; db only where the backward writes it
            std::vector<GroupAffineTask> ha(tb->h.size());
            for (size_t k = 0; k < ha.size(); ++k) {
                const lq_group_offset& o = b->offs[tb->index[k]];
                memset(&ha[k], 0, sizeof(GroupAffineTask));
                ha[k].t = tb->h[k];
                ha[k].b = o.b;
                ha[k].db = tb == &b->bwd ? o.db : nullptr;
                ha[k].kb = o.b ? o.offset_grad_scale : 0.0f;
            }
            e = hipMemcpy(tb->da, ha.data(), ha.size() * sizeof(GroupAffineTask), hipMemcpyHostToDevice);
        } else if (mx) {      // the ordered tasks, each with its descriptor's format
            std::vector<GroupMxTask> hm(tb->h.size());
            for (size_t k = 0; k < hm.size(); ++k) {
                const lq_group_mx_format& f = b->fmts[tb->index[k]];
                GroupMxParams mp{};
                mx_fill(mp, f.format, f.scale_format);
                memset(&hm[k], 0, sizeof(GroupMxTask));
                hm[k].t = tb->h[k];
                hm[k].M = mp.M;
                hm[k].emin = mp.emin;
                hm[k].bits = mp.bits;
                hm[k].e8m0_mask = mp.e8m0_mask;
            }
            e = hipMemcpy(tb->dm, hm.data(), hm.size() * sizeof(GroupMxTask), hipMemcpyHostToDevice);
        } else {
            e = hipMemcpy(tb->d, tb->h.data(), tb->h.size() * sizeof(GroupTask), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) rc = fail(LQ_EHIP, "%s: table upload failed", fn);
    }
    if (rc) {
        (void)lq_group_batch_destroy(b);
        return rc;
    }
    *out = b;
    return LQ_OK;
}

int lq_group_batch_create(const lq_group_desc* descs, int n, int rounding, lq_group_batch** out) {
    return group_batch_create("lq_group_batch_create", descs, nullptr, nullptr, false, n, rounding, out);
}

int lq_group_batch_create_affine(const lq_group_desc* descs, const lq_group_offset* offs, int n, int rounding, lq_group_batch** out) {
    return group_batch_create("lq_group_batch_create_affine", descs, offs, nullptr, false, n, rounding, out);
}

int lq_group_batch_create_mx(const lq_group_desc* descs, const lq_group_mx_format* fmts, int n, lq_group_batch** out) {
    return group_batch_create("lq_group_batch_create_mx", descs, nullptr, fmts, true, n, LQ_ROUND_NEAREST_EVEN, out);
}

int lq_group_batch_destroy(lq_group_batch* b) {
    if (!b) return fail(LQ_EINVAL, "lq_group_batch_destroy: NULL batch");
    free_group_table(b->fwd);
    free_group_table(b->bwd);
    if (b->counts_d) (void)hipFree(b->counts_d);
    delete b;
    return LQ_OK;
}

size_t lq_group_batch_workspace_bytes(const lq_group_batch* b) {
    (void)b;
    return 0;      // every form is single-stage (lq_group.hpp)
}

int lq_group_batch_forward(const lq_group_batch* b, void* stream) {
    if (!b) return fail(LQ_EINVAL, "lq_group_batch_forward: NULL batch");
    PtrPack pk;
    CoefPack cf;
    memset(&pk, 0, sizeof(pk));
    memset(&cf, 0, sizeof(cf));
    const lq_group_table& tb = b->fwd;
    hipStream_t st = (hipStream_t)stream;
    const bool rne = b->rounding == LQ_ROUND_NEAREST_EVEN;
    if (b->mx) {
        hipLaunchKernelGGL((k_group_batch_mx<false>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.dm, tb.block_task_d, pk, cf, 0);
    } else if (b->affine) {
        if (rne) hipLaunchKernelGGL((k_group_batch_affine<true, false>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.da, tb.block_task_d, pk, cf, 0);
        else hipLaunchKernelGGL((k_group_batch_affine<false, false>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.da, tb.block_task_d, pk, cf, 0);
    } else if (rne)
        hipLaunchKernelGGL((k_group_batch<true, false>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, pk, cf, 0);
    else
        hipLaunchKernelGGL((k_group_batch<false, false>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, pk, cf, 0);
    return check_hip("group batch forward launch");
}

int lq_group_batch_backward(const lq_group_batch* b, const float* const* dy, const float* grad_scale, void* ws, size_t ws_bytes,
                            void* stream) {
    const char* fn = "lq_group_batch_backward";
    (void)ws; (void)ws_bytes;      // lq_group_batch_workspace_bytes() == 0: ws may be NULL and is never touched
    if (!b) return fail(LQ_EINVAL, "%s: NULL batch", fn);
    if (!dy) return fail(LQ_EINVAL, "%s: dy is NULL", fn);
    PtrPack pk;
    CoefPack cf;
    memset(&pk, 0, sizeof(pk));
    memset(&cf, 0, sizeof(cf));
    const lq_group_table& tb = b->bwd;
    for (size_t k = 0; k < tb.h.size(); ++k) {
        const GroupTask& t = tb.h[k];
        const int i = tb.index[k];
        const float* d = dy[i];
        if (!d) return fail(LQ_EINVAL, "%s: no upstream gradient for tensor %d", fn, i);
        if (!aligned(d, 4)) return fail(LQ_EALIGN, "%s: dy of tensor %d is not 4-byte aligned", fn, i);
        if ((t.form == GROUP_COLS4 || t.form == GROUP_ROWS4) && !aligned(d, 16))
            return fail(LQ_EALIGN, "%s: tensor %d is traversed with 16-byte accesses but its dy is not 16-byte aligned", fn, i);
        if (grad_scale && !t.p.ds) return fail(LQ_EINVAL, "%s: tensor %d has no ds buffer (pass grad_scale = NULL for the mask alone)", fn, i);
        pk.dy[k] = d;
        cf.c[k] = grad_scale ? grad_scale[i] : 0.0f;
    }
    hipStream_t st = (hipStream_t)stream;
    const int mask_only = grad_scale ? 0 : 1;
    const bool rne = b->rounding == LQ_ROUND_NEAREST_EVEN;
    if (b->mx) {
        hipLaunchKernelGGL((k_group_batch_mx<true>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.dm, tb.block_task_d, pk, cf, mask_only);
    } else if (b->affine) {
        if (rne) hipLaunchKernelGGL((k_group_batch_affine<true, true>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.da, tb.block_task_d, pk, cf, mask_only);
        else hipLaunchKernelGGL((k_group_batch_affine<false, true>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.da, tb.block_task_d, pk, cf, mask_only);
    } else if (rne)
        hipLaunchKernelGGL((k_group_batch<true, true>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, pk, cf, mask_only);
    else
        hipLaunchKernelGGL((k_group_batch<false, true>), dim3(tb.blocks), dim3(kBlock), 0, st, tb.d, tb.block_task_d, pk, cf, mask_only);
    return check_hip("group batch backward launch");
}

int lq_group_batch_clip_counts(const lq_group_batch* b, int tensor, const uint32_t** dev, int64_t* groups) {
    const char* fn = "lq_group_batch_clip_counts";
    if (!b || !dev || !groups) return fail(LQ_EINVAL, "%s: NULL argument", fn);
    if (tensor < 0 || tensor >= b->n) return fail(LQ_EINVAL, "%s: tensor %d of %d", fn, tensor, b->n);
    *dev = b->counts[tensor];
    *groups = b->groups[tensor];
    return LQ_OK;
}

int lq_loss_log_append(const float* scce_dev, const float* penalty_dev, float rate, float* rows_dev, int64_t capacity,
                       int64_t* cursor_dev, float* last_dev, void* stream) {
    if (!scce_dev || !penalty_dev) return fail(LQ_EINVAL, "lq_loss_log_append: scce_dev / penalty_dev is NULL");
    if (!rows_dev) return fail(LQ_EINVAL, "lq_loss_log_append: rows_dev is NULL");
    if (!cursor_dev) return fail(LQ_EINVAL, "lq_loss_log_append: cursor_dev is NULL");
    if (capacity <= 0) return fail(LQ_EINVAL, "lq_loss_log_append: capacity must be positive");
    if (!aligned(scce_dev, 4) || !aligned(penalty_dev, 4) || !aligned(rows_dev, 4) || !aligned(last_dev, 4))
        return fail(LQ_EALIGN, "lq_loss_log_append: scce_dev, penalty_dev, rows_dev and last_dev must be 4-byte aligned");
    if (!aligned(cursor_dev, 8)) return fail(LQ_EALIGN, "lq_loss_log_append: cursor_dev must be 8-byte aligned (two int64)");
    hipLaunchKernelGGL(k_loss_log_append, dim3(1), dim3(64), 0, (hipStream_t)stream, scce_dev, penalty_dev, rate, rows_dev, capacity, cursor_dev,
                       last_dev);
    return check_hip("lq_loss_log_append");
}

int lq_batch_scale_adam(const lq_batch* b, double lr, double beta1, double beta2, double eps, int64_t step,
                        const int64_t* step_dev, int mode, void* stream) {
    if (!b) return fail(LQ_EINVAL, "lq_batch_scale_adam: NULL batch");
    if (b->adam_h.empty()) return LQ_OK;
    if (!step_dev && step < 1) return fail(LQ_EINVAL, "lq_batch_scale_adam: step is 1-based");
    if (mode != LQ_ADAM_KERAS && mode != LQ_ADAM_TORCH) return fail(LQ_EINVAL, "lq_batch_scale_adam: bad mode %d", mode);
    hipLaunchKernelGGL(k_batch_adam, dim3((unsigned)b->adam_h.size()), dim3(kBlock), 0, (hipStream_t)stream, b->adam_d,
                       adam_hyper(lr, beta1, beta2, eps, step, step_dev, mode, 1));
    return check_hip("batch adam launch");
}

int lq_selftest_ratio_division(uint64_t seed, uint32_t blocks, uint32_t pairs_per_thread, uint64_t* mismatches_dev, void* stream) {
    if (!mismatches_dev || !aligned(mismatches_dev, 8)) return fail(LQ_EINVAL, "lq_selftest_ratio_division: mismatches_dev must be an 8-byte aligned device pointer");
    if (blocks == 0 || pairs_per_thread == 0) return fail(LQ_EINVAL, "lq_selftest_ratio_division: empty test");
    hipLaunchKernelGGL(k_selftest_ratio_div, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, seed, pairs_per_thread,
                       reinterpret_cast<unsigned long long*>(mismatches_dev));
    return check_hip("selftest launch");
}

int lq_q_minmax(const float* P, const float* s, int32_t* minmax_dev, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(minmax_dev);
    const int64_t n = outer * G * inner;
    int64_t blocks = ceil_div(n, (int64_t)kBlock * 8);
    if (blocks > 1024) blocks = 1024;      // 4 blocks per CU; 2 x 1024 same-address atomics at the end
    // grid-stride index + stride stays below 2^32 for n < 2^31 (stride <= 1024 * 256)
    if (n < 2147483648ll) hipLaunchKernelGGL(k_q_minmax<uint32_t>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, P, s, minmax_dev, n, G, inner);
    else hipLaunchKernelGGL(k_q_minmax<int64_t>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, P, s, minmax_dev, n, G, inner);
    return check_hip("q minmax launch");
}

int lq_q_histogram(const float* P, const float* s, int32_t qmin, int64_t nbins, uint32_t* bins_dev, int64_t outer, int64_t G,
                   int64_t inner, void* stream) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    if (nbins <= 0) return fail(LQ_EINVAL, "lq_q_histogram: nbins must be positive");
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    LQ_REQUIRE_PTR(bins_dev);
    const int64_t n = outer * G * inner;
    int64_t blocks = ceil_div(n, (int64_t)kBlock * 16);
    if (blocks > 2048) blocks = 2048;
    if (n < 2147483648ll) hipLaunchKernelGGL(k_q_histogram<uint32_t>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, P, s, qmin, nbins, bins_dev, n, G, inner);
    else hipLaunchKernelGGL(k_q_histogram<int64_t>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, P, s, qmin, nbins, bins_dev, n, G, inner);
    return check_hip("q histogram launch");
}

static int check_pack(const char* fn, int bits, int64_t outer, int64_t G, int64_t inner) {
    int rc = check_desc(outer, G, inner);
    if (rc) return rc;
    if (bits < 0 || bits > 32) return fail(LQ_EINVAL, "%s: bits must be in 0..32, got %d", fn, bits);
    if (outer * G * inner > 2147483648ll) return fail(LQ_EINVAL, "%s: at most 2^31 elements (32-bit element indices)", fn);
    return LQ_OK;
}

static dim3 pack_grid(int64_t n) { return dim3((unsigned)ceil_div(n, (int64_t)kPackWaves * kPackElems)); }

int lq_q_pack(const float* P, const float* s, int32_t qmin, int bits, uint32_t* words, uint64_t* bad_dev, int64_t outer, int64_t G,
              int64_t inner, void* stream) {
    int rc = check_pack("lq_q_pack", bits, outer, G, inner);
    if (rc) return rc;
    LQ_REQUIRE_PTR(P);
    LQ_REQUIRE_PTR(s);
    if (!aligned(P, 16)) return fail(LQ_EALIGN, "lq_q_pack: P must be 16-byte aligned (float4 loads)");
    if (bits > 0) LQ_REQUIRE_PTR(words);
    if (!bad_dev) return fail(LQ_EINVAL, "lq_q_pack: argument 'bad_dev' is NULL");
    if (!aligned(bad_dev, 8)) return fail(LQ_EALIGN, "lq_q_pack: bad_dev must be 8-byte aligned");
    const int64_t n = outer * G * inner;
    hipLaunchKernelGGL(k_q_pack, pack_grid(n), dim3(kPackWaves * 64), 0, (hipStream_t)stream, P, s, qmin, bits, words,
                       reinterpret_cast<unsigned long long*>(bad_dev), (uint32_t)n, (uint64_t)((n * bits + 31) / 32),
                       make_fastdiv((uint32_t)inner), make_fastdiv((uint32_t)G));
    return check_hip("q pack launch");
}

int lq_q_unpack(const uint32_t* words, int32_t qmin, int bits, const float* s, float* out, int32_t* q, float* p_restore,
                uint64_t* bad_dev, int64_t outer, int64_t G, int64_t inner, void* stream) {
    int rc = check_pack("lq_q_unpack", bits, outer, G, inner);
    if (rc) return rc;
    if (bits > 0) LQ_REQUIRE_PTR(words);
    LQ_REQUIRE_PTR(s);
    if (!out && !q && !p_restore) return fail(LQ_EINVAL, "lq_q_unpack: out, q and p_restore are all NULL");
    if ((out && !aligned(out, 16)) || (q && !aligned(q, 16)) || (p_restore && !aligned(p_restore, 16)))
        return fail(LQ_EALIGN, "lq_q_unpack: out, q and p_restore must be 16-byte aligned (16-byte stores)");
    if (p_restore && !bad_dev) return fail(LQ_EINVAL, "lq_q_unpack: p_restore needs bad_dev (the check of every restored value)");
    if (bad_dev && !aligned(bad_dev, 8)) return fail(LQ_EALIGN, "lq_q_unpack: bad_dev must be 8-byte aligned");
    const int64_t n = outer * G * inner;
    hipLaunchKernelGGL(k_q_unpack, pack_grid(n), dim3(kPackWaves * 64), 0, (hipStream_t)stream, words, qmin, bits, s, out,
                       q, p_restore, reinterpret_cast<unsigned long long*>(bad_dev), (uint32_t)n,
                       (uint64_t)((n * bits + 31) / 32), make_fastdiv((uint32_t)inner), make_fastdiv((uint32_t)G));
    return check_hip("q unpack launch");
}

int lq_selftest_uniform_division(uint64_t seed, uint32_t blocks, uint32_t pairs_per_thread, uint64_t* mismatches_dev, void* stream) {
    if (!mismatches_dev || !aligned(mismatches_dev, 8)) return fail(LQ_EINVAL, "lq_selftest_uniform_division: mismatches_dev must be an 8-byte aligned device pointer");
    if (blocks == 0 || pairs_per_thread == 0) return fail(LQ_EINVAL, "lq_selftest_uniform_division: empty test");
    hipLaunchKernelGGL(k_selftest_uniform_div, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, seed, pairs_per_thread,
                       reinterpret_cast<unsigned long long*>(mismatches_dev));
    return check_hip("selftest launch");
}

}  // extern "C" (reopened below)

struct lq_adam_set {
    std::vector<lq::VecTask> h;
    lq::VecTask* d = nullptr;
    uint32_t blocks = 0;
};

extern "C" {

int lq_adam_set_create(float* const* w, float* const* m, float* const* v, const int64_t* n, const float* min_value, int count,
                       lq_adam_set** out) {
    if (!w || !m || !v || !n || !out) return fail(LQ_EINVAL, "lq_adam_set_create: NULL argument");
    if (count <= 0 || count > kBatchMax) return fail(LQ_EINVAL, "lq_adam_set_create: count must be in 1..%d", kBatchMax);
    lq_adam_set* a = new (std::nothrow) lq_adam_set();
    if (!a) return fail(LQ_EHIP, "lq_adam_set_create: out of host memory");
    for (int i = 0; i < count; ++i) {
        if (!w[i] || !m[i] || !v[i] || n[i] <= 0 || !aligned(w[i], 4) || !aligned(m[i], 4) || !aligned(v[i], 4)) {
            delete a;
            return fail(LQ_EINVAL, "lq_adam_set_create: tensor %d has a NULL/misaligned pointer or a non-positive size", i);
        }
        VecTask t;
        t.w = w[i];
        t.m = m[i];
        t.v = v[i];
        t.n = n[i];
        t.min_value = min_value ? min_value[i] : -INFINITY;
        t.first_block = a->blocks;
        const int64_t nb = ceil_div(n[i], (int64_t)kBlock * 4);
        if ((uint64_t)a->blocks + (uint64_t)nb > 0x7fffffffull) {
            delete a;
            return fail(LQ_EINVAL, "lq_adam_set_create: too many blocks");
        }
        a->blocks += (uint32_t)nb;
        a->h.push_back(t);
    }
    hipError_t e = hipMalloc(&a->d, a->h.size() * sizeof(VecTask));
    if (e == hipSuccess) e = hipMemcpy(a->d, a->h.data(), a->h.size() * sizeof(VecTask), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const int rc = fail(LQ_EHIP, "lq_adam_set_create: %s", hipGetErrorString(e));
        if (a->d) (void)hipFree(a->d);
        delete a;
        return rc;
    }
    *out = a;
    return LQ_OK;
}

int lq_adam_set_destroy(lq_adam_set* a) {
    if (!a) return LQ_OK;
    if (a->d) (void)hipFree(a->d);
    delete a;
    return LQ_OK;
}

int lq_adam_set_step(const lq_adam_set* a, const float* const* grads, double lr, double beta1, double beta2, double eps, int64_t step,
                     const int64_t* step_dev, int mode, void* stream) {
    if (!a || !grads) return fail(LQ_EINVAL, "lq_adam_set_step: NULL argument");
    if (!step_dev && step < 1) return fail(LQ_EINVAL, "lq_adam_set_step: step is 1-based");
    if (mode != LQ_ADAM_KERAS && mode != LQ_ADAM_TORCH) return fail(LQ_EINVAL, "lq_adam_set_step: bad mode %d", mode);
    PtrPack pk;
    memset(&pk, 0, sizeof(pk));
    for (size_t i = 0; i < a->h.size(); ++i) {
        if (grads[i] && !aligned(grads[i], 4)) return fail(LQ_EINVAL, "lq_adam_set_step: gradient %zu is misaligned", i);
        pk.dy[i] = grads[i];     // NULL = no gradient this step: that tensor is skipped
    }
    hipLaunchKernelGGL(k_multi_adam, dim3(a->blocks), dim3(kBlock), 0, (hipStream_t)stream, a->d, (int)a->h.size(), pk, (float)lr,
                       (float)beta1, (float)beta2, lr, beta1, beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, step_dev, step,
                       mode);
    return check_hip("multi adam launch");
}

}  // extern "C"
