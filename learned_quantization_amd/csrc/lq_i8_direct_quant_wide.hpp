// lq_i8_direct_quant_wide.hpp -- the pixel-operand epilogue of the direct int8 convolution for rows wider than the register file
// (lq_hip.h: lq_i8_conv2d_quantize_wide)
//
// k_i8_conv2d_quantize (lq_i8_direct_quant.hpp) keeps a whole output row in registers, 32 column tiles (co <= 512) at the most.
// Here the row is parked in LDS as fp32, so a block of four waves owns 16 lines by up to 128 column tiles (co <= 2048):
//
//   sweep 1  the padded row's OT = CPo / 16 column tiles are walked in CHUNKS of 32; wave w takes the 8 tiles [32 c + 8 w, + 8) of
//            chunk c.  Per chunk the wave runs the full tap walk of k_i8_conv2d_quantize<STEP, 8, true, RES> -- the next step's
//            fragments requested before this step's instructions, the row's pixel scale across by shuffle, a tap's exact int32 sum
//            flushed at its end -- then the filter's scale, the bias, affine / residual / activation in the one-wide fp32 forms, and
//            +0 for what lies past M or co.  Every lane then stores its 8 x 4 values v to the parking area and folds them into its
//            running absmax partial.  A wave whose tiles of a chunk all lie past OT skips the chunk (wave-uniform; the loop holds
//            no barrier).
//   merge    the partials over a row's 16 lanes (i8_row_absmax), then over the four waves through 768 bytes of static LDS with ONE
//            barrier; every wave derives the same row scale (i8_row_scale: k_i8_pixels' rule).
//   sweep 2  every lane reads its own v back, makes the codes (GroupStep's element step), transposes each quad (mx_quad_gather) and
//            stores one dword per tile; one lane per row of wave 0 stores the scale.
//
// The parking area is laid out by thread, float park[chunk][tile 0..7][row 0..3][thread 0..255]: a lane reads back only what it
// wrote, so the area itself needs no barrier, and a wave's 64 stores (loads) of one (tile, row) are 64 consecutive dwords -- no
// bank conflict.  It takes 32 KB per chunk, kI8WideChunkBytes * ceil(OT / 32) bytes of DYNAMIC LDS (16 CPo 4 bytes when CPo is a
// multiple of 512; 128 KB at co = 2048), above the 64 KB a kernel gets unasked: the host raises the kernel's limit once per
// instantiation (i8_conv_wide_lds_limit below), not in the launch path.
//
// Y is lq_i8_conv2d's bit for bit and the epilogue's order is k_i8_conv2d_quantize's, so for a co both accept the bytes are those
// of lq_i8_conv2d_quantize[_residual].  The tap walk is restated here rather than shared: the shipped kernels keep their
// instruction streams (profiles/i8_conv_wide/asm_compare.txt).  The four waves of a block ask for the same A fragments once per
// chunk; the cache serves them (profiles/i8_conv_wide/bench.jsonl).
#ifndef LQ_I8_DIRECT_QUANT_WIDE_HPP_
#define LQ_I8_DIRECT_QUANT_WIDE_HPP_
#include "lq_i8_direct_quant.hpp"

namespace lq {

constexpr int kI8WideNTT = 8;                                        // column tiles of a wave per chunk
constexpr int kI8WideChunk = 4 * kI8WideNTT;                         // column tiles of a chunk: four waves
constexpr int kI8WideChunkBytes = kI8WideNTT * 4 * kBlock * 4;       // parked fp32 of a chunk: 32 KB
constexpr int kI8WideMaxTiles = 4 * kI8WideChunk;                    // four chunks, 128 KB: co <= 2048

// dynamic LDS of a launch whose padded row holds OT column tiles
inline size_t i8_conv_wide_lds(int32_t OT) { return (size_t)((OT + kI8WideChunk - 1) / kI8WideChunk) * kI8WideChunkBytes; }

template <int STEP, bool RES>
__global__ __launch_bounds__(kBlock) void k_i8_conv2d_quantize_wide(const I8ConvQuantArgs<RES> q) {
    using Fr = I8Frag<STEP>;
    using FT = typename Fr::T;
    using Step = GroupStep<true, GroupParams>;
    constexpr int FB = STEP / 4, NTT = kI8WideNTT;
    extern __shared__ float i8_wide_park[];            // [chunk][NTT][4][kBlock]
    __shared__ float sh_f[2][4][kI8TileLines];
    __shared__ uint32_t sh_u[4][kI8TileLines];
    const I8Conv2dParams& p = q.c;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int32_t mt = (int32_t)blockIdx.x;
    const int32_t chunks = (q.OT + kI8WideChunk - 1) / kI8WideChunk;
    float* const park = i8_wide_park + threadIdx.x;

    // the window of the lane's A line: the corner, and the first pixel of its image.  A line past M gets a corner no tap brings inside
    const int32_t ml = mt * kI8TileLines + (lane & 15);
    const uint32_t lb = fd_div(p.ohow, (uint32_t)ml), lr = (uint32_t)ml - lb * p.ohow.d;
    const uint32_t loh = fd_div(p.ow, lr), low = lr - loh * p.ow.d;
    const int32_t ih0 = ml < p.M ? (int32_t)loh * p.stride_h - p.pad_top : -p.KH;
    const int32_t iw0 = (int32_t)low * p.stride_w - p.pad_left;
    const int32_t pb = (int32_t)lb * p.H * p.W;
    const int32_t coff = FB * (lane >> 4);                      // the lane's channels inside a step
    const int32_t khkw = p.KH * p.KW, steps = khkw * p.CS;
    const int col = lane & 15, g4 = (lane >> 4) * 4, qd = lane & 3;
    const int32_t ms = mt * kI8TileLines + g4 + qd;             // the row whose dwords the lane loads (RES) and stores

    // RES: the four row scales of the residual, once for all chunks: lane l < 16 of each sixteen reads row l's; row g4 + r's comes
    // across by the shuffle that brings the pixel scales in the tap loop
    float rsc[4];
    if constexpr (RES) {
        const int32_t mr = mt * kI8TileLines + col;
        float rs = 0.f;
        if (mr < p.M) rs = q.res_scales[mr];
#pragma unroll
        for (int r = 0; r < 4; ++r) rsc[r] = __shfl(rs, g4 + r);
    }

    InitAcc ar[4];                                              // the lane's absmax partial of row g4 + r, over all chunks
#pragma unroll
    for (int r = 0; r < 4; ++r) ar[r] = InitAcc{0.f, 0.f, 0.0, 0u};

    // ---- sweep 1: per chunk the tap walk and the epilogue; v to the parking area
    for (int32_t c = 0; c < chunks; ++c) {
        const int32_t t0 = c * kI8WideChunk + wave * NTT;       // the wave's column tiles [t0, t0 + own) of this chunk
        const int32_t own = min(q.OT - t0, NTT);                // wave-uniform
        if (own <= 0) continue;                                 // an idle wave of a ragged last chunk: the loop holds no barrier
        int32_t nt[NTT];                                        // a tile past the kernel's last one re-reads the last one
        const uint8_t* bsrc[NTT];
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            nt[j] = min(t0 + j, p.NT - 1);
            bsrc[j] = p.k_codes + ((int64_t)nt[j] * khkw * p.CS * 64 + lane) * FB;
        }
        i8_v4i acc[NTT];
        float y[NTT][4];
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            acc[j] = i8_v4i{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) y[j][r] = 0.f;
        }

        // the tap being requested: (ti, tj) and its channel step tcs are wave-uniform; `in` and `pix` are the lane's
        int32_t ti = 0, tj = 0, tcs = 0;
        bool in = false;
        int64_t pix = 0;
        float san = 0.f, sa = 0.f;
        auto enter_tap = [&]() {      // the lane's pixel under tap (ti, tj), and its scale: +0 where the tap is skipped
            const int32_t ih = ih0 + ti, iw = iw0 + tj;
            in = (uint32_t)ih < (uint32_t)p.H && (uint32_t)iw < (uint32_t)p.W;
            pix = in ? (int64_t)(pb + ih * p.W + iw) : 0;
            san = 0.f;
            if (in) san = p.pix_scales[pix];
        };
        FT a, an, b[NTT], bn[NTT];
        auto request = [&]() {        // the fragments of step (ti, tj, tcs)
            const int64_t boff = ((int64_t)(ti * p.KW + tj) * p.CS + tcs) * (64 * FB);
            an = Fr::zero();
            if (in) an = Fr::load(p.pix_codes + pix * p.CP + (STEP * tcs + coff));
#pragma unroll
            for (int j = 0; j < NTT; ++j) bn[j] = Fr::load(bsrc[j] + boff);
        };
        enter_tap();
        request();
        for (int32_t t = 0; t < steps; ++t) {
            // take the fragments requested a step ago, request the next step's, multiply
            const bool first = tcs == 0, last = tcs == p.CS - 1;      // of the tap taken now: wave-uniform
            a = an;
#pragma unroll
            for (int j = 0; j < NTT; ++j) b[j] = bn[j];
            if (first) sa = san;
            if (t + 1 < steps) {
                if (++tcs == p.CS) {
                    tcs = 0;
                    if (++tj == p.KW) { tj = 0; ++ti; }
                    enter_tap();
                }
                request();
            }
#pragma unroll
            for (int j = 0; j < NTT; ++j) acc[j] = Fr::mfma(a, b[j], acc[j]);
            if (last) {               // the tap ends: its exact sums under the pixel scales of the result rows
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sr = __shfl(sa, g4 + r);
#pragma unroll
                    for (int j = 0; j < NTT; ++j) y[j][r] = i8_scalar(__fadd_rn(y[j][r], i8_scalar(__fmul_rn((float)acc[j][r], sr))));
                }
#pragma unroll
                for (int j = 0; j < NTT; ++j) acc[j] = i8_v4i{0, 0, 0, 0};
            }
        }

        // RES: the residual's dwords, requested only now, at the address the lane later stores to (row g4 + qd, the quad's four
        // columns); the quad transpose, its own inverse, brings byte r = row g4 + r of column `col`
        uint32_t rw[RES ? NTT : 1];
        if constexpr (RES) {
            const uint8_t* src = q.res_codes + (int64_t)ms * q.CPo + (col & ~3);
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                rw[j] = 0u;
                if (j < own && ms < p.M) rw[j] = *reinterpret_cast<const uint32_t*>(src + (t0 + j) * kI8TileLines);
            }
        }
        // the filter's scale, the bias, the epilogue, and +0 for what lies past M, past co or in a tile the wave does not own
        float* const pc = park + (int64_t)c * (kI8WideChunkBytes / 4);
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            const int32_t n = (t0 + j) * kI8TileLines + col;
            const bool live_n = j < own && n < p.N;
            const float sk = p.k_scales[nt[j] * kI8TileLines + col];
            const float bv = (p.bias && live_n) ? p.bias[n] : 0.f;
            const float ps = (q.post_scale && live_n) ? q.post_scale[n] : 0.f;
            const float ph = (q.post_scale && live_n) ? q.post_shift[n] : 0.f;
            uint32_t rt = 0u;                              // RES: the residual codes of column `col`, row g4 + r in byte r
            if constexpr (RES) rt = mx_quad_gather(rw[j], qd);        // every lane takes part in the transpose
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int32_t m = mt * kI8TileLines + g4 + r;
                float v = i8_scalar(__fmul_rn(y[j][r], sk));
                if (p.bias) v = i8_scalar(__fadd_rn(v, bv));
                if (q.post_scale && q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
                if constexpr (RES) {                       // directly before the activation; the product and the sum round separately
                    const float rr = i8_scalar(__fmul_rn((float)(int8_t)(rt >> (8 * r)), rsc[r]));
                    v = i8_scalar(__fadd_rn(v, rr));
                }
                if (q.act == LQ_ACT_RELU) v = i8_relu(v);
                if (q.post_scale && !q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
                v = (live_n && m < p.M) ? v : 0.f;
                init_take<LQ_INIT_ABSMAX>(v, ar[r]);       // a masked +0 changes neither maximum
                if (j < own) pc[(j * 4 + r) * kBlock] = v;
            }
        }
    }

    // ---- a row's absmax: its 16 lanes, then the four waves through LDS; one barrier, which every wave reaches
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        i8_row_absmax(ar[r]);
        if (col == r) {
            sh_f[0][wave][g4 + r] = ar[r].f0;
            sh_f[1][wave][g4 + r] = ar[r].f1;
            sh_u[wave][g4 + r] = ar[r].bad;
        }
    }
    __syncthreads();
    Ctx cx[4];
    bool live_m[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ar[r] = InitAcc{0.f, 0.f, 0.0, 0u};
#pragma unroll
        for (int w = 0; w < 4; ++w) init_merge<LQ_INIT_ABSMAX>(ar[r], sh_f[0][w][g4 + r], sh_f[1][w][g4 + r], 0.0, sh_u[w][g4 + r]);
        const int32_t m = mt * kI8TileLines + g4 + r;
        live_m[r] = m < p.M;
        const float s = i8_row_scale(q.ip, ar[r], p.N, live_m[r]);
        cx[r] = Step::ctx(q.gp, s);
        if (col == r && live_m[r] && wave == 0) q.scales[m] = s;      // one lane per row
    }

    // ---- sweep 2: the lane's own v back, the codes, one dword per tile.  Lane qd of a quad stores row g4 + qd: the quad's four
    // columns of it, four consecutive bytes of the NHWC row
    uint8_t* const dst = q.codes + (int64_t)ms * q.CPo + (col & ~3);
    for (int32_t c = 0; c < chunks; ++c) {
        const int32_t t0 = c * kI8WideChunk + wave * NTT;
        const int32_t own = min(q.OT - t0, NTT);
        if (own <= 0) continue;
        const float* const pc = park + (int64_t)c * (kI8WideChunkBytes / 4);
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            if (j < own) {                                 // wave-uniform: every lane takes part in the transpose
                const bool live_n = (t0 + j) * kI8TileLines + col < p.N;
                uint32_t wd = 0u;                          // the lane's codes of tile j, row r in byte r
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float qv = Step::quant(q.gp, cx[r], div_by_uniform(pc[(j * 4 + r) * kBlock], cx[r]));
                    const uint32_t code = (live_n && live_m[r]) ? i8_view_byte(Step::view(q.gp, qv)) : 0u;
                    wd |= code << (8 * r);
                }
                const uint32_t word = mx_quad_gather(wd, qd);
                if (ms < p.M) *reinterpret_cast<uint32_t*>(dst + (t0 + j) * kI8TileLines) = word;
            }
        }
    }
}

// Host side.  A launch may ask for more dynamic LDS than a kernel gets unasked (64 KB): each instantiation's limit is raised ONCE,
// by the first call that reaches it (a function-local static), to the most a launch can ask for.  This is no stream operation and
// stands before the launch, not in it: a call under capture records the kernel node alone
template <int STEP, bool RES>
inline hipError_t i8_conv_wide_lds_limit() {
    static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_i8_conv2d_quantize_wide<STEP, RES>),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)i8_conv_wide_lds(kI8WideMaxTiles));
    return e;
}

// what raising the limit said; hipSuccess: the launch is enqueued (its own error is the caller's hipGetLastError)
template <int STEP, bool RES>
inline hipError_t i8_conv2d_quantize_wide_launch(const I8ConvQuantArgs<RES>& q, hipStream_t st) {
    const hipError_t e = i8_conv_wide_lds_limit<STEP, RES>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_i8_conv2d_quantize_wide<STEP, RES>), dim3((unsigned)q.c.MT), dim3(kBlock), i8_conv_wide_lds(q.OT), st, q);
    return hipSuccess;
}

}  // namespace lq

#endif
