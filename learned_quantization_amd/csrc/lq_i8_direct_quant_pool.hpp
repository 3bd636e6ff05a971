// lq_i8_direct_quant_pool.hpp -- the direct int8 convolution whose epilogue takes a non-overlapping 2 x 2 maximum and writes the
// NEXT conv's pixel operand of the POOLED image (lq_hip.h: lq_i8_conv2d_quantize_pool)
//
// conv -> relu / BatchNorm affine -> MaxPool(2) -> the next conv's pixel operand in ONE launch: no fp32 Y, no pooling pass over it,
// no second read.  The tap walk is k_i8_conv2d_quantize's (lq_i8_direct_quant.hpp), restated here so that the shipped kernels keep
// their instruction streams; what differs is the ORDER OF THE A LINES and the epilogue.
//
// Line order.  POH = OH / 2, POW = OW / 2 (floored: the conv outputs of a dropped last row or column are never computed), PM =
// B POH POW pooled lines, pooled line pm = (b POH + ph) POW + pw.  A tile mt owns the four pooled lines 4 mt + w, w = 0 .. 3, and
// its A row 4 w + e, e = 2 di + dj, is conv output pixel (b, 2 ph + di, 2 pw + dj): the four members of one pooling window lie in
// four CONSECUTIVE rows.  In the 16 x 16 result tile of the matrix instruction a lane holds column (lane & 15) and the rows
// 4 (lane >> 4) + r in its four accumulator registers -- so a lane's four registers ARE the four members of window w = lane >> 4,
// in the window's order, and the pool is a sequential maximum over the lane's own registers: no cross-lane step, no LDS, no
// second pass.  The shuffle that brings the pixel scales of the result rows in the tap loop is unchanged: lane l < 16 holds row l's.
//
// Epilogue.  Per lane and tile the four v (the filter's scale, the bias, relu / affine in either order: k_i8_conv2d_quantize's
// steps), then m = v00; for u in (v01, v10, v11): if (u > m || u != u) m = u -- torch's rule, a NaN is sticky -- then the absmax of
// ONE row per lane over its tiles and the row's 16 lanes (i8_row_absmax), in the BLOCK form over the four waves through 192 bytes
// of LDS with one barrier (4 rows per block instead of 16), then k_i8_pixels' scale rule and element step: a quarter of the rows
// of k_i8_conv2d_quantize to quantise and store.
//
// Stores.  A lane holds ONE code byte per tile.  Byte t of word jj is the code of tile 4 jj + t; after the quad transpose
// (mx_quad_gather) lane qd of a quad holds, in word jj, the quad's four columns of tile 4 jj + qd: four consecutive bytes of the
// pooled pixel's NHWC row, stored as one dword.  No byte stores; NTT = 2 keeps one word whose upper two lanes store nothing.
//
//   BLOCK = false, OT <= 8 (co <= 128): a wave owns one A tile (4 pooled lines) by all OT column tiles, a block 16 pooled lines.
//   BLOCK = true, OT <= 32 (co <= 512): a block owns one A tile, wave w the column tiles [w OT / 4, (w + 1) OT / 4).
// The parameter block is I8ConvQuantParams with c.M = PM, c.MT = ceil(PM / 4), c.ohow = POH POW and c.ow = POW: the lines the
// kernel counts are the pooled ones.  No atomics, no memset, no workspace.
#ifndef LQ_I8_DIRECT_QUANT_POOL_HPP_
#define LQ_I8_DIRECT_QUANT_POOL_HPP_
#include "lq_i8_direct_quant.hpp"

namespace lq {

constexpr int kI8PoolLines = kI8TileLines / 4;      // pooled lines of an A tile: 4 windows of 2 x 2

// the sequential maximum of torch's max_pool2d over a window in (di, dj) order: a later member wins only if greater, or a NaN
__device__ __forceinline__ float i8_pool4(const float (&v)[4]) {
    float m = v[0];
#pragma unroll
    for (int e = 1; e < 4; ++e)
        if (v[e] > m || v[e] != v[e]) m = v[e];
    return m;
}

template <int STEP, int NTT, bool BLOCK>
__global__ __launch_bounds__(kBlock) void k_i8_conv2d_quantize_pool(const I8ConvQuantParams q) {
    using Fr = I8Frag<STEP>;
    using FT = typename Fr::T;
    using Step = GroupStep<true, GroupParams>;
    constexpr int FB = STEP / 4;
    constexpr int NW = (NTT + 3) / 4;                 // code words of a lane: byte t of word jj is tile 4 jj + t
    const I8Conv2dParams& p = q.c;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int32_t mt, t0, t1;       // the wave's A tile and its column tiles [t0, t1), at most NTT
    if constexpr (BLOCK) {
        mt = (int32_t)blockIdx.x;
        t0 = wave * q.OT / 4;
        t1 = (wave + 1) * q.OT / 4;
    } else {
        mt = (int32_t)blockIdx.x * 4 + wave;
        t0 = 0;
        t1 = q.OT;
        if (mt >= p.MT) return;       // wave-uniform; this form has no barrier
    }
    const int32_t own = t1 - t0;      // wave-uniform

    // the lane's A line: member e = 2 di + dj of the window of pooled line 4 mt + w.  Its conv output pixel, the window's corner
    // in the input, and the first pixel of its image.  The row of a pooled line past PM gets a corner no tap brings inside
    const int arow = lane & 15;
    const int32_t pl = mt * kI8PoolLines + (arow >> 2);
    const uint32_t lb = fd_div(p.ohow, (uint32_t)pl), lr = (uint32_t)pl - lb * p.ohow.d;
    const uint32_t lph = fd_div(p.ow, lr), lpw = lr - lph * p.ow.d;
    const int32_t loh = 2 * (int32_t)lph + ((arow >> 1) & 1), low = 2 * (int32_t)lpw + (arow & 1);
    const int32_t ih0 = pl < p.M ? loh * p.stride_h - p.pad_top : -p.KH;
    const int32_t iw0 = low * p.stride_w - p.pad_left;
    const int32_t pb = (int32_t)lb * p.H * p.W;
    const int32_t coff = FB * (lane >> 4);                      // the lane's channels inside a step
    const int32_t khkw = p.KH * p.KW;
    int32_t nt[NTT];                                            // a tile past the kernel's last one re-reads the last one
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
    const int32_t steps = khkw * p.CS;
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
                const float sr = __shfl(sa, (lane >> 4) * 4 + r);
#pragma unroll
                for (int j = 0; j < NTT; ++j) y[j][r] = i8_scalar(__fadd_rn(y[j][r], i8_scalar(__fmul_rn((float)acc[j][r], sr))));
            }
#pragma unroll
            for (int j = 0; j < NTT; ++j) acc[j] = i8_v4i{0, 0, 0, 0};
        }
    }

    // result tile: column (lane & 15) on the lane, and in its four registers the four members of window lane >> 4.  The filter's
    // scale, the bias and the epilogue per member, then the window's maximum; +0 for what lies past PM, past co or in a tile the
    // wave does not own (a clamped tile holds a copy of the last one)
    const int col = lane & 15, w = lane >> 4, qd = lane & 3;
    const int32_t pm = mt * kI8PoolLines + w;         // the lane's pooled line
    const bool live_m = pm < p.M;
    float pv[NTT];
    bool live_n[NTT];
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        const int32_t n = (t0 + j) * kI8TileLines + col;
        live_n[j] = j < own && n < p.N;
        const float sk = p.k_scales[nt[j] * kI8TileLines + col];
        const float bv = (p.bias && live_n[j]) ? p.bias[n] : 0.f;
        const float ps = (q.post_scale && live_n[j]) ? q.post_scale[n] : 0.f;
        const float ph = (q.post_scale && live_n[j]) ? q.post_shift[n] : 0.f;
        float vv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = i8_scalar(__fmul_rn(y[j][r], sk));
            if (p.bias) v = i8_scalar(__fadd_rn(v, bv));
            if (q.post_scale && q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
            if (q.act == LQ_ACT_RELU) v = i8_relu(v);
            if (q.post_scale && !q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
            vv[r] = v;
        }
        pv[j] = (live_n[j] && live_m) ? i8_pool4(vv) : 0.f;
    }

    // the pooled row's absmax: the lane's tiles, then the row's 16 lanes; BLOCK: then the four waves, through LDS
    InitAcc ar{0.f, 0.f, 0.0, 0u};
#pragma unroll
    for (int j = 0; j < NTT; ++j) init_take<LQ_INIT_ABSMAX>(pv[j], ar);      // a masked +0 changes neither maximum
    i8_row_absmax(ar);
    if constexpr (BLOCK) {
        __shared__ float sh_f[2][4][kI8PoolLines];
        __shared__ uint32_t sh_u[4][kI8PoolLines];
        if (col == 0) {
            sh_f[0][wave][w] = ar.f0;
            sh_f[1][wave][w] = ar.f1;
            sh_u[wave][w] = ar.bad;
        }
        __syncthreads();
        ar = InitAcc{0.f, 0.f, 0.0, 0u};
#pragma unroll
        for (int u = 0; u < 4; ++u) init_merge<LQ_INIT_ABSMAX>(ar, sh_f[0][u][w], sh_f[1][u][w], 0.0, sh_u[u][w]);
    }

    const float s = i8_row_scale(q.ip, ar, p.N, live_m);
    const Ctx c = Step::ctx(q.gp, s);
    uint32_t wd[NW];                                   // the lane's codes: tile 4 jj + t in byte t of word jj
#pragma unroll
    for (int jj = 0; jj < NW; ++jj) wd[jj] = 0u;
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        const float qv = Step::quant(q.gp, c, div_by_uniform(pv[j], c));
        const uint32_t code = (live_n[j] && live_m) ? i8_view_byte(Step::view(q.gp, qv)) : 0u;
        wd[j >> 2] |= code << (8 * (j & 3));
    }
    if (col == 0 && live_m && (!BLOCK || wave == 0)) q.scales[pm] = s;      // one lane per pooled row
    // lane qd of a quad stores tile 4 jj + qd: the quad's four columns of it, four consecutive bytes of the pooled NHWC row
    uint8_t* dst = q.codes + (int64_t)pm * q.CPo + (col & ~3);
#pragma unroll
    for (int jj = 0; jj < NW; ++jj) {
        const uint32_t word = mx_quad_gather(wd[jj], qd);     // every lane takes part in the transpose
        const int32_t j = 4 * jj + qd;
        if (j < own && live_m) *reinterpret_cast<uint32_t*>(dst + (t0 + j) * kI8TileLines) = word;
    }
}

// the instantiation by the padded row's tiles, beside i8_conv2d_quantize_launch: host side, called from lq_i8_conv2d_quantize_pool
template <int STEP>
inline void i8_conv2d_quantize_pool_launch(const I8ConvQuantParams& q, hipStream_t st) {
    const dim3 blk(kBlock);
    if (q.OT <= 8) {              // a row per wave, four A tiles (16 pooled lines) per block
        const dim3 grid((unsigned)((q.c.MT + 3) / 4));
        if (q.OT <= 2) hipLaunchKernelGGL((k_i8_conv2d_quantize_pool<STEP, 2, false>), grid, blk, 0, st, q);
        else if (q.OT <= 4) hipLaunchKernelGGL((k_i8_conv2d_quantize_pool<STEP, 4, false>), grid, blk, 0, st, q);
        else hipLaunchKernelGGL((k_i8_conv2d_quantize_pool<STEP, 8, false>), grid, blk, 0, st, q);
    } else {                      // a row per block: ceil(OT / 4) tiles on the widest wave
        const dim3 grid((unsigned)q.c.MT);
        if (q.OT <= 16) hipLaunchKernelGGL((k_i8_conv2d_quantize_pool<STEP, 4, true>), grid, blk, 0, st, q);
        else hipLaunchKernelGGL((k_i8_conv2d_quantize_pool<STEP, 8, true>), grid, blk, 0, st, q);
    }
}

}  // namespace lq

#endif
