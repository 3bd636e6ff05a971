// lq_i8_stem.hpp -- the direct int8 convolution of a FIRST layer: an input of at most 4 channels under one scale per image ROW
// (lq_hip.h: lq_i8_rows_quantize / lq_i8_stem_kernel_pack / lq_i8_stem_conv2d / lq_i8_stem_conv2d_quantize)
//
// lq_i8_direct.hpp sums a tap exactly under one pixel scale, which leaves v_mfma_i32_16x16x32_i8 with C of its 32 reduction slots:
// at C = 3 a 7 x 7 stem is 49 instructions per tile of 29 padded zeros each.  Here the scale belongs to an image row, so a whole
// KERNEL ROW -- KW taps x 4 channel bytes <= 32 -- is one exact int32 reduction step: 7 instructions per tile for that stem.
//
//   rows    codes [B][H][W][4] int8 (NHWC4: channel c in byte c, bytes C .. 3 code 0); scales [B][H] fp32: the absmax scale of the
//           row's W C elements and the nearest-even codes under it -- k_i8_quantize's scale rule and element step (init_take /
//           init_merge / init_raw / init_final, GroupStep<true, GroupParams>, div_by_uniform, i8_view_byte), called, not restated.
//   kernel  codes [NT][KH][64 lanes][8], NT = ceil(co / 16): lane l, byte jj holds filter 16 nt + (l & 15), tap column
//           j = 2 (l >> 4) + (jj >> 2), channel jj & 3; code 0 for j >= KW, c >= ci and filters past co.  scales [16 NT], 1.0f past co.
//
// k_i8_rows: a wave per image row, four rows to a block, the lanes striding over the pixels so that a wave's load of one channel of
// an NCHW row is one contiguous run.  A lane keeps its first kI8RowCache pixels (4 channels each) in registers between the maximum
// and the codes: a row of W <= 64 kI8RowCache = 256 pixels is read once, what lies beyond a second time.  The 64 partial maxima
// merge by k_i8_quantize's xor butterfly of init_merge; every lane then stores one dword per pixel.
//
// k_i8_stem_conv2d<NTT, OUT>: the K loop is KH steps, N is at most 8 column tiles and M is enormous, so the kernel is bound by its
// A gather and its store, not by the matrix unit, and is shaped for that:
//   * a block stages its column tiles of the kernel operand -- NTT KH 512 bytes, 14 KB for 7 x 7 x 64 -- in LDS once, and every
//     row's B fragments come back as 8-byte reads at consecutive lanes (conflict free);
//   * a wave owns one line tile (16 output pixels) by ALL NTT column tiles: A is gathered once per line and, with OUT, the whole
//     output row is in registers for the pixel-operand epilogue;
//   * a wave walks kI8StemWalk = 4 line tiles (a block 16 tiles, 256 lines), so the staging is paid once per 256 lines: 14 KB
//     from the cache against 64 KB of fp32 result at 64 filters;
//   * per kernel row a lane loads its 8 bytes of the A fragment as two predicated dwords, pixels iw0 + 2 (l >> 4) and + 1 of row
//     ih0 + i (the window corner comes from FastDiv once per tile); a pixel outside [0, W) or a row outside [0, H) is zero and
//     forms no address.  A pixel past the window's last column but inside the image is read: the kernel's code there is 0;
//   * the row scale of the lane's line is loaded with the fragment and reaches the result rows by the four shuffles of
//     k_i8_conv2d; the next row's fragment and scale are requested before this row's instructions;
//   * OUT = false writes fp32 Y (a grid.y block per NTT column tiles, so any co); OUT = true (co <= 128) is the epilogue of
//     lq_i8_direct_quant.hpp's wave form: i8_row_absmax, i8_row_scale, i8_relu, mx_quad_gather and the quantizer's element step.
// A row outside the image adds RN(0 * 0) = +0 to a y that is never -0: the bits of skipping it.  No scratch, no atomics; the one
// barrier follows the staging, so no wave returns before it (profiles/i8_stem/kernel_resources.txt).
#ifndef LQ_I8_STEM_HPP_
#define LQ_I8_STEM_HPP_
#include "lq_i8_direct_quant.hpp"

namespace lq {

constexpr int kI8StemChannels = 4;    // channel bytes of a pixel: one dword
constexpr int kI8StemMaxKW = 8;       // taps of a kernel row: 8 x 4 bytes fill one step of v_mfma_i32_16x16x32_i8
constexpr int kI8StemMaxKH = 16;      // 8 column tiles x 16 kernel rows x 512 bytes are the 64 KB of LDS a block may hold
constexpr int kI8StemMaxTiles = 8;    // column tiles a wave holds: the pixel-operand form takes co <= 128
constexpr int kI8StemWalk = 4;        // line tiles a wave walks behind one staging
constexpr int kI8RowCache = 4;        // pixels per lane held in registers between the scale and the codes: W <= 256 is read once

struct I8RowsParams {
    GroupParams g;            // P = X, lo = -127, hi = 127; nothing else is read
    InitParams ip;            // lo, hi, min_value
    uint32_t* codes;          // [B H][W] dwords
    float* scales;            // [B H]
    int64_t xs_b, xs_c, xs_h, xs_w;       // of X, in elements
    FastDiv h;                // row -> (b, h)
    int32_t NR, C, W;         // rows B H; channels read; pixels of a row
};

__global__ __launch_bounds__(kBlock) void k_i8_rows(const I8RowsParams op) {
    using Step = GroupStep<true, GroupParams>;
    const int lane = (int)threadIdx.x & 63;
    const int32_t row = (int32_t)blockIdx.x * (kBlock / 64) + ((int)threadIdx.x >> 6);
    if (row >= op.NR) return;                 // wave-uniform; the kernel has no barrier
    const uint32_t b = fd_div(op.h, (uint32_t)row), h = (uint32_t)row - b * op.h.d;
    const float* src = op.g.P + ((int64_t)b * op.xs_b + (int64_t)h * op.xs_h);

    auto load_px = [&](int32_t w, float (&xv)[kI8StemChannels]) {      // w < W; a channel at or past C is +0 and forms no address
#pragma unroll
        for (int e = 0; e < kI8StemChannels; ++e) {
            xv[e] = 0.f;
            if (e < op.C) xv[e] = src[(int64_t)w * op.xs_w + (int64_t)e * op.xs_c];      // kernel-uniform
        }
    };
    float x[kI8RowCache][kI8StemChannels];
    InitAcc a{0.f, 0.f, 0.0, 0u};
#pragma unroll
    for (int it = 0; it < kI8RowCache; ++it) {
        const int32_t w = it * 64 + lane;
#pragma unroll
        for (int e = 0; e < kI8StemChannels; ++e) x[it][e] = 0.f;
        if (w < op.W) {
            load_px(w, x[it]);
#pragma unroll
            for (int e = 0; e < kI8StemChannels; ++e) init_take<LQ_INIT_ABSMAX>(x[it][e], a);      // a padded +0 changes no maximum
        }
    }
    for (int32_t w = kI8RowCache * 64 + lane; w < op.W; w += 64) {      // what the registers do not hold
        float t[kI8StemChannels];
        load_px(w, t);
#pragma unroll
        for (int e = 0; e < kI8StemChannels; ++e) init_take<LQ_INIT_ABSMAX>(t[e], a);
    }
    for (int off = 32; off > 0; off >>= 1)        // the fixed butterfly of k_i8_quantize over the whole wave: every lane ends with the total
        init_merge<LQ_INIT_ABSMAX>(a, __shfl_xor(a.f0, off), __shfl_xor(a.f1, off), 0.0, __shfl_xor(a.bad, off));
    const float s = init_final(op.ip, init_raw<LQ_INIT_ABSMAX>(op.ip, a, (int64_t)op.W * op.C), a.bad);
    if (lane == 0) op.scales[row] = s;
    const Ctx cx = Step::ctx(op.g, s);
    uint32_t* dst = op.codes + (int64_t)row * op.W;

    auto emit = [&](int32_t w, const float (&xv)[kI8StemChannels]) {
        uint32_t wd = 0u;
#pragma unroll
        for (int e = 0; e < kI8StemChannels; ++e) {
            const float q = Step::quant(op.g, cx, div_by_uniform(xv[e], cx));
            wd |= (e < op.C ? i8_view_byte(Step::view(op.g, q)) : 0u) << (8 * e);
        }
        dst[w] = wd;
    };
#pragma unroll
    for (int it = 0; it < kI8RowCache; ++it) {
        const int32_t w = it * 64 + lane;
        if (w < op.W) emit(w, x[it]);
    }
    for (int32_t w = kI8RowCache * 64 + lane; w < op.W; w += 64) {
        float t[kI8StemChannels];
        load_px(w, t);
        emit(w, t);
    }
}

struct I8StemPackParams {
    GroupParams g;            // P, s, lo, hi; the geometry fields are not read
    uint8_t* codes;
    float* scales;
    int32_t co, ci, KH, KW, NT;
};

// one thread per fragment: (nt, i, lane), lanes fastest -- the 8-byte stores of a wave are contiguous
template <bool RNE>
__global__ __launch_bounds__(kBlock) void k_i8_stem_pack(const I8StemPackParams op) {
    using Step = GroupStep<RNE, GroupParams>;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tid >= (int64_t)op.NT * op.KH * 64) return;
    const int lane = (int)(tid & 63);
    const int32_t rest = (int32_t)(tid >> 6), i = rest % op.KH, nt = rest / op.KH;
    const int32_t n = nt * kI8TileLines + (lane & 15), j0 = 2 * (lane >> 4);
    const bool live = n < op.co;
    const float s = live ? op.g.s[n] : 1.0f;
    uint32_t w[2] = {0u, 0u};
    if (live) {
        const Ctx c = Step::ctx(op.g, s);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int32_t j = j0 + (jj >> 2), ch = jj & 3;
            if (j < op.KW && ch < op.ci) {
                const float v = op.g.P[(((int64_t)n * op.ci + ch) * op.KH + i) * op.KW + j];      // P[n][c][i][j]
                const float q = Step::quant(op.g, c, div_by_uniform(v, c));
                w[jj >> 2] |= i8_view_byte(Step::view(op.g, q)) << (8 * (jj & 3));
            }
        }
    }
    *reinterpret_cast<uint2*>(op.codes + tid * 8) = make_uint2(w[0], w[1]);
    if (i == 0 && lane < kI8TileLines) op.scales[n] = s;      // the filter's scale, bit for bit; 1.0f past co
}

// The parameters are the twin's: I8Conv2dParams (pix_codes / pix_scales hold the row operand; CS and CP are not read) and, with
// OUT, I8ConvQuantParams around it
template <bool OUT>
using I8StemArgs = std::conditional_t<OUT, I8ConvQuantParams, I8Conv2dParams>;

template <int NTT, bool OUT>
__global__ __launch_bounds__(kBlock) void k_i8_stem_conv2d(const I8StemArgs<OUT> q) {
    const I8Conv2dParams& p = [&]() -> const I8Conv2dParams& {
        if constexpr (OUT) return q.c;
        else return q;
    }();
    // The staging, the gather (`request`) and the epilogue value below are stated a second time in lq_i8_stem_pool.hpp (i8_stem_stage,
    // i8_stem_gather, i8_stem_value): an edit to one is an edit to both
    extern __shared__ uint4 stem_lds[];               // [NTT][KH][64 lanes] fragments of 8 bytes
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int32_t nt0 = (int32_t)blockIdx.y * NTT;    // OUT: grid.y = 1
    // the block's column tiles [nt0, nt0 + NTT) are one contiguous run of the operand; a tile past NT is zero, and masked below
    {
        const int32_t have = max(0, min(NTT, p.NT - nt0)) * p.KH * 32, all = NTT * p.KH * 32;      // in 16-byte units
        const uint4* srcv = reinterpret_cast<const uint4*>(p.k_codes + (int64_t)nt0 * p.KH * 512);
        for (int32_t u = (int32_t)threadIdx.x; u < all; u += kBlock) stem_lds[u] = u < have ? srcv[u] : make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const long* bl = reinterpret_cast<const long*>(stem_lds) + lane;
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(p.pix_codes);
    const int col = lane & 15, g4 = (lane >> 4) * 4;

    for (int32_t wk = 0; wk < kI8StemWalk; ++wk) {
        const int32_t mt = ((int32_t)blockIdx.x * kI8StemWalk + wk) * (kBlock / 64) + wave;
        if (mt >= p.MT) break;                        // wave-uniform, and behind the only barrier

        // the window of the lane's A line: its corner, the lane's two pixels of every row, the first row of its image.  A line past
        // M gets a corner that no kernel row brings inside
        const int32_t ml = mt * kI8TileLines + col;
        const uint32_t lb = fd_div(p.ohow, (uint32_t)ml), lr = (uint32_t)ml - lb * p.ohow.d;
        const uint32_t loh = fd_div(p.ow, lr), low = lr - loh * p.ow.d;
        const int32_t ih0 = ml < p.M ? (int32_t)loh * p.stride_h - p.pad_top : -p.KH;
        const int32_t px0 = (int32_t)low * p.stride_w - p.pad_left + 2 * (lane >> 4), px1 = px0 + 1;
        const bool in0 = (uint32_t)px0 < (uint32_t)p.W, in1 = (uint32_t)px1 < (uint32_t)p.W;
        const int32_t rb = (int32_t)lb * p.H;

        float y[NTT][4];
#pragma unroll
        for (int j = 0; j < NTT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[j][r] = 0.f;

        uint32_t an0 = 0u, an1 = 0u;
        float san = 0.f;
        auto request = [&](int32_t i) {               // the lane's fragment of kernel row i and its row's scale: zero where skipped
            const int32_t ih = ih0 + i;
            const bool inr = (uint32_t)ih < (uint32_t)p.H;
            const int32_t row = inr ? rb + ih : 0;
            an0 = 0u;
            an1 = 0u;
            san = 0.f;
            if (inr) san = p.pix_scales[row];
            if (inr && in0) an0 = codes[(int64_t)row * p.W + px0];
            if (inr && in1) an1 = codes[(int64_t)row * p.W + px1];
        };
        request(0);
        for (int32_t i = 0; i < p.KH; ++i) {
            // take the fragment requested a row ago, request the next row's, multiply
            const long a = (long)(((uint64_t)an1 << 32) | (uint64_t)an0);
            const float sa = san;
            if (i + 1 < p.KH) request(i + 1);
            i8_v4i acc[NTT];
#pragma unroll
            for (int j = 0; j < NTT; ++j)
                acc[j] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, bl[(j * p.KH + i) * 64], i8_v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {             // the row's exact sums under the row scales of the result rows
                const float sr = __shfl(sa, g4 + r);
#pragma unroll
                for (int j = 0; j < NTT; ++j) y[j][r] = i8_scalar(__fadd_rn(y[j][r], i8_scalar(__fmul_rn((float)acc[j][r], sr))));
            }
        }

        // result tile: column `col` on the lane, rows g4 + r in the registers
        if constexpr (!OUT) {
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                const int32_t n = (nt0 + j) * kI8TileLines + col;
                if (n >= p.N) continue;
                const float sk = p.k_scales[n];
                const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int32_t m = mt * kI8TileLines + g4 + r;
                    const float v = i8_scalar(__fmul_rn(y[j][r], sk));
                    if (m < p.M) p.Y[(int64_t)m * p.ldy + n] = p.bias ? i8_scalar(__fadd_rn(v, bv)) : v;
                }
            }
        } else {
            // the epilogue of k_i8_conv2d_quantize's wave form: the filter's scale, the bias, activation and affine, +0 for what lies
            // past M or past co; the row's absmax over its 16 lanes; the quantizer's element step; a quad's transpose for the store
            using Step = GroupStep<true, GroupParams>;
            const int qd = lane & 3;
            bool live_n[NTT];
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                const int32_t n = j * kI8TileLines + col;
                live_n[j] = j < q.OT && n < p.N;
                const float sk = live_n[j] ? p.k_scales[n] : 1.0f;
                const float bv = (p.bias && live_n[j]) ? p.bias[n] : 0.f;
                const float ps = (q.post_scale && live_n[j]) ? q.post_scale[n] : 0.f;
                const float ph = (q.post_scale && live_n[j]) ? q.post_shift[n] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int32_t m = mt * kI8TileLines + g4 + r;
                    float v = i8_scalar(__fmul_rn(y[j][r], sk));
                    if (p.bias) v = i8_scalar(__fadd_rn(v, bv));
                    if (q.post_scale && q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
                    if (q.act == LQ_ACT_RELU) v = i8_relu(v);
                    if (q.post_scale && !q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
                    y[j][r] = (live_n[j] && m < p.M) ? v : 0.f;
                }
            }
            uint32_t wd[NTT];                          // the lane's codes of tile j, row r in byte r
#pragma unroll
            for (int j = 0; j < NTT; ++j) wd[j] = 0u;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                InitAcc ar{0.f, 0.f, 0.0, 0u};
#pragma unroll
                for (int j = 0; j < NTT; ++j) init_take<LQ_INIT_ABSMAX>(y[j][r], ar);      // a masked +0 changes neither maximum
                i8_row_absmax(ar);
                const int32_t m = mt * kI8TileLines + g4 + r;
                const bool live_m = m < p.M;
                const float s = i8_row_scale(q.ip, ar, p.N, live_m);
                const Ctx c = Step::ctx(q.gp, s);
#pragma unroll
                for (int j = 0; j < NTT; ++j) {
                    const float qv = Step::quant(q.gp, c, div_by_uniform(y[j][r], c));
                    const uint32_t code = (live_n[j] && live_m) ? i8_view_byte(Step::view(q.gp, qv)) : 0u;
                    wd[j] |= code << (8 * r);
                }
                if (col == r && live_m) q.scales[m] = s;      // one lane per row
            }
            // lane qd of a quad stores row g4 + qd: the quad's four columns of it, four consecutive bytes of the NHWC row
            const int32_t ms = mt * kI8TileLines + g4 + qd;
            uint8_t* dst = q.codes + (int64_t)ms * q.CPo + (col & ~3);
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                const uint32_t word = mx_quad_gather(wd[j], qd);      // every lane takes part in the transpose
                if (j < q.OT && ms < p.M) *reinterpret_cast<uint32_t*>(dst + j * kI8TileLines) = word;
            }
        }
    }
}

// the instantiation by the column tiles a wave holds: `tiles` of them per grid.y block (OUT: the padded row's OT, grid.y = 1)
template <bool OUT>
inline void i8_stem_conv2d_launch(const I8StemArgs<OUT>& q, int32_t MT, int32_t KH, int32_t tiles, hipStream_t st) {
    const int ntt = tiles <= 2 ? 2 : tiles <= 4 ? 4 : kI8StemMaxTiles;
    const int32_t per_block = kI8StemWalk * (kBlock / 64);
    const dim3 grid((unsigned)((MT + per_block - 1) / per_block), (unsigned)((tiles + ntt - 1) / ntt)), blk(kBlock);
    const size_t lds = (size_t)ntt * KH * 512;
    if (ntt == 2) hipLaunchKernelGGL((k_i8_stem_conv2d<2, OUT>), grid, blk, lds, st, q);
    else if (ntt == 4) hipLaunchKernelGGL((k_i8_stem_conv2d<4, OUT>), grid, blk, lds, st, q);
    else hipLaunchKernelGGL((k_i8_stem_conv2d<8, OUT>), grid, blk, lds, st, q);
}

}  // namespace lq

#endif
