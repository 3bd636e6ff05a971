// lq_i8_direct_quant.hpp -- the direct int8 convolution with an epilogue that writes the NEXT conv's pixel operand
// (lq_hip.h: lq_i8_conv2d_quantize)
//
// The product of lq_i8_direct.hpp, but what leaves the kernel is lq_i8_pixels_quantize of v = epilogue(Y): int8 NHWC codes
// [M][CPo], CPo = 32 ceil(co / 32), and one fp32 scale per output pixel -- no fp32 Y, no relu / BatchNorm passes over it, no second
// read.  lq_i8_conv2d's Y is a function of the operands alone (an exact int32 sum per tap, then the stated fp32 roundings in
// ascending tap order), so this kernel is free in its tiling and still computes that Y bit for bit.
//
// A pixel's scale is the absmax over ALL co channels of its line: a complete output row must be resident before its first code.
// The padded row holds OT = CPo / 16 = 2 ceil(co / 32) column tiles, an even number; a tile past the kernel's last one (NT =
// ceil(co / 16)) re-reads the last one and is masked to +0, so a ragged co and the CPo padding are written without a memset.
//
//   BLOCK = false, OT <= 8 (co <= 128): a wave owns one A tile (16 lines) by all OT column tiles, NTT in {2, 4, 8} of them in
//       registers; a block of four waves owns 64 lines.  No LDS, no barrier: a wave past MT returns.
//   BLOCK = true, OT <= 32 (co <= 512): a block owns 16 lines, wave w the column tiles [w OT / 4, (w + 1) OT / 4) -- at most 8, and
//       at least two, so every wave holds live work -- NTT in {4, 8}.  A row's absmax partial of each wave (two maxima and the bad
//       flag: exact in any order) goes through 768 bytes of LDS with ONE barrier; every wave then derives the same scale and writes
//       its own codes.  No wave returns early.  The four waves ask for the same A fragments, which the cache serves.
//
// The tap walk is k_i8_conv2d's for one A tile: (i, j, cs) wave-uniform, each lane's pixel formed from its own line, the fragments
// of the next step requested before this step's instructions, the exact int32 sum of a tap flushed under the pixel scale of the
// result ROW, which comes across by a shuffle.  Then the filter's scale, the bias, and the epilogue in the one-wide fp32 forms
// (i8_scalar); a row's absmax partials merge over its 16 lanes by the four DPP steps of i8_row_absmax; the scale rule and the
// element step are k_i8_pixels' own device functions; a quad's 4 x 4 bytes are transposed in registers (mx_quad_gather) so that a
// lane stores one dword per tile into the NHWC row, and one lane per row stores the scale.
//
// RES = true (lq_i8_conv2d_quantize_residual): a residual pixel operand of the OUTPUT's shape is decoded, r = RN(code * scale), and
// added directly before the activation.  Its NHWC row is laid out as this kernel stores its own codes, so after the tap loop a lane
// reads one dword per owned tile at the very address it later stores to, and the same quad transpose (its own inverse) brings
// byte r = row g4 + r of the lane's column; the four row scales come by one load per lane and the shuffle of the tap loop.  In the
// BLOCK form every wave adds its own tiles' residual before its absmax partials go through LDS.  Two more VGPRs than RES = false,
// the same waves per SIMD, no scratch, no LDS of its own (profiles/i8_conv_residual/kernel_resources.txt).
#ifndef LQ_I8_DIRECT_QUANT_HPP_
#define LQ_I8_DIRECT_QUANT_HPP_
#include "lq_i8_direct.hpp"
#include "lq_i8_gemm_quant.hpp"

namespace lq {

struct I8ConvQuantParams {
    I8Conv2dParams c;         // Y and ldy are not read
    GroupParams gp;           // lo = -127, hi = 127; nothing else is read
    InitParams ip;            // lo, hi, min_value
    const float* post_scale;  // [co], or both NULL
    const float* post_shift;
    uint8_t* codes;           // [M][CPo]
    float* scales;            // [M]
    int32_t act;              // lq_mx_activation
    int32_t affine_first;     // 0: aff(act(Y)); 1: act(aff(Y))
    int32_t OT, CPo;          // column tiles of the padded row; its bytes
};
// lq_i8_conv2d_quantize_residual: the same, and a residual pixel operand of the OUTPUT's shape.  A derived struct, passed only to
// the RES = true kernels, so that the kernel without a residual keeps its argument block and with it its instruction stream
struct I8ConvQuantResParams : I8ConvQuantParams {
    const uint8_t* res_codes;     // [M][CPo]
    const float* res_scales;      // [M]
};
template <bool RES>
using I8ConvQuantArgs = std::conditional_t<RES, I8ConvQuantResParams, I8ConvQuantParams>;

template <int STEP, int NTT, bool BLOCK, bool RES>
__global__ __launch_bounds__(kBlock) void k_i8_conv2d_quantize(const I8ConvQuantArgs<RES> q) {
    using Fr = I8Frag<STEP>;
    using FT = typename Fr::T;
    using Step = GroupStep<true, GroupParams>;
    constexpr int FB = STEP / 4;
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

    // the window of the lane's A line: the corner, and the first pixel of its image.  A line past M gets a corner no tap brings inside
    const int32_t ml = mt * kI8TileLines + (lane & 15);
    const uint32_t lb = fd_div(p.ohow, (uint32_t)ml), lr = (uint32_t)ml - lb * p.ohow.d;
    const uint32_t loh = fd_div(p.ow, lr), low = lr - loh * p.ow.d;
    const int32_t ih0 = ml < p.M ? (int32_t)loh * p.stride_h - p.pad_top : -p.KH;
    const int32_t iw0 = (int32_t)low * p.stride_w - p.pad_left;
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

    // result tile: column (lane & 15) on the lane, rows 4 (lane >> 4) + r in the registers.  The filter's scale, the bias, the
    // epilogue, and +0 for what lies past M, past co or in a tile the wave does not own (a clamped tile holds a copy of the last one)
    const int col = lane & 15, g4 = (lane >> 4) * 4, qd = lane & 3;
    // RES: the residual, requested only now, after the tap loop (holding NTT dwords through it costs the widest forms registers
    // they do not have).  Lane qd of a quad reads the dword it later STORES to -- row g4 + qd, the quad's four columns -- and the
    // transpose that lays the codes out for the store is its own inverse, so it brings byte r = row g4 + r of column `col` here.
    // A lane forms no address for a row past M or a tile the wave does not own.  The row scales: lane l < 16 of each sixteen
    // reads row l's once; row g4 + r's comes across by the shuffle that brings the pixel scales in the tap loop
    uint32_t rw[RES ? NTT : 1];
    float rsc[4];
    if constexpr (RES) {
        const int32_t ms = mt * kI8TileLines + g4 + qd;
        const uint8_t* src = q.res_codes + (int64_t)ms * q.CPo + (col & ~3);
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            rw[j] = 0u;
            if (j < own && ms < p.M) rw[j] = *reinterpret_cast<const uint32_t*>(src + (t0 + j) * kI8TileLines);
        }
        const int32_t mr = mt * kI8TileLines + col;
        float rs = 0.f;
        if (mr < p.M) rs = q.res_scales[mr];
#pragma unroll
        for (int r = 0; r < 4; ++r) rsc[r] = __shfl(rs, g4 + r);
    }
    bool live_n[NTT];
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        const int32_t n = (t0 + j) * kI8TileLines + col;
        live_n[j] = j < own && n < p.N;
        const float sk = p.k_scales[nt[j] * kI8TileLines + col];
        const float bv = (p.bias && live_n[j]) ? p.bias[n] : 0.f;
        const float ps = (q.post_scale && live_n[j]) ? q.post_scale[n] : 0.f;
        const float ph = (q.post_scale && live_n[j]) ? q.post_shift[n] : 0.f;
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
            y[j][r] = (live_n[j] && m < p.M) ? v : 0.f;
        }
    }

    // a row's absmax: the lane's tiles, then the row's 16 lanes; BLOCK: then the four waves, through LDS
    InitAcc ar[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ar[r] = InitAcc{0.f, 0.f, 0.0, 0u};
#pragma unroll
        for (int j = 0; j < NTT; ++j) init_take<LQ_INIT_ABSMAX>(y[j][r], ar[r]);      // a masked +0 changes neither maximum
        i8_row_absmax(ar[r]);
    }
    if constexpr (BLOCK) {
        __shared__ float sh_f[2][4][kI8TileLines];
        __shared__ uint32_t sh_u[4][kI8TileLines];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (col == r) {
                sh_f[0][wave][g4 + r] = ar[r].f0;
                sh_f[1][wave][g4 + r] = ar[r].f1;
                sh_u[wave][g4 + r] = ar[r].bad;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ar[r] = InitAcc{0.f, 0.f, 0.0, 0u};
#pragma unroll
            for (int w = 0; w < 4; ++w) init_merge<LQ_INIT_ABSMAX>(ar[r], sh_f[0][w][g4 + r], sh_f[1][w][g4 + r], 0.0, sh_u[w][g4 + r]);
        }
    }

    uint32_t wd[NTT];                                  // the lane's codes of tile j, row r in byte r
#pragma unroll
    for (int j = 0; j < NTT; ++j) wd[j] = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int32_t m = mt * kI8TileLines + g4 + r;
        const bool live_m = m < p.M;
        const float s = i8_row_scale(q.ip, ar[r], p.N, live_m);
        const Ctx c = Step::ctx(q.gp, s);
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            const float qv = Step::quant(q.gp, c, div_by_uniform(y[j][r], c));
            const uint32_t code = (live_n[j] && live_m) ? i8_view_byte(Step::view(q.gp, qv)) : 0u;
            wd[j] |= code << (8 * r);
        }
        if (col == r && live_m && (!BLOCK || wave == 0)) q.scales[m] = s;      // one lane per row
    }
    // lane qd of a quad stores row g4 + qd: the quad's four columns of it, four consecutive bytes of the NHWC row
    const int32_t ms = mt * kI8TileLines + g4 + qd;
    uint8_t* dst = q.codes + (int64_t)ms * q.CPo + (col & ~3);
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        const uint32_t word = mx_quad_gather(wd[j], qd);      // every lane takes part in the transpose
        if (j < own && ms < p.M) *reinterpret_cast<uint32_t*>(dst + (t0 + j) * kI8TileLines) = word;
    }
}

// the instantiation by the padded row's tiles: host side, called from lq_i8_conv2d_quantize (RES = false) and
// lq_i8_conv2d_quantize_residual (RES = true)
template <int STEP, bool RES>
inline void i8_conv2d_quantize_launch(const I8ConvQuantArgs<RES>& q, hipStream_t st) {
    const dim3 blk(kBlock);
    if (q.OT <= 8) {              // a row per wave, four A tiles per block
        const dim3 grid((unsigned)((q.c.MT + 3) / 4));
        if (q.OT <= 2) hipLaunchKernelGGL((k_i8_conv2d_quantize<STEP, 2, false, RES>), grid, blk, 0, st, q);
        else if (q.OT <= 4) hipLaunchKernelGGL((k_i8_conv2d_quantize<STEP, 4, false, RES>), grid, blk, 0, st, q);
        else hipLaunchKernelGGL((k_i8_conv2d_quantize<STEP, 8, false, RES>), grid, blk, 0, st, q);
    } else {                      // a row per block: ceil(OT / 4) tiles on the widest wave
        const dim3 grid((unsigned)q.c.MT);
        if (q.OT <= 16) hipLaunchKernelGGL((k_i8_conv2d_quantize<STEP, 4, true, RES>), grid, blk, 0, st, q);
        else hipLaunchKernelGGL((k_i8_conv2d_quantize<STEP, 8, true, RES>), grid, blk, 0, st, q);
    }
}

}  // namespace lq

#endif
