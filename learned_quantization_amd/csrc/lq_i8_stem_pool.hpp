// lq_i8_stem_pool.hpp -- the stem convolution whose epilogue takes the OVERLAPPING 3 x 3 / 2 maximum and writes the next conv's
// pixel operand of the POOLED image (lq_hip.h: lq_i8_stem_conv2d_quantize_pool)
//
// conv -> relu / BatchNorm affine -> pad(-inf) -> MaxPool(3, 2) -> the next conv's pixel operand in ONE launch: the largest
// activation of a ResNet never exists in fp32.  The staging, the gather and the epilogue value are k_i8_stem_conv2d's steps
// (lq_i8_stem.hpp), as device functions below; the split of the work is this kernel's own, because that kernel's tile -- 16
// consecutive output lines -- holds no window whole.
//
// Pooled geometry.  PH = (OH + pt + pb - 3) / 2 + 1, PW likewise (floored), paddings in {0, 1}.  Pooled pixel (ph, pw) is the
// maximum over conv rows 2 ph - pt + {0, 1, 2} and conv columns 2 pw - pl + {0, 1, 2}; a row or column outside the conv output is
// the -inf padding, which never wins.  With paddings <= 1 every window holds a real element.
//
// Unit.  A wave owns a STRIP of 16 consecutive conv columns by all NTT column tiles, and walks down R = kI8StemPoolRows pooled rows.
// Strip t starts at the window start of pooled column 7 t, conv column 14 t - pl, and strips step 14 columns: local columns 0 .. 14
// hold the seven windows 2 k + {0, 1, 2}, k = 0 .. 6, whole; local column 15 is computed and never read.  The recompute factor is
// 16 / 14 across and (2 R + 1) / (2 R) down.  Units are numbered strip fastest, so the four waves of a block gather from the same
// image rows; the block stages the kernel operand in LDS once, as k_i8_stem_conv2d does.
//
// A conv row.  The 16 A lines of a strip lie in ONE conv row, so the image row of kernel row i and with it the row scale are
// wave-uniform: the scale is the lane's own load and no shuffle brings it.  The sums and roundings are k_i8_stem_conv2d's, in its
// order, so v is the value lq_i8_stem_conv2d_quantize quantises, bit for bit.  In the 16 x 16 result a lane holds channel
// (lane & 15) of tile j and, in its four registers, conv columns 4 g + r of the strip, g = lane >> 4.  A column outside [0, OW) and
// a whole row outside [0, OH) become -inf here (dead lines: a row outside is not computed at all).
//
// Vertical.  Per pooled row the two new conv rows are computed and the third is carried: row 2 p + 2 - pt of one window is row
// 2 (p + 1) - pt of the next.  The maximum over the three is elementwise over registers of identical layout: no cross-lane step.
// Horizontal.  Window 2 g is registers 0, 1, 2; window 2 g + 1 is registers 2, 3 and register 0 of lane + 16 -- ONE exchange per
// tile and pooled row.  Group 3's second window would be the strip's eighth: dead.  The maximum is i8_pool4's rule (u > m || u != u):
// a NaN is sticky, -inf never wins over a real element.
//
// Scale, codes, store.  A lane holds two pooled pixels (w = 0, 1) by NTT tiles.  Per pixel: absmax over the lane's tiles and the 16
// lanes of its group (i8_row_absmax), i8_row_scale, the quantizer's element step; byte t of word jj is tile 4 jj + t, and the quad
// transpose (mx_quad_gather) over the TILE index leaves lane qd with the quad's four channels of tile 4 jj + qd: one dword of the
// pooled pixel's NHWC row.  One lane per pixel stores the scale.  No atomics, no memset, no workspace; the one barrier follows
// the staging (profiles/i8_stem_pool/kernel_resources.txt).
#ifndef LQ_I8_STEM_POOL_HPP_
#define LQ_I8_STEM_POOL_HPP_
#include "lq_i8_stem.hpp"

namespace lq {

constexpr int kI8StemPoolWindows = 7;     // whole windows of a strip of 16 conv columns
constexpr int kI8StemPoolRows = 4;        // pooled rows a wave walks: 9 conv rows for 8; 3584 units at the ResNet stem, batch 32

struct I8StemPoolParams : I8ConvQuantParams {
    FastDiv ts, rb;           // unit -> (image, row block, strip): strips of a pooled row, row blocks of an image
    int32_t OH, OW;           // the conv output
    int32_t PH, PW;           // the pooled image
    int32_t pool_top, pool_left;
    int32_t R;                // pooled rows of a row block
    int32_t units;            // B * row blocks * strips
};

// Three steps of k_i8_stem_conv2d as device functions.  That kernel states them inline and, like every shipped kernel, keeps its
// instruction stream (profiles/i8_stem_pool/asm_compare.txt), so the steps are stated twice: an edit here is an edit there.
// Staging: the block's column tiles [nt0, nt0 + NTT) are one contiguous run of the operand; a tile past NT is zero, and masked by
// the caller.  The caller's barrier follows
template <int NTT>
__device__ __forceinline__ void i8_stem_stage(uint4* lds, const I8Conv2dParams& p, int32_t nt0) {
    const int32_t have = max(0, min(NTT, p.NT - nt0)) * p.KH * 32, all = NTT * p.KH * 32;      // in 16-byte units
    const uint4* srcv = reinterpret_cast<const uint4*>(p.k_codes + (int64_t)nt0 * p.KH * 512);
    for (int32_t u = (int32_t)threadIdx.x; u < all; u += kBlock) lds[u] = u < have ? srcv[u] : make_uint4(0u, 0u, 0u, 0u);
}

// Gather: the lane's fragment of image row ih (of the image whose first row is rb) -- pixels px0 and px1, inside [0, W) where in0 /
// in1 say so -- and the row's scale: zero where skipped, and no address formed
__device__ __forceinline__ void i8_stem_gather(const I8Conv2dParams& p, const uint32_t* codes, int32_t rb, int32_t ih, int32_t px0,
                                               int32_t px1, bool in0, bool in1, uint32_t& an0, uint32_t& an1, float& san) {
    const bool inr = (uint32_t)ih < (uint32_t)p.H;
    const int32_t row = inr ? rb + ih : 0;
    an0 = 0u;
    an1 = 0u;
    san = 0.f;
    if (inr) san = p.pix_scales[row];
    if (inr && in0) an0 = codes[(int64_t)row * p.W + px0];
    if (inr && in1) an1 = codes[(int64_t)row * p.W + px1];
}

// Epilogue value: the filter's scale, the bias, activation and affine in the order affine_first says, in the one-wide fp32 forms
__device__ __forceinline__ float i8_stem_value(const I8ConvQuantParams& q, float y, float sk, float bv, float ps, float ph) {
    float v = i8_scalar(__fmul_rn(y, sk));
    if (q.c.bias) v = i8_scalar(__fadd_rn(v, bv));
    if (q.post_scale && q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
    if (q.act == LQ_ACT_RELU) v = i8_relu(v);
    if (q.post_scale && !q.affine_first) v = i8_scalar(__fadd_rn(i8_scalar(__fmul_rn(v, ps)), ph));
    return v;
}
// torch's maximum, one member at a time: a later member wins only if greater, or a NaN (i8_pool4's rule)
__device__ __forceinline__ void i8_pool_take(float& m, float u) {
    if (u > m || u != u) m = u;
}

template <int NTT>
__global__ __launch_bounds__(kBlock) void k_i8_stem_conv2d_quantize_pool(const I8StemPoolParams q) {
    using Step = GroupStep<true, GroupParams>;
    constexpr int NW = (NTT + 3) / 4;                 // code words of a lane and pixel: byte t of word jj is tile 4 jj + t
    const I8Conv2dParams& p = q.c;
    extern __shared__ uint4 stem_pool_lds[];          // [NTT][KH][64 lanes] fragments of 8 bytes
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    i8_stem_stage<NTT>(stem_pool_lds, p, 0);
    __syncthreads();
    const int32_t unit = (int32_t)blockIdx.x * (kBlock / 64) + wave;
    if (unit >= q.units) return;                      // wave-uniform, and behind the only barrier
    const long* bl = reinterpret_cast<const long*>(stem_pool_lds) + lane;
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(p.pix_codes);
    const int col = lane & 15, g = lane >> 4, qd = lane & 3;
    const float dead = -__builtin_huge_valf();

    const uint32_t ub = fd_div(q.ts, (uint32_t)unit), t = (uint32_t)unit - ub * q.ts.d;
    const uint32_t b = fd_div(q.rb, ub), rk = ub - b * q.rb.d;
    // the lane's A line is conv column c0 + col of whichever row is being computed; one outside [0, OW) forms no address
    const int32_t c0 = 2 * kI8StemPoolWindows * (int32_t)t - q.pool_left;
    const bool line_in = (uint32_t)(c0 + col) < (uint32_t)q.OW;
    const int32_t px0 = line_in ? (c0 + col) * p.stride_w - p.pad_left + 2 * g : -1, px1 = line_in ? px0 + 1 : -1;
    const bool in0 = (uint32_t)px0 < (uint32_t)p.W, in1 = (uint32_t)px1 < (uint32_t)p.W;
    const int32_t rbase = (int32_t)b * p.H;
    bool col_in[4];                                   // of the lane's result registers: conv column c0 + 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) col_in[r] = (uint32_t)(c0 + 4 * g + r) < (uint32_t)q.OW;

    bool live_n[NTT];
#pragma unroll
    for (int j = 0; j < NTT; ++j) live_n[j] = j < q.OT && j * kI8TileLines + col < p.N;

    // conv row oh of the strip after the epilogue, dead lines as -inf: v[j][r] is channel 16 j + col at conv column c0 + 4 g + r
    auto conv_row = [&](int32_t oh, float (&v)[NTT][4]) {
        if ((uint32_t)oh >= (uint32_t)q.OH) {         // wave-uniform
#pragma unroll
            for (int j = 0; j < NTT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[j][r] = dead;
            return;
        }
        const int32_t ih0 = oh * p.stride_h - p.pad_top;
        float y[NTT][4];
#pragma unroll
        for (int j = 0; j < NTT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[j][r] = 0.f;
        uint32_t an0 = 0u, an1 = 0u;
        float san = 0.f;
        i8_stem_gather(p, codes, rbase, ih0, px0, px1, in0, in1, an0, an1, san);
        for (int32_t i = 0; i < p.KH; ++i) {
            // take the fragment requested a row ago, request the next row's, multiply
            const long a = (long)(((uint64_t)an1 << 32) | (uint64_t)an0);
            const float sa = san;                     // the image row's scale: the same on every lane
            if (i + 1 < p.KH) i8_stem_gather(p, codes, rbase, ih0 + i + 1, px0, px1, in0, in1, an0, an1, san);
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                const i8_v4i acc = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, bl[(j * p.KH + i) * 64], i8_v4i{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) y[j][r] = i8_scalar(__fadd_rn(y[j][r], i8_scalar(__fmul_rn((float)acc[r], sa))));
            }
        }
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            const int32_t n = j * kI8TileLines + col;
            const float sk = live_n[j] ? p.k_scales[n] : 1.0f;
            const float bv = (p.bias && live_n[j]) ? p.bias[n] : 0.f;
            const float ps = (q.post_scale && live_n[j]) ? q.post_scale[n] : 0.f;
            const float ph = (q.post_scale && live_n[j]) ? q.post_shift[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[j][r] = col_in[r] ? i8_stem_value(q, y[j][r], sk, bv, ps, ph) : dead;
        }
    };

    const int32_t p0 = (int32_t)rk * q.R, p1 = min(p0 + q.R, q.PH);
    float carry[NTT][4];                              // the third row of the window above; nothing above the first
#pragma unroll
    for (int j = 0; j < NTT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) carry[j][r] = dead;

    for (int32_t pp = p0; pp < p1; ++pp) {
        const int32_t oh = 2 * pp - q.pool_top;
        float m[NTT][4];
#pragma unroll
        for (int j = 0; j < NTT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) m[j][r] = carry[j][r];
#pragma unroll 1
        for (int32_t e = pp == p0 ? 0 : 1; e < 3; ++e) {      // the walk's first window computes all three rows
            conv_row(oh + e, carry);
#pragma unroll
            for (int j = 0; j < NTT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) i8_pool_take(m[j][r], carry[j][r]);
        }

        // the lane's two windows: pooled columns 7 t + 2 g + w; the strip's eighth and what lies past PW are not written
        const int32_t pw0 = kI8StemPoolWindows * (int32_t)t + 2 * g;
        const bool live_px[2] = {pw0 < q.PW, g < 3 && pw0 + 1 < q.PW};
        float pv[2][NTT];
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            const float x = __shfl(m[j][0], (lane + 16) & 63);        // register 0 of the next group; every lane takes part
            float wa = m[j][0], wb = m[j][2];
            i8_pool_take(wa, m[j][1]);
            i8_pool_take(wa, m[j][2]);
            i8_pool_take(wb, m[j][3]);
            i8_pool_take(wb, g < 3 ? x : dead);
            pv[0][j] = (live_n[j] && live_px[0]) ? wa : 0.f;
            pv[1][j] = (live_n[j] && live_px[1]) ? wb : 0.f;
        }
        const int64_t pm0 = ((int64_t)((int32_t)b * q.PH + pp)) * q.PW + pw0;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            InitAcc ar{0.f, 0.f, 0.0, 0u};
#pragma unroll
            for (int j = 0; j < NTT; ++j) init_take<LQ_INIT_ABSMAX>(pv[w][j], ar);      // a masked +0 changes neither maximum
            i8_row_absmax(ar);
            const float s = i8_row_scale(q.ip, ar, p.N, live_px[w]);
            const Ctx c = Step::ctx(q.gp, s);
            uint32_t wd[NW];
#pragma unroll
            for (int jj = 0; jj < NW; ++jj) wd[jj] = 0u;
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                const float qv = Step::quant(q.gp, c, div_by_uniform(pv[w][j], c));
                const uint32_t code = (live_n[j] && live_px[w]) ? i8_view_byte(Step::view(q.gp, qv)) : 0u;
                wd[j >> 2] |= code << (8 * (j & 3));
            }
            const int64_t pm = pm0 + w;
            if (col == 0 && live_px[w]) q.scales[pm] = s;     // one lane per pooled pixel
            // lane qd of a quad stores tile 4 jj + qd: the quad's four channels of it, four consecutive bytes of the pooled NHWC row
            uint8_t* dst = q.codes + pm * q.CPo + (col & ~3);
#pragma unroll
            for (int jj = 0; jj < NW; ++jj) {
                const uint32_t word = mx_quad_gather(wd[jj], qd);     // every lane takes part in the transpose
                const int32_t j = 4 * jj + qd;
                if (j < q.OT && j < NTT && live_px[w]) *reinterpret_cast<uint32_t*>(dst + j * kI8TileLines) = word;
            }
        }
    }
}

// the instantiation by the padded row's tiles, beside i8_stem_conv2d_launch: host side, called from lq_i8_stem_conv2d_quantize_pool
inline void i8_stem_conv2d_quantize_pool_launch(const I8StemPoolParams& q, hipStream_t st) {
    const int per = kBlock / 64;                      // a unit per wave
    const dim3 grid((unsigned)((q.units + per - 1) / per)), blk(kBlock);
    const int ntt = q.OT <= 2 ? 2 : q.OT <= 4 ? 4 : kI8StemMaxTiles;
    const size_t lds = (size_t)ntt * q.c.KH * 512;
    if (ntt == 2) hipLaunchKernelGGL((k_i8_stem_conv2d_quantize_pool<2>), grid, blk, lds, st, q);
    else if (ntt == 4) hipLaunchKernelGGL((k_i8_stem_conv2d_quantize_pool<4>), grid, blk, lds, st, q);
    else hipLaunchKernelGGL((k_i8_stem_conv2d_quantize_pool<8>), grid, blk, lds, st, q);
}

}  // namespace lq

#endif
