// lq_i8_direct.hpp -- a direct int8 convolution: every pixel quantised once, the windows gathered inside the product
// (lq_hip.h: lq_i8_pixels_quantize / lq_i8_conv_kernel_pack / lq_i8_conv2d)
//
// The im2col path writes an A operand KH KW times the input and reads it back.  Here the input becomes ONE int8 NHWC copy with a
// scale per pixel, the kernel is packed per tap in fragment order, and the product walks the taps: per tap the reduction runs over
// the channels alone, so the int32 sum of a tap is exact and one pixel scale applies to it.
//
//   pixels  codes [B][H][W][CP] int8, CP = 32 ceil(C / 32), channels past C code 0; scales [B][H][W] fp32: the absmax scale of the
//           pixel's C channels and the nearest-even codes under it -- k_i8_quantize's scale rule and element step (init_take /
//           init_raw / init_final, GroupStep<true, GroupParams>, div_by_uniform, i8_view_byte), called, not restated.
//   kernel  codes [NT][KH KW][CS][64 lanes][FB], NT = ceil(co / 16), tap index i KW + j.  CP % 64 == 0: STEP = 64, FB = 16; otherwise
//           STEP = 32, FB = 8; CS = CP / STEP.  Lane l holds filter 16 nt + (l & 15) and channels STEP cs + FB (l >> 4) + jj in byte
//           jj.  scales [16 NT]: one per filter, 1.0f past co.  The element step is k_i8_pack's.
//
// k_i8_pixels: pixels along the lanes, so a wave's load of one channel of an NCHW input is one contiguous run along w; a thread
// walks its pixel's channels in units of 16 (one 16-byte store), keeps the first kI8PixCache units in registers between the maximum
// and the codes (C <= 64: X is read once) and reads the rest a second time, a unit's 16 loads in flight together.  A channel index
// past C is clamped to C - 1 rather than predicated: the load stays inside the pixel, a repeated element changes no maximum, and
// its code is masked to 0 when the unit is written.
//
// k_i8_conv2d<STEP>: the shape of k_i8_gemm -- a wave owns 2 x 2 result tiles, a block of four waves 64 lines x 64 filters, four
// matrix instructions per step, the fragments of the next step requested before this step's instructions, no LDS, only the store
// of Y masked.  What differs is the A side.  The tap loop is wave-uniform ((i, j) in scalar registers); per tap a lane forms, for
// each of its two A tiles, the pixel of ITS line (l & 15) -- the window's corner comes from FastDiv once, before the loop -- and
// loads its fragment straight from the NHWC codes: FB bytes at channel STEP cs + FB (l >> 4).  The 16 lines of a tile under stride 1
// are neighbouring pixels, so the four lane groups together read one contiguous run of 16 CP bytes per STEP.  A lane whose tap lies
// outside the image, or whose line lies past M, holds zero and forms no address.  At the end of a tap the four int32 accumulators
// are converted, multiplied by the scale of the pixel of the result ROW and added into fp32 (__fmul_rn / __fadd_rn: no build
// contracts them).  A result row 4 (l >> 4) + r of a tile is the A line of lane 4 (l >> 4) + r, which loaded that pixel's scale
// when the tap began: the row scales come across by four wave shuffles per tile and tap, not from a second set of windows in
// registers.  A skipped tap adds RN(0 * 0) = +0 to a y that is never -0: the bits of skipping it.
#ifndef LQ_I8_DIRECT_HPP_
#define LQ_I8_DIRECT_HPP_
#include "lq_i8_gemm.hpp"
#include "lq_fastdiv.hpp"

namespace lq {

// A precaution, not arithmetic: the products and sums of the two epilogues are kept in the one-wide fp32 forms (v_mul_f32,
// v_add_f32) that every other result of this path is checked against bit for bit, instead of letting the vectorizer pair them into
// the two-wide v_pk_mul_f32 / v_pk_add_f32.  Both forms are specified to round alike; the helper only takes the choice of form away
// from the compiler.  It is an empty statement that makes a value opaque -- no instruction, no register move, not volatile, so the
// scheduler stays free -- and profiles/i8_direct/resource_usage.txt counts the packed forms in the built kernels (0).
__device__ __forceinline__ float i8_scalar(float v) {
    asm("" : "+v"(v));
    return v;
}

constexpr int kI8PixUnit = 16;        // channels of a unit: one 16-byte store
constexpr int kI8PixCache = 4;        // units per thread held in registers between the scale and the codes: C <= 64 is read once
constexpr int kI8PixAlign = 32;       // CP is a multiple of it: one step of v_mfma_i32_16x16x32_i8

struct I8PixelsParams {
    GroupParams g;            // P = X, lo = -127, hi = 127; nothing else is read
    InitParams ip;            // lo, hi, min_value
    uint8_t* codes;
    float* scales;
    int64_t xs_b, xs_c, xs_h, xs_w;       // of X, in elements
    FastDiv hw, w;            // pixel -> (b, h, w)
    int32_t NP, C, CP;        // pixels B H W; channels read; channels written
};

__global__ __launch_bounds__(kBlock) void k_i8_pixels(const I8PixelsParams op) {
    using Step = GroupStep<true, GroupParams>;
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= op.NP) return;
    const uint32_t b = fd_div(op.hw, (uint32_t)pix), r = (uint32_t)pix - b * op.hw.d;
    const uint32_t h = fd_div(op.w, r), w = r - h * op.w.d;
    const float* src = op.g.P + ((int64_t)b * op.xs_b + (int64_t)h * op.xs_h + (int64_t)w * op.xs_w);
    const int32_t nu = (op.C + kI8PixUnit - 1) / kI8PixUnit, nus = op.CP / kI8PixUnit;      // units read (rounded up), written

    // A channel index past C is clamped to C - 1, not predicated: the load stays inside the pixel, a repeated element changes
    // neither maximum, and its code is masked to 0 when the unit is written -- no branch per element
    const int32_t clast = op.C - 1;
    auto load_unit = [&](int32_t u, float (&xv)[kI8PixUnit]) {
#pragma unroll
        for (int e = 0; e < kI8PixUnit; ++e) xv[e] = src[(int64_t)min(u * kI8PixUnit + e, clast) * op.xs_c];
    };
    float x[kI8PixCache][kI8PixUnit];
    InitAcc a{0.f, 0.f, 0.0, 0u};
#pragma unroll
    for (int it = 0; it < kI8PixCache; ++it) {
#pragma unroll
        for (int e = 0; e < kI8PixUnit; ++e) x[it][e] = 0.f;
        if (it < nu) {                        // kernel-uniform
            load_unit(it, x[it]);
#pragma unroll
            for (int e = 0; e < kI8PixUnit; ++e) init_take<LQ_INIT_ABSMAX>(x[it][e], a);
        }
    }
    for (int32_t u = kI8PixCache; u < nu; ++u) {      // what the registers do not hold: a unit's 16 loads are in flight together
        float t[kI8PixUnit];
        load_unit(u, t);
#pragma unroll
        for (int e = 0; e < kI8PixUnit; ++e) init_take<LQ_INIT_ABSMAX>(t[e], a);
    }
    const float s = init_final(op.ip, init_raw<LQ_INIT_ABSMAX>(op.ip, a, op.C), a.bad);
    op.scales[pix] = s;
    const Ctx cx = Step::ctx(op.g, s);
    uint8_t* dst = op.codes + pix * op.CP;

    auto emit = [&](int32_t c0, const float (&xv)[kI8PixUnit]) {      // c0 < CP; channels at or past C are padding: code 0
        uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < kI8PixUnit; ++e) {
            const float q = Step::quant(op.g, cx, div_by_uniform(xv[e], cx));
            wd[e >> 2] |= (c0 + e < op.C ? i8_view_byte(Step::view(op.g, q)) : 0u) << (8 * (e & 3));
        }
        *reinterpret_cast<uint4*>(dst + c0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    };
#pragma unroll
    for (int it = 0; it < kI8PixCache; ++it) {
        if (it < nus) emit(it * kI8PixUnit, x[it]);      // kernel-uniform
    }
    for (int32_t u = kI8PixCache; u < nus; ++u) {
        float t[kI8PixUnit];
        load_unit(u, t);
        emit(u * kI8PixUnit, t);
    }
}

struct I8ConvPackParams {
    GroupParams g;            // P, s, lo, hi; the geometry fields are not read
    uint8_t* codes;
    float* scales;
    int32_t co, ci, KHKW;
    int32_t NT, CS;
};

// one thread per fragment: (nt, tap, cs, lane), lanes fastest -- the FB-byte stores of a wave are contiguous
template <bool RNE, int STEP>
__global__ __launch_bounds__(kBlock) void k_i8_conv_pack(const I8ConvPackParams op) {
    using Step = GroupStep<RNE, GroupParams>;
    constexpr int FB = STEP / 4;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t frags = (int64_t)op.NT * op.KHKW * op.CS * 64;
    if (tid >= frags) return;
    const int lane = (int)(tid & 63);
    int64_t rest = tid >> 6;
    const int32_t cs = (int32_t)(rest % op.CS);
    rest /= op.CS;
    const int32_t tap = (int32_t)(rest % op.KHKW), nt = (int32_t)(rest / op.KHKW);
    const int32_t n = nt * kI8TileLines + (lane & 15), c0 = STEP * cs + FB * (lane >> 4);
    const bool live = n < op.co;
    const float s = live ? op.g.s[n] : 1.0f;
    uint32_t w[FB / 4];
#pragma unroll
    for (int k = 0; k < FB / 4; ++k) w[k] = 0u;
    if (live) {
        const Ctx c = Step::ctx(op.g, s);
        const float* src = op.g.P + ((int64_t)n * op.ci + c0) * op.KHKW + tap;      // P[n][c][i][j]: the channel stride is KH KW
#pragma unroll
        for (int jj = 0; jj < FB; ++jj) {
            if (c0 + jj < op.ci) {
                const float q = Step::quant(op.g, c, div_by_uniform(src[(int64_t)jj * op.KHKW], c));
                w[jj >> 2] |= i8_view_byte(Step::view(op.g, q)) << (8 * (jj & 3));
            }
        }
    }
    uint8_t* dst = op.codes + tid * FB;
    if constexpr (FB == 16) *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    else *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
    if (tap == 0 && cs == 0 && lane < kI8TileLines) op.scales[n] = s;      // the filter's scale, bit for bit; 1.0f past co
}

struct I8Conv2dParams {
    const uint8_t* pix_codes;
    const float* pix_scales;
    const uint8_t* k_codes;
    const float* k_scales;    // [16 NT]
    const float* bias;        // [co] or NULL
    float* Y;
    int64_t ldy;
    FastDiv ohow, ow;         // line -> (b, oh, ow)
    int32_t M, N;             // lines, filters
    int32_t MT, NT, CS, CP;
    int32_t H, W, KH, KW;
    int32_t stride_h, stride_w, pad_top, pad_left;
};

template <int STEP> struct I8Frag;
template <> struct I8Frag<64> {
    using T = i8_v4i;
    static __device__ __forceinline__ T zero() { return T{0, 0, 0, 0}; }
    static __device__ __forceinline__ T load(const uint8_t* p) {
        return *reinterpret_cast<const T*>(p);
    }
    static __device__ __forceinline__ i8_v4i mfma(T a, T b, i8_v4i c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
};
template <> struct I8Frag<32> {
    using T = long;
    static __device__ __forceinline__ T zero() { return 0l; }
    static __device__ __forceinline__ T load(const uint8_t* p) { return *reinterpret_cast<const long*>(p); }
    static __device__ __forceinline__ i8_v4i mfma(T a, T b, i8_v4i c) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, c, 0, 0, 0); }
};

template <int STEP>
__global__ __launch_bounds__(kBlock) void k_i8_conv2d(const I8Conv2dParams p) {
    using Fr = I8Frag<STEP>;
    using FT = typename Fr::T;
    constexpr int FB = STEP / 4;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int32_t mt0 = ((int32_t)blockIdx.y * 2 + (wave & 1)) * 2;
    const int32_t nt0 = ((int32_t)blockIdx.x * 2 + (wave >> 1)) * 2;
    if (mt0 >= p.MT || nt0 >= p.NT) return;      // wave-uniform; the kernel has no barrier
    const int32_t nt[2] = {nt0, min(nt0 + 1, p.NT - 1)};      // a clamped second tile re-reads the last one

    // the window of the lane's A line in each of its two tiles: the corner, and the first pixel of its image.  A line past M gets
    // a corner that no tap brings inside
    int32_t ih0[2], iw0[2], pb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int32_t m = (mt0 + i) * kI8TileLines + (lane & 15);
        const uint32_t b = fd_div(p.ohow, (uint32_t)m), r = (uint32_t)m - b * p.ohow.d;
        const uint32_t oh = fd_div(p.ow, r), ow = r - oh * p.ow.d;
        ih0[i] = m < p.M ? (int32_t)oh * p.stride_h - p.pad_top : -p.KH;
        iw0[i] = (int32_t)ow * p.stride_w - p.pad_left;
        pb[i] = (int32_t)b * p.H * p.W;
    }
    const int32_t coff = FB * (lane >> 4);                      // the lane's channels inside a step
    const int32_t khkw = p.KH * p.KW;
    const uint8_t* bsrc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) bsrc[j] = p.k_codes + ((int64_t)nt[j] * khkw * p.CS * 64 + lane) * FB;

    i8_v4i acc[2][2];
    float y[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc[i][j] = i8_v4i{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) y[i][j][r] = 0.f;
        }

    // the tap being requested: (ti, tj) and its channel step tcs are wave-uniform; `in` and `pix` are the lane's
    int32_t ti = 0, tj = 0, tcs = 0;
    bool in[2];
    int64_t pix[2];
    float san[2], sa[2] = {0.f, 0.f};
    auto enter_tap = [&]() {      // the lane's pixel under tap (ti, tj), and its scale: +0 where the tap is skipped
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int32_t ih = ih0[i] + ti, iw = iw0[i] + tj;
            in[i] = (uint32_t)ih < (uint32_t)p.H && (uint32_t)iw < (uint32_t)p.W;
            pix[i] = in[i] ? (int64_t)(pb[i] + ih * p.W + iw) : 0;
            san[i] = 0.f;
            if (in[i]) san[i] = p.pix_scales[pix[i]];
        }
    };
    FT a[2], b[2], an[2], bn[2];
    auto request = [&]() {        // the fragments of step (ti, tj, tcs)
        const int64_t boff = ((int64_t)(ti * p.KW + tj) * p.CS + tcs) * (64 * FB);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            an[i] = Fr::zero();
            if (in[i]) an[i] = Fr::load(p.pix_codes + pix[i] * p.CP + (STEP * tcs + coff));
            bn[i] = Fr::load(bsrc[i] + boff);
        }
    };
    enter_tap();
    request();
    const int32_t steps = khkw * p.CS;
    for (int32_t t = 0; t < steps; ++t) {
        // take the fragments requested a step ago, request the next step's, multiply
        const bool first = tcs == 0, last = tcs == p.CS - 1;      // of the tap taken now: wave-uniform
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a[i] = an[i];
            b[i] = bn[i];
            if (first) sa[i] = san[i];
        }
        if (t + 1 < steps) {
            if (++tcs == p.CS) {
                tcs = 0;
                if (++tj == p.KW) { tj = 0; ++ti; }
                enter_tap();
            }
            request();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = Fr::mfma(a[i], b[j], acc[i][j]);
        if (last) {               // the tap ends: its exact sums under the pixel scales of the result rows
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sr = __shfl(sa[i], (lane >> 4) * 4 + r);
#pragma unroll
                    for (int j = 0; j < 2; ++j) y[i][j][r] = i8_scalar(__fadd_rn(y[i][j][r], i8_scalar(__fmul_rn((float)acc[i][j][r], sr))));
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = i8_v4i{0, 0, 0, 0};
            }
        }
    }

    // result tile: column (lane & 15) on the lane, rows 4 (lane >> 4) + r in the registers
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int32_t n = (nt0 + j) * kI8TileLines + (lane & 15);
        if (n >= p.N) continue;
        const float sk = p.k_scales[n];
        const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int32_t m = (mt0 + i) * kI8TileLines + (lane >> 4) * 4 + r;
                const float v = i8_scalar(__fmul_rn(y[i][j][r], sk));
                if (m < p.M) p.Y[(int64_t)m * p.ldy + n] = p.bias ? i8_scalar(__fadd_rn(v, bv)) : v;
            }
    }
}

}  // namespace lq

#endif
