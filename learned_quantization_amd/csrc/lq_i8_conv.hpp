// lq_i8_conv.hpp -- the packed int8 operand of the im2col matrix of a convolution's input, without the matrix
// (lq_hip.h: lq_i8_operand_im2col)
//
// A[m][k] is lq_mx_conv.hpp's: m = (b OH + oh) OW + ow, k = (c KH + i) KW + j, the pixel where it exists and +0 otherwise.  The
// operand of A is what lq_i8_operand_quantize(A, M, K, block) writes (lq_i8_operand.hpp: the layout, i8_code_offset): one fp32
// absmax scale per (line, scale block) -- the whole row for block == 0 -- and the clipped nearest-even codes under it.
//
// The gather of lq_im2col.hpp, which k_mx_im2col shares, around the scale rule and element step of k_i8_quantize.  Lines lie
// along the lanes: a thread block is kBlock / S consecutive lines of ONE scale block, so (c, i, j) of every tap is uniform over a
// wave (scalar registers), a wave's load of one tap of an NCHW input at stride 1 is one contiguous run, and the 16-byte code
// stores of 16 neighbouring lines are contiguous 256 B.  A UNIT is 16 consecutive k from a multiple of 16: one 16-byte fragment of a line.  The span of a work item
// (line, scale block) is cut into units, and S SLICES -- the S waves of the thread block -- take the units s, s + S, ...:
// with one scale per row a late-network shape has few lines and a long row, and one thread per line would leave the device idle.
// Two passes: maxima, then codes.  A slice keeps its first kI8ConvCache units (16 floats each) in registers between them and
// gathers the rest a second time, from the cache hierarchy.  The host launches the plain form (S == 1) only for spans of at most
// kI8ConvCache units -- one K step of the instruction --, so that form has no second gather.  The slices' absmax partials are two maxima and an OR, merged through
// LDS by every thread for its own line: order-free, therefore exact.  The last scale block of a line writes the k padding up to
// 64 KT; lines past M up to 16 LT get codes 0 and scale 1.0f; slice 0 writes the scale.  Geometry, window and the predicated
// loads are lq_im2col.hpp's.  The arithmetic is called, not restated: init_take / init_merge / init_raw / init_final, GroupStep<true,
// GroupParams>, div_by_uniform, i8_view_byte.  The few lines around them repeat k_i8_quantize's: that kernel walks a row with a
// team of lanes, this one a window with one lane per line, and k_i8_quantize's instruction streams are pinned ("One
// im2col gather").  No scratch, no atomics.
#ifndef LQ_I8_CONV_HPP_
#define LQ_I8_CONV_HPP_
#include "lq_i8_operand.hpp"
#include "lq_im2col.hpp"

namespace lq {

constexpr int kI8ConvUnit = 16;       // k of a unit: one 16-byte fragment of a line
constexpr int kI8ConvCache = 4;       // units per thread held in registers between the scale and the codes
constexpr int kI8ConvSlices = 4;      // slices of the split form: one wave each

struct I8Im2colParams {
    GroupParams g;            // P = X, lo = -127, hi = 127; nothing else is read
    InitParams ip;            // lo, hi, min_value
    uint8_t* codes;
    float* scales;
    Im2colGeom geom;          // geom.M lines; geom.chunks: blockIdx.x -> (scale block, chunk of kBlock / S lines)
    int32_t K, block;         // block == 0: one scale per line
    int32_t nbs, LT, KT;
};

// S slices of kBlock / S lines each.  S == 1: a thread owns its (line, scale block), whose span is at most kI8ConvCache units;
// S == kI8ConvSlices: a wave per slice
template <int S>
__global__ __launch_bounds__(kBlock) void k_i8_im2col(const I8Im2colParams op) {
    using Step = GroupStep<true, GroupParams>;
    constexpr int kLines = kBlock / S;
    static_assert(S == 1 || kLines == 64, "a slice is one wave: its units are wave-uniform");
    const int32_t sb = (int32_t)fd_div(op.geom.chunks, blockIdx.x);                    // uniform over the block
    const int32_t slice = S == 1 ? 0 : __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x / kLines));
    const int64_t lines = (int64_t)op.LT * kI8TileLines;
    const int64_t line = (int64_t)(blockIdx.x - (uint32_t)sb * op.geom.chunks.d) * kLines + (threadIdx.x % kLines);
    const bool valid = line < lines;          // no early return: the split form meets at a barrier
    const int32_t ln = (int32_t)line;
    const bool live = valid && ln < op.geom.M;
    const int32_t span = op.block ? op.block : op.K;
    const int32_t c0 = sb * span;                                         // < K: nbs = ceil(K / block)
    const int32_t c1 = min(c0 + span, op.K);                              // elements read
    const int32_t c1s = sb == op.nbs - 1 ? op.KT * kI8TileK : c0 + span;  // codes written: the last block writes the padding of k
    // in units from c0, so that no index past the span is ever formed: those read (rounded up) and those written
    const int32_t nu1 = (c1 - c0 + kI8ConvUnit - 1) / kI8ConvUnit, nus = (c1s - c0) / kI8ConvUnit;

    Im2colWindow w{0, 0, 0};
    if (live) w = im2col_window(op.geom, ln);
    float x[kI8ConvCache][kI8ConvUnit];
    InitAcc a{0.f, 0.f, 0.0, 0u};             // the zeros of the padding and past c1 change neither maximum
#pragma unroll
    for (int it = 0; it < kI8ConvCache; ++it) {
#pragma unroll
        for (int e = 0; e < kI8ConvUnit; ++e) x[it][e] = 0.f;
        if (slice + it * S >= nu1) continue;  // wave-uniform
        if (live) {
            const int32_t k0 = c0 + (slice + it * S) * kI8ConvUnit;      // taps at or past c1 are +0
            im2col_gather(op.geom, op.g.P, w, (uint32_t)k0, c1 - k0, x[it]);
#pragma unroll
            for (int e = 0; e < kI8ConvUnit; ++e) init_take<LQ_INIT_ABSMAX>(x[it][e], a);
        }
    }
    if constexpr (S > 1) {
        for (int32_t u = slice + kI8ConvCache * S; u < nu1; u += S) {      // what the registers do not hold
            if (live) {
                float t[kI8ConvUnit];
                const int32_t k0 = c0 + u * kI8ConvUnit;
                im2col_gather(op.geom, op.g.P, w, (uint32_t)k0, c1 - k0, t);
#pragma unroll
                for (int e = 0; e < kI8ConvUnit; ++e) init_take<LQ_INIT_ABSMAX>(t[e], a);
            }
        }
        // every thread merges the S partials of its own line: two maxima and an OR
        __shared__ float sh_f0[S][kLines], sh_f1[S][kLines];
        __shared__ uint32_t sh_bad[S][kLines];
        const int tl = (int)(threadIdx.x % kLines);
        sh_f0[slice][tl] = a.f0;
        sh_f1[slice][tl] = a.f1;
        sh_bad[slice][tl] = a.bad;
        __syncthreads();
        a = InitAcc{0.f, 0.f, 0.0, 0u};
#pragma unroll
        for (int s = 0; s < S; ++s) init_merge<LQ_INIT_ABSMAX>(a, sh_f0[s][tl], sh_f1[s][tl], 0.0, sh_bad[s][tl]);
    }
    if (!valid) return;
    const float s = live ? init_final(op.ip, init_raw<LQ_INIT_ABSMAX>(op.ip, a, c1 - c0), a.bad) : 1.0f;
    if (slice == 0) op.scales[(int64_t)sb * lines + ln] = s;
    const Ctx cx = Step::ctx(op.g, s);
    const int32_t c1l = live ? c1 : c0;       // a line past M holds code 0 throughout

    auto emit = [&](int32_t k0, const float (&xv)[kI8ConvUnit]) {      // k0 < c1s; elements at or past c1l are padding: code 0
        uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < kI8ConvUnit; ++e) {
            if (k0 + e < c1l) {
                const float q = Step::quant(op.g, cx, div_by_uniform(xv[e], cx));
                wd[e >> 2] |= i8_view_byte(Step::view(op.g, q)) << (8 * (e & 3));
            }
        }
        *reinterpret_cast<uint4*>(op.codes + i8_code_offset(op.KT, ln, k0)) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    };
#pragma unroll
    for (int it = 0; it < kI8ConvCache; ++it) {
        if (slice + it * S < nus) emit(c0 + (slice + it * S) * kI8ConvUnit, x[it]);      // wave-uniform
    }
    if constexpr (S > 1) {
        for (int32_t u = slice + kI8ConvCache * S; u < nus; u += S) {
            const int32_t k0 = c0 + u * kI8ConvUnit;
            float t[kI8ConvUnit];
#pragma unroll
            for (int e = 0; e < kI8ConvUnit; ++e) t[e] = 0.f;
            if (k0 < c1l) im2col_gather(op.geom, op.g.P, w, (uint32_t)k0, c1 - k0, t);
            emit(k0, t);
        }
    }
}

}  // namespace lq

#endif
