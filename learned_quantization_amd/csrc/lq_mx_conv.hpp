// lq_mx_conv.hpp -- the packed MX operand of the im2col matrix of a convolution's input, without the matrix
// (lq_hip.h: lq_mx_im2col_dims / lq_mx_operand_im2col)
//
// A[m][k] with m = (b OH + oh) OW + ow and k = (c KH + i) KW + j is X[b][c][oh stride_h - pad_top + i][ow stride_w - pad_left + j]
// where that pixel exists and +0 otherwise; the operand of A is what lq_mx_operand_quantize(A, M, K) writes (lq_mx_operand.hpp: the
// layout, mx_code_offset / mx_scale_offset).  k is the memory order of an OIHW kernel's (ci, kh, kw) run, so the B side is
// lq_mx_operand_pack(kernel, axis 1).
//
// One thread per (line, block of 32 k), as k_mx_operand has it, lines fastest: a thread block is kBlock consecutive lines of ONE k
// block, so (c, i, j) of each of the 32 taps is uniform over the block (scalar registers) and only (b, oh, ow) is per lane.  For an
// NCHW input at stride 1 a wave's load of one tap is 64 consecutive addresses (up to the row ends), and the fragment stores of 16
// neighbouring lines are contiguous.  The geometry and the line's window are lq_im2col.hpp's, shared with k_i8_im2col; the gather
// -- 32 predicated 4-byte loads, zero outside the image and past K -- is im2col_gather's tap walk written out in the kernel, because
// the call measured slower here ("One im2col gather").  The scale rule and the element step are those k_mx_operand
// runs, called, not restated: init_take / init_raw / init_final, GroupStep<true, GroupMxParams>, mx_code_bits.  The few lines
// around them (block scale byte, code packing, fragment stores, idle scale bytes) repeat k_mx_operand's: the two kernels differ in
// what feeds those lines (a strided row there, a gathered window here), and k_mx_operand's instruction streams are pinned
// ("One im2col gather").  No LDS, no scratch, no atomics.
#ifndef LQ_MX_CONV_HPP_
#define LQ_MX_CONV_HPP_
#include "lq_im2col.hpp"
#include "lq_mx_operand.hpp"

namespace lq {

struct MxIm2colParams {
    GroupMxParams mp;         // the format; g.P is X
    InitParams ip;            // emax, mm_frac, min_value
    uint8_t* codes;
    uint8_t* scales;
    Im2colGeom geom;          // geom.M lines; geom.chunks: blockIdx.x -> (k block, chunk of kBlock lines)
    int32_t K, nbk;           // nbk = ceil(K / 32)
    int32_t LT, KT, KG;
};

template <int METHOD, bool FP4>
__global__ __launch_bounds__(kBlock) void k_mx_im2col(const MxIm2colParams op) {
    using Step = GroupStep<true, GroupMxParams>;
    const int32_t kb = (int32_t)fd_div(op.geom.chunks, blockIdx.x);                    // uniform over the block
    const int64_t line = (int64_t)(blockIdx.x - (uint32_t)kb * op.geom.chunks.d) * kBlock + threadIdx.x;
    if (line >= (int64_t)op.LT * kMxTileLines) return;
    const int32_t ln = (int32_t)line;
    const bool live = ln < op.geom.M && kb < op.nbk;
    uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t byte = 127u;
    if (live) {
        const int n = min(kMxBlockLen, op.K - kb * kMxBlockLen);
        const Im2colGeom& g = op.geom;
        const Im2colWindow win = im2col_window(g, ln);
        // im2col_gather<32>, written out: called, it costs this kernel about 9 instructions and 0.4 % on two of nine shapes
        const uint32_t k0 = (uint32_t)kb * kMxBlockLen;
        uint32_t c = fd_div(g.khkw, k0);
        const uint32_t rk = k0 - c * g.khkw.d;
        uint32_t i = fd_div(g.kw, rk), j = rk - i * g.kw.d;
        const float* X = op.mp.g.P;
        float x[kMxBlockLen];
#pragma unroll
        for (int e = 0; e < kMxBlockLen; ++e) {
            const int64_t ih = win.ih0 + i, iw = win.iw0 + j;
            const bool in = e < n && (uint64_t)ih < (uint64_t)g.H && (uint64_t)iw < (uint64_t)g.W;
            x[e] = 0.f;
            if (in) x[e] = X[win.base + (int64_t)c * g.xs_c + (int64_t)i * g.xs_h + (int64_t)j * g.xs_w];
            if (++j == g.kw.d) {
                j = 0u;
                if (++i == (uint32_t)g.KH) { i = 0u; ++c; }
            }
        }
        InitAcc a{0.f, 0.f, 0.0, 0u};      // the zeros of the padding and past n change neither maximum
#pragma unroll
        for (int e = 0; e < kMxBlockLen; ++e) init_take<METHOD>(x[e], a);
        const float s = init_final(op.ip, init_raw<METHOD>(op.ip, a, n), a.bad);
        const Ctx cx = Step::ctx(op.mp, s);
        byte = (cx.s != cx.s) ? 255u : (__float_as_uint(cx.s) >> 23);      // s_eff is a power of two in [2^-126, 2^127], or NaN
#pragma unroll
        for (int e = 0; e < kMxBlockLen; ++e) {
            const float q = Step::quant(op.mp, cx, div_by_uniform(x[e], cx));
            const uint32_t code = e < n ? mx_code_bits(q, op.mp.M, op.mp.emin, op.mp.bits) : 0u;
            if constexpr (FP4) w[e >> 3] |= code << (4 * (e & 7));
            else w[e >> 2] |= code << (8 * (e & 3));
        }
    }
    // as k_mx_operand stores them: fp4 one fragment, fp8 the halves of two; then the scale byte and the idle bytes of steps KT .. 4 KG - 1
    *reinterpret_cast<uint4*>(op.codes + mx_code_offset(op.KT, FP4, ln, kb * kMxBlockLen)) = make_uint4(w[0], w[1], w[2], w[3]);
    if constexpr (!FP4)
        *reinterpret_cast<uint4*>(op.codes + mx_code_offset(op.KT, false, ln, kb * kMxBlockLen + 16)) = make_uint4(w[4], w[5], w[6], w[7]);
    op.scales[mx_scale_offset(op.KG, ln, kb)] = (uint8_t)byte;
    if ((kb >> 2) == op.KT - 1)
        for (int32_t kt = op.KT; kt < 4 * op.KG; ++kt) op.scales[mx_scale_offset(op.KG, ln, kt * 4 + (kb & 3))] = 127u;
}

}  // namespace lq

#endif
