// lq_im2col.hpp -- the im2col matrix of a convolution's input as both operand quantizers read it (lq_mx_conv.hpp, lq_i8_conv.hpp)
//
// A[m][k] is lq_mx_conv.hpp's.  A line m fixes a WINDOW of X, its corner and the corner's offset; a run of k from k0 walks the taps
// (c, i, j) of that window with j fastest.  The kernels keep k0 uniform over a wave, so (c, i, j) of every tap sits in scalar
// registers and only the window is per lane.  Every load is predicated and addressed in int64 through the strides of X (NCHW,
// channels_last or any view with non-negative strides): no address is formed into a load unless the definition names it.
#ifndef LQ_IM2COL_HPP_
#define LQ_IM2COL_HPP_
#include "lq_fastdiv.hpp"

namespace lq {

// what both kernels' parameter structs hold of the convolution, embedded in place: 152 bytes, no tail padding
struct Im2colGeom {
    int64_t xs_b, xs_c, xs_h, xs_w;       // of X, in elements
    int64_t H, W;
    FastDiv ohow, ow;         // m -> (b, oh, ow)
    FastDiv khkw, kw;         // k -> (c, i, j)
    FastDiv chunks;           // blockIdx.x -> (block of k, chunk of lines): the kernel's own cut
    int32_t KH, stride_h, stride_w, pad_top, pad_left;
    int32_t M;                // lines
};
static_assert(sizeof(Im2colGeom) == 152, "the kernel arguments behind the geometry keep their offsets");

// the window of one line: the corner's coordinates and its offset in X (which may lie outside X: it is never loaded from)
struct Im2colWindow { int64_t ih0, iw0, base; };

__device__ __forceinline__ Im2colWindow im2col_window(const Im2colGeom& g, int32_t line) {
    const uint32_t b = fd_div(g.ohow, (uint32_t)line), r = (uint32_t)line - b * g.ohow.d;
    const uint32_t oh = fd_div(g.ow, r), ow = r - oh * g.ow.d;
    const int64_t ih0 = (int64_t)oh * g.stride_h - g.pad_top, iw0 = (int64_t)ow * g.stride_w - g.pad_left;
    return Im2colWindow{ih0, iw0, (int64_t)b * g.xs_b + ih0 * g.xs_h + iw0 * g.xs_w};
}

// N taps from k0 (uniform over the wave) of the line whose window is w; taps at or past n and outside the image are +0
template <int N>
__device__ __forceinline__ void im2col_gather(const Im2colGeom& g, const float* X, const Im2colWindow& w, uint32_t k0, int n,
                                              float (&x)[N]) {
    uint32_t c = fd_div(g.khkw, k0);
    const uint32_t rk = k0 - c * g.khkw.d;
    uint32_t i = fd_div(g.kw, rk), j = rk - i * g.kw.d;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int64_t ih = w.ih0 + i, iw = w.iw0 + j;
        const bool in = e < n && (uint64_t)ih < (uint64_t)g.H && (uint64_t)iw < (uint64_t)g.W;
        x[e] = 0.f;
        if (in) x[e] = X[w.base + (int64_t)c * g.xs_c + (int64_t)i * g.xs_h + (int64_t)j * g.xs_w];
        if (++j == g.kw.d) {
            j = 0u;
            if (++i == (uint32_t)g.KH) { i = 0u; ++c; }
        }
    }
}

}  // namespace lq

#endif
