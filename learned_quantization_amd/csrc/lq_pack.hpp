// lq_pack.hpp -- lossless bit-packed integer view (export.save_packed_parameters / load_packed_parameters)
//
// The reference exports floor(P/s) cast to int8 (CIFAR-10/nested_quantization_layer/utils/log_scripts.py:61-97), which wraps
// whenever |q| > 127.  Here every integer q = floor(P/s) (custom_layers.py:55-60, the quotient of K1) is stored as the code
// c = q - qmin of `bits` bits, LSB-first in a little-endian stream of uint32 words: element i occupies stream bits
// [i*bits, i*bits + bits), stream bit j is bit (j mod 32) of word j/32; ceil(n*bits/32) words, pad bits 0.
//
// Geometry: one wave64 owns 2048 consecutive elements = 64*bits words, so no two waves share a word (no atomics,
// deterministic).  Lane l loads float4s k*256 + 4l (k = 0..7, coalesced), the codes are staged through LDS (one pad dword per
// 32: lane l's run of 32 codes then starts on bank l), lane l assembles the `bits` words of codes [32l, 32l + 32) and stages
// them again, and the wave stores its run with one coalesced dword per lane and word row.  Unpack is the mirror image.
// The quotient is K1's own: div_ctx + fq_core4 (lq_math.hpp) when the four elements of a float4 share a row of the group
// descriptor, div_ctx + fq_core per element otherwise.  Tensors below 2^31 elements (weights): 32-bit indices, lq_fastdiv.
#ifndef LQ_PACK_HPP_
#define LQ_PACK_HPP_
#include "lq_math.hpp"

namespace lq {

constexpr int kPackWaves = 4;                               // waves per block
constexpr int kPackElems = 2048;                            // elements per wave (64 lanes x 32 codes)
constexpr int kPackLds = kPackElems + kPackElems / 32;      // dwords of LDS per wave, padded
constexpr float kQIntLimit = 2147483520.0f;                 // largest float below 2^31: the range lq_q_minmax counts

__device__ __forceinline__ int pack_pad(int j) { return j + (j >> 5); }

// scales of elements i .. i+3 and whether they share one row (then one division context serves all four)
struct Scale4 {
    float4 s;
    bool one;
};

__device__ __forceinline__ Scale4 scales4(const float* __restrict__ s, const FastDiv& fin, const FastDiv& fG, uint32_t i) {
    Scale4 r;
    const uint32_t r0 = fd_div(fin, i), r3 = fd_div(fin, i + 3u);
    r.one = r0 == r3;
    if (r.one) {
        const float v = s[fd_mod(fG, r0)];
        r.s = make_float4(v, v, v, v);
    } else {
        r.s.x = s[fd_mod(fG, r0)];
        r.s.y = s[fd_mod(fG, fd_div(fin, i + 1u))];
        r.s.z = s[fd_mod(fG, fd_div(fin, i + 2u))];
        r.s.w = s[fd_mod(fG, r3)];
    }
    return r;
}

__device__ __forceinline__ float quot1(float x, float sv) {
    Ctx c{};
    c.s = sv;
    div_ctx(c);
    float q, o;
    fq_core(x, c, q, o);
    return q;
}

// floor(x / s) of four elements with K1's division (custom_layers.py:56-59)
__device__ __forceinline__ float4 quot4(const float4& x, const Scale4& sc) {
    float4 q;
    if (sc.one) {
        Ctx c{};
        c.s = sc.s.x;
        div_ctx(c);
        float4 o;
        fq_core4(x, c, q, o);
    } else {
        q.x = quot1(x.x, sc.s.x);
        q.y = quot1(x.y, sc.s.y);
        q.z = quot1(x.z, sc.s.z);
        q.w = quot1(x.w, sc.s.w);
    }
    return q;
}

// (q + 1/2) * s floors back to q for |q| < 2^22 (q + 1/2 exact, two roundings of 2^-24 stay inside [q + 1/4, q + 3/4]).
// Beyond, q + 1/2 can round to q + 1: the quotient is monotonic in p, so a few one-ulp steps against the error find a float
// inside [q*s, (q+1)*s) when there is one (always for a power-of-two s).  Returns whether p now floors to q.
__device__ __noinline__ bool restore_fixup(float& p, float q, float sv) {
    for (int step = 0; step < 8; ++step) {
        const float b = quot1(p, sv);
        if (b == q) return true;
        p = nextafterf(p, b > q ? -INFINITY : INFINITY);
    }
    return quot1(p, sv) == q;
}

__device__ __forceinline__ float f4get(const float4& v, int u) { return u == 0 ? v.x : (u == 1 ? v.y : (u == 2 ? v.z : v.w)); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// words[ceil(n*bits/32)] <- codes floor(P/s) - qmin.  bad += elements whose quotient is NaN, +-Inf, outside the range
// lq_q_minmax counts, or outside [qmin, qmin + 2^bits - 1] (such an element is stored as code 0).
__global__ __launch_bounds__(kPackWaves * 64) void k_q_pack(const float* __restrict__ P, const float* __restrict__ s, int32_t qmin,
                                                            int bits, uint32_t* __restrict__ words, unsigned long long* bad,
                                                            uint32_t n, uint64_t nwords, FastDiv fin, FastDiv fG) {
    __shared__ uint32_t lds[kPackWaves * kPackLds];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* buf = lds + wv * kPackLds;
    const uint32_t wave = blockIdx.x * kPackWaves + wv;
    const uint32_t base = wave * (uint32_t)kPackElems;     // n < 2^31: no overflow for any wave of the grid
    const int64_t cmax = (int64_t)((1ull << bits) - 1ull);
    float4 x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {                          // every load in flight before the first division
        const uint32_t i = base + (uint32_t)(k * 256 + lane * 4);
        if (i + 4u <= n) {
            x[k] = *reinterpret_cast<const float4*>(P + i);
        } else {
            x[k].x = i < n ? P[i] : 0.0f;
            x[k].y = i + 1u < n ? P[i + 1u] : 0.0f;
            x[k].z = i + 2u < n ? P[i + 2u] : 0.0f;
            x[k].w = i + 3u < n ? P[i + 3u] : 0.0f;
        }
    }
    uint32_t nbad = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t i = base + (uint32_t)(k * 256 + lane * 4);
        const float4 q = quot4(x[k], scales4(s, fin, fG, i));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float qf = f4get(q, u);
            uint32_t c = 0u;
            if (i + (uint32_t)u < n) {
                const bool fin_q = fabsf(qf) < kQIntLimit;  // false for NaN and +-Inf
                const int64_t d = fin_q ? (int64_t)qf - (int64_t)qmin : -1;
                const bool ok = d >= 0 && d <= cmax;
                c = ok ? (uint32_t)d : 0u;
                nbad += ok ? 0u : 1u;
            }
            buf[pack_pad(k * 256 + lane * 4 + u)] = c;
        }
    }
    __syncthreads();
    uint32_t c[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) c[e] = buf[pack_pad(lane * 32 + e)];
    __syncthreads();
    uint64_t acc = 0;
    int nb = 0, t = 0;
#pragma unroll
    for (int e = 0; e < 32; ++e) {                         // LSB-first: code e at bits [e*bits, e*bits + bits) of the lane's run
        acc |= (uint64_t)c[e] << nb;
        nb += bits;
        if (nb >= 32) {
            buf[pack_pad(lane * bits + t)] = (uint32_t)acc;
            ++t;
            acc >>= 32;
            nb -= 32;
        }
    }
    __syncthreads();
    const uint64_t wbase = (uint64_t)wave * 64u * (uint64_t)bits;
    for (int r = 0; r < bits; ++r) {                       // the wave's run: 64*bits consecutive words
        const int j = r * 64 + lane;
        if (wbase + (uint64_t)j < nwords) words[wbase + (uint64_t)j] = buf[pack_pad(j)];
    }
    nbad = wave_sum_u32(nbad);
    if (lane == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
}

// codes -> q = qmin + c (int32), out = (float)q * s (= K1's out), p_restore = (q + 1/2) * s; every p_restore is divided back with
// K1's division and an element whose floor is not q counts into bad (as does a code whose q leaves int32).
__global__ __launch_bounds__(kPackWaves * 64) void k_q_unpack(const uint32_t* __restrict__ words, int32_t qmin, int bits,
                                                              const float* __restrict__ s, float* __restrict__ out,
                                                              int32_t* __restrict__ qo, float* __restrict__ pr,
                                                              unsigned long long* bad, uint32_t n, uint64_t nwords, FastDiv fin,
                                                              FastDiv fG) {
    __shared__ uint32_t lds[kPackWaves * kPackLds];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* buf = lds + wv * kPackLds;
    const uint32_t wave = blockIdx.x * kPackWaves + wv;
    const uint32_t base = wave * (uint32_t)kPackElems;
    const uint64_t wbase = (uint64_t)wave * 64u * (uint64_t)bits;
    for (int r = 0; r < bits; ++r) {
        const int j = r * 64 + lane;
        buf[pack_pad(j)] = wbase + (uint64_t)j < nwords ? words[wbase + (uint64_t)j] : 0u;
    }
    __syncthreads();
    const uint64_t mask = (1ull << bits) - 1ull;           // bits <= 32
    uint32_t c[32];
    uint64_t acc = 0;
    int nb = 0, t = 0;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        if (nb < bits) {
            acc |= (uint64_t)buf[pack_pad(lane * bits + t)] << nb;
            ++t;
            nb += 32;
        }
        c[e] = (uint32_t)(acc & mask);
        acc >>= bits;
        nb -= bits;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 32; ++e) buf[pack_pad(lane * 32 + e)] = c[e];
    __syncthreads();
    uint32_t nbad = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t i = base + (uint32_t)(k * 256 + lane * 4);
        if (i >= n) break;
        const Scale4 sc = scales4(s, fin, fG, i);
        int32_t qa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t v = (int64_t)qmin + (int64_t)buf[pack_pad(k * 256 + lane * 4 + u)];
            const bool in32 = v <= (int64_t)INT32_MAX;      // v >= qmin >= INT32_MIN always
            nbad += (!in32 && i + (uint32_t)u < n) ? 1u : 0u;
            qa[u] = in32 ? (int32_t)v : INT32_MAX;
        }
        const int4 qi = make_int4(qa[0], qa[1], qa[2], qa[3]);
        const float4 qf = make_float4((float)qa[0], (float)qa[1], (float)qa[2], (float)qa[3]);   // exact: q came from a float integer
        const float4 o = make_float4(qf.x * sc.s.x, qf.y * sc.s.y, qf.z * sc.s.z, qf.w * sc.s.w);   // custom_layers.py:60
        float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (pr) {
            p = make_float4((qf.x + 0.5f) * sc.s.x, (qf.y + 0.5f) * sc.s.y, (qf.z + 0.5f) * sc.s.z, (qf.w + 0.5f) * sc.s.w);
            const float4 back = quot4(p, sc);
            if (back.x != qf.x) nbad += restore_fixup(p.x, qf.x, sc.s.x) ? 0u : 1u;
            if (back.y != qf.y) nbad += (restore_fixup(p.y, qf.y, sc.s.y) || i + 1u >= n) ? 0u : 1u;
            if (back.z != qf.z) nbad += (restore_fixup(p.z, qf.z, sc.s.z) || i + 2u >= n) ? 0u : 1u;
            if (back.w != qf.w) nbad += (restore_fixup(p.w, qf.w, sc.s.w) || i + 3u >= n) ? 0u : 1u;
        }
        if (i + 4u <= n) {
            if (out) *reinterpret_cast<float4*>(out + i) = o;
            if (qo) *reinterpret_cast<int4*>(qo + i) = qi;
            if (pr) *reinterpret_cast<float4*>(pr + i) = p;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (i + (uint32_t)u >= n) continue;
                if (out) out[i + u] = f4get(o, u);
                if (qo) qo[i + u] = qa[u];
                if (pr) pr[i + u] = f4get(p, u);
            }
        }
    }
    if (bad) {
        nbad = wave_sum_u32(nbad);
        if (lane == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
    }
}

}  // namespace lq

#endif
