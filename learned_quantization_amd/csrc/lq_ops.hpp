// lq_ops.hpp -- per-operation traits (what one element contributes), consumed by every traversal
#ifndef LQ_OPS_HPP_
#define LQ_OPS_HPP_
#include "lq_math.hpp"

namespace lq {

// ------------------------------------------------------------------------------------------
//  Op traits.  elem() consumes one element (x, dy) of group context c at flat index i, returns
//  the value of the primary dense output (stored, vectorised, by the traversal when kStore)
//  and folds into acc when kReduce.
// ------------------------------------------------------------------------------------------
template <int OP>
struct OpT;

struct OpBase {
    static constexpr bool kStdMerge = true;   // merge is (max, add, add): DPP reduction applies
    static constexpr bool kVec4 = false;      // op provides elem4()
    static constexpr bool kVec4c = false;     // op provides elem4c(): float4 with one context/accumulator per element
    static constexpr bool kDy = false;
    static constexpr bool kStore = false;
    static constexpr bool kReduce = false;
    static constexpr bool kSecond = false;    // the op carries a second f64 sum (see OP_DIFF_BWD_V)
    template <typename A>
    __device__ static __forceinline__ A init() {
        A a;
        a.a = 0u;
        a.b = 0;
        a.c = 0;
        return a;
    }
    template <typename A, typename B>
    __device__ static __forceinline__ void merge(A& x, const B& y) {
        x.a = y.a > x.a ? y.a : x.a;
        x.b += y.b;
        x.c += y.c;
    }
    __device__ static __forceinline__ Ctx ctx_of(const Params& p, float s) {      // context of a scale that is already in a register
        Ctx c;
        c.s = s;
        div_ctx(c);
        c.k0 = 0.f;
        c.k1 = 0.f;
        vote_ctx(c, p.lam);
        return c;
    }
    __device__ static __forceinline__ Ctx ctx(const Params& p, int64_t g) { return ctx_of(p, p.s[g]); }
};

// PERM = true: the variant that can also emit the OIHW companion of an HWIO conv kernel ELEMENT BY ELEMENT -- the fallback
// for the conv kernels lq_conv_tile.hpp does not take (more than 9 taps: a 7x7 stem; co % 4 != 0; exotic descriptors).  The
// companion costs two integer divisions and a 4-byte scattered store per element, so these instantiations provide the
// scalar element path only (kVec4 = false: the traversals still load float4, the op walks its elements).
template <bool PERM>
struct FwdOp : OpBase {
    static constexpr bool kStore = true;
    __device__ static __forceinline__ void side4(const Params& p, int64_t i, const float4& q, const float4& o) {
        if (p.q) {
            store_q(p.q, p.q_dtype, i + 0, q.x);
            store_q(p.q, p.q_dtype, i + 1, q.y);
            store_q(p.q, p.q_dtype, i + 2, q.z);
            store_q(p.q, p.q_dtype, i + 3, q.w);
        }
    }
    __device__ static __noinline__ void scatter1(float* __restrict__ out_perm, uint32_t hw, uint32_t ci, uint32_t co, uint32_t i, float o) {
        const uint32_t t = i / co, oc = i - t * co;
        const uint32_t h = t / ci, c = t - h * ci;
        out_perm[(oc * ci + c) * hw + h] = o;
    }
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t i, float x, float, Acc&) {
        float q, o;
        fq_core(x, c, q, o);
        if (p.q) store_q(p.q, p.q_dtype, i, q);
        if constexpr (PERM) {
            if (p.out_perm) scatter1(p.out_perm, p.perm_hw, p.perm_ci, p.perm_co, (uint32_t)i, o);
        }
        return o;
    }
    static constexpr bool kVec4 = !PERM;
    __device__ static __forceinline__ float4 elem4(const Params& p, const Ctx& c, int64_t i, const float4& x, const float4&, Acc&) {
        float4 q, o;
        fq_core4(x, c, q, o);
        side4(p, i, q, o);
        return o;
    }
    static constexpr bool kVec4c = !PERM;
    __device__ static __forceinline__ float4 elem4c(const Params& p, const Ctx* c, int64_t i, const float4& x, const float4&, Acc*) {
        float4 q, o;
        fq_core4c(x, c, q, o);
        side4(p, i, q, o);
        return o;
    }
};
template <>
struct OpT<OP_FWD> : FwdOp<false> {};
template <>
struct OpT<OP_FWD_PERM> : FwdOp<true> {};

template <>
struct OpT<OP_QONLY> : OpBase {
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t i, float x, float, Acc&) {
        float q, o;
        fq_core(x, c, q, o);
        store_q(p.q, p.q_dtype, i, q);
        return 0.f;
    }
};

template <bool PERM>
struct BwdOp : OpBase {
    static constexpr bool kDy = true;
    static constexpr bool kReduce = true;
    // upstream gradient of an HWIO conv kernel that arrives in OIHW order (MIOpen's weight gradient): gathered here, and
    // handed back in HWIO order as dP (dP == dy, custom_layers.py:118) -- weight-sized tensors, L2-resident
    // out of line: the fallback serves a 7x7 stem or an odd head, its divisions need not sit in every traversal's registers
    __device__ static __noinline__ float gather1(const float* __restrict__ dy_perm, float* __restrict__ dp_out, uint32_t hw, uint32_t ci,
                                                 uint32_t co, uint32_t i) {
        const uint32_t t = i / co, o = i - t * co;
        const uint32_t h = t / ci, c = t - h * ci;
        const float d = dy_perm[(o * ci + c) * hw + h];
        dp_out[i] = d;
        return d;
    }
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t i, float x, float dy, Acc& acc) {
        float q, o;
        fq_core(x, c, q, o);
        if constexpr (PERM) {
            if (p.dy_perm) dy = gather1(p.dy_perm, p.dp_out, p.perm_hw, p.perm_ci, p.perm_co, (uint32_t)i);
        }
        nq_accumulate(q, o, dy, p.lam, p.tmode, acc);
        return 0.f;
    }
    static constexpr bool kVec4 = !PERM;       // PERM: scalar element path only (see FwdOp)
    __device__ static __forceinline__ float4 elem4(const Params& p, const Ctx& c, int64_t, const float4& x, const float4& dy, Acc& acc) {
        float4 q, o;
        fq_core4(x, c, q, o);
        nq_accumulate4(q, o, dy, c, p.lam, p.tmode, acc);
        return o;
    }
    static constexpr bool kVec4c = !PERM;
    __device__ static __forceinline__ float4 elem4c(const Params& p, const Ctx* c, int64_t, const float4& x, const float4& dy, Acc* acc) {
        float4 q, o;
        fq_core4c(x, c, q, o);
        nq_accumulate4c(q, o, dy, c, p.lam, p.tmode, acc);
        return o;
    }
};
template <>
struct OpT<OP_BWD> : BwdOp<false> {};
template <>
struct OpT<OP_BWD_PERM> : BwdOp<true> {};

template <>
struct OpT<OP_FUSED> : OpBase {
    static constexpr bool kDy = true;
    static constexpr bool kStore = true;
    static constexpr bool kReduce = true;
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t, float x, float dy, Acc& acc) {
        float q, o;
        fq_core(x, c, q, o);
        nq_accumulate(q, o, dy, p.lam, p.tmode, acc);
        return o;
    }
    static constexpr bool kVec4 = true;
    __device__ static __forceinline__ float4 elem4(const Params& p, const Ctx& c, int64_t, const float4& x, const float4& dy, Acc& acc) {
        float4 q, o;
        fq_core4(x, c, q, o);
        nq_accumulate4(q, o, dy, c, p.lam, p.tmode, acc);
        return o;
    }
    static constexpr bool kVec4c = true;
    __device__ static __forceinline__ float4 elem4c(const Params& p, const Ctx* c, int64_t, const float4& x, const float4& dy, Acc* acc) {
        float4 q, o;
        fq_core4c(x, c, q, o);
        nq_accumulate4c(q, o, dy, c, p.lam, p.tmode, acc);
        return o;
    }
};

// K5a forward: a = bits(max |P|/s), b = number of elements attaining it.
template <>
struct OpT<OP_MAXBIN_FWD> : OpBase {
    static constexpr bool kReduce = true;
    static constexpr bool kStdMerge = false;
    template <typename A, typename B>
    __device__ static __forceinline__ void merge(A& x, const B& y) {
        if (y.a > x.a) {
            x.a = y.a;
            x.b = y.b;
        } else if (y.a == x.a) {
            x.b += y.b;
        }
    }
    __device__ static __forceinline__ float elem(const Params&, const Ctx& c, int64_t, float x, float, Acc& acc) {
        float t = fabsf(x) / c.s;                       // custom_loss_functions.py:92
        uint32_t tb = __float_as_uint(fabsf(t));        // s > 0 in practice; |.| keeps the bit trick valid if not
        if (tb > acc.a) {
            acc.a = tb;
            acc.b = 1u;
        } else if (tb == acc.a) {
            acc.b += 1u;
        }
        return 0.f;
    }
};

// K5a backward: dP_i = (|P_i|/s == mb) ? sign(P_i) * coef / s : 0, coef = c / (G * ties)
template <>
struct OpT<OP_MAXBIN_BWD> : OpBase {
    static constexpr bool kStore = true;
    __device__ static __forceinline__ Ctx ctx(const Params& p, int64_t g) {
        Ctx c;
        c.s = p.s[g];
        c.r = 0.f;
        c.fast = 0;
        c.lam_hi = 0.f;
        c.sure_ok = 0;
        c.k0 = p.mb[g];
        float up = (p.c_dev ? p.c_dev[0] : 1.0f) * p.c_scale;
        c.k1 = (up / (float)p.G) / (float)p.ties[g];
        return c;
    }
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t i, float x, float, Acc&) {
        float t = fabsf(fabsf(x) / c.s);
        float sgn = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
        const float g = (t == c.k0) ? (c.k1 / c.s) * sgn : 0.f;
        return p.accum ? p.out[i] + g : g;
    }
};

// K5b forward: c = sum |P - P/s|
template <>
struct OpT<OP_DIFF_FWD> : OpBase {
    static constexpr bool kReduce = true;
    __device__ static __forceinline__ float elem(const Params&, const Ctx& c, int64_t, float x, float, Acc& acc) {
        float pq = x / c.s;                             // custom_loss_functions.py:172
        acc.c += (double)fabsf(x - pq);                 // :175
        return 0.f;
    }
};

// K5b backward: gi = sign(u) * c/N ; dP = gi - gi/s ; ds[g] = sum gi * (P/s) / s
template <>
struct OpT<OP_DIFF_BWD> : OpBase {
    static constexpr bool kStore = true;
    static constexpr bool kReduce = true;
    __device__ static __forceinline__ Ctx ctx(const Params& p, int64_t g) {
        Ctx c;
        c.s = p.s[g];
        c.r = 0.f;
        c.fast = 0;
        c.lam_hi = 0.f;
        c.sure_ok = 0;
        double n = (double)p.outer * (double)p.G * (double)p.inner;
        c.k0 = ((p.c_dev ? p.c_dev[0] : 1.0f) * p.c_scale) / (float)n;
        c.k1 = 0.f;
        return c;
    }
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t i, float x, float, Acc& acc) {
        float pq = x / c.s;
        float u = x - pq;
        float sgn = (u > 0.f) ? 1.f : ((u < 0.f) ? -1.f : 0.f);
        float gi = sgn * c.k0;
        acc.c += (double)((gi * pq) / c.s);
        const float g = gi - gi / c.s;
        return p.accum ? p.out[i] + g : g;
    }
};

// K5b backward + value: the OP_DIFF_BWD arithmetic, untouched (same acc.c, same stores: dP and ds are its bits), and next to it
// sum |u| = sum |P - P/s| of OP_DIFF_FWD for the VALUE of the term -- u is already in a register, so the value costs no second
// read of the tensor.  The second sum is an f64 like the first; while a thread accumulates, its bits live in the (a, b) pair of
// the accumulator, which this op does not use otherwise (64 bits, the registers of one double).  Before the traversal reduces,
// take_second() moves it into the c of a SECOND accumulator of the same type and clears (a, b): both go through the same
// standard merge one after the other, the first exactly as OP_DIFF_BWD's, the second into a second slice of partials.
template <>
struct OpT<OP_DIFF_BWD_V> : OpT<OP_DIFF_BWD> {
    static constexpr bool kSecond = true;
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t i, float x, float, Acc& acc) {
        float pq = x / c.s;
        float u = x - pq;
        float sgn = (u > 0.f) ? 1.f : ((u < 0.f) ? -1.f : 0.f);
        float gi = sgn * c.k0;
        acc.c += (double)((gi * pq) / c.s);
        const double v = __hiloint2double((int)acc.b, (int)acc.a) + (double)fabsf(u);      // custom_loss_functions.py:175
        acc.a = (uint32_t)__double2loint(v);
        acc.b = (uint32_t)__double2hiint(v);
        const float g = gi - gi / c.s;
        return p.accum ? p.out[i] + g : g;
    }
    __device__ static __forceinline__ Acc take_second(Acc& acc) {
        Acc s;
        s.a = 0u;
        s.b = 0u;
        s.c = __hiloint2double((int)acc.b, (int)acc.a);
        acc.a = 0u;
        acc.b = 0u;
        return s;
    }
};

// Straight-through scale gradient (lq_hip.h: lq_fq_scale_grad_ste): with floor' == 1, d out / d s = floor(P/s) - P/s, so
//   t = P / s (K1's fp32 quotient, bit for bit)   r = floorf(t) - t (ONE fp32 subtraction, in [-1, 0])   acc.c += dy * r
// product and sum in f64; the factor k (Params::c_scale) is applied once per group by FinT::emit.  |t| >= 2^23 gives r == 0
// exactly; a NaN or +-Inf quotient gives a NaN term.  The terms have no common quantum: unlike the vote sums of OP_BWD at
// lambda < 4e-4 the f64 sum depends on the traversal's order (below 2^-50 relative), so different traversals of one tensor may
// differ in the last bit of ds -- every one of them is run-to-run bit-stable.
template <>
struct OpT<OP_STE_SCALE> : OpBase {
    static constexpr bool kDy = true;
    static constexpr bool kReduce = true;
    __device__ static __forceinline__ Ctx ctx(const Params& p, int64_t g) {
        Ctx c;
        c.s = p.s[g];
        div_ctx(c);
        c.k0 = 0.f;
        c.k1 = 0.f;
        c.lam_hi = 0.f;
        c.sure_ok = 0;
        return c;
    }
    __device__ static __forceinline__ void term(float t, float dy, Acc& acc) {
        const float r = floorf(t) - t;
        acc.c += (double)dy * (double)r;
    }
    __device__ static __forceinline__ float elem(const Params&, const Ctx& c, int64_t, float x, float dy, Acc& acc) {
        term(div_by_uniform(x, c), dy, acc);
        return 0.f;
    }
    static constexpr bool kVec4 = true;
    __device__ static __forceinline__ float4 elem4(const Params&, const Ctx& c, int64_t, const float4& x, const float4& dy, Acc& acc) {
        const float4 t = fq_quot4(x, c);
        term(t.x, dy.x, acc);
        term(t.y, dy.y, acc);
        term(t.z, dy.z, acc);
        term(t.w, dy.w, acc);
        return t;
    }
    static constexpr bool kVec4c = true;
    __device__ static __forceinline__ float4 elem4c(const Params&, const Ctx* c, int64_t, const float4& x, const float4& dy, Acc* acc) {
        const float4 t = fq_quot4c(x, c);
        term(t.x, dy.x, acc[0]);
        term(t.y, dy.y, acc[1]);
        term(t.z, dy.z, acc[2]);
        term(t.w, dy.w, acc[3]);
        return t;
    }
};

// Clipped b-bit fake-quant (lq_hip.h: lq_fq_forward_clip / lq_fq_backward_clip).  lo = (float)qmin and hi = (float)qmax travel in
// Ctx::k0 / k1 (Params::clip_lo / clip_hi).  The quotient is K1's (div_by_uniform, fq_quot4, fq_quot4c); the clamp is two
// comparisons and two selects, not fmin / fmax: a NaN floor stays NaN, +-Inf saturates.
// RNE (compile time, never a runtime flag) picks the rounding of the quotient: false = floorf (OP_CLIP_FWD / OP_CLIP_BWD), true =
// rintf, round half to even (OP_CLIP_FWD_RNE / OP_CLIP_BWD_RNE: lq_fq_forward_clip_r / lq_fq_backward_clip_r with
// LQ_ROUND_NEAREST_EVEN).  Either is one instruction (v_floor_f32 / v_rndne_f32); |t| >= 2^23 comes back unchanged from both.
template <bool RNE>
struct ClipBase : OpBase {
    __device__ static __forceinline__ float rnd(float t) {
        if constexpr (RNE) return rintf(t);
        else return floorf(t);
    }
    __device__ static __forceinline__ Ctx ctx(const Params& p, int64_t g) {
        Ctx c;
        c.s = p.s[g];
        div_ctx(c);
        c.k0 = p.clip_lo;
        c.k1 = p.clip_hi;
        c.lam_hi = 0.f;
        c.sure_ok = 0;
        return c;
    }
    __device__ static __forceinline__ float clampq(float q0, float lo, float hi) { return q0 < lo ? lo : (q0 > hi ? hi : q0); }
};

template <bool RNE>
struct ClipFwdOp : ClipBase<RNE> {
    using ClipBase<RNE>::rnd;
    using ClipBase<RNE>::clampq;
    static constexpr bool kStore = true;
    __device__ static __forceinline__ void side4(const Params& p, int64_t i, const float4& q) {      // one test per float4, as FwdOp
        if (p.q) {
            store_q(p.q, p.q_dtype, i + 0, q.x);
            store_q(p.q, p.q_dtype, i + 1, q.y);
            store_q(p.q, p.q_dtype, i + 2, q.z);
            store_q(p.q, p.q_dtype, i + 3, q.w);
        }
    }
    __device__ static __forceinline__ float elem(const Params& p, const Ctx& c, int64_t i, float x, float, Acc&) {
        const float q = clampq(rnd(div_by_uniform(x, c)), c.k0, c.k1);
        if (p.q) store_q(p.q, p.q_dtype, i, q);
        return q * c.s;
    }
    static constexpr bool kVec4 = true;
    __device__ static __forceinline__ float4 elem4(const Params& p, const Ctx& c, int64_t i, const float4& x, const float4&, Acc&) {
        const float4 t = fq_quot4(x, c);
        float4 q, o;
        q.x = clampq(rnd(t.x), c.k0, c.k1); q.y = clampq(rnd(t.y), c.k0, c.k1);
        q.z = clampq(rnd(t.z), c.k0, c.k1); q.w = clampq(rnd(t.w), c.k0, c.k1);
        o.x = q.x * c.s; o.y = q.y * c.s; o.z = q.z * c.s; o.w = q.w * c.s;
        side4(p, i, q);
        return o;
    }
    static constexpr bool kVec4c = true;
    __device__ static __forceinline__ float4 elem4c(const Params& p, const Ctx* c, int64_t i, const float4& x, const float4&, Acc*) {
        const float4 t = fq_quot4c(x, c);
        float4 q, o;
        q.x = clampq(rnd(t.x), c[0].k0, c[0].k1); q.y = clampq(rnd(t.y), c[1].k0, c[1].k1);
        q.z = clampq(rnd(t.z), c[2].k0, c[2].k1); q.w = clampq(rnd(t.w), c[3].k0, c[3].k1);
        o.x = q.x * c[0].s; o.y = q.y * c[1].s; o.z = q.z * c[2].s; o.w = q.w * c[3].s;
        side4(p, i, q);
        return o;
    }
};
template <>
struct OpT<OP_CLIP_FWD> : ClipFwdOp<false> {};
template <>
struct OpT<OP_CLIP_FWD_RNE> : ClipFwdOp<true> {};

// Backward: the value returned (stored by the traversal in the primary dense output) is dP.  acc.c carries sum dy * r in f64
// from the first addition (r = rnd(t) - t inside the range, ONE fp32 subtraction as OP_STE_SCALE, in [-1, 0] for floor and in
// [-1/2, 1/2] for nearest; the bound lo or hi outside; NaN for a NaN q0), acc.b the number of elements outside the range (a NaN
// q0 counts); the standard merge adds both.  The factor k (Params::c_scale) is applied once per group by FinT::emit.  As for OP_STE_SCALE the terms have no
// common quantum: different traversals may differ in the last bit of ds, each one is run-to-run bit-stable.
template <bool RNE>
struct ClipBwdOp : ClipBase<RNE> {
    using ClipBase<RNE>::rnd;
    using ClipBase<RNE>::clampq;
    static constexpr bool kDy = true;
    static constexpr bool kStore = true;
    static constexpr bool kReduce = true;
    __device__ static __forceinline__ float one(float t, float dy, float lo, float hi, Acc& acc) {
        const float q0 = rnd(t);
        const bool inside = (q0 >= lo) & (q0 <= hi);           // false for NaN
        const float r = inside ? q0 - t : clampq(q0, lo, hi);
        acc.c += (double)dy * (double)r;
        acc.b += inside ? 0u : 1u;
        return inside ? dy : 0.f;
    }
    __device__ static __forceinline__ float elem(const Params&, const Ctx& c, int64_t, float x, float dy, Acc& acc) {
        return one(div_by_uniform(x, c), dy, c.k0, c.k1, acc);
    }
    static constexpr bool kVec4 = true;
    __device__ static __forceinline__ float4 elem4(const Params&, const Ctx& c, int64_t, const float4& x, const float4& dy, Acc& acc) {
        const float4 t = fq_quot4(x, c);
        float4 o;
        o.x = one(t.x, dy.x, c.k0, c.k1, acc);
        o.y = one(t.y, dy.y, c.k0, c.k1, acc);
        o.z = one(t.z, dy.z, c.k0, c.k1, acc);
        o.w = one(t.w, dy.w, c.k0, c.k1, acc);
        return o;
    }
    static constexpr bool kVec4c = true;
    __device__ static __forceinline__ float4 elem4c(const Params&, const Ctx* c, int64_t, const float4& x, const float4& dy, Acc* acc) {
        const float4 t = fq_quot4c(x, c);
        float4 o;
        o.x = one(t.x, dy.x, c[0].k0, c[0].k1, acc[0]);
        o.y = one(t.y, dy.y, c[1].k0, c[1].k1, acc[1]);
        o.z = one(t.z, dy.z, c[2].k0, c[2].k1, acc[2]);
        o.w = one(t.w, dy.w, c[3].k0, c[3].k1, acc[3]);
        return o;
    }
};
template <>
struct OpT<OP_CLIP_BWD> : ClipBwdOp<false> {};
template <>
struct OpT<OP_CLIP_BWD_RNE> : ClipBwdOp<true> {};

}  // namespace lq

#endif
