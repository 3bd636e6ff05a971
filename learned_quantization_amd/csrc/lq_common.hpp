// lq_common.hpp -- constants, kernel parameter block, accumulator types (overview: lq_kernels.hip)
#ifndef LQ_COMMON_HPP_
#define LQ_COMMON_HPP_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lq_hip.h"
#include "lq_fastdiv.hpp"

namespace lq {

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr float kEpsF32 = 1.1920928955078125e-07f;   // np.finfo(np.float32).eps, custom_layers.py:11
constexpr int64_t kPeriodic4Min = 4ll << 20;         // column mode, C <= 64: elements from which the float4 grid-stride variant is used
                                                     // (the same 4 M boundary as the 512-thread streaming units: below it single-tensor
                                                     // and batched launches share one geometry and give bit-identical results)
constexpr int64_t kNtBytes = 64ll << 20;             // tensors at least this large are streamed with nontemporal accesses
// Cache policy of the two streaming kernels of one tensor, the forward K1 (k_flat_fwd) and the scale gradient K2 (k_row_stream,
// kMallWalk) -- DESIGN.md section 3, "Infinity Cache reuse" and "Cache-policy mix".  Both stream fastest with PART of their P
// loads under the default policy and the rest `nt`, and with that part interleaved through the tensor, not in one piece: on
// math-free kernels of the same shapes 3/8 of K1's blocks in runs of 16 take 2.6 us off its 45.7, a quarter of K2's units 0.5 us
// off its 44.5 (profiles/policy_mix/membench_mix.txt).  A mix word holds an 8-bit mask for P (bits 0-7), one for dy (bits 8-15,
// K2 only) and the log2 of a run length (bits 16-20): unit u is picked when bit (u >> log2run) & 7 of its stream's mask is set.
// The constants are the pair with the shortest K1, K2, K3 step in tools/sweep_policy.py (profiles/policy_mix/sweep.jsonl).
constexpr uint32_t mix_word(uint32_t mask_p, uint32_t mask_dy, uint32_t log2run) { return mask_p | (mask_dy << 8) | (log2run << 16); }
constexpr uint32_t kMixK1 = mix_word(0x15, 0x00, 4);      // K1 blocks of 512 float4: 3 of every 8 runs of 16 blocks
constexpr uint32_t kMixK2 = mix_word(0x11, 0x00, 0);      // K2 units of 4096 elements: every 4th unit's P; dy stays nt
// Before the mix, K1 loaded the LAST kMallKeepBytes of P with the default policy (44 MiB) and K2, which walks its units backwards
// and so meets those lines first, did the same: a line `d` bytes before the end of P sees about 4 d bytes of other traffic between
// its two uses and can survive in the 256 MiB Infinity Cache for d <= 64 MiB.  With the mix in place the same sweep finds no point
// with such a tail ahead of the ones without: the hits were never measurably faster than HBM (membench_survive.txt), the tail
// acted as one more, coarser, mix.  The tail stays as a development knob (LQ_TUNE_MALL_T, lq_dev_set_flags 0xf00); shipped: none.
constexpr int64_t kMallKeepBytes = 0;

// ------------------------------------------------------------------------------------------
//  Parameters shared by every kernel (passed by value in the kernarg segment).
// ------------------------------------------------------------------------------------------
struct Params {
    const float* P;
    const float* s;
    const float* dy;
    float* out;          // primary dense output (out for K1/K4, dP for penalty backward)
    void* q;             // optional integer view
    int q_dtype;
    float lam;
    int tmode;           // 0: lambda < 4e-4 (tanh(d) == d), 1: lambda <= 0.25 (polynomial), 2: general (ocml tanhf)
    float clip_lo;       // OP_CLIP_* (floor and nearest pair): (float)qmin (this word and clip_hi below sit where alignment padding was: no
                         // other field moves and the struct keeps its size, so the other kernels' argument offsets stay)
    const float* mb;     // per-group max(|P|/s)      (maxbin backward)
    const uint32_t* ties;
    const float* c_dev;  // upstream gradient, device scalar
    float c_scale;
    int accum;           // penalty backward: add to the existing contents of `out` instead of overwriting
    uint32_t* pa;        // partials, SoA
    uint32_t* pb;
    double* pc;          // vote sums are carried in f64 (exact for lambda < 4e-4, see Acc below)
    int64_t outer, G, inner;
    // direct emit (scale-gradient ops whose groups have exactly one partial: biases, row-wise Dense, one row per group):
    // the traversal writes the op's outputs itself and the finalize launch is skipped
    int direct;
    float clip_hi;       // OP_CLIP_*: (float)qmax
    float* e0;           // ds[G]
    float* e1;           // optional parts[3*G]
    double ecount;       // elements per group
    // conv kernels: the parameter is HWIO (custom_layers.py:321), MIOpen consumes OIHW.  Element i = (h*ci + c)*co + o of the
    // HWIO tensor (h = kh*KW + kw) is element (o*ci + c)*hw + h of the OIHW one.  K1 can emit the OIHW tensor next to
    // `out`; K2 can take the upstream gradient in OIHW order and write dP (= dy, custom_layers.py:118) back in HWIO order.
    float* out_perm;       // K1: second output in OIHW order, or NULL
    const float* dy_perm;  // K2: upstream gradient in OIHW order (then `dy` is only a valid dummy), or NULL
    float* dp_out;         // K2: dP in HWIO order, written when dy_perm is set
    uint32_t perm_hw, perm_ci, perm_co;
};

static_assert(sizeof(Params) == 208, "Params: clip_lo / clip_hi must stay inside the former padding");

__device__ __forceinline__ uint32_t perm_index(const Params& p, int64_t i) {      // conv kernels are far below 2^32 elements
    const uint32_t iu = (uint32_t)i;
    const uint32_t t = iu / p.perm_co, o = iu - t * p.perm_co;
    const uint32_t h = t / p.perm_ci, c = t - h * p.perm_ci;
    return (o * p.perm_ci + c) * p.perm_hw + h;
}

struct FlatIdx {          // group of flat element i: (i / inner) % G
    FastDiv inner, G;
    uint32_t keep_from;   // k_flat_fwd, streaming forward of long aligned rows: first block that loads P with the default cache policy
    uint32_t keep_mix;    // ... and the mix word of the blocks before it (kMixK1; 0: none).  It sits where the kernel arguments had
                          // padding: no argument of any k_flat_fwd moves
};
static_assert(sizeof(FlatIdx) == 40, "FlatIdx: keep_mix must stay inside the former padding before nv");

// Per-group context, loaded once per row / column.
struct Ctx {
    float s;
    float r;      // RN(1/s)
    int fast;     // s is inside the window where the uniform-divisor division is exact
    float k0;
    float k1;
    float lam_hi; // RN(lambda * 1.000001): a >= lam_hi*b  =>  RN(a/b) >= lambda for sure
    int sure_ok;  // lam_hi*b cannot underflow for any b this row can produce (b >= min(s, eps_f32))
};

// Narrow accumulator (inside the traversal kernels) and wide accumulator (finalize).
//
// The sum `c` is carried in f64 from the first addition on.  For the nested-quantization vote (custom_layers.py:84 / :110) with
// lambda < 4e-4 -- every published threshold; there |tanh(d)| == d in fp32 -- this makes the sum EXACT and therefore independent
// of the order in which a traversal visits the elements: with lambda in [2^e, 2^(e+1)) every term d = RN(lambda - ratio),
// 0 <= ratio < lambda, is a multiple of 2^(e-24) (Sterbenz for ratio >= lambda/2; one rounding at ulp(lambda/2) below) and
// at most lambda, i.e. an integer below 2^25 in units of 2^(e-24); a group of up to 2^28 elements sums to less than 2^53 units.
// Every traversal (row stream, tiles, columns, multi-tensor batch, conv tiles, any block size, any number of ranks' partials
// merged in any order) therefore yields the SAME bits of ds -- and that value is the correctly rounded mean.  For lambda >= 4e-4
// the terms are polynomial / ocml tanh values without a common quantum: there the f64 sum still depends on the order, below
// 2^-50 relative, which survives the final rounding to fp32 only when the mean sits on a rounding boundary.
template <typename TB, typename TC>
struct AccT {
    uint32_t a;
    TB b;
    TC c;
};
using Acc = AccT<uint32_t, double>;
using AccW = AccT<double, double>;   // finalize: count in f64 as well (counts are exact below 2^53)

enum OpKind {
    OP_FWD = 0,        // K1
    OP_BWD = 1,        // K2
    OP_FUSED = 2,      // K4
    OP_MAXBIN_FWD = 3, // K5a
    OP_MAXBIN_BWD = 4,
    OP_DIFF_FWD = 5,   // K5b
    OP_DIFF_BWD = 6,
    OP_QONLY = 7,      // integer view only (callbacks / export)
    OP_FWD_PERM = 8,   // K1 that can also emit the OIHW companion of an HWIO conv kernel
    OP_BWD_PERM = 9,   // K2 that can take dy in OIHW order and write dP in HWIO order
    OP_DIFF_BWD_V = 10, // K5b backward that also carries sum |P - P/s| (the term's VALUE) in a second accumulator
    OP_STE_SCALE = 11,  // straight-through scale gradient: ds[g] = k * sum dy * (floor(P/s) - P/s)
    OP_CLIP_FWD = 12,   // clipped forward: out = clamp(floor(P/s), qmin, qmax) * s
    OP_CLIP_BWD = 13,   // clipped backward: dP = inside ? dy : 0, ds[g] = k * sum dy * r, clipped[g] = #{!inside}
    OP_CLIP_FWD_RNE = 14,   // OP_CLIP_FWD with rintf (round half to even) in place of floorf, a compile-time parameter of the trait
    OP_CLIP_BWD_RNE = 15,   // OP_CLIP_BWD with rintf: r = rint(t) - t in [-1/2, 1/2]
};

}  // namespace lq

#endif
