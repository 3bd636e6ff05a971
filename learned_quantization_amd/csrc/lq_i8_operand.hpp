// lq_i8_operand.hpp -- packed int8 operands in the order the int8 matrix instruction consumes them
// (lq_hip.h: lq_i8_operand_bytes / lq_i8_operand_pack / lq_i8_operand_quantize / lq_i8_operand_decode)
//
// An operand is a matrix of L lines by K reduction elements: one int8 code per element and fp32 scales, one per line and per SCALE
// BLOCK of `block` consecutive k (block == 0: one scale per line; otherwise block % 64 == 0, nbs = ceil(K / block), the last block
// may be short).  The codes are cut into tiles of 16 lines by 64 k, the A (or B) operand of one v_mfma_i32_16x16x64_i8:
//
//   codes   [LT][KT][64 lanes][16 bytes]      LT = ceil(L / 16), KT = ceil(K / 64)
//           fragment `lane` of tile (lt, kt) holds line 16 lt + (lane & 15) and, with g = lane >> 4, k = 64 kt + 16 g + j in byte j
//           (j = 0 .. 15): read as four little-endian dwords these are the lane's operand registers, one 16-byte load
//   scales  [nbs][16 LT] fp32                 scale of (block, line) at [block][line]: the 16 lines of a tile are contiguous
//
// Lines past L and k past K hold code 0; the scales of lines past L are 1.0f.  The GEMM loads whole tiles without a bounds check.
// What the device pins about the lane map (tests/test_gpu_i8.py, the one-hot sweep over k = 0 .. 127): lane l supplies line l & 15
// of A and of B, A's lines are the rows and B's the columns of the result, and the two operands take the SAME k from the same
// (lane >> 4, byte): a product of two operands packed by one rule is exact for every k.  The instruction sums all 64 k of a step
// into one int32, so WHICH k a (lane >> 4, byte) pair is called is not observable: any permutation of k inside a step, applied to
// both operands, gives the same sums (unlike the block-scaled instruction, whose scales apply per k and forced fp8's two half
// blocks 64 k apart).  The rule above, 16 consecutive k per lane, is therefore the definition, and a scale block is a whole number
// of steps so that no permutation inside a step could move an element to another scale.
//
// pack: one thread per (line, 16 k): the element step is lq_group.hpp's GroupStep<RNE, GroupParams> -- ctx, quant, view, the step of
// lq_fq_forward_group, not a restatement -- and the byte is the LQ_Q_I8 integer view's (store_q_scalar).  quantize: a team of
// 2^log_team lanes per (row, scale block), the lanes side by side along the row (a wave reads whole contiguous runs), the absmax
// partials of lq_scale_init.hpp (init_take / init_merge / init_raw / init_final) merged by an xor butterfly inside the team.  The
// team keeps the first kI8Cache accesses per lane in registers between the two passes: a scale block (or, with block == 0, a row)
// of up to kI8Cache * 64 * V elements (V = 4 with 16-byte loads: 4096; V = 1: 1024) is read from memory once; what lies beyond is
// read a second time, from the cache hierarchy.
#ifndef LQ_I8_OPERAND_HPP_
#define LQ_I8_OPERAND_HPP_
#include "lq_group.hpp"
#include "lq_scale_init.hpp"

namespace lq {

constexpr int kI8TileLines = 16;      // lines of an operand tile
constexpr int kI8TileK = 64;          // k of an operand tile: one instruction
constexpr int kI8Cache = 16;          // quantize: accesses per lane held in registers between the scale and the codes

// byte offset of the code of element k of line ln; 16 consecutive k from a multiple of 16 are 16 consecutive bytes
__host__ __device__ __forceinline__ int64_t i8_code_offset(int32_t KT, int32_t ln, int32_t k) {
    const int64_t tile = (int64_t)(ln >> 4) * KT + (k >> 6);
    return (tile * 64 + (((k & 63) >> 4) << 4) + (ln & 15)) * 16 + (k & 15);
}

// the LQ_Q_I8 integer view of a clamped grid value, as a byte
__device__ __forceinline__ uint32_t i8_view_byte(float q) {
    int8_t b;
    store_q_scalar<LQ_Q_I8>(&b, 0, q);
    return (uint32_t)(uint8_t)b;
}

struct I8PackParams {
    GroupParams g;            // P, s, lo, hi; the geometry fields are not read
    uint8_t* codes;
    float* scales;
    int64_t line_stride, k_stride;        // of P, in elements
    int64_t s_line_stride, s_blk_stride;  // of s, in elements
    int32_t L, K, block;      // block == 0: one scale per line
    int32_t LT, KT;
};

// with an offset per group (lq_i8_operand_pack_affine): b in the layout of s, offsets in the layout of scales
struct I8PackAffineParams : I8PackParams {
    const float* b;
    float* offsets;
};

// LINE_FAST: neighbouring threads hold neighbouring lines (the parameter's contiguous axis under axis 0), else neighbouring k runs.
// AFF: the element step of lq_fq_forward_group_affine, u = P - b before the quotient, and the offset of a scale block carried
// across like its scale; lines past L get offset +0.
template <bool RNE, bool LINE_FAST, bool AFF = false>
__global__ __launch_bounds__(kBlock) void k_i8_pack(const std::conditional_t<AFF, I8PackAffineParams, I8PackParams> op) {
    using Step = GroupStep<RNE, GroupParams>;
    const int64_t lines = (int64_t)op.LT * kI8TileLines, runs = (int64_t)op.KT * 4;
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tid >= lines * runs) return;
    const int32_t ln = (int32_t)(LINE_FAST ? tid % lines : tid / runs);
    const int32_t k0 = (int32_t)(LINE_FAST ? tid / lines : tid % runs) * 16;
    const int32_t blk = op.block ? k0 / op.block : 0;
    const bool live = ln < op.L && k0 < op.K;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    float s = 1.0f;
    if (live) s = op.g.s[(int64_t)ln * op.s_line_stride + (int64_t)blk * op.s_blk_stride];
    [[maybe_unused]] float b = 0.f;
    if constexpr (AFF) {
        if (live) b = op.b[(int64_t)ln * op.s_line_stride + (int64_t)blk * op.s_blk_stride];
    }
    if (live) {
        const Ctx c = Step::ctx(op.g, s);
        const int n = min(16, op.K - k0);
        const float* src = op.g.P + (int64_t)ln * op.line_stride + (int64_t)k0 * op.k_stride;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < n) {
                float u = src[(int64_t)j * op.k_stride];
                if constexpr (AFF) u = u - b;
                const float q = Step::quant(op.g, c, div_by_uniform(u, c));
                w[j >> 2] |= i8_view_byte(Step::view(op.g, q)) << (8 * (j & 3));
            }
        }
    }
    *reinterpret_cast<uint4*>(op.codes + i8_code_offset(op.KT, ln, k0)) = make_uint4(w[0], w[1], w[2], w[3]);
    // the first run of a scale block carries its scale across, bit for bit
    if (k0 < op.K && (op.block ? k0 % op.block == 0 : k0 == 0)) {
        op.scales[(int64_t)blk * lines + ln] = s;
        if constexpr (AFF) op.offsets[(int64_t)blk * lines + ln] = b;
    }
}

struct I8QuantParams {
    GroupParams g;            // P = X, lo = -127, hi = 127; nothing else is read
    InitParams ip;            // lo, hi, min_value
    uint8_t* codes;
    float* scales;
    int32_t M, K, block;      // block == 0: one scale per row
    int32_t nbs, LT, KT;
};

// V = 4: K % 4 == 0 and X 16-byte aligned.  A team of T = 1 << log_team lanes owns (row, scale block) `pair`; T * V covers the scale
// block where it is at most 64 V long, so that a wave's teams read one contiguous run of the row per access.
template <int V>
__global__ __launch_bounds__(kBlock) void k_i8_quantize(const I8QuantParams op, const int log_team) {
    using Step = GroupStep<true, GroupParams>;
    const int T = 1 << log_team;
    const int lt = (int)threadIdx.x & (T - 1);
    const int64_t lines = (int64_t)op.LT * kI8TileLines;
    const int64_t pairs = lines * op.nbs;
    const int64_t pair = (int64_t)blockIdx.x * (kBlock >> log_team) + (threadIdx.x >> log_team);
    if (pair >= pairs) return;                // team-uniform, and a team lies inside one wave: the shuffles below stay inside it
    const int32_t row = (int32_t)(pair / op.nbs), blk = (int32_t)(pair - (int64_t)row * op.nbs);
    const bool live_row = row < op.M;
    const int32_t span = op.block ? op.block : op.K;
    const int32_t c0 = blk * span;                                        // < K: nbs = ceil(K / block)
    const int32_t c1 = live_row ? min(c0 + span, op.K) : c0;              // elements read
    const int32_t c1s = blk == op.nbs - 1 ? op.KT * kI8TileK : c0 + span; // codes written: the last block writes the padding of k
    const float* src = op.g.P + (int64_t)row * op.K;
    const int32_t step = T * V;

    float x[kI8Cache][V];
    InitAcc a = InitAcc{0.f, 0.f, 0.0, 0u};
#pragma unroll
    for (int it = 0; it < kI8Cache; ++it) {
        const int32_t col = c0 + it * step + lt * V;
#pragma unroll
        for (int v = 0; v < V; ++v) x[it][v] = 0.f;
        if (c0 + it * step >= c1) continue;   // team-uniform
        if (col < c1) {                       // V = 4: K % 4 == 0 and block % 64 == 0: the lane's four are inside together
            if constexpr (V == 4) {
                const float4 t = *reinterpret_cast<const float4*>(src + col);
                x[it][0] = t.x; x[it][1] = t.y; x[it][2] = t.z; x[it][3] = t.w;
            } else {
                x[it][0] = src[col];
            }
#pragma unroll
            for (int v = 0; v < V; ++v) init_take<LQ_INIT_ABSMAX>(x[it][v], a);
        }
    }
    for (int32_t col = c0 + kI8Cache * step + lt * V; col < c1; col += step) {      // what the registers do not hold
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(src + col);
            init_take<LQ_INIT_ABSMAX>(t.x, a);
            init_take<LQ_INIT_ABSMAX>(t.y, a);
            init_take<LQ_INIT_ABSMAX>(t.z, a);
            init_take<LQ_INIT_ABSMAX>(t.w, a);
        } else {
            init_take<LQ_INIT_ABSMAX>(src[col], a);
        }
    }
    for (int off = T >> 1; off > 0; off >>= 1)      // fixed butterfly inside the aligned team: every lane ends with the total
        init_merge<LQ_INIT_ABSMAX>(a, __shfl_xor(a.f0, off), __shfl_xor(a.f1, off), 0.0, __shfl_xor(a.bad, off));
    const float s = live_row ? init_final(op.ip, init_raw<LQ_INIT_ABSMAX>(op.ip, a, c1 - c0), a.bad) : 1.0f;
    if (lt == 0) op.scales[(int64_t)blk * lines + row] = s;
    const Ctx c = Step::ctx(op.g, s);

    auto emit = [&](int32_t col, const float (&xv)[V]) {      // col < c1s; elements at or past c1 are padding: code 0
        uint32_t w = 0u;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (col + v < c1) {
                const float q = Step::quant(op.g, c, div_by_uniform(xv[v], c));
                w |= i8_view_byte(Step::view(op.g, q)) << (8 * v);
            }
        }
        uint8_t* dst = op.codes + i8_code_offset(op.KT, row, col);
        if constexpr (V == 4) *reinterpret_cast<uint32_t*>(dst) = w;
        else *dst = (uint8_t)w;
    };
#pragma unroll
    for (int it = 0; it < kI8Cache; ++it) {
        const int32_t col = c0 + it * step + lt * V;
        if (c0 + it * step >= c1s) continue;  // team-uniform
        if (col < c1s) emit(col, x[it]);
    }
    for (int32_t col = c0 + kI8Cache * step + lt * V; col < c1s; col += step) {
        float xv[V];
#pragma unroll
        for (int v = 0; v < V; ++v) xv[v] = col + v < c1 ? src[col + v] : 0.f;
        emit(col, xv);
    }
}

struct I8DecodeParams {
    const uint8_t* codes;
    const float* scales;
    float* out;
    int32_t L, K, block, LT, KT;
};

struct I8DecodeAffineParams {
    I8DecodeParams d;
    const float* offsets;     // the layout of scales
};

__global__ __launch_bounds__(kBlock) void k_i8_decode(const I8DecodeParams dp) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)dp.L * dp.K) return;
    const int32_t ln = (int32_t)(i / dp.K), k = (int32_t)(i % dp.K);
    const int32_t blk = dp.block ? k / dp.block : 0;
    const float code = (float)(int8_t)dp.codes[i8_code_offset(dp.KT, ln, k)];
    dp.out[i] = code * dp.scales[(int64_t)blk * dp.LT * kI8TileLines + ln];
}

// out = RN(RN(code * scale) + offset): the two roundings of lq_fq_forward_group_affine's out
__global__ __launch_bounds__(kBlock) void k_i8_decode_affine(const I8DecodeAffineParams ap) {
    const I8DecodeParams& dp = ap.d;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)dp.L * dp.K) return;
    const int32_t ln = (int32_t)(i / dp.K), k = (int32_t)(i % dp.K);
    const int32_t blk = dp.block ? k / dp.block : 0;
    const float code = (float)(int8_t)dp.codes[i8_code_offset(dp.KT, ln, k)];
    const int64_t si = (int64_t)blk * dp.LT * kI8TileLines + ln;
    dp.out[i] = __fadd_rn(__fmul_rn(code, dp.scales[si]), ap.offsets[si]);
}

}  // namespace lq

#endif
