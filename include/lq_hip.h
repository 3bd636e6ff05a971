/* lq_hip.h -- C ABI of the MI355X (gfx950) learned-quantization hot path.
 *
 * The reference (anuunchin/learned-quantization) is pure Python on TensorFlow 2.11
 * and has no native interface of its own; the operator surface it exposes for this
 * path is the Python op `my_custom_gradient` and the loss-term methods.  Every entry
 * point below names the reference interface it replaces (file:line relative to
 * /root/reference).  The ctypes binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no framework types; all tensor pointers are DEVICE
 *     pointers to contiguous float32 unless stated otherwise;
 *   - group descriptor (outer, G, inner): element i of a contiguous tensor uses scale
 *     element  g = (i / inner) % G ; numel = outer * G * inner.  It encodes the four
 *     `orientation`s of CustomQuantizedScaleLayer.build
 *     (MNIST/nested_quantization_layer/custom_components/custom_layers.py:147-197);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); kernels are
 *     enqueued and the call returns without synchronising; nothing is allocated;
 *   - `ws` is caller-owned DEVICE scratch of at least lq_workspace_bytes(outer,G,inner)
 *     bytes, 16-byte aligned; it carries deterministic two-stage reduction partials
 *     (no float atomics: results are run-to-run bit-stable);
 *   - memory contract: the contents of `ws` on entry are irrelevant.  No call writes outside the stated extent of its outputs
 *     and of [ws, ws + lq_workspace_bytes), and no byte outside the stated extents of its inputs influences any result;
 *   - return value: LQ_OK (0) or a negative lq_status; lq_last_error() returns a
 *     thread-local message for the last failing call on this thread.
 */
#ifndef LQ_HIP_H_
#define LQ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LQ_ABI_VERSION 3

typedef enum lq_status {
    LQ_OK = 0,
    LQ_EINVAL = -1,      /* bad argument (null pointer, non-positive extent, bad enum) */
    LQ_EHIP = -2,        /* a HIP runtime call / kernel launch failed                  */
    LQ_EWORKSPACE = -3,  /* workspace missing or too small                             */
    LQ_EALIGN = -4       /* pointer not 4-byte aligned / workspace not 16-byte aligned */
} lq_status;

typedef enum lq_qdtype {
    LQ_Q_NONE = 0,
    LQ_Q_F32 = 1,        /* integer-valued float32, exactly the reference's tf.floor output */
    LQ_Q_I32 = 2,        /* saturating float->int32                                          */
    LQ_Q_I8 = 3          /* two's-complement wrap of the integer, = numpy .astype(int8) of
                            CIFAR-10/nested_quantization_layer/utils/log_scripts.py:74-79    */
} lq_qdtype;

typedef enum lq_adam_mode {
    LQ_ADAM_KERAS = 0,   /* Keras 2.11: var -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps) */
    LQ_ADAM_TORCH = 1    /* torch.optim.Adam: m_hat / (sqrt(v_hat) + eps)                      */
} lq_adam_mode;

int lq_version(void);                 /* LQ_ABI_VERSION of the loaded library            */
const char* lq_last_error(void);      /* thread-local, never NULL                        */
const char* lq_status_string(int status);

/* Scratch bytes needed by every reducing entry point for this descriptor. */
size_t lq_workspace_bytes(int64_t outer, int64_t G, int64_t inner);

/* ---- K1: fake-quant forward -------------------------------------------------------
 * Replaces the forward of `my_custom_gradient`
 *   MNIST/nested_quantization_layer/custom_components/custom_layers.py:55-60,120
 *   CIFAR-10/custom_loss_terms/custom_components/custom_layers.py:53-59,64
 * t = P / s (IEEE RN), q = floor(t), out = q * s.  `out` may be NULL when only q is
 * wanted (callbacks/export: custom_callbacks.py:85-87, log_scripts.py:74-79).       */
int lq_fq_forward(const float* P, const float* s, float* out, void* q, int q_dtype,
                  int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- K2+K3: nested-quantization scale gradient ------------------------------------
 * Replaces `custom_grad` of the NQ op, custom_layers.py:62-118:
 *   ratio = |dy| / |where(out==0, eps_f32, out)|            (:63-64)
 *   m_g = max|q| , A_g = all(ratio >= lambda)                (:68-73, :94-99)
 *   mean_g = A_g ? -|tanh(lambda)| : mean(ratio>=lambda ? 0 : -|tanh(lambda-ratio)|)  (:77-88,:103-114)
 *   ds[g] = mean_g * m_g                                     (:116)
 * dP is `dy` itself (STE, :118) and is therefore not an output.
 * `parts` (optional, DEVICE float[3*G]) receives m_g, mean_g and the count of elements
 * with ratio < lambda (as float) for diagnostics / tests.                             */
int lq_fq_scale_grad(const float* P, const float* s, const float* dy, float lambda,
                     float* ds, float* parts, void* ws, size_t ws_bytes,
                     int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- straight-through scale gradient (the step-size gradient of LSQ and relatives, for this floor quantizer) ----
 * Fills the slot the reference leaves open: CIFAR-10/paper_implementation returns zeros for the scale (a TODO).  Under
 * the straight-through convention that already gives dP = dy (floor' == 1), d out / d s = floor(P/s) - P/s, in [-1, 0]:
 *   t_i = P_i / s[g]       IEEE fp32 division: K1's quotient, bit for bit
 *   q_i = floorf(t_i)
 *   r_i = q_i - t_i        ONE fp32 subtraction (not always exact: t = -2^-40 gives r = -1)
 *   ds[g] = RN_f32( (double)grad_scale * sum_{i in g} (double)dy_i * (double)r_i )
 * dP is `dy` itself (STE) and is therefore not an output.  The fp32 quotient is part of the definition (what a TensorFlow
 * fp32 graph computes; an f64 quotient moves the sum by ~3e-4 of sum |terms| at the initial scale, |q| ~ 1e4).  The sum is f64
 * from the first addition, two-stage and ordered (no float atomics): run-to-run bit-stable.  NaN / Inf as fp32 arithmetic gives
 * them: a NaN or +-Inf quotient makes that group's ds NaN, other groups are unaffected; |t| >= 2^23 contributes exactly 0.
 * NO bit-identity across traversals: unlike the NQ vote at lambda < 4e-4 the terms have no common quantum, so the single-tensor
 * call, the batch and different descriptors of the same data may differ in the last bits of the f64 sum (~2^-50 relative, visible
 * in fp32 only on a rounding boundary); each is within ~2^-23 * sum |dy_i r_i| of the exact value.
 * Runs the generic traversal bodies at every size (tensors from 4 M elements: correct, slower than K2's streaming forms).  */
int lq_fq_scale_grad_ste(const float* P, const float* s, const float* dy, float grad_scale,
                         float* ds, void* ws, size_t ws_bytes,
                         int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- clipped b-bit fake-quant with LSQ gradients (the integer range is chosen, not an outcome of training) ----
 * Integers qmin <= qmax with -2^24 <= qmin, qmax <= 2^24 (exact in fp32); lo = (float)qmin, hi = (float)qmax.  For element i
 * of group g:
 *   t  = P_i / s[g]                              IEEE fp32 division: K1's quotient, bit for bit
 *   q0 = floorf(t)
 *   q  = q0 < lo ? lo : (q0 > hi ? hi : q0)      comparisons, not fmin/fmax: a NaN q0 stays NaN, +-Inf saturates
 *   out_i = q * s[g]                             one fp32 product, as K1
 *   inside_i = (q0 >= lo) && (q0 <= hi)          false for NaN
 *   dP_i  = inside_i ? dy_i : +0.0f
 *   r_i   = inside_i ? (q0 - t)  [ONE fp32 subtraction, as lq_fq_scale_grad_ste]  :  q   [lo or hi; NaN if q0 is NaN]
 *   ds[g] = RN_f32( (double)grad_scale * sum_{i in g} (double)dy_i * (double)r_i )
 *   clipped[g] = #{ i in g : !inside_i }         exact, uint32 (saturates at 2^32 - 1)
 * Clipped elements pass no gradient to P and pull the scale towards covering them.  The sum is f64 from the first addition,
 * two-stage and ordered (no float atomics): run-to-run bit-stable.  As for lq_fq_scale_grad_ste the terms have no common
 * quantum, so different traversals of the same data need not give bit-identical ds.  With qmin = -2^24, qmax = 2^24 and
 * |t| < 2^24: out has lq_fq_forward's bits, dP == dy, ds is lq_fq_scale_grad_ste's up to the summation order.
 * lq_fq_forward_clip: `out` is required; q / q_dtype optionally give the CLAMPED integers (as lq_fq_forward's integer view).
 * lq_fq_backward_clip: dP is required (same memory order as P); ds == NULL means "mask only" (the loss-term-only rule: the
 * same kernel runs and the sum is dropped when the outputs are written); clipped may be NULL.  ws: lq_workspace_bytes() of the
 * descriptor, required in every case.  A NULL required pointer, qmin > qmax, a bound outside +-2^24, a workspace that is
 * missing or too small and a bad descriptor return LQ_EINVAL before any launch.  Both calls only enqueue (capturable).
 * Run the generic traversal bodies at every size, as lq_fq_scale_grad_ste.  */
int lq_fq_forward_clip(const float* P, const float* s, float* out, void* q, int q_dtype,
                       int32_t qmin, int32_t qmax, int64_t outer, int64_t G, int64_t inner, void* stream);
int lq_fq_backward_clip(const float* P, const float* s, const float* dy, int32_t qmin, int32_t qmax, float grad_scale,
                        float* dP, float* ds /* may be NULL */, uint32_t* clipped /* may be NULL */,
                        void* ws, size_t ws_bytes, int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- the clipped pair with a choice of rounding ----
 * `rounding` replaces the floorf of q0 above: LQ_ROUND_FLOOR runs exactly what lq_fq_forward_clip / lq_fq_backward_clip run (those
 * two forward here); LQ_ROUND_NEAREST_EVEN takes q0 = rintf(t), round half to even (|t| >= 2^23 gives q0 == t).  Everything else in
 * the definition reads the same with that q0: r = q0 - t is then in [-1/2, 1/2]; t = qmax + 1/2 rounds to qmax + 1 when qmax is
 * odd and is clipped, t = qmin - 1/2 rounds to qmin when qmin is even and is inside; P in [-s/2, 0) gives q0 = -0.0, out keeps
 * the sign (-0.0 * s) and the integer outputs store 0.  The nearest pair has kernels of its own (the rounding is a compile-time
 * parameter of the op trait).  Any other `rounding` returns LQ_EINVAL before any launch; every other rule is the floor pair's. */
typedef enum lq_rounding { LQ_ROUND_FLOOR = 0, LQ_ROUND_NEAREST_EVEN = 1 } lq_rounding;
int lq_fq_forward_clip_r(const float* P, const float* s, float* out, void* q, int q_dtype,
                         int32_t qmin, int32_t qmax, int rounding, int64_t outer, int64_t G, int64_t inner, void* stream);
int lq_fq_backward_clip_r(const float* P, const float* s, const float* dy, int32_t qmin, int32_t qmax, int rounding, float grad_scale,
                          float* dP, float* ds /* may be NULL */, uint32_t* clipped /* may be NULL */,
                          void* ws, size_t ws_bytes, int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- group-wise (block) scales of the clipped pair ----
 * The parameter is seen in MEMORY order as a matrix [R][C], C contiguous, R * C < 2^31.  axis = 0: groups run along R (strided: the
 * `in` dimension of a Dense kernel stored (in, out)); axis = 1: groups run along C (contiguous: the (ci, kh, kw) run of one output
 * channel of an OIHW conv kernel).  gs >= 1 is the group size and nb = ceil(len / gs) with len = R for axis 0 and C for axis 1: the
 * last group of a line may be short, gs >= len gives one group per line.  The scale matrix is dense fp32, [nb][C] for axis 0 and
 * [R][nb] for axis 1: element (r, c) uses s[r / gs][c] for axis 0 and s[r][c / gs] for axis 1.
 * Per element and per group the definition is exactly the one of lq_fq_forward_clip_r / lq_fq_backward_clip_r above:
 *   t = P / s (IEEE fp32 division), q0 = floorf(t) or rintf(t) by `rounding`, q = q0 < lo ? lo : (q0 > hi ? hi : q0) (comparisons),
 *   out = q * s; inside = (q0 >= lo) && (q0 <= hi); dP = inside ? dy : +0.0f; r = inside ? q0 - t : q;
 *   ds[g] = RN_f32( (double)grad_scale * sum_{i in g} (double)dy_i * (double)r_i ); clipped[g] = #{ i in g : !inside_i }, exact, uint32.
 * ds and clipped have the scale's shape.  NaN and Inf behave as there and spoil only their own group.  The sums are f64 from the first
 * addition and taken in one fixed order (no float atomics): run-to-run bit-stable; the note "no bit-identity of ds across traversals"
 * carries over (the same data under the per-axis descriptor of lq_fq_backward_clip_r may differ in the last bits of the f64 sum).
 * Any 4-byte aligned base works (16-byte aligned bases with C % 4 == 0 -- and gs % 4 == 0 on axis 1 -- take 16-byte accesses); a
 * worse alignment returns LQ_EALIGN.  Dispatch is a pure function of the arguments; the library reads no environment.
 * lq_group_workspace_bytes: scratch the backward needs for this shape.  Every shipped form emits ds and clipped from the launch
 * that computes them, so it is 0 for every shape and `ws` may be NULL; a caller that sizes `ws` with it stays correct if a
 * two-stage form is added (memory contract as above: the contents of `ws` on entry are irrelevant, no call writes outside the
 * stated extents of its outputs and of [ws, ws + lq_group_workspace_bytes)).
 * lq_fq_forward_group: `out` is required; q / q_dtype optionally give the CLAMPED integers.  lq_fq_backward_group: dP is required;
 * ds == NULL means "mask only", clipped may be NULL.  A NULL required pointer, qmin > qmax, a bound outside +-2^24, a bad `rounding`,
 * axis not in {0, 1}, gs < 1, a non-positive extent and R * C >= 2^31 return LQ_EINVAL before any launch.  Both calls only enqueue
 * (capturable), ONE launch each.  */
size_t lq_group_workspace_bytes(int64_t R, int64_t C, int axis, int64_t gs);
int lq_fq_forward_group(const float* P, const float* s, float* out, void* q, int q_dtype, int32_t qmin, int32_t qmax, int rounding,
                        int64_t R, int64_t C, int axis, int64_t gs, void* stream);
int lq_fq_backward_group(const float* P, const float* s, const float* dy, int32_t qmin, int32_t qmax, int rounding, float grad_scale,
                         float* dP, float* ds /* may be NULL: mask only */, uint32_t* clipped /* may be NULL */,
                         void* ws, size_t ws_bytes, int64_t R, int64_t C, int axis, int64_t gs, void* stream);

/* ---- scale initialisation: the group-wise scales of the clipped pair from the weights themselves ----
 * At the library's initial scale (1.19e-5) a range clips every weight of an ordinary layer: dP is masked to zero and only the scale
 * moves.  This call writes a starting scale per group that covers the weights.  Geometry: lq_fq_forward_group's ([R][C] in memory
 * order, axis, gs clamped to the line length, nb = ceil(len / gs), the last group may be short); s is the OUTPUT, [nb][C] or [R][nb].
 * A 1-D parameter with a scalar scale (a bias) is R = 1, C = numel, axis = 1, gs = numel.
 * n: the element count of a group (its own when short); lo = (float)qmin, hi = (float)qmax.  Every group's result is
 * fmaxf(s_raw, min_value), min_value > 0 and finite.
 *   LQ_INIT_ABSMAX  ap = max(max_i P_i, 0), an = max(max_i -P_i, 0)                                   (exact)
 *                   a  = max(qmax > 0 ? RN_f32(ap / hi) : 0, qmin < 0 ? RN_f32(an / -lo) : 0)         (IEEE fp32 quotients)
 *                   s_raw = RN_f32(a * (1 + 2^-22))
 *                   RN(x/d) >= (x/d)(1 - 2^-24), and two such roundings against the factor 1 + 2^-22 leave s_raw strictly above the
 *                   real quotient: |P_i| / s <= bound in the reals, so the ROUNDED quotient of every element stays inside the range
 *                   for floor and for nearest -- no element on a side with a nonzero bound is clipped.
 *   LQ_INIT_LSQ     qp = qmax > 0 ? qmax : -qmin;  s_raw = RN_f32( 2 * sum_i (double)|P_i| / ((double)n * sqrt((double)qp)) ),
 *                   the LSQ paper's 2 <|w|> / sqrt(Qp); the sum is f64 in one fixed order.  (The range [0, 0] has qp = 0: the
 *                   quotient is then +Inf, or NaN -> min_value for a group of zeros, as IEEE arithmetic gives it.)
 *   LQ_INIT_MSE     s0 = the group's LQ_INIT_ABSMAX s_raw.  Candidates k = 0 .. 27: s_k = fmaxf(RN_f32(s0 * c_k), min_value) with
 *                   c_k = (32 - k) / 32 (exact in fp32, 1 down to 5/32).  E_k = sum_i ((double)P_i - (double)out_i)^2 with out_i the
 *                   fp32 fake-quantised value of the clipped quantizer above under s_k (IEEE P_i / s_k, floorf or rintf by
 *                   `rounding`, clamp by comparisons, one fp32 product); d * d and the addition round separately, the sum is f64 in
 *                   one fixed order per candidate.  The result is the s_k of the smallest E_k; on equal E_k the smallest k wins.
 * A group that holds a NaN or +-Inf gets s = NaN under every method, other groups are unaffected; a group of zeros gets min_value.
 * `rounding` is validated for every method and used by LQ_INIT_MSE only.  Two runs give the same bits (no atomics); there is no
 * workspace.  A NULL pointer, qmin > qmax, a bound outside +-2^24, an unknown `rounding` or `method`, min_value not finite or <= 0,
 * gs < 1, axis not in {0, 1}, a non-positive extent and R * C >= 2^31 return LQ_EINVAL before any launch; a base off the 4-byte grid
 * returns LQ_EALIGN (16-byte aligned P with C % 4 == 0 -- and gs % 4 == 0 on axis 1 -- takes 16-byte loads).  The call only enqueues
 * ONE launch, allocates nothing, reads P's extent and writes s's extent and nothing else.  */
typedef enum lq_scale_init_method { LQ_INIT_ABSMAX = 0, LQ_INIT_LSQ = 1, LQ_INIT_MSE = 2 } lq_scale_init_method;
int lq_scale_init_group(const float* P, float* s, int32_t qmin, int32_t qmax, int rounding, int method, float min_value,
                        int64_t R, int64_t C, int axis, int64_t gs, void* stream);

/* ---- asymmetric group-wise scales: a learned offset per group ----
 * Geometry is exactly lq_fq_forward_group's: matrix [R][C] in memory order, axis, gs, nb = ceil(len / gs), ragged last group.  The
 * offset b is a dense fp32 matrix of the scale's shape and indexed like it.  lo = (float)qmin, hi = (float)qmax.  All operations
 * are fp32 unless stated otherwise, and every operation rounds on its own (the library is built without contraction: no fma
 * fuses q * s + b).
 *   u  = P - b                      (one subtraction)
 *   t  = u / s                      (IEEE division: K1's division on u)
 *   q0 = floorf(t) | rintf(t)       by `rounding`
 *   q  = q0 < lo ? lo : (q0 > hi ? hi : q0)
 *   out = (q * s) + b               (product rounds, then the sum rounds)
 *   inside = (q0 >= lo) && (q0 <= hi)
 *   dP = inside ? dy : +0.0f
 *   r  = inside ? q0 - t : q
 *   ds[g] = RN_f32( (double)grad_scale        * sum_{i in g} (double)dy_i * (double)r_i )
 *   db[g] = RN_f32( (double)offset_grad_scale * sum_{i in g, !inside_i} (double)dy_i )
 *   clipped[g] = #{ i in g : !inside_i }      exact, uint32
 * db is LSQ+'s offset gradient: under the straight-through rule d out / d b is 0 inside the range and 1 outside.
 * The sums are f64 from the first addition.  They are taken in the one fixed order the symmetric backward uses for the same
 * geometry and alignment, with no float atomics and no workspace: lq_group_workspace_bytes covers this pair too and stays 0.
 * NaN or Inf in P, s or b spoils only its own group, as for the symmetric pair.  With b == +0.0f everywhere, dP, ds and clipped
 * are bit-identical to lq_fq_backward_group on the same buffers; out is equal as a value, only -0.0 comes back as +0.0; the
 * integer view is identical.  The kernels take the symmetric pair's form, vector width, team width, row split and grid.
 * lq_fq_forward_group_affine: `out` is required; q / q_dtype optionally give the CLAMPED integers q.
 * lq_fq_backward_group_affine: dP is required; ds, db and clipped may each be NULL; both gradient pointers NULL means mask only.
 * A NULL required pointer, qmin > qmax, a bound outside +-2^24, a bad `rounding`, axis not in {0, 1}, gs < 1, a non-positive
 * extent and R * C >= 2^31 return LQ_EINVAL before any launch; a base off the 4-byte grid returns LQ_EALIGN; 16-byte accesses are
 * used under the symmetric rule (16-byte aligned dense bases, C % 4 == 0, and gs % 4 == 0 on axis 1).  Both calls only enqueue
 * (capturable), ONE launch each.
 *
 * lq_scale_init_group_minmax writes s AND b per group ("minmax").  n below is the range width, not an element count.
 *   mn = min_i P_i, mx = max_i P_i (exact);  n = (float)(qmax - qmin)
 *   s  = fmaxf( RN(RN(RN(mx - mn) / n) * (1 + 2^-22)), min_value )
 *   mid = RN(0.5f*mn + 0.5f*mx)
 *   c   = (qmin + qmax)/2 + (floor ? 1/2 : 0)      (formed in double on the host, exact as a float)
 *   b   = RN(mid - RN(c * s))
 * The data lands on t in [lo + 1/2, hi + 1/2] for floor and [lo, hi] for nearest: half a step of slack on both sides.
 * When nothing is clipped (a sufficient condition).  Let M = max_i |P_i| and let no intermediate overflow or be subnormal.  Three
 * roundings against the factor 1 + 2^-22 leave s >= (mx - mn) / n in the reals, so the exact quotient t* = (P_i - (mn + mx)/2) / s + c
 * lies in [c - n/2, c + n/2].  The computed t differs from t* by the roundings of mid, c * s, b, u and t, each at most 2^-24 of
 * its result: |t - t*| <= 2^-24 * (2 M / s + 4 |c| + n) up to second order.  Both roundings keep the element inside while
 * |t - t*| < 1/2, so NO element of the group is clipped whenever  2 M / s + 4 |c| + n <= 2^22.  For b-bit ranges (n, |c| <= 2^16)
 * that is M <= ~2^20 * s: the group's distance from zero may be up to a million steps.  Beyond it the offset's own rounding
 * exceeds the slack and an extreme element may be clipped by one code.
 * qmax > qmin and both bounds within +-2^22 are required, otherwise LQ_EINVAL (as is a bad rounding, min_value not finite or <= 0
 * and the geometry checks above); LQ_EALIGN as above.  A group holding NaN or +-Inf gets s = b = NaN.  A group of equal values
 * gets s = min_value and b by the formula (where its minimum is a zero of either sign and c == 0, the sign of b's zero is that
 * of the zero fminf kept).  ONE launch, only enqueues, no workspace, two runs give the same bits.  */
int lq_fq_forward_group_affine(const float* P, const float* s, const float* b, float* out, void* q, int q_dtype, int32_t qmin,
                               int32_t qmax, int rounding, int64_t R, int64_t C, int axis, int64_t gs, void* stream);
int lq_fq_backward_group_affine(const float* P, const float* s, const float* b, const float* dy, int32_t qmin, int32_t qmax,
                                int rounding, float grad_scale, float offset_grad_scale, float* dP, float* ds /* may be NULL */,
                                float* db /* may be NULL */, uint32_t* clipped /* may be NULL */, void* ws, size_t ws_bytes,
                                int64_t R, int64_t C, int axis, int64_t gs, void* stream);
int lq_scale_init_group_minmax(const float* P, float* s, float* b, int32_t qmin, int32_t qmax, int rounding, float min_value,
                               int64_t R, int64_t C, int axis, int64_t gs, void* stream);

/* ---- OCP microscaling (MX) element formats: a minifloat grid under one scale per group ----
 * Geometry is exactly lq_fq_forward_group's: matrix [R][C] in memory order, axis, gs clamped to the line length, nb = ceil(len / gs),
 * ragged last group; the scale is [nb][C] or [R][nb].  (An MX block is gs = 32.)
 *
 * Element formats (lq_elem_format)      id  bits  E  M  emin  emax  max
 *   LQ_ELEM_FP4_E2M1                     0    4   2  1     0     2  6
 *   LQ_ELEM_FP6_E2M3                     1    6   2  3     0     2  7.5
 *   LQ_ELEM_FP6_E3M2                     2    6   3  2    -2     4  28
 *   LQ_ELEM_FP8_E4M3 (OCP e4m3fn)        3    8   4  3    -6     8  448
 *   LQ_ELEM_FP8_E5M2 (OCP e5m2)          4    8   5  2   -14    15  57344
 * Neither fp8 format is an FNUZ variant.
 *
 * Effective scale s_eff of a stored scale s, by `scale_format` (bits(s): the fp32 pattern of s):
 *   LQ_SCALE_E8M0  s is valid iff 0x00800000 <= bits(s) < 0x7F800000 (positive, normal, finite).
 *                  nb = (bits(s) + 0x004AFB0D) & 0x7F800000: the nearest power of two in the log domain; the mantissa threshold is
 *                  sqrt(2) (fraction bits 0x3504F3) and rounds up.  s_eff = the float with pattern nb if s is valid and
 *                  nb < 0x7F800000, otherwise NaN.  So s_eff is in [2^-126, 2^127]; a zero, negative, subnormal, non-finite or too
 *                  large scale spoils its own group and no other.
 *   LQ_SCALE_FP32  s_eff = s, used as the group-wise pair uses it.
 *
 * Per element, in fp32, every operation rounding on its own; mx is the format's max:
 *   t  = P / s_eff                              IEEE division
 *   a  = |t|;  e = max(unbiased exponent field of a, emin)      (zero / fp32-subnormal a: the field is -127, so e = emin)
 *   u  = 2^(e - M)
 *   q0 = copysign(rintf(a / u) * u, t)          ties to even; a / u and the product are exact; a non-finite t passes through
 *   inside = |q0| <= mx                         false for NaN
 *   q  = q0 < -mx ? -mx : (q0 > mx ? mx : q0)   comparisons: NaN stays NaN, +-Inf saturates
 *   out = q * s_eff
 *   dP = inside ? dy : +0.0f
 *   r  = inside ? q0 - t : q
 *   ds[g]      = RN_f32( (double)grad_scale * sum_{i in g} (double)dy_i * (double)r_i )      f64 from the first addition
 *   clipped[g] = #{ i in g : !inside_i }        exact, uint32
 * ds is the straight-through gradient with respect to the STORED s: the power-of-two rounding passes it unchanged.  With E8M0, t,
 * q0 - t and out are exact barring under/overflow; only the order of the f64 sum is left open, and it is the group-wise backward's
 * for the same geometry and alignment: no atomics, no workspace, run-to-run bit-stable.
 *
 * Code view.  The optional integer output of the forward (`code` / `code_dtype`, the q / q_dtype mechanism of the other forwards)
 * holds the element's ENCODING, the bits a packed MX operand carries:
 *   sign = signbit(q), a = |q|;  a < 2^emin: mag = a * 2^(M - emin);  otherwise, with e the exponent of a,
 *   mag = (e - emin + 1) * 2^M + (a * 2^(M - e) - 2^M);  code = sign * 2^(E+M) + mag, in [0, 2^bits); -0.0 keeps its sign bit.
 *   A NaN q gets code 2^(E+M) - 1: all ones below the sign bit, sign bit clear (the sign of a NaN is not defined by the arithmetic
 *   that made it).
 *
 * lq_fq_forward_mx: `out` is required.  lq_fq_backward_mx: dP is required, ds == NULL means mask only, clipped may be NULL.
 * LQ_EINVAL and LQ_EALIGN under exactly the conditions of the group-wise pair (range and rounding aside: there are none); an
 * unknown `format`, `scale_format` or `method` returns LQ_EINVAL too.  The kernels take the group-wise pair's form, vector width,
 * team width, row split and grid.  Each call only enqueues (capturable) ONE launch, needs no workspace and reads no environment.
 *
 * lq_scale_init_mx writes a power-of-two starting scale per group (s is the OUTPUT).  A = max_i |P_i| (exact) = m * 2^e with m in
 * [1, 2), a subnormal A normalised; mx = mm * 2^emax with mm = 1.5, 1.875, 1.75, 1.75, 1.75 in table order.
 *   LQ_MX_INIT_OCP    p = 2^(e - emax): the OCP MX rule; elements up to 2^(emax+1) steps may saturate.
 *   LQ_MX_INIT_COVER  p = m <= mm ? 2^(e - emax) : 2^(e - emax + 1): the smallest power of two under which nothing saturates.
 * p is raised to 2^-126 if below it; the result is fmaxf(p, min_value) (min_value > 0 and finite, else LQ_EINVAL).  A group of
 * zeros gets min_value, a group holding NaN or +-Inf gets NaN.  Integer exponent arithmetic: no rounding is involved.  */
typedef enum lq_elem_format {
    LQ_ELEM_FP4_E2M1 = 0, LQ_ELEM_FP6_E2M3 = 1, LQ_ELEM_FP6_E3M2 = 2, LQ_ELEM_FP8_E4M3 = 3, LQ_ELEM_FP8_E5M2 = 4
} lq_elem_format;
typedef enum lq_scale_format { LQ_SCALE_E8M0 = 0, LQ_SCALE_FP32 = 1 } lq_scale_format;
typedef enum lq_mx_init_method { LQ_MX_INIT_OCP = 0, LQ_MX_INIT_COVER = 1 } lq_mx_init_method;
int lq_fq_forward_mx(const float* P, const float* s, float* out, void* code, int code_dtype, int format, int scale_format,
                     int64_t R, int64_t C, int axis, int64_t gs, void* stream);
int lq_fq_backward_mx(const float* P, const float* s, const float* dy, int format, int scale_format, float grad_scale, float* dP,
                      float* ds /* may be NULL: mask only */, uint32_t* clipped /* may be NULL */, int64_t R, int64_t C, int axis,
                      int64_t gs, void* stream);
int lq_scale_init_mx(const float* P, float* s /* out */, int format, int method, float min_value, int64_t R, int64_t C, int axis,
                     int64_t gs, void* stream);

/* ---- quantization statistics of the clipped pair: per group and per tensor, read only ----
 * What the quantizer does to P under the scales (and offsets) it has NOW: how much each group loses on either side of the range,
 * the squared error and the squared signal of each group, and the histogram of the codes of the tensor.
 * Geometry is exactly lq_fq_forward_group's: matrix [R][C] in memory order, axis, gs clamped to the line length, nb = ceil(len / gs),
 * ragged last group; s (and b) are [nb][C] or [R][nb].  A bias with a scalar scale is R = 1, C = numel, axis = 1, gs = numel.
 * b == NULL: the symmetric pair; otherwise the offset of the asymmetric pair, the scale's shape.  lo = (float)qmin, hi = (float)qmax.
 * Per element, in fp32, every operation rounding on its own (the library is built without contraction):
 *   u  = P - b                      (with an offset only; otherwise u is P)
 *   t  = u / s                      (IEEE division: the forward's quotient bit for bit)
 *   q0 = floorf(t) | rintf(t)       by `rounding`
 *   q  = q0 < lo ? lo : (q0 > hi ? hi : q0)
 *   out = q * s                     (with an offset: (q * s) + b, product and sum round separately)
 * Per group g, in the scale's shape:
 *   below[g] = #{ i in g : q0_i < lo }        exact, uint32
 *   above[g] = #{ i in g : q0_i > hi }        exact, uint32      (below + above is lq_fq_backward_group's clipped)
 *   err2[g]  = sum_{i in g} e_i * e_i  with e_i = (double)P_i - (double)out_i;  the product and the addition round separately
 *   sig2[g]  = sum_{i in g} (double)P_i * (double)P_i
 * The group's SQNR is 10 log10 of sig2 / err2.  The sums are f64 from the first addition and taken in one fixed order (no float
 * atomics, no workspace): two runs give the same bits.  All four are written for every group.
 * Per tensor, when hist != NULL: hist[q - qmin] += 1 for every element whose q is a number; qmax - qmin + 1 uint32 bins that the
 * caller has zeroed (counts are ADDED, as by lq_q_histogram).  The bins are summed with integer atomics, which are exact in
 * any order.  hist != NULL needs qmax - qmin + 1 <= 4096, otherwise LQ_EINVAL.
 * Non-finite values: a NaN q0 counts on neither side and is not binned, and its group's err2 is NaN by IEEE arithmetic; +-Inf t
 * counts on its side and q saturates at the bound.  Other groups are unaffected.
 * A NULL P, s, below, above, err2 or sig2, qmin > qmax, a bound outside +-2^24, a bad `rounding`, axis not in {0, 1}, gs < 1, a
 * non-positive extent and R * C >= 2^31 return LQ_EINVAL before any launch.  P, s, b, below, above or hist off the 4-byte grid and
 * err2 or sig2 off the 8-byte grid return LQ_EALIGN; 16-byte loads of P are used under the group rule (16-byte aligned P,
 * C % 4 == 0, and gs % 4 == 0 on axis 1).  The kernels take the group-wise backward's form, team width and grid.  The call only
 * enqueues ONE launch (capturable), allocates nothing, reads the extents of P, s and b and writes the extents of its five
 * outputs and nothing else.  */
int lq_group_stats(const float* P, const float* s, const float* b /* NULL: symmetric */, int32_t qmin, int32_t qmax, int rounding,
                   uint32_t* below, uint32_t* above, double* err2, double* sig2, uint32_t* hist /* may be NULL */,
                   int64_t R, int64_t C, int axis, int64_t gs, void* stream);

/* ---- quantization statistics of the microscaling pair: per group and per tensor, read only ----
 * What lq_group_stats is for the integer grid, for the minifloat grids of lq_fq_forward_mx under the scales P has NOW: how much each
 * group saturates on either side, how much of it the grid flushes to zero, its squared error and squared signal, and the
 * histogram of the encodings of the tensor.
 * Geometry is exactly lq_fq_forward_mx's: matrix [R][C] in memory order, axis, gs clamped to the line length, nb = ceil(len / gs),
 * ragged last group; s is [nb][C] or [R][nb].  A bias with a scalar scale is R = 1, C = numel, axis = 1, gs = numel.
 * Per element, the definition under "OCP microscaling (MX) element formats" above, operation for operation: s_eff by
 * `scale_format`, t = P / s_eff, q0 (t on the element grid, ties to even), q = q0 < -mx ? -mx : (q0 > mx ? mx : q0),
 * out = q * s_eff; mx is the format's max.
 * Per group g, in the scale's shape:
 *   below[g]   = #{ i in g : q0_i < -mx }     exact, uint32
 *   above[g]   = #{ i in g : q0_i > mx }      exact, uint32      (below + above is lq_fq_backward_mx's clipped)
 *   flushed[g] = #{ i in g : P_i != 0 and q_i == 0 }      exact, uint32: the elements the grid turns into +-0 (|t| <= half the
 *                smallest subnormal 2^(emin - M)); a NaN q is not zero
 *   err2[g]    = sum_{i in g} e_i * e_i  with e_i = (double)P_i - (double)out_i;  the product and the addition round separately
 *   sig2[g]    = sum_{i in g} (double)P_i * (double)P_i
 * The group's SQNR is 10 log10 of sig2 / err2.  The sums are f64 from the first addition and taken in one fixed order (no float
 * atomics, no workspace): two runs give the same bits.  All five are written for every group.
 * Per tensor, when hist != NULL: hist[code] += 1 for every element whose q is a number, `code` the element's encoding exactly as
 * the forward's code view defines it (-0.0 keeps its sign bit); 2^bits uint32 bins (16 / 64 / 256) that the caller has zeroed
 * (counts are ADDED).  A NaN q is not binned: its "code" 2^(E+M) - 1 is a value's code in the fp4 and fp6 formats.  The bins are
 * summed with integer atomics, which are exact in any order.
 * Non-finite values: a NaN q0 counts on neither side, is not flushed and is not binned, and its group's err2 is NaN by IEEE
 * arithmetic; +-Inf t counts on its side and q saturates at +-mx.  An invalid E8M0 scale gives a NaN s_eff: nothing of its group
 * is counted on any side, as flushed, or binned, the group's err2 is NaN and its sig2 is still the sum of squares.  Other groups
 * are unaffected.
 * A NULL P, s, below, above, flushed, err2 or sig2, an unknown `format` or `scale_format`, axis not in {0, 1}, gs < 1, a
 * non-positive extent and R * C >= 2^31 return LQ_EINVAL before any launch.  P, s, below, above, flushed or hist off the 4-byte
 * grid and err2 or sig2 off the 8-byte grid return LQ_EALIGN; 16-byte loads of P are used under the group rule (16-byte aligned P,
 * C % 4 == 0, and gs % 4 == 0 on axis 1).  The kernels take the group-wise backward's form, team width and grid.  The call only
 * enqueues ONE launch (capturable), allocates nothing, reads no environment, reads the extents of P and s and writes the extents
 * of its six outputs and nothing else.  */
int lq_mx_stats(const float* P, const float* s, int format, int scale_format, uint32_t* below, uint32_t* above, uint32_t* flushed,
                double* err2, double* sig2, uint32_t* hist /* may be NULL */, int64_t R, int64_t C, int axis, int64_t gs,
                void* stream);

/* ---- packed MX operands and the block-scaled GEMM ----
 * An OPERAND is a matrix of L lines by K reduction elements in the order gfx950's v_mfma_scale_f32_16x16x128_f8f6f4 consumes it:
 * element codes at the instruction's width (8 bits: LQ_ELEM_FP8_E4M3, LQ_ELEM_FP8_E5M2; 4 bits: LQ_ELEM_FP4_E2M1) and one E8M0 byte
 * per block of 32 along K.  To callers it is opaque apart from its size (lq_mx_operand_bytes); the layout is stated here so that it
 * can be checked:
 *   LT = ceil(L / 16), KT = ceil(K / 128), KG = ceil(KT / 4), FB = 32 (fp8) or 16 (fp4) bytes per fragment
 *   codes   [LT][KT][64][FB]   fragment `lane` of tile (lt, kt) holds line 16 lt + (lane & 15) and, with g = lane >> 4, of K step kt
 *                              fp4: k = 32 g + j, j = 0 .. 31 (one MX block), element j in bits 4 (j & 1) .. + 3 of byte j >> 1;
 *                              fp8: k = 16 g + j in byte j and k = 64 + 16 g + j in byte 16 + j, j = 0 .. 15 (halves of two blocks)
 *   scales  [LT][KG][64][4]    byte u of dword `lane` of cell (lt, kg) is the E8M0 byte of block g (k = 32 g .. 32 g + 31) of K step
 *                              kt = 4 kg + u of that line, for every format
 *   code_bytes = LT * KT * 64 * FB, scale_bytes = LT * KG * 256.  Lines past L and elements past K hold code 0 under byte 127, and
 *   the scale bytes of the K steps KT .. 4 KG - 1, which no instruction reads, are 127 too: the buffers are a function of the input.
 * This is the lane map of the instruction as pinned on the device by exact-arithmetic GEMM tests (tests/test_gpu_mx_gemm.py): lane l
 * supplies the A (B) line l & 15; 4-bit data is one block per lane, 8-bit data two half blocks 64 apart; the scale byte selected by
 * op-sel from lane l's scale register applies to block l >> 4 whichever lane holds its data; the result tile has column l & 15 on the
 * lane and rows 4 (l >> 4) + r in register r.
 * The scale byte of a block is the biased exponent of its s_eff (a power of two in [2^-126, 2^127]: bytes 1 .. 254); byte 255
 * marks a block whose s_eff is NaN.  Pack and quantize never write byte 0; decode and the GEMM accept it in a buffer built elsewhere
 * and read it as OCP defines E8M0, 2^-127.
 *
 * lq_mx_operand_pack: the operand of a stored parameter under its stored scales.  Geometry is lq_fq_forward_group's ([R][C] in
 * memory order, s [nb][C] or [R][nb]).  axis 0: the lines are the C columns and K = R (a Dense kernel (in, out)); axis 1: the lines
 * are the R rows and K = C (a conv kernel stored OIHW seen as (co, ci kh kw)).  The code of every element is bit for bit the code
 * view of lq_fq_forward_mx under LQ_SCALE_E8M0, NaN code rule included; the element step is that kernel's.
 * lq_mx_operand_quantize: the operand of a row-major X [M][K] (lines: rows; blocks of 32 along the contiguous axis) under scales
 * taken from X itself: per block what lq_scale_init_mx(X, s, format, method, min_value = 2^-126, M, K, axis 1, gs 32) writes, then
 * the codes of lq_fq_forward_mx under that scale.  A block holding a NaN or an Inf gets byte 255.  One read of X.
 * lq_mx_operand_decode: out [L][K] row-major, out = value(code) * 2^(byte - 127) in fp32 (byte 255: NaN) -- for a packed parameter
 * lq_fq_forward_mx's `out` bit for bit, except where the format has no NaN code (fp4) and the element is NaN under a valid scale.
 * lq_mx_gemm: Y[m][n] = sum_k A[m][k] * B[n][k] (+ bias[n]) in fp32, Y row-major with leading dimension ldy >= N, A and B operands of
 * M and N lines over the same K, any of the nine format pairs.  The products and the sum of a K step of 128 are the instruction's;
 * the steps accumulate in ascending K into fp32; the bias is added last, one fp32 addition.  No atomics: run-to-run bit-stable.
 * Every element code is the instruction's: subnormals, the top binade, NaN (fp8_e4m3 S.1111.111; fp8_e5m2 S.11111.mm) and +-Inf
 * (fp8_e5m2) multiply as IEEE values do (0 * Inf = NaN).  The two scale bytes of a product act on its EXPONENT, not on one operand at
 * a time in fp32: a product under bytes 254 and 1, or 0 and 254, is exact although one scaled operand alone leaves fp32's normal
 * range; a block under byte 255 makes its line's results NaN.  Measured on an MI355X, one term per output, bytes 0 .. 255 on both
 * sides (tests/test_gpu_mx_gemm_codes.py): exact inside [2^-126, 2^128), +-Inf from 2^128, and below 2^-126 the correctly rounded
 * fp32 SUBNORMAL (nearest, ties to even) -- nothing is flushed; a result that rounds to zero is +0 whatever the product's sign.
 *
 * LQ_EINVAL before any launch: a NULL pointer (bias may be NULL), a non-positive extent, L * K >= 2^31, an unknown format or
 * method, an fp6 format (6-bit lanes need a 96-byte fragment packing of their own: not built), scale_format LQ_SCALE_FP32 (the
 * instruction takes E8M0 only), gs != 32, ldy < N.  LQ_EALIGN: codes off the 16-byte grid; scales, P, s, X, bias, out or Y off the
 * 4-byte grid.  16-byte loads of P / X are used where the base is 16-byte aligned and the contiguous axis a multiple of 4 (axis 1
 * and quantize).  Each call only enqueues ONE launch (capturable), allocates nothing, reads no environment, and writes exactly
 * code_bytes and scale_bytes (pack, quantize), L * K floats (decode) or the M x N elements of Y (gemm).  */
int lq_mx_operand_bytes(int format, int64_t L, int64_t K, size_t* code_bytes, size_t* scale_bytes);
int lq_mx_operand_pack(const float* P, const float* s, int format, int scale_format, int64_t R, int64_t C, int axis, int64_t gs,
                       void* codes, void* scales, void* stream);
int lq_mx_operand_quantize(const float* X, int format, int method, int64_t M, int64_t K, void* codes, void* scales, void* stream);
int lq_mx_operand_decode(const void* codes, const void* scales, int format, int64_t L, int64_t K, float* out, void* stream);
int lq_mx_gemm(const void* a_codes, const void* a_scales, int a_format, const void* b_codes, const void* b_scales, int b_format,
               const float* bias /* may be NULL */, float* Y, int64_t M, int64_t N, int64_t K, int64_t ldy, void* stream);

/* lq_mx_gemm_quantize: lq_mx_gemm with an operand-out epilogue.  Instead of an fp32 Y it writes the operand of act(Y) for the NEXT
 * product: L = M lines over K' = N, elements of out_format (LQ_ELEM_FP8_E4M3, LQ_ELEM_FP8_E5M2 or LQ_ELEM_FP4_E2M1) under block
 * scales taken from act(Y) by `method` (lq_mx_init_method).  out_codes / out_scales have lq_mx_operand_bytes(out_format, M, N)
 * bytes, and byte for byte they are what
 *     lq_mx_operand_quantize(act(lq_mx_gemm(a, b, bias)), out_format, method, M, N)
 * writes, padding included: the K loop is lq_mx_gemm's (same fragments, same instructions, ascending K), the bias is the same one
 * fp32 addition, and the scale rule and the element step are lq_mx_operand_quantize's.  LQ_ACT_NONE leaves v as it is; LQ_ACT_RELU
 * is v > 0 ? v : (v != v ? v : +0): a NaN stays NaN, negative values and -0 become +0.
 * It writes exactly those bytes in ONE launch (no memset, no fp32 intermediate), is capturable, allocates nothing and reads no
 * environment.  LQ_EINVAL before any launch: a NULL pointer (bias may be NULL), a non-positive extent, M * K, N * K or M * N >= 2^31,
 * an unknown or fp6 format on any of the three sides, a bad method, a bad activation, M above 65535 * 64.  LQ_EALIGN: codes off the
 * 16-byte grid; scales or bias off the 4-byte grid.  */
typedef enum lq_mx_activation { LQ_ACT_NONE = 0, LQ_ACT_RELU = 1 } lq_mx_activation;
int lq_mx_gemm_quantize(const void* a_codes, const void* a_scales, int a_format, const void* b_codes, const void* b_scales, int b_format,
                        const float* bias /* may be NULL */, int activation, int out_format, int method, void* out_codes,
                        void* out_scales, int64_t M, int64_t N, int64_t K, void* stream);

/* lq_mx_operand_im2col: the A operand of a convolution run as a GEMM, gathered from the input in one launch -- the im2col matrix
 * never exists in fp32.  With OH = (H + pad_top + pad_bottom - KH) / stride_h + 1 (rounded down; OW likewise from W, the left and
 * right pads, KW and stride_w), M = B * OH * OW lines and K = C * KH * KW:
 *     line m = (b * OH + oh) * OW + ow,  reduction index k = (c * KH + i) * KW + j
 *     A[m][k] = X[b][c][oh * stride_h - pad_top + i][ow * stride_w - pad_left + j]   where that pixel exists, +0 otherwise
 * k is the memory order of the (ci, kh, kw) run of an OIHW kernel, so the B side is lq_mx_operand_pack(kernel, R = co,
 * C = ci * kh * kw, axis 1) and lq_mx_gemm(A, B) is the convolution as [M][co], i.e. NHWC.  codes / scales have
 * lq_mx_operand_bytes(format, M, K) bytes and, byte for byte, padding and idle scale bytes included, hold what
 * lq_mx_operand_quantize(A, format, method, M, K) writes: a padding zero takes part in its block as a zero, an all-zero block gets
 * byte 1, and a block whose window covers a NaN or Inf pixel gets byte 255 -- no other block does.  X is addressed through its
 * strides, given in ELEMENTS (NCHW-contiguous, channels_last or any view with non-negative strides), in 64-bit arithmetic, with
 * 4-byte loads; no byte of X is read that the definition does not name.
 * lq_mx_im2col_dims answers M, K, OH and OW of a geometry (the strides of X are not read) and runs nothing on a device; it accepts
 * an M * K that the operand call refuses, so that a caller can cut the batch.
 * LQ_EINVAL before any launch: a NULL pointer, a non-positive extent, kernel size or stride, a negative pad, OH or OW < 1, an
 * unknown or fp6 format, an unknown method, M * K >= 2^31, a negative stride of X.  LQ_EALIGN: codes off the 16-byte grid; scales or
 * X off the 4-byte grid.  The operand call only enqueues ONE launch (capturable), allocates nothing, reads no environment and writes
 * exactly code_bytes and scale_bytes.  Dilation and groups are not built.  */
typedef struct lq_conv_geom {
    int64_t B, C, H, W;               /* the input, logically [B][C][H][W] */
    int64_t xs_b, xs_c, xs_h, xs_w;   /* its strides in ELEMENTS */
    int32_t KH, KW, stride_h, stride_w;
    int32_t pad_top, pad_left, pad_bottom, pad_right;   /* zero padding, each >= 0 */
} lq_conv_geom;
int lq_mx_im2col_dims(const lq_conv_geom* g, int64_t* M, int64_t* K, int64_t* OH, int64_t* OW);
int lq_mx_operand_im2col(const float* X, const lq_conv_geom* g, int format, int method, void* codes, void* scales, void* stream);

/* ---- packed int8 operands and the int8 GEMM ----
 * The integer counterpart of the packed MX operands: a trained b-bit layer (b <= 8, signed range) multiplied on gfx950's
 * v_mfma_i32_16x16x64_i8.  An OPERAND is a matrix of L lines by K reduction elements: one int8 code per element and fp32 scales,
 * one per line and per SCALE BLOCK of `block` consecutive k.  block == 0: one scale per line (nbs = 1); otherwise
 * block % 64 == 0 and nbs = ceil(K / block), the last block may be short.  To callers it is opaque apart from its sizes
 * (lq_i8_operand_bytes); the layout is stated here so that it can be checked:
 *   LT = ceil(L / 16), KT = ceil(K / 64)
 *   codes   [LT][KT][64][16]   fragment `lane` of tile (lt, kt) holds line 16 lt + (lane & 15) and k = 64 kt + 16 (lane >> 4) + j in
 *                              byte j, j = 0 .. 15 (two's complement).  The byte of (line, k) is at
 *                              (((line >> 4) * KT + (k >> 6)) * 64 + 16 * ((k & 63) >> 4) + (line & 15)) * 16 + (k & 15)
 *   scales  [nbs][16 LT] fp32  the scale of (block, line) at index block * 16 LT + line
 *   code_bytes = LT * KT * 1024, scale_bytes = nbs * LT * 64.  Lines past L and k past K hold code 0; scales of lines past L are 1.0f.
 * What the device pins about the instruction (tests/test_gpu_i8.py: one-hot operands for every k = 0 .. 127, every code against
 * {-128, -1, 1, 127}): lane l supplies line l & 15 of A and of B; A's lines are the result's rows, B's its columns (column l & 15 on
 * the lane, rows 4 (l >> 4) + r in register r); both operands take the same k from the same (lane >> 4, byte).  The instruction
 * adds all 64 k of a step into one int32, so the NAME of the k that a (lane >> 4, byte) pair holds cannot be observed: any
 * permutation of k inside a step applied to both operands gives the same sums.  The rule above -- 16 consecutive k per lane, no
 * two half blocks as 8-bit data in the block-scaled instruction -- is therefore this library's definition, not a hardware fact, and
 * scale blocks are whole steps so that nothing depends on it.
 *
 * lq_i8_operand_pack: the operand of a stored parameter under its stored scales, in lq_fq_forward_group's geometry exactly
 * ([R][C] in memory order; axis 0: s [nb][C], the lines are the C columns and K = R; axis 1: s [R][nb], the lines are the R rows and
 * K = C).  The codes are the clamped integers of lq_fq_forward_group's LQ_Q_I8 integer view (the same element step, `rounding`
 * included); the scales are s copied bit for bit.  gs >= K gives block = 0; otherwise gs % 64 == 0 is required and block = gs.
 * lq_i8_operand_quantize: the dynamic symmetric quantizer of a row-major X [M][K] (lines: rows).  Per (row, scale block) the scale
 * is lq_scale_init_group's LQ_INIT_ABSMAX with qmin = -127, qmax = 127, min_value = 2^-126, and the codes are the clipped step
 * with LQ_ROUND_NEAREST_EVEN under that scale: byte for byte the buffers of
 *     lq_i8_operand_pack(X, lq_scale_init_group(X, ABSMAX, -127, 127, axis 1, gs = block or K), -127, 127, nearest, M, K, axis 1, ...)
 * A row block of zeros gets scale 2^-126 and codes 0.  A NaN or +-Inf element gives that one block a NaN scale; its codes are
 * then all 0, because the integer view stores 0 for a NaN quotient (as lq_fq_forward_group's does).  One launch; a scale block
 * (a row for block == 0) of up to 4096 elements (1024 where K % 4 != 0 or X is off the 16-byte grid) is read from memory once,
 * the tail of a longer one a second time.
 * lq_i8_operand_decode: out [L][K] row-major, out = (float)code * scale, one fp32 product.  For a packed parameter this equals
 * lq_fq_forward_group's `out` as values, with two exceptions that both come from code 0: a -0.0 there (a negative element that
 * rounds to zero) decodes as +0.0, and a NaN element under a valid scale, NaN there, decodes as 0 (the integer view stores 0 for
 * it).  Under a NaN scale both are NaN.
 * lq_i8_gemm: Y[m][n] = sum_k A[m][k] B[n][k] (+ bias[n]), Y row-major with leading dimension ldy >= N, A and B operands of M and N
 * lines over the same K with scale blocks a_block and b_block.  DEFINITION (bit exact; tests/_i8_reference.py states it in NumPy):
 *   a PERIOD is a maximal run of k on which neither operand's scale changes: the whole K if both blocks are 0, otherwise runs of
 *   F = the smaller non-zero block (the larger must be a multiple of it, else LQ_EINVAL); the last period may be short.  A period
 *   longer than 65536 is refused: |a b| <= 2^14, so 65536 terms stay inside int32.  For output (m, n), over the periods p in
 *   ascending k, starting from y = +0:
 *       I_p = sum_{k in p} a[m][k] * b[n][k]            exact, int32
 *       t_p = RN(sa[m][p] * sb[n][p])                   fp32
 *       y   = RN(y + RN((float)I_p * t_p))              (float): round to nearest even; the product and the sum round separately
 *   and last, with a bias, y = RN(y + bias[n]).  A NaN scale makes its row or column NaN and touches nothing else.  No atomics:
 *   run-to-run bit-stable.
 *
 * LQ_EINVAL before any launch: a NULL pointer (bias may be NULL), a non-positive extent, L * K >= 2^31, a block that is negative
 * or no multiple of 64, a period above 65536, blocks of which neither divides the other, ldy < N, M above 65535 * 64; for pack also
 * a range not inside [-128, 127], a gs that is neither >= K nor a multiple of 64, and everything lq_fq_forward_group refuses.
 * LQ_EALIGN: codes or scales off the 16-byte grid; P, s, X, bias, out or Y off the 4-byte grid.  Each call only enqueues ONE launch
 * (capturable), allocates nothing, reads no environment, and writes exactly code_bytes and scale_bytes (pack, quantize), L * K
 * floats (decode) or the M x N elements of Y (gemm).
 *
 * lq_i8_operand_im2col: the A operand of a convolution run as an int8 GEMM, gathered from the input in one launch -- the im2col
 * matrix never exists in fp32.  M, K, OH, OW and A[m][k] are exactly lq_mx_operand_im2col's (lq_mx_im2col_dims answers the
 * extents): line m = (b * OH + oh) * OW + ow, k = (c * KH + i) * KW + j, +0 where the pixel does not exist.  codes / scales have
 * lq_i8_operand_bytes(M, K, block) bytes and hold, byte for byte, what lq_i8_operand_quantize(A, M, K, block) writes, the padding
 * of lines and of k and the scales of lines past M included: a (line, scale block) whose taps are all padding or all zero gets
 * scale 2^-126 and codes 0; one whose taps cover a NaN or +-Inf pixel gets a NaN scale and codes 0, and no other pair does.  k is
 * the memory order of the (ci, kh, kw) run of an OIHW kernel, so the B side is lq_i8_operand_pack(kernel, R = co,
 * C = ci * kh * kw, axis 1) and lq_i8_gemm(A, B) is the convolution as [M][co].  X is addressed through its strides, given in
 * ELEMENTS (NCHW-contiguous, channels_last or any view with non-negative strides), in 64-bit arithmetic, with 4-byte loads; no
 * byte of X is read that the definition does not name.  A span (scale block, or the padded row for block == 0) of more than 64 k is
 * split over the four waves of a thread block and merged through LDS; the result does not depend on the form.
 * LQ_EINVAL before any launch: everything lq_mx_operand_im2col refuses about the geometry (a NULL pointer, a non-positive extent,
 * kernel size or stride, a negative pad, OH or OW < 1, a negative stride of X) and everything lq_i8_operand_quantize refuses about
 * M, K and block (M * K >= 2^31, a block that is negative or no multiple of 64).  LQ_EALIGN: codes or scales off the 16-byte grid, X
 * off the 4-byte grid.  ONE launch (capturable), no memset, no atomics; allocates nothing, reads no environment and writes exactly
 * code_bytes and scale_bytes.  Dilation and groups are not built.
 *
 * lq_i8_gemm_quantize: lq_i8_gemm with an operand-out epilogue.  Instead of an fp32 Y it writes the int8 operand of act(Y) for the
 * NEXT product: L = M lines over K' = N with scale blocks of out_block.  out_codes / out_scales have
 * lq_i8_operand_bytes(M, N, out_block) bytes, and byte for byte they are what
 *     lq_i8_operand_quantize(act(lq_i8_gemm(a, b, bias)), M, N, out_block)
 * writes, the padding included: codes of lines past M and of k past N up to 64 ceil(N / 64) are 0, scales of lines
 * M .. 16 ceil(M / 16) - 1 are 1.0f.  Y is lq_i8_gemm's DEFINITION exactly (it does not depend on a tiling, so the kernel's wave
 * shape is its own: 16 rows by 64 columns), the bias is the same single RN addition, and the scale rule and the element step are
 * lq_i8_operand_quantize's.  `activation` is an lq_mx_activation: LQ_ACT_NONE leaves v as it is; LQ_ACT_RELU is
 * v > 0 ? v : (v != v ? v : +0).  A (row, block) of zeros -- or all non-positive under relu -- gets scale 2^-126 and codes 0; a NaN
 * or +-Inf value gives that one (row, block) a NaN scale and codes 0 and touches no other pair.
 * out_block must be 64: a block of 64 outputs is the smallest the layout allows, and one thread block's 64 columns cover it.  One
 * scale per row (0) or a larger block needs every column tile of the row before the first code: a different kernel, refused.
 * ONE launch (capturable): no memset, no fp32 intermediate, no atomics, no workspace; it reads no environment and writes exactly
 * code_bytes and scale_bytes.  LQ_EINVAL before any launch: everything lq_i8_gemm refuses about pointers, extents, blocks and
 * periods (there is no ldy), out_block != 64, an unknown activation, M * N >= 2^31, M above 65535 * 64.  LQ_EALIGN: what lq_i8_gemm
 * refuses, and out_codes or out_scales off the 16-byte grid.
 *
 * OFFSETS ON THE B OPERAND (asymmetric group-wise layers, W[n][k] = q[n][k] s[n][g] + b[n][g]).  An operand's `offsets` is an fp32
 * buffer in the layout of its scales: [nbs][16 LT], scale_bytes long, on the 16-byte grid, the offset of (block, line) at index
 * block * 16 LT + line; offsets of lines past L are +0.0f.  Only B carries offsets; the A side (lq_i8_operand_quantize,
 * lq_i8_operand_im2col) is unchanged, and its padded k and padded conv taps hold code 0 and so add nothing to a row sum.
 * lq_i8_operand_pack_affine: lq_i8_operand_pack's geometry and refusals; b has the shape of s.  The codes are the clamped integers
 * of lq_fq_forward_group_affine's LQ_Q_I8 integer view, from the same element step (u = P - b, the quotient, the rounding and the
 * clamp); scales is s bit for bit and offsets is b bit for bit.
 * lq_i8_operand_decode_affine: out = RN(RN((float)code * scale) + offset).  For a packed parameter this equals
 * lq_fq_forward_group_affine's `out` as values, except for a NaN element under a valid scale (code 0 decodes as the offset).
 * lq_i8_gemm_affine: lq_i8_gemm's refusals and periods; B's offsets change where its scales change.  DEFINITION (bit exact;
 * tests/_i8_affine_reference.py states it in NumPy): everything of lq_i8_gemm holds, and in each period p, directly after
 * y = RN(y + RN((float)I_p * t_p)):
 *       R_p = sum_{k in p} a[m][k]                      exact, int32 (|R_p| <= 2^23: a period is at most 65536)
 *       c_p = RN((float)R_p * sa[m][p])                 fp32, per row: independent of n
 *       y   = RN(y + RN(c_p * ob[n][p]))                the product and the sum round separately
 *   The bias follows last, as before.  A NaN offset makes its column NaN and touches nothing else.  With all offsets +-0 and
 *   finite scales Y is lq_i8_gemm's bit for bit (y is never -0).  The definition does not depend on a tiling.
 * lq_i8_gemm_quantize_affine: lq_i8_gemm_quantize with b_offsets: byte for byte
 *     lq_i8_operand_quantize(act(lq_i8_gemm_affine(a, b, bias)), M, N, 64)
 * the padding included.
 * Each of the four is ONE launch (capturable); none allocates, uses atomics or a workspace, or reads the environment.  They refuse
 * what their symmetric twins refuse, and LQ_EINVAL for a NULL b / offsets / b_offsets, LQ_EALIGN for b off the 4-byte grid or
 * offsets off the 16-byte grid.  The row sums cost matrix instructions (one more per A tile and K step: 6 instead of 4 in
 * lq_i8_gemm_affine, 5 instead of 4 in lq_i8_gemm_quantize_affine), which is why a caller opts in.
 *
 * Not built: epilogue output blocks other than 64 (per row, 128), offsets on the A operand (asymmetric activations), HWIO-stored conv kernels, any backward, sub-byte packing of
 * 4-bit codes.  */
int lq_i8_operand_bytes(int64_t L, int64_t K, int64_t block, size_t* code_bytes, size_t* scale_bytes);
int lq_i8_operand_pack(const float* P, const float* s, int32_t qmin, int32_t qmax, int rounding, int64_t R, int64_t C, int axis,
                       int64_t gs, void* codes, void* scales, void* stream);
int lq_i8_operand_quantize(const float* X, int64_t M, int64_t K, int64_t block, void* codes, void* scales, void* stream);
int lq_i8_operand_decode(const void* codes, const void* scales, int64_t L, int64_t K, int64_t block, float* out, void* stream);
int lq_i8_operand_im2col(const float* X, const lq_conv_geom* g, int64_t block, void* codes, void* scales, void* stream);
int lq_i8_gemm(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales, int64_t b_block,
               const float* bias /* may be NULL */, float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, void* stream);
int lq_i8_gemm_quantize(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales,
                        int64_t b_block, const float* bias /* may be NULL */, int activation /* lq_mx_activation */,
                        int64_t out_block, void* out_codes, void* out_scales, int64_t M, int64_t N, int64_t K, void* stream);
int lq_i8_operand_pack_affine(const float* P, const float* s, const float* b, int32_t qmin, int32_t qmax, int rounding, int64_t R,
                              int64_t C, int axis, int64_t gs, void* codes, void* scales, void* offsets, void* stream);
int lq_i8_operand_decode_affine(const void* codes, const void* scales, const void* offsets, int64_t L, int64_t K, int64_t block,
                                float* out, void* stream);
int lq_i8_gemm_affine(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales,
                      const void* b_offsets, int64_t b_block, const float* bias /* may be NULL */, float* Y, int64_t ldy, int64_t M,
                      int64_t N, int64_t K, void* stream);
int lq_i8_gemm_quantize_affine(const void* a_codes, const void* a_scales, int64_t a_block, const void* b_codes, const void* b_scales,
                               const void* b_offsets, int64_t b_block, const float* bias /* may be NULL */,
                               int activation /* lq_mx_activation */, int64_t out_block, void* out_codes, void* out_scales, int64_t M,
                               int64_t N, int64_t K, void* stream);

/* ---- K4: forward and NQ backward of one tensor in a single pass (benchmark path) ---
 * Same results as lq_fq_forward followed by lq_fq_scale_grad (out, max|q| and the vote count bit for bit; on
 * streaming-size tensors the vote sum may differ by fp32 summation order, ~1e-7 relative); P is read once.  */
int lq_fq_fwd_bwd_fused(const float* P, const float* s, const float* dy, float lambda,
                        float* out, float* ds, void* ws, size_t ws_bytes,
                        int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- K5a: MaxBin penalty tensor term ------------------------------------------------
 * Replaces the per-tensor part of SCCEMaxBin.compute_maxbin_penalty,
 *   CIFAR-10/custom_loss_terms/custom_components/custom_loss_functions.py:90-100,110:
 *   mb[g] = max_{i in g} |P_i| / s[g] ;  *term = mean_g mb[g].
 * `ties[g]` = number of elements attaining the maximum (TensorFlow's reduce_max gradient
 * splits evenly over ties).  Backward for upstream c = (*c_dev) * c_scale on `term`:
 *   dP_i = (|P_i|/s == mb[g]) ? sign(P_i) * c / (G * ties[g] * s[g]) : 0
 *   ds[g] = -c * mb[g] / (G * s[g])                                                   */
int lq_penalty_maxbin_fwd(const float* P, const float* s, float* mb, uint32_t* ties, float* term,
                          void* ws, size_t ws_bytes,
                          int64_t outer, int64_t G, int64_t inner, void* stream);
int lq_penalty_maxbin_bwd(const float* P, const float* s, const float* mb, const uint32_t* ties,
                          const float* c_dev, float c_scale, float* dP, float* ds,
                          int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- K5b: Difference penalty tensor term --------------------------------------------
 * Replaces the per-tensor part of SCCEDifference.compute_difference_penalty,
 *   custom_loss_functions.py:172-176:  *term = mean_i |P_i - P_i / s[g]|.
 * Backward, u = P - P/s, gi = sign(u) * c / N:
 *   dP_i = gi - gi / s[g] ;  ds[g] = sum_{i in g} gi * (P_i / s[g]) / s[g]           */
int lq_penalty_difference_fwd(const float* P, const float* s, float* term,
                              void* ws, size_t ws_bytes,
                              int64_t outer, int64_t G, int64_t inner, void* stream);
int lq_penalty_difference_bwd(const float* P, const float* s, const float* c_dev, float c_scale,
                              float* dP, float* ds, void* ws, size_t ws_bytes,
                              int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- K5c: Inverse penalty tensor term -----------------------------------------------
 * Replaces the per-tensor part of SCCEInverse.compute_inverse_penalty,
 *   custom_loss_functions.py:252-256:  *term = mean_g 1 / where(s[g]==0, eps_f32, s[g]).
 * Backward: ds[g] = s[g]==0 ? 0 : -c / (G * s[g]^2).                                  */
int lq_penalty_inverse_fwd(const float* s, float* term, int64_t G, void* stream);
int lq_penalty_inverse_bwd(const float* s, const float* c_dev, float c_scale, float* ds,
                           int64_t G, void* stream);

/* ---- K6: scale update ---------------------------------------------------------------
 * Adam step on a scale vector fused with the projection of MinValueConstraint
 *   custom_layers.py:35-46, attached at :158,170,182,191 with min_value = 100*eps_f32:
 *   s <- max(adam(s, ds), min_value).  `step` is the 1-based iteration count.  Hyper-parameters are
 *   doubles because Keras/torch form (1-beta) and the bias corrections from Python doubles before
 *   the fp32 tensor arithmetic; passing floats would change the last bits of every update.
 * lq_min_value_project is the bare constraint  w <- max(w, min_value)  (:42-43).      */
int lq_scale_adam_step(float* s, const float* ds, float* m, float* v, int64_t n,
                       double lr, double beta1, double beta2, double eps, int64_t step,
                       float min_value, int mode, void* stream);
/* Capture-safe form: the 1-based step is read from DEVICE memory at execution time (int64), so the launch can
 * live inside a hipGraph and be replayed while the caller increments the counter on the device.           */
int lq_scale_adam_step_dev(float* s, const float* ds, float* m, float* v, int64_t n,
                           double lr, double beta1, double beta2, double eps, const int64_t* step_dev,
                           float min_value, int mode, void* stream);
int lq_min_value_project(float* w, int64_t n, float min_value, void* stream);

/* ---- integer-view statistics (callbacks) ----------------------------------------------
 * max |floor(P/s)| over all elements sharing the index along `axis` of a tensor viewed
 * as (pre, n_axis, post) -- the reduce_max(abs(q), axis=1) of
 *   CIFAR-10/nested_quantization_layer/custom_components/custom_callbacks.py:98-99
 * is the complementary reduction: it keeps every axis but 1.  Here `keep_pre`/`keep_post`
 * select the kept extents: result[pre_i, post_j] = max over the middle axis.
 * The scale descriptor (outer,G,inner) is independent of the reduction geometry.      */
int lq_q_absmax_over_axis(const float* P, const float* s, float* result,
                          int64_t pre, int64_t n_axis, int64_t post,
                          int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- multi-tensor batch -----------------------------------------------------------------
 * A training step fake-quantises every custom layer's kernel and bias (4 / 12 / 40 tensors in the
 * reference's MNIST / CIFAR-10 / Imagenette models); one by one they are pure launch latency.
 * An lq_batch is a device-resident table of per-tensor tasks built ONCE from stable pointers:
 *   lq_batch_forward     = lq_fq_forward of every tensor in ONE launch                   (custom_layers.py:55-60)
 *   lq_batch_scale_grad  = lq_fq_scale_grad of every tensor with a finite lambda in TWO  (custom_layers.py:62-118)
 *                          launches; `dy` (optional, [n] device pointers, indexed like the descriptors)
 *                          overrides the descriptors' dy -- the upstream gradients move every step
 *   lq_batch_scale_adam  = lq_scale_adam_step(_dev) of every scale with Adam state in ONE launch
 *   lq_batch_scale_grad_step = the two above in the two launches of the first
 * q, out, max|q| and vote counts are bit-identical to the single-tensor entry points, and so is ds for lambda < 4e-4 (every
 * published threshold: the vote sums are exact in float64, any traversal and finalize order gives the same bits); for larger
 * lambda the float64 summation order of the traversal (tensors from 4 M elements) or of the finalize form may differ, which
 * reaches the fp32 result only when the mean sits on a rounding boundary.
 * lq_batch_create/destroy allocate/free the table (hipMalloc; not stream-ordered, never inside a capture);
 * the other calls only enqueue.  lambda = NaN marks an STE-only tensor (custom_loss_terms variant).        */
typedef struct lq_tensor_desc {
    const float* P;      /* parameter, dense fp32; (outer, G, inner) describes its elements in MEMORY order */
    const float* s;      /* scale [G]                                            */
    const float* dy;     /* default upstream gradient (may be NULL)              */
    float* out;          /* fake-quantised output (may be NULL next to out_oihw when lq_conv_tile_supported) */
    float* ds;           /* scale gradient [G] (required when lambda is finite)  */
    float* m;            /* Adam first moment of the scale [G] or NULL           */
    float* v;            /* Adam second moment of the scale [G] or NULL          */
    int64_t outer, G, inner;
    float lambda;        /* penalty_threshold, or NaN for STE-only               */
    float min_value;     /* MinValueConstraint bound used by lq_batch_scale_adam */
    /* conv kernels (HWIO, custom_layers.py:321): optional OIHW companions, see lq_fq_forward_oihw below; conv_co = 0: none */
    float* out_oihw;     /* second forward output in OIHW order, or NULL          */
    float* dp;           /* dP in HWIO order, written by lq_batch_scale_grad_oihw; conv_co = 0: dP of lq_batch_backward_clip, else unused */
    int64_t conv_hw, conv_ci, conv_co;   /* kh*kw, input channels, output channels  */
} lq_tensor_desc;

typedef struct lq_batch lq_batch;

int lq_batch_create(const lq_tensor_desc* descs, int n, lq_batch** out);
int lq_batch_destroy(lq_batch* batch);
size_t lq_batch_workspace_bytes(const lq_batch* batch);
int lq_batch_forward(const lq_batch* batch, void* stream);
int lq_batch_scale_grad(const lq_batch* batch, const float* const* dy, void* ws, size_t ws_bytes, void* stream);
/* As lq_batch_scale_grad, but for every tensor that has an OIHW companion dy[i] is in OIHW order (MIOpen's weight gradient
 * as it stands) and dP (= dy, custom_layers.py:118) is written in HWIO order to the descriptor's `dp` buffer.            */
int lq_batch_scale_grad_oihw(const lq_batch* batch, const float* const* dy, void* ws, size_t ws_bytes, void* stream);
int lq_batch_scale_adam(const lq_batch* batch, double lr, double beta1, double beta2, double eps, int64_t step,
                        const int64_t* step_dev, int mode, void* stream);
/* lq_batch_scale_grad (dy_oihw = 0) or lq_batch_scale_grad_oihw (dy_oihw = 1) followed by lq_batch_scale_adam, in the TWO
 * launches of the former: the finalize that emits ds[g] applies the Adam step and the MinValueConstraint to s[g] itself
 * (custom_layers.py:116, 158).  Same ds, m, v and s, bit for bit, as the two calls one after the other.  For the step in which
 * nothing reads or changes ds between its computation and the update (nested-quantization training without a loss term and
 * without an exchange of ds); every tensor of the batch must have lambda, ds and Adam state (LQ_EINVAL otherwise).          */
int lq_batch_scale_grad_step(const lq_batch* batch, const float* const* dy, int dy_oihw, void* ws, size_t ws_bytes,
                             double lr, double beta1, double beta2, double eps, int64_t step, const int64_t* step_dev,
                             int mode, void* stream);

/* Custom-loss-term gradients of every tensor of the batch in 2-4 launches
 *   (CIFAR-10/custom_loss_terms/custom_components/custom_loss_functions.py:75-116, 161-195, 240-275).
 * The total loss is mean(SCCE) + gamma * penalty (:58), so the upstream coefficient of tensor i's term is the HOST
 * constant coeff[i] = gamma * numel_i / normalizer -- no autograd node per tensor is needed:
 *   grad[i][...] += coeff[i] * d term_i / d P_i     (MaxBin, Difference; accumulated into the existing gradient)
 *   ds_i[...]     = coeff[i] * d term_i / d s_i     (written to the descriptors' ds buffers)
 * coeff: host array [n]; grad: host array [n] of device pointers (unused for LQ_PENALTY_INVERSE).
 * kind | LQ_PENALTY_ACCUMULATE_DS: ds_i[...] += ... instead of = (a nested-quantization layer trained WITH a loss term:
 * the penalty's scale gradient is added to the hand-written one already in the buffer; no reference call site).     */
typedef enum lq_penalty_kind { LQ_PENALTY_MAXBIN = 0, LQ_PENALTY_DIFFERENCE = 1, LQ_PENALTY_INVERSE = 2 } lq_penalty_kind;
#define LQ_PENALTY_ACCUMULATE_DS 0x100
int lq_batch_penalty_grads(const lq_batch* batch, int kind, const float* coeff, float* const* grad,
                           void* ws, size_t ws_bytes, void* stream);

/* lq_fq_scale_grad_ste of every tensor of the batch that has a ds buffer, whatever its lambda (NaN included), in TWO launches
 * (traversal + finalize).  dy: optional host array [n] of device pointers, indexed like the descriptors, in the memory order of
 * P; overrides the descriptors' dy.  grad_scale: host float[n], or NULL = 1 for every tensor.  Same definition and the same
 * "no bit-identity across traversals" note as the single-tensor call.  ws as for lq_batch_penalty_grads; only enqueues.
 * To add a loss term's scale gradient, call lq_batch_penalty_grads[_values] with LQ_PENALTY_ACCUMULATE_DS afterwards.     */
int lq_batch_scale_grad_ste(const lq_batch* batch, const float* const* dy, const float* grad_scale,
                            void* ws, size_t ws_bytes, void* stream);

/* Clipped b-bit tensors in the batch (opt-in): lq_fq_forward_clip_r / lq_fq_backward_clip_r of every tensor, each with its own
 * integer range, one rounding per batch.
 * lq_batch_set_clip: HOST call (allocates and uploads: never inside a capture; a repeated call replaces the ranges).  qmin / qmax:
 *   host int32[n], indexed like the descriptors, each pair under the single-tensor rule (qmin <= qmax, |q| <= 2^24); rounding:
 *   LQ_ROUND_FLOOR or LQ_ROUND_NEAREST_EVEN; n must be the batch's tensor count.  Every tensor needs conv_co == 0 (no OIHW
 *   companions: store conv kernels in the order the convolution consumes) and a `dp` buffer of the parameter's size, which
 *   receives dP.  The clipped pair runs on task tables of its own (generic traversal bodies); a tensor whose traversal uses 16-byte
 *   accesses and whose `dp` is not 16-byte aligned is refused here with LQ_EALIGN.  lq_batch_workspace_bytes covers the pair
 *   afterwards (query it after this call).
 * lq_batch_forward_clip: ONE launch, out_i = clamp(rnd(P_i / s_i), qmin_i, qmax_i) * s_i, bit-identical to the single-tensor call.
 * lq_batch_backward_clip: TWO launches (traversal + finalize).  dy as for lq_batch_scale_grad_ste (NULL entry: LQ_EINVAL; 4-byte
 *   alignment; 16-byte alignment where the tensor's traversal needs it: LQ_EALIGN).  Writes dP_i = inside ? dy_i : 0 to `dp`, the
 *   exact per-group clip counts to batch-owned memory (lq_batch_clip_counts) and -- grad_scale != NULL, host float[n] --
 *   ds_i[g] = (float)(grad_scale[i] * sum dy * r) to the descriptors' ds (every tensor then needs one).  grad_scale == NULL is
 *   "mask only": ds is not written at all.  dP and the counts are bit-identical to the single-tensor call; ds carries its "no
 *   bit-identity across traversals" note.  Moves 12 bytes per element (P, dy, dP).
 * Both return LQ_EINVAL on a batch without ranges; they only enqueue, never allocate, and can be captured.
 * lq_batch_clip_counts: device address of tensor `tensor`'s clip counts (uint32[groups], rewritten by every backward).     */
int lq_batch_set_clip(lq_batch* batch, const int32_t* qmin, const int32_t* qmax, int n, int rounding);
int lq_batch_forward_clip(const lq_batch* batch, void* stream);
int lq_batch_backward_clip(const lq_batch* batch, const float* const* dy, const float* grad_scale, void* ws, size_t ws_bytes,
                           void* stream);
int lq_batch_clip_counts(const lq_batch* batch, int tensor, const uint32_t** dev, int64_t* groups);

/* ---- group-wise tensors in a batch: ONE launch per pass ----
 * lq_fq_forward_group / lq_fq_backward_group of up to 256 tensors.  Per tensor the definition is exactly the one stated at
 * lq_fq_forward_group above; each tensor has its own range and geometry, the batch has one rounding.  A 1-D parameter with a
 * scalar scale (a bias) is the geometry R = 1, C = numel, axis = 1, gs = numel: one group.
 * lq_group_batch_create / _destroy: HOST calls (allocate and upload: never inside a capture).  create validates every descriptor
 *   before its first HIP call: n outside 1 .. 256, a NULL P / s / out / dp, a bad axis, gs < 1, a non-positive extent,
 *   R * C >= 2^31, qmin > qmax, a bound outside +-2^24 and a bad rounding return LQ_EINVAL, a base that is not 4-byte aligned
 *   returns LQ_EALIGN; the message names the tensor.  Each tensor takes the form (axis, 16-byte or 4-byte accesses, lanes per
 *   group) that the single-tensor call takes for the same geometry and alignment: the forward by P and out, the backward by P and dp.
 * lq_group_batch_forward: ONE launch; out_i is bit-identical to lq_fq_forward_group on the same buffers.
 * lq_group_batch_backward: ONE launch.  dy: host array [n] of device pointers, indexed like the descriptors (a NULL entry:
 *   LQ_EINVAL; an entry off the 16-byte grid for a tensor whose backward uses 16-byte accesses: LQ_EALIGN, before any launch).
 *   grad_scale: host float[n], or NULL for "mask only": then no ds is written at all; when given, every tensor needs a ds.
 *   dp_i is written for every tensor, and the exact uint32 clip counts, in the scale's shape, go to batch-owned memory that every
 *   backward rewrites (lq_group_batch_clip_counts gives the address and the element count).  dP, the counts AND ds are
 *   bit-identical to lq_fq_backward_group on the same buffers with the same grad_scale: a block of the batch runs the same code
 *   on the same unit of work, so every sum has the single-tensor call's order.
 * lq_group_batch_workspace_bytes: scratch the backward needs; 0 for every shipped form, and `ws` may then be NULL.  The memory
 *   contract of lq_group_workspace_bytes applies.
 * Both passes only enqueue, never allocate, and can be captured.  The library reads no environment.  */
typedef struct lq_group_desc {
    const float* P;      /* parameter in MEMORY order, matrix [R][C], C contiguous           */
    const float* s;      /* scale, [nb][C] (axis 0) or [R][nb] (axis 1), as lq_fq_*_group    */
    float* out;          /* forward output, required                                         */
    float* dp;           /* masked dP of the backward, required                              */
    float* ds;           /* scale gradient in the scale's shape; may be NULL (mask only)     */
    int64_t R, C, gs;
    int32_t axis, qmin, qmax;
} lq_group_desc;
typedef struct lq_group_batch lq_group_batch;
int lq_group_batch_create(const lq_group_desc* descs, int n, int rounding, lq_group_batch** out);
int lq_group_batch_destroy(lq_group_batch* b);
size_t lq_group_batch_workspace_bytes(const lq_group_batch* b);
int lq_group_batch_forward(const lq_group_batch* b, void* stream);
int lq_group_batch_backward(const lq_group_batch* b, const float* const* dy, const float* grad_scale,
                            void* ws, size_t ws_bytes, void* stream);
int lq_group_batch_clip_counts(const lq_group_batch* b, int tensor, const uint32_t** dev, int64_t* groups);

/* ---- group-wise tensors with a learned offset in the batch ----
 * lq_group_batch_create_affine builds the same kind of batch from the same descriptors plus, per tensor, an optional offset:
 * a tensor with b != NULL is lq_fq_forward_group_affine / lq_fq_backward_group_affine (the definition stated in "asymmetric
 * group-wise scales" above), a tensor with b == NULL is lq_fq_forward_group / lq_fq_backward_group as in a batch without offsets
 * (a bias of an asymmetric model: it keeps the symmetric bits, the sign of -0.0 included).  The handle is an lq_group_batch:
 * _forward, _backward, _clip_counts, _workspace_bytes (still 0: no workspace is used) and _destroy serve it unchanged, ONE launch
 * per pass.  offs == NULL, or no tensor with a b, is exactly lq_group_batch_create: the same tables and the same kernels.
 * out, dP, the clip counts, ds AND db of every tensor are bit-identical to the single-tensor call of its kind on the same buffers
 * with the same grad_scale and offset_grad_scale: a block runs the same code on the same unit of work.
 * offset_grad_scale (kb of the definition) is FIXED at create time and lives in the device-resident task table: the kernel's
 * argument block already carries one pointer and one coefficient per tensor for dy and grad_scale, and a second coefficient
 * array would pass its 4 KB limit.  A layer's kb is a function of its geometry and range, so nothing is lost.
 * Backward: grad_scale == NULL stays "mask only": neither ds nor db is written.  With grad_scale every tensor needs a ds, and db
 * is written where it was given.
 * Refused before the first HIP call, in addition to everything lq_group_batch_create refuses: a db without a b and an
 * offset_grad_scale that is not finite on a tensor with a b (LQ_EINVAL); b or db off the 4-byte grid (LQ_EALIGN; they need no
 * more, as in the single-tensor call).  The message names the tensor.
 * create is a HOST call (allocates and uploads: never inside a capture); both passes only enqueue and can be captured.  */
typedef struct lq_group_offset {
    const float* b;            /* offset, the scale's shape; NULL: this tensor is symmetric          */
    float* db;                 /* offset gradient, the scale's shape; may be NULL (not written)      */
    float offset_grad_scale;   /* kb of lq_fq_backward_group_affine, fixed for the batch's life      */
} lq_group_offset;
int lq_group_batch_create_affine(const lq_group_desc* descs, const lq_group_offset* offs /* [n] or NULL */,
                                 int n, int rounding, lq_group_batch** out);

/* ---- microscaling (MX) tensors in the batch ----
 * lq_group_batch_create_mx builds the same kind of batch from the same descriptors plus, per tensor, an element format and a
 * scale format: tensor i is lq_fq_forward_mx / lq_fq_backward_mx (the definition stated in "OCP microscaling (MX) element
 * formats" above) with fmts[i].  The format lives in the device-resident task table, per tensor: one batch may hold tensors of
 * different element formats and scale formats.  qmin / qmax of a descriptor are not read (the range is the format's +-max) and
 * there is no rounding argument (a minifloat grid has one rounding, ties to even).  A 1-D parameter with a scalar scale (a bias)
 * is the one-group line R = 1, C = numel, axis = 1, gs = numel, as in lq_fq_*_mx.
 * The handle is an lq_group_batch: _forward, _backward, _clip_counts (the counts are the saturation counts), _workspace_bytes
 * (still 0: no workspace is used) and _destroy serve it unchanged, ONE launch per pass.  Each tensor takes the form the
 * single-tensor MX call takes for the same geometry and alignment.
 * out, dP, the saturation counts AND ds of every tensor are bit-identical to lq_fq_forward_mx / lq_fq_backward_mx on the same
 * buffers with the same grad_scale: a block runs the same code on the same unit of work.  No encodings are written (the batch
 * has no `code` output).
 * Backward: the dy rules of lq_group_batch_backward hold (a NULL entry: LQ_EINVAL; an entry off the 16-byte grid for a tensor
 * whose backward uses 16-byte accesses: LQ_EALIGN, before any launch); grad_scale == NULL stays "mask only": no ds is written.
 * Refused before the first HIP call, in addition to everything lq_group_batch_create refuses (its range checks aside): a NULL
 * fmts, an unknown format or scale_format (LQ_EINVAL).  The message names the tensor.
 * create is a HOST call (allocates and uploads: never inside a capture); both passes only enqueue and can be captured.  */
typedef struct lq_group_mx_format {
    int32_t format;        /* lq_elem_format  */
    int32_t scale_format;  /* lq_scale_format */
} lq_group_mx_format;
int lq_group_batch_create_mx(const lq_group_desc* descs, const lq_group_mx_format* fmts /* [n] */, int n, lq_group_batch** out);

/* VALUE of the custom-loss-term penalty for the whole batch (compute_{maxbin,difference,inverse}_penalty,
 *   custom_loss_functions.py:75-116, 161-195, 240-275), the number compute_total_loss adds to the cross-entropy (:47-58).
 * Per-tensor term t_i as in lq_penalty_{maxbin,difference,inverse}_fwd; the model penalty in the reference's order (:102-116):
 *   per layer  t_k * dim_k (+ t_b * dim_b),  running fp32 sum over the layers in descriptor order,  / sum(dims).
 * dims: host float[n], the element counts (:102-108); layer_start: host uint8[n], 1 where tensor i opens a new layer (kernel and
 * bias of one layer are paired as the reference pairs them).  terms_dev: device float[n]; penalty_dev: one device float.
 * lq_batch_penalty_values: values only -- MaxBin 4 launches, Difference 4 (a forward traversal of the batch, its finalize, terms,
 *   combine), Inverse 2 (the two small ones: terms, combine).
 * lq_batch_penalty_grads_values: lq_batch_penalty_grads (same arguments, LQ_PENALTY_ACCUMULATE_DS included; bit-identical
 *   gradient outputs) and the values, without reading any parameter more often than lq_batch_penalty_grads does.  MaxBin and
 *   Inverse reduce what the gradient launches left behind (mb[g], s[g]) in the two small launches.  Difference: the backward
 *   traversal carries sum |P - P/s| in a second accumulator next to the scale-gradient sum (the same f64 accumulation and merge
 *   order for ds: the same bits), one finalize launch emits ds and the groups' mean |u|, then the two small launches -- 4
 *   launches instead of lq_batch_penalty_grads' 2.
 * All reductions are two-stage and ordered (no float atomics): run-to-run bit-stable.  ws as for lq_batch_penalty_grads
 * (lq_batch_workspace_bytes, which covers the second partial slice; not needed for LQ_PENALTY_INVERSE).  Nothing allocates;
 * the calls only enqueue.                                                                                                */
int lq_batch_penalty_values(const lq_batch* batch, int kind, const float* dims, const uint8_t* layer_start,
                            float* terms_dev, float* penalty_dev, void* ws, size_t ws_bytes, void* stream);
int lq_batch_penalty_grads_values(const lq_batch* batch, int kind, const float* coeff, float* const* grad,
                                  const float* dims, const uint8_t* layer_start, float* terms_dev, float* penalty_dev,
                                  void* ws, size_t ws_bytes, void* stream);

/* One row of the reference's per-step logs custom_losses/{total,scce,<term>}_loss.log (custom_loss_functions.py:58-71),
 * appended ON THE DEVICE in one tiny launch: no device->host synchronisation per step, and -- the cursor lives in device
 * memory -- the launch can be captured into a hipGraph once and replayed.
 *   row = { scce + rate * penalty, scce, rate * penalty }   (fp32, in this order of operations, :58)
 * is written to rows_dev[3 * cursor_dev[0]] and cursor_dev[0] (int64) is incremented; when cursor_dev[0] == capacity nothing
 * is written to rows_dev and cursor_dev[1] (dropped rows) is incremented instead.  cursor_dev: two int64, 8-byte aligned.
 * last_dev (optional, device float[3]): always receives the row, whether it was logged or dropped.                      */
int lq_loss_log_append(const float* scce_dev, const float* penalty_dev, float rate, float* rows_dev, int64_t capacity,
                       int64_t* cursor_dev, float* last_dev, void* stream);

/* ---- multi-tensor Adam for the ordinary parameters (SURVEY f-4) -------------------------------------------
 * The reference trains everything with Keras 2.11 Adam(learning_rate=1e-4)
 *   CIFAR-10/nested_quantization_layer/experiment.py:435-443.
 * An lq_adam_set holds (w, m, v, n[, min_value]) of up to 256 tensors; lq_adam_set_step applies one Adam step to all of
 * them in ONE launch with the arithmetic of lq_scale_adam_step (mode LQ_ADAM_KERAS / LQ_ADAM_TORCH); `grads` is a host
 * array of device pointers (they move every step; a NULL entry skips that tensor), `step_dev` (optional) a device int64 for hipGraph capture.        */
typedef struct lq_adam_set lq_adam_set;
int lq_adam_set_create(float* const* w, float* const* m, float* const* v, const int64_t* n, const float* min_value, int count,
                       lq_adam_set** out);
int lq_adam_set_destroy(lq_adam_set* set);
int lq_adam_set_step(const lq_adam_set* set, const float* const* grads, double lr, double beta1, double beta2, double eps,
                     int64_t step, const int64_t* step_dev, int mode, void* stream);

/* ---- integer-view range and histogram (tracking callbacks) -----------------------------------------
 * The reference's callbacks pull floor(P/s) to the host and run np.unique on it every epoch
 *   CIFAR-10/nested_quantization_layer/custom_components/custom_callbacks.py:85-96, 131-207.
 * lq_q_minmax: minmax_dev[0] = min q, minmax_dev[1] = max q over the tensor (int32; the caller initialises the
 *   pair to {INT32_MAX, INT32_MIN}; NaN/Inf/out-of-int32 quotients are skipped).
 * lq_q_histogram: bins_dev[q - qmin] += count for qmin <= q < qmin + nbins (uint32 bins, zeroed by the caller).
 *   #unique = number of non-zero bins; (value, count) pairs = the non-zero bins.  Integer atomics: exact.      */
int lq_q_minmax(const float* P, const float* s, int32_t* minmax_dev, int64_t outer, int64_t G, int64_t inner, void* stream);
int lq_q_histogram(const float* P, const float* s, int32_t qmin, int64_t nbins, uint32_t* bins_dev,
                   int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- bit-packed integer view: lossless export and exact restore -----------------------------------------
 * The reference's export casts floor(P/s) to int8 (CIFAR-10/nested_quantization_layer/utils/log_scripts.py:61-97,
 * lossy once |q| > 127); these store q = floor(P/s) (custom_layers.py:55-60, K1's division) without loss.
 * Stream format: code c_i = q_i - qmin of `bits` (0..32) bits, element i at stream bits [i*bits, i*bits + bits),
 * stream bit j = bit (j mod 32) of words[j/32], ceil(numel*bits/32) little-endian uint32 words, pad bits 0.
 * Elements in the contiguous order of P; at most 2^31 of them.  bits = 0: no words (`words` may be NULL).
 * lq_q_pack: writes the words; ADDS to *bad_dev (uint64 on the device, zeroed by the caller) the number of elements
 *   whose quotient is NaN, +-Inf, outside what lq_q_minmax counts or outside [qmin, qmin + 2^bits - 1] (stored as 0).
 *   P must be 16-byte aligned.
 * lq_q_unpack: any of out (float, = lq_fq_forward's out bit for bit except that -0 comes back as +0), q (int32) and
 *   p_restore (float whose K1 quotient floors to q: (q + 1/2) * s) may be NULL, not all three; each 16-byte aligned.
 *   With p_restore, every value is divided back with K1's division and the misses are ADDED to *bad_dev (required then;
 *   0 for |q| < 2^22, the caller must refuse the restore otherwise).                                            */
int lq_q_pack(const float* P, const float* s, int32_t qmin, int bits, uint32_t* words, uint64_t* bad_dev,
              int64_t outer, int64_t G, int64_t inner, void* stream);
int lq_q_unpack(const uint32_t* words, int32_t qmin, int bits, const float* s, float* out, int32_t* q, float* p_restore,
                uint64_t* bad_dev, int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- device self-test -------------------------------------------------------------------
 * Compares the kernels' in-window ratio division (rcp + Newton + fma chain, see lq_kernels.hip window_div)
 * with the IEEE `/` on blocks*256*pairs_per_thread pseudo-random operand pairs in [2^-40, 2^40]; ADDS the
 * number of bit mismatches to *mismatches_dev (uint64 on the device, zeroed by the caller). Expected: 0.   */
int lq_selftest_ratio_division(uint64_t seed, uint32_t blocks, uint32_t pairs_per_thread, uint64_t* mismatches_dev,
                               void* stream);
/* The same for the uniform-divisor division of the streaming kernels (r = RN(1/s) + two fma refinements, see
 * lq_math.hpp): random s in [2^-40, 2^40], random x in [2^-80, 2^81), both signs.  Expected: 0 mismatches.      */
int lq_selftest_uniform_division(uint64_t seed, uint32_t blocks, uint32_t pairs_per_thread, uint64_t* mismatches_dev,
                                 void* stream);

/* ---- conv kernels: HWIO parameter, OIHW consumer ---------------------------------------------------------------
 * The reference keeps conv kernels in HWIO (custom_layers.py:321) and `orientation` names HWIO axes; MIOpen consumes OIHW.
 * Instead of a separate transpose launch after K1 and another before K2 (what `qk.permute(3, 2, 0, 1)` costs in torch),
 *   lq_fq_forward_oihw     writes out (HWIO, as lq_fq_forward) AND out_oihw[(o*ci + c)*hw + h] = out[(h*ci + c)*co + o];
 *   lq_fq_scale_grad_oihw  takes dy in OIHW order, computes ds exactly as lq_fq_scale_grad would on the un-permuted dy
 *                          (same traversal, same summation order: bit-identical) and writes dP = dy in HWIO order.
 * hw = kh*kw; hw*ci*co must equal outer*G*inner.  Weight-sized tensors (below 2^32 elements).
 * Kernels of at most 9 taps with co % 4 == 0 and one of the reference's four orientations run as LDS tiles (whole 128-byte
 * lines on both the HWIO and the OIHW side); lq_fq_scale_grad_oihw then needs lq_conv_workspace_bytes() of scratch.
 * When the OIHW tensor is the only consumer (tf.nn.conv2d(x, qk) at custom_layers.py:340-348 is the kernel's ONLY use in a
 * training step), `out` may be NULL for kernels the tile path takes -- lq_conv_tile_supported() == 1 and P 16-byte aligned:
 * the forward then moves 8 bytes per element instead of 12.                                                             */
int lq_conv_tile_supported(int64_t hw, int64_t ci, int64_t co, int64_t outer, int64_t G, int64_t inner);
size_t lq_conv_workspace_bytes(int64_t hw, int64_t ci, int64_t co, int64_t outer, int64_t G, int64_t inner);
int lq_fq_forward_oihw(const float* P, const float* s, float* out, float* out_oihw, int64_t hw, int64_t ci, int64_t co,
                       int64_t outer, int64_t G, int64_t inner, void* stream);
int lq_fq_scale_grad_oihw(const float* P, const float* s, const float* dy_oihw, float lambda, float* ds, float* dP,
                          void* ws, size_t ws_bytes, int64_t hw, int64_t ci, int64_t co,
                          int64_t outer, int64_t G, int64_t inner, void* stream);

/* ---- profiling hook ----------------------------------------------------------------------
 * lq_profile_events(start, stop): while set (both hipEvent_t, created with timing enabled), every row-stream traversal
 * kernel this host thread launches (K1 / K2 / K4 of streaming-size tensors with rows >= 1024 elements: the BENCH path) is
 * launched through hipExtLaunchKernelGGL with these events, which then carry the kernel's OWN begin and end timestamps --
 * hipEventElapsedTime(start, stop) is the kernel duration rocprofv3 reports, without the cost of bracketing event records
 * and without the finalize launch of the two-launch calls.  lq_profile_events(NULL, NULL) switches it off.            */
int lq_profile_events(void* start, void* stop);

#ifdef __cplusplus
}
#endif
#endif /* LQ_HIP_H_ */
