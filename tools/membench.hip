// tools/membench.hip -- development microbenchmark (not part of the product): what can two/one
// read streams and read+write streams sustain on this MI355X with the traversal geometries the
// library uses?  Build: hipcc -O3 --offload-arch=gfx950 -o membench tools/membench.hip
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

constexpr int kBlock = 256;

typedef float v4f __attribute__((ext_vector_type(4)));
template <int NT>
__device__ __forceinline__ float4 ld(const float4* p) {
    if (NT) { v4f v = __builtin_nontemporal_load((const v4f*)p); return make_float4(v.x, v.y, v.z, v.w); }
    return *p;
}
template <int NT>
__device__ __forceinline__ void st(float4* p, float4 v) {
    if (NT) { v4f t = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t, (v4f*)p); } else *p = v;
}

// MODE 0: read A            (sum)
// MODE 1: read A, read B    (sum)
// MODE 2: read A, write C   (copy*2)
// MODE 3: read A, read B, write C
template <int MODE, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_chunk(const float* A, const float* B, float* C, float* sink, int CH) {
    const int64_t base = (int64_t)blockIdx.x * CH;
    const float4* A4 = (const float4*)(A + base);
    const float4* B4 = (const float4*)(B + base);
    float4* C4 = (float4*)(C + base);
    const int n4 = CH / 4;
    float acc = 0.f;
    for (int j0 = 0; j0 < n4; j0 += U * kBlock) {
        float4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int j = j0 + u * kBlock + threadIdx.x;
            a[u] = ld<NT>(A4 + j);
            if (MODE == 1 || MODE == 3) b[u] = ld<NT>(B4 + j);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int j = j0 + u * kBlock + threadIdx.x;
            float4 r = a[u];
            if (MODE == 1 || MODE == 3) { r.x += b[u].x; r.y += b[u].y; r.z += b[u].z; r.w += b[u].w; }
            if (MODE >= 2) st<NT>(C4 + j, r); else acc += r.x + r.y + r.z + r.w;
        }
    }
    if (MODE < 2 && acc == 123.456f) sink[0] = acc;
}

// persistent grid-stride over chunks
template <int MODE, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_persist(const float* A, const float* B, float* C, float* sink, int CH, int nchunks) {
    float acc = 0.f;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t base = (int64_t)c * CH;
        const float4* A4 = (const float4*)(A + base);
        const float4* B4 = (const float4*)(B + base);
        float4* C4 = (float4*)(C + base);
        const int n4 = CH / 4;
        for (int j0 = 0; j0 < n4; j0 += U * kBlock) {
            float4 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int j = j0 + u * kBlock + threadIdx.x;
                a[u] = ld<NT>(A4 + j);
                if (MODE == 1 || MODE == 3) b[u] = ld<NT>(B4 + j);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int j = j0 + u * kBlock + threadIdx.x;
                float4 r = a[u];
                if (MODE == 1 || MODE == 3) { r.x += b[u].x; r.y += b[u].y; r.z += b[u].z; r.w += b[u].w; }
                if (MODE >= 2) st<NT>(C4 + j, r); else acc += r.x + r.y + r.z + r.w;
            }
        }
    }
    if (MODE < 2 && acc == 123.456f) sink[0] = acc;
}

// persistent, software-pipelined: prefetch chunk k+1 while processing chunk k (U float4 per thread per stream)
template <int MODE, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_pipe(const float* A, const float* B, float* C, float* sink, int nchunks) {
    constexpr int CH = U * kBlock * 4;
    float acc = 0.f;
    int c = blockIdx.x;
    if (c >= nchunks) return;
    float4 a[U], b[U];
    {
        const float4* A4 = (const float4*)(A + (int64_t)c * CH);
        const float4* B4 = (const float4*)(B + (int64_t)c * CH);
#pragma unroll
        for (int u = 0; u < U; ++u) { a[u] = ld<NT>(A4 + u * kBlock + threadIdx.x); if (MODE == 1 || MODE == 3) b[u] = ld<NT>(B4 + u * kBlock + threadIdx.x); }
    }
    for (;;) {
        const int cn = c + gridDim.x;
        float4 an[U], bn[U];
        if (cn < nchunks) {
            const float4* A4 = (const float4*)(A + (int64_t)cn * CH);
            const float4* B4 = (const float4*)(B + (int64_t)cn * CH);
#pragma unroll
            for (int u = 0; u < U; ++u) { an[u] = ld<NT>(A4 + u * kBlock + threadIdx.x); if (MODE == 1 || MODE == 3) bn[u] = ld<NT>(B4 + u * kBlock + threadIdx.x); }
        }
        float4* C4 = (float4*)(C + (int64_t)c * CH);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float4 r = a[u];
            if (MODE == 1 || MODE == 3) { r.x += b[u].x; r.y += b[u].y; r.z += b[u].z; r.w += b[u].w; }
            if (MODE >= 2) st<NT>(C4 + u * kBlock + threadIdx.x, r); else acc += r.x + r.y + r.z + r.w;
        }
        if (cn >= nchunks) break;
#pragma unroll
        for (int u = 0; u < U; ++u) { a[u] = an[u]; b[u] = bn[u]; }
        c = cn;
    }
    if (MODE < 2 && acc == 123.456f) sink[0] = acc;
}

template <int MODE, int BS, int NT>
__global__ __launch_bounds__(BS) void k_one(const float* A, const float* B, float* C, float* sink) {
    const int64_t j = (int64_t)blockIdx.x * BS + threadIdx.x;
    float4 a = ld<NT>((const float4*)A + j), b;
    if (MODE == 1 || MODE == 3) { b = ld<NT>((const float4*)B + j); a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
    if (MODE >= 2) st<NT>((float4*)C + j, a);
    else if (a.x + a.y + a.z + a.w == 123.456f) sink[0] = a.x;
}

// XCD-aware variant of k_one: workgroup w runs on XCD w % 8 (round-robin dispatch); XMAP 1 gives every XCD one contiguous
// eighth of the buffer (logical block = (w % 8) * (nb / 8) + w / 8) instead of every eighth block.
template <int MODE, int BS, int NT, int XMAP>
__global__ __launch_bounds__(BS) void k_one_x(const float* A, const float* B, float* C, float* sink, int nb) {
    int w = blockIdx.x;
    if (XMAP) { const int per = nb >> 3; w = (w & 7) * per + (w >> 3); }
    const int64_t j = (int64_t)w * BS + threadIdx.x;
    float4 a = ld<NT>((const float4*)A + j), b;
    if (MODE == 1 || MODE == 3) { b = ld<NT>((const float4*)B + j); a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
    if (MODE >= 2) st<NT>((float4*)C + j, a);
    else if (a.x + a.y + a.z + a.w == 123.456f) sink[0] = a.x;
}

// Cache-policy probe (gfx950 global_load/global_store modifiers sc0 / sc1 / nt), one float4 per thread per stream.
#define LQ_POL_KERNEL(NAME, LDPOL, STPOL)                                                                              \
    __global__ __launch_bounds__(512) void NAME(const float* A, const float* B, float* C, float* sink, int mode) {    \
        const int64_t j = (int64_t)blockIdx.x * 512 + threadIdx.x;                                                     \
        const float4* pa = (const float4*)A + j;                                                                       \
        const float4* pb = (const float4*)B + j;                                                                       \
        float4* pc = (float4*)C + j;                                                                                   \
        v4f a, b;                                                                                                      \
        if (mode == 1) {                                                                                               \
            asm volatile("global_load_dwordx4 %0, %2, off " LDPOL "\n\tglobal_load_dwordx4 %1, %3, off " LDPOL          \
                         "\n\ts_waitcnt vmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(pa), "v"(pb) : "memory");                 \
            if (a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w == 123.456f) sink[0] = a.x;                              \
        } else {                                                                                                       \
            asm volatile("global_load_dwordx4 %0, %1, off " LDPOL "\n\ts_waitcnt vmcnt(0)" : "=&v"(a) : "v"(pa) : "memory"); \
            a.x += 1.0f;                                                                                               \
            asm volatile("global_store_dwordx4 %0, %1, off " STPOL : : "v"(pc), "v"(a) : "memory");                    \
        }                                                                                                              \
    }
LQ_POL_KERNEL(k_pol_plain, "", "")
LQ_POL_KERNEL(k_pol_nt, "nt", "nt")
LQ_POL_KERNEL(k_pol_sc1nt, "sc1 nt", "sc1 nt")
LQ_POL_KERNEL(k_pol_sc0sc1nt, "sc0 sc1 nt", "sc0 sc1 nt")
LQ_POL_KERNEL(k_pol_sc1, "sc1", "sc1")
LQ_POL_KERNEL(k_pol_sc0sc1, "sc0 sc1", "sc0 sc1")
LQ_POL_KERNEL(k_pol_ldnt_stsc, "nt", "sc0 sc1 nt")
LQ_POL_KERNEL(k_pol_ldsc_stnt, "sc0 sc1 nt", "nt")

// Survival probe: a store-only stream with an explicit policy (vector stores), and the same behind a nontemporal read (K1's mix).
#define LQ_ST_KERNEL(NAME, STPOL)                                                                                      \
    __global__ __launch_bounds__(512) void NAME(const float* A, float* C, int rd) {                                   \
        const int64_t j = (int64_t)blockIdx.x * 512 + threadIdx.x;                                                     \
        float4* pc = (float4*)C + j;                                                                                   \
        v4f a = {1.f, 2.f, 3.f, 4.f};                                                                                  \
        if (rd) a = __builtin_nontemporal_load((const v4f*)A + j);                                                     \
        asm volatile("global_store_dwordx4 %0, %1, off " STPOL : : "v"(pc), "v"(a) : "memory");                        \
    }
LQ_ST_KERNEL(k_st_plain, "")
LQ_ST_KERNEL(k_st_nt, "nt")
LQ_ST_KERNEL(k_st_sc1nt, "sc1 nt")
LQ_ST_KERNEL(k_st_sc0sc1nt, "sc0 sc1 nt")
LQ_ST_KERNEL(k_st_sc1, "sc1")
LQ_ST_KERNEL(k_st_sc0sc1, "sc0 sc1")

// the re-read of the probe: the table with the default policy NEXT TO a cold nontemporal stream of the same size, as K2 reads
// P next to dy -- alone, a 62 MB read runs at the same 5.2 TB/s from the cache and from HBM and tells nothing
__global__ __launch_bounds__(512) void k_table2(const float* A, const float* B, float* sink) {
    const int64_t j = (int64_t)blockIdx.x * 512 + threadIdx.x;
    const float4 a = *((const float4*)A + j);
    const v4f b = __builtin_nontemporal_load((const v4f*)B + j);
    if (a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w == 123.456f) sink[0] = a.x;
}

// Cache-policy MIX rows (`membench mix`; DESIGN.md section 3 "Cache-policy mix"): the two BENCH access shapes with a
// block-uniform predicate per stream that picks the stream's policy -- loads: default (picked) or nt; stores: nt (picked) or
// sc1 nt.  A predicate picks the blocks from `from` on (a contiguous tail) or those whose bit is set in an 8-bit mask indexed
// by (block >> shift) & 7 (interleaved: shift 0 = single blocks, which also pins the picked blocks to fixed XCDs of the
// round-robin dispatch; shift 3 = runs of 8 consecutive blocks, spread over every XCD).
struct Pick { int from; unsigned mask; int shift; };
__device__ __forceinline__ bool picked(const Pick q, int b) { return b >= q.from || ((q.mask >> ((b >> q.shift) & 7)) & 1u); }
#define LQ_MIX_LD(DST, PTR, KEEP)                                                                                      \
    if (KEEP) asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(DST) : "v"(PTR) : "memory");                      \
    else asm volatile("global_load_dwordx4 %0, %1, off nt" : "=&v"(DST) : "v"(PTR) : "memory");
// read + write: 512 threads, one float4 per thread (K1's shape)
__global__ __launch_bounds__(512) void k_mix_rw(const float* A, float* C, float* sink, Pick ld, Pick stp) {
    const int b = blockIdx.x;
    const int64_t j = (int64_t)b * 512 + threadIdx.x;
    const float4* pa = (const float4*)A + j;
    float4* pc = (float4*)C + j;
    const bool keep = picked(ld, b), snt = picked(stp, b);
    v4f a;
    LQ_MIX_LD(a, pa, keep)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a));
    a.x += 1.0f;
    if (snt) asm volatile("global_store_dwordx4 %0, %1, off nt" : : "v"(pc), "v"(a) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" : : "v"(pc), "v"(a) : "memory");
}
// two reads: 512 threads, two float4 per thread and stream (K2's unit of 4096 elements)
__global__ __launch_bounds__(512) void k_mix_r2(const float* A, const float* B, float* sink, Pick pa_, Pick pb_) {
    const int b = blockIdx.x;
    const int64_t j = (int64_t)b * 1024 + threadIdx.x;
    const float4 *pa0 = (const float4*)A + j, *pa1 = pa0 + 512, *pb0 = (const float4*)B + j, *pb1 = pb0 + 512;
    const bool ka = picked(pa_, b), kb = picked(pb_, b);
    v4f a0, a1, b0, b1;
    LQ_MIX_LD(a0, pa0, ka)
    LQ_MIX_LD(b0, pb0, kb)
    LQ_MIX_LD(a1, pa1, ka)
    LQ_MIX_LD(b1, pb1, kb)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1));
    const v4f t = a0 + a1 + b0 + b1;
    if (t.x + t.y + t.z + t.w == 123.456f) sink[0] = t.x;
}

int main(int argc, char** argv) {
    const int64_t N = 256ll * 3 * 224 * 224;
    const int SETS = 4;
    const size_t pad = argc > 1 && strcmp(argv[1], "survive") && strcmp(argv[1], "mix") ? (size_t)atol(argv[1]) : 0;   // extra bytes between buffers (de-alias test)
    std::vector<float*> A(SETS), B(SETS), C(SETS);
    char* pool;
    size_t each = N * 4 + pad;
    each = (each + 255) / 256 * 256;
    CK(hipMalloc(&pool, each * 3 * SETS + 4096));
    CK(hipMemset(pool, 0, each * 3 * SETS));
    for (int i = 0; i < SETS; ++i) { A[i] = (float*)(pool + each * (3 * i)); B[i] = (float*)(pool + each * (3 * i + 1)); C[i] = (float*)(pool + each * (3 * i + 2)); }
    float* sink; CK(hipMalloc(&sink, 4));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int iters = 40;
    auto report = [&](const char* name, double bytes, float ms) {
        printf("%-44s %8.1f us  %7.0f GB/s\n", name, ms * 1000.0 / iters, bytes * iters / (ms * 1e-3) / 1e9);
    };
    auto run = [&](const char* name, double bytes, auto launch) {
        for (int w = 0; w < 5; ++w) launch(w % SETS);
        CK(hipEventRecord(e0));
        for (int it = 0; it < iters; ++it) launch(it % SETS);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipGetLastError()); report(name, bytes, ms);
    };
    const double b2 = N * 8.0, b3 = N * 12.0;
    // "mix" rows (`membench mix` prints only these): every point in turn, three rounds, so that drift hits all points alike
    if (argc > 1 && !strcmp(argv[1], "mix")) {
        struct Pt { char name[80]; int r2; Pick p, q; };
        std::vector<Pt> pts;
        const int nb1 = (int)(N / 4 / 512), nb2 = (int)(N / 4 / 1024), never = 0x7fffffff;
        const int keep1 = (int)((44ll << 20) / 8192), keep2 = keep1 / 2;      // the shipped 44 MiB tail, in blocks of each shape
        const Pick none = {never, 0u, 0}, all = {0, 0u, 0};
        const char* fn[4] = {"1/8", "1/4", "3/8", "1/2"};
        const unsigned fm[4] = {0x01u, 0x11u, 0x15u, 0x55u};                 // every 8th, 4th, (3 of 8), 2nd
        const char* pn[3] = {"tail", "every-kth-block", "every-kth-run-of-8"};
        auto pick = [&](int pat, int f, int nb) { return pat == 0 ? Pick{nb - nb * (f + 1) / 8, 0u, 0} : Pick{never, fm[f], pat == 1 ? 0 : 3}; };
        auto add = [&](int r2, Pick p, Pick q, const char* fmt, const char* a, const char* b) {
            Pt t; t.r2 = r2; t.p = p; t.q = q; snprintf(t.name, 80, fmt, a, b); pts.push_back(t); };
        // read + write; p = loads with the default policy, q = stores with plain nt (else sc1 nt)
        add(0, Pick{nb1 - keep1, 0u, 0}, none, "rw PARENT  ld tail 44MiB, st sc1nt%s%s", "", "");
        add(0, none, none, "rw ld f=0 (all nt), st sc1nt%s%s", "", "");
        add(0, all, none, "rw ld f=1 (all default), st sc1nt%s%s", "", "");
        for (int pat = 0; pat < 3; ++pat) for (int f = 0; f < 4; ++f) add(0, pick(pat, f, nb1), none, "rw ld %s f=%s, st sc1nt", pn[pat], fn[f]);
        add(0, Pick{nb1 - keep1, 0u, 0}, all, "rw ld tail 44MiB, st f=1 (all nt)%s%s", "", "");
        for (int pat = 0; pat < 2; ++pat) for (int f = 1; f < 4; f += 2) add(0, Pick{nb1 - keep1, 0u, 0}, pick(pat, f, nb1), "rw ld tail 44MiB, st nt %s f=%s", pn[pat], fn[f]);
        // two reads; p = stream A (P) default, q = stream B (dy) default
        add(1, Pick{nb2 - keep2, 0u, 0}, none, "r2 PARENT  A tail 44MiB, B nt%s%s", "", "");
        add(1, none, none, "r2 f=0 (all nt)%s%s", "", "");
        add(1, all, none, "r2 A f=1%s%s", "", "");
        add(1, none, all, "r2 B f=1%s%s", "", "");
        add(1, all, all, "r2 A+B f=1%s%s", "", "");
        for (int pat = 0; pat < 3; ++pat) for (int f = 0; f < 4; ++f) {
            add(1, pick(pat, f, nb2), none, "r2 A %s f=%s", pn[pat], fn[f]);
            add(1, none, pick(pat, f, nb2), "r2 B %s f=%s", pn[pat], fn[f]);
            add(1, pick(pat, f, nb2), pick(pat, f, nb2), "r2 A+B %s f=%s", pn[pat], fn[f]);
        }
        // beyond the issue's grid: other run lengths of the interleave (2^shift blocks), and the shipped tail kept next to it
        for (int sh = 1; sh <= 6; ++sh) for (int f = 1; f < 3; ++f) {
            if (sh == 3) continue;
            char rl[24]; snprintf(rl, 24, "every-kth-run-of-%d", 1 << sh);
            add(0, Pick{never, fm[f], sh}, none, "rw ld %s f=%s, st sc1nt", rl, fn[f]);
            if (sh <= 4) add(1, Pick{never, fm[f], sh}, none, "r2 A %s f=%s", rl, fn[f]);
        }
        for (int f = 0; f < 2; ++f) {
            add(0, Pick{nb1 - keep1, fm[f], 3}, none, "rw ld tail 44MiB + %s f=%s, st sc1nt", pn[2], fn[f]);
            add(1, Pick{nb2 - keep2, fm[f], 0}, none, "r2 A tail 44MiB + %s f=%s, B nt", pn[1], fn[f]);
        }
        for (int f = 0; f < 3; ++f) add(1, Pick{nb2 - keep2, 0u, 0}, Pick{never, fm[f], 0}, "r2 A tail 44MiB, B %s f=%s", pn[1], fn[f]);
        const int mi = 100;
        for (int rnd = 0; rnd < 3; ++rnd)
            for (const Pt& t : pts) {
                auto launch = [&](int k) {
                    if (t.r2) hipLaunchKernelGGL(k_mix_r2, dim3(nb2), dim3(512), 0, 0, A[k], B[k], sink, t.p, t.q);
                    else hipLaunchKernelGGL(k_mix_rw, dim3(nb1), dim3(512), 0, 0, A[k], C[k], sink, t.p, t.q);
                };
                for (int w = 0; w < 8; ++w) launch(w % SETS);
                CK(hipEventRecord(e0));
                for (int it = 0; it < mi; ++it) launch(it % SETS);
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                CK(hipGetLastError());
                printf("round %d  %-52s %8.2f us  %7.0f GB/s\n", rnd, t.name, ms * 1000.0 / mi, b2 * mi / (ms * 1e-3) / 1e9);
            }
        return 0;
    }
    // "survive" rows (`membench survive` prints only these): a 62 MB table (the first 0.4 of A[0]) is read with the default
    // policy, then 154 MB are stored to C[1] under one store policy, then the table is read again next to a cold 62 MB stream
    // (k_table2) and THAT kernel is timed.  "hot" re-reads it at once, "cold" after 616 MB of nontemporal read + write on other
    // buffers.  The second group reads A[1] (nontemporal) in the storing kernel as well, which is K1's mix.
    {
        const int nbt = (int)(N * 2 / 5 / 4 / 512), nb = (int)(N / 4 / 512);
        const double tb = (double)nbt * 512 * 16;
        auto table = [&] { hipLaunchKernelGGL((k_one<0, 512, 0>), dim3(nbt), dim3(512), 0, 0, A[0], B[0], C[0], sink); };
        int slice = 0;      // the cold stream walks six 62 MB slices of B[0], B[2], B[3]: far more than the cache between two uses of one
        auto survive = [&](const char* name, auto between) {
            float tot = 0.f;
            const int reps = 20;
            for (int it = 0; it < reps + 2; ++it) {
                table();
                between();
                const int bi[3] = {0, 2, 3};
                const float* cold = B[bi[slice / 2 % 3]] + (size_t)(slice % 2) * nbt * 2048;
                slice = (slice + 1) % 6;
                hipExtLaunchKernelGGL(k_table2, dim3(nbt), dim3(512), 0, 0, e0, e1, 0, A[0], cold, sink);      // the kernel's own duration
                CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (it >= 2) tot += ms;
            }
            CK(hipGetLastError());
            printf("%-52s %8.1f us  %7.0f GB/s\n", name, tot * 1000.0 / reps, 2 * tb * reps / (tot * 1e-3) / 1e9);
        };
        for (int rep = 0; rep < 2; ++rep) {
            survive("survive 62MB table: hot", [&] {});
            survive("survive 62MB table: cold (616MB between)", [&] {
                hipLaunchKernelGGL((k_one<2, 512, 1>), dim3(nb), dim3(512), 0, 0, A[2], B[2], C[2], sink);
                hipLaunchKernelGGL((k_one<2, 512, 1>), dim3(nb), dim3(512), 0, 0, A[3], B[3], C[3], sink); });
#define SURV(K, label) \
            survive("survive 62MB table: 154MB stores " label, [&] { hipLaunchKernelGGL(K, dim3(nb), dim3(512), 0, 0, A[1], C[1], 0); }); \
            survive("survive 62MB table: nt read + stores " label, [&] { hipLaunchKernelGGL(K, dim3(nb), dim3(512), 0, 0, A[1], C[1], 1); });
            SURV(k_st_plain, "(none)") SURV(k_st_nt, "nt") SURV(k_st_sc1nt, "sc1 nt") SURV(k_st_sc0sc1nt, "sc0 sc1 nt")
            SURV(k_st_sc1, "sc1") SURV(k_st_sc0sc1, "sc0 sc1")
        }
        if (argc > 1 && !strcmp(argv[1], "survive")) return 0;
    }
#define TB(label, MODE, bytes, BS) { char nm[96]; const int nb = (int)(N / 4 / BS); \
        snprintf(nm, 96, "one BS%d %s", BS, label); \
        run(nm, bytes, [&](int k){ hipLaunchKernelGGL((k_one<MODE, BS, 0>), dim3(nb), dim3(BS), 0, 0, A[k], B[k], C[k], sink); }); \
        snprintf(nm, 96, "one BS%d %s nt", BS, label); \
        run(nm, bytes, [&](int k){ hipLaunchKernelGGL((k_one<MODE, BS, 1>), dim3(nb), dim3(BS), 0, 0, A[k], B[k], C[k], sink); }); }
    for (int rep = 0; rep < 2; ++rep) {
    TB("read2", 1, b2, 256) TB("read2", 1, b2, 512) TB("read2", 1, b2, 1024)
    TB("read1+write1", 2, b2, 256) TB("read1+write1", 2, b2, 512) TB("read1+write1", 2, b2, 1024)
    TB("read2+write1", 3, b3, 256) TB("read2+write1", 3, b3, 512) TB("read2+write1", 3, b3, 1024)
    }
#define POL(K, label) { const int nb = (int)(N / 4 / 512); \
        run("policy " label "  read1+write1", b2, [&](int k){ hipLaunchKernelGGL(K, dim3(nb), dim3(512), 0, 0, A[k], B[k], C[k], sink, 2); }); \
        run("policy " label "  read2", b2, [&](int k){ hipLaunchKernelGGL(K, dim3(nb), dim3(512), 0, 0, A[k], B[k], C[k], sink, 1); }); }
    for (int rep = 0; rep < 2; ++rep) {
        POL(k_pol_plain, "(none)      ") POL(k_pol_nt, "nt          ") POL(k_pol_sc1nt, "sc1 nt      ") POL(k_pol_sc0sc1nt, "sc0 sc1 nt  ")
        POL(k_pol_sc1, "sc1         ") POL(k_pol_sc0sc1, "sc0 sc1     ") POL(k_pol_ldnt_stsc, "ld nt/st sc*") POL(k_pol_ldsc_stnt, "ld sc*/st nt")
    }
    for (int rep = 0; rep < 2; ++rep) {     // nb = N/4/512 = 18816 is a multiple of 8
        const int nb = (int)(N / 4 / 512);
        run("xcd round-robin  BS512 read1+write1 nt", b2, [&](int k){ hipLaunchKernelGGL((k_one_x<2, 512, 1, 0>), dim3(nb), dim3(512), 0, 0, A[k], B[k], C[k], sink, nb); });
        run("xcd contiguous   BS512 read1+write1 nt", b2, [&](int k){ hipLaunchKernelGGL((k_one_x<2, 512, 1, 1>), dim3(nb), dim3(512), 0, 0, A[k], B[k], C[k], sink, nb); });
        run("xcd round-robin  BS512 read2 nt", b2, [&](int k){ hipLaunchKernelGGL((k_one_x<1, 512, 1, 0>), dim3(nb), dim3(512), 0, 0, A[k], B[k], C[k], sink, nb); });
        run("xcd contiguous   BS512 read2 nt", b2, [&](int k){ hipLaunchKernelGGL((k_one_x<1, 512, 1, 1>), dim3(nb), dim3(512), 0, 0, A[k], B[k], C[k], sink, nb); });
    }
    {
        const int nb = (int)(N / 1024); char nm[96];
        snprintf(nm, 96, "ALTERNATE BS256 nt: R1W1 then R2 (616MB)");
        run(nm, N * 16.0, [&](int k){
            hipLaunchKernelGGL((k_one<2, 256, 1>), dim3(nb), dim3(256), 0, 0, A[k], B[k], C[k], sink);
            hipLaunchKernelGGL((k_one<1, 256, 1>), dim3(nb), dim3(256), 0, 0, A[k], B[k], C[k], sink); });
    }
    return 0;
}
