// advstep_common.h — helpers shared by the csrc/*.hip translation units (internal: not part of the C ABI in include/).
//
// Each .hip file is its own translation unit and includes this once, so every helper keeps internal linkage.  Some of
// these are rules that separate kernels must agree on bit for bit: the max-feature-map / 2x2 pool selection written by
// the forward kernels (lcnn_conv0.hip, lcnn_wino.hip, lcnn_mfm.hip) and read back by the backward ones (lcnn_mfm.hip),
// and the dB backward of the plain and the fused LFCC tails (lfcc.hip, lfcc_stft.hip).  The attack files (advstep.hip, apgd.hip,
// momentum.hip, radius.hip, perturb.hip, multiattack.hip, fab.hip, apgdl1.hip, snr.hip, universal.hip, spsa.hip, channel.hip,
// l0.hip, hsj.hip, smooth.hip, smoothadv.hip, fmn.hip, fmn_sparse.hip) share the scalar semantics, the reduction operators with the wave butterfly, and the host's rows_vec /
// ROW_KERNEL_PAIR / overlaps; what depends on the 256-thread (tile, row) geometry is in row_tiles.h; fab.hip, apgdl1.hip and
// l0.hip (and fmn_sparse.hip, which shares their projections: row_project.h) give a row to one 1024-thread workgroup instead:
// row_workgroup.h, which also holds their sort-free threshold search.

#ifndef ADVSTEP_COMMON_H
#define ADVSTEP_COMMON_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>

#include "advstep.h"

#define ADVSTEP_REQUIRE(cond) \
    do {                      \
        if (!(cond)) return ADVSTEP_EINVAL; \
    } while (0)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- host side --------------------------------------------------------------------------------------------------------

constexpr int64_t kMaxGridY = 65535;

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline hipStream_t as_stream(advstep_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline int status_after_launch() { return hipGetLastError() == hipSuccess ? ADVSTEP_OK : ADVSTEP_ELAUNCH; }

// Are rows of T samples float4-addressable from every (non-null) base?  The VEC choice of every row kernel, 256- or 1024-thread.
inline bool rows_vec(int64_t T, std::initializer_list<const void *> ptrs) {
    if (T % 4 != 0) return false;
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return false;
    return true;
}
// The two instantiations of a row kernel whose first template parameter is VEC, indexed by rows_vec(...); further arguments are
// the kernel's further template arguments: ROW_KERNEL_PAIR(K, 2) = {K<false, 2>, K<true, 2>}.  The only place that writes the
// pair, so its order is fixed once; row_tiles.h's launch_tiles and row_workgroup.h's launch_rows take it.
#define ROW_KERNEL_PAIR(KERNEL, ...) {KERNEL<false, ##__VA_ARGS__>, KERNEL<true, ##__VA_ARGS__>}

inline bool overlaps(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}
// ... and for two buffers of different sizes (multiattack.hip, radius.hip)
inline bool overlap2(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + b_bytes && q < p + a_bytes;
}

// ---- the row workspace of include/advstep.h (ABI 3): advstep.hip, apgd.hip and momentum.hip carve the same buffer ----------

// One float partial per (row, 4096-sample tile): C = ceil(T / 4096) tiles per row.
constexpr int64_t kWsRowTile = 4096;
inline int ws_tiles_per_row(int64_t T) { return (int)ceil_div(T, kWsRowTile); }

struct RowWs {
    float *p0;
    float *p1;
    unsigned *epoch;               // single-pass PGD-L2 exchange: call counter (the tags' epoch) ...
    unsigned long long *gran0;     // ... two planes of B x C 8-byte {tag, value} granules ...
    unsigned long long *gran1;
    unsigned *fail;                // ... the live "row needs repair" flags and the flags of the LAST single-pass call as its
    unsigned *last;                //     repair pass left them (advstep_pgd_l2_repaired_rows reads those)
};
// Layout for a (B, T) batch, C = tiles per row (round 5: the exchange area no longer lies over the float planes):
//   [16-byte header: epoch word][granule plane 0][granule plane 1][fail flags][last flags][float plane 0][float plane 1]
inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
constexpr size_t kWsHeader = 16;
inline size_t row_ws_plane(int64_t B, int64_t T) { return align16((size_t)B * (size_t)ws_tiles_per_row(T) * sizeof(float)); }
inline size_t row_ws_granules(int64_t B, int64_t T) {
    return align16((size_t)B * (size_t)ws_tiles_per_row(T) * sizeof(unsigned long long));
}
inline size_t row_ws_flags(int64_t B) { return align16((size_t)B * sizeof(unsigned)); }
inline size_t row_ws_bytes(int64_t B, int64_t T) {
    return kWsHeader + 2 * row_ws_granules(B, T) + 2 * row_ws_flags(B) + 2 * row_ws_plane(B, T);
}
inline bool carve_ws(void *ws, size_t ws_bytes, int64_t B, int64_t T, RowWs *out) {
    if (!ws || !aligned16(ws) || ws_bytes < row_ws_bytes(B, T)) return false;
    char *p = static_cast<char *>(ws);
    out->epoch = reinterpret_cast<unsigned *>(p);
    p += kWsHeader;
    out->gran0 = reinterpret_cast<unsigned long long *>(p);
    p += row_ws_granules(B, T);
    out->gran1 = reinterpret_cast<unsigned long long *>(p);
    p += row_ws_granules(B, T);
    out->fail = reinterpret_cast<unsigned *>(p);
    p += row_ws_flags(B);
    out->last = reinterpret_cast<unsigned *>(p);
    p += row_ws_flags(B);
    out->p0 = reinterpret_cast<float *>(p);
    out->p1 = reinterpret_cast<float *>(p + row_ws_plane(B, T));
    return true;
}

// ---- device side ------------------------------------------------------------------------------------------------------

// ---- scalar semantics shared by all kernels (include/advstep.h): torch's, NaN included ------------------------------------

// torch.max(a, b) / torch.min(a, b) for tensors: NaN propagates.
__device__ __forceinline__ float max_nan(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}
__device__ __forceinline__ float min_nan(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return a < b ? a : b;
}

// torch.sign: (0 < g) - (g < 0); NaN and +-0 give 0.
__device__ __forceinline__ float sgn(float g) { return (float)(0.0f < g) - (float)(g < 0.0f); }

// torch.clamp(v, lo, hi) = min(max(v, lo), hi), NaN in v propagates.
__device__ __forceinline__ float clampf(float v, float lo, float hi) {
    v = (v < lo) ? lo : v;
    return (v > hi) ? hi : v;
}

// Is a one-logit row misclassified?  multi_select_kernel's rule (multiattack.hip): torch.max(cat([-z, z], 1), 1) takes the first
// maximal index, so +-0 and NaN give class 0.  radius.hip's search round and fmn.hip's row decision.
__device__ __forceinline__ bool judged_wrong(float z, int64_t y) { return (int64_t)(z > 0.0f) != y; }

// The PGD L-inf move and projection of one sample (pgd.py:74-76): advstep.hip's advstep_pgd_linf_step_f32 and spsa.hip's step,
// which promises that entry point's bits for its estimated gradient.
__device__ __forceinline__ float pgd_linf_elem(float a, float g, float x, float alpha, float eps, float lo, float hi) {
    a = a + alpha * sgn(g);
    float d = clampf(a - x, -eps, eps);
    return clampf(x + d, lo, hi);
}

// log(1 + exp(t)), stable: the 2-logit cross-entropy in closed form.
__device__ __forceinline__ float softplusf(float t) { return (t > 0.0f ? t : 0.0f) + log1pf(expf(-fabsf(t))); }

// ---- reductions: wave64 xor shuffles (offsets 32 -> 1), then over a 256-thread workgroup one LDS slot per wave, combined as
// ((l0 . l1) . l2) . l3.  All threads receive the result; `lds` holds >= 4 floats, and two calls in a row must use different
// slots (each ends on a barrier over its own).  Partials that separate kernels re-reduce must agree bit for bit: this is the
// one body.  (row_workgroup.h's 1024-thread row_reduce is built on wave_reduce and states its own contract: 16 slots per value,
// several values per barrier pair, a trailing barrier.)
constexpr int kWgThreads = 256;
template <class Op>
__device__ __forceinline__ float wave_reduce(float v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}
template <class Op>
__device__ __forceinline__ float wg_reduce(float v, Op op, float *lds) {
    v = wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(op(lds[0], lds[1]), lds[2]), lds[3]);
}
struct SumOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};
struct MinNanOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return min_nan(a, b); }
};
struct MaxNanOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return max_nan(a, b); }
};
__device__ __forceinline__ float wg_sum(float v, float *lds) { return wg_reduce(v, SumOp(), lds); }
__device__ __forceinline__ float wg_max_nan(float v, float *lds) { return wg_reduce(v, MaxNanOp(), lds); }
__device__ __forceinline__ float wg_min_nan(float v, float *lds) { return wg_reduce(v, MinNanOp(), lds); }

// ---- Philox4x32-10 (Salmon et al., SC'11), counter-based: the random starts of advstep.hip and apgd.hip draw from it, and
// spsa.hip takes its direction bits from it, smooth.hip the normals of its noisy copies ----

struct Quad {
    uint32_t v[4];
};

__device__ __forceinline__ Quad philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Quad{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float u01(uint32_t bits) { return (float)(bits >> 8) * 5.9604644775390625e-08f; }
__device__ __forceinline__ float u01_open0(uint32_t bits) {  // (0, 1]
    return (float)((bits >> 8) + 1u) * 5.9604644775390625e-08f;
}

// 4 uniforms in [-eps, eps) for quad q of the flat buffer, as Tensor.uniform_(-eps, eps) forms them: u * (eps - (-eps)) + (-eps)
__device__ __forceinline__ float4 philox_uniform4(uint64_t q, uint64_t seed, uint64_t offset, float eps) {
    const Quad r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)offset, (uint32_t)(offset >> 32),
                                 (uint32_t)seed, (uint32_t)(seed >> 32));
    const float from = -eps, range = eps - from;
    return make_float4(u01(r.v[0]) * range + from, u01(r.v[1]) * range + from, u01(r.v[2]) * range + from,
                       u01(r.v[3]) * range + from);
}

// 4 standard normals for quad q of row b (Box-Muller on two uniform pairs).
__device__ __forceinline__ float4 philox_normal4(uint32_t q, uint32_t b, uint64_t seed, uint64_t offset) {
    const Quad r = philox4x32_10(q, b, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                                 (uint32_t)(seed >> 32));
    // Round 4: the hardware transcendentals (v_log_f32, v_sin_f32 / v_cos_f32: ~1 ulp / ~1e-6 absolute) instead of OCML's
    // correctly-rounded-ish logf / sinf / cosf, which were what this start kernel spent its time in (24 us for 8 B / sample = 0.34
    // of the HBM roofline).  The random start has no reference bit pattern to match (pgdl2.py:55-62 draws from torch's own
    // generator); the oracle twin (oracle/kernels.py, libm) agrees to ~1e-9 after the eps / ||n|| scaling, inside the 1e-7 bound
    // oracle/checked_ops.py applies, and every path of the library (single-pass, repair, two-kernel) calls THIS function.
    const float r0 = sqrtf(-2.0f * __logf(u01_open0(r.v[0])));
    const float r1 = sqrtf(-2.0f * __logf(u01_open0(r.v[2])));
    const float t0 = 6.283185307179586f * u01(r.v[1]);
    const float t1 = 6.283185307179586f * u01(r.v[3]);
    return make_float4(r0 * __cosf(t0), r0 * __sinf(t0), r1 * __cosf(t1), r1 * __sinf(t1));
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding global access
// (s_waitcnt vmcnt(0)): inside the step loops that put each step's stores — and the prefetch of the next step's inputs —
// on the critical path of a 25-step recurrence.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// at::native::MaxOps combine for two candidates at indices 0 (a) and 1 (b): true when b is selected.
__device__ __forceinline__ bool mfm_takes_b(float a, float b) { return !(a != a) && !(a >= b); }

// One pooled output from its 2x2 window of (a, b) pairs, in ATen's order: MFM per position, then the pool scan
// (0,0), (0,1), (1,0), (1,1) with  take = (v > best || isnan(v)),  best = -inf initially.
__device__ __forceinline__ float pool_select(float a00, float b00, float a01, float b01, float a10, float b10,
                                             float a11, float b11, int &code) {
    const bool t00 = mfm_takes_b(a00, b00), t01 = mfm_takes_b(a01, b01);
    const bool t10 = mfm_takes_b(a10, b10), t11 = mfm_takes_b(a11, b11);
    const float m00 = t00 ? b00 : a00, m01 = t01 ? b01 : a01, m10 = t10 ? b10 : a10, m11 = t11 ? b11 : a11;
    float best = -INFINITY;
    int pos = 0;
    bool tb = t00;
    if (m00 > best || m00 != m00) { best = m00; pos = 0; tb = t00; }
    if (m01 > best || m01 != m01) { best = m01; pos = 1; tb = t01; }
    if (m10 > best || m10 != m10) { best = m10; pos = 2; tb = t10; }
    if (m11 > best || m11 != m11) { best = m11; pos = 3; tb = t11; }
    code = ((int)tb << 2) | pos;
    return best;
}

// The same selection in 4 + 15 instead of ~33 vector instructions (round 3): gfx950's v_maximum3_f32 propagates NaN, so the
// maximum of the 8 candidates is the pooled value whenever no candidate is NaN, and the winner's code is the FIRST candidate
// in the reference's scan order (a00, b00, a01, b01, a10, b10, a11, b11: `a` keeps ties inside a position, the earlier position
// keeps ties between positions) that equals it.  A NaN among the candidates (best != best) takes the step-by-step rule above.
// (A tie between -0 and +0 returns +0 where the scan returns the first: convolution outputs, not bit-compared.)
__device__ __forceinline__ float pool_select_fast(float a00, float b00, float a01, float b01, float a10, float b10,
                                                  float a11, float b11, int &code) {
    const float best = __builtin_elementwise_maximum(
        __builtin_elementwise_maximum(__builtin_elementwise_maximum(a00, b00), __builtin_elementwise_maximum(a01, b01)),
        __builtin_elementwise_maximum(__builtin_elementwise_maximum(a10, b10), __builtin_elementwise_maximum(a11, b11)));
    if (best != best) return pool_select(a00, b00, a01, b01, a10, b10, a11, b11, code);
    int c = 7;
    c = a11 == best ? 3 : c;
    c = b10 == best ? 6 : c;
    c = a10 == best ? 2 : c;
    c = b01 == best ? 5 : c;
    c = a01 == best ? 1 : c;
    c = b00 == best ? 4 : c;
    c = a00 == best ? 0 : c;
    code = c;
    return best;
}

// AmplitudeToDB's floor and scale: 10 log10(clamp(band, kAmin)).
constexpr float kAmin = 1e-10f;
constexpr float kDbScale = 4.342944819032518f;  // 10 / ln(10)

// d/d band of 10 log10(clamp(band, amin)), band recovered from its dB value
__device__ __forceinline__ float dlog_of_db(float db) {
    return (db > -100.0f) ? kDbScale / expf(db * 0.23025850929940457f) : 0.0f;
}

}  // namespace

#endif  // ADVSTEP_COMMON_H
