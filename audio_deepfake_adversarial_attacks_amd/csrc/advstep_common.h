// advstep_common.h — helpers shared by the csrc/*.hip translation units (internal: not part of the C ABI in include/).
//
// Each .hip file is its own translation unit and includes this once, so every helper keeps internal linkage.  Some of
// these are rules that separate kernels must agree on bit for bit: the max-feature-map / 2x2 pool selection written by
// the forward kernels (lcnn_conv0.hip, lcnn_wino.hip, lcnn_mfm.hip) and read back by the backward ones (lcnn_mfm.hip),
// and the dB backward of the plain and the fused LFCC tails (lfcc.hip, lfcc_stft.hip).

#ifndef ADVSTEP_COMMON_H
#define ADVSTEP_COMMON_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

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

// ---- device side ------------------------------------------------------------------------------------------------------

// torch.max(a, b) for tensors: NaN propagates.
__device__ __forceinline__ float max_nan(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
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
