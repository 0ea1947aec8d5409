// advstep.hip — gfx950 (MI355X / CDNA4) kernels + the C ABI declared in include/advstep.h.
//
// Every kernel here is HBM-bound streaming or row-reduction work over (B, T) float32 waveforms:
//   * 16 B per lane (float4) coalesced loads, 4 independent float4 per input stream per thread in flight
//     (a wave64 instruction moves 1 KiB; a 256-thread workgroup owns one 16 KiB tile per stream);
//   * row reductions: wave64 xor-shuffles -> 4-entry LDS -> one partial per (row, tile) in the caller's
//     workspace -> re-reduced by every workgroup of the row in the consuming pass (fixed order, no float
//     atomics: run-to-run deterministic);
//   * the (row, tile) -> workgroup id map is identical in the producing and consuming pass of a row
//     operation, so with the observed id % 8 -> XCD placement a tile is re-read on the XCD whose L2 saw it;
//   * arithmetic follows the reference expression by expression (see include/advstep.h): this file is built
//     with -ffp-contract=off, divisions are IEEE (hipcc default for f32), clamps propagate NaN.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared (see build.py).

#include <hip/hip_runtime.h>
#include <atomic>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "advstep.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

constexpr int kMaxGrid = 256 * 16;                 // flat kernels: grid-stride beyond 16 tiles per CU

__device__ __forceinline__ float fgsm_elem(float x, float g, float eps, float lo, float hi) {
    return clampf(x + eps * sgn(g), lo, hi);
}

// ---------------------------------------------------------------------------------------------------------
// flat elementwise kernels: n = B*T samples, tile-strided, float4 when all pointers are 16-byte aligned
// ---------------------------------------------------------------------------------------------------------

// Generic driver: NIN input streams, one output stream, Op applied per sample; VECS float4 per thread per stream.
template <int NIN, int VECS, class Op>
__global__ __launch_bounds__(kWgThreads) void flat_vec_kernel(const float4 *__restrict__ in0,
                                                          const float4 *__restrict__ in1,
                                                          const float4 *__restrict__ in2, float4 *out, int64_t n4,
                                                          int64_t ntiles, Op op) {
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * (kWgThreads * VECS) + threadIdx.x;
        float4 a[VECS] = {}, b[VECS] = {}, c[VECS] = {};
#pragma unroll
        for (int j = 0; j < VECS; ++j) {
            const int64_t i = base + (int64_t)j * kWgThreads;
            if (i < n4) {
                a[j] = in0[i];
                if (NIN > 1) b[j] = in1[i];
                if (NIN > 2) c[j] = in2[i];
            }
        }
#pragma unroll
        for (int j = 0; j < VECS; ++j) {
            const int64_t i = base + (int64_t)j * kWgThreads;
            if (i < n4) {
                float4 o;
                o.x = op(a[j].x, b[j].x, c[j].x);
                o.y = op(a[j].y, b[j].y, c[j].y);
                o.z = op(a[j].z, b[j].z, c[j].z);
                o.w = op(a[j].w, b[j].w, c[j].w);
                out[i] = o;
            }
        }
    }
}

// Scalar twin for the (< 4)-sample tail and for unaligned buffers: samples [begin, n).
template <int NIN, class Op>
__global__ __launch_bounds__(kWgThreads) void flat_scalar_kernel(const float *__restrict__ in0,
                                                             const float *__restrict__ in1,
                                                             const float *__restrict__ in2, float *out,
                                                             int64_t begin, int64_t n, Op op) {
    for (int64_t i = begin + (int64_t)blockIdx.x * kWgThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWgThreads) {
        const float a = in0[i];
        const float b = NIN > 1 ? in1[i] : 0.0f;
        const float c = NIN > 2 ? in2[i] : 0.0f;
        out[i] = op(a, b, c);
    }
}

struct FgsmOp {
    float eps, lo, hi;
    __device__ __forceinline__ float operator()(float x, float g, float) const {
        return fgsm_elem(x, g, eps, lo, hi);
    }
};
struct PgdLinfOp {
    float alpha, eps, lo, hi;
    __device__ __forceinline__ float operator()(float a, float g, float x) const {
        return pgd_linf_elem(a, g, x, alpha, eps, lo, hi);
    }
};
struct AddClampOp {
    float lo, hi;
    __device__ __forceinline__ float operator()(float x, float nz, float) const { return clampf(x + nz, lo, hi); }
};
struct CwInitOp {
    // cw.py:117-122: atanh(x*2 - 1) spelled 0.5*log((1+y)/(1-y))
    __device__ __forceinline__ float operator()(float x, float, float) const {
        const float y = x * 2.0f - 1.0f;
        return 0.5f * logf((1.0f + y) / (1.0f - y));
    }
};

// PGD L-inf random start with in-kernel Philox: quad index == float4 index.
__global__ __launch_bounds__(kWgThreads) void pgd_linf_init_philox_vec_kernel(const float4 *__restrict__ x, float4 *out,
                                                                          int64_t n4, int64_t ntiles, float eps,
                                                                          float lo, float hi, uint64_t seed,
                                                                          uint64_t offset) {
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * kTileVec + threadIdx.x;
        float4 a[kVecs];
#pragma unroll
        for (int j = 0; j < kVecs; ++j) {
            const int64_t i = base + (int64_t)j * kWgThreads;
            if (i < n4) a[j] = x[i];
        }
#pragma unroll
        for (int j = 0; j < kVecs; ++j) {
            const int64_t i = base + (int64_t)j * kWgThreads;
            if (i < n4) {
                const float4 nz = philox_uniform4((uint64_t)i, seed, offset, eps);
                float4 o;
                o.x = clampf(a[j].x + nz.x, lo, hi);
                o.y = clampf(a[j].y + nz.y, lo, hi);
                o.z = clampf(a[j].z + nz.z, lo, hi);
                o.w = clampf(a[j].w + nz.w, lo, hi);
                out[i] = o;
            }
        }
    }
}

__global__ __launch_bounds__(kWgThreads) void pgd_linf_init_philox_scalar_kernel(const float *__restrict__ x, float *out,
                                                                             int64_t begin, int64_t n, float eps,
                                                                             float lo, float hi, uint64_t seed,
                                                                             uint64_t offset) {
    for (int64_t i = begin + (int64_t)blockIdx.x * kWgThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWgThreads) {
        const float4 nz = philox_uniform4((uint64_t)(i >> 2), seed, offset, eps);
        out[i] = clampf(x[i] + lane(nz, (int)(i & 3)), lo, hi);
    }
}

// CW Adam step on w (tanh recomputed; see header).
struct AdamScalars {
    float w1;        // 1 - beta1           (lerp weight)
    float beta2;     // beta2
    float omb2;      // 1 - beta2
    float neg_step;  // -(lr / (1 - beta1^t))
    float bc2_sqrt;  // sqrt(1 - beta2^t)
    float eps;
};

__device__ __forceinline__ void cw_adam_elem(float &w, float &m, float &v, float x, float gm, const AdamScalars &s) {
    const float y = tanhf(w);
    const float a = 0.5f * (y + 1.0f);
    const float g = ((2.0f * (a - x) + gm) * 0.5f) * (1.0f - y * y);
    m = m + s.w1 * (g - m);
    v = v * s.beta2 + (s.omb2 * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    w = w + s.neg_step * (m / denom);
}

__global__ __launch_bounds__(kWgThreads) void cw_adam_vec_kernel(float4 *w, float4 *m, float4 *v,
                                                             const float4 *__restrict__ x,
                                                             const float4 *__restrict__ gm, int64_t n4,
                                                             int64_t ntiles, AdamScalars s) {
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * kTileVec + threadIdx.x;
#pragma unroll 2
        for (int j = 0; j < kVecs; ++j) {
            const int64_t i = base + (int64_t)j * kWgThreads;
            if (i < n4) {
                float4 W = w[i], M = m[i], V = v[i];
                const float4 X = x[i], G = gm[i];
                cw_adam_elem(W.x, M.x, V.x, X.x, G.x, s);
                cw_adam_elem(W.y, M.y, V.y, X.y, G.y, s);
                cw_adam_elem(W.z, M.z, V.z, X.z, G.z, s);
                cw_adam_elem(W.w, M.w, V.w, X.w, G.w, s);
                w[i] = W;
                m[i] = M;
                v[i] = V;
            }
        }
    }
}

__global__ __launch_bounds__(kWgThreads) void cw_adam_scalar_kernel(float *w, float *m, float *v,
                                                                const float *__restrict__ x,
                                                                const float *__restrict__ gm, int64_t begin,
                                                                int64_t n, AdamScalars s) {
    for (int64_t i = begin + (int64_t)blockIdx.x * kWgThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWgThreads) {
        float W = w[i], M = m[i], V = v[i];
        cw_adam_elem(W, M, V, x[i], gm[i], s);
        w[i] = W;
        m[i] = M;
        v[i] = V;
    }
}

// ---------------------------------------------------------------------------------------------------------
// row kernels: grid = (C tiles per row, B rows); tile addressing, whole-tile loads / stores and the re-reduction of a row's
// partials are row_tiles.h's.  VEC = rows are float4-addressable (T % 4 == 0 and 16-byte aligned bases).
// ---------------------------------------------------------------------------------------------------------

// ---- a1: to_minmax ----------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void minmax_partial_kernel(const float *__restrict__ x, int64_t T,
                                                                float *__restrict__ pmin, float *__restrict__ pmax) {
    __shared__ float lds[8];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    const float *row = x + b * T;
    // neutral fill: the row's first sample (always in range) keeps NaN propagation intact
    const float fill = row[0];
    float4 r[kVecs];
    load_tile<VEC>(row, T, tile, fill, r);
    float lo = fill, hi = fill;
    for_each_lane(r, [&](float e) {
        lo = min_nan(lo, e);
        hi = max_nan(hi, e);
    });
    lo = wg_min_nan(lo, lds);
    hi = wg_max_nan(hi, lds + 4);
    if (threadIdx.x == 0) {
        pmin[b * C + tile] = lo;
        pmax[b * C + tile] = hi;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void minmax_apply_kernel(const float *__restrict__ x, float *x01,
                                                              float *__restrict__ mn_out, float *__restrict__ mx_out,
                                                              int64_t T, const float *__restrict__ pmin,
                                                              const float *__restrict__ pmax) {
    __shared__ float lds[8];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 r[kVecs];
    load_tile<VEC>(x + b * T, T, tile, 0.0f, r);
    const float mn = row_min(pmin + b * C, C, lds);
    const float mx = row_max(pmax + b * C, C, lds + 4);
    const float range = mx - mn;
    for_each_lane(r, [&](float &e) { e = (e - mn) / range; });
    store_tile<VEC>(x01 + b * T, T, tile, r);
    if (tile == 0 && threadIdx.x == 0) {
        mn_out[b] = mn;
        mx_out[b] = mx;
    }
}

// ---- a2: revert_minmax ------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void minmax_revert_kernel(const float *__restrict__ x01,
                                                               const float *__restrict__ mn,
                                                               const float *__restrict__ mx, float *out, int64_t T) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    float4 r[kVecs];
    load_tile<VEC>(x01 + b * T, T, tile, 0.0f, r);
    const float lo = mn[b];
    const float range = mx[b] - lo;
    for_each_lane(r, [&](float &e) { e = (e * range) + lo; });
    store_tile<VEC>(out + b * T, T, tile, r);
}

// (the row sum of squares, sumsq_partial_kernel, is row_tiles.h's: radius.hip launches it too)

// ---- a6: PGD-L2 step ------------------------------------------------------------------------------------------

// pass 2 and pass 3: the bodies are row_tiles.h's (radius.hip runs them with a radius per row)
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void pgd_l2_delta_kernel(const float *__restrict__ adv,
                                                              const float *__restrict__ grad,
                                                              const float *__restrict__ orig, int64_t T, float alpha,
                                                              float eps_div, const float *__restrict__ gpart,
                                                              float *__restrict__ dpart, float *__restrict__ gnorm) {
    __shared__ float lds[8];
    l2_delta_pass<VEC>(adv, grad, orig, T, alpha, eps_div, gpart, dpart, gnorm, lds);
}

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void pgd_l2_project_kernel(const float *__restrict__ adv,
                                                                const float *__restrict__ grad,
                                                                const float *__restrict__ orig, float *out, int64_t T,
                                                                float alpha, float eps, float eps_div, float lo,
                                                                float hi, const float *__restrict__ gpart,
                                                                const float *__restrict__ dpart,
                                                                float *__restrict__ dnorm) {
    __shared__ float lds[8];
    l2_project_pass<VEC, false>(adv, grad, orig, out, T, alpha, eps, eps_div, lo, hi, gpart, dpart, dnorm, lds);
}


// ---- a6 in ONE pass: the row's workgroups keep their tiles in registers across the two row reductions ----------------------
// 16 B per sample (adv, grad, orig read once; out written once) instead of 32.  A row is 16 workgroups (T = 64 600); its
// two norms are exchanged INSIDE the launch through 8-byte {tag, value} granules (one per workgroup and phase, written by ONE
// agent-scope store, re-read with agent-scope loads until every tag of the row shows the phase: the data is the flag, no
// fence — the CDNA HIP programming guide's Guideline 16, form R2).  tag = {call epoch, phase}: the workspace's first
// word counts the single-pass calls that used it (the repair kernel behind every call advances it), so a granule of an earlier
// call — or a word some other user of the scratch left there — never carries this call's tag and nothing has to be cleaned
// between calls (round 5; rounds 2-3 zeroed the granules with a memset node, round 4 in the repair kernel).  The partial sums
// and their re-reduction are the three-kernel path's own (same wg_sum, same order): results are bit-identical to it.
//
// Co-residency.  A spinning workgroup must not wait for one that has no slot.  The host takes this path only when the
// launch fits the device's resident capacity for THIS kernel (CU count x hipOccupancyMaxActiveBlocksPerMultiprocessor,
// queried once per device: l2_resident_capacity) — but capacity is not a guarantee: another stream or process may hold
// slots (two ranks sharing a device, a partitioned device).  So the wait is bounded, and a sweep that does not complete
// does NOT produce a wrong row: the workgroup raises the row's flag in the workspace, poisons its later granules (its
// siblings stop waiting at once) and leaves; a repair kernel queued behind every single-pass launch recomputes flagged rows
// from global memory with the three-kernel path's arithmetic (one workgroup per row, tiles in sequence: same partial sums,
// same re-reduction, same bits) and returns immediately for all other rows.
typedef unsigned long long __attribute__((address_space(1))) gu64;
// Tags of one call: (epoch + 1) << 2 | {1, 2: the two row sums; 3: poison}.  30 bits of epoch; a zero-filled workspace holds no
// valid tag (the smallest is 5), and the flag values below (high bit set) are no tag of the first 2^29 calls either.
constexpr unsigned kPoisonPhase = 3u;
constexpr unsigned kRowFlagged = 0x80000001u;
__device__ __forceinline__ unsigned exchange_tag_base(const unsigned *epoch) {
    return (*epoch + 1u) << 2;
}

// Returns the row sum; *failed (workgroup-uniform, valid after the call) tells that the sweep was abandoned.
__device__ __forceinline__ float row_exchange_sum(unsigned long long *granules, int C, int tile, float mine, unsigned base,
                                                  unsigned phase_no, unsigned spin_limit, float *lds, int *lds_failed) {
    const unsigned phase = base | phase_no, poison_tag = base | kPoisonPhase;
    if (threadIdx.x == 0) {
        *lds_failed = 0;
        __hip_atomic_store((gu64 *)(granules + tile), ((unsigned long long)phase << 32) | __float_as_uint(mine),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float v = 0.0f;
    if (threadIdx.x < 64) {                       // wave 0 sweeps the row's granules: lane i < C reads granule i
        bool done = false;
        for (unsigned spins = 0; spins < spin_limit; ++spins) {
            bool ok = true, poisoned = false;
            unsigned long long x = 0;
            if ((int)threadIdx.x < C) {
                x = __hip_atomic_load((gu64 *)(granules + threadIdx.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = (unsigned)(x >> 32) == phase;
                poisoned = (unsigned)(x >> 32) == poison_tag;
            }
            if (__any(poisoned)) break;
            if (__all(ok)) {
                v = (int)threadIdx.x < C ? __uint_as_float((unsigned)x) : 0.0f;
                done = true;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (!done && threadIdx.x == 0) *lds_failed = 1;
    }
    // same reduction as row_sum(): thread i holds partial i (C <= 64 on this path), the others the identity
    // (wg_sum's barrier also publishes *lds_failed)
    return wg_sum(v, lds);
}

// A workgroup that gives up: flag the row, poison this workgroup's granules of the phases it will not reach.
__device__ __forceinline__ void row_exchange_abandon(unsigned *fail, int64_t b, unsigned long long *g0, unsigned long long *g1,
                                                     int tile, unsigned base) {
    if (threadIdx.x == 0) {
        __hip_atomic_store((unsigned __attribute__((address_space(1))) *)(fail + b), kRowFlagged, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long poison = (unsigned long long)(base | kPoisonPhase) << 32;
        if (g0) __hip_atomic_store((gu64 *)(g0 + tile), poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g1) __hip_atomic_store((gu64 *)(g1 + tile), poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Register budget: all 2 048 workgroups (8 192 waves) must be resident, i.e. 64 VGPRs per lane, and adv + grad + orig of a tile
// are 48 of them — the three arrays of the batch are 100 MB, three quarters of the chip's register files.  `orig` therefore sits
// in LDS (16 KB per workgroup, 8 workgroups per CU = 128 of the 160 KB) and is read back where it is used; adv and grad stay
// in registers.  (With all three in registers hipcc spilled 15 dwords per lane: 31 MB of scratch writes per launch.)
template <bool VEC>
__global__ __launch_bounds__(kWgThreads, 8) void pgd_l2_fused_kernel(const float *__restrict__ adv, const float *__restrict__ grad,
                                                                 const float *__restrict__ orig, float *out, int64_t T,
                                                                 float alpha, float eps, float eps_div, float lo, float hi,
                                                                 unsigned long long *__restrict__ gran_g,
                                                                 unsigned long long *__restrict__ gran_d,
                                                                 unsigned *__restrict__ fail,
                                                                 const unsigned *__restrict__ epoch, unsigned spin_limit,
                                                                 float *__restrict__ gnorm, float *__restrict__ dnorm) {
    __shared__ float4 xs[kTileVec];
    __shared__ float lds[12];
    __shared__ int failed;
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 a[kVecs], g[kVecs];
    {
        float4 x[kVecs];
        load_tile<VEC>(orig + b * T, T, tile, 0.0f, x);
#pragma unroll
        for (int j = 0; j < kVecs; ++j) xs[j * kWgThreads + threadIdx.x] = x[j];      // each thread reads back only its own slots
    }
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
    load_tile<VEC>(grad + b * T, T, tile, 0.0f, g);
    float s = wg_sum(tile_sumsq(g), lds);
    const unsigned base = exchange_tag_base(epoch);
    const float gsq = row_exchange_sum(gran_g + b * C, C, tile, s, base, 1u, spin_limit, lds + 4, &failed);
    if (failed) {
        row_exchange_abandon(fail, b, gran_g + b * C, gran_d + b * C, tile, base);
        return;
    }
    const float gn_raw = sqrtf(gsq);
    const float gn = gn_raw + eps_div;
    s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j)
        s += sumsq4(zero_outside_row(l2_move4(a[j], g[j], xs[j * kWgThreads + threadIdx.x], alpha, gn), T, quad_of(tile, j)));
    s = wg_sum(s, lds + 8);
    const float dn = sqrtf(row_exchange_sum(gran_d + b * C, C, tile, s, base, 2u, spin_limit, lds + 4, &failed));
    if (failed) {
        row_exchange_abandon(fail, b, nullptr, gran_d + b * C, tile, base);
        return;
    }
    const float f = l2_scale_factor<false>(dn, eps);
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {      // d recomputed (l2_move4 again: same bits) rather than kept across the exchange
        const float4 x = xs[j * kWgThreads + threadIdx.x];
        a[j] = l2_project4(x, l2_move4(a[j], g[j], x, alpha, gn), f, lo, hi);
    }
    store_tile<VEC>(out + b * T, T, tile, a);
    if (tile == 0 && threadIdx.x == 0) {
        if (gnorm) gnorm[b] = gn_raw;
        if (dnorm) dnorm[b] = dn;
    }
}

// The repair kernel queued behind every single-pass launch also closes the call: it moves the row's flag to `last` (diagnostics),
// lowers it, and workgroup 0 advances the workspace's epoch word — after which no granule of this call carries a valid tag.
// Contract (include/advstep.h): the caller zero-fills a workspace once, before its first use (stale FLAGS would send rows to
// the repair pass: slow, not wrong).  Granules need no cleaning and the float partial planes of the other entry points do not
// overlap the exchange area of the same (B, T); a word left by a call of ANOTHER shape is consumed only if it equals this
// call's 32-bit tag at the moment a sibling looks — the epoch makes that a coincidence, not a pattern (the cleaned
// granules of round 4 could meet `last[b] = 1` of another layout, and 1 was a phase tag).
// Returns the row's flag (workgroup-uniform).
__device__ __forceinline__ unsigned take_flag(unsigned *fail, unsigned *last, unsigned *epoch, int64_t b) {
    __shared__ unsigned flag_s;
    if (threadIdx.x == 0) {
        flag_s = fail[b];
        last[b] = flag_s ? kRowFlagged : 0u;
        fail[b] = 0u;
        if (b == 0) *epoch = *epoch + 1u;          // single writer; the next launch on this stream reads it
    }
    __syncthreads();
    return flag_s;
}

// Repair pass of the single-pass step: one workgroup per row, returns at once unless the row's flag is up.  The row's tiles
// are visited in sequence with the three-kernel path's own expressions (row_tiles.h's per-quad helpers) and reductions, so a
// repaired row carries the same bits as any other.  adv / orig / grad are re-read from global memory:
// the single-pass path is not taken when `out` aliases an input.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void pgd_l2_repair_kernel(const float *__restrict__ adv, const float *__restrict__ grad,
                                                               const float *__restrict__ orig, float *out, int64_t T, int C,
                                                               float alpha, float eps, float eps_div, float lo, float hi,
                                                               unsigned *fail, unsigned *last, unsigned *epoch,
                                                               float *__restrict__ gnorm, float *__restrict__ dnorm) {
    const int64_t b = blockIdx.x;
    if (!take_flag(fail, last, epoch, b)) return;
    __shared__ float gpart[64], dpart[64], lds[12];
    float4 a[kVecs], g[kVecs], x[kVecs];
    for (int tile = 0; tile < C; ++tile) {
        load_tile<VEC>(grad + b * T, T, tile, 0.0f, g);
        const float s = wg_sum(tile_sumsq(g), lds);
        if (threadIdx.x == 0) gpart[tile] = s;
        __syncthreads();
    }
    const float gn_raw = sqrtf(row_sum(gpart, C, lds + 4));
    const float gn = gn_raw + eps_div;
    for (int tile = 0; tile < C; ++tile) {
        load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
        load_tile<VEC>(grad + b * T, T, tile, 0.0f, g);
        load_tile<VEC>(orig + b * T, T, tile, 0.0f, x);
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < kVecs; ++j) s += sumsq4(zero_outside_row(l2_move4(a[j], g[j], x[j], alpha, gn), T, quad_of(tile, j)));
        s = wg_sum(s, lds);
        if (threadIdx.x == 0) dpart[tile] = s;
        __syncthreads();
    }
    const float dn = sqrtf(row_sum(dpart, C, lds + 8));
    const float f = l2_scale_factor<false>(dn, eps);
    for (int tile = 0; tile < C; ++tile) {
        load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
        load_tile<VEC>(grad + b * T, T, tile, 0.0f, g);
        load_tile<VEC>(orig + b * T, T, tile, 0.0f, x);
#pragma unroll
        for (int j = 0; j < kVecs; ++j) a[j] = l2_project4(x[j], l2_move4(a[j], g[j], x[j], alpha, gn), f, lo, hi);
        store_tile<VEC>(out + b * T, T, tile, a);
    }
    if (threadIdx.x == 0) {
        if (gnorm) gnorm[b] = gn_raw;
        if (dnorm) dnorm[b] = dn;
    }
}

// rows whose flag is up (diagnostics / tests: how often the repair pass had work)
__global__ __launch_bounds__(64) void count_flags_kernel(const unsigned *__restrict__ fail, int64_t B, int *__restrict__ count) {
    int n = 0;
    for (int64_t i = threadIdx.x; i < B; i += 64) n += fail[i] == kRowFlagged;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (threadIdx.x == 0) *count = n;
}

// ---- a6: PGD-L2 random start -----------------------------------------------------------------------------------

// explicit draws: out = clamp(x + normal * ((r / nrm) * eps), lo, hi)
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void pgd_l2_init_noise_kernel(const float *__restrict__ x,
                                                                   const float *__restrict__ normal,
                                                                   const float *__restrict__ r, float *out, int64_t T,
                                                                   float eps, float lo, float hi,
                                                                   const float *__restrict__ npart) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 xv[kVecs], nz[kVecs];
    load_tile<VEC>(x + b * T, T, tile, 0.0f, xv);
    load_tile<VEC>(normal + b * T, T, tile, 0.0f, nz);
    const float nrm = sqrtf(row_sum(npart + b * C, C, lds));
    const float scale = (r[b] / nrm) * eps;
    l2_start_apply(xv, nz, scale, lo, hi);
    store_tile<VEC>(out + b * T, T, tile, xv);
}

// (philox_normal_tile, philox_start_scale and l2_start_apply are row_tiles.h's)

__global__ __launch_bounds__(kWgThreads) void philox_normal_sumsq_kernel(int64_t T, uint64_t seed, uint64_t offset,
                                                                     float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 nz[kVecs];
    philox_normal_tile(T, tile, (uint32_t)b, seed, offset, nz);
    const float s = wg_sum(tile_sumsq(nz), lds);
    if (threadIdx.x == 0) part[b * C + tile] = s;
}

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void pgd_l2_init_philox_kernel(const float *__restrict__ x, float *out,
                                                                    int64_t T, float eps, float lo, float hi,
                                                                    uint64_t seed, uint64_t offset,
                                                                    const float *__restrict__ npart) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 xv[kVecs], nz[kVecs];
    load_tile<VEC>(x + b * T, T, tile, 0.0f, xv);
    philox_normal_tile(T, tile, (uint32_t)b, seed, offset, nz);
    const float nrm = sqrtf(row_sum(npart + b * C, C, lds));
    const float scale = philox_start_scale(b, seed, offset, nrm, eps);
    l2_start_apply(xv, nz, scale, lo, hi);
    store_tile<VEC>(out + b * T, T, tile, xv);
}

// The same start in ONE launch: the normals are generated once and stay in registers across the row exchange of ||n||^2
// (granule protocol of pgd_l2_fused_kernel; same partial sums and re-reduction as the two-kernel path: bit-identical).
template <bool VEC>
__global__ __launch_bounds__(kWgThreads, 8) void pgd_l2_init_philox_fused_kernel(const float *__restrict__ x, float *out, int64_t T,
                                                                             float eps, float lo, float hi, uint64_t seed,
                                                                             uint64_t offset,
                                                                             unsigned long long *__restrict__ gran,
                                                                             unsigned *__restrict__ fail,
                                                                             const unsigned *__restrict__ epoch,
                                                                             unsigned spin_limit) {
    __shared__ float lds[8];
    __shared__ int failed;
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 nz[kVecs];
    philox_normal_tile(T, tile, (uint32_t)b, seed, offset, nz);
    const float s = wg_sum(tile_sumsq(nz), lds);
    // the tile of x is requested BEFORE the exchange (16-byte path): its HBM latency then runs under the wait for the row's other
    // workgroups; the scalar path (rows not 16-byte addressable) keeps it behind - 16 more live registers make it spill
    float4 xv[kVecs];
    if constexpr (VEC) load_tile<VEC>(x + b * T, T, tile, 0.0f, xv);
    const unsigned base = exchange_tag_base(epoch);
    const float nrm = sqrtf(row_exchange_sum(gran + b * C, C, tile, s, base, 1u, spin_limit, lds + 4, &failed));
    if (failed) {
        row_exchange_abandon(fail, b, gran + b * C, nullptr, tile, base);
        return;
    }
    const float scale = philox_start_scale(b, seed, offset, nrm, eps);
    if constexpr (!VEC) load_tile<VEC>(x + b * T, T, tile, 0.0f, xv);
    l2_start_apply(xv, nz, scale, lo, hi);
    store_tile<VEC>(out + b * T, T, tile, xv);
}

// Repair pass of the single-pass start (see pgd_l2_repair_kernel): the two-kernel path's arithmetic, one workgroup per
// flagged row.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void pgd_l2_init_philox_repair_kernel(const float *__restrict__ x, float *out, int64_t T, int C,
                                                                           float eps, float lo, float hi, uint64_t seed,
                                                                           uint64_t offset, unsigned *fail, unsigned *last,
                                                                           unsigned *epoch) {
    const int64_t b = blockIdx.x;
    if (!take_flag(fail, last, epoch, b)) return;
    __shared__ float npart[64], lds[8];
    float4 nz[kVecs], xv[kVecs];
    for (int tile = 0; tile < C; ++tile) {
        philox_normal_tile(T, tile, (uint32_t)b, seed, offset, nz);
        const float s = wg_sum(tile_sumsq(nz), lds);
        if (threadIdx.x == 0) npart[tile] = s;
        __syncthreads();
    }
    const float nrm = sqrtf(row_sum(npart, C, lds + 4));
    const float scale = philox_start_scale(b, seed, offset, nrm, eps);
    for (int tile = 0; tile < C; ++tile) {
        load_tile<VEC>(x + b * T, T, tile, 0.0f, xv);
        philox_normal_tile(T, tile, (uint32_t)b, seed, offset, nz);
        l2_start_apply(xv, nz, scale, lo, hi);
        store_tile<VEC>(out + b * T, T, tile, xv);
    }
}

// ---- a7: CW -------------------------------------------------------------------------------------------------------

// adv = 1/2 * (tanh(w) + 1); partial sum (adv - x)^2
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void cw_tanh_sqdist_kernel(const float *__restrict__ w,
                                                                const float *__restrict__ x, float *adv, int64_t T,
                                                                float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 wv[kVecs], xv[kVecs];
    load_tile<VEC>(w + b * T, T, tile, 0.0f, wv);
    // fill = 0.5 == tanh_space(0): out-of-row lanes contribute (0.5 - 0.5)^2 = 0
    load_tile<VEC>(x + b * T, T, tile, 0.5f, xv);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        wv[j].x = 0.5f * (tanhf(wv[j].x) + 1.0f);
        wv[j].y = 0.5f * (tanhf(wv[j].y) + 1.0f);
        wv[j].z = 0.5f * (tanhf(wv[j].z) + 1.0f);
        wv[j].w = 0.5f * (tanhf(wv[j].w) + 1.0f);
        const float dx = wv[j].x - xv[j].x, dy = wv[j].y - xv[j].y, dz = wv[j].z - xv[j].z, dw = wv[j].w - xv[j].w;
        s += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    store_tile<VEC>(adv + b * T, T, tile, wv);
    s = wg_sum(s, lds);
    if (threadIdx.x == 0) part[b * C + tile] = s;
}

// one wave per row: l2[b] = sum of the row's partials
__global__ __launch_bounds__(64) void row_partials_sum_kernel(const float *__restrict__ part, int C,
                                                              float *__restrict__ out) {
    const int64_t b = blockIdx.x;
    float v = 0.0f;
    for (int i = threadIdx.x; i < C; i += 64) v += part[b * C + i];
    v = wave_reduce(v, SumOp());
    if (threadIdx.x == 0) out[b] = v;
}

// best = mask * adv + (1 - mask) * best
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void cw_best_update_kernel(const float *__restrict__ adv,
                                                                const float *__restrict__ mask, float *best,
                                                                int64_t T) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    const float mk = mask[b];
    const float inv = 1.0f - mk;
    float4 a[kVecs], bs[kVecs];
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
    load_tile<VEC>(best + b * T, T, tile, 0.0f, bs);
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        bs[j].x = mk * a[j].x + inv * bs[j].x;
        bs[j].y = mk * a[j].y + inv * bs[j].y;
        bs[j].z = mk * a[j].z + inv * bs[j].z;
        bs[j].w = mk * a[j].w + inv * bs[j].w;
    }
    store_tile<VEC>(best + b * T, T, tile, bs);
}

// ---- a8: 2-logit cross-entropy, closed form ------------------------------------------------------------------------

__global__ __launch_bounds__(kWgThreads) void ce2_loss_grad_kernel(const float *__restrict__ z,
                                                               const int64_t *__restrict__ labels,
                                                               float *__restrict__ dz, float *__restrict__ loss,
                                                               int64_t B, float scale) {
    __shared__ float lds[4];
    const float invB = 1.0f / (float)B;
    float acc = 0.0f;
    for (int64_t b = threadIdx.x; b < B; b += kWgThreads) {
        // CE([-z, z], y) = softplus(u), u = (1 - 2y) * 2z;  d/dz = (1 - 2y) * 2 * sigmoid(u).
        // (sigmoid(2z) - y written without the cancellation at saturated logits.)
        const float flip = 1.0f - 2.0f * (float)labels[b];
        const float u = flip * (2.0f * z[b]);
        acc += softplusf(u);
        const float sig = 1.0f / (1.0f + expf(-u));
        dz[b] = scale * ((2.0f * invB) * (flip * sig));
    }
    acc = wg_sum(acc, lds);
    if (threadIdx.x == 0) loss[0] = scale * (acc * invB);
}

// ---------------------------------------------------------------------------------------------------------
// host-side helpers
// ---------------------------------------------------------------------------------------------------------

// ADVSTEP_L2_SINGLE_PASS=0 keeps the three-kernel PGD-L2 step (A/B measurements, read at every call); default on.
inline bool l2_single_pass() {
    const char *e = getenv("ADVSTEP_L2_SINGLE_PASS");
    return !(e && e[0] == '0');
}

// Bound of the in-launch wait, in sweeps (one sweep = an agent-scope load + s_sleep, ~1 us): ~0.1 s, after which the row goes
// to the repair pass.  ADVSTEP_L2_SPIN_LIMIT overrides it (0 = every row gives up at once: tests of the repair pass).
inline unsigned l2_spin_limit() {
    const char *e = getenv("ADVSTEP_L2_SPIN_LIMIT");
    if (e && *e) return (unsigned)strtoul(e, nullptr, 10);
    return 1u << 17;
}

// How many workgroups of `kernel` (kWgThreads threads, its static LDS) the CURRENT device holds at once: CU count x the
// occupancy the runtime computes for this kernel's registers / LDS.  Queried once per (device, kernel); 0 if the query
// fails (the caller then takes the multi-kernel path).  ADVSTEP_L2_CAPACITY overrides it (tests: a "smaller device").
enum { kCapStepVec, kCapStepScalar, kCapInitVec, kCapInitScalar, kCapKinds };
inline int64_t l2_resident_capacity(int kind, const void *kernel) {
    const char *e = getenv("ADVSTEP_L2_CAPACITY");
    if (e && *e) return (int64_t)strtoll(e, nullptr, 10);
    static std::atomic<int64_t> cache[kCapKinds][64];      // zero-initialised: 0 = not queried yet, -1 = query failed
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int64_t c = cache[kind][dev].load(std::memory_order_relaxed);
    if (c == 0) {
        int cus = 0, per_cu = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kWgThreads, 0) == hipSuccess && cus > 0 && per_cu > 0)
            c = (int64_t)cus * per_cu;
        else
            c = -1;
        (void)hipGetLastError();
        cache[kind][dev].store(c, std::memory_order_relaxed);
    }
    return c > 0 ? c : 0;
}

// float4 per thread per stream of the flat kernels.  Measured on MI355X at B = 128, T = 64 600 (tools/tune_pgd_step.hip,
// profiles/): one float4 per stream per thread (8 076 workgroups) beats 4 (2 019 workgroups) by 3 % hot / 7 % cold.
// ADVSTEP_FLAT_VECS = 1 | 2 | 4 overrides it for experiments.
inline int flat_vecs() {
    static const int v = [] {
        const char *e = getenv("ADVSTEP_FLAT_VECS");
        const int x = e ? atoi(e) : 1;
        return (x == 1 || x == 2 || x == 4) ? x : 1;
    }();
    return v;
}

// The repair kernel behind a single-pass launch: one workgroup per row.
template <class... P, class... A>
void launch_row_repair(void (*const (&pair)[2])(P...), bool vec, int64_t B, hipStream_t st, A... args) {
    hipLaunchKernelGGL(pair[vec], dim3((unsigned)B), dim3(kWgThreads), 0, st, args...);
}

template <int NIN, int VECS, class Op>
void launch_flat_vec(const float *in0, const float *in1, const float *in2, float *out, int64_t n4, Op op,
                     hipStream_t st) {
    const int64_t ntiles = ceil_div(n4, kWgThreads * VECS);
    const int64_t cap = (int64_t)kMaxGrid * (4 / VECS);
    const int grid = (int)(ntiles < cap ? ntiles : cap);
    hipLaunchKernelGGL((flat_vec_kernel<NIN, VECS, Op>), dim3(grid), dim3(kWgThreads), 0, st,
                       reinterpret_cast<const float4 *>(in0), reinterpret_cast<const float4 *>(in1),
                       reinterpret_cast<const float4 *>(in2), reinterpret_cast<float4 *>(out), n4, ntiles, op);
}

template <int NIN, class Op>
int launch_flat(const float *in0, const float *in1, const float *in2, float *out, int64_t n, Op op,
                hipStream_t st) {
    if (n == 0) return ADVSTEP_OK;
    const bool vec = aligned16(in0) && aligned16(out) && (NIN < 2 || aligned16(in1)) && (NIN < 3 || aligned16(in2));
    const int64_t n4 = vec ? n / 4 : 0;
    if (n4 > 0) {
        switch (flat_vecs()) {
            case 4: launch_flat_vec<NIN, 4>(in0, in1, in2, out, n4, op, st); break;
            case 2: launch_flat_vec<NIN, 2>(in0, in1, in2, out, n4, op, st); break;
            default: launch_flat_vec<NIN, 1>(in0, in1, in2, out, n4, op, st); break;
        }
    }
    const int64_t begin = n4 * 4;
    if (begin < n) {
        const int64_t blocks = ceil_div(n - begin, kWgThreads);
        const int grid = (int)(blocks < kMaxGrid ? blocks : kMaxGrid);
        hipLaunchKernelGGL((flat_scalar_kernel<NIN, Op>), dim3(grid), dim3(kWgThreads), 0, st, in0, in1, in2, out, begin,
                           n, op);
    }
    return status_after_launch();
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------

extern "C" {

int advstep_abi_version(void) { return ADVSTEP_ABI_VERSION; }

const char *advstep_status_string(int status) {
    switch (status) {
        case ADVSTEP_OK: return "ok";
        case ADVSTEP_EINVAL: return "invalid argument";
        case ADVSTEP_EWORKSPACE: return "row workspace missing, misaligned or too small";
        case ADVSTEP_ELAUNCH: return "HIP kernel launch failed";
        case ADVSTEP_ENODEVICE: return "no HIP device";
        default: return "unknown status";
    }
}

int advstep_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

size_t advstep_row_workspace_bytes(int64_t B, int64_t T) {
    if (B <= 0 || T <= 0) return 0;
    return row_ws_bytes(B, T);
}

int advstep_minmax_normalize_f32(const float *x, float *x01, float *mn, float *mx, int64_t B, int64_t T, void *ws,
                                 size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && x01 && mn && mx && x != x01);
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {x, x01});
    const int C = ws_tiles_per_row(T);
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(minmax_partial_kernel), vec, nb, T, st, x + b0 * T, T, w.p0 + b0 * C, w.p1 + b0 * C);
    });
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(minmax_apply_kernel), vec, nb, T, st, x + b0 * T, x01 + b0 * T, mn + b0, mx + b0, T,
                     w.p0 + b0 * C, w.p1 + b0 * C);
    });
    return status_after_launch();
}

int advstep_minmax_revert_f32(const float *x01, const float *mn, const float *mx, float *out, int64_t B, int64_t T,
                              advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x01 && mn && mx && out);
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {x01, out});
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(minmax_revert_kernel), vec, nb, T, st, x01 + b0 * T, mn + b0, mx + b0, out + b0 * T, T);
    });
    return status_after_launch();
}

int advstep_fgsm_step_f32(const float *x, const float *grad, float *out, int64_t n, float eps, float lo, float hi,
                          advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && grad && out);
    return launch_flat<2>(x, grad, nullptr, out, n, FgsmOp{eps, lo, hi}, as_stream(stream));
}

int advstep_pgd_linf_init_noise_f32(const float *x, const float *noise, float *out, int64_t n, float lo, float hi,
                                    advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && noise && out);
    return launch_flat<2>(x, noise, nullptr, out, n, AddClampOp{lo, hi}, as_stream(stream));
}

int advstep_pgd_linf_init_philox_f32(const float *x, float *out, int64_t n, float eps, float lo, float hi,
                                     uint64_t seed, uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && out);
    hipStream_t st = as_stream(stream);
    const bool vec = aligned16(x) && aligned16(out);
    const int64_t n4 = vec ? n / 4 : 0;
    if (n4 > 0) {
        const int64_t ntiles = ceil_div(n4, kTileVec);
        const int grid = (int)(ntiles < kMaxGrid ? ntiles : kMaxGrid);
        hipLaunchKernelGGL(pgd_linf_init_philox_vec_kernel, dim3(grid), dim3(kWgThreads), 0, st,
                           reinterpret_cast<const float4 *>(x), reinterpret_cast<float4 *>(out), n4, ntiles, eps, lo,
                           hi, seed, offset);
    }
    const int64_t begin = n4 * 4;
    if (begin < n) {
        const int64_t blocks = ceil_div(n - begin, kWgThreads);
        const int grid = (int)(blocks < kMaxGrid ? blocks : kMaxGrid);
        hipLaunchKernelGGL(pgd_linf_init_philox_scalar_kernel, dim3(grid), dim3(kWgThreads), 0, st, x, out, begin, n, eps,
                           lo, hi, seed, offset);
    }
    return status_after_launch();
}

int advstep_pgd_linf_step_f32(const float *adv, const float *grad, const float *orig, float *out, int64_t n,
                              float alpha, float eps, float lo, float hi, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && grad && orig && out);
    return launch_flat<3>(adv, grad, orig, out, n, PgdLinfOp{alpha, eps, lo, hi}, as_stream(stream));
}

int advstep_pgd_l2_init_noise_f32(const float *x, const float *normal, const float *r, float *out, int64_t B,
                                  int64_t T, float eps, float lo, float hi, void *ws, size_t ws_bytes,
                                  advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && normal && r && out);
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {x, normal, out});
    const int C = ws_tiles_per_row(T);
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(sumsq_partial_kernel), vec, nb, T, st, normal + b0 * T, T, w.p0 + b0 * C);
    });
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(pgd_l2_init_noise_kernel), vec, nb, T, st, x + b0 * T, normal + b0 * T, r + b0, out + b0 * T, T,
                     eps, lo, hi, w.p0 + b0 * C);
    });
    return status_after_launch();
}

int advstep_pgd_l2_init_philox_f32(const float *x, float *out, int64_t B, int64_t T, float eps, float lo, float hi,
                                   uint64_t seed, uint64_t offset, void *ws, size_t ws_bytes,
                                   advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && out);
    ADVSTEP_REQUIRE(B <= kMaxGridY);  // the Philox counter carries the absolute row index
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {x, out});
    const int C = ws_tiles_per_row(T);
    static constexpr decltype(&pgd_l2_init_philox_fused_kernel<true>) fused[2] = ROW_KERNEL_PAIR(pgd_l2_init_philox_fused_kernel);
    if (l2_single_pass() && C <= 64 && !overlaps(x, out, (size_t)B * T * sizeof(float)) &&
        B * C <= l2_resident_capacity(vec ? kCapInitVec : kCapInitScalar, (const void *)fused[vec])) {
        // the repair kernel behind the launch serves flagged rows, lowers their flags and advances the epoch (closes the call)
        launch_tiles(fused, vec, B, T, st, x, out, T, eps, lo, hi, seed, offset, w.gran0, w.fail, w.epoch, l2_spin_limit());
        launch_row_repair(ROW_KERNEL_PAIR(pgd_l2_init_philox_repair_kernel), vec, B, st, x, out, T, C, eps, lo, hi, seed, offset,
                          w.fail, w.last, w.epoch);
        return status_after_launch();
    }
    hipLaunchKernelGGL(philox_normal_sumsq_kernel, dim3(C, (unsigned)B), dim3(kWgThreads), 0, st, T, seed, offset, w.p0);
    launch_tiles(ROW_KERNEL_PAIR(pgd_l2_init_philox_kernel), vec, B, T, st, x, out, T, eps, lo, hi, seed, offset, w.p0);
    return status_after_launch();
}

int advstep_pgd_l2_step_f32(const float *adv, const float *grad, const float *orig, float *out, int64_t B, int64_t T,
                            float alpha, float eps, float eps_div, float lo, float hi, float *gnorm, float *dnorm,
                            void *ws, size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && grad && orig && out);
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {adv, grad, orig, out});
    const int C = ws_tiles_per_row(T);
    static constexpr decltype(&pgd_l2_fused_kernel<true>) fused[2] = ROW_KERNEL_PAIR(pgd_l2_fused_kernel);
    const size_t row_bytes = (size_t)B * T * sizeof(float);
    if (l2_single_pass() && C <= 64 && !overlaps(adv, out, row_bytes) && !overlaps(grad, out, row_bytes) &&
        !overlaps(orig, out, row_bytes) &&
        B * C <= l2_resident_capacity(vec ? kCapStepVec : kCapStepScalar, (const void *)fused[vec])) {
        // the launch fits the device's resident capacity for this kernel: one launch, 16 B per sample; the repair kernel behind
        // it serves rows whose exchange was abandoned, lowers their flags and advances the epoch (no memset node, nothing cleaned)
        launch_tiles(fused, vec, B, T, st, adv, grad, orig, out, T, alpha, eps, eps_div, lo, hi, w.gran0, w.gran1, w.fail, w.epoch,
                     l2_spin_limit(), gnorm, dnorm);
        launch_row_repair(ROW_KERNEL_PAIR(pgd_l2_repair_kernel), vec, B, st, adv, grad, orig, out, T, C, alpha, eps, eps_div, lo, hi,
                          w.fail, w.last, w.epoch, gnorm, dnorm);
        return status_after_launch();
    }
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(sumsq_partial_kernel), vec, nb, T, st, grad + b0 * T, T, w.p0 + b0 * C);
    });
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(pgd_l2_delta_kernel), vec, nb, T, st, adv + b0 * T, grad + b0 * T, orig + b0 * T, T, alpha,
                     eps_div, w.p0 + b0 * C, w.p1 + b0 * C, gnorm ? gnorm + b0 : nullptr);
    });
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(pgd_l2_project_kernel), vec, nb, T, st, adv + b0 * T, grad + b0 * T, orig + b0 * T,
                     out + b0 * T, T, alpha, eps, eps_div, lo, hi, w.p0 + b0 * C, w.p1 + b0 * C, dnorm ? dnorm + b0 : nullptr);
    });
    return status_after_launch();
}

int advstep_pgd_l2_repaired_rows(const void *ws, size_t ws_bytes, int64_t B, int64_t T, int *count,
                                 advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && count);
    if (B == 0 || T == 0) return hipMemsetAsync(count, 0, sizeof(int), as_stream(stream)) == hipSuccess ? ADVSTEP_OK : ADVSTEP_ELAUNCH;
    if (!ws || !aligned16(ws) || ws_bytes < row_ws_bytes(B, T)) return ADVSTEP_EWORKSPACE;
    RowWs w;
    carve_ws(const_cast<void *>(ws), ws_bytes, B, T, &w);
    hipLaunchKernelGGL(count_flags_kernel, dim3(1), dim3(64), 0, as_stream(stream), (const unsigned *)w.last, B, count);
    return status_after_launch();
}

int advstep_cw_init_w_f32(const float *x, float *w, int64_t n, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && w);
    return launch_flat<1>(x, nullptr, nullptr, w, n, CwInitOp{}, as_stream(stream));
}

int advstep_cw_tanh_sqdist_f32(const float *w, const float *x, float *adv, float *l2, int64_t B, int64_t T, void *ws,
                               size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(w && x && adv && l2);
    RowWs wsp;
    if (!carve_ws(ws, ws_bytes, B, T, &wsp)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {w, x, adv});
    const int C = ws_tiles_per_row(T);
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(cw_tanh_sqdist_kernel), vec, nb, T, st, w + b0 * T, x + b0 * T, adv + b0 * T, T,
                     wsp.p0 + b0 * C);
    });
    hipLaunchKernelGGL(row_partials_sum_kernel, dim3((unsigned)B), dim3(64), 0, st, wsp.p0, C, l2);
    return status_after_launch();
}

int advstep_cw_adam_step_f32(float *w, float *m, float *v, const float *x, const float *grad_adv, int64_t n,
                             int64_t step, double lr, double beta1, double beta2, double adam_eps,
                             advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0 && step >= 1);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(w && m && v && x && grad_adv);
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    AdamScalars s;
    s.w1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.omb2 = (float)(1.0 - beta2);
    s.neg_step = (float)(-(lr / bc1));
    s.bc2_sqrt = (float)sqrt(bc2);
    s.eps = (float)adam_eps;
    hipStream_t st = as_stream(stream);
    const bool vec = aligned16(w) && aligned16(m) && aligned16(v) && aligned16(x) && aligned16(grad_adv);
    const int64_t n4 = vec ? n / 4 : 0;
    if (n4 > 0) {
        const int64_t ntiles = ceil_div(n4, kTileVec);
        const int grid = (int)(ntiles < kMaxGrid ? ntiles : kMaxGrid);
        hipLaunchKernelGGL(cw_adam_vec_kernel, dim3(grid), dim3(kWgThreads), 0, st, reinterpret_cast<float4 *>(w),
                           reinterpret_cast<float4 *>(m), reinterpret_cast<float4 *>(v),
                           reinterpret_cast<const float4 *>(x), reinterpret_cast<const float4 *>(grad_adv), n4, ntiles,
                           s);
    }
    const int64_t begin = n4 * 4;
    if (begin < n) {
        const int64_t blocks = ceil_div(n - begin, kWgThreads);
        const int grid = (int)(blocks < kMaxGrid ? blocks : kMaxGrid);
        hipLaunchKernelGGL(cw_adam_scalar_kernel, dim3(grid), dim3(kWgThreads), 0, st, w, m, v, x, grad_adv, begin, n, s);
    }
    return status_after_launch();
}

int advstep_cw_best_update_f32(const float *adv, const float *mask, float *best, int64_t B, int64_t T,
                               advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && mask && best);
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {adv, best});
    for_row_slabs(B, [&](int64_t b0, int64_t nb) {
        launch_tiles(ROW_KERNEL_PAIR(cw_best_update_kernel), vec, nb, T, st, adv + b0 * T, mask + b0, best + b0 * T, T);
    });
    return status_after_launch();
}

int advstep_ce2_loss_grad_f32(const float *z, const int64_t *labels, float *dz, float *loss, int64_t B, float scale,
                              advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 1);
    ADVSTEP_REQUIRE(z && labels && dz && loss);
    hipLaunchKernelGGL(ce2_loss_grad_kernel, dim3(1), dim3(kWgThreads), 0, as_stream(stream), z, labels, dz, loss, B,
                       scale);
    return status_after_launch();
}

}  // extern "C"
