// row_workgroup.h — the one-workgroup-per-row geometry of fab.hip, apgdl1.hip, l0.hip and fmn_sparse.hip (internal: not part of the C ABI in include/).
//
// One workgroup of kRow = 1024 threads (16 wave64) owns one row of T samples and makes several passes over it; at the repo's
// T = 64 600 a row is 258 KB: it does not fit LDS, but stays L2 / Infinity-Cache resident between the passes, so only the first
// pass reads HBM.  This header holds what those kernels share: the 16-wave reduction, the row traversal (whose order is part of
// every reduced result's bits), the digit-walk search behind every per-row threshold (digit_search, bucket_add: FAB's greedy L1
// key, l1-APGD's lambda and top-k rank, L0's k-th score and index cut) and the launch helper.  Include after advstep_common.h
// (wave_reduce, SumOp, ROW_KERNEL_PAIR, status_after_launch, kMaxGridY).  The 256-thread (tile, row) geometry of the other
// attack files is row_tiles.h.

#ifndef ADVSTEP_ROW_WORKGROUP_H
#define ADVSTEP_ROW_WORKGROUP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "advstep_common.h"

namespace {

constexpr int kRow = 1024;       // threads per row workgroup
constexpr int kRowWaves = kRow / 64;

// Reduce NV per-thread values over the 1024-thread workgroup with advstep_common.h's wave_reduce, then one LDS slot per wave and
// value, combined as ((w0 . w1) . w2) ... w15; every thread receives the results.  Against wg_reduce: 16 waves instead of 4, NV
// values per barrier pair (lds: NV * kRowWaves floats), and a trailing barrier that frees the slots, so two calls in a row may
// use the same ones.
template <int NV, class Op>
__device__ __forceinline__ void row_reduce(float (&v)[NV], Op op, float *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const float x = wave_reduce(v[k], op);
        if (lane == 0) lds[k * kRowWaves + wave] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float r = lds[k * kRowWaves];
#pragma unroll
        for (int w = 1; w < kRowWaves; ++w) r = op(r, lds[k * kRowWaves + w]);
        v[k] = r;
    }
    __syncthreads();
}

// The one row traversal: f(a_i, b_i, ...) over the samples of the N rows `in`, or f(i, a_i, b_i, ...) where f takes the sample
// index.  The index form is chosen iff f is callable with N + 1 arguments, so f must have a fixed arity (no generic lambda).
// ROUTE (a kernel's bool VEC converts to the first two): kRouteQuads: quads q = threadIdx.x, += kRow, lanes x, y, z, w in order,
// one float4 load per row; kRouteSamples: samples i = threadIdx.x, += kRow; kRouteQuadsBySample (fmn_sparse.hip, T % 4 == 0 with
// a base that is not 16-byte aligned): the quads' sample -> thread map and order with four 4-byte accesses per quad, so every
// reduced result has kRouteQuads' bits.  That order is each thread's accumulation order, so part of every reduced result's bits.
// STORE: out_i = f(...), one store per quad after all of the quad's loads.  out may alias an input (no __restrict__).
enum : int { kRouteSamples = 0, kRouteQuads = 1, kRouteQuadsBySample = 2 };
static_assert((int)false == kRouteSamples && (int)true == kRouteQuads, "a kernel's VEC selects the first two routes");

template <int ROUTE>
__device__ __forceinline__ float4 load_quad(const float *p, int64_t q) {
    if constexpr (ROUTE == kRouteQuads) return reinterpret_cast<const float4 *>(p)[q];
    else return make_float4(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
}
template <int ROUTE>
__device__ __forceinline__ void store_quad(float *p, int64_t q, float4 v) {
    if constexpr (ROUTE == kRouteQuads) {
        reinterpret_cast<float4 *>(p)[q] = v;
    } else {
        p[4 * q] = v.x;
        p[4 * q + 1] = v.y;
        p[4 * q + 2] = v.z;
        p[4 * q + 3] = v.w;
    }
}

template <size_t>
using Sample = float;

template <int ROUTE, bool STORE, class F, size_t... K>
__device__ __forceinline__ void traverse(const float *const (&in)[sizeof...(K)], float *out, int64_t T, F f,
                                         std::index_sequence<K...>) {
    auto at = [&](int64_t i, Sample<K>... s) {
        if constexpr (std::is_invocable_v<F, int64_t, Sample<K>...>) return f(i, s...);
        else return f(s...);
    };
    if constexpr (ROUTE != kRouteSamples) {
        const int64_t n4 = T >> 2;
        for (int64_t q = threadIdx.x; q < n4; q += kRow) {
            const float4 v[] = {load_quad<ROUTE>(in[K], q)...};
            if constexpr (STORE) {
                float4 o;
                o.x = at(4 * q, v[K].x...);
                o.y = at(4 * q + 1, v[K].y...);
                o.z = at(4 * q + 2, v[K].z...);
                o.w = at(4 * q + 3, v[K].w...);
                store_quad<ROUTE>(out, q, o);
            } else {
                at(4 * q, v[K].x...);
                at(4 * q + 1, v[K].y...);
                at(4 * q + 2, v[K].z...);
                at(4 * q + 3, v[K].w...);
            }
        }
    } else {
        for (int64_t i = threadIdx.x; i < T; i += kRow) {
            if constexpr (STORE) out[i] = at(i, in[K][i]...);
            else at(i, in[K][i]...);
        }
    }
}
template <int ROUTE, size_t N, class F>
__device__ __forceinline__ void visit_rows(const float *const (&in)[N], int64_t T, F f) {
    traverse<ROUTE, false>(in, nullptr, T, f, std::make_index_sequence<N>());
}
template <int ROUTE, size_t N, class F>
__device__ __forceinline__ void map_rows(const float *const (&in)[N], float *out, int64_t T, F f) {
    traverse<ROUTE, true>(in, out, T, f, std::make_index_sequence<N>());
}

// visit_rows for the search passes of apgdl1.hip and l0.hip: f(s) with s[k] = the sample of row in[k], or f(i, s) where f takes
// the sample index, in visit_rows' order and sample -> thread map, but with the next element's loads issued before this
// element's arithmetic (with one quad per thread in flight a pass waits out a full L2 latency per quad).
template <int ROUTE, int N, class F>
__device__ __forceinline__ void visit_rows_ahead(const float *const (&in)[N], int64_t T, F f) {
    constexpr bool VEC = ROUTE != kRouteSamples;
    using Elem = std::conditional_t<VEC, float4, float>;
    auto load = [](const float *p, int64_t e) {
        if constexpr (VEC) return load_quad<ROUTE>(p, e);
        else return p[e];
    };
    auto at = [&](int64_t i, const float(&s)[N]) {
        if constexpr (std::is_invocable_v<F, int64_t, const float(&)[N]>) f(i, s);
        else f(s);
    };
    const int64_t n = VEC ? T >> 2 : T;
    int64_t e = threadIdx.x;
    Elem next[N];
    if (e < n) {
#pragma unroll
        for (int k = 0; k < N; ++k) next[k] = load(in[k], e);
    }
    for (; e < n; e += kRow) {
        Elem v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = next[k];
        if (e + kRow < n) {
#pragma unroll
            for (int k = 0; k < N; ++k) next[k] = load(in[k], e + kRow);
        }
        float s[N];
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < N; ++k) s[k] = v[k].x;
            at(4 * e, s);
#pragma unroll
            for (int k = 0; k < N; ++k) s[k] = v[k].y;
            at(4 * e + 1, s);
#pragma unroll
            for (int k = 0; k < N; ++k) s[k] = v[k].z;
            at(4 * e + 2, s);
#pragma unroll
            for (int k = 0; k < N; ++k) s[k] = v[k].w;
            at(4 * e + 3, s);
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) s[k] = v[k];
            at(e, s);
        }
    }
}

// ---- the digit-walk search: a per-row threshold without a sort -----------------------------------------------------------
//
// rho = the largest `bits`-bit pattern that a predicate, monotone in the pattern (true up to some pattern, false above it),
// still accepts; pattern 0 counts as accepted.  The bits are fixed from the top, kDigit at a time (the last digit takes what
// is left): one streaming pass over the row per digit fills kCand bins, bin j - 1 for the digit's candidate
// rho | j << shift, row_reduce sums them over the workgroup, and a scan takes the candidates in ascending order up to the
// first one refused.  31 bits (a non-negative float's pattern) are 11 passes, always all of them.
//
//   fill(rho, shift, h)  the caller's streaming pass: per-thread partial sums into the zeroed h.  Where bin j - 1 is to hold
//                        what the samples with pattern in [candidate j - 1, candidate j) contribute, that is
//                        bucket_add(h, key, rho, shift, v) per sample, and the scan accumulates.
//   accept(h[j - 1])     for j = 1 .. 2^(digit's bits) - 1, in order, until the first false; a running sum or count lives in
//                        the caller's capture and moves on only where the candidate is accepted.
//
// Contract.  The predicate is monotone in the candidate.  `bits`, and everything accept reads besides the reduced bins, are
// workgroup-uniform: every thread then picks the same digits, which also keeps the two barriers that row_reduce issues per
// pass convergent (lds: kCand * kRowWaves floats, free again on return).  Every pass's fill must give each sample to the same
// thread in the same order (visit_rows, visit_rows_ahead): a thread may then read back row samples it wrote itself with no
// further barrier, and the bins' bits do not depend on the pass.  h is left holding the last pass's reduced bins.
//
// The scan is one loop that indexes h by its counter on purpose.  Written so that the compiler peels its first iteration
// (`for j = 1 .. limit` with a separate pick), the sums of bins 1 .. 6 sink out of row_reduce into the scan's later blocks,
// 96 LDS words stay live across the barrier and every kernel with a search drops from 8 to 4 waves per SIMD
// (profiles/row_search_refactor_resource_usage.txt).

constexpr int kDigit = 3, kCand = (1 << kDigit) - 1;          // bits and candidates per streaming pass
constexpr int64_t kMaxRowLength = int64_t(1) << 24;            // per-row counts and indices are carried as exact floats

// v into the bin of the digit that `key` has at `shift` above rho; keys below rho belong to no candidate of this pass
__device__ __forceinline__ void bucket_add(float (&h)[kCand], uint32_t key, uint32_t rho, int shift, float v) {
    if (key >= rho) {
        const uint32_t q = (key - rho) >> shift;              // q > kCand - 1: above every candidate, no bin
#pragma unroll
        for (int k = 0; k < kCand; ++k) h[k] += (q == (uint32_t)k) ? v : 0.0f;
    }
}

template <class Fill, class Accept>
__device__ __forceinline__ uint32_t digit_search(int bits, float (&h)[kCand], float *lds, Fill fill, Accept accept) {
    uint32_t rho = 0;
    for (int top = bits; top > 0; top -= kDigit) {            // bits [shift, top) of the pattern
        const int shift = top >= kDigit ? top - kDigit : 0;
        const uint32_t limit = (1u << (top - shift)) - 1u;    // candidates j = 1 .. limit
#pragma unroll
        for (int k = 0; k < kCand; ++k) h[k] = 0.0f;
        fill(rho, shift, h);
        row_reduce<kCand>(h, SumOp(), lds);
        uint32_t pick = 0;
        while (pick < limit && accept(h[pick])) ++pick;
        rho |= pick << shift;
    }
    return rho;
}

inline unsigned grid_rows(int64_t rows) { return (unsigned)(rows < kMaxGridY ? rows : kMaxGridY); }

// One kRow-thread workgroup per row (the kernels stride on past kMaxGridY rows): k is a ROW_KERNEL_PAIR (advstep_common.h).
template <class... P, class... A>
int launch_rows(void (*const (&k)[2])(P...), bool vec, int64_t rows, advstep_stream_t stream, A... args) {
    hipLaunchKernelGGL(k[vec], dim3(grid_rows(rows)), dim3(kRow), 0, as_stream(stream), args...);
    return status_after_launch();
}

}  // namespace

#endif  // ADVSTEP_ROW_WORKGROUP_H
