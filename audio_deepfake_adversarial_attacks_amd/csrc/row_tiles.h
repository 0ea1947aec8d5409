// row_tiles.h — the (tile, row) addressing of every row kernel (advstep.hip, apgd.hip, momentum.hip, radius.hip) and the re-reduction of a
// row's per-tile partials (internal, like advstep_common.h, which has the rules that do not depend on this 256-thread tile:
// scalar semantics, reductions, rows_vec, overlaps).
//
// grid = (C tiles of 4096 samples, B rows), 256 threads, 4 float4 per thread and stream; float4 q of a row is loaded whole when
// the rows are float4-addressable (VEC) and sample by sample otherwise (T % 4 != 0 leaves rows 2 .. B unaligned).  Tile c of
// row b owns partial b * C + c of a workspace plane (RowWs in advstep_common.h), whichever file's kernel wrote it.

#ifndef ADVSTEP_ROW_TILES_H
#define ADVSTEP_ROW_TILES_H

#include "advstep_common.h"

namespace {

constexpr int kVecs = 4;                           // float4 per thread per stream
constexpr int kTileVec = kWgThreads * kVecs;       // float4 per workgroup tile
static_assert(kTileVec * 4 == kWsRowTile, "one workspace partial per tile");

// ---- tiles: float4 q of the row; VEC = rows are float4-addressable -----------------------------------------------------

__device__ __forceinline__ int64_t quad_of(int tile, int j) { return (int64_t)tile * kTileVec + j * kWgThreads + threadIdx.x; }

// VEC rows have T % 4 == 0, so a quad is inside the row or outside it as a whole: q < T / 4.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *row, int64_t T, int64_t q, float fill) {
    if (VEC) return (q < (T >> 2)) ? reinterpret_cast<const float4 *>(row)[q] : make_float4(fill, fill, fill, fill);
    const int64_t s = q * 4;
    return make_float4(s + 0 < T ? row[s + 0] : fill, s + 1 < T ? row[s + 1] : fill, s + 2 < T ? row[s + 2] : fill,
                       s + 3 < T ? row[s + 3] : fill);
}

template <bool VEC>
__device__ __forceinline__ void store4(float *row, int64_t T, int64_t q, float4 v) {
    if (VEC) {
        if (q < (T >> 2)) reinterpret_cast<float4 *>(row)[q] = v;
        return;
    }
    const int64_t s = q * 4;
    if (s + 0 < T) row[s + 0] = v.x;
    if (s + 1 < T) row[s + 1] = v.y;
    if (s + 2 < T) row[s + 2] = v.z;
    if (s + 3 < T) row[s + 3] = v.w;
}

// Is sample k (0..3) of quad q inside the row?  (only needed where `fill` cannot be neutral)
__device__ __forceinline__ bool in_row(int64_t T, int64_t q, int k) { return q * 4 + k < T; }

// Sample k of a float4: by reference (k known at compile time, after unrolling), or by value for a k known only at run time.
__device__ __forceinline__ float &lane(float4 &v, int k) { return reinterpret_cast<float *>(&v)[k]; }
__device__ __forceinline__ float lane(const float4 &v, int k) { return f32x4{v.x, v.y, v.z, v.w}[k]; }

// The workgroup's whole tile of one row in registers (out-of-row lanes get `fill`), for kernels that keep it across a reduction.
template <bool VEC>
__device__ __forceinline__ void load_tile(const float *__restrict__ row, int64_t T, int tile, float fill, float4 (&r)[kVecs]) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j) r[j] = load4<VEC>(row, T, quad_of(tile, j), fill);
}

template <bool VEC>
__device__ __forceinline__ void store_tile(float *row, int64_t T, int tile, const float4 (&r)[kVecs]) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j) store4<VEC>(row, T, quad_of(tile, j), r[j]);
}

// f(sample) over the 16 samples a thread holds of a tile.
template <class F>
__device__ __forceinline__ void for_each_lane(float4 (&r)[kVecs], F f) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) f(lane(r[j], k));
    }
}

// Re-reduce the C partials of one row in a fixed order (every workgroup of the row does the same; C is 16 at T = 64 600).
// Min and max start from the row's first partial, not from an infinity: NaN propagates as in the partials themselves.
__device__ __forceinline__ float row_sum(const float *__restrict__ part, int C, float *lds) {
    float v = 0.0f;
    for (int i = threadIdx.x; i < C; i += kWgThreads) v += part[i];
    return wg_sum(v, lds);
}
__device__ __forceinline__ float row_max(const float *__restrict__ part, int C, float *lds) {
    float v = part[0];
    for (int i = threadIdx.x; i < C; i += kWgThreads) v = max_nan(v, part[i]);
    return wg_max_nan(v, lds);
}
__device__ __forceinline__ float row_min(const float *__restrict__ part, int C, float *lds) {
    float v = part[0];
    for (int i = threadIdx.x; i < C; i += kWgThreads) v = min_nan(v, part[i]);
    return wg_min_nan(v, lds);
}

// ---- row sum of squares (||grad||^2, ||normal||^2): one partial per (row, tile); advstep.hip and radius.hip launch it ------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void sumsq_partial_kernel(const float *__restrict__ g, int64_t T,
                                                               float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 r[kVecs];
    load_tile<VEC>(g + b * T, T, tile, 0.0f, r);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) s += (r[j].x * r[j].x + r[j].y * r[j].y) + (r[j].z * r[j].z + r[j].w * r[j].w);
    s = wg_sum(s, lds);
    if (threadIdx.x == 0) part[b * C + tile] = s;
}

// ---- the PGD-L2 step's two row passes (advstep.hip: launch scalars alpha, eps; radius.hip: the row's a, e) ---------------------
// One body each, so the fixed-radius and the per-row kernels agree bit for bit by construction.  `lds` holds >= 8 floats.

// pass 2: gn from the grad partials; a = adv + alpha * (g / gn); d = a - orig; partial sum d^2
template <bool VEC>
__device__ __forceinline__ void l2_delta_pass(const float *__restrict__ adv, const float *__restrict__ grad,
                                              const float *__restrict__ orig, int64_t T, float alpha, float eps_div,
                                              const float *__restrict__ gpart, float *__restrict__ dpart,
                                              float *__restrict__ gnorm, float *lds) {
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 a[kVecs], g[kVecs], x[kVecs];
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
    load_tile<VEC>(grad + b * T, T, tile, 0.0f, g);
    load_tile<VEC>(orig + b * T, T, tile, 0.0f, x);
    const float gsq = row_sum(gpart + b * C, C, lds);
    const float gn_raw = sqrtf(gsq);
    const float gn = gn_raw + eps_div;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        float4 d;
        d.x = (a[j].x + alpha * (g[j].x / gn)) - x[j].x;
        d.y = (a[j].y + alpha * (g[j].y / gn)) - x[j].y;
        d.z = (a[j].z + alpha * (g[j].z / gn)) - x[j].z;
        d.w = (a[j].w + alpha * (g[j].w / gn)) - x[j].w;
        // out-of-row lanes: a = g = x = 0 -> d = 0 when gn != 0; mask explicitly so gn == 0 / NaN cannot leak
        if (!in_row(T, quad_of(tile, j), 0)) d.x = 0.0f;
        if (!in_row(T, quad_of(tile, j), 1)) d.y = 0.0f;
        if (!in_row(T, quad_of(tile, j), 2)) d.z = 0.0f;
        if (!in_row(T, quad_of(tile, j), 3)) d.w = 0.0f;
        s += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
    s = wg_sum(s, lds + 4);
    if (threadIdx.x == 0) {
        dpart[b * C + tile] = s;
        if (tile == 0 && gnorm) gnorm[b] = gn_raw;
    }
}

// pass 3: recompute d, f = min((1/dn) * eps, 1), out = clamp(orig + d * f, lo, hi).  out may be adv (a thread reads its own
// samples before it writes them).  ZERO_NORM_KEEPS: f = 1 when dn == 0 — what min(inf * eps, 1) gives for every eps > 0 — also at
// eps = 0, where inf * 0 would be NaN (radius.hip's radius-0 rows).
template <bool VEC, bool ZERO_NORM_KEEPS>
__device__ __forceinline__ void l2_project_pass(const float *adv, const float *__restrict__ grad,
                                                const float *__restrict__ orig, float *out, int64_t T, float alpha, float eps,
                                                float eps_div, float lo, float hi, const float *__restrict__ gpart,
                                                const float *__restrict__ dpart, float *__restrict__ dnorm, float *lds) {
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 a[kVecs], g[kVecs], x[kVecs];
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
    load_tile<VEC>(grad + b * T, T, tile, 0.0f, g);
    load_tile<VEC>(orig + b * T, T, tile, 0.0f, x);
    const float gn = sqrtf(row_sum(gpart + b * C, C, lds)) + eps_div;
    const float dn = sqrtf(row_sum(dpart + b * C, C, lds + 4));
    const float f = (ZERO_NORM_KEEPS && dn == 0.0f) ? 1.0f : min_nan((1.0f / dn) * eps, 1.0f);
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        float4 d;
        d.x = (a[j].x + alpha * (g[j].x / gn)) - x[j].x;
        d.y = (a[j].y + alpha * (g[j].y / gn)) - x[j].y;
        d.z = (a[j].z + alpha * (g[j].z / gn)) - x[j].z;
        d.w = (a[j].w + alpha * (g[j].w / gn)) - x[j].w;
        a[j].x = clampf(x[j].x + d.x * f, lo, hi);
        a[j].y = clampf(x[j].y + d.y * f, lo, hi);
        a[j].z = clampf(x[j].z + d.z * f, lo, hi);
        a[j].w = clampf(x[j].w + d.w * f, lo, hi);
    }
    store_tile<VEC>(out + b * T, T, tile, a);
    if (tile == 0 && threadIdx.x == 0 && dnorm) dnorm[b] = dn;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

inline dim3 row_grid(int64_t B, int64_t T) { return dim3((unsigned)ws_tiles_per_row(T), (unsigned)B); }

}  // namespace

#endif  // ADVSTEP_ROW_TILES_H
