// row_tiles.h — the (tile, row) addressing of every row kernel (advstep.hip, apgd.hip, momentum.hip) and the re-reduction of a
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

// ---- host side ------------------------------------------------------------------------------------------------------------

inline dim3 row_grid(int64_t B, int64_t T) { return dim3((unsigned)ws_tiles_per_row(T), (unsigned)B); }

}  // namespace

#endif  // ADVSTEP_ROW_TILES_H
