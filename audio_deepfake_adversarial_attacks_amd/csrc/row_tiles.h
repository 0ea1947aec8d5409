// row_tiles.h — the (tile, row) addressing of the row kernels in apgd.hip and momentum.hip (internal, like advstep_common.h).
//
// grid = (C tiles of 4096 samples, B rows), 256 threads, 4 float4 per thread and stream; float4 q of a row is loaded whole when
// the rows are float4-addressable (VEC) and sample by sample otherwise (T % 4 != 0 leaves rows 2 .. B unaligned).

#ifndef ADVSTEP_ROW_TILES_H
#define ADVSTEP_ROW_TILES_H

#include <initializer_list>

#include "advstep_common.h"

namespace {

constexpr int kVecs = 4;                           // float4 per thread per stream
constexpr int kTileVec = kWgThreads * kVecs;       // float4 per workgroup tile
static_assert(kTileVec * 4 == kWsRowTile, "one workspace partial per tile");

// ---- tiles: float4 q of the row; VEC = rows are float4-addressable -----------------------------------------------------

__device__ __forceinline__ int64_t quad_of(int tile, int j) { return (int64_t)tile * kTileVec + j * kWgThreads + threadIdx.x; }

template <bool VEC>
__device__ __forceinline__ float4 load4(const float *row, int64_t T, int64_t q, float fill) {
    const int64_t s = q * 4;
    if (VEC) return (s < T) ? reinterpret_cast<const float4 *>(row)[q] : make_float4(fill, fill, fill, fill);
    return make_float4(s + 0 < T ? row[s + 0] : fill, s + 1 < T ? row[s + 1] : fill, s + 2 < T ? row[s + 2] : fill,
                       s + 3 < T ? row[s + 3] : fill);
}

template <bool VEC>
__device__ __forceinline__ void store4(float *row, int64_t T, int64_t q, float4 v) {
    const int64_t s = q * 4;
    if (VEC) {
        if (s < T) reinterpret_cast<float4 *>(row)[q] = v;
        return;
    }
    if (s + 0 < T) row[s + 0] = v.x;
    if (s + 1 < T) row[s + 1] = v.y;
    if (s + 2 < T) row[s + 2] = v.z;
    if (s + 3 < T) row[s + 3] = v.w;
}

__device__ __forceinline__ float &lane(float4 &v, int k) { return reinterpret_cast<float *>(&v)[k]; }

// Re-reduce the C partials of one row in a fixed order (every workgroup of the row does the same).
__device__ __forceinline__ float row_sum(const float *__restrict__ part, int C, float *lds) {
    float v = 0.0f;
    for (int i = threadIdx.x; i < C; i += kWgThreads) v += part[i];
    return wg_sum(v, lds);
}

// ---- host side ------------------------------------------------------------------------------------------------------------

inline bool rows_vec(int64_t T, std::initializer_list<const void *> ptrs) {
    if (T % 4 != 0) return false;
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return false;
    return true;
}

inline bool overlaps(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

inline dim3 row_grid(int64_t B, int64_t T) { return dim3((unsigned)ws_tiles_per_row(T), (unsigned)B); }

}  // namespace

#endif  // ADVSTEP_ROW_TILES_H
