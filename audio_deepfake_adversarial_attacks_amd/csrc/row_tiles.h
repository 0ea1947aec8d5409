// row_tiles.h — the (tile, row) geometry of the 256-thread row kernels (advstep.hip, apgd.hip, momentum.hip, radius.hip, perturb.hip,
// multiattack.hip, snr.hip, universal.hip, spsa.hip, hsj.hip, smooth.hip, smoothadv.hip, fmn.hip): tile addressing, the re-reduction of a row's per-tile partials, the L2
// arithmetic that several kernels must agree on bit for bit, and the launch on the (tile, row) grid (internal, like
// advstep_common.h, which has the rules that do not depend on this tile: scalar semantics, reductions, rows_vec, ROW_KERNEL_PAIR,
// overlaps).
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

// ---- the L2 arithmetic: one body per expression -------------------------------------------------------------------------------
// Several kernels promise the same bits for the same row (the three-launch PGD-L2 step, its single-pass and repair kernels in
// advstep.hip, radius.hip's per-row step, apgd.hip's row norms); what they must agree on is written once, here.  The helpers
// work on one quad: the single-pass kernel reads `orig` back from LDS quad by quad, and the repair kernels loop over tiles.

// A thread's sum of squares: a quad as (x^2 + y^2) + (z^2 + w^2), the tile's kVecs quads one after the other.  The order is part
// of every norm's bits (radius.hip's header derives the tests' bounds from it).
__device__ __forceinline__ float sumsq4(float4 v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
__device__ __forceinline__ float tile_sumsq(const float4 (&r)[kVecs]) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) s += sumsq4(r[j]);
    return s;
}

// Samples of quad q outside the row -> 0, where a neutral `fill` cannot be relied on (a 0 / 0 or a NaN norm must not leak into a sum).
__device__ __forceinline__ float4 zero_outside_row(float4 d, int64_t T, int64_t q) {
    if (!in_row(T, q, 0)) d.x = 0.0f;
    if (!in_row(T, q, 1)) d.y = 0.0f;
    if (!in_row(T, q, 2)) d.z = 0.0f;
    if (!in_row(T, q, 3)) d.w = 0.0f;
    return d;
}

// The PGD-L2 move of one quad: d = (adv + alpha * (g / gn)) - orig.
__device__ __forceinline__ float4 l2_move4(float4 a, float4 g, float4 x, float alpha, float gn) {
    return make_float4((a.x + alpha * (g.x / gn)) - x.x, (a.y + alpha * (g.y / gn)) - x.y, (a.z + alpha * (g.z / gn)) - x.z,
                       (a.w + alpha * (g.w / gn)) - x.w);
}

// f = min((1 / dn) * eps, 1).  ZERO_NORM_KEEPS: f = 1 when dn == 0 — what min(inf * eps, 1) gives for every eps > 0 — also at
// eps = 0, where inf * 0 would be NaN (radius.hip's radius-0 rows).
template <bool ZERO_NORM_KEEPS>
__device__ __forceinline__ float l2_scale_factor(float dn, float eps) {
    return (ZERO_NORM_KEEPS && dn == 0.0f) ? 1.0f : min_nan((1.0f / dn) * eps, 1.0f);
}

// The projection of one quad: clamp(orig + d * f, lo, hi).
__device__ __forceinline__ float4 l2_project4(float4 x, float4 d, float f, float lo, float hi) {
    return make_float4(clampf(x.x + d.x * f, lo, hi), clampf(x.y + d.y * f, lo, hi), clampf(x.z + d.z * f, lo, hi),
                       clampf(x.w + d.w * f, lo, hi));
}

// ---- row sum of squares (||grad||^2, ||normal||^2): one partial per (row, tile); advstep.hip, apgd.hip and radius.hip launch it ---

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void sumsq_partial_kernel(const float *__restrict__ g, int64_t T,
                                                               float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 r[kVecs];
    load_tile<VEC>(g + b * T, T, tile, 0.0f, r);
    const float s = wg_sum(tile_sumsq(r), lds);
    if (threadIdx.x == 0) part[b * C + tile] = s;
}

// ---- the PGD-L2 step's two row passes (advstep.hip and smoothadv.hip: launch scalars alpha, eps; radius.hip: the row's a, e; fmn.hip: alpha, the row's e) ----
// One body each, so the fixed-radius and the per-row kernels agree bit for bit by construction.  `lds` holds >= 8 floats.

// pass 2: gn from the grad partials; d = l2_move4; partial sum d^2
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
    // out-of-row lanes: a = g = x = 0 -> d = 0 when gn != 0; masked explicitly so gn == 0 / NaN cannot leak
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) s += sumsq4(zero_outside_row(l2_move4(a[j], g[j], x[j], alpha, gn), T, quad_of(tile, j)));
    s = wg_sum(s, lds + 4);
    if (threadIdx.x == 0) {
        dpart[b * C + tile] = s;
        if (tile == 0 && gnorm) gnorm[b] = gn_raw;
    }
}

// pass 3: recompute d, f = l2_scale_factor, out = l2_project4.  out may be adv (a thread reads its own samples before it writes
// them).
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
    const float f = l2_scale_factor<ZERO_NORM_KEEPS>(dn, eps);
#pragma unroll
    for (int j = 0; j < kVecs; ++j) a[j] = l2_project4(x[j], l2_move4(a[j], g[j], x[j], alpha, gn), f, lo, hi);
    store_tile<VEC>(out + b * T, T, tile, a);
    if (tile == 0 && threadIdx.x == 0 && dnorm) dnorm[b] = dn;
}

// ---- the PGD-L2 random start from Philox (advstep.hip's two-kernel, single-pass and repair kernels) ---------------------------

// Philox normals for this thread's kVecs quads of (row b, tile); out-of-row samples are zeroed.
__device__ __forceinline__ void philox_normal_tile(int64_t T, int tile, uint32_t b, uint64_t seed, uint64_t offset,
                                                   float4 (&nz)[kVecs]) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const int64_t q = quad_of(tile, j);
        if (in_row(T, q, 0)) {
            nz[j] = philox_normal4((uint32_t)q, b, seed, offset);
            if (!in_row(T, q, 1)) nz[j].y = 0.0f;
            if (!in_row(T, q, 2)) nz[j].z = 0.0f;
            if (!in_row(T, q, 3)) nz[j].w = 0.0f;
        } else {
            nz[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

// The row's scale (r / ||n||) * eps, r = the first uniform of counter (b, offset + 1).
__device__ __forceinline__ float philox_start_scale(int64_t b, uint64_t seed, uint64_t offset, float nrm, float eps) {
    const uint64_t off1 = offset + 1;
    const Quad rq = philox4x32_10((uint32_t)b, (uint32_t)((uint64_t)b >> 32), (uint32_t)off1, (uint32_t)(off1 >> 32),
                                  (uint32_t)seed, (uint32_t)(seed >> 32));
    return (u01(rq.v[0]) / nrm) * eps;
}

// xv = clamp(xv + nz * scale, lo, hi) over a tile (explicit draws and Philox alike).
__device__ __forceinline__ void l2_start_apply(float4 (&xv)[kVecs], const float4 (&nz)[kVecs], float scale, float lo, float hi) {
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        xv[j].x = clampf(xv[j].x + nz[j].x * scale, lo, hi);
        xv[j].y = clampf(xv[j].y + nz[j].y * scale, lo, hi);
        xv[j].z = clampf(xv[j].z + nz[j].z * scale, lo, hi);
        xv[j].w = clampf(xv[j].w + nz[j].w * scale, lo, hi);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------

inline dim3 row_grid(int64_t B, int64_t T) { return dim3((unsigned)ws_tiles_per_row(T), (unsigned)B); }

// One launch of pair[vec] (a ROW_KERNEL_PAIR: [1] where the rows are float4-addressable) on the (tile, row) grid of B rows.  The
// arguments convert to the kernel's own parameter types, as in a direct call; the status is read by the caller after its last launch.
template <class... P, class... A>
void launch_tiles(void (*const (&pair)[2])(P...), bool vec, int64_t B, int64_t T, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(pair[vec], row_grid(B, T), dim3(kWgThreads), 0, stream, args...);
}

// f(b0, nb) for every slab of at most kMaxGridY rows (grid.y is 16 bits): rows b0 .. b0 + nb of B.  Only advstep.hip slabs; the
// other files reject B > kMaxGridY.
template <class F>
void for_row_slabs(int64_t B, F f) {
    for (int64_t b0 = 0; b0 < B; b0 += kMaxGridY) f(b0, B - b0 < kMaxGridY ? B - b0 : kMaxGridY);
}

}  // namespace

#endif  // ADVSTEP_ROW_TILES_H
