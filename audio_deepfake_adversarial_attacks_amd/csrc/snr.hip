// snr.hip — gfx950 (MI355X / CDNA4) kernels of the SNR-budget PGD (torchattacks.PGDSNR) + the C ABI declared in
// include/advstep_snr.h: the segmental step (a product of L2 balls, one per 256-sample segment) and the per-row radii of the
// global budget, which then runs through radius.hip's advstep_row_pgd_l2_step_f32.
//
// The segmental step is ONE launch on the (tile, row) grid of row_tiles.h at 16 B per sample.  A segment is what one wavefront
// loads for one j of a tile (perturb.hip's header: quad_of(tile, j) gives the 64 lanes of wave w the samples [256 s, 256 s + 256),
// s = tile * 16 + j * 4 + w, in the float4 path and sample by sample alike), so the segment's three sums — the signal energy, the
// gradient's and the step's squared norms — are a thread's sumsq4 plus one wave_reduce each: no LDS, no workspace, no barrier,
// no second pass, and nothing a workgroup needs from another.  Every wave_reduce is reached by all 64 lanes (no lane leaves the
// kernel early; out-of-row samples are masked, not skipped).
//
// The arithmetic is row_tiles.h's L2 step (l2_move4, l2_scale_factor<true>, l2_project4, sumsq4) with the segment's radius
// r = rho * sqrtf(sum (x + c)^2) in the place of the row's.  Built with -ffp-contract=off; division and sqrt are IEEE; clamps
// propagate NaN (include/advstep.h).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_snr.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

constexpr int kSegment = 256;  // samples per segment: perturb.hip's, the segment of the report's segmental SNR

static_assert(64 * 4 == kSegment, "a segment is one wavefront's float4 load: 64 lanes of 4 samples");
static_assert(kWgThreads % 64 == 0 && (kWgThreads * 4) % kSegment == 0, "one j of a tile is a whole number of segments");
static_assert(kWsRowTile % kSegment == 0, "no segment straddles a tile");

// (x + c) of quad q, each sum rounded once; samples outside the row give 0 (the fill 0 would give c).
__device__ __forceinline__ float4 signal4(float4 x, float c, int64_t T, int64_t q) {
    return zero_outside_row(make_float4(x.x + c, x.y + c, x.z + c, x.w + c), T, q);
}

// ---- a. the segmental step -----------------------------------------------------------------------------------------------------

// out may be adv: a thread reads its own samples before it writes them.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void seg_pgd_step_kernel(const float *adv, const float *__restrict__ grad,
                                                                  const float *__restrict__ orig,
                                                                  const float *__restrict__ offset_rows, float *out, int64_t T,
                                                                  float rho, float alpha_rel, float eps_div, float lo, float hi) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y, o = b * T;
    float4 a[kVecs], g[kVecs], x[kVecs];
    load_tile<VEC>(adv + o, T, tile, 0.0f, a);
    load_tile<VEC>(grad + o, T, tile, 0.0f, g);
    load_tile<VEC>(orig + o, T, tile, 0.0f, x);
    const float c = offset_rows ? offset_rows[b] : 0.0f;  // uniform over the workgroup
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const int64_t q = quad_of(tile, j);
        const float r = rho * sqrtf(wave_reduce(sumsq4(signal4(x[j], c, T, q)), SumOp()));
        const float gn = sqrtf(wave_reduce(sumsq4(g[j]), SumOp())) + eps_div;  // out-of-row g = 0: neutral
        // out-of-row lanes: a = g = x = 0 -> d = 0 when gn != 0; masked explicitly so gn == 0 / NaN cannot leak
        const float4 d = zero_outside_row(l2_move4(a[j], g[j], x[j], alpha_rel * r, gn), T, q);
        const float dn = sqrtf(wave_reduce(sumsq4(d), SumOp()));
        a[j] = l2_project4(x[j], d, l2_scale_factor<true>(dn, r), lo, hi);
    }
    store_tile<VEC>(out + o, T, tile, a);
}

// ---- b. the global budget's radii ------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void snr_energy_partial_kernel(const float *__restrict__ x,
                                                                        const float *__restrict__ offset_rows, int64_t T,
                                                                        float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 r[kVecs];
    load_tile<VEC>(x + b * T, T, tile, 0.0f, r);
    const float c = offset_rows ? offset_rows[b] : 0.0f;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) s += sumsq4(signal4(r[j], c, T, quad_of(tile, j)));
    s = wg_sum(s, lds);
    if (threadIdx.x == 0) part[b * C + tile] = s;
}

// One workgroup per row: the fixed-order re-reduction of the row's C partials.
__global__ __launch_bounds__(kWgThreads) void snr_row_radius_kernel(const float *__restrict__ part, int C, float rho,
                                                                    float *__restrict__ eps_rows) {
    __shared__ float lds[4];
    const int64_t b = blockIdx.x;
    const float s = row_sum(part + b * C, C, lds);
    if (threadIdx.x == 0) eps_rows[b] = rho * sqrtf(s);
}

}  // namespace

extern "C" {

int advstep_seg_pgd_step_f32(const float *adv, const float *grad, const float *orig, const float *offset_rows, float rho,
                             float alpha_rel, float eps_div, float lo, float hi, float *out, int64_t B, int64_t T,
                             advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY && rho >= 0.0f);  // (a NaN rho fails the comparison)
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && grad && orig && out);
    const size_t bytes = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(out == adv || !overlaps(out, adv, bytes));
    ADVSTEP_REQUIRE(!overlaps(out, grad, bytes) && !overlaps(out, orig, bytes));
    ADVSTEP_REQUIRE(!offset_rows || !overlap2(out, bytes, offset_rows, (size_t)B * sizeof(float)));
    const bool vec = rows_vec(T, {adv, grad, orig, out});
    launch_tiles(ROW_KERNEL_PAIR(seg_pgd_step_kernel), vec, B, T, as_stream(stream), adv, grad, orig, offset_rows, out, T, rho,
                 alpha_rel, eps_div, lo, hi);
    return status_after_launch();
}

int advstep_snr_row_radius_f32(const float *x, const float *offset_rows, float rho, float *eps_rows, int64_t B, int64_t T,
                               void *ws, size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY && rho >= 0.0f);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && eps_rows);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(eps_rows, per_row, x, rows));
    ADVSTEP_REQUIRE(!offset_rows || !overlaps(eps_rows, offset_rows, per_row));
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    launch_tiles(ROW_KERNEL_PAIR(snr_energy_partial_kernel), rows_vec(T, {x}), B, T, st, x, offset_rows, T, w.p0);
    hipLaunchKernelGGL(snr_row_radius_kernel, dim3((unsigned)B), dim3(kWgThreads), 0, st, (const float *)w.p0,
                       ws_tiles_per_row(T), rho, eps_rows);
    return status_after_launch();
}

}  // extern "C"
