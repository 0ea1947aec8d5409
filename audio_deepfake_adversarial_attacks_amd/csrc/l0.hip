// l0.hip — gfx950 (MI355X / CDNA4) kernels of the L0 threat model (PGD0 of Croce & Hein, "Sparse and Imperceivable Adversarial
// Attacks", ICCV 2019) + the C ABI declared in include/advstep_l0.h: the exact-k projection onto the L0 ball intersected with
// the box (and an optional per-sample cap), and the L1-normalised gradient step fused with it.
//
// Layout as apgdl1.hip (row_workgroup.h): one workgroup of 1024 threads per row, the row re-read from L2 by every pass, float4
// loads where the rows allow, fixed-order reductions.  No sort and no atomics: the k-th largest score is found by
// row_workgroup.h's digit_search over the 31 bits of a non-negative float's pattern (11 streaming passes that count the scores
// between consecutive candidates); where scores tie at the threshold a second digit_search walks the bits of the sample index
// for the cut that keeps exactly k.  A thread only ever re-reads samples it wrote itself (the traversals give every pass the
// same sample -> thread map), so the passes over the output row need no barrier beyond the reductions'.
//
// Algorithmic bytes per row sample: step 4 (grad) + 12 (cur, grad -> u) + 8 x 11 (x, u) [+ 8 x ceil(bits(T - 1) / 3) for the
// cut] + 12 (x, u -> out), of which 16 B are first touches and the rest L2 / Infinity-Cache re-reads; projection alone
// 8 x 11 [+ cut] + 12.  Built with -ffp-contract=off; divisions are IEEE.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_common.h"
#include "advstep_l0.h"
#include "row_workgroup.h"

namespace {

// c_i of include/advstep_l0.h: d clipped to what the box and the cap leave of it
__device__ __forceinline__ float l0_clip(float d, float xi, float cap) {
    const float lb = -xi > -cap ? -xi : -cap, ub = 1.0f - xi < cap ? 1.0f - xi : cap;
    return clampf(d, lb, ub);
}
// the bit pattern of s_i (>= 0, so patterns order like scores; the mask keeps a NaN's inside the 31 searched bits)
__device__ __forceinline__ uint32_t l0_key(float xi, float ui, float cap) {
    const float d = ui - xi, r = d - l0_clip(d, xi, cap);
    return __float_as_uint(d * d - r * r) & 0x7FFFFFFFu;
}

// out row = P0(u row; x row, kk = min(k, T), cap).  ur may be outr.  stats: the row's four floats or NULL; stats[0] is the caller's.
template <bool VEC>
__device__ __forceinline__ void l0_project_row(const float *xr, const float *ur, float *outr, int64_t T, float kk, float cap,
                                               float *stats, float *lds) {
    // rho = the largest pattern with #{key >= rho} >= kk, which is the kk-th largest key; `above` is that count
    float h[kCand], above = (float)T;
    const uint32_t rho = digit_search(
        31, h, lds,
        [&](uint32_t lo, int shift, float(&hh)[kCand]) {
            visit_rows_ahead<VEC, 2>({xr, ur}, T, [&](const float(&xu)[2]) {
                bucket_add(hh, l0_key(xu[0], xu[1], cap), lo, shift, 1.0f);
            });
        },
        [&](float hj) {                                        // #{key >= candidate j} = above - h[0..j): non-increasing in j
            const float at = above - hj;
            if (!(at >= kk)) return false;
            above = at;
            return true;
        });
    const float eq = (rho & 1u) ? h[1] : h[0];                 // the last pass has one bit: h[pick] = #{key == rho}
    const float gt = above - eq;                               // #{key > rho} < kk <= above
    // the cut: the smallest index with #{i <= cut : key_i == rho} = kk - gt, wanted only where ties exceed what is left of kk.
    // cut = the largest c with #{i < c : key_i == rho} < need, found like rho, over the bits of an index
    int64_t cut = T;
    if (above > kk) {                                          // workgroup-uniform: every thread holds the same counts
        const float need = kk - gt;
        float below = 0.0f;
        cut = (int64_t)digit_search(
            32 - __clz((int)(T - 1)), h, lds,                  // T - 1 >= 1 here (above > kk >= 1)
            [&](uint32_t c, int shift, float(&hh)[kCand]) {
                visit_rows_ahead<VEC, 2>({xr, ur}, T, [&](int64_t i, const float(&xu)[2]) {
                    if (l0_key(xu[0], xu[1], cap) == rho) bucket_add(hh, (uint32_t)i, c, shift, 1.0f);
                });
            },
            [&](float hj) {                                    // #{i < candidate j : tie} = below + h[0..j)
                const float at = below + hj;
                if (!(at < need)) return false;
                below = at;
                return true;
            });
    }
    float last[1] = {-1.0f};                                   // the last kept tie (a thread's indices ascend)
    map_rows<VEC>({xr, ur}, outr, T, [&](int64_t i, float xi, float ui) {
        const float d = ui - xi, ci = l0_clip(d, xi, cap), r = d - ci;
        const uint32_t key = __float_as_uint(d * d - r * r) & 0x7FFFFFFFu;
        const bool tie = key == rho && i <= cut;
        if (tie) last[0] = (float)i;
        return (key > rho || tie) ? clampf(xi + ci, 0.0f, 1.0f) : xi;
    });
    if (stats) {                                               // a kernel argument: uniform
        row_reduce<1>(last, MaxNanOp(), lds);
        if (threadIdx.x == 0) {
            stats[1] = __uint_as_float(rho);
            stats[2] = gt;
            stats[3] = last[0];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kRow) void l0_box_project_kernel(const float *__restrict__ x, const float *u, float *out,
                                                              int64_t B, int64_t T, float kk, float cap) {
    __shared__ float lds[kCand * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x)
        l0_project_row<VEC>(x + row * T, u + row * T, out + row * T, T, kk, cap, nullptr, lds);
}

// ---- the step: the L1-normalised gradient step into the output row, then the projection ----------------------------------

template <bool VEC>
__global__ __launch_bounds__(kRow) void pgdl0_step_kernel(const float *cur, const float *__restrict__ grad,
                                                          const float *__restrict__ x, float *out, float *stats, int64_t B,
                                                          int64_t T, float step, float kk, float cap) {
    __shared__ float lds[kCand * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float *cr = cur + row * T, *gr = grad + row * T;
        float *orow = out + row * T;
        float gn[1] = {0.0f};
        visit_rows<VEC>({gr}, T, [&](float gi) { gn[0] += fabsf(gi); });
        row_reduce<1>(gn, SumOp(), lds);
        if (threadIdx.x == 0 && stats) stats[4 * row] = gn[0];
        const float den = gn[0] + 1e-10f;
        map_rows<VEC>({cr, gr}, orow, T, [&](float ci, float gi) { return ci + (step * gi) / den; });
        l0_project_row<VEC>(x + row * T, orow, orow, T, kk, cap, stats ? stats + 4 * row : nullptr, lds);
    }
}

inline float kept(int64_t k, int64_t T) { return (float)(k < T ? k : T); }

}  // namespace

extern "C" {

int advstep_l0_box_project_f32(const float *x, const float *u, float *out, int64_t k, float eps_inf, int64_t B, int64_t T,
                               advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && k >= 1 && eps_inf > 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && x && u && out && !overlaps(out, x, (size_t)B * T * sizeof(float)));
    return launch_rows(ROW_KERNEL_PAIR(l0_box_project_kernel), rows_vec(T, {x, u, out}), B, stream, x, u, out, B, T,
                       kept(k, T), eps_inf);
}

int advstep_pgdl0_step_f32(const float *cur, const float *grad, const float *x, float *out, float *stats, float step,
                           int64_t k, float eps_inf, int64_t B, int64_t T, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && k >= 1 && eps_inf > 0.0f && step >= 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && cur && grad && x && out);
    const size_t bytes = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(out, grad, bytes) && !overlaps(out, x, bytes));
    ADVSTEP_REQUIRE(!stats || !overlap2(stats, (size_t)B * 4 * sizeof(float), out, bytes));
    return launch_rows(ROW_KERNEL_PAIR(pgdl0_step_kernel), rows_vec(T, {cur, grad, x, out}), B, stream, cur, grad, x, out,
                       stats, B, T, step, kept(k, T), eps_inf);
}

}  // extern "C"
