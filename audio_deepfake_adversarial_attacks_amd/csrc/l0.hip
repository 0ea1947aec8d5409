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
#include "row_project.h"

namespace {

// l0_clip, l0_key and l0_project_row are row_project.h's (fmn_sparse.hip projects with them too)

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
