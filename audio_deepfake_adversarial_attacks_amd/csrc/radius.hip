// radius.hip — gfx950 (MI355X / CDNA4) kernels of the minimal-radius search (torchattacks.MinRadiusPGD) + the C ABI declared in
// include/advstep_radius.h: the PGD L-inf and L2 steps with a radius per row, and the bookkeeping of a per-utterance bisection.
//
// Every kernel but `begin` runs on grid = (C tiles of 4096 samples, B rows), 256 threads, 4 float4 per thread and stream
// (row_tiles.h); a workgroup reads its row's radius once (uniform over the workgroup: scalar loads).  All of them are
// HBM-bound row passes: 16 B per sample for the L-inf step, 4 + 12 + 16 for the three launches of the L2 step, 8 per COPIED
// sample for the search round.  No atomics, no workgroup waits on another: the L2 step's row norms go through launch
// boundaries (per-(row, tile) partials in the caller's workspace, re-reduced in a fixed order by every workgroup of the row),
// and the search round reads one state buffer and writes another.  Reruns are bit-identical.
// Built with -ffp-contract=off; divisions are IEEE; clamps propagate NaN (see include/advstep.h).
//
// Summation order of the L2 norms (tests derive their bound from it; it is advstep.hip's): a thread adds its 4 quads, each as
// (x^2 + y^2) + (z^2 + w^2), one after the other (2 + 4 additions deep); a wave adds in 6 xor-shuffle levels; the 4 waves add
// in 3; the re-reduction adds ceil(C / 256) partials per thread, then 6 + 3 again: 24 + ceil(C / 256) additions on the longest
// chain, over squares that round once each.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_radius.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

// The row's step size: a = alpha_abs + alpha_rel * e (the product rounds, then the sum).
__device__ __forceinline__ float row_alpha(float alpha_abs, float alpha_rel, float e) { return alpha_abs + alpha_rel * e; }

// ---- a. L-inf step ------------------------------------------------------------------------------------------------------------

// out may be adv: a thread reads its own samples before it writes them.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void row_linf_step_kernel(const float *adv, const float *__restrict__ grad,
                                                                   const float *__restrict__ orig,
                                                                   const float *__restrict__ eps_rows, float *out, int64_t T,
                                                                   float alpha_abs, float alpha_rel, float lo, float hi) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y, o = b * T;
    float4 a[kVecs], g[kVecs], x[kVecs];
    load_tile<VEC>(adv + o, T, tile, 0.0f, a);
    load_tile<VEC>(grad + o, T, tile, 0.0f, g);
    load_tile<VEC>(orig + o, T, tile, 0.0f, x);
    const float e = eps_rows[b];
    const float al = row_alpha(alpha_abs, alpha_rel, e);
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float xx = lane(x[j], k);
            const float x1 = lane(a[j], k) + al * sgn(lane(g[j], k));
            lane(a[j], k) = clampf(xx + clampf(x1 - xx, -e, e), lo, hi);
        }
    }
    store_tile<VEC>(out + o, T, tile, a);
}

// ---- b. L2 step ------------------------------------------------------------------------------------------------------------

// pass 1 is row_tiles.h's sumsq_partial_kernel; passes 2 and 3 are its l2_delta_pass / l2_project_pass (built on l2_move4,
// l2_scale_factor and l2_project4, like advstep.hip's step kernels) with the row's a and e
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void row_l2_delta_kernel(const float *__restrict__ adv, const float *__restrict__ grad,
                                                                  const float *__restrict__ orig,
                                                                  const float *__restrict__ eps_rows, int64_t T, float alpha_abs,
                                                                  float alpha_rel, float eps_div,
                                                                  const float *__restrict__ gpart, float *__restrict__ dpart,
                                                                  float *__restrict__ gnorm) {
    __shared__ float lds[8];
    l2_delta_pass<VEC>(adv, grad, orig, T, row_alpha(alpha_abs, alpha_rel, eps_rows[blockIdx.y]), eps_div, gpart, dpart, gnorm, lds);
}

// out may be adv
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void row_l2_project_kernel(const float *adv, const float *__restrict__ grad,
                                                                    const float *__restrict__ orig,
                                                                    const float *__restrict__ eps_rows, float *out, int64_t T,
                                                                    float alpha_abs, float alpha_rel, float eps_div, float lo,
                                                                    float hi, const float *__restrict__ gpart,
                                                                    const float *__restrict__ dpart, float *__restrict__ dnorm) {
    __shared__ float lds[8];
    const float e = eps_rows[blockIdx.y];
    l2_project_pass<VEC, true>(adv, grad, orig, out, T, row_alpha(alpha_abs, alpha_rel, e), e, eps_div, lo, hi, gpart, dpart, dnorm,
                               lds);
}

// ---- c. search bookkeeping ----------------------------------------------------------------------------------------------------

// the row's verdict: advstep_common.h's judged_wrong (fmn.hip takes the same)

__global__ __launch_bounds__(kWgThreads) void radius_begin_kernel(const float *__restrict__ z0, const int64_t *__restrict__ labels,
                                                                  float eps_max, float *__restrict__ state, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (b >= B) return;
    const bool wrong = judged_wrong(z0[b], labels[b]);
    const float hi = wrong ? 0.0f : eps_max;
    state[0 * B + b] = 0.0f;
    state[1 * B + b] = hi;
    state[2 * B + b] = hi;
    state[3 * B + b] = wrong ? 0.0f : INFINITY;
}

// `state` is only read and `state_out` only written (ping-pong, include/advstep_radius.h): every workgroup of a row derives the
// same decision whenever it runs.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void radius_round_kernel(const float *__restrict__ adv, const float *__restrict__ z,
                                                                  const int64_t *__restrict__ labels, int first,
                                                                  const float *__restrict__ state, float *__restrict__ state_out,
                                                                  float *__restrict__ best_adv, int64_t B, int64_t T) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    float lo = state[0 * B + b], hi = state[1 * B + b], best = state[3 * B + b];
    const float eps = state[2 * B + b];
    const bool flipped = judged_wrong(z[b], labels[b]);
    bool copy = false;
    if (flipped && eps < best) {
        best = eps;
        hi = eps;
        copy = true;
    } else if (!flipped) {
        lo = eps;
        copy = first != 0;
    }
    if (tile == 0 && threadIdx.x == 0) {
        state_out[0 * B + b] = lo;
        state_out[1 * B + b] = hi;
        state_out[2 * B + b] = 0.5f * (lo + hi);
        state_out[3 * B + b] = best;
    }
    if (!copy) return;  // uniform over the workgroup
    float4 r[kVecs];
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, r);
    store_tile<VEC>(best_adv + b * T, T, tile, r);
}

// The steps' aliasing rule: out is adv itself or overlaps none of adv, grad, orig; the per-row operands (nullable) lie outside out.
inline bool step_aliasing_ok(const float *adv, const float *grad, const float *orig, const float *out, int64_t B, int64_t T,
                             std::initializer_list<const void *> per_row) {
    const size_t bytes = (size_t)B * T * sizeof(float);
    if (out != adv && overlaps(out, adv, bytes)) return false;
    if (overlaps(out, grad, bytes) || overlaps(out, orig, bytes)) return false;
    for (const void *p : per_row)
        if (p && overlap2(out, bytes, p, (size_t)B * sizeof(float))) return false;
    return true;
}

}  // namespace

extern "C" {

int advstep_row_pgd_linf_step_f32(const float *adv, const float *grad, const float *orig, const float *eps_rows, float alpha_abs,
                                  float alpha_rel, float lo, float hi, float *out, int64_t B, int64_t T,
                                  advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && grad && orig && eps_rows && out);
    ADVSTEP_REQUIRE(step_aliasing_ok(adv, grad, orig, out, B, T, {eps_rows}));
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {adv, grad, orig, out});
    launch_tiles(ROW_KERNEL_PAIR(row_linf_step_kernel), vec, B, T, st, adv, grad, orig, eps_rows, out, T, alpha_abs, alpha_rel, lo, hi);
    return status_after_launch();
}

int advstep_row_pgd_l2_step_f32(const float *adv, const float *grad, const float *orig, const float *eps_rows, float alpha_abs,
                                float alpha_rel, float eps_div, float lo, float hi, float *out, float *gnorm, float *dnorm,
                                int64_t B, int64_t T, void *ws, size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && grad && orig && eps_rows && out);
    ADVSTEP_REQUIRE(step_aliasing_ok(adv, grad, orig, out, B, T, {eps_rows, gnorm, dnorm}));
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {adv, grad, orig, out});
    launch_tiles(ROW_KERNEL_PAIR(sumsq_partial_kernel), vec, B, T, st, grad, T, w.p0);
    launch_tiles(ROW_KERNEL_PAIR(row_l2_delta_kernel), vec, B, T, st, adv, grad, orig, eps_rows, T, alpha_abs, alpha_rel, eps_div,
                 w.p0, w.p1, gnorm);
    launch_tiles(ROW_KERNEL_PAIR(row_l2_project_kernel), vec, B, T, st, adv, grad, orig, eps_rows, out, T, alpha_abs, alpha_rel,
                 eps_div, lo, hi, w.p0, w.p1, dnorm);
    return status_after_launch();
}

int advstep_radius_begin_f32(const float *z0, const int64_t *labels, float eps_max, float *state, int64_t B,
                             advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && B <= kMaxGridY && eps_max >= 0.0f);  // (a NaN eps_max fails the comparison)
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(z0 && labels && state);
    ADVSTEP_REQUIRE(!overlap2(state, 4 * (size_t)B * sizeof(float), z0, (size_t)B * sizeof(float)) &&
                    !overlap2(state, 4 * (size_t)B * sizeof(float), labels, (size_t)B * sizeof(int64_t)));
    hipLaunchKernelGGL(radius_begin_kernel, dim3((unsigned)ceil_div(B, kWgThreads)), dim3(kWgThreads), 0, as_stream(stream), z0,
                       labels, eps_max, state, B);
    return status_after_launch();
}

int advstep_radius_round_f32(const float *adv, const float *z, const int64_t *labels, int first, const float *state,
                             float *state_out, float *best_adv, int64_t B, int64_t T, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && z && labels && state && state_out && best_adv);
    const size_t rows = (size_t)B * T * sizeof(float), planes = 4 * (size_t)B * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(state, state_out, planes));  // ping-pong: the launch never reads what it writes
    ADVSTEP_REQUIRE(!overlaps(best_adv, adv, rows) && !overlap2(best_adv, rows, state, planes) &&
                    !overlap2(best_adv, rows, state_out, planes));
    ADVSTEP_REQUIRE(!overlap2(state_out, planes, z, (size_t)B * sizeof(float)) &&
                    !overlap2(state_out, planes, labels, (size_t)B * sizeof(int64_t)) && !overlap2(state_out, planes, adv, rows));
    ADVSTEP_REQUIRE(!overlap2(best_adv, rows, z, (size_t)B * sizeof(float)) &&
                    !overlap2(best_adv, rows, labels, (size_t)B * sizeof(int64_t)));
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {adv, best_adv});
    launch_tiles(ROW_KERNEL_PAIR(radius_round_kernel), vec, B, T, st, adv, z, labels, first, state, state_out, best_adv, B, T);
    return status_after_launch();
}

}  // extern "C"
