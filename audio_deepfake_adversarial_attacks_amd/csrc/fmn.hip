// fmn.hip — gfx950 (MI355X / CDNA4) kernels of the minimal-norm attack (torchattacks.FMN) + the C ABI declared in
// include/advstep_fmn.h: the per-(row, tile) partials of an iterate's four norms, and the step that re-reduces them, takes the
// row's decision (radius, best norm, found flag), keeps the row's best adversarial iterate and moves and projects.
//
// Every kernel but `begin` runs on grid = (C tiles of 4096 samples, B rows), 256 threads, 4 float4 per thread and stream
// (row_tiles.h).  All are HBM-bound row passes: 12 B per sample for the norms, 16 (+ 4 per copied sample) for the L-inf step,
// 12 (+ 8 per copied sample) + 16 for the two launches of the L2 step, 8 per copied sample for the last (move == 0) call.  No
// atomics, no workgroup waits on another: a row's norms go through launch boundaries (per-(row, tile) partials in the caller's
// workspace, re-reduced in a fixed order by every workgroup of the row), and the step reads one state buffer and writes another.
// Reruns are bit-identical.  Built with -ffp-contract=off; divisions are IEEE; clamps and minima propagate NaN.
//
// The L2 move is the PGD-L2 step's: row_tiles.h's l2_delta_pass / l2_project_pass (radius.hip's bodies) with the launch scalar
// alpha and the row's new radius; the summation order of every sum is radius.hip's (its header derives the tests' bounds).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_fmn.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

enum { kNormLinf = 0, kNormL2 = 1 };
enum { kFormLast = 0, kFormLinf = 1, kFormL2 = 2 };   // what the step launch does after the decision

// ---- workspace: five float planes of one partial per (row, tile) ---------------------------------------------------------------

struct FmnWs {
    float *dsq, *dmax, *gsq, *gabs, *msq;   // sum d^2, max |d|, sum g^2, sum |g|; the L2 move's sum d'^2
};
constexpr int kFmnPlanes = 5;
inline size_t fmn_ws_bytes(int64_t B, int64_t T) { return (B <= 0 || T <= 0) ? 0 : kFmnPlanes * row_ws_plane(B, T); }
inline bool carve_fmn_ws(void *ws, size_t ws_bytes, int64_t B, int64_t T, FmnWs *out) {
    if (!ws || !aligned16(ws) || ws_bytes < fmn_ws_bytes(B, T)) return false;
    const size_t plane = row_ws_plane(B, T);
    char *p = static_cast<char *>(ws);
    out->dsq = reinterpret_cast<float *>(p);
    out->dmax = reinterpret_cast<float *>(p + plane);
    out->gsq = reinterpret_cast<float *>(p + 2 * plane);
    out->gabs = reinterpret_cast<float *>(p + 3 * plane);
    out->msq = reinterpret_cast<float *>(p + 4 * plane);
    return true;
}

// ---- a. begin ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kWgThreads) void fmn_begin_kernel(float *__restrict__ state, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (b >= B) return;
    state[0 * B + b] = INFINITY;
    state[1 * B + b] = INFINITY;
    state[2 * B + b] = 0.0f;
    state[3 * B + b] = 0.0f;
}

// ---- b. norms ---------------------------------------------------------------------------------------------------------------

// A thread's sum of magnitudes, in tile_sumsq's order: a quad as (|x| + |y|) + (|z| + |w|), the quads one after the other.
__device__ __forceinline__ float sumabs4(float4 v) { return (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w)); }

// out-of-row lanes load 0 from every stream: d = 0 and g = 0 there, neutral in all four reductions.  grad may be null (uniform).
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void fmn_norms_kernel(const float *__restrict__ adv, const float *__restrict__ grad,
                                                               const float *__restrict__ orig, int64_t T, FmnWs w) {
    __shared__ float lds[16];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y, o = b * T;
    float4 a[kVecs], x[kVecs];
    load_tile<VEC>(adv + o, T, tile, 0.0f, a);
    load_tile<VEC>(orig + o, T, tile, 0.0f, x);
    float dm = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = lane(a[j], k) - lane(x[j], k);
            lane(a[j], k) = d;
            dm = max_nan(dm, fabsf(d));
        }
    }
    const float ds = tile_sumsq(a);
    float gs = 0.0f, ga = 0.0f;
    if (grad) {
        float4 g[kVecs];
        load_tile<VEC>(grad + o, T, tile, 0.0f, g);
        gs = tile_sumsq(g);
#pragma unroll
        for (int j = 0; j < kVecs; ++j) ga += sumabs4(g[j]);
    }
    const float r0 = wg_sum(ds, lds), r1 = wg_max_nan(dm, lds + 4), r2 = wg_sum(gs, lds + 8), r3 = wg_sum(ga, lds + 12);
    if (threadIdx.x == 0) {
        const int64_t i = b * C + tile;
        w.dsq[i] = r0;
        w.dmax[i] = r1;
        w.gsq[i] = r2;
        w.gabs[i] = r3;
    }
}

// ---- c. step ----------------------------------------------------------------------------------------------------------------

struct RowDecision {
    float eps, gsq;   // the row's new radius; sum g^2 (the move's gn)
    bool copy;        // the row improved: its tiles go to best_adv
};

// The row's decision from its partials, its logit and the planes of `state` (only read); the first thread of tile 0 writes the
// new planes into `state_out` (and the re-reduced norms into `row_norms`).  Every workgroup of the row derives the same values
// whenever it runs.  `lds` holds >= 16 floats.
__device__ __forceinline__ RowDecision fmn_decide(const FmnWs &w, const float *__restrict__ z, const int64_t *__restrict__ labels,
                                                  const float *__restrict__ state, float *__restrict__ state_out,
                                                  float *__restrict__ row_norms, int64_t B, float gamma, int norm, float *lds) {
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    const float dsq = row_sum(w.dsq + b * C, C, lds);
    const float dmx = row_max(w.dmax + b * C, C, lds + 4);
    const float gsq = row_sum(w.gsq + b * C, C, lds + 8);
    const float gab = row_sum(w.gabs + b * C, C, lds + 12);
    const float dn = norm == kNormL2 ? sqrtf(dsq) : dmx;
    const float gq = norm == kNormL2 ? sqrtf(gsq) : gab;
    const float e = state[0 * B + b], best = state[1 * B + b];
    const bool found = state[2 * B + b] != 0.0f;
    const float zb = z[b];
    const bool is_adv = judged_wrong(zb, labels[b]);
    const bool better = is_adv && dn < best;
    const float best1 = better ? dn : best;
    float eps1;
    if (is_adv) {
        eps1 = min_nan(e, best1) * (1.0f - gamma);
    } else if (found) {
        eps1 = e * (1.0f + gamma);
    } else {
        eps1 = (dn + (gq > 0.0f ? fabsf(zb) / gq : INFINITY)) * (1.0f + gamma);
    }
    if (tile == 0 && threadIdx.x == 0) {
        state_out[0 * B + b] = eps1;
        state_out[1 * B + b] = best1;
        state_out[2 * B + b] = (found || is_adv) ? 1.0f : 0.0f;
        state_out[3 * B + b] = dn;
        if (row_norms) {
            row_norms[0 * B + b] = dsq;
            row_norms[1 * B + b] = dmx;
            row_norms[2 * B + b] = gsq;
            row_norms[3 * B + b] = gab;
        }
    }
    return RowDecision{eps1, gsq, better};
}

// FORM = kFormLast: the decision and the copy.  kFormLinf: ... and the L-inf move and projection (out may be adv: a thread reads
// its own samples before it writes them).  kFormL2: ... and the PGD-L2 delta pass (partials of sum d'^2 into w.msq).
template <bool VEC, int FORM>
__global__ __launch_bounds__(kWgThreads) void fmn_step_kernel(const float *adv, const float *__restrict__ grad,
                                                              const float *__restrict__ orig, const float *__restrict__ z,
                                                              const int64_t *__restrict__ labels, const float *__restrict__ state,
                                                              float *__restrict__ state_out, float *__restrict__ best_adv,
                                                              float *out, float *__restrict__ row_norms, float alpha, float gamma,
                                                              int norm, float eps_div, float lo, float hi, int64_t B, int64_t T,
                                                              FmnWs w) {
    __shared__ float lds[24];
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y, o = b * T;
    const RowDecision r = fmn_decide(w, z, labels, state, state_out, row_norms, B, gamma, norm, lds);
    if (FORM == kFormLinf) {
        float4 a[kVecs], g[kVecs], x[kVecs];
        load_tile<VEC>(adv + o, T, tile, 0.0f, a);
        load_tile<VEC>(grad + o, T, tile, 0.0f, g);
        load_tile<VEC>(orig + o, T, tile, 0.0f, x);
        if (r.copy) store_tile<VEC>(best_adv + o, T, tile, a);   // uniform over the workgroup
        const float gn = sqrtf(r.gsq) + eps_div, e = r.eps;
#pragma unroll
        for (int j = 0; j < kVecs; ++j) {
            const float4 d = l2_move4(a[j], g[j], x[j], alpha, gn);
            a[j] = make_float4(clampf(x[j].x + clampf(d.x, -e, e), lo, hi), clampf(x[j].y + clampf(d.y, -e, e), lo, hi),
                               clampf(x[j].z + clampf(d.z, -e, e), lo, hi), clampf(x[j].w + clampf(d.w, -e, e), lo, hi));
        }
        store_tile<VEC>(out + o, T, tile, a);
        return;
    }
    if (r.copy) {   // uniform over the workgroup
        float4 a[kVecs];
        load_tile<VEC>(adv + o, T, tile, 0.0f, a);
        store_tile<VEC>(best_adv + o, T, tile, a);
    }
    if (FORM == kFormL2) l2_delta_pass<VEC>(adv, grad, orig, T, alpha, eps_div, w.gsq, w.msq, nullptr, lds + 16);
}

// The L2 projection into the row's NEW radius (state_out's first plane): l2_project_pass, out may be adv.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void fmn_l2_project_kernel(const float *adv, const float *__restrict__ grad,
                                                                    const float *__restrict__ orig,
                                                                    const float *__restrict__ eps_rows, float *out, int64_t T,
                                                                    float alpha, float eps_div, float lo, float hi,
                                                                    const float *__restrict__ gpart,
                                                                    const float *__restrict__ dpart, float *__restrict__ dnorm) {
    __shared__ float lds[8];
    l2_project_pass<VEC, true>(adv, grad, orig, out, T, alpha, eps_rows[blockIdx.y], eps_div, lo, hi, gpart, dpart, dnorm, lds);
}

}  // namespace

extern "C" {

size_t advstep_fmn_workspace_bytes(int64_t B, int64_t T) { return fmn_ws_bytes(B, T); }

int advstep_fmn_begin_f32(float *state, int64_t B, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && B <= kMaxGridY);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(state);
    hipLaunchKernelGGL(fmn_begin_kernel, dim3((unsigned)ceil_div(B, kWgThreads)), dim3(kWgThreads), 0, as_stream(stream), state, B);
    return status_after_launch();
}

int advstep_fmn_norms_f32(const float *adv, const float *grad, const float *orig, int64_t B, int64_t T, void *ws, size_t ws_bytes,
                          advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && orig);
    FmnWs w;
    if (!carve_fmn_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    const size_t rows = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(ws, fmn_ws_bytes(B, T), adv, rows) && !overlap2(ws, fmn_ws_bytes(B, T), orig, rows) &&
                    !(grad && overlap2(ws, fmn_ws_bytes(B, T), grad, rows)));
    const bool vec = rows_vec(T, {adv, grad, orig});
    launch_tiles(ROW_KERNEL_PAIR(fmn_norms_kernel), vec, B, T, as_stream(stream), adv, grad, orig, T, w);
    return status_after_launch();
}

int advstep_fmn_step_f32(const float *adv, const float *grad, const float *orig, const float *z, const int64_t *labels,
                         const float *state, float *state_out, float *best_adv, float *out, float *row_norms, float alpha,
                         float gamma, int norm, int move, float eps_div, float lo, float hi, int64_t B, int64_t T, void *ws,
                         size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE((norm == kNormLinf || norm == kNormL2) && gamma > 0.0f && gamma < 1.0f);   // (a NaN fails the comparisons)
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && orig && z && labels && state && state_out && best_adv);
    if (move) ADVSTEP_REQUIRE(grad && out && alpha >= 0.0f && eps_div >= 0.0f);
    const size_t rows = (size_t)B * T * sizeof(float), planes = 4 * (size_t)B * sizeof(float);
    const size_t per_f = (size_t)B * sizeof(float), per_y = (size_t)B * sizeof(int64_t), norms5 = 5 * per_f;
    ADVSTEP_REQUIRE(!overlaps(state, state_out, planes));   // ping-pong: the launch never reads what it writes
    ADVSTEP_REQUIRE(!overlaps(best_adv, adv, rows) && !overlaps(best_adv, orig, rows) && !(grad && overlaps(best_adv, grad, rows)));
    ADVSTEP_REQUIRE(!overlap2(best_adv, rows, state, planes) && !overlap2(best_adv, rows, state_out, planes) &&
                    !overlap2(best_adv, rows, z, per_f) && !overlap2(best_adv, rows, labels, per_y));
    ADVSTEP_REQUIRE(!overlap2(state_out, planes, z, per_f) && !overlap2(state_out, planes, labels, per_y) &&
                    !overlap2(state_out, planes, adv, rows) && !overlap2(state_out, planes, orig, rows) &&
                    !(grad && overlap2(state_out, planes, grad, rows)));
    if (row_norms)
        ADVSTEP_REQUIRE(!overlap2(row_norms, norms5, state, planes) && !overlap2(row_norms, norms5, state_out, planes) &&
                        !overlap2(row_norms, norms5, z, per_f) && !overlap2(row_norms, norms5, labels, per_y) &&
                        !overlap2(row_norms, norms5, best_adv, rows) && !overlap2(row_norms, norms5, adv, rows) &&
                        !overlap2(row_norms, norms5, orig, rows) && !(grad && overlap2(row_norms, norms5, grad, rows)));
    if (move) {
        ADVSTEP_REQUIRE(out == adv || !overlaps(out, adv, rows));
        ADVSTEP_REQUIRE(!overlaps(out, grad, rows) && !overlaps(out, orig, rows) && !overlaps(out, best_adv, rows));
        ADVSTEP_REQUIRE(!overlap2(out, rows, state, planes) && !overlap2(out, rows, state_out, planes) &&
                        !overlap2(out, rows, z, per_f) && !overlap2(out, rows, labels, per_y) &&
                        !(row_norms && overlap2(out, rows, row_norms, norms5)));
    }
    FmnWs w;
    if (!carve_fmn_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    const size_t wsb = fmn_ws_bytes(B, T);
    ADVSTEP_REQUIRE(!overlap2(ws, wsb, best_adv, rows) && !overlap2(ws, wsb, state_out, planes) &&
                    !(move && overlap2(ws, wsb, out, rows)) && !(row_norms && overlap2(ws, wsb, row_norms, norms5)));
    hipStream_t st = as_stream(stream);
    if (!move) {
        const bool vec = rows_vec(T, {adv, best_adv});
        launch_tiles(ROW_KERNEL_PAIR(fmn_step_kernel, kFormLast), vec, B, T, st, adv, grad, orig, z, labels, state, state_out,
                     best_adv, out, row_norms, alpha, gamma, norm, eps_div, lo, hi, B, T, w);
        return status_after_launch();
    }
    const bool vec = rows_vec(T, {adv, grad, orig, best_adv, out});
    if (norm == kNormLinf) {
        launch_tiles(ROW_KERNEL_PAIR(fmn_step_kernel, kFormLinf), vec, B, T, st, adv, grad, orig, z, labels, state, state_out,
                     best_adv, out, row_norms, alpha, gamma, norm, eps_div, lo, hi, B, T, w);
    } else {
        launch_tiles(ROW_KERNEL_PAIR(fmn_step_kernel, kFormL2), vec, B, T, st, adv, grad, orig, z, labels, state, state_out,
                     best_adv, out, row_norms, alpha, gamma, norm, eps_div, lo, hi, B, T, w);
        launch_tiles(ROW_KERNEL_PAIR(fmn_l2_project_kernel), vec, B, T, st, adv, grad, orig, state_out, out, T, alpha, eps_div, lo,
                     hi, w.gsq, w.msq, row_norms ? row_norms + 4 * B : nullptr);
    }
    return status_after_launch();
}

}  // extern "C"
