// smoothadv.hip — gfx950 (MI355X / CDNA4) kernels of the attack on the smoothed detector (torchattacks.SmoothAdvPGD; Salman et
// al., NeurIPS 2019) + the C ABI declared in include/advstep_smoothadv.h: the noised copies of the current iterate in the
// detector's input domain, the soft-vote loss across the slots, and the sum over the slot gradients fused with PGD's step.
//
// The fill is smooth.hip's kernel body (smooth_fill.h) behind one multiply and one add per sample.  The loss gives a row to one
// thread, like smooth_tally_kernel: m * B logits is a few kilobytes.  The step streams on the (4096-sample tile, row) grid of
// row_tiles.h: a thread adds its 16 samples of every slot in slot order in registers; for L-inf it applies pgd_linf_elem there
// and then, for L2 it also leaves the tile's sum of squares in the row workspace, where row_tiles.h's l2_delta_pass and
// l2_project_pass — the bodies of advstep.hip's three-launch PGD-L2 step — pick it up.  That is what makes `out` the bits of
// pgd_linf_step / pgd_l2_step on the summed gradient.
//
// Built with -ffp-contract=off: every expression rounds as the header writes it.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_smoothadv.h"
#include "advstep_common.h"
#include "row_tiles.h"
#include "smooth_fill.h"

namespace {

// ---- a. the noised copies of the iterate ------------------------------------------------------------------------------------------

template <bool VEC, bool AFFINE>
__global__ __launch_bounds__(kWgThreads) void smoothadv_fill_kernel(const float *__restrict__ adv, const float *__restrict__ scale,
                                                                    const float *__restrict__ shift, float *__restrict__ out,
                                                                    int64_t B, int64_t T, int64_t ns, float sigma, uint64_t seed,
                                                                    uint64_t offset0) {
    noised_slots<VEC, AFFINE>(adv, scale, shift, out, B, T, ns, sigma, seed, offset0);
}

// ---- b. the soft vote and its gradient --------------------------------------------------------------------------------------------

constexpr int kLossThreads = 64;

__global__ __launch_bounds__(kLossThreads) void smoothadv_loss_grad_kernel(const float *__restrict__ z,
                                                                           const int64_t *__restrict__ labels, float *__restrict__ dz,
                                                                           float *__restrict__ cost, int64_t B, int64_t m, float scale) {
    const int64_t b = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    if (b >= B) return;
    const float s = 2.0f * (float)labels[b] - 1.0f;
    float M = -softplusf(-(s * z[b]));  // log p_0
    for (int64_t i = 1; i < m; ++i) M = max_nan(M, -softplusf(-(s * z[i * B + b])));
    float S = 0.0f;
    for (int64_t i = 0; i < m; ++i) {
        const float e = expf(-softplusf(-(s * z[i * B + b])) - M);
        S = i == 0 ? e : S + e;
    }
    cost[b] = (logf((float)m) - M) - logf(S);
    const float k = scale * (-s);
    for (int64_t i = 0; i < m; ++i) {
        const float t = s * z[i * B + b];
        const float e = expf(-softplusf(-t) - M);
        dz[i * B + b] = (k * (e / S)) * expf(-softplusf(t));
    }
}

// ---- c. the sum over the slots, and the step --------------------------------------------------------------------------------------

// g = ((g_0 + g_1) + g_2) + ... for the thread's 16 samples of (tile, row b); out-of-row lanes are 0.
template <bool VEC>
__device__ __forceinline__ void slot_sum_tile(const float *__restrict__ grads, int64_t B, int64_t T, int64_t m, int tile, int64_t b,
                                              float4 (&g)[kVecs]) {
    load_tile<VEC>(grads + b * T, T, tile, 0.0f, g);
#pragma unroll 2
    for (int64_t i = 1; i < m; ++i) {
        float4 t[kVecs];
        load_tile<VEC>(grads + (i * B + b) * T, T, tile, 0.0f, t);
#pragma unroll
        for (int j = 0; j < kVecs; ++j) {
            g[j].x += t[j].x;
            g[j].y += t[j].y;
            g[j].z += t[j].z;
            g[j].w += t[j].w;
        }
    }
}

// L-inf: the whole step.  out may be adv: a thread reads its samples of adv before it writes them.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void smoothadv_linf_step_kernel(const float *adv, const float *__restrict__ orig,
                                                                         const float *__restrict__ grads, float *__restrict__ gsum,
                                                                         float *out, int64_t B, int64_t T, int64_t m, float alpha,
                                                                         float eps, float lo, float hi) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    float4 g[kVecs], a[kVecs], x[kVecs];
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
    load_tile<VEC>(orig + b * T, T, tile, 0.0f, x);
    slot_sum_tile<VEC>(grads, B, T, m, tile, b, g);
    store_tile<VEC>(gsum + b * T, T, tile, g);
#pragma unroll
    for (int j = 0; j < kVecs; ++j)
        a[j] = make_float4(pgd_linf_elem(a[j].x, g[j].x, x[j].x, alpha, eps, lo, hi), pgd_linf_elem(a[j].y, g[j].y, x[j].y, alpha, eps, lo, hi),
                           pgd_linf_elem(a[j].z, g[j].z, x[j].z, alpha, eps, lo, hi), pgd_linf_elem(a[j].w, g[j].w, x[j].w, alpha, eps, lo, hi));
    store_tile<VEC>(out + b * T, T, tile, a);
}

// L2, launch 1: the sum, and the partial of ||gsum||^2 that sumsq_partial_kernel would write for this (row, tile).
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void smoothadv_sum_sumsq_kernel(const float *__restrict__ grads, float *__restrict__ gsum,
                                                                         int64_t B, int64_t T, int64_t m, float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float4 g[kVecs];
    slot_sum_tile<VEC>(grads, B, T, m, tile, b, g);
    store_tile<VEC>(gsum + b * T, T, tile, g);
    const float s = wg_sum(tile_sumsq(g), lds);
    if (threadIdx.x == 0) part[b * C + tile] = s;
}

// L2, launches 2 and 3: row_tiles.h's bodies, as advstep.hip's pgd_l2_delta_kernel / pgd_l2_project_kernel run them
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void smoothadv_l2_delta_kernel(const float *__restrict__ adv, const float *__restrict__ grad,
                                                                        const float *__restrict__ orig, int64_t T, float alpha,
                                                                        float eps_div, const float *__restrict__ gpart,
                                                                        float *__restrict__ dpart) {
    __shared__ float lds[8];
    l2_delta_pass<VEC>(adv, grad, orig, T, alpha, eps_div, gpart, dpart, nullptr, lds);
}

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void smoothadv_l2_project_kernel(const float *adv, const float *__restrict__ grad,
                                                                          const float *__restrict__ orig, float *out, int64_t T,
                                                                          float alpha, float eps, float eps_div, float lo, float hi,
                                                                          const float *__restrict__ gpart,
                                                                          const float *__restrict__ dpart) {
    __shared__ float lds[8];
    l2_project_pass<VEC, false>(adv, grad, orig, out, T, alpha, eps, eps_div, lo, hi, gpart, dpart, nullptr, lds);
}

}  // namespace

extern "C" {

int advstep_smoothadv_fill_f32(const float *adv, const float *scale, const float *shift, float *out, int64_t B, int64_t T, int64_t s0,
                               int64_t ns, float sigma, uint64_t seed, uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && s0 >= 0 && ns >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(sigma >= 0.0f && sigma <= 3.402823466e+38f);  // finite and not negative: false for NaN
    ADVSTEP_REQUIRE((scale == nullptr) == (shift == nullptr));
    if (B == 0 || T == 0 || ns == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && out);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(out, (size_t)ns * rows, adv, rows));
    const bool vec = rows_vec(T, {adv, out});
    hipStream_t st = as_stream(stream);
    const uint64_t offset0 = offset + (uint64_t)s0;
    if (scale) {
        ADVSTEP_REQUIRE(!overlap2(out, (size_t)ns * rows, scale, per_row) && !overlap2(out, (size_t)ns * rows, shift, per_row));
        launch_tiles(ROW_KERNEL_PAIR(smoothadv_fill_kernel, true), vec, B, T, st, adv, scale, shift, out, B, T, ns, sigma, seed, offset0);
    } else {
        launch_tiles(ROW_KERNEL_PAIR(smoothadv_fill_kernel, false), vec, B, T, st, adv, scale, shift, out, B, T, ns, sigma, seed, offset0);
    }
    return status_after_launch();
}

int advstep_smoothadv_loss_grad_f32(const float *z, const int64_t *labels, float *dz, float *cost, int64_t B, int64_t m, float scale,
                                    advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && m >= 0);
    if (B == 0 || m == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(z && labels && dz && cost);
    const size_t zb = (size_t)m * B * sizeof(float), cb = (size_t)B * sizeof(float), lb = (size_t)B * sizeof(int64_t);
    ADVSTEP_REQUIRE(!overlap2(dz, zb, z, zb) && !overlap2(dz, zb, labels, lb) && !overlap2(cost, cb, z, zb) &&
                    !overlap2(cost, cb, labels, lb) && !overlap2(dz, zb, cost, cb));
    hipLaunchKernelGGL(smoothadv_loss_grad_kernel, dim3((unsigned)ceil_div(B, kLossThreads)), dim3(kLossThreads), 0, as_stream(stream),
                       z, labels, dz, cost, B, m, scale);
    return status_after_launch();
}

int advstep_smoothadv_step_f32(const float *adv, const float *orig, const float *grads, float *gsum, float *out, int64_t B, int64_t T,
                               int64_t m, int norm, float alpha, float eps, float eps_div, float lo, float hi, void *ws, size_t ws_bytes,
                               advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && m >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(norm == ADVSTEP_SMOOTHADV_LINF || norm == ADVSTEP_SMOOTHADV_L2);
    if (B == 0 || T == 0 || m == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && orig && grads && gsum && out);
    const size_t rows = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(grads, (size_t)m * rows, gsum, rows) && !overlap2(grads, (size_t)m * rows, out, rows));
    ADVSTEP_REQUIRE(!overlaps(gsum, orig, rows) && !overlaps(out, orig, rows) && !overlaps(gsum, adv, rows) && !overlaps(gsum, out, rows));
    ADVSTEP_REQUIRE(out == adv || !overlaps(out, adv, rows));
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {adv, orig, grads, gsum, out});
    if (norm == ADVSTEP_SMOOTHADV_LINF) {
        launch_tiles(ROW_KERNEL_PAIR(smoothadv_linf_step_kernel), vec, B, T, st, adv, orig, grads, gsum, out, B, T, m, alpha, eps, lo, hi);
        return status_after_launch();
    }
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    launch_tiles(ROW_KERNEL_PAIR(smoothadv_sum_sumsq_kernel), vec, B, T, st, grads, gsum, B, T, m, w.p0);
    launch_tiles(ROW_KERNEL_PAIR(smoothadv_l2_delta_kernel), vec, B, T, st, adv, gsum, orig, T, alpha, eps_div, w.p0, w.p1);
    launch_tiles(ROW_KERNEL_PAIR(smoothadv_l2_project_kernel), vec, B, T, st, adv, gsum, orig, out, T, alpha, eps, eps_div, lo, hi, w.p0,
                 w.p1);
    return status_after_launch();
}

}  // extern "C"
