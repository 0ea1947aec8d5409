// apgd.hip — gfx950 (MI355X / CDNA4) kernels of APGD + the C ABI declared in include/advstep_apgd.h: the random start,
// the per-row loss / state update after each model evaluation, the step-size checkpoint, best-point tracking and the L-inf /
// L2 momentum steps (reference: adversarial_attacks/torchattacks/attacks/apgd.py).
//
// Row kernels follow advstep.hip: grid = (C tiles of 4096 samples, B rows), 256 threads, 4 float4 per thread and stream.
// A row sum goes through one partial per (row, tile) in a float plane of the caller's workspace and is re-reduced in a fixed
// order by every workgroup of the row (no atomics: reruns are bit-identical).  The (B) state kernels are one workgroup.
// Built with -ffp-contract=off; divisions and sqrt are IEEE; min / max / clamp propagate NaN (see include/advstep.h).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_apgd.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

constexpr int kNormLinf = 0, kNormL2 = 1;
constexpr uint8_t kFooled = 1, kImproved = 2, kReset = 4;

// torch.clamp(torch.min(torch.max(v, x - eps), x + eps), 0, 1)
__device__ __forceinline__ float ball_box(float v, float x, float eps) {
    return clampf(min_nan(max_nan(v, x - eps), x + eps), 0.0f, 1.0f);
}

// ---- random start ------------------------------------------------------------------------------------------------------

// The start's t for the 4 samples of quad q of row b: L-inf t = 2 d - 1, L2 t = d; d from the caller's draw or Philox.
// Out-of-row samples are 0 (neutral for max |t| and for sum t^2).
template <bool VEC, bool PHILOX>
__device__ __forceinline__ float4 start_t(const float *__restrict__ draw, int64_t b, int64_t T, int64_t q, int norm,
                                          uint64_t seed, uint64_t offset) {
    float4 d;
    if (!PHILOX) {
        d = load4<VEC>(draw + b * T, T, q, 0.0f);
    } else if (norm == kNormL2) {
        d = philox_normal4((uint32_t)q, (uint32_t)b, seed, offset);
    } else if (VEC) {  // T % 4 == 0: the quad of the flat stream is this float4
        const uint64_t fq = (uint64_t)(b * T) / 4 + (uint64_t)q;
        const Quad r = philox4x32_10((uint32_t)fq, (uint32_t)(fq >> 32), (uint32_t)offset, (uint32_t)(offset >> 32),
                                     (uint32_t)seed, (uint32_t)(seed >> 32));
        d = make_float4(u01(r.v[0]), u01(r.v[1]), u01(r.v[2]), u01(r.v[3]));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = (uint64_t)(b * T + q * 4 + k);
            const uint64_t fq = i >> 2;
            const Quad r = philox4x32_10((uint32_t)fq, (uint32_t)(fq >> 32), (uint32_t)offset, (uint32_t)(offset >> 32),
                                         (uint32_t)seed, (uint32_t)(seed >> 32));
            lane(d, k) = u01(r.v[i & 3]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float &e = lane(d, k);
        if (norm == kNormLinf) e = 2.0f * e - 1.0f;
        if (!in_row(T, q, k)) e = 0.0f;
    }
    return d;
}

// pass 1: partial max |t| (L-inf) or sum t^2 (L2) of (row, tile)
template <bool VEC, bool PHILOX>
__global__ __launch_bounds__(kWgThreads) void apgd_init_reduce_kernel(const float *__restrict__ draw, int64_t T, int norm,
                                                                      uint64_t seed, uint64_t offset,
                                                                      float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const float4 t = start_t<VEC, PHILOX>(draw, b, T, quad_of(tile, j), norm, seed, offset);
        if (norm == kNormLinf)
            acc = max_nan(acc, max_nan(max_nan(fabsf(t.x), fabsf(t.y)), max_nan(fabsf(t.z), fabsf(t.w))));
        else
            acc += sumsq4(t);
    }
    acc = (norm == kNormLinf) ? wg_max_nan(acc, lds) : wg_sum(acc, lds);
    if (threadIdx.x == 0) part[b * C + tile] = acc;
}

// pass 2: out = clamp(x + ((eps * 1) * t) / m, lo, hi), m = max |t| or sqrt(sum t^2) + 1e-12
template <bool VEC, bool PHILOX>
__global__ __launch_bounds__(kWgThreads) void apgd_init_apply_kernel(const float *__restrict__ x,
                                                                     const float *__restrict__ draw, float *out, int64_t T,
                                                                     int norm, float eps, float lo, float hi, uint64_t seed,
                                                                     uint64_t offset, const float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    const float m = (norm == kNormLinf) ? row_max(part + b * C, C, lds) : sqrtf(row_sum(part + b * C, C, lds)) + 1e-12f;
    const float scale = eps * 1.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const int64_t q = quad_of(tile, j);
        if (!in_row(T, q, 0)) continue;
        const float4 t = start_t<VEC, PHILOX>(draw, b, T, q, norm, seed, offset);
        float4 v = load4<VEC>(x + b * T, T, q, 0.0f);
        v.x = clampf(v.x + (scale * t.x) / m, lo, hi);
        v.y = clampf(v.y + (scale * t.y) / m, lo, hi);
        v.z = clampf(v.z + (scale * t.z) / m, lo, hi);
        v.w = clampf(v.w + (scale * t.w) / m, lo, hi);
        store4<VEC>(out + b * T, T, q, v);
    }
}

// ---- per-row state ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kWgThreads) void apgd_eval_kernel(const float *__restrict__ z, const int64_t *__restrict__ labels,
                                                               float *__restrict__ dz, float *__restrict__ loss, int mode,
                                                               int64_t i, uint8_t *__restrict__ acc, uint8_t *__restrict__ flags,
                                                               float *__restrict__ loss_best,
                                                               float *__restrict__ loss_best_last_check,
                                                               uint8_t *__restrict__ reduced, float *__restrict__ loss_steps,
                                                               int64_t B) {
    for (int64_t b = threadIdx.x; b < B; b += kWgThreads) {
        const int64_t y = labels[b];
        const float zb = z[b];
        // CE([-z, z], y) = softplus(u), u = (1 - 2y) 2z;  d/dz of the SUMMED loss = 2 (1 - 2y) sigmoid(u)
        const float flip = 1.0f - 2.0f * (float)y;
        const float u = flip * (2.0f * zb);
        const float l = softplusf(u);
        const float sig = 1.0f / (1.0f + expf(-u));
        dz[b] = 2.0f * (flip * sig);
        loss[b] = l;
        const bool pred = (zb > 0.0f ? 1 : 0) == y;  // argmax([-z, z]): a tie and NaN give index 0
        if (mode == 1) {
            acc[b] = pred;
            loss_best[b] = l;
            loss_best_last_check[b] = l;
            reduced[b] = 1;
            flags[b] = 0;
        } else if (mode == 2) {
            acc[b] = (uint8_t)(acc[b] && pred);
            const bool improved = l > loss_best[b];
            if (improved) loss_best[b] = l;
            loss_steps[i * B + b] = l;
            flags[b] = (uint8_t)((pred ? 0 : kFooled) | (improved ? kImproved : 0));
        }
    }
}

__global__ __launch_bounds__(kWgThreads) void apgd_checkpoint_kernel(const float *__restrict__ loss_steps, int64_t steps,
                                                                     int64_t i, int64_t k, double rho,
                                                                     const float *__restrict__ loss_best,
                                                                     float *__restrict__ loss_best_last_check,
                                                                     uint8_t *__restrict__ reduced, float *__restrict__ step_size,
                                                                     uint8_t *__restrict__ flags, int64_t B) {
    for (int64_t b = threadIdx.x; b < B; b += kWgThreads) {
        int64_t count = 0;
        for (int64_t c = 0; c < k; ++c) {
            int64_t j = i - c, jm = i - c - 1;  // numpy wraps the one negative index (-1) to the last row
            if (j < 0) j += steps;
            if (jm < 0) jm += steps;
            count += loss_steps[j * B + b] > loss_steps[jm * B + b];
        }
        const bool osc = (double)count <= (double)k * rho;
        const float lb = loss_best[b];
        const bool fl = osc || (!reduced[b] && (loss_best_last_check[b] >= lb));
        reduced[b] = (uint8_t)fl;
        loss_best_last_check[b] = lb;
        if (fl) step_size[b] = step_size[b] / 2.0f;
        flags[b] = (uint8_t)((flags[b] & ~kReset) | (fl ? kReset : 0));
    }
}

// ---- tracking + reset (flagged rows only) ---------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void apgd_track_kernel(float *x_adv, float *grad, float *x_best, float *grad_best,
                                                                float *x_best_adv, const uint8_t *__restrict__ flags,
                                                                int64_t T) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    const uint8_t f = flags[b];
    if (!f) return;
    const int64_t o = b * T;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const int64_t q = quad_of(tile, j);
        if (!in_row(T, q, 0)) continue;
        if (f & (kFooled | kImproved)) {
            const float4 xa = load4<VEC>(x_adv + o, T, q, 0.0f);
            if (f & kFooled) store4<VEC>(x_best_adv + o, T, q, xa);
            if (f & kImproved) {
                store4<VEC>(x_best + o, T, q, xa);
                store4<VEC>(grad_best + o, T, q, load4<VEC>(grad + o, T, q, 0.0f));
            }
        }
        if ((f & kReset) && !(f & kImproved)) {  // an improved row's best point IS x_adv: its reset changes nothing
            store4<VEC>(x_adv + o, T, q, load4<VEC>(x_best + o, T, q, 0.0f));
            store4<VEC>(grad + o, T, q, load4<VEC>(grad_best + o, T, q, 0.0f));
        }
    }
}

// ---- L-inf step ---------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void apgd_linf_step_kernel(const float *__restrict__ cur, const float *prev,
                                                                    const float *__restrict__ grad,
                                                                    const float *__restrict__ x,
                                                                    const float *__restrict__ step_size, float *out,
                                                                    int64_t T, float eps, float a, float oma) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y, o = b * T;
    const float st = step_size[b];
    float4 c[kVecs], p[kVecs], g[kVecs], xv[kVecs];
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const int64_t q = quad_of(tile, j);
        c[j] = load4<VEC>(cur + o, T, q, 0.0f);
        p[j] = load4<VEC>(prev + o, T, q, 0.0f);
        g[j] = load4<VEC>(grad + o, T, q, 0.0f);
        xv[j] = load4<VEC>(x + o, T, q, 0.0f);
    }
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float cc = lane(c[j], k), xx = lane(xv[j], k);
            const float x1 = ball_box(cc + st * sgn(lane(g[j], k)), xx, eps);
            lane(c[j], k) = ball_box((cc + (x1 - cc) * a) + (cc - lane(p[j], k)) * oma, xx, eps);
        }
        store4<VEC>(out + o, T, quad_of(tile, j), c[j]);
    }
}

// ---- L2 step: four row passes --------------------------------------------------------------------------------------------

// pass 1, the partial sums of g^2, is row_tiles.h's sumsq_partial_kernel

struct L2Row {
    float st, gn, n1, n2, eps, a, oma;
};
// The chain of one sample up to what a pass needs: STAGE 1 = x1 - x, 2 = x2 - x, 3 = out.
template <int STAGE>
__device__ __forceinline__ float l2_chain(float c, float p, float g, float xx, const L2Row &r) {
    const float x1 = c + (r.st * g) / r.gn;
    const float d1 = x1 - xx;
    if (STAGE == 1) return d1;
    const float x1p = clampf(xx + (d1 / (r.n1 + 1e-12f)) * min_nan(r.eps, r.n1), 0.0f, 1.0f);
    const float x2 = (c + (x1p - c) * r.a) + (c - p) * r.oma;
    const float d2 = x2 - xx;
    if (STAGE == 2) return d2;
    return clampf(xx + (d2 / (r.n2 + 1e-12f)) * min_nan(r.eps, r.n2 + 1e-12f), 0.0f, 1.0f);
}

// pass 2 (STAGE 1): partials of sum (x1 - x)^2 -> part_out, norms[b, 0] = ||g||
// pass 3 (STAGE 2): partials of sum (x2 - x)^2 -> part_out, norms[b, 1] = ||x1 - x||
// pass 4 (STAGE 3): out,                                    norms[b, 2] = ||x2 - x||
template <bool VEC, int STAGE>
__global__ __launch_bounds__(kWgThreads) void apgd_l2_pass_kernel(const float *__restrict__ cur, const float *prev,
                                                                  const float *__restrict__ grad,
                                                                  const float *__restrict__ x,
                                                                  const float *__restrict__ step_size, float *out,
                                                                  float *norms, int64_t T, float eps, float a, float oma,
                                                                  const float *__restrict__ part_in,
                                                                  float *__restrict__ part_out) {
    __shared__ float lds[8];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y, o = b * T;
    L2Row r;
    r.st = step_size[b];
    r.eps = eps;
    r.a = a;
    r.oma = oma;
    r.n1 = r.n2 = 0.0f;
    const float reduced = sqrtf(row_sum(part_in + b * C, C, lds));  // ||g||, ||x1 - x||, ||x2 - x|| for STAGE 1, 2, 3
    if (STAGE == 1) {
        r.gn = reduced + 1e-12f;
    } else {
        r.gn = norms[b * 3 + 0] + 1e-12f;
        if (STAGE == 2) r.n1 = reduced;
        if (STAGE == 3) {
            r.n1 = norms[b * 3 + 1];
            r.n2 = reduced;
        }
    }
    if (tile == 0 && threadIdx.x == 0) norms[b * 3 + (STAGE - 1)] = reduced;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const int64_t q = quad_of(tile, j);
        const float4 c = load4<VEC>(cur + o, T, q, 0.0f);
        const float4 p = STAGE >= 2 ? load4<VEC>(prev + o, T, q, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 g = load4<VEC>(grad + o, T, q, 0.0f);
        const float4 xv = load4<VEC>(x + o, T, q, 0.0f);
        float4 v;
        v.x = l2_chain<STAGE>(c.x, p.x, g.x, xv.x, r);
        v.y = l2_chain<STAGE>(c.y, p.y, g.y, xv.y, r);
        v.z = l2_chain<STAGE>(c.z, p.z, g.z, xv.z, r);
        v.w = l2_chain<STAGE>(c.w, p.w, g.w, xv.w, r);
        if (STAGE == 3) {
            store4<VEC>(out + o, T, q, v);
        } else {
            s += sumsq4(zero_outside_row(v, T, q));  // out-of-row lanes must not leak a 0/0 into the sum
        }
    }
    if (STAGE != 3) {
        s = wg_sum(s, lds + 4);
        if (threadIdx.x == 0) part_out[b * C + tile] = s;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------

template <bool PHILOX>
int apgd_init(const float *x, const float *draw, float *out, int64_t B, int64_t T, int norm, float eps, float lo, float hi,
              uint64_t seed, uint64_t offset, void *ws, size_t ws_bytes, hipStream_t st) {
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    const bool vec = rows_vec(T, {x, draw, out});
    launch_tiles(ROW_KERNEL_PAIR(apgd_init_reduce_kernel, PHILOX), vec, B, T, st, draw, T, norm, seed, offset, w.p0);
    launch_tiles(ROW_KERNEL_PAIR(apgd_init_apply_kernel, PHILOX), vec, B, T, st, x, draw, out, T, norm, eps, lo, hi, seed, offset,
                 w.p0);
    return status_after_launch();
}

}  // namespace

extern "C" {

int advstep_apgd_init_noise_f32(const float *x, const float *draw, float *out, int64_t B, int64_t T, int norm, float eps,
                                float lo, float hi, void *ws, size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY && (norm == kNormLinf || norm == kNormL2));
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && draw && out && !overlaps(draw, out, (size_t)B * T * sizeof(float)));
    return apgd_init<false>(x, draw, out, B, T, norm, eps, lo, hi, 0, 0, ws, ws_bytes, as_stream(stream));
}

int advstep_apgd_init_philox_f32(const float *x, float *out, int64_t B, int64_t T, int norm, float eps, float lo, float hi,
                                 uint64_t seed, uint64_t offset, void *ws, size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY && (norm == kNormLinf || norm == kNormL2));
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && out);
    return apgd_init<true>(x, nullptr, out, B, T, norm, eps, lo, hi, seed, offset, ws, ws_bytes, as_stream(stream));
}

int advstep_apgd_eval_f32(const float *z, const int64_t *labels, float *dz, float *loss, int mode, int64_t i, uint8_t *acc,
                          uint8_t *flags, float *loss_best, float *loss_best_last_check, uint8_t *reduced_last_check,
                          float *loss_steps, int64_t B, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 1 && z && labels && dz && loss && mode >= 0 && mode <= 2);
    if (mode == 1) ADVSTEP_REQUIRE(acc && flags && loss_best && loss_best_last_check && reduced_last_check);
    if (mode == 2) ADVSTEP_REQUIRE(acc && flags && loss_best && loss_steps && i >= 0);
    hipLaunchKernelGGL(apgd_eval_kernel, dim3(1), dim3(kWgThreads), 0, as_stream(stream), z, labels, dz, loss, mode, i, acc,
                       flags, loss_best, loss_best_last_check, reduced_last_check, loss_steps, B);
    return status_after_launch();
}

int advstep_apgd_checkpoint_f32(const float *loss_steps, int64_t steps, int64_t i, int64_t k, double rho,
                                const float *loss_best, float *loss_best_last_check, uint8_t *reduced_last_check,
                                float *step_size, uint8_t *flags, int64_t B, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 1 && steps >= 1 && i >= 0 && i < steps && k >= 1 && i - k >= -1);
    ADVSTEP_REQUIRE(loss_steps && loss_best && loss_best_last_check && reduced_last_check && step_size && flags);
    hipLaunchKernelGGL(apgd_checkpoint_kernel, dim3(1), dim3(kWgThreads), 0, as_stream(stream), loss_steps, steps, i, k, rho,
                       loss_best, loss_best_last_check, reduced_last_check, step_size, flags, B);
    return status_after_launch();
}

int advstep_apgd_track_f32(float *x_adv, float *grad, float *x_best, float *grad_best, float *x_best_adv,
                           const uint8_t *flags, int64_t B, int64_t T, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x_adv && grad && x_best && grad_best && x_best_adv && flags);
    hipStream_t st = as_stream(stream);
    launch_tiles(ROW_KERNEL_PAIR(apgd_track_kernel), rows_vec(T, {x_adv, grad, x_best, grad_best, x_best_adv}), B, T, st, x_adv,
                 grad, x_best, grad_best, x_best_adv, flags, T);
    return status_after_launch();
}

int advstep_apgd_linf_step_f32(const float *cur, const float *prev, const float *grad, const float *x, const float *step_size,
                               float *out, int64_t B, int64_t T, float eps, double a, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && prev && grad && x && step_size && out);
    const size_t bytes = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(out, cur, bytes) && !overlaps(out, grad, bytes) && !overlaps(out, x, bytes));
    hipStream_t st = as_stream(stream);
    const float af = (float)a, oma = (float)(1.0 - a);
    launch_tiles(ROW_KERNEL_PAIR(apgd_linf_step_kernel), rows_vec(T, {cur, prev, grad, x, out}), B, T, st, cur, prev, grad, x,
                 step_size, out, T, eps, af, oma);
    return status_after_launch();
}

int advstep_apgd_l2_step_f32(const float *cur, const float *prev, const float *grad, const float *x, const float *step_size,
                             float *out, float *norms, int64_t B, int64_t T, float eps, double a, void *ws, size_t ws_bytes,
                             advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && prev && grad && x && step_size && out && norms);
    const size_t bytes = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(out, cur, bytes) && !overlaps(out, grad, bytes) && !overlaps(out, x, bytes));
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const float af = (float)a, oma = (float)(1.0 - a);
    const bool vec = rows_vec(T, {cur, prev, grad, x, out});
    launch_tiles(ROW_KERNEL_PAIR(sumsq_partial_kernel), vec, B, T, st, grad, T, w.p0);
    launch_tiles(ROW_KERNEL_PAIR(apgd_l2_pass_kernel, 1), vec, B, T, st, cur, prev, grad, x, step_size, out, norms, T, eps, af, oma,
                 w.p0, w.p1);
    launch_tiles(ROW_KERNEL_PAIR(apgd_l2_pass_kernel, 2), vec, B, T, st, cur, prev, grad, x, step_size, out, norms, T, eps, af, oma,
                 w.p1, w.p0);
    launch_tiles(ROW_KERNEL_PAIR(apgd_l2_pass_kernel, 3), vec, B, T, st, cur, prev, grad, x, step_size, out, norms, T, eps, af, oma,
                 w.p0, nullptr);
    return status_after_launch();
}

}  // extern "C"
