// apgdl1.hip — gfx950 (MI355X / CDNA4) kernels of l1-APGD (Croce & Hein, "Mind the box: l1-APGD for sparse adversarial
// attacks on image classifiers", ICML 2021) + the C ABI declared in include/advstep_apgdl1.h: the exact projection onto the
// L1 ball intersected with the box [0, 1], the sparse top-k sign step fused with it, the random start and the sparsity
// checkpoint.  The per-row loss / flags and the best-point tracking are apgd.hip's (advstep_apgd_eval / _track).
//
// Layout as fab.hip (row_workgroup.h): one workgroup of 1024 threads per row, the row re-read from L2 by every pass, float4
// loads where the rows allow, fixed-order reductions.  No sort: both per-row searches (the projection's lambda, the step's
// top-k rank) are row_workgroup.h's digit_search over the 31 bits of a non-negative float's pattern, 11 streaming passes
// each.  A thread only ever re-reads samples it wrote itself (the traversal gives every pass the same sample -> thread
// map), so the passes over the output row need no barrier beyond the reductions'.
//
// Algorithmic bytes per row sample: step 4 x 12 (grad) + 12 + 4 (cur, grad, x -> u) + 8 x 12 (x, u) + 4 = 164 B, of which
// 20 B are first touches and the rest L2 / Infinity-Cache re-reads; projection alone 8 x 13 + 4; checkpoint 8 B.
// Built with -ffp-contract=off; divisions are IEEE.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "advstep_apgdl1.h"
#include "advstep_common.h"
#include "row_workgroup.h"
#include "row_project.h"

namespace {

constexpr uint8_t kImproved = 2, kReset = 4;           // the flag bits of include/advstep_apgd.h

// ---- the projection --------------------------------------------------------------------------------------------------

// l1_move, l1_cap, l1_move0 and l1_box_project_row are row_project.h's (fmn_sparse.hip projects with them too)

template <bool VEC>
__global__ __launch_bounds__(kRow) void l1_box_project_kernel(const float *__restrict__ x, const float *u, float *out,
                                                              int64_t B, int64_t T, float eps) {
    __shared__ float lds[kCand * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float *xr = x + row * T, *ur = u + row * T;
        float phi[1] = {0.0f};
        visit_rows<VEC>({xr, ur}, T, [&](float xi, float ui) { phi[0] += l1_move0(xi, ui); });
        row_reduce<1>(phi, SumOp(), lds);
        l1_box_project_row<VEC>(xr, ur, out + row * T, T, eps, phi[0], lds);
    }
}

// ---- the step: top-k threshold by radix selection, sparse sign step, projection -------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kRow) void apgdl1_step_kernel(const float *cur, const float *__restrict__ grad,
                                                           const float *__restrict__ x,
                                                           const float *__restrict__ step_size,
                                                           const float *__restrict__ topk, float *out,
                                                           float *__restrict__ stats, int64_t B, int64_t T, float eps) {
    __shared__ float lds[kCand * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float *cr = cur + row * T, *gr = grad + row * T, *xr = x + row * T;
        float *orow = out + row * T;
        // n = the rank of the threshold in the ascending order of |g|, as a float (T < 2^24: exact)
        float n = truncf(clampf((1.0f - topk[row]) * (float)T, 0.0f, (float)(T - 1)));
        if (!(n >= 0.0f)) n = 0.0f;                            // a NaN topk
        // rho = the largest key with #{key_i < rho} <= n, which is the key of rank n; `below` is that count
        float h[kCand], below = 0.0f;
        const uint32_t rho = digit_search(
            31, h, lds,
            [&](uint32_t lo, int shift, float(&hh)[kCand]) {
                visit_rows_ahead<VEC, 1>({gr}, T, [&](const float (&gi)[1]) {
                    bucket_add(hh, __float_as_uint(gi[0]) & 0x7FFFFFFFu, lo, shift, 1.0f);   // |g|'s pattern: NaN sorts above +inf
                });
            },
            [&](float hj) {                                    // #{key < candidate j} = below + h[0..j)
                const float at = below + hj;
                if (!(at <= n)) return false;
                below = at;
                return true;
            });
        const float thr = __uint_as_float(rho);
        float cnt[1] = {0.0f};
        visit_rows<VEC>({gr}, T, [&](float gi) { cnt[0] += (fabsf(gi) >= thr && gi != 0.0f) ? 1.0f : 0.0f; });
        row_reduce<1>(cnt, SumOp(), lds);
        if (threadIdx.x == 0 && stats) {
            stats[2 * row] = thr;
            stats[2 * row + 1] = cnt[0];
        }
        // u into the output row, phi(0) on the way
        const float st = step_size[row], den = cnt[0] + 1e-10f;
        float phi[1] = {0.0f};
        map_rows<VEC>({cr, gr, xr}, orow, T, [&](float ci, float gi, float xi) {
            const float s = fabsf(gi) >= thr ? sgn(gi) : 0.0f;
            const float ui = ci + (st * s) / den;
            phi[0] += l1_move0(xi, ui);
            return ui;
        });
        row_reduce<1>(phi, SumOp(), lds);
        l1_box_project_row<VEC>(xr, orow, orow, T, eps, phi[0], lds);
    }
}

// ---- the random start ------------------------------------------------------------------------------------------------------

// u = x + t into the output row in the traversal's order (quads q = threadIdx.x, += kRow; samples likewise), t from the
// caller's draw or the Philox normals of quad q of the row; then the projection.
template <bool VEC, bool PHILOX>
__global__ __launch_bounds__(kRow) void apgdl1_init_kernel(const float *__restrict__ x, const float *draw, float *out,
                                                           int64_t B, int64_t T, float eps, uint64_t seed,
                                                           uint64_t offset) {
    __shared__ float lds[kCand * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float *xr = x + row * T;
        float *orow = out + row * T;
        float phi[1] = {0.0f};
        if constexpr (VEC) {
            const int64_t n4 = T >> 2;
            for (int64_t q = threadIdx.x; q < n4; q += kRow) {
                const float4 xv = reinterpret_cast<const float4 *>(xr)[q];
                float4 t;
                if constexpr (PHILOX) t = philox_normal4((uint32_t)q, (uint32_t)row, seed, offset);
                else t = reinterpret_cast<const float4 *>(draw + row * T)[q];
                const float4 u = make_float4(xv.x + t.x, xv.y + t.y, xv.z + t.z, xv.w + t.w);
                phi[0] += l1_move0(xv.x, u.x);
                phi[0] += l1_move0(xv.y, u.y);
                phi[0] += l1_move0(xv.z, u.z);
                phi[0] += l1_move0(xv.w, u.w);
                reinterpret_cast<float4 *>(orow)[q] = u;
            }
        } else {
            for (int64_t i = threadIdx.x; i < T; i += kRow) {
                float t;
                if constexpr (PHILOX) {
                    const float4 n4 = philox_normal4((uint32_t)(i >> 2), (uint32_t)row, seed, offset);
                    const int k = (int)(i & 3);
                    t = k == 0 ? n4.x : (k == 1 ? n4.y : (k == 2 ? n4.z : n4.w));
                } else {
                    t = draw[row * T + i];
                }
                const float xi = xr[i], ui = xi + t;
                phi[0] += l1_move0(xi, ui);
                orow[i] = ui;
            }
        }
        row_reduce<1>(phi, SumOp(), lds);
        l1_box_project_row<VEC>(xr, orow, orow, T, eps, phi[0], lds);
    }
}

// ---- the sparsity checkpoint ---------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kRow) void apgdl1_checkpoint_kernel(const float *__restrict__ cur,
                                                                 const float *__restrict__ x_best,
                                                                 const float *__restrict__ x, uint8_t *flags, float *sp_old,
                                                                 float *topk, float *step_size, int64_t B, int64_t T,
                                                                 float eps) {
    __shared__ float lds[kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const uint8_t f = flags[row];                          // read by every thread before thread 0 writes it below
        const float *br = ((f & kImproved) ? cur : x_best) + row * T;
        float sp[1] = {0.0f};
        visit_rows<VEC>({br, x + row * T}, T, [&](float bi, float xi) { sp[0] += (bi - xi != 0.0f) ? 1.0f : 0.0f; });
        row_reduce<1>(sp, SumOp(), lds);
        if (threadIdx.x == 0) {
            const bool red = (sp[0] / sp_old[row]) < 0.95f;
            topk[row] = (sp[0] / (float)T) / 1.5f;
            step_size[row] = clampf(red ? eps : step_size[row] / 1.5f, eps / 10.0f, eps);
            sp_old[row] = sp[0];
            flags[row] = (uint8_t)((f & ~kReset) | (red ? kReset : 0));
        }
    }
}

template <bool PHILOX>
int apgdl1_init(const float *x, const float *draw, float *out, int64_t B, int64_t T, float eps, uint64_t seed,
                uint64_t offset, advstep_stream_t stream) {
    static constexpr decltype(&apgdl1_init_kernel<true, PHILOX>) kernels[2] = {apgdl1_init_kernel<false, PHILOX>,
                                                                               apgdl1_init_kernel<true, PHILOX>};
    return launch_rows(kernels, rows_vec(T, {x, draw, out}), B, stream, x, draw, out, B, T, eps, seed, offset);
}

}  // namespace

extern "C" {

int advstep_l1_box_project_f32(const float *x, const float *u, float *out, float eps, int64_t B, int64_t T,
                               advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && eps > 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && x && u && out && !overlaps(out, x, (size_t)B * T * sizeof(float)));
    return launch_rows(ROW_KERNEL_PAIR(l1_box_project_kernel), rows_vec(T, {x, u, out}), B, stream, x, u, out, B, T, eps);
}

int advstep_apgdl1_step_f32(const float *cur, const float *grad, const float *x, const float *step_size, const float *topk,
                            float *out, float *stats, int64_t B, int64_t T, float eps, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && eps > 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && cur && grad && x && step_size && topk && out);
    const size_t bytes = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(out, grad, bytes) && !overlaps(out, x, bytes));
    ADVSTEP_REQUIRE(!stats || !overlap2(stats, (size_t)B * 2 * sizeof(float), out, bytes));
    return launch_rows(ROW_KERNEL_PAIR(apgdl1_step_kernel), rows_vec(T, {cur, grad, x, out}), B, stream, cur, grad, x,
                       step_size, topk, out, stats, B, T, eps);
}

int advstep_apgdl1_init_f32(const float *x, const float *draw, float *out, int64_t B, int64_t T, float eps,
                            advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && eps > 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && x && draw && out && !overlaps(out, x, (size_t)B * T * sizeof(float)));
    return apgdl1_init<false>(x, draw, out, B, T, eps, 0, 0, stream);
}

int advstep_apgdl1_init_philox_f32(const float *x, float *out, int64_t B, int64_t T, float eps, uint64_t seed,
                                   uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && eps > 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && x && out && !overlaps(out, x, (size_t)B * T * sizeof(float)));
    return apgdl1_init<true>(x, nullptr, out, B, T, eps, seed, offset, stream);
}

int advstep_apgdl1_checkpoint_f32(const float *cur, const float *x_best, const float *x, uint8_t *flags, float *sp_old,
                                  float *topk, float *step_size, int64_t B, int64_t T, float eps,
                                  advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && eps > 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && cur && x_best && x && flags && sp_old && topk && step_size);
    return launch_rows(ROW_KERNEL_PAIR(apgdl1_checkpoint_kernel), rows_vec(T, {cur, x_best, x}), B, stream, cur, x_best, x,
                       flags, sp_old, topk, step_size, B, T, eps);
}

}  // extern "C"
