// row_project.h — the two sparse projections of a row that one 1024-thread workgroup owns (internal: not part of the C ABI in
// include/): the exact projection onto the L1 ball intersected with the box [0, 1] (include/advstep_apgdl1.h has the
// definition) and the exact-k projection onto the L0 ball intersected with the box and a per-sample cap
// (include/advstep_l0.h).  apgdl1.hip and l0.hip launch them with one radius for the whole batch; fmn_sparse.hip with the
// radius its own decision gave the row.  Both are sort-free: row_workgroup.h's digit_search over the 31 bits of a
// non-negative float's pattern, and for L0's ties over the bits of the sample index.  Include after row_workgroup.h.
//
// Every pass traverses with row_workgroup.h's order (visit_rows_ahead / map_rows), so a thread only ever re-reads samples it
// wrote itself: the passes over an output row that is also the input row need no barrier beyond the reductions'.
// lds: kCand * kRowWaves floats, free again on return.  Built with -ffp-contract=off.

#ifndef ADVSTEP_ROW_PROJECT_H
#define ADVSTEP_ROW_PROJECT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_common.h"
#include "row_workgroup.h"

namespace {

// ---- L1: the box-aware projection ------------------------------------------------------------------------------------------

// m_i(lam) = min(max(|d_i| - lam, 0), cap_i): how far coordinate i moves from x_i towards u_i.  The median of the three is
// that value whenever 0 <= cap (x in [0, 1]), in one instruction instead of two; the searches' passes are VALU-bound.
__device__ __forceinline__ float l1_move(float ad, float cap, float lam) {
    return __builtin_amdgcn_fmed3f(ad - lam, 0.0f, cap);
}
__device__ __forceinline__ float l1_cap(float d, float xi) { return d > 0.0f ? 1.0f - xi : xi; }

// (the search passes traverse with row_workgroup.h's visit_rows_ahead: the next element's loads before this one's arithmetic)

// out row = P(u row; x row, eps), phi0 = phi(0) as the caller's pass over (x, u) summed it.  ur may be outr.
// ROUTE: row_workgroup.h's traversal route (a kernel's bool VEC converts)
template <int ROUTE>
__device__ __forceinline__ void l1_box_project_row(const float *xr, const float *ur, float *outr, int64_t T, float eps,
                                                   float phi0, float *lds) {
    float lam = 0.0f;
    if (phi0 > eps) {                                          // workgroup-uniform: every thread holds the same phi0
        // rho = the largest bit pattern with phi > eps (phi(0) > eps: it exists); lam* is the next float
        float h[kCand];
        const uint32_t rho = digit_search(
            31, h, lds,
            [&](uint32_t lo, int shift, float(&hh)[kCand]) {   // bin k = phi at candidate k + 1 itself: nothing to accumulate
                float cand[kCand];
#pragma unroll
                for (int k = 0; k < kCand; ++k) cand[k] = __uint_as_float(lo | ((uint32_t)(k + 1) << shift));
                visit_rows_ahead<ROUTE, 2>({xr, ur}, T, [&](const float (&xu)[2]) {
                    const float d = xu[1] - xu[0], ad = fabsf(d), cap = l1_cap(d, xu[0]);
#pragma unroll
                    for (int k = 0; k < kCand; ++k) hh[k] += l1_move(ad, cap, cand[k]);
                });
            },
            [&](float phi) { return phi > eps; });             // phi is non-increasing: the first candidate that fits ends the scan
        lam = __uint_as_float(rho + 1u);
    }
    map_rows<ROUTE>({xr, ur}, outr, T, [&](float xi, float ui) {
        const float d = ui - xi;
        return clampf(xi + sgn(d) * l1_move(fabsf(d), l1_cap(d, xi), lam), 0.0f, 1.0f);
    });
}

// one term of phi(0) for the sample (x_i, u_i)
__device__ __forceinline__ float l1_move0(float xi, float ui) {
    const float d = ui - xi;
    return l1_move(fabsf(d), l1_cap(d, xi), 0.0f);
}

// ---- L0: the exact-k projection --------------------------------------------------------------------------------------------

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
template <int ROUTE>
__device__ __forceinline__ void l0_project_row(const float *xr, const float *ur, float *outr, int64_t T, float kk, float cap,
                                               float *stats, float *lds) {
    // rho = the largest pattern with #{key >= rho} >= kk, which is the kk-th largest key; `above` is that count
    float h[kCand], above = (float)T;
    const uint32_t rho = digit_search(
        31, h, lds,
        [&](uint32_t lo, int shift, float(&hh)[kCand]) {
            visit_rows_ahead<ROUTE, 2>({xr, ur}, T, [&](const float(&xu)[2]) {
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
                visit_rows_ahead<ROUTE, 2>({xr, ur}, T, [&](int64_t i, const float(&xu)[2]) {
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
    map_rows<ROUTE>({xr, ur}, outr, T, [&](int64_t i, float xi, float ui) {
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

}  // namespace

#endif  // ADVSTEP_ROW_PROJECT_H
