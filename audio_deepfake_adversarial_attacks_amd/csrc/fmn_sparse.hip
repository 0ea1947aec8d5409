// fmn_sparse.hip — gfx950 (MI355X / CDNA4) kernel of the sparse forms of the minimal-norm attack (torchattacks.FMNSparse) + the
// C ABI declared in include/advstep_fmn_sparse.h: FMN's recurrence (fmn.hip) for the L1 and the L0 threat model, composed with
// the two sort-free sparse projections of row_project.h (apgdl1.hip's box-aware L1 projection, l0.hip's exact-k projection),
// each into a radius PER ROW that the same launch has just decided.
//
// Layout as apgdl1.hip and l0.hip (row_workgroup.h): one workgroup of 1024 threads per row, the row re-read from L2 by every
// pass, float4 loads where the rows allow, fixed-order reductions.  Because one workgroup owns its row, the row's norms, its
// decision, the copy of an improved iterate, the move and the projection are ONE launch without a workspace: nothing has to
// cross a launch boundary, where fmn.hip's (tile, row) grid needs a norms launch, partial planes and, in L2, a third launch.
// A thread only ever re-reads samples it wrote itself (the traversals give every pass the same sample -> thread map), so the
// passes over the output row — which may be the input row — need no barrier beyond the reductions'.
//
// Algorithmic bytes per row sample: 12 (adv, orig, grad: the norms, the only first touches) + 12 + 4 (the move: adv, grad, orig
// -> u) + the projection's passes over (orig, u) at 8 each (L1: 11 when phi(0) > eps'; L0: 11 [+ ceil(bits(T - 1) / 3) for the
// cut]) + 12 for its last pass; + 8 per sample of an improved row.  Built with -ffp-contract=off; divisions and square roots
// are IEEE; clamps, minima and maxima propagate NaN.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_fmn_sparse.h"
#include "advstep_common.h"
#include "row_workgroup.h"
#include "row_project.h"

namespace {

enum { kNormL1 = 2, kNormL0 = 3 };                   // include/advstep_fmn.h's numbering, continued
enum { kFormLast = 0, kFormMove = 1 };               // what the launch does after the decision and the copy

// One row.  FORM = kFormLast: the norms of d, the decision and the copy.  kFormMove: ... and the norms of g, the move and the
// projection into the row's new radius (out may be adv: a thread reads its own samples before it writes them).
template <int ROUTE, int NORM, int FORM>
__device__ __forceinline__ void fmn_sparse_row(const float *adv, const float *__restrict__ grad, const float *__restrict__ orig,
                                               const float *__restrict__ z, const int64_t *__restrict__ labels,
                                               const float *__restrict__ state, float *__restrict__ state_out,
                                               float *__restrict__ best_adv, float *out, float *__restrict__ row_norms,
                                               float alpha, float gamma, float eps_div, int64_t B, int64_t T, int64_t row,
                                               float *lds) {
    const float *ar = adv + row * T, *xr = orig + row * T;
    // ---- pass 1: dabs, dcnt, gsq and gmax ------------------------------------------------------------------------------
    float s[3] = {0.0f, 0.0f, 0.0f}, m[1] = {0.0f};
    if (FORM == kFormMove) {
        visit_rows<ROUTE>({ar, xr, grad + row * T}, T, [&](float ai, float xi, float gi) {
            const float d = ai - xi;
            s[0] += fabsf(d);
            s[1] += d != 0.0f ? 1.0f : 0.0f;
            s[2] += gi * gi;
            m[0] = max_nan(m[0], fabsf(gi));
        });
    } else {
        visit_rows<ROUTE>({ar, xr}, T, [&](float ai, float xi) {
            const float d = ai - xi;
            s[0] += fabsf(d);
            s[1] += d != 0.0f ? 1.0f : 0.0f;
        });
    }
    row_reduce<3>(s, SumOp(), lds);
    row_reduce<1>(m, MaxNanOp(), lds);
    const float dabs = s[0], dcnt = s[1], gsq = s[2], gmax = m[0];
    // ---- the decision: every thread derives the same values --------------------------------------------------------------
    const float dn = NORM == kNormL1 ? dabs : dcnt;
    const float e = state[0 * B + row], best = state[1 * B + row];
    const bool found = state[2 * B + row] != 0.0f;
    const float zb = z[row];
    const bool is_adv = judged_wrong(zb, labels[row]);
    const bool better = is_adv && dn < best;
    const float best1 = better ? dn : best;
    float eps1;
    if (NORM == kNormL1) {                                 // fmn.hip's fmn_decide, with the dual norm max |g|
        if (is_adv) {
            eps1 = min_nan(e, best1) * (1.0f - gamma);
        } else if (found) {
            eps1 = e * (1.0f + gamma);
        } else {
            eps1 = (dn + (gmax > 0.0f ? fabsf(zb) / gmax : INFINITY)) * (1.0f + gamma);
        }
    } else {                                               // the paper's integer rule; begin's +inf is the starting radius 1
        const float e1 = e == INFINITY ? 1.0f : e;
        eps1 = is_adv ? min_nan(min_nan(e1 - 1.0f, floorf(e1 * (1.0f - gamma))), best1)
                      : max_nan(e1 + 1.0f, floorf(e1 * (1.0f + gamma)));
        eps1 = clampf(eps1, 0.0f, (float)T);
    }
    if (threadIdx.x == 0) {
        state_out[0 * B + row] = eps1;
        state_out[1 * B + row] = best1;
        state_out[2 * B + row] = (found || is_adv) ? 1.0f : 0.0f;
        state_out[3 * B + row] = dn;
        if (row_norms) {
            row_norms[0 * B + row] = dabs;
            row_norms[1 * B + row] = dcnt;
            row_norms[2 * B + row] = gsq;
            row_norms[3 * B + row] = gmax;
        }
    }
    // ---- the copy: before the move, by the threads that will overwrite these samples where out is adv -------------------
    if (better) map_rows<ROUTE>({ar}, best_adv + row * T, T, [](float ai) { return ai; });   // uniform over the workgroup
    if (FORM == kFormMove) {
        const float *gr = grad + row * T;
        float *orow = out + row * T;
        const float gn = sqrtf(gsq) + eps_div;
        if (NORM == kNormL1) {
            float phi[1] = {0.0f};                         // u into the output row, phi(0) on the way
            map_rows<ROUTE>({ar, gr, xr}, orow, T, [&](float ai, float gi, float xi) {
                const float ui = ai + alpha * (gi / gn);
                phi[0] += l1_move0(xi, ui);
                return ui;
            });
            row_reduce<1>(phi, SumOp(), lds);
            l1_box_project_row<ROUTE>(xr, orow, orow, T, eps1, phi[0], lds);
        } else {
            const float kk = min_nan(eps1, (float)T);
            if (kk < 1.0f) {                               // uniform; l0_project_row is not defined for kk = 0
                map_rows<ROUTE>({xr}, orow, T, [](float xi) { return xi; });
            } else {
                map_rows<ROUTE>({ar, gr}, orow, T, [&](float ai, float gi) { return ai + alpha * (gi / gn); });
                l0_project_row<ROUTE>(xr, orow, orow, T, kk, INFINITY, nullptr, lds);
            }
        }
    }
}

// VEC: 16-byte accesses (T % 4 == 0, every waveform base aligned).  Otherwise 4-byte accesses: in the quads' order where
// T % 4 == 0 — a base off the 16-byte grid then changes no bit of any result — and sample by sample where it is not.
template <bool VEC, int NORM, int FORM>
__global__ __launch_bounds__(kRow) void fmn_sparse_step_kernel(const float *adv, const float *__restrict__ grad,
                                                               const float *__restrict__ orig, const float *__restrict__ z,
                                                               const int64_t *__restrict__ labels,
                                                               const float *__restrict__ state, float *__restrict__ state_out,
                                                               float *__restrict__ best_adv, float *out,
                                                               float *__restrict__ row_norms, float alpha, float gamma,
                                                               float eps_div, int64_t B, int64_t T) {
    __shared__ float lds[kCand * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        if (VEC)
            fmn_sparse_row<kRouteQuads, NORM, FORM>(adv, grad, orig, z, labels, state, state_out, best_adv, out, row_norms, alpha,
                                                    gamma, eps_div, B, T, row, lds);
        else if ((T & 3) == 0)                                 // uniform
            fmn_sparse_row<kRouteQuadsBySample, NORM, FORM>(adv, grad, orig, z, labels, state, state_out, best_adv, out, row_norms,
                                                            alpha, gamma, eps_div, B, T, row, lds);
        else
            fmn_sparse_row<kRouteSamples, NORM, FORM>(adv, grad, orig, z, labels, state, state_out, best_adv, out, row_norms, alpha,
                                                      gamma, eps_div, B, T, row, lds);
    }
}

}  // namespace

extern "C" {

int advstep_fmn_sparse_step_f32(const float *adv, const float *grad, const float *orig, const float *z, const int64_t *labels,
                                const float *state, float *state_out, float *best_adv, float *out, float *row_norms,
                                float alpha, float gamma, int norm, int move, float eps_div, int64_t B, int64_t T,
                                advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY && T < kMaxRowLength);
    ADVSTEP_REQUIRE((norm == kNormL1 || norm == kNormL0) && gamma > 0.0f && gamma < 1.0f);   // (a NaN fails the comparisons)
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && orig && z && labels && state && state_out && best_adv);
    if (move) ADVSTEP_REQUIRE(grad && out && alpha >= 0.0f && eps_div >= 0.0f);
    const size_t rows = (size_t)B * T * sizeof(float), planes = 4 * (size_t)B * sizeof(float);
    const size_t per_f = (size_t)B * sizeof(float), per_y = (size_t)B * sizeof(int64_t);
    ADVSTEP_REQUIRE(!overlaps(state, state_out, planes));   // ping-pong: the launch never reads what it writes
    ADVSTEP_REQUIRE(!overlaps(best_adv, adv, rows) && !overlaps(best_adv, orig, rows) && !(grad && overlaps(best_adv, grad, rows)));
    ADVSTEP_REQUIRE(!overlap2(best_adv, rows, state, planes) && !overlap2(best_adv, rows, state_out, planes) &&
                    !overlap2(best_adv, rows, z, per_f) && !overlap2(best_adv, rows, labels, per_y));
    ADVSTEP_REQUIRE(!overlap2(state_out, planes, z, per_f) && !overlap2(state_out, planes, labels, per_y) &&
                    !overlap2(state_out, planes, adv, rows) && !overlap2(state_out, planes, orig, rows) &&
                    !(grad && overlap2(state_out, planes, grad, rows)));
    if (row_norms)
        ADVSTEP_REQUIRE(!overlap2(row_norms, planes, state, planes) && !overlap2(row_norms, planes, state_out, planes) &&
                        !overlap2(row_norms, planes, z, per_f) && !overlap2(row_norms, planes, labels, per_y) &&
                        !overlap2(row_norms, planes, best_adv, rows) && !overlap2(row_norms, planes, adv, rows) &&
                        !overlap2(row_norms, planes, orig, rows) && !(grad && overlap2(row_norms, planes, grad, rows)));
    if (move) {
        ADVSTEP_REQUIRE(out == adv || !overlaps(out, adv, rows));
        ADVSTEP_REQUIRE(!overlaps(out, grad, rows) && !overlaps(out, orig, rows) && !overlaps(out, best_adv, rows));
        ADVSTEP_REQUIRE(!overlap2(out, rows, state, planes) && !overlap2(out, rows, state_out, planes) &&
                        !overlap2(out, rows, z, per_f) && !overlap2(out, rows, labels, per_y) &&
                        !(row_norms && overlap2(out, rows, row_norms, planes)));
    }
    if (!move) {
        const bool vec = rows_vec(T, {adv, orig, best_adv});
        if (norm == kNormL1)
            return launch_rows(ROW_KERNEL_PAIR(fmn_sparse_step_kernel, kNormL1, kFormLast), vec, B, stream, adv, grad, orig, z,
                               labels, state, state_out, best_adv, out, row_norms, alpha, gamma, eps_div, B, T);
        return launch_rows(ROW_KERNEL_PAIR(fmn_sparse_step_kernel, kNormL0, kFormLast), vec, B, stream, adv, grad, orig, z, labels,
                           state, state_out, best_adv, out, row_norms, alpha, gamma, eps_div, B, T);
    }
    const bool vec = rows_vec(T, {adv, grad, orig, best_adv, out});
    if (norm == kNormL1)
        return launch_rows(ROW_KERNEL_PAIR(fmn_sparse_step_kernel, kNormL1, kFormMove), vec, B, stream, adv, grad, orig, z, labels,
                           state, state_out, best_adv, out, row_norms, alpha, gamma, eps_div, B, T);
    return launch_rows(ROW_KERNEL_PAIR(fmn_sparse_step_kernel, kNormL0, kFormMove), vec, B, stream, adv, grad, orig, z, labels,
                       state, state_out, best_adv, out, row_norms, alpha, gamma, eps_div, B, T);
}

}  // extern "C"
