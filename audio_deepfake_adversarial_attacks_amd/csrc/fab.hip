// fab.hip — the FAB attack's per-iteration tensor work on gfx950 (C ABI: include/advstep_fab.h).
//
// Reference: adversarial_attacks/torchattacks/attacks/fab.py:208-292 (loop body), :562-717 (projections).
//
// Layout: every kernel gives ONE workgroup of 1024 threads (16 wave64) to ONE row of T samples.  At the repo's
// T = 64 600 a row is 258 KB: it does not fit LDS, but the (t, w) pair of a row stays L2 / Infinity-Cache resident
// between the passes its workgroup makes over it, so only the first pass reads HBM.  2B = 256 rows at B = 128 is one
// workgroup per CU.  Loads are float4 (rows are 16-byte aligned when T % 4 == 0), reductions are wave64 butterflies
// joined through LDS in a fixed order — deterministic, and every thread of the workgroup sees the same scalar, which
// keeps the data-dependent iteration counts workgroup-uniform.
//
// From advstep_common.h: the NaN-propagating maximum, the reduction operators, the wave butterfly, rows_vec, kMaxGridY.
// From row_workgroup.h (shared with apgdl1.hip and l0.hip, the other files with 1024-thread rows): kRow, row_reduce, the
// row traversal (visit_rows / map_rows), the digit-walk search of the L1 projection (digit_search) and launch_rows.
//
// No sort: see include/advstep_fab.h.  Algorithmic bytes per row sample: hyperplane 8 B, projection 12 B (t, w in, d
// out; the re-reads of the fixed-point iteration hit L2), combine 20 B, backward step 8-20 B.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_fab.h"
#include "advstep_common.h"
#include "row_workgroup.h"

namespace {

constexpr int kMaxNewton = 64;   // the iteration is finite (<= number of breakpoints); in practice 3-8 passes
constexpr float kBig = 1e12f;

__device__ __forceinline__ float dual_norm_finish(float v, int kind) { return kind == ADVSTEP_FAB_L2 ? sqrtf(v) : v; }

// ---- hyperplane: row statistics of gz + the 2-logit selection ------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kRow) void fab_hyperplane_kernel(const float *__restrict__ gz, const float *__restrict__ x,
                                                              const float *__restrict__ z,
                                                              const int64_t *__restrict__ labels, float *wscale, float *b,
                                                              float *gnorm, float *gdot, int64_t B, int64_t T, int kind) {
    __shared__ float lds[2 * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float *g = gz + row * T, *xr = x + row * T;
        float dot[1] = {0.0f}, nrm[1] = {0.0f};
        if (kind == ADVSTEP_FAB_LINF) {
            visit_rows<VEC>({g, xr}, T, [&](float gi, float xi) { dot[0] += gi * xi; nrm[0] += fabsf(gi); });
        } else if (kind == ADVSTEP_FAB_L2) {
            visit_rows<VEC>({g, xr}, T, [&](float gi, float xi) { dot[0] += gi * xi; nrm[0] += gi * gi; });
        } else {
            // max_nan selects by a > b; torch.max's fmaxf differs from it only in which zero wins a (+0, -0) tie, and every
            // use in this file folds fabsf values into a 0.0f start, so no -0 occurs
            visit_rows<VEC>({g, xr}, T, [&](float gi, float xi) { dot[0] += gi * xi; nrm[0] = max_nan(nrm[0], fabsf(gi)); });
        }
        row_reduce<1>(dot, SumOp(), lds);
        if (kind == ADVSTEP_FAB_L1) row_reduce<1>(nrm, MaxNanOp(), lds + kRowWaves);
        else row_reduce<1>(nrm, SumOp(), lds + kRowWaves);
        if (threadIdx.x == 0) {
            const float n = dual_norm_finish(nrm[0], kind);
            if (gnorm) gnorm[row] = n;
            if (gdot) gdot[row] = dot[0];
            if (z && labels) {
                // y = [-z, z]; column k's gradient is (k ? +1 : -1) * gz
                const int la = labels[row] != 0;
                const float zz = z[row];
                const float y0 = -zz, y1 = zz, yla = la ? y1 : y0;
                const float s_la = la ? 1.0f : -1.0f;
                float dist[2], dfv[2], cv[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float c = (k ? 1.0f : -1.0f) - s_la;          // 0 or +-2
                    float df = (k ? y1 : y0) - yla;
                    if (k == la) df = 1e10f;
                    dfv[k] = df;
                    cv[k] = c;
                    dist[k] = fabsf(df) / (1e-12f + fabsf(c) * n);       // |c| in {0, 2}: scaling commutes with the norm
                }
                // torch.min over dim 1: first minimum, NaN wins
                int ind = 0;
                if (!(dist[0] != dist[0]) && ((dist[1] != dist[1]) || dist[1] < dist[0])) ind = 1;
                wscale[row] = cv[ind];
                b[row] = -dfv[ind] + cv[ind] * dot[0];
            }
        }
    }
}

// ---- projections ---------------------------------------------------------------------------------------------------
// Fixed point of  lam = (target - sum_{cap<=lam} wt*cap) / sum_{cap>lam} wt,  started from the all-active guess.
// `pass(lam, A, S, cnt)` streams the row once.  Monotone (lam only grows), ends when the active count repeats.
template <class Pass>
__device__ __forceinline__ float waterfill(float target, float total_weight, float n_active, Pass pass) {
    float lam = target / total_weight;
    float prev = n_active;
    for (int it = 0; it < kMaxNewton; ++it) {
        float A, S, cnt;
        pass(lam, A, S, cnt);
        if (cnt == prev) break;
        if (!(S > 0.0f)) return INFINITY;
        lam = fmaxf(lam, (target - A) / S);
        prev = cnt;
    }
    return lam;
}

template <bool VEC>
__global__ __launch_bounds__(kRow) void fab_projection_linf_kernel(const float *__restrict__ t,
                                                                   const float *__restrict__ w,
                                                                   const float *__restrict__ wscale,
                                                                   const float *__restrict__ b, float *__restrict__ d,
                                                                   float *__restrict__ dnorm, int64_t R, int64_t w_rows,
                                                                   int64_t T) {
    __shared__ float lds[5 * kRowWaves];
    for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
        const float *tr = t + row * T, *wr = w + (row % w_rows) * T;
        const float sc = wscale ? wscale[row % w_rows] : 1.0f;
        // pass 1: w.t, sum|w|, and sum|w| * room for both orientations of the hyperplane, count of w != 0
        float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        visit_rows<VEC>({tr, wr}, T, [&](float ti, float wraw) {
            const float wi = sc * wraw, aw = fabsf(wi);
            acc[0] += wi * ti;
            acc[1] += aw;
            acc[2] += aw * (wi < 0.0f ? 1.0f - ti : ti);
            acc[3] += aw * (wi > 0.0f ? 1.0f - ti : ti);
            acc[4] += (wi != 0.0f) ? 1.0f : 0.0f;
        });
        row_reduce<5>(acc, SumOp(), lds);
        const float c = acc[0] - b[row];
        const bool keep = c >= 0.0f;                  // fab.py:566: sign = 2 * ((w*t).sum(1) - b >= 0) - 1
        const float beta = fabsf(c);                  // -(b*sign - (w*sign * t).sum(1))
        const float reach = keep ? acc[2] : acc[3];   // -b0: what moving every coordinate to its box face buys
        float lam = INFINITY;
        if (reach - beta > 0.0f) {                    // fab.py:588  b - b0 > 0
            lam = waterfill(beta, acc[1], acc[4], [&](float cur, float &A, float &S, float &cnt) {
                float v[3] = {0.0f, 0.0f, 0.0f};
                visit_rows<VEC>({tr, wr}, T, [&](float ti, float wraw) {
                    const float wi = sc * wraw, aw = fabsf(wi);
                    const bool up = keep ? wi < 0.0f : wi > 0.0f;
                    const float p = up ? 1.0f - ti : ti;
                    const bool active = p > cur;
                    v[0] += active ? 0.0f : aw * p;
                    v[1] += active ? aw : 0.0f;
                    v[2] += (active && wi != 0.0f) ? 1.0f : 0.0f;
                });
                row_reduce<3>(v, SumOp(), lds);
                A = v[0];
                S = v[1];
                cnt = v[2];
            });
            lam = fmaxf(lam, 0.0f);                   // clamp_min(lmbd_opt, 0)
        }
        float mx[1] = {0.0f};
        map_rows<VEC>({tr, wr}, d + row * T, T, [&](float ti, float wraw) {
            const float wi = sc * wraw;
            const bool up = keep ? wi < 0.0f : wi > 0.0f;
            const float p = up ? 1.0f - ti : ti;
            const float m = fminf(lam, p);            // lam is never NaN here; p NaN propagates below
            float di = (p != p) ? p : (up ? m : -m);
            if (wi == 0.0f) di = 0.0f;
            mx[0] = max_nan(mx[0], fabsf(di));
            return di;
        });
        row_reduce<1>(mx, MaxNanOp(), lds);
        if (threadIdx.x == 0 && dnorm) dnorm[row] = mx[0];
    }
}

// fab.py:626-628: r = max(t/w, (t-1)/w) clamped to +-1e12, 1e12 where |w| < 1e-8, -1e12 -> 1e12
__device__ __forceinline__ float l2_ratio(float ti, float wi) {
    const float q1 = ti / wi, q2 = (ti - 1.0f) / wi;
    float r = (q1 != q1 || q2 != q2) ? NAN : fmaxf(q1, q2);
    r = (r != r) ? r : fminf(fmaxf(r, -kBig), kBig);
    if (fabsf(wi) < 1e-8f) r = kBig;
    if (r == -kBig) r = kBig;
    return r;
}

template <bool VEC>
__global__ __launch_bounds__(kRow) void fab_projection_l2_kernel(const float *__restrict__ t, const float *__restrict__ w,
                                                                 const float *__restrict__ wscale,
                                                                 const float *__restrict__ b, float *__restrict__ d,
                                                                 float *__restrict__ dnorm, int64_t R, int64_t w_rows,
                                                                 int64_t T) {
    __shared__ float lds[4 * kRowWaves];
    for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
        const float *tr = t + row * T, *wr = w + (row % w_rows) * T;
        const float sc = wscale ? wscale[row % w_rows] : 1.0f;
        // pass 1: w.t, sum w^2, and sum (r w) w over the movable coordinates for both orientations
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        visit_rows<VEC>({tr, wr}, T, [&](float ti, float wraw) {
            const float wi = sc * wraw;
            acc[0] += wi * ti;
            acc[1] += wi * wi;
            if (fabsf(wi) > 1e-8f) {
                acc[2] += (l2_ratio(ti, wi) * wi) * wi;
                acc[3] += (l2_ratio(ti, -wi) * wi) * wi;
            }
        });
        row_reduce<4>(acc, SumOp(), lds);
        const float c0 = acc[0] - b[row];
        const float sg = c0 >= 0.0f ? 1.0f : -1.0f;
        const float c = fabsf(c0);
        const float reach = sg > 0.0f ? acc[2] : acc[3];
        float alpha = INFINITY;
        if (!(c - reach > 0.0f)) {                   // fab.py:642  c3 = (d*w).sum + c > 0  -> every coordinate to its face
            alpha = waterfill(c, acc[1], (float)T, [&](float cur, float &A, float &S, float &cnt) {
                float v[3] = {0.0f, 0.0f, 0.0f};
                visit_rows<VEC>({tr, wr}, T, [&](float ti, float wraw) {
                    const float wi = sg * (sc * wraw);
                    const float r = l2_ratio(ti, wi), w2 = wi * wi;
                    const bool active = r > cur;
                    v[0] += active ? 0.0f : w2 * r;
                    v[1] += active ? w2 : 0.0f;
                    v[2] += active ? 1.0f : 0.0f;
                });
                row_reduce<3>(v, SumOp(), lds);
                A = v[0];
                S = v[1];
                cnt = v[2];
            });
        }
        float ss[1] = {0.0f};
        map_rows<VEC>({tr, wr}, d + row * T, T, [&](float ti, float wraw) {
            const float wi = sg * (sc * wraw);
            const float r = l2_ratio(ti, wi);
            float di = (alpha > r) ? -(r * wi) : -(alpha * wi);   // fab.py:666-667
            if (!(fabsf(wi) > 1e-8f)) di = 0.0f;
            ss[0] += di * di;
            return di;
        });
        row_reduce<1>(ss, SumOp(), lds);
        if (threadIdx.x == 0 && dnorm) dnorm[row] = sqrtf(ss[0]);
    }
}

__device__ __forceinline__ float l1_ratio(float wi) {  // fab.py:681  r = (1 / w).abs().clamp_max(1e12)
    return fminf(fabsf(1.0f / wi), kBig);
}
__device__ __forceinline__ float l1_gain(float ti, float wi) { return fminf(-wi * ti, wi * (1.0f - ti)); }
__device__ __forceinline__ float l1_face(float ti, float wi) {
    return (wi != 0.0f) ? ((wi < 0.0f ? 1.0f : 0.0f) - ti) : 0.0f;
}

// Greedy L1: coordinates in order of increasing key r = |1/w| (= decreasing |w|, index order within equal keys) move to
// their face while the residual stays positive.  Keys are non-negative floats, so their bit patterns order like
// integers: the last key whose residual-before is positive is found by row_workgroup.h's digit_search over the 31 key
// bits (the bins hold the gains between consecutive candidates), then the tie group is walked in index order with a
// workgroup prefix scan.  The output row doubles as scratch for the keys (one division per coordinate in total), so d
// must not alias t or w.
template <bool VEC>
__global__ __launch_bounds__(kRow) void fab_projection_l1_kernel(const float *__restrict__ t, const float *__restrict__ w,
                                                                 const float *__restrict__ wscale,
                                                                 const float *__restrict__ b, float *d,
                                                                 float *__restrict__ dnorm, int64_t R, int64_t w_rows,
                                                                 int64_t T) {
    __shared__ float lds[kCand * kRowWaves];
    __shared__ float wave_tot[kRowWaves];
    for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
        const float *tr = t + row * T, *wr = w + (row % w_rows) * T;
        float *dr = d + row * T;
        const float sc = wscale ? wscale[row % w_rows] : 1.0f;
        // pass 1: w.t, total gain for either orientation; keys into the output row
        float acc[3] = {0.0f, 0.0f, 0.0f};
        map_rows<VEC>({tr, wr}, dr, T, [&](float ti, float wraw) {
            const float wi = sc * wraw;
            acc[0] += wi * ti;
            acc[1] += l1_gain(ti, wi);
            acc[2] += l1_gain(ti, -wi);
            return l1_ratio(wi);
        });
        row_reduce<3>(acc, SumOp(), lds);
        const float c0 = acc[0] - b[row];
        const float sg = c0 >= 0.0f ? 1.0f : -1.0f;
        const float c = fabsf(c0);
        const float total = c + (sg > 0.0f ? acc[1] : acc[2]);   // s[:, -1]
        float sum_abs[1] = {0.0f};
        if (!(total < 0.0f)) {
            // the farthest corner does not reach the hyperplane: every coordinate to its face (fab.py:686)
            map_rows<VEC>({tr, wr}, dr, T, [&](float ti, float wraw) {
                const float wi = sg * (sc * wraw);
                float di = l1_face(ti, wi);
                if (!(fabsf(wi) > 1e-8f)) di = 0.0f;
                sum_abs[0] += fabsf(di);
                return di;
            });
        } else {
            // largest key bits rho with  c + sum_{key < rho} gain > 0;  `before` is that residual
            uint32_t rho = 0;
            float before = c;
            if (c > 0.0f) {
                float h[kCand];
                rho = digit_search(
                    31, h, lds,
                    [&](uint32_t lo, int shift, float(&hh)[kCand]) {
                        visit_rows<VEC>({tr, wr, dr}, T, [&](float ti, float wraw, float ri) {
                            bucket_add(hh, __float_as_uint(ri), lo, shift, l1_gain(ti, sg * (sc * wraw)));
                        });
                    },
                    [&](float hj) {                                    // residual before candidate j = before + h[0..j)
                        const float at = before + hj;
                        if (!(at > 0.0f)) return false;
                        before = at;
                        return true;
                    });
            }
            // every key below rho moves to its face, every key above stays; the tie group at rho holds the coordinate
            // that crosses the hyperplane.  One coalesced pass writes everything but the tie group and counts it.
            float ties[1] = {0.0f};
            float tie_t = 0.0f, tie_w = 0.0f;
            int64_t tie_i = -1;
            map_rows<VEC>({tr, wr, dr}, dr, T, [&](int64_t i, float ti, float wraw, float ri) {
                const float wi = sg * (sc * wraw);
                const uint32_t key = __float_as_uint(ri);
                float di = 0.0f;
                if (key < rho) di = l1_face(ti, wi);
                if (key == rho) {
                    ties[0] += 1.0f;
                    tie_i = i;
                    tie_t = ti;
                    tie_w = wi;
                }
                if (!(fabsf(wi) > 1e-8f)) di = 0.0f;
                sum_abs[0] += fabsf(di);
                return di;
            });
            row_reduce<1>(ties, SumOp(), lds);
            if (ties[0] == 1.0f) {
                // the usual case: the tie group is one coordinate, the one that would overshoot (fab.py:711,715)
                if (tie_i >= 0) {
                    const float after = before + l1_gain(tie_t, tie_w);
                    float di = after > 0.0f ? l1_face(tie_t, tie_w) : (before > 0.0f ? -before / tie_w : 0.0f);
                    if (!(fabsf(tie_w) > 1e-8f)) di = 0.0f;
                    dr[tie_i] = di;
                    sum_abs[0] += fabsf(di);
                }
            } else if (ties[0] > 1.0f) {
                // equal keys: walk the group in index order (contiguous chunk per thread, exclusive workgroup prefix of
                // the group's gains); keys are recomputed, the output row no longer holds them
                __syncthreads();
                const int64_t chunk = (T + kRow - 1) / kRow;
                const int64_t lo = (int64_t)threadIdx.x * chunk, hi = lo + chunk < T ? lo + chunk : T;
                float local = 0.0f;
                for (int64_t i = lo; i < hi; ++i) {
                    const float wi = sg * (sc * wr[i]);
                    if (__float_as_uint(l1_ratio(wi)) == rho) local += l1_gain(tr[i], wi);
                }
                const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
                float incl = local;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float up = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += up;
                }
                if (lane == 63) wave_tot[wave] = incl;
                __syncthreads();
                float run = before;
                for (int wv = 0; wv < wave; ++wv) run += wave_tot[wv];
                run += incl - local;
                for (int64_t i = lo; i < hi; ++i) {
                    const float ti = tr[i], wi = sg * (sc * wr[i]);
                    if (__float_as_uint(l1_ratio(wi)) != rho) continue;
                    const float after = run + l1_gain(ti, wi);
                    float di = after > 0.0f ? l1_face(ti, wi) : (run > 0.0f ? -run / wi : 0.0f);
                    run = after;
                    if (!(fabsf(wi) > 1e-8f)) di = 0.0f;
                    dr[i] = di;
                    sum_abs[0] += fabsf(di);
                }
            }
        }
        row_reduce<1>(sum_abs, SumOp(), lds);
        if (threadIdx.x == 0 && dnorm) dnorm[row] = sum_abs[0];
        __syncthreads();
    }
}

// ---- combine -----------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kRow) void fab_combine_kernel(const float *__restrict__ x1, const float *__restrict__ x0,
                                                           const float *__restrict__ d1, const float *__restrict__ d2,
                                                           const float *__restrict__ n1, const float *__restrict__ n2,
                                                           float *out, int64_t B, int64_t T, float eta, float alpha_max) {
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float a1 = fmaxf(n1[row], 1e-8f), a2 = fmaxf(n2[row], 1e-8f);
        float alpha = a1 / (a1 + a2);
        alpha = (alpha != alpha) ? alpha : fminf(fmaxf(alpha, 0.0f), alpha_max);
        const float keep = 1.0f - alpha;
        map_rows<VEC>({x1 + row * T, x0 + row * T, d1 + row * T, d2 + row * T}, out + row * T, T,
                      [&](float p1, float p0, float m1, float m2) {
                          const float v = (p1 + eta * m1) * keep + (p0 + m2 * eta) * alpha;
                          return (v != v) ? v : fminf(fmaxf(v, 0.0f), 1.0f);
                      });
    }
}

// ---- backward step -------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kRow) void fab_backward_step_kernel(float *x1, const float *__restrict__ x0, float *adv,
                                                                 float *res2, const uint8_t *__restrict__ is_adv,
                                                                 int64_t B, int64_t T, float beta, int kind) {
    __shared__ float lds[kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        if (!is_adv[row]) continue;   // workgroup-uniform
        float *p1 = x1 + row * T;
        const float *p0 = x0 + row * T;
        float *pa = adv + row * T;
        float v[1] = {0.0f};
        if (kind == ADVSTEP_FAB_LINF) {
            visit_rows<VEC>({p1, p0}, T, [&](float a, float c) { v[0] = max_nan(v[0], fabsf(a - c)); });
            row_reduce<1>(v, MaxNanOp(), lds);
        } else if (kind == ADVSTEP_FAB_L2) {
            visit_rows<VEC>({p1, p0}, T, [&](float a, float c) { v[0] += (a - c) * (a - c); });
            row_reduce<1>(v, SumOp(), lds);
            v[0] = sqrtf(v[0]);
        } else {
            visit_rows<VEC>({p1, p0}, T, [&](float a, float c) { v[0] += fabsf(a - c); });
            row_reduce<1>(v, SumOp(), lds);
        }
        const float tn = v[0], best = res2[row];
        const bool better = tn < best, worse = tn >= best;   // both false for a NaN norm: the reference's masks zero adv
        if (!worse) {
            if (better) map_rows<VEC>({p1, p0}, pa, T, [&](float a, float) { return a; });
            else map_rows<VEC>({p1, pa}, pa, T, [&](float a, float o) { return a * 0.0f + o * 0.0f; });
        }
        map_rows<VEC>({p1, p0}, p1, T, [&](float a, float c) { return c + (a - c) * beta; });
        __syncthreads();
        if (threadIdx.x == 0) res2[row] = better ? tn : (worse ? best : tn * 0.0f + best * 0.0f);
    }
}

}  // namespace

extern "C" {

int advstep_fab_hyperplane_f32(const float *gz, const float *x, const float *z, const int64_t *labels, float *wscale,
                               float *b, float *gnorm, float *gdot, int64_t B, int64_t T, int norm_kind,
                               advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && norm_kind >= 0 && norm_kind <= 2);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(gz && x && ((z == nullptr) == (labels == nullptr)) && (!z || (wscale && b)));
    return launch_rows(ROW_KERNEL_PAIR(fab_hyperplane_kernel), rows_vec(T, {gz, x}), B, stream, gz, x, z,
                       labels, wscale, b, gnorm, gdot, B, T, norm_kind);
}

int advstep_fab_projection_f32(const float *t, const float *w, const float *wscale, const float *b, float *d,
                               float *dnorm, int64_t R, int64_t w_rows, int64_t T, int norm_kind,
                               advstep_stream_t stream) {
    ADVSTEP_REQUIRE(R >= 0 && T >= 0 && w_rows >= 0 && norm_kind >= 0 && norm_kind <= 2);
    if (R == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(t && w && b && d && d != t && d != w && w_rows >= 1 && T >= 1 && T < kMaxRowLength);
    static_assert(ADVSTEP_FAB_LINF == 0 && ADVSTEP_FAB_L2 == 1 && ADVSTEP_FAB_L1 == 2, "the table's row order");
    static constexpr decltype(&fab_projection_linf_kernel<true>) kernels[3][2] = {   // [norm_kind][vec]
        ROW_KERNEL_PAIR(fab_projection_linf_kernel), ROW_KERNEL_PAIR(fab_projection_l2_kernel),
        ROW_KERNEL_PAIR(fab_projection_l1_kernel)};
    return launch_rows(kernels[norm_kind], rows_vec(T, {t, w, d}), R, stream, t, w, wscale, b, d, dnorm, R, w_rows, T);
}

int advstep_fab_combine_f32(const float *x1, const float *x0, const float *d1, const float *d2, const float *n1,
                            const float *n2, float *out, int64_t B, int64_t T, float eta, float alpha_max,
                            advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x1 && x0 && d1 && d2 && n1 && n2 && out);
    return launch_rows(ROW_KERNEL_PAIR(fab_combine_kernel), rows_vec(T, {x1, x0, d1, d2, out}), B, stream, x1,
                       x0, d1, d2, n1, n2, out, B, T, eta, alpha_max);
}

int advstep_fab_backward_step_f32(float *x1, const float *x0, float *adv, float *res2, const uint8_t *is_adv, int64_t B,
                                  int64_t T, float beta, int norm_kind, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && norm_kind >= 0 && norm_kind <= 2);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x1 && x0 && adv && res2 && is_adv);
    return launch_rows(ROW_KERNEL_PAIR(fab_backward_step_kernel), rows_vec(T, {x1, x0, adv}), B, stream,
                       x1, x0, adv, res2, is_adv, B, T, beta, norm_kind);
}

}  // extern "C"
