/*
 * advstep_fmn_sparse.h — C ABI of the sparse forms of the minimal-norm attack of libadvstep.so (torchattacks.FMNSparse): Fast
 * Minimum-Norm (Pintor, Roli, Brendel, Biggio, NeurIPS 2021) for the L1 and the L0 threat model.  As in include/advstep_fmn.h
 * every row carries its own radius, which shrinks while the iterate is adversarial and grows while it is not, and radii,
 * norms and decisions are device data from the first launch to the last: a whole attack makes no host read.
 *
 * The reference has no such attack.  Conventions are those of include/advstep_fmn.h: raw device pointers, int64_t sizes,
 * stream-ordered launches, status codes, nothing thrown, no state in the library.  Arithmetic is float32, expression by
 * expression: no FMA contraction, IEEE division and square root, NaN-propagating clamps, minima and maxima.
 *
 * Geometry: ONE workgroup of 1024 threads per row (csrc/row_workgroup.h, as include/advstep_apgdl1.h and advstep_l0.h), with
 * 16-byte accesses when T % 4 == 0 and every waveform base is 16-byte aligned, and 4-byte accesses otherwise — in the SAME
 * quad order where T % 4 == 0, so a base off the 16-byte grid changes no bit of any result, and sample by sample where
 * T % 4 != 0.  The workgroup owns its row's norms, decision, copy, move and projection, so the step is ONE launch and needs NO
 * workspace.  No atomics; no workgroup waits on another; reruns are bit-identical.  The box is [0, 1], as both projections
 * define it.
 *
 * State: the (4, B) planes eps, best, found, dnorm of include/advstep_fmn.h, initialised by advstep_fmn_begin_f32 and used
 * ping-pong exactly as advstep_fmn_step_f32 uses them.  In L0 the planes eps, best and dnorm hold sample counts (exact
 * floats: T < 2^24).
 *
 * Summation order (tests derive their bounds from it).  A thread adds its samples one after the other, in the traversal's
 * order: for T % 4 == 0 quads q = thread, thread + 1024, ... with the lanes x, y, z, w in turn (4 ceil(T / 4096) samples at
 * most), otherwise samples i = thread, thread + 1024, ... (ceil(T / 1024) <= 4 ceil(T / 4096)); a wave adds in 6 xor-shuffle
 * levels; the 16 waves are added one after the other (15): 4 ceil(T / 4096) + 21 additions on the longest chain, over
 * non-negative terms.  A count and a maximum are exact in any order.
 */
#ifndef ADVSTEP_FMN_SPARSE_H_
#define ADVSTEP_FMN_SPARSE_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step of the recurrence: z (B) is the logit of model(adv), taken in the pass that gave grad = d z / d adv turned towards
 * the other class (as for advstep_fmn_step_f32).  norm: 2 = L1, 3 = L0 — FMN's numbering continued; advstep_fmn_step_f32 keeps
 * refusing these two, and this entry point refuses 0 and 1.
 *
 * Pass 1, per row, d = adv - orig, g = grad (move == 0: grad is not read, gsq = gmax = 0):
 *   dabs = sum |d_i|     dcnt = #{i : d_i != 0}  (a NaN d_i counts)     gsq = sum g_i^2     gmax = max |g_i|  (NaN propagates)
 *
 * Decision (workgroup-uniform; thread 0 writes state_out and row_norms), with e = state.eps:
 *   is_adv  = (int64)(z > 0) != label                           (+-0 and NaN are class 0, as in include/advstep_fmn.h)
 *   better  = is_adv && dn < best ;   best' = better ? dn : best ;   found' = found || is_adv
 *   L1:  dn = dabs,  gq = gmax (the dual norm), and FMN's three-way rule verbatim, its widened never-found rule included:
 *        eps' = is_adv ? min(e, best') * (1 - gamma)
 *             : found  ? e * (1 + gamma)
 *             :          (dn + (gq > 0 ? |z| / gq : +inf)) * (1 + gamma)
 *   L0:  dn = dcnt, and the paper's integer rule; e1 = (e == +inf) ? 1 : e  (begin's value is read as the starting radius 1):
 *        eps' = is_adv ? min(min(e1 - 1, floorf(e1 * (1 - gamma))), best')
 *             :          max(e1 + 1, floorf(e1 * (1 + gamma)))
 *        then clamped to [0, T].  There is no reach rule: L0 has no dual norm.
 *   state_out = (eps', best', found', dn);   best_adv[b, :] = adv[b, :] iff better
 * A row that did not improve has NO byte of best_adv written.  `state` is only read and `state_out` only written; the two
 * must not overlap (ADVSTEP_EINVAL).
 *
 * Move (move != 0), FMN's own expression, into the `out` row:
 *   u_i = adv_i + alpha * (g_i / (sqrtf(gsq) + eps_div))
 * `out` may be `adv` itself: a thread reads its own samples before it writes them, and the copy into best_adv is made by the
 * same threads before the move.
 *
 * Projection into the row's NEW radius, about orig, in place on the `out` row:
 *   L1:  the exact projection onto {v : ||v - orig||_1 <= eps', 0 <= v <= 1} of include/advstep_apgdl1.h (the same row body as
 *        advstep_l1_box_project_f32: the same bits for the same u and radius), phi(0) summed during the move;
 *   L0:  kk = min(eps', T);  kk < 1: the out row is the orig row, bit for bit;  otherwise the exact-kk projection of
 *        include/advstep_l0.h without a per-sample cap (the same row body as advstep_l0_box_project_f32 with eps_inf = +inf):
 *        the kk samples whose keeping saves most squared distance, ties to the LOWER index.
 * move == 0 is the LAST call: the decision and the copy only; it writes no `out`; grad and out may be NULL, alpha and eps_div
 * are ignored.
 *
 * Edge rows:
 *   - an all-zero gradient row does not move (g / (0 + eps_div) = 0 for eps_div > 0); in L1, never found, it gets
 *     eps' = +inf, and the projection is then the identity followed by the clamp to the box;
 *   - a row the clean input already gets wrong has best' = eps' = 0 at the first step and comes back as orig from every move,
 *     in both norms (L1: eps' = 0 lets no coordinate move; L0: kk < 1);
 *   - a NaN in one row's gradient or logit stays in that row's planes and samples: no reduction crosses rows.  A NaN eps' in
 *     L1 fails phi(0) > eps' and leaves lambda = 0; in L0 it fails kk < 1 and every comparison of the search, which then keeps
 *     every sample.  The kernel terminates (every search makes a fixed number of passes) and writes every in-row sample,
 *     which is the existing projections' contract;
 *   - in L0, eps' >= T keeps every sample (clamped to the box).
 *
 * row_norms (nullable, (4, B)): dabs, dcnt, gsq, gmax as the decision used them.
 *
 * Traffic per sample: 12 B first touches (adv, grad, orig) + 4 B (out); the move re-reads 12 B and the projections' passes
 * re-read 8 B each from L2 / Infinity Cache (L1: 11 passes when phi(0) > eps', L0: 11 + the tie cut's) + 12 B for the last;
 * + 8 B per copied sample.  move == 0: 8 B + 8 B per copied sample.
 *
 * ADVSTEP_EINVAL for a negative size, B > 65535, T >= 2^24 (counts and indices are carried as exact floats), a null pointer
 * with work to do, norm not in {2, 3}, gamma outside (0, 1) or NaN and, with move, alpha < 0, eps_div < 0 or NaN.  out may
 * be adv itself and otherwise overlaps none of adv, grad, orig; best_adv overlaps none of adv, grad, orig, out; the per-row
 * buffers overlap neither out, best_adv nor state_out.  B == 0 or T == 0 returns ADVSTEP_OK, launches nothing and writes nothing. */
int advstep_fmn_sparse_step_f32(const float *adv, const float *grad, const float *orig, const float *z, const int64_t *labels,
                                const float *state, float *state_out, float *best_adv, float *out, float *row_norms,
                                float alpha, float gamma, int norm, int move, float eps_div, int64_t B, int64_t T,
                                advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_FMN_SPARSE_H_ */
