/*
 * advstep_fmn.h — C ABI of the minimal-norm attack of libadvstep.so (torchattacks.FMN): Fast Minimum-Norm (Pintor, Roli,
 * Brendel, Biggio, NeurIPS 2021) for the L-inf and the L2 threat model.  Every row carries its own radius eps, which shrinks
 * while the iterate is adversarial and grows while it is not; radii, norms and decisions are device data from the first launch
 * to the last, so a whole attack makes no host read.
 *
 * The reference has no such attack.  Conventions are those of include/advstep_radius.h: raw device pointers, int64_t sizes,
 * stream-ordered launches, status codes, nothing thrown, no state in the library.  Arithmetic is float32, expression by
 * expression: no FMA contraction, IEEE division and square root, NaN-propagating clamps and minima.  The row kernels run on
 * the (tile, row) grid of 4096-sample tiles, with 16-byte accesses when T % 4 == 0 and every waveform base is 16-byte aligned
 * and sample by sample otherwise.  No atomics; no workgroup waits on another: a row's reductions go through launch boundaries
 * (one partial per (row, tile) in the caller's workspace, re-reduced in a fixed order by every workgroup of the row); reruns are
 * bit-identical.
 *
 * Every entry point: ADVSTEP_EINVAL for a negative size, B > 65535, a null pointer with work to do or a bad scalar; B == 0 or
 * T == 0 (B == 0 for advstep_fmn_begin_f32) returns ADVSTEP_OK, launches nothing and writes nothing.
 *
 * Workspace: `ws` holds five float planes of one partial per (row, tile) — sum d^2, max |d|, sum g^2, sum |g| and the L2 move's
 * sum d'^2 — in advstep_fmn_workspace_bytes(B, T) bytes, 16-byte aligned (ADVSTEP_EWORKSPACE otherwise).  It is NOT the row
 * workspace of include/advstep.h, whose two float planes are too few, and needs no zero-fill: every partial is written by one
 * launch before the next reads it.  One stream at a time, as there.
 *
 * Summation order (tests derive their bounds from it; it is csrc/radius.hip's): a thread adds its 4 quads one after the
 * other, each as (x^2 + y^2) + (z^2 + w^2) resp. (|x| + |y|) + (|z| + |w|); a wave adds in 6 xor-shuffle levels; the 4 waves
 * in 3; the re-reduction adds ceil(C / 256) partials per thread, then 6 + 3 again: 24 + ceil(C / 256) additions on the longest
 * chain, C = ceil(T / 4096).  A maximum is exact in any order.
 */
#ifndef ADVSTEP_FMN_H_
#define ADVSTEP_FMN_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the five partial planes for a (B, T) batch: 5 * align16(4 * B * ceil(T / 4096)); 0 for B <= 0 or T <= 0. */
size_t advstep_fmn_workspace_bytes(int64_t B, int64_t T);

/* Attack state: (4, B) float32, planes eps, best, found, dnorm in this order (plane p of row b at state[p * B + b]).
 *   eps    the row's radius: the ball the next move is projected into
 *   best   the smallest norm of an adversarial iterate seen so far: 0 for a row the clean input already gets wrong, +inf
 *          while none was found
 *   found  1.0 once any iterate of the row was adversarial, else 0.0
 *   dnorm  the norm of the iterate the last step judged (a diagnostic: nothing reads it)
 *
 * begin:  eps = best = +inf, found = 0, dnorm = 0.  One launch of ceil(B / 256) workgroups. */
int advstep_fmn_begin_f32(float *state, int64_t B, advstep_stream_t stream);

/* Per (row, tile) partials of the iterate's four norms, d = adv - orig, g = grad:
 *   sum d^2,  max |d|,  sum g^2,  sum |g|
 * One launch, 12 B per sample; grad may be NULL (the forward-only last pass: the g planes receive 0, 8 B per sample). */
int advstep_fmn_norms_f32(const float *adv, const float *grad, const float *orig, int64_t B, int64_t T, void *ws,
                          size_t ws_bytes, advstep_stream_t stream);

/* One step of the recurrence after advstep_fmn_norms_f32 of the same adv, grad, orig: z (B) is the logit of model(adv),
 * taken in the pass that gave grad = d z / d adv (the RAW logit gradient: its sign does not enter the decision, only the move,
 * where the caller has already turned it towards the other class).  norm: 0 = L-inf, 1 = L2.
 *
 * Every workgroup of a row re-reduces the row's partials and takes the row's decision; with e = state.eps:
 *   dn      = sqrt(sum d^2) (L2)  |  max |d| (L-inf)            gq = sqrt(sum g^2) (L2)  |  sum |g| (L-inf: the dual norm)
 *   is_adv  = (int64)(z > 0) != label                           (+-0 and NaN are class 0, as in include/advstep_radius.h)
 *   better  = is_adv && dn < best ;   best' = better ? dn : best ;   found' = found || is_adv
 *   eps'    = is_adv ? min(e, best') * (1 - gamma)
 *           : found  ? e * (1 + gamma)
 *           :          (dn + (gq > 0 ? |z| / gq : +inf)) * (1 + gamma)
 *   state_out = (eps', best', found', dn);   best_adv[b, :] = adv[b, :] iff better
 * A row that did not improve has NO byte of best_adv written.  `state` is only read and `state_out` only written (PING-PONG,
 * as advstep_radius_round_f32: the two must not overlap, ADVSTEP_EINVAL), so no workgroup of a row can read a plane that tile 0
 * has already overwritten.
 *
 * DEPARTURE FROM THE PAPER: its never-found rule is eps' = dn + |z| / gq, the distance to the boundary of the local linear
 * model, without the factor (1 + gamma).  On a locally linear detector that rule puts the iterate exactly ON the boundary,
 * where the rounding of z decides, and the row can stall there unfound: on the linear detectors of tests/test_fmn_host.py
 * (K = 100, T = 257 / 4099, ten rows) the float32 restatement of this recurrence leaves 2 and 4 rows unfound in L2 (4 and 1 in
 * L-inf) with the paper's rule and none with this one.
 *
 * Then the move (move != 0), gn = sqrt(sum g^2) for BOTH norms:
 *   d'      = (adv + alpha * (g / (gn + eps_div))) - orig
 *   L-inf:  out = clamp(orig + clamp(d', -eps', eps'), lo, hi)                                       (this launch)
 *   L2:     dn' = sqrt(sum d'^2);  f = dn' == 0 ? 1 : min((1 / dn') * eps', 1);  out = clamp(orig + d' * f, lo, hi)
 * The L2 form needs ||d'||, so it takes two more row passes — the delta pass and the projection pass of the PGD-L2 step
 * (include/advstep_radius.h: the same bodies, the same bits), the first inside this entry point's decision launch.
 * move == 0 is the LAST call: it absorbs the final iterate's decision into best / best_adv and writes no `out`; grad and out
 * may then be NULL, alpha and eps_div are ignored.
 *
 * Edge rows:
 *   - an all-zero gradient row does not move (g / (0 + eps_div) = 0 for eps_div > 0) and, never found, gets eps' = +inf;
 *   - a NaN in one row's gradient or logit stays in that row's planes and samples: no reduction crosses rows.  (A NaN z
 *     is class 0; a NaN eps' makes clamp(d', -eps', eps') = d' in the L-inf form and the row NaN in the L2 form);
 *   - a row the clean input already gets wrong has best' = 0 and eps' = 0 after the first step and comes back as orig
 *     (clamped) from every move: it stays the clean row with radius 0.
 *
 * row_norms (nullable, (5, B)): the row's re-reduced sum d^2, max |d|, sum g^2, sum |g| as the decision used them, and, in the L2
 * move only, dn' (plane 4 is not written otherwise).
 *
 * Traffic per sample: L-inf 16 B (adv, grad, orig read, out written) + 4 B per copied sample; L2 12 B (decision and delta
 * launch) + 8 B per copied sample + 16 B (projection launch); move == 0: 8 B per copied sample, nothing else.
 *
 * gamma must lie in (0, 1), alpha and eps_div be >= 0 (ADVSTEP_EINVAL; a NaN fails).  out may be adv itself (elementwise) and
 * otherwise overlaps none of adv, grad, orig; best_adv overlaps none of adv, grad, orig, out; the per-row buffers overlap
 * neither out, best_adv nor state_out. */
int advstep_fmn_step_f32(const float *adv, const float *grad, const float *orig, const float *z, const int64_t *labels,
                         const float *state, float *state_out, float *best_adv, float *out, float *row_norms, float alpha,
                         float gamma, int norm, int move, float eps_div, float lo, float hi, int64_t B, int64_t T, void *ws,
                         size_t ws_bytes, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_FMN_H_ */
