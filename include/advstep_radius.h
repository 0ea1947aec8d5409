/*
 * advstep_radius.h — C ABI of the minimal-radius search of libadvstep.so (torchattacks.MinRadiusPGD): the PGD steps with a
 * radius PER ROW, and the bookkeeping of a per-utterance bisection on the radius that never leaves the device.
 *
 * The reference has no such attack; the step expressions are those of include/advstep.h's PGD entry points
 * (adversarial_attacks/torchattacks/attacks/pgd.py:74-76, pgdl2.py:78-88) with the launch scalars `alpha` and `eps` replaced by
 * the row's
 *   e = eps_rows[b]        a = alpha_abs + alpha_rel * e          (two float32 roundings, no FMA contraction)
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, the caller's row workspace `ws`
 * (advstep_row_workspace_bytes(B, T), zero-filled once; only its two float partial-sum planes are used here, never the
 * single-pass PGD-L2 exchange area), stream-ordered launches, status codes, nothing thrown, no state in the library.
 * Arithmetic is float32, expression by expression: no FMA contraction, IEEE division, NaN-propagating clamps,
 * sign(0) = sign(NaN) = 0.  All kernels run on the (tile, row) grid of 4096-sample tiles, with 16-byte accesses when T % 4 == 0
 * and every waveform base is 16-byte aligned and sample by sample otherwise.  No atomics; no workgroup waits on another (a row's
 * norms go through launch boundaries); reruns are bit-identical.
 *
 * Every entry point: ADVSTEP_EINVAL for a negative size, B > 65535 or a null pointer with B > 0 and T > 0; B == 0 or T == 0
 * (B == 0 for advstep_radius_begin_f32) returns ADVSTEP_OK, launches nothing and writes nothing.
 */
#ifndef ADVSTEP_RADIUS_H_
#define ADVSTEP_RADIUS_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The L-inf step of advstep_pgd_linf_step_f32 with per-row scalars, one launch, 16 B per sample:
 *   out = clamp(orig + clamp((adv + a * sign(grad)) - orig, -e, e), lo, hi)
 * A row with e = 0 and alpha_abs = 0 returns clamp(orig, lo, hi).  out may be adv itself (elementwise) and otherwise overlaps
 * none of adv, grad, orig; eps_rows overlaps out nowhere (ADVSTEP_EINVAL). */
int advstep_row_pgd_linf_step_f32(const float *adv, const float *grad, const float *orig, const float *eps_rows,
                                  float alpha_abs, float alpha_rel, float lo, float hi, float *out, int64_t B, int64_t T,
                                  advstep_stream_t stream);

/* The L2 step of advstep_pgd_l2_step_f32 in its three-launch form (partial sums of g^2, the delta pass, the projection) with
 * per-row scalars: the same expressions, the same partial sums and the same fixed-order re-reduction, so with every radius
 * equal and alpha_rel = 0 the result is bit-identical to that entry point (ADVSTEP_L2_SINGLE_PASS=0 or not: its two forms
 * agree bit for bit):
 *   gn  = sqrt(sum_t g^2) + eps_div
 *   d   = (adv + a * (g / gn)) - orig
 *   dn  = sqrt(sum_t d^2)
 *   f   = dn == 0 ? 1 : min((1 / dn) * e, 1)
 *   out = clamp(orig + d * f, lo, hi)
 * The guard on dn == 0 is the one addition: the fixed-radius expression gives min(inf * eps, 1) = 1 there for every eps > 0,
 * and this entry point keeps that value for e = 0 too (inf * 0 would be NaN) — a radius-0 row under a relative step has
 * d = 0 and must come back as clamp(orig, lo, hi), not as NaN.
 * gnorm / dnorm (nullable) receive sqrt(sum g^2) (before eps_div) and dn per row.  32 B per sample.
 * out may be adv itself and otherwise overlaps none of adv, grad, orig; eps_rows, gnorm, dnorm overlap out nowhere.
 * ADVSTEP_EWORKSPACE as in include/advstep.h. */
int advstep_row_pgd_l2_step_f32(const float *adv, const float *grad, const float *orig, const float *eps_rows,
                                float alpha_abs, float alpha_rel, float eps_div, float lo, float hi, float *out,
                                float *gnorm, float *dnorm, int64_t B, int64_t T, void *ws, size_t ws_bytes,
                                advstep_stream_t stream);

/* Search state: (4, B) float32, planes lo, hi, eps, best in this order (plane p of row b at state[p * B + b]).
 *   lo    the largest radius tried at which the row was NOT flipped (0 at the start)
 *   hi    the smallest radius at which it was (eps_max at the start)
 *   eps   the radius of the next attempt
 *   best  the smallest radius with a witnessed adversarial example: 0 for a row the clean input already gets wrong,
 *         +inf while none was found
 *
 * begin:  wrong = (int64)(z0[b] > 0) != labels[b]       (the first maximal index of cat([-z, z], 1): +-0 and NaN give class 0)
 *         lo = 0,  hi = wrong ? 0 : eps_max,  eps = hi,  best = wrong ? 0 : +inf
 * One launch of ceil(B / 256) workgroups.  eps_max must be >= 0 and not NaN (ADVSTEP_EINVAL). */
int advstep_radius_begin_f32(const float *z0, const int64_t *labels, float eps_max, float *state, int64_t B,
                             advstep_stream_t stream);

/* One search round after the attempt `adv` (B, T) at the radii state[2] was judged: z (B) is the logit of model(adv).
 *   flipped = (int64)(z[b] > 0) != labels[b]
 *   if flipped and eps < best:   best = eps,  hi = eps,  best_adv[b, :] = adv[b, :]
 *   elif not flipped:            lo = eps,    best_adv[b, :] = adv[b, :] iff first != 0
 *   (flipped and eps >= best — the radius-0 rows: nothing)
 *   eps' = 0.5f * (lo + hi)
 * so a row the clean input gets wrong keeps the best_adv the caller initialised (the clean input) and best = 0, and a row
 * that never flips keeps its first attempt at eps_max with best = +inf.
 *
 * One launch on the (tile, row) grid: every workgroup of a row takes the row's decision from z, labels and the planes of
 * `state`, which the launch ONLY READS; it copies its tile when the decision says so (8 B per sample moved, rows that are not
 * copied cost nothing); the first thread of tile 0 writes the row's new planes into `state_out`.  PING-PONG: the new state goes
 * to a second (4, B) buffer, which must not overlap `state` (ADVSTEP_EINVAL), so no workgroup of a row can read a plane that
 * tile 0 has already overwritten, whatever the order in which the row's workgroups run.  best_adv overlaps neither adv nor
 * the two states. */
int advstep_radius_round_f32(const float *adv, const float *z, const int64_t *labels, int first, const float *state,
                             float *state_out, float *best_adv, int64_t B, int64_t T, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_RADIUS_H_ */
