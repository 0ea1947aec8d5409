/*
 * advstep_smoothadv.h — C ABI of the attack on the smoothed detector in libadvstep.so (torchattacks.SmoothAdvPGD; Salman et al.,
 * NeurIPS 2019, "Provably Robust Deep Learning via Adversarially Trained Smoothed Classifiers").  The certificate of
 * include/advstep_smooth.h is about g(x) = the majority class of f(x + N(0, sigma^2 I)); SmoothAdv runs PGD on the Monte-Carlo
 * estimate of g's soft score over m noise draws:
 *     J(x') = -log( (1 / m) sum_i sigmoid(s * f(x' + sigma z_i)) ),   s = 2 y - 1.
 *
 * The reference has no such procedure.  The m draws are SLOTS, slot-major (m, B, T) as in include/advstep_smooth.h, and a step is
 *   advstep_smoothadv_fill_f32        the m noised copies of the current iterate, in the detector's input domain
 *   the detector                      z (m, B): one logit per slot and row; its input gradient per slot, (m, B, T)
 *   advstep_smoothadv_loss_grad_f32   J per row and dJ / dz
 *   advstep_smoothadv_step_f32        the sum over the slot gradients and PGD's step, L-inf or L2
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes, nothing
 * thrown, no state in the library; float32 expression by expression, no FMA contraction (fl(.) below is one float32 rounding);
 * 16-byte accesses when T % 4 == 0 and every base is 16-byte aligned, sample by sample otherwise, with the same bits either way.
 * No atomics; reruns are bit-identical on any stream; safe under stream capture.  A NaN stays in its row.
 * Every entry point: ADVSTEP_EINVAL for a negative size, B > 65535, a null pointer with non-zero sizes, or a bad scalar or forbidden
 * overlap as listed below; an empty size returns ADVSTEP_OK, launches nothing and writes nothing.
 */
#ifndef ADVSTEP_SMOOTHADV_H_
#define ADVSTEP_SMOOTHADV_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADVSTEP_SMOOTHADV_LINF 0
#define ADVSTEP_SMOOTHADV_L2 1

/* out[s - s0, b, t] = fl( v + fl(sigma * z) ) with v = fl( shift[b] + fl(scale[b] * adv[b, t]) ), s = s0 .. s0 + ns - 1, and z
 * the normal of include/advstep_smooth.h at counter offset + s: mapping, seed and the carry into the high counter word are
 * exactly advstep_smooth_noise_f32's (the two kernels instantiate one body).  `scale` and `shift` hold B floats each, or are both
 * null: then v = adv[b, t] and the bytes are advstep_smooth_noise_f32's.
 * The attack iterates in the min-max domain of an utterance while the smoothed detector and sigma live in the waveform's units:
 * with scale = mx - mn and shift = mn, v is minmax_revert's expression fl(fl(adv * range) + mn), so copy s is what
 * torchattacks.Smoothing.votes would feed the model for the reverted iterate, and no reverted tensor is ever stored.
 * No clamp; a NaN in adv, scale or shift propagates within its row.
 * Traffic: 4 B read and 4 * ns B written per sample; the slot loop runs over registers.
 * ADVSTEP_EINVAL also for exactly one of scale / shift null, out overlapping adv, scale or shift, or a sigma that is negative or
 * not finite; B == 0, T == 0 or ns == 0 is empty. */
int advstep_smoothadv_fill_f32(const float *adv, const float *scale, const float *shift, float *out, int64_t B, int64_t T, int64_t s0,
                               int64_t ns, float sigma, uint64_t seed, uint64_t offset, advstep_stream_t stream);

/* The soft vote of the m slots and its gradient.  z and dz are (m, B) slot-major, labels (B) int64 in {0, 1}, cost (B).
 * With s = 2 y - 1 and p_i = sigmoid(s z_i):
 *     cost[b]  = -log( (1 / m) sum_i p_i )
 *     dz[i, b] = scale * (-s) * w_i * sigmoid(-s z_i),   w_i = p_i / sum_j p_j
 * evaluated through log sigmoid and a max shift, per row, in this order (sp(t) = fl(max(t, 0) + log1pf(expf(-|t|))), the library's
 * softplus; expf, log1pf and logf are the accurate ones of the device library, not the hardware approximations):
 *     t_i = fl(s * z_i)                                  (exact: s = +-1)
 *     l_i = -sp(-t_i)                                    log p_i
 *     M   = max_i l_i                                    (a NaN wins: the row is NaN then)
 *     e_i = expf(fl(l_i - M)),  S = ((e_0 + e_1) + e_2) + ...   in slot order
 *     cost = fl( fl(logf((float)m) - M) - logf(S) )
 *     dz_i = fl( fl( fl(scale * (-s)) * fl(e_i / S) ) * expf(-sp(t_i)) )
 * so |z| = 80 stays finite (l = -80, never log(0)), and a row whose every slot is saturated on the wrong side has e_i = 1 and
 * w_i = 1 / m exactly.  scale = +-1 is the targeted switch of advstep_ce2_loss_grad_f32; the cost is not scaled.
 * The cost is the ROW's, not a batch mean: there is no 1 / B in dz.  Every step that consumes the gradient normalises it per row
 * (L2) or takes its signs (L-inf), so a positive factor per row is immaterial; the same holds for the Jacobian scale[b] * I of
 * the fill, which the caller does not apply.
 * One thread per row (m * B logits is a few kilobytes).
 * ADVSTEP_EINVAL also for dz or cost overlapping z or labels, or dz overlapping cost; B == 0 or m == 0 is empty. */
int advstep_smoothadv_loss_grad_f32(const float *z, const int64_t *labels, float *dz, float *cost, int64_t B, int64_t m, float scale,
                                    advstep_stream_t stream);

/* gsum[b, t] = ((g_0 + g_1) + g_2) + ... over grads (m, B, T) in slot order, one float32 rounding per add, and PGD's step
 * along it.  gsum is written out: a momentum or APGD variant would start from it.
 *   norm = ADVSTEP_SMOOTHADV_LINF: one launch; out = advstep_pgd_linf_step_f32(adv, gsum, orig, alpha, eps, lo, hi) evaluated as
 *       the sum is formed: (m + 2) * 4 B read and 8 B written per sample.  eps_div, ws and ws_bytes are not used (ws may be null).
 *   norm = ADVSTEP_SMOOTHADV_L2: launch 1 forms the sum, writes gsum and puts the row's sum-of-squares partials into the row
 *       workspace in the order of the three-launch advstep_pgd_l2_step_f32 (a thread's quads as (x^2 + y^2) + (z^2 + w^2) one after
 *       the other, the wave butterfly, then the 4 waves); launches 2 and 3 are that entry point's delta and projection passes on
 *       gsum, the same bodies.  One pass over gsum less than sum + advstep_pgd_l2_step_f32.  `ws`: advstep_row_workspace_bytes(B, T),
 *       16-byte aligned (include/advstep.h; ADVSTEP_EWORKSPACE as there).
 * BIT-IDENTITY: `out` equals advstep_pgd_linf_step_f32 / advstep_pgd_l2_step_f32 applied to (adv, gsum, orig) with the same
 * scalars, bit for bit, with gsum the slot-order float32 sum.
 * `out` may be `adv` itself (a thread reads its samples before it writes them).
 * ADVSTEP_EINVAL also for a norm other than the two above, gsum or out overlapping grads or orig, gsum overlapping adv or out,
 * or out overlapping adv without being adv; B == 0, T == 0 or m == 0 is empty.  The scalars are not checked, as in the two PGD
 * entry points. */
int advstep_smoothadv_step_f32(const float *adv, const float *orig, const float *grads, float *gsum, float *out, int64_t B, int64_t T,
                               int64_t m, int norm, float alpha, float eps, float eps_div, float lo, float hi, void *ws, size_t ws_bytes,
                               advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_SMOOTHADV_H_ */
