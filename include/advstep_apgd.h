/*
 * advstep_apgd.h — C ABI of the APGD (Auto-PGD, Croce & Hein 2020) update kernels of libadvstep.so.
 *
 * Reference: adversarial_attacks/torchattacks/attacks/apgd.py (attack_single_run / perturb), adapted to (B, T) waveforms:
 * a row of (B, T) stands for an image, "sum over dims (1, 2, 3)" is the sum over T and the (B, 1, 1, 1) per-row tensors are
 * (B).  The detectors emit one logit z; the attack scores cat([-z, z], 1) (the two-logit adapter of pgd.py:62).
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, the caller's row workspace `ws`
 * (advstep_row_workspace_bytes(B, T), zero-filled once; only its two float partial-sum planes are used here, never the
 * single-pass PGD-L2 exchange area), stream-ordered launches, status codes, nothing thrown.  Arithmetic follows the
 * reference expression by expression in float32: no FMA contraction, IEEE division and sqrt, NaN-propagating
 * min / max / clamp, sign(0) = sign(NaN) = 0, Python scalars as float32.  Row sums of squares are re-associated (a fixed
 * order per (B, T): reruns are bit-identical); everything else rounds as the reference does.
 *
 * Per-row state (B): acc (uint8, 1 = still classified correctly), flags (uint8: bit 0 = fooled at the last evaluation,
 * bit 1 = improved the best loss, bit 2 = reset to the best point at a checkpoint), loss_best, loss_best_last_check,
 * reduced_last_check (uint8), step_size.  loss_steps is (steps, B).  `norm`: 0 = L-inf, 1 = L2.
 */
#ifndef ADVSTEP_APGD_H_
#define ADVSTEP_APGD_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* apgd.py:89-95 with the caller's full (B, T) draw d:
 *   L-inf: t = 2 d - 1 (d ~ U[0, 1)),  out = clamp(x + ((eps * 1) * t) / max_T |t|, lo, hi)
 *   L2:    t = d (d ~ N(0, 1)),        out = clamp(x + ((eps * 1) * t) / (sqrt(sum_T t^2) + 1e-12), lo, hi)
 * An all-zero L-inf row divides 0 by 0 (NaN), as the reference does.  out must not alias draw. */
int advstep_apgd_init_noise_f32(const float *x, const float *draw, float *out, int64_t B, int64_t T, int norm,
                                float eps, float lo, float hi, void *ws, size_t ws_bytes, advstep_stream_t stream);

/* The same start with the draw generated in-kernel and never stored (8 B per sample): L-inf takes d from the stream of
 * advstep_pgd_linf_init_philox_f32 (counter = (flat index / 4, offset)), L2 the normals of advstep_pgd_l2_init_philox_f32
 * (counter = (quad of the row, row, offset)). */
int advstep_apgd_init_philox_f32(const float *x, float *out, int64_t B, int64_t T, int norm, float eps, float lo,
                                 float hi, uint64_t seed, uint64_t offset, void *ws, size_t ws_bytes,
                                 advstep_stream_t stream);

/* One workgroup over the B logits of one model evaluation (apgd.py:113-124, 166-190).
 *   u_b = (1 - 2 y_b) * 2 z_b ;  loss_b = softplus(u_b) ;  dz_b = 2 * ((1 - 2 y_b) * sigmoid(u_b))   (gradient of the SUM)
 *   pred_b = (argmax([-z_b, z_b]) == y_b), argmax = 1 iff z_b > 0 (a tie and NaN give 0)
 * mode 0: dz and loss only (the extra passes of EOT).
 * mode 1 (start point): acc = pred, loss_best = loss_best_last_check = loss, reduced_last_check = 1, flags = 0.
 * mode 2 (iteration i): acc = min(acc, pred); fooled = !pred; improved = loss > loss_best (strict: NaN gives 0);
 *   loss_best = improved ? loss : loss_best; loss_steps[i, b] = loss; flags = fooled | improved << 1.
 * Pointers a mode does not use may be NULL.  labels are int64 in {0, 1}. */
int advstep_apgd_eval_f32(const float *z, const int64_t *labels, float *dz, float *loss, int mode, int64_t i,
                          uint8_t *acc, uint8_t *flags, float *loss_best, float *loss_best_last_check,
                          uint8_t *reduced_last_check, float *loss_steps, int64_t B, advstep_stream_t stream);

/* One workgroup over the rows: the step-size checkpoint of apgd.py:194-211 after iteration i with window k.
 *   osc_b = (sum_{c < k} [L[i - c, b] > L[i - c - 1, b]]) <= k * rho   (losses compared in float32, the threshold in
 *           double; a negative step index wraps to steps - 1 as numpy's does)
 *   fl_b  = osc_b | (!reduced_last_check_b & (loss_best_last_check_b >= loss_best_b))
 *   reduced_last_check = fl ; loss_best_last_check = loss_best ; step_size /= 2 where fl ; flags bit 2 = fl. */
int advstep_apgd_checkpoint_f32(const float *loss_steps, int64_t steps, int64_t i, int64_t k, double rho,
                                const float *loss_best, float *loss_best_last_check, uint8_t *reduced_last_check,
                                float *step_size, uint8_t *flags, int64_t B, advstep_stream_t stream);

/* Best-point tracking and checkpoint reset (apgd.py:178, 186-189, 207-208) on flagged rows only, in this order:
 *   fooled:   x_best_adv = x_adv ;  improved: x_best = x_adv, grad_best = grad ;
 *   reset:    x_adv = x_best, grad = grad_best  (x_adv and grad are written in place).
 * Rows without a flag are neither read nor written. */
int advstep_apgd_track_f32(float *x_adv, float *grad, float *x_best, float *grad_best, float *x_best_adv,
                           const uint8_t *flags, int64_t B, int64_t T, advstep_stream_t stream);

/* The L-inf momentum step of apgd.py:141-149 (a = 1 at the first iteration, 0.75 afterwards; 1 - a formed in double):
 *   x1  = clamp(min(max(cur + step_b * sign(g), x - eps), x + eps), 0, 1)
 *   out = clamp(min(max((cur + (x1 - cur) * a) + (cur - prev) * (1 - a), x - eps), x + eps), 0, 1)
 * 20 B per sample.  out may alias prev (ping-pong), not cur / grad / x. */
int advstep_apgd_linf_step_f32(const float *cur, const float *prev, const float *grad, const float *x,
                               const float *step_size, float *out, int64_t B, int64_t T, float eps, double a,
                               advstep_stream_t stream);

/* The L2 momentum step of apgd.py:151-157 as four row passes that recompute rather than store (52 B per sample):
 *   x1  = cur + (step_b * g) / (||g|| + 1e-12)
 *   x1  = clamp(x + (x1 - x) / (||x1 - x|| + 1e-12) * min(eps, ||x1 - x||), 0, 1)
 *   x2  = (cur + (x1 - cur) * a) + (cur - prev) * (1 - a)
 *   out = clamp(x + (x2 - x) / (||x2 - x|| + 1e-12) * min(eps, ||x2 - x|| + 1e-12), 0, 1)
 * norms (B, 3) receives ||g||, ||x1 - x||, ||x2 - x|| per row (also the hand-over between the passes).
 * out may alias prev (ping-pong), not cur / grad / x / norms. */
int advstep_apgd_l2_step_f32(const float *cur, const float *prev, const float *grad, const float *x,
                             const float *step_size, float *out, float *norms, int64_t B, int64_t T, float eps,
                             double a, void *ws, size_t ws_bytes, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_APGD_H_ */
