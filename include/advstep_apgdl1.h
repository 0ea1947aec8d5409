/*
 * advstep_apgdl1.h — C ABI of the l1-APGD kernels of libadvstep.so: the L1 member of the APGD family.
 *
 * Algorithm: Croce & Hein, "Mind the box: l1-APGD for sparse adversarial attacks on image classifiers", ICML 2021
 * [https://arxiv.org/abs/2103.01208], adapted to (B, T) waveforms as include/advstep_apgd.h adapts APGD: a row of (B, T)
 * stands for an image and the per-row tensors are (B).  The reference tree has no L1 branch; the definitions below are the
 * specification.  advstep_apgd_eval_f32 and advstep_apgd_track_f32 serve this attack unchanged.
 *
 * Layout: one workgroup of 1024 threads per row, striding past 65 535 rows; the row is re-read from L2 by every pass;
 * float4 loads where T % 4 == 0 and the bases are 16-byte aligned.  Nothing is sorted: the k-th largest |gradient| and the
 * projection's multiplier are found by a radix search over float bit patterns (non-negative floats order like their
 * integer bit patterns), 3 bits = 7 candidates per streaming pass, 11 passes for the 31 bits.  Every search runs that
 * fixed number of passes and every loop condition is workgroup-uniform.  Reductions are fixed-order trees: reruns are
 * bit-identical.  float32, IEEE division, no FMA contraction.
 *
 * The projection.  P(u; x, eps) = argmin ||z - u||_2  over  {z : ||z - x||_1 <= eps, 0 <= z <= 1},  x in [0, 1], eps > 0:
 *     d = u - x ;  cap_i = (d_i > 0) ? 1 - x_i : x_i ;  m_i(lam) = min(max(|d_i| - lam, 0), cap_i)
 *     phi(lam) = sum_i m_i(lam)            (the kernel's own fixed-order float32 sum)
 *     lam* = the smallest non-negative float32 with phi(lam*) <= eps      (0 when phi(0) <= eps)
 *     P_i = clamp(x_i + sign(d_i) * m_i(lam*), 0, 1)
 * phi is continuous and non-increasing, and so is its float32 evaluation (a fixed-order sum of monotone terms), so the
 * search over lam's bits is exact and reproducible.  phi is NOT convex (a coordinate's slope goes 0 -> -1 -> 0 as lam
 * passes |d_i| - cap_i and |d_i|): a Newton / Michelot fixed point from lam = 0 can overshoot, a bracket search cannot.
 * Non-finite x / u: unspecified values, but every kernel terminates and writes every in-row sample.
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes,
 * arguments validated before any launch, B = 0 returns OK and launches nothing.  1 <= T < 2^24 (counts are exact floats).
 */
#ifndef ADVSTEP_APGDL1_H_
#define ADVSTEP_APGDL1_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = P(u; x, eps) per row.  x, u, out (B, T).  One pass for phi(0), 11 search passes unless phi(0) <= eps, one
 * writing pass, 8 B per sample and pass.  out may alias u, not x. */
int advstep_l1_box_project_f32(const float *x, const float *u, float *out, float eps, int64_t B, int64_t T,
                               advstep_stream_t stream);

/* One l1-APGD iteration (the sparse steepest-ascent step for the L1 ball, then the projection), one launch:
 *   n_b   = (int64) clamp((1 - topk_b) * T, 0, T - 1)            (float32 product, the cast truncates)
 *   thr_b = element n_b of row b's |grad| sorted ascending, NaN above +inf as torch.sort orders
 *   s_i   = (|g_i| >= thr_b) ? sign(g_i) : 0                     (false on NaN; sign(NaN) = sign(0) = 0)
 *   cnt_b = sum_i |s_i|                                          (an exact integer)
 *   u_i   = cur_i + (step_b * s_i) / (cnt_b + 1e-10f)
 *   out   = P(u; x, eps)
 * cur, grad, x, out (B, T); step_size, topk (B).  stats (B, 2), optional (NULL = not written): thr_b, cnt_b.
 * Passes: 11 + 1 over grad (selection, count), 1 over cur, grad, x that writes u into out, then the projection's over
 * x and out.  out may alias cur (a thread reads its own samples before it writes them), not grad or x. */
int advstep_apgdl1_step_f32(const float *cur, const float *grad, const float *x, const float *step_size,
                            const float *topk, float *out, float *stats, int64_t B, int64_t T, float eps,
                            advstep_stream_t stream);

/* The random start: out = P(x + t; x, eps), t ~ N(0, 1) from the caller's (B, T) draw.  out may alias draw, not x. */
int advstep_apgdl1_init_f32(const float *x, const float *draw, float *out, int64_t B, int64_t T, float eps,
                            advstep_stream_t stream);

/* The same start with t generated in-kernel and never stored: the normals of advstep_pgd_l2_init_philox_f32
 * (counter = (quad of the row, row, offset)). */
int advstep_apgdl1_init_philox_f32(const float *x, float *out, int64_t B, int64_t T, float eps, uint64_t seed,
                                   uint64_t offset, advstep_stream_t stream);

/* The sparsity checkpoint, per row, BEFORE advstep_apgd_track_f32 of the same iteration:
 *   xb    = (flags_b & 2) ? cur : x_best          (the best point including this iteration's improvement)
 *   sp    = (float) #{i : xb_i - x_i != 0}
 *   red   = (sp / sp_old_b) < 0.95f
 *   topk_b = (sp / (float)T) / 1.5f
 *   step_b = clamp(red ? eps : step_b / 1.5f, eps / 10.0f, eps) ;  sp_old_b = sp
 *   flags bit 2 = red (advstep_apgd_track_f32 then resets the row to its best point), other bits kept.
 * cur, x_best, x (B, T); flags (B) uint8; sp_old, topk, step_size (B) float32, updated in place.  8 B per sample. */
int advstep_apgdl1_checkpoint_f32(const float *cur, const float *x_best, const float *x, uint8_t *flags, float *sp_old,
                                  float *topk, float *step_size, int64_t B, int64_t T, float eps,
                                  advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_APGDL1_H_ */
