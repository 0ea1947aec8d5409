/*
 * advstep_l0.h — C ABI of the L0 (sparse) kernels of libadvstep.so: the exact-k projection and the PGD0 step.
 *
 * Algorithm: PGD0 of Croce & Hein, "Sparse and Imperceivable Adversarial Attacks", ICCV 2019 [https://arxiv.org/abs/1909.05040],
 * adapted to (B, T) waveforms: a row of (B, T) stands for an image, a sample for a pixel.  The reference tree has no
 * counterpart (its sparsefool.py / onepixel.py are other algorithms); the definitions below are the specification.
 *
 * Threat model: the attacker changes at most k samples of an utterance, each as far as the box [0, 1] allows, or, with a
 * finite eps_inf, by at most eps_inf ("sparse and bounded").  k >= T means "all"; eps_inf = +inf means no cap.
 *
 * The projection.  P0(u; x, k, eps_inf) projects u onto
 *     {z : #{i : z_i != x_i} <= k,  max(0, x - eps_inf) <= z <= min(1, x + eps_inf)},   x in [0, 1]:
 *     d_i  = u_i - x_i
 *     lb_i = max(-x_i, -eps_inf) ;  ub_i = min(1 - x_i, eps_inf)
 *     c_i  = min(max(d_i, lb_i), ub_i)
 *     r_i  = d_i - c_i
 *     s_i  = d_i * d_i - r_i * r_i            (what keeping coordinate i saves in squared distance)
 *     keep = the first min(k, T) indices of a STABLE descending sort of s      (ties: the lower index first)
 *     P0_i = keep_i ? clamp(x_i + c_i, 0, 1) : x_i
 * s_i >= 0 in float32 (|r_i| <= |d_i| and rounding is monotone), so scores order like their bit patterns, and with
 *     thr = the min(k, T)-th largest score ;  gt = #{s > thr} ;  cut = the index of the (min(k, T) - gt)-th i with s_i == thr
 * the kept set is {s > thr} u {i <= cut : s_i == thr}: exactly min(k, T) indices, the stable sort's.  A projection that
 * kept every tie (s >= thr) would not stay inside the L0 ball, and sign-like steps on audio do tie: a row u = x +- 0.25 has
 * hundreds of scores equal to the k-th.  The paper's 1e-12 * U(-0.5, 0.5) jitter is dropped: the index rule replaces it and
 * is reproducible.  A kept sample whose d_i * d_i underflows to 0 scores like an unmoved one.
 *
 * Layout (csrc/row_workgroup.h, as include/advstep_apgdl1.h): one workgroup of 1024 threads per row, striding past 65 535
 * rows; the row is re-read from L2 by every pass; float4 loads where T % 4 == 0 and the bases are 16-byte aligned.  Nothing is
 * sorted and there are no atomics.  thr: a radix search over the 31 bits of a score's pattern, 3 bits per streaming pass,
 * counting the scores AT OR ABOVE each of the 7 candidates: always 11 passes, the last of which also yields #{s == thr}.
 * cut: only where #{s >= thr} > min(k, T) (a workgroup-uniform condition), a second radix search over the bits of the sample
 * index, ceil(log2 T) / 3 passes (6 at T = 64 600).  Scores are recomputed from (x_i, u_i) in every pass and never stored:
 * 8 B per sample and pass.  Counts are exact floats (T < 2^24), every loop condition is workgroup-uniform, reductions are
 * fixed-order trees: reruns are bit-identical.  float32, IEEE division, no FMA contraction.
 * Non-finite x / u / grad: unspecified values, but every kernel terminates and writes every in-row sample.
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes,
 * arguments validated before any launch (NULL pointers, k < 1, !(eps_inf > 0), !(step >= 0), T >= 2^24: EINVAL), B = 0
 * returns OK and launches nothing.  1 <= T < 2^24.
 */
#ifndef ADVSTEP_L0_H_
#define ADVSTEP_L0_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = P0(u; x, k, eps_inf) per row.  x, u, out (B, T).  11 selection passes, the cut's where scores tie at the threshold,
 * one writing pass, 8 B per sample and pass.  out may alias u, not x. */
int advstep_l0_box_project_f32(const float *x, const float *u, float *out, int64_t k, float eps_inf, int64_t B, int64_t T,
                               advstep_stream_t stream);

/* One PGD0 iteration (the L1-normalised gradient step, then the projection), one launch:
 *   gnorm_b = sum_i |g_i|                            (the kernel's own fixed-order float32 sum)
 *   u_i     = cur_i + (step * g_i) / (gnorm_b + 1e-10f)
 *   out     = P0(u; x, k, eps_inf)
 * cur, grad, x, out (B, T).  stats (B, 4), optional (NULL = not written): gnorm_b, thr_b, gt_b = #{s > thr_b}, cut_b = the
 * index of the last kept sample with s_i == thr_b (-1 when none); counts and indices as exact floats.
 * A zero-gradient row gives u = cur, hence P0(cur): cur itself, bit for bit, when cur has at most k samples off x, lies in
 * the box and x_i + (cur_i - x_i) == cur_i in float32 (true within a factor of two of x_i, and at x_i = 0).
 * Passes: 1 over grad (gnorm), 1 over cur and grad that writes u into out, then the projection's over x and out.
 * out may alias cur (a thread reads its own samples before it writes them), not grad or x. */
int advstep_pgdl0_step_f32(const float *cur, const float *grad, const float *x, float *out, float *stats, float step,
                           int64_t k, float eps_inf, int64_t B, int64_t T, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_L0_H_ */
