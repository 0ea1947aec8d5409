/*
 * advstep_masking.h — C ABI of the psychoacoustic-masking kernels of libadvstep.so: the short-time power spectrum, the fused
 * hinge penalty with its exact gradient, and the PGD step that mixes the two gradients.
 *
 * Idea: a perturbation whose short-time power spectrum stays under the frequency-masking threshold of the clean utterance is
 * masked by the speech (Qin et al., "Imperceptible, Robust, and Targeted Adversarial Examples for Automatic Speech
 * Recognition", ICML 2019; Schoenherr et al., NDSS 2019).  The reference tree has no counterpart; the definitions below are
 * the specification.  The kernels take the threshold theta as data (torchattacks/masking.py builds one).
 *
 * Framing: the frontend's (include/advstep_frontend.h).  n_fft = 512, a 512-float window w passed by pointer, hop h, centre
 * framing with reflect padding, NF = 1 + T / h frames, and for a row d of T samples
 *     reflect(q) = -q for q < 0,  2 (T - 1) - q for q >= T,  q otherwise
 *     X[f, k]    = sum_{n < 512} w[n] d[reflect(f h + n - 256)] e^(-2 pi i k n / 512),   k = 0 .. 256
 *     P[f, k]    = |X[f, k]|^2
 * (nfft, hop, T) must satisfy advstep_stft_bands_supported: nfft == 512, 128 <= hop <= 512, T > 257; anything else is EINVAL.
 *
 * The hinge.  With d = adv - x (formed in registers, never stored), theta (B, NF, 257), row_scale s (B) and e = P - theta:
 *     loss_b  = s_b * sum_{f, k} max(e, 0)
 *     count_b = #{(f, k) : e > 0}
 *     worst_b = max(0, max_{f, k} P / theta)        (NaN propagates)
 *     grad_b  = d loss_b / d d: the adjoint of the framing above, reflections included, applied to 2 s_b [e > 0] X
 * A cell with e > 0 false (theta = +inf, NaN) contributes nothing: its spectrum gradient is an exact 0.
 *
 * Layout.  Two workgroups of 1024 threads (16 wave64) share a row; a wave transforms 4 consecutive frames at a time on 16 lanes
 * each with the register-resident transform of lfcc_stft.hip (256-point complex FFT as 16 x 16, one LDS transposition), decides
 * the hinge on the spectrum in registers, and runs the inverse, the window and the overlap-add of its 4 frames itself.  Groups
 * that share a sample (at most two: hop >= 128) combine with one float atomic each onto the zero-filled gradient: two operands,
 * commutative, so the bits do not depend on the order.  loss and count are per-lane sums over a lane's frames in ascending
 * order, a wave butterfly, then the 16 waves in order; the row's two workgroups then add their shares to the zero-filled stats
 * with one atomic each (again two operands; the maximum is order-free): reruns are bit-identical.  Rows never meet: a NaN row
 * cannot touch another row's results.  float32; no FMA contraction outside the complex products of the transform.
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes,
 * arguments validated before any launch, B = 0 returns OK and launches nothing.
 */
#ifndef ADVSTEP_MASKING_H_
#define ADVSTEP_MASKING_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* power (B, NF, 257) = P of a - b, or of a when b is NULL.  a, b (B, T); window 512 floats.  One launch. */
int advstep_stft_power_f32(const float *a, const float *b, const float *window, float *power, int64_t B, int64_t T, int64_t NF,
                           int64_t hop, int64_t nfft, advstep_stream_t stream);

/* The hinge of adv - x against theta: grad (B, T) written in full (zero fills of grad and stats, then one launch), stats (B, 3) =
 * (loss_b, count_b, worst_b), the count as an exact float.  grad and stats must not overlap any input. */
int advstep_masking_hinge_grad_f32(const float *adv, const float *x, const float *window, const float *theta,
                                   const float *row_scale, float *grad, float *stats, int64_t B, int64_t T, int64_t NF,
                                   int64_t hop, int64_t nfft, advstep_stream_t stream);

/* The mixed step (sign, clamp: include/advstep.h's advstep_pgd_linf_step_f32), per row, one launch:
 *     m1 = (sum_i |g_ce_i|) / T,  m2 = (sum_i |g_mask_i|) / T       (the kernel's own fixed-order float32 sums)
 *     u  = g_ce / m1 - lambda * (g_mask / m2)                        (a term whose mean is 0 is dropped)
 *     out = clamp(x + clamp(cur + step * sign(u) - x, -eps, eps), 0, 1)
 * lambda == 0: no sums, u = g_ce, and out is advstep_pgd_linf_step_f32's bit for bit (g_mask may then be NULL).
 * One workgroup of 1024 threads per row (csrc/row_workgroup.h), striding past 65 535 rows; float4 loads where T % 4 == 0 and
 * the bases are 16-byte aligned.  1 <= T < 2^24.  out may alias cur, not g_ce, g_mask or x. */
int advstep_psy_step_f32(const float *cur, const float *g_ce, const float *g_mask, const float *x, float lambda, float step,
                         float eps, float *out, int64_t B, int64_t T, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_MASKING_H_ */
