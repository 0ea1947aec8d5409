/*
 * advstep_momentum.h — C ABI of the momentum-attack kernels of libadvstep.so: the fused MI-FGSM / NI-FGSM update and the
 * variance-tuning helpers of VMI-FGSM / VNI-FGSM.
 *
 * Reference: adversarial_attacks/torchattacks/attacks/mifgsm.py:70-76, nifgsm.py:56,67-71, vmifgsm.py:77-101,
 * vnifgsm.py:65,78-102, adapted to (B, T) waveforms: a row of (B, T) stands for an image and "mean over dims (1, 2, 3)" is the
 * mean over T.
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, the caller's row workspace `ws`
 * (advstep_row_workspace_bytes(B, T), zero-filled once; only its two float partial-sum planes are used here, never the
 * single-pass PGD-L2 exchange area), stream-ordered launches, status codes, nothing thrown.  Arithmetic follows the
 * reference expression by expression in float32: no FMA contraction, IEEE division, NaN-propagating clamps,
 * sign(0) = sign(NaN) = 0, Python scalars as float32.  The row sum of |a| is re-associated (a fixed order per (B, T): reruns
 * are bit-identical); everything else rounds as the reference does.  No launch waits on another workgroup.
 */
#ifndef ADVSTEP_MOMENTUM_H_
#define ADVSTEP_MOMENTUM_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One whole momentum update (mifgsm.py:70-76; nifgsm.py:67-71; vmifgsm.py:77-79, 99-101):
 *   a    = grad                          (v == NULL)   |   grad + v
 *   mu_b = (sum_t |a[b, t]|) / (float)T
 *   n    = a / mu_b
 *   m'   = n + momentum * decay          momentum is updated IN PLACE
 *   x1   = adv + alpha * sign(m')
 *   d    = clamp(x1 - orig, -eps, eps)
 *   out  = clamp(orig + d, lo, hi)
 *   nes  = out + nes_scale * m'          only when nes_out != NULL (NI-FGSM's next look-ahead point,
 *                                        nes_scale = float32(decay * alpha))
 * gmean (nullable) receives mu_b per row.  A row whose a is all zero gives n = m' = NaN, a zero sign and out = the
 * projection of adv, as the reference does.
 * Two launches: per-(row, tile) partial sums of |a|, then the apply pass (28 B per sample: grad twice, momentum, adv, orig
 * in; momentum, out back; + 8 with v, + 4 with nes_out).
 * out may be adv itself (the update is elementwise once mu_b is known) and otherwise overlaps no operand; momentum and
 * nes_out overlap no other operand. */
int advstep_mi_step_f32(const float *adv, const float *grad, const float *v, const float *orig, float *momentum,
                        float *out, float *nes_out, int64_t B, int64_t T, float alpha, float eps, float decay,
                        float nes_scale, float lo, float hi, float *gmean, void *ws, size_t ws_bytes,
                        advstep_stream_t stream);

/* vmifgsm.py:84-85 with the caller's draw ~ U(-eps * beta, eps * beta): out = adv + draw (no clamp, as the reference).
 * out may be adv or draw (elementwise). */
int advstep_vt_neighbor_noise_f32(const float *adv, const float *draw, float *out, int64_t n, advstep_stream_t stream);

/* The same with the draw generated in-kernel and never stored (8 B per sample), from the uniform stream of
 * advstep_pgd_linf_init_philox_f32 (counter = (flat index / 4, offset)): draw = u * (bound - (-bound)) + (-bound),
 * bound = float32(eps * beta).  Neighbour j of iteration i uses offset = i * N + j. */
int advstep_vt_neighbor_philox_f32(const float *adv, float *out, int64_t n, float bound, uint64_t seed, uint64_t offset,
                                   advstep_stream_t stream);

/* vmifgsm.py:82, 94-95: gv = g when first != 0 (the zero-filled accumulator plus g), else gv += g. */
int advstep_vt_accumulate_f32(float *gv, const float *g, int64_t n, int first, advstep_stream_t stream);

/* vmifgsm.py:97: v = gv / (float)N - adv_grad.  v may be gv or adv_grad. */
int advstep_vt_variance_f32(const float *gv, const float *adv_grad, float *v, int64_t n, int64_t N,
                            advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_MOMENTUM_H_ */
