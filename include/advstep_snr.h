/*
 * advstep_snr.h — C ABI of the SNR-budget PGD of libadvstep.so (torchattacks.PGDSNR): PGD under a budget stated in dB of
 * signal-to-noise ratio, per utterance (global) or per 256-sample segment (segmental).
 *
 * The reference has no such attack.  The attack sees x01 = (x - mn) / (mx - mn); the waveform is (mx - mn) * (x01 + c) with
 * c = mn / (mx - mn) per row, and a perturbation scales by (mx - mn), so the waveform-domain SNR of a perturbation d01 is
 * sum (x01 + c)^2 / sum d01^2, scale-free.  With rho = 10^(-snr_db / 20) (formed by the caller in double, passed as one float32;
 * no log / pow runs on the device) the budgets are
 *   global:     ||d_b||_2 <= rho * sqrt(sum_t (x01 + c_b)^2)                     an L2 ball with a radius per row
 *   segmental:  the same inequality for every segment [256 s, 256 s + 256) of the row on its own: a product of L2 balls.  The
 *               last, partial segment is a segment like the others over its in-row samples; a silent segment has radius 0 and
 *               is not touched; there is no energy floor, so every segment's SNR is >= snr_db.
 *
 * Conventions are those of include/advstep_radius.h: raw device pointers, int64_t sizes, stream-ordered launches, status
 * codes, nothing thrown, no state in the library; float32 expression by expression, no FMA contraction, IEEE division and
 * square root, NaN-propagating clamps; the (tile, row) grid of 4096-sample tiles with 16-byte accesses when T % 4 == 0 and every
 * waveform base is 16-byte aligned, sample by sample otherwise.  No atomics, no workgroup waits on another, reruns are
 * bit-identical, safe under stream capture.
 *
 * Both entry points: ADVSTEP_EINVAL for a negative size, B > 65535, a NaN or negative rho, a null pointer with B > 0 and T > 0
 * (offset_rows excepted: null means c = 0 for every row) or a forbidden overlap; B == 0 or T == 0 returns ADVSTEP_OK, launches
 * nothing and writes nothing.
 */
#ifndef ADVSTEP_SNR_H_
#define ADVSTEP_SNR_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The segmental step: the steepest-ascent direction of the product-ball geometry (each segment's gradient normalised by its
 * own norm and scaled by its own radius, as sign() is for L-inf), then the projection onto each segment's ball.  Per segment s
 * of row b, c = offset_rows ? offset_rows[b] : 0, sums over the segment's in-row samples:
 *   e_x = sum (x_t + c)^2                       (x_t + c rounds once)
 *   r   = rho * sqrtf(e_x)
 *   gn  = sqrtf(sum g_t^2) + eps_div
 *   a   = alpha_rel * r
 *   d_t = (adv_t + a * (g_t / gn)) - x_t
 *   dn  = sqrtf(sum d_t^2)
 *   f   = dn == 0 ? 1 : min((1 / dn) * r, 1)
 *   out = clamp(x_t + d_t * f, lo, hi)
 * A sum is a thread's four samples as (p + q) + (r + s), then the wavefront's 6 xor-shuffle levels (offsets 32 .. 1): a segment
 * is one wavefront's float4 load, so there are three wave reductions per segment and nothing else — one launch, 16 B per
 * sample, no workspace, no LDS.  A NaN in a segment's gradient makes that segment NaN and no other.
 * out may be adv itself (a thread reads its own samples before it writes them) and otherwise overlaps none of adv, grad, orig;
 * offset_rows overlaps out nowhere. */
int advstep_seg_pgd_step_f32(const float *adv, const float *grad, const float *orig, const float *offset_rows, float rho,
                             float alpha_rel, float eps_div, float lo, float hi, float *out, int64_t B, int64_t T,
                             advstep_stream_t stream);

/* The radii of the global budget: eps_rows[b] = rho * sqrtf(sum_t (x + c_b)^2), for advstep_row_pgd_l2_step_f32 (with
 * alpha_abs = 0 the step is then the global SNR step).  Two launches: per-tile partial sums into plane 0 of the row workspace
 * `ws` (advstep_row_workspace_bytes(B, T), include/advstep.h; ADVSTEP_EWORKSPACE as there), then one workgroup per row adds the
 * row's partials in the fixed order of the L2 step's norms (a thread's 4 quads one after the other, 6 + 3 levels in the
 * workgroup, ceil(C / 256) + 6 + 3 in the re-reduction).  4 B per sample read, 4 B per row written.
 * eps_rows overlaps neither x nor offset_rows. */
int advstep_snr_row_radius_f32(const float *x, const float *offset_rows, float rho, float *eps_rows, int64_t B, int64_t T,
                               void *ws, size_t ws_bytes, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_SNR_H_ */
