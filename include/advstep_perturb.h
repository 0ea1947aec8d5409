/*
 * advstep_perturb.h — C ABI of the per-utterance perturbation report of libadvstep.so: how far an attacked batch lies from
 * the batch it was made from, per row, as L-inf, mean L1, L2, signal energy, SNR and segmental SNR (the audio convention
 * for an attack budget; it stands where the reference's src/aa/qualitative/attacks_postanalysis.py put a distortion
 * figure beside its WAV pairs).
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes,
 * nothing thrown, no state in the library.  The pass reads x and adv once (8 B per sample) and writes only `stats` and the
 * caller's workspace.  No atomics, no workgroup waits on another, no host synchronisation: it may be captured into a graph,
 * and reruns are bit-identical.
 */
#ifndef ADVSTEP_PERTURB_H_
#define ADVSTEP_PERTURB_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace of advstep_perturb_stats_f32 for a (B, T) batch: five planes of B * ceil(T / 4096) floats back to
 * back (sum x^2, sum d^2, sum |d|, max |d|, sum of the clamped segment SNRs: one partial per row and 4096-sample tile), the
 * total rounded up to a multiple of 16 bytes.  0 for B <= 0 or T <= 0.  This is NOT the row workspace of include/advstep.h
 * (advstep_row_workspace_bytes), whose layout is fixed by ABI 3; the buffer needs no initialisation and carries nothing from
 * one call to the next, but two calls that may run concurrently (two streams) need a buffer each. */
size_t advstep_perturb_stats_workspace_bytes(int64_t B, int64_t T);

/* x, adv: (B, T) contiguous float32.  stats: (6, B) float32, plane p of row b at stats[p * B + b].  With d = adv - x rounded
 * once to float32 and sums accumulated in float32 (a fixed order per (B, T)):
 *   0 linf        max_t |d|, NaN-propagating
 *   1 l1_mean     (sum_t |d|) / (float)T
 *   2 l2          sqrtf(sum_t d^2)
 *   3 energy      sum_t x^2
 *   4 snr_db      10 log10(sum x^2 / sum d^2): +inf when sum d^2 == 0 < sum x^2, -inf when sum x^2 == 0 < sum d^2,
 *                 NaN when both are 0 or anything is NaN
 *   5 seg_snr_db  mean over the S = floor(T / 256) full segments [256 s, 256 s + 256) of
 *                 clamp(10 log10(e_x / e_d), -10, 35), e_x / e_d the segment's sum of x^2 / d^2; a segment with e_d == 0
 *                 counts 35 (also when e_x == 0), one with e_x == 0 < e_d counts -10, NaN propagates; samples past 256 S
 *                 belong to no segment; S == 0 gives NaN
 * A row of T == 0 samples gets (0, NaN, 0, 0, NaN, NaN) and x, adv and ws are not read.
 *
 * Two launches: one over the (tile, row) grid of the row kernels that writes the five partials of every tile into ws, one
 * workgroup per row that re-reduces them in a fixed order and writes the six values.  16-byte loads when T % 4 == 0 and x and
 * adv are 16-byte aligned, sample by sample otherwise; the values do not depend on which.
 *
 * ADVSTEP_EINVAL for a negative size, B > 65535, a null x, adv or ws with B * T > 0, a null stats with B > 0, or stats / ws
 * overlapping x or adv (or each other); ADVSTEP_EWORKSPACE when ws is shorter than
 * advstep_perturb_stats_workspace_bytes(B, T) or not 16-byte aligned.  B == 0 returns ADVSTEP_OK and launches nothing. */
int advstep_perturb_stats_f32(const float *x, const float *adv, float *stats, void *ws, size_t ws_bytes, int64_t B,
                              int64_t T, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_PERTURB_H_ */
