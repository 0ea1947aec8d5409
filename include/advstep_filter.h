/*
 * advstep_filter.h — C ABI of the universal adversarial FIR filter of libadvstep.so (torchattacks.UniversalFilter, after Malafide:
 * Panariello et al., Interspeech 2023): ONE short linear time-invariant filter for the whole batch, applied to the rows of the
 * source class; its evaluation, the gradient of a loss with respect to its taps, and the Adam step on the taps.
 *
 * The reference has no such attack, and every other attack of this library is additive.  THE ARITHMETIC IS PART OF THIS ABI.
 * Rows x (B, T) live in the attacks' min-max domain; c[b] = -mn_b / (mx_b - mn_b) is the value that means silence in row b (as in
 * include/advstep_channel.h), m[b] in {0, 1} selects the rows the filter acts on (a null row_mask: every row), and h[0 .. L-1] is
 * the filter, L odd, 1 <= L <= ADVSTEP_FILTER_MAX_TAPS, centred: P = (L - 1) / 2.
 *
 *   xc[b, u]  = x[b, u] - c[b]  for 0 <= u < T,  0 otherwise                          (silence outside the utterance)
 *   acc       = 0;  for i = 0 .. L-1 in this order:  acc = acc + h[i] * xc[b, t + P - i]
 *   out[b, t] = m[b] != 0 ? clamp(c[b] + acc, lo, hi) : x[b, t]                       (a row with m[b] == 0: x's bits)
 *
 * Every product and every sum of the forward is rounded to float32 on its own (no FMA contraction), so a float32 restatement in
 * this order gives the same BYTES; the values are those of advstep_channel_apply_f32 with K = 1, the same taps in every row,
 * shift = -P, gain 1 and noise 0, clamped (L <= 256, where both exist; the channel's a n = +-0 term can change the sign of a zero,
 * nothing else).  Filtering is linear and c maps to waveform 0, so before the clamp the reverted waveform is h * waveform: the same
 * physical filter for every utterance, whatever its minimum and maximum.
 *
 * The gradient with respect to the taps takes g = d loss / d out and out itself, for the clamp's mask:
 *
 *   gm[b, t] = (m[b] != 0 and lo < out[b, t] and out[b, t] < hi) ? g[b, t] : 0
 *   dh[i]    = sum_b sum_t gm[b, t] * xc[b, t + P - i]
 *
 * The inequalities are strict: a sample that sits exactly on lo or hi contributes nothing, whether the clamp moved it or not.
 * dh is held to a bound, not to bytes, and its terms are accumulated with EXPLICIT fused multiply-adds (fmaf: one rounding per
 * term).  The order of the additions is a function of (B, T, L) alone; with C = ceil(T / 4096) tiles per row,
 * TL = ceil(L / 16) tap lanes and NS = floor(256 / TL) sample segments of a tile:
 *   1. thread     a thread owns 16 consecutive taps and one segment of its tile.  A tile of n samples (4096, or what is left of the
 *                 row) is cut into n16 / 16 chunks of 16 samples, n16 = 16 ceil(n / 16) (samples n .. n16 - 1 enter with gm = 0), and
 *                 segment s holds the chunks  s CPS .. min((s + 1) CPS, n16 / 16) - 1,  CPS = ceil((n16 / 16) / NS).  The thread
 *                 starts from +0 and takes its samples in ascending order:  a = fmaf(gm[t], xc[t + P - i], a).
 *   2. workgroup  a tap's NS segment sums are folded through LDS in ascending order of the segment:  p = ((0 + a_0) + a_1) + ...
 *   3. tile       p is the partial of (tile c, row b): L floats at partials[(b C + c) L + i].  A row with m[b] == 0 writes zeros.
 *   4. row        advstep_filter_tap_update_f32 adds a row's tiles in order:  r_b = ((0 + p_{b,0}) + p_{b,1}) + ...
 *   5. row group  rows are cut into groups of ADVSTEP_FILTER_GROUP_ROWS consecutive rows, a group's rows are added in order,
 *                 P_g = ((0 + r_{16 g}) + r_{16 g + 1}) + ...,  and  dh[i] = ((0 + P_0) + P_1) + ...  over the groups in order.
 * There are no float atomics and no workgroup waits on another: reruns give the same bits on any stream and under capture.  A term
 * passes through at most 16 CPS + NS + C + min(B, 16) + ceil(B / 16) rounded additions.
 *
 * Inputs are specified for finite values; for anything else the kernels are only memory-safe (taps, center, row_mask and the
 * workspace are device data the host cannot validate: no value in them moves an address).
 *
 * Conventions are those of include/advstep_channel.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes,
 * nothing thrown, no state in the library, safe under stream capture.  The bytes do not depend on the alignment of any base or on
 * T % 4.
 *
 * All entry points: ADVSTEP_EINVAL for a negative size, B > 65535, an even L, L < 1, L > ADVSTEP_FILTER_MAX_TAPS, a null pointer
 * with non-zero sizes (row_mask and dh_out excepted) or a forbidden overlap; B == 0 or T == 0 returns ADVSTEP_OK, launches nothing
 * and writes nothing.
 */
#ifndef ADVSTEP_FILTER_H_
#define ADVSTEP_FILTER_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADVSTEP_FILTER_MAX_TAPS 1025  /* 64 ms at 16 kHz */
#define ADVSTEP_FILTER_GROUP_ROWS 16  /* rows per group of the fold over rows */

/* out[b, t] above.  x (B, T), center (B), row_mask (B) float32 or null, taps (L), out (B, T).  One launch on the (4096-sample tile,
 * row) grid, 8 B per sample and 2 L operations; the workgroup of a row with m[b] == 0 copies its tile and leaves.
 * out may be x itself where no workgroup reads what another writes: when a row is one tile (T <= 4096) or the filter is one tap
 * (L == 1); with longer rows a tile's halo lies in its neighbours' samples, and out == x is ADVSTEP_EINVAL.  Otherwise out
 * overlaps none of x, center, row_mask, taps. */
int advstep_filter_apply_f32(const float *x, const float *center, const float *row_mask, const float *taps, float *out, int64_t B,
                             int64_t T, int64_t L, float lo, float hi, advstep_stream_t stream);

/* Bytes of the partials of the tap gradient for a (B, T) batch and L taps: B * ceil(T / 4096) * L floats (2 MB at (128, 64 600,
 * 255)); 0 for an empty batch, a negative size or an L that the entry points refuse.  Every advstep_filter_tap_grad_f32 call
 * rewrites all of it: the buffer needs no initialisation and carries nothing from one call to the next. */
size_t advstep_filter_workspace_bytes(int64_t B, int64_t T, int64_t L);

/* partials[(b C + c) L + i] = p above, for every tile, row and tap (steps 1 to 3 of the order).  x, grad, out_adv (B, T), center
 * (B), row_mask (B) or null; partials_ws: advstep_filter_workspace_bytes(B, T, L) bytes, ADVSTEP_EWORKSPACE if null or smaller.
 * One launch on the (tile, row) grid, 12 B per sample against 2 L operations: bound by the vector ALUs.  The workspace overlaps
 * none of the inputs. */
int advstep_filter_tap_grad_f32(const float *x, const float *center, const float *row_mask, const float *grad, const float *out_adv,
                                void *partials_ws, size_t ws_bytes, int64_t B, int64_t T, int64_t L, float lo, float hi,
                                advstep_stream_t stream);

/* dh = the fold of the partials that advstep_filter_tap_grad_f32 left for the same (B, T, L) (steps 4 and 5), written to dh_out
 * (L floats) unless that is null, and one Adam step on the taps along it, with the arithmetic of advstep_cw_adam_step_f32:
 *   g = ascend ? -dh : dh                                   (ascend != 0: the taps climb the loss)
 *   m = m + (1 - beta1) * (g - m) ;  v = v * beta2 + ((1 - beta2) * g) * g
 *   h = h + (-(lr / (1 - beta1^step))) * (m / (sqrt(v) / sqrt(1 - beta2^step) + adam_eps))
 * The bias corrections are formed in double on the host and applied as float32 scalars; `step` is 1-based (step < 1:
 * ADVSTEP_EINVAL).  taps, adam_m, adam_v (L floats each) are updated in place; one small launch, no host read.  dh_out overlaps
 * none of the others. */
int advstep_filter_tap_update_f32(const void *partials_ws, float *taps, float *adam_m, float *adam_v, float *dh_out, int64_t B,
                                  int64_t T, int64_t L, int64_t step, double lr, double beta1, double beta2, double adam_eps,
                                  int ascend, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_FILTER_H_ */
