/*
 * advstep_multi.h — C ABI of the MultiAttack row router of libadvstep.so: one stage of the bookkeeping of
 * adversarial_attacks/torchattacks/attacks/multiattack.py:55-66 (judge the member's output, keep the first successful
 * adversarial row per utterance, compact the survivors for the next member).
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes,
 * nothing thrown, no state in the library.  The pass only moves bytes: every output sample is a bit-for-bit copy of one input
 * sample (NaN payloads and signed zeros included), so reruns are bit-identical.  No atomics; no launch waits on another
 * workgroup.
 */
#ifndef ADVSTEP_MULTI_H_
#define ADVSTEP_MULTI_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One routing stage over the n rows of a sub-batch of a (B, T) batch.
 *   adv (n, T)      the member's output                      x (n, T)   the sub-batch the member was given
 *   z (n)           the logit of model(adv)                  labels (n) int64
 *   rows (n) int32  index of row i in the full batch, ascending, each in [0, B)
 *
 *   pre[i]   = z[i] > 0            the first maximal index of cat([-z, z], 1): z = +-0 and NaN give class 0
 *   wrong[i] = pre[i] != labels[i]
 * and, with the rows visited in ascending i and k starting at 0:
 *   wrong:  final[rows[i], :] = adv[i, :]
 *   kept:   next_x[k, :] = x[i, :],  next_y[k] = labels[i],  next_rows[k] = rows[i],  k++
 *   counts[0] = number wrong,  counts[1] = number kept = k           (int32, on the device)
 * Rows of final that no wrong row names, and rows k .. n - 1 of next_x / next_y / next_rows, are not written.  A rows[i]
 * outside [0, B) is counted but its row is not copied (nothing is ever written outside final's B rows).
 *
 * Two launches: a one-wave select that gives every row its destination (into `scratch`, int32[n], the caller's) and writes
 * next_y, next_rows and counts; then one copy pass over a (tile, row) grid that moves every sample exactly once (8 B per
 * sample: 4 read, 4 written), with 16-byte accesses when T % 4 == 0 and adv, x, final and next_x are 16-byte aligned and
 * sample by sample otherwise.
 *
 * Aliasing (checked, ADVSTEP_EINVAL): next_x overlaps none of x, adv and final — a compaction in place would race between
 * workgroups — and final overlaps none of adv, x and next_x.  next_y / next_rows must not overlap labels / rows either.
 *
 * ADVSTEP_EINVAL for a negative size, n > 65535, B < n, B > INT32_MAX, or a null pointer with n > 0 and T > 0;
 * n == 0 or T == 0 returns ADVSTEP_OK, launches nothing and writes nothing (not even counts). */
int advstep_multi_route_f32(const float *adv, const float *x, const float *z, const int64_t *labels, const int32_t *rows,
                            float *final_rows, float *next_x, int64_t *next_y, int32_t *next_rows, int32_t *counts,
                            int32_t *scratch, int64_t n, int64_t B, int64_t T, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_MULTI_H_ */
