/*
 * advstep_universal.h — C ABI of the universal perturbation of libadvstep.so (torchattacks.UniversalPGD): ONE delta of T samples
 * that is added to every utterance.  Two memory-bound passes are all it needs beyond include/advstep.h: the reduction of a batch
 * of gradients over its rows, (B, T) -> (T), and the broadcast of delta over a batch.
 *
 * The reference has no such attack.  Fitting sees, per batch,
 *   adv  = universal_apply(x, delta, w)              w_b = [y_b == source] / (mx_b - mn_b), or 1
 *   g    = d loss / d adv                             the model, (B, T)
 *   s    = universal_colsum(g, w)                     d loss / d delta = sum_b w_b g_b, (T)
 *   the update of delta                               NO NEW KERNEL: delta is a (1, T) row whose `orig` is a row of zeros,
 *     L-inf:  advstep_pgd_linf_step_f32(adv = delta, grad = s, orig = 0, alpha, eps, lo = -eps, hi = eps)
 *     L2:     advstep_pgd_l2_step_f32(adv = delta, grad = s, orig = 0, B = 1, T, alpha, eps, eps_div, lo = -eps, hi = eps)
 *   With orig = 0 the step's d = (delta + alpha * dir) - 0 is the moved delta itself, its projection onto the eps ball around 0
 *   is the projection of delta, and the [lo, hi] = [-eps, eps] clamp that follows acts on a point the projection already put
 *   inside the ball: for L-inf it changes nothing, for L2 it only ever removes rounding excess of a sample (|d_t f| <= ||d|| f
 *   <= eps up to rounding).
 * and evaluating a frozen delta is universal_apply alone: one launch per batch.
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes,
 * nothing thrown, no state in the library; float32 expression by expression, no FMA contraction, NaN-propagating clamps;
 * 16-byte accesses when T % 4 == 0 and every base is 16-byte aligned, sample by sample otherwise, with the same bits either way.
 * No atomics, no workgroup waits on another, no LDS; reruns are bit-identical on any stream; safe under stream capture.
 *
 * All entry points: ADVSTEP_EINVAL for a negative size, B > 65535, a null pointer with B > 0 and T > 0 (row_weight excepted:
 * null means w_b = 1 for every row) or a forbidden overlap; B == 0 or T == 0 returns ADVSTEP_OK, launches nothing and writes
 * nothing.
 */
#ifndef ADVSTEP_UNIVERSAL_H_
#define ADVSTEP_UNIVERSAL_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows per row group of the column sum (R below). */
#define ADVSTEP_UNIVERSAL_GROUP_ROWS 16

/* Bytes of the workspace of advstep_universal_colsum_f32 for a (B, T) batch: G = ceil(B / R) planes of T floats, each padded to
 * a multiple of 4 floats, when G > 1; 0 when one group holds every row (B <= R: no workspace is touched, `ws` may be null), when
 * the batch is empty or a size is negative.  Every call rewrites what it reads: the buffer needs no initialisation and carries
 * nothing from one call to the next. */
size_t advstep_universal_workspace_bytes(int64_t B, int64_t T);

/* out[t] = sum_b fl(w_b * grad[b, t]),  w_b = row_weight ? row_weight[b] : 1   (every product rounds once; w_b = 0 multiplies
 * like any other weight: 0 * NaN = NaN, 0 * inf = NaN).
 * The order of the additions is a function of (B, T) alone: rows are cut into G = ceil(B / R) groups of R consecutive rows, group
 * g's partial is  P_g[t] = (((0 + p_{gR}) + p_{gR + 1}) + ...)  over its rows in order, and  out[t] = ((0 + P_0[t]) + P_1[t]) + ...
 * over the groups in order (G == 1: out = P_0, written by the first launch).  A NaN or inf in column t reaches out[t] and no other
 * column.
 * grid = (ceil(T / 1024) column tiles, G): a thread owns 4 adjacent columns and walks its group's rows with R independent loads
 * in flight; the second launch (G > 1) folds the G planes of the workspace column by column.  Traffic: 4 B per sample of grad,
 * plus 8 B per column and group.
 * `ws`: advstep_universal_workspace_bytes(B, T) bytes, 16-byte aligned; ADVSTEP_EWORKSPACE if null, unaligned or too small while
 * G > 1.  out holds T floats and overlaps neither grad nor row_weight (nor ws). */
int advstep_universal_colsum_f32(const float *grad, const float *row_weight, float *out, int64_t B, int64_t T, void *ws,
                                 size_t ws_bytes, advstep_stream_t stream);

/* out[b, t] = clamp(fl(x[b, t] + fl(w_b * delta[t])), lo, hi),  w_b = row_weight ? row_weight[b] : 1.
 * One launch on the (4096-sample tile, row) grid, 8 B per sample (delta's T floats are read once per row, from the cache).  A row
 * with w_b = 0 and a finite delta is clamp(x + 0): the row itself, bit for bit, wherever x lies in [lo, hi] (a sample -0 comes
 * back +0, as x + 0 does).
 * out may be x itself (a thread reads its own samples before it writes them) and otherwise overlaps none of x, delta (T floats),
 * row_weight. */
int advstep_universal_apply_f32(const float *x, const float *delta, const float *row_weight, float *out, int64_t B, int64_t T,
                                float lo, float hi, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_UNIVERSAL_H_ */
