/*
 * advstep_hsj.h — C ABI of the label-only black-box attack of libadvstep.so (torchattacks.HopSkipJump): HopSkipJump (Chen, Jordan
 * and Wainwright, IEEE S&P 2020) in its L-inf form, restated with device-resident state and fixed shapes.  The attacker submits
 * waveforms and reads the detector's DECISION; the logits below are only ever compared with 0.
 *
 * The reference has no such attack.  Per row b of a (B, T) batch: orig is the utterance, cur the row's current adversarial point,
 * dist[b] = max |cur - orig| (plane 0 of advstep_perturb_stats_f32), active[b] != 0 a row that still moves.  A logit z is
 * ADVERSARIAL for row b iff (z > 0) != (labels[b] == 1): +-0 and NaN are class 0, as in include/advstep_spsa.h.
 *
 *   point(r) = clamp(orig + clamp(cur - orig, -r, r), lo, hi)       one subtraction, one addition, in this order
 *
 * 1. Boundary search: R rounds of bisection on the radius r of point(r), one launch per model query.  The state is (4, B) float32,
 *    plane p of row b at state[p * B + b]: 0 lo, 1 hi, 2 mid, 3 dist0.
 *      advstep_hsj_search_open_f32     lo = 0, hi = dist0 = dist[b], mid = (lo + hi) * 0.5;  out = point(mid)
 *      advstep_hsj_search_next_f32     z judged point(mid): adversarial -> hi = mid, else lo = mid; mid = (lo + hi) * 0.5;
 *                                      out = point(mid)
 *      advstep_hsj_search_close_f32    the same decision; where hi < dist0: out = point(hi) — the bytes of the probe that was judged
 *                                      adversarial, the same function of the same inputs — otherwise out = cur's bytes
 *                                      (orig + fl(cur - orig) need not be cur); queries[b] += rounds
 *    `next` reads one state buffer and writes another (ping-pong): every workgroup of a row derives the same decision whenever
 *    it runs.
 * 2. Normal estimate: advstep_hsj_probe_f32 fills slot j = clamp(cur + (bit_j ? -m : m), lo, hi), m = mag[b], bit_j the direction
 *    bit of include/advstep_spsa.h: the same Philox mapping, 32 directions per call, O = offset + (j >> 5).
 * 3. Step: advstep_hsj_candidates_f32 reads the n logits of the probes.  With c the row's adversarial probes and, for a sample,
 *    a = the adversarial probes whose bit is set there, e = the other probes whose bit is set there,
 *      v = c e - (n - c) a     if 0 < c < n       (n / 2 times the estimate sum_j (phi_j - mean phi) v_j, an integer)
 *      v = n - 2 a             if c == n          (the probes weighted by phi_j itself: all agree)
 *      v = 2 e - n             if c == 0
 *    s = sign(v), exact in int32 for n <= 1024; xi = fl(dist[b] * xi_rel);
 *      slot k = clamp(cur + (xi * 2^-k) * s, lo, hi)      k = 0 .. trials - 1
 *    advstep_hsj_take_f32 reads the logits of the candidates: the first adversarial slot k becomes the row (queries[b] += n + k + 1);
 *    none: the row stays (queries[b] += n + trials).
 * An INACTIVE row is copied byte for byte by every entry point (a -0 keeps its sign), counts no query, and every plane of its
 * search state is dist[b].
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes, nothing
 * thrown, no state in the library; float32 expression by expression, no FMA contraction, NaN-propagating clamps; 16-byte accesses
 * when T % 4 == 0 and every base is 16-byte aligned, sample by sample otherwise, with the same bits either way.  One launch each on
 * the (4096-sample tile, row) grid; no atomics, no workgroup waits on another; reruns are bit-identical on any stream (the query
 * counts are read and written by one thread per row); safe under stream capture.
 *
 * Every entry point: ADVSTEP_EINVAL for a negative size, B > 65535, a cap exceeded, a null pointer with non-zero sizes, or an
 * overlap of an output with any other operand that is not a stated alias; B == 0 or T == 0 (probe: ns == 0; candidates, take:
 * trials == 0) returns ADVSTEP_OK, launches nothing and writes nothing.
 */
#ifndef ADVSTEP_HSJ_H_
#define ADVSTEP_HSJ_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upper bound of n, the probes of one normal estimate: c e - (n - c) a stays below 2^21 in int32, and the (n, B) logit buffer and the
 * 2 n decision bits a workgroup keeps in LDS stay small. */
#define ADVSTEP_HSJ_MAX_DIRECTIONS 1024
/* Upper bound of `trials`, the candidate slots of one step. */
#define ADVSTEP_HSJ_MAX_TRIALS 8

/* cur, orig, out (B, T) float32; dist (B) float32; active (B) int32; state (4, B) float32, written.  out overlaps nothing.
 * Traffic: 12 B per sample of an active row, 8 B of an inactive one. */
int advstep_hsj_search_open_f32(const float *cur, const float *orig, const float *dist, const int32_t *active, float *state,
                                float *out, int64_t B, int64_t T, float lo, float hi, advstep_stream_t stream);

/* z (B) float32: the logits of the previous launch's `out`; labels (B) int64; state read, state_out written (another buffer).
 * out overlaps nothing (it may be the buffer z was computed from).  Traffic: as open. */
int advstep_hsj_search_next_f32(const float *cur, const float *orig, const float *z, const int64_t *labels, const int32_t *active,
                                const float *state, float *state_out, float *out, int64_t B, int64_t T, float lo, float hi,
                                advstep_stream_t stream);

/* queries (B) int32, read and written: rounds (>= 0) is added for active rows.  out may be cur itself (a thread reads its own
 * samples before it writes them; only rows with hi < dist0 are then written) and otherwise overlaps nothing.
 * Traffic: 12 B per sample of a row that moves. */
int advstep_hsj_search_close_f32(const float *cur, const float *orig, const float *z, const int64_t *labels, const int32_t *active,
                                 const float *state, int32_t *queries, int64_t rounds, float *out, int64_t B, int64_t T, float lo,
                                 float hi, advstep_stream_t stream);

/* out[j - s0, b, t] = slot j, j = s0 .. s0 + ns - 1, s0 + ns <= ADVSTEP_HSJ_MAX_DIRECTIONS; there is no copy of cur among the
 * slots.  mag (B) float32.  A fill in chunks gives the same bytes as a whole one.  out holds (ns, B, T) floats and overlaps nothing.
 * Traffic: 4 B read and 4 * ns B written per sample. */
int advstep_hsj_probe_f32(const float *cur, const float *mag, const int32_t *active, float *out, int64_t B, int64_t T, int64_t s0,
                          int64_t ns, float lo, float hi, uint64_t seed, uint64_t offset, advstep_stream_t stream);

/* z (n, B) float32: the logits of the n probes filled with the same (seed, offset); 0 <= n <= ADVSTEP_HSJ_MAX_DIRECTIONS (n == 0:
 * s = 0); out (trials, B, T), trials <= ADVSTEP_HSJ_MAX_TRIALS, overlaps nothing.  One launch writes every slot, so s is computed
 * once: per sample and 8 directions two ANDs and two population counts of a Philox word against row-uniform masks built from the
 * decisions.  Traffic: 4 B read and 4 * trials B written per sample plus the (n, B) logits (read once per workgroup). */
int advstep_hsj_candidates_f32(const float *cur, const float *z, const int64_t *labels, const float *dist, const int32_t *active,
                               float *out, int64_t B, int64_t T, int64_t n, int64_t trials, float xi_rel, float lo, float hi,
                               uint64_t seed, uint64_t offset, advstep_stream_t stream);

/* cand (trials, B, T); zc (trials, B) float32: the candidates' logits; n >= 0: the probes the estimate spent.  out may be cur itself
 * (only the rows that move are then written) and otherwise overlaps nothing.  Traffic: 8 B per sample of a row that moves. */
int advstep_hsj_take_f32(const float *cur, const float *cand, const float *zc, const int64_t *labels, const int32_t *active,
                         int32_t *queries, float *out, int64_t B, int64_t T, int64_t n, int64_t trials, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_HSJ_H_ */
