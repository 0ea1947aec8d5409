/*
 * advstep_spsa.h — C ABI of the score-based black-box attack of libadvstep.so (torchattacks.SPSA): simultaneous-perturbation
 * gradient estimation (Spall 1992; Uesato et al., ICML 2018) with the sign step of ZO-signSGD, inside the L-inf ball of
 * include/advstep.h's PGD.  The attacker submits waveforms and reads the detector's logit; nothing is differentiated.
 *
 * The reference has no such attack.  One iteration on a (B, T) batch with n direction pairs and probe size delta uses
 * S = 1 + 2 n SLOTS, stored slot-major as (S, B, T):
 *   slot 0          adv itself
 *   slot 1 + 2 j    clamp(adv + delta * v_j, lo, hi)
 *   slot 2 + 2 j    clamp(adv - delta * v_j, lo, hi)           j = 0 .. n - 1
 * with v_j a Rademacher vector in {+1, -1}^T per row (delta * v is exact, so a probe sample rounds once), then
 *   advstep_spsa_probe_f32      fills slots s0 .. s0 + ns - 1 (the caller may forward the slots in chunks)
 *   the detector                z (S, B): one logit per slot and row
 *   advstep_spsa_step_f32       estimates the gradient's sign from z, moves and projects like advstep_pgd_linf_step_f32
 *
 * THE DIRECTIONS are a function of (seed, offset, row b, sample t, direction j) and are never written to memory: both entry points
 * regenerate them, and the mapping is part of this ABI.  With q = t >> 2, k = t & 3 and O = offset + (j >> 5),
 *   R = philox4x32_10(c0 = lo32(q), c1 = b, c2 = lo32(O), c3 = hi32(O), k0 = lo32(seed), k1 = hi32(seed))
 *       (Salmon et al., SC'11: the generator of the library's random starts),
 *   bit i = 4 * (j & 31) + k of R's 128 bits is word R.v[i >> 5], bit i & 31,
 *   v_j[b, t] = -1 where that bit is set and +1 where it is clear.
 * One Philox call per quad of samples therefore serves 32 directions; an iteration consumes ceil(n / 32) offsets, so a caller that
 * wants fresh directions in every iteration passes offset = iteration * ceil(n / 32).
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes, nothing
 * thrown, no state in the library; float32 expression by expression, no FMA contraction, NaN-propagating clamps; 16-byte accesses
 * when T % 4 == 0 and every base is 16-byte aligned, sample by sample otherwise, with the same bits either way.  One launch each
 * on the (4096-sample tile, row) grid; no atomics, no LDS, no workgroup waits on another; reruns are bit-identical on any stream;
 * safe under stream capture.
 *
 * Both entry points: ADVSTEP_EINVAL for a negative size, B > 65535, more than ADVSTEP_SPSA_MAX_DIRECTIONS directions (probe: a
 * slot past 2 * ADVSTEP_SPSA_MAX_DIRECTIONS), a null pointer with non-zero sizes or a forbidden overlap; B == 0, T == 0 (probe:
 * ns == 0) returns ADVSTEP_OK, launches nothing and writes nothing.
 */
#ifndef ADVSTEP_SPSA_H_
#define ADVSTEP_SPSA_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upper bound of n, the direction pairs of one iteration (S <= 2049 slots).  The step kernel walks the 2 n logits of its row once
 * per thread, so its time grows with n while its traffic does not; the bound keeps that walk and the (S, B) logit buffer small. */
#define ADVSTEP_SPSA_MAX_DIRECTIONS 1024

/* out[s - s0, b, t] = slot s of the batch, s = s0 .. s0 + ns - 1 (see above); slot 0 is adv's bytes, unclamped.  `out` holds
 * (ns, B, T) floats and does not overlap adv.  A fill in chunks gives the same bytes as a whole one: a slot depends on
 * (adv, s, seed, offset) alone.  A thread keeps its samples of adv in registers and loops over the slots.
 * Traffic: 4 B read and 4 * ns B written per sample. */
int advstep_spsa_probe_f32(const float *adv, float *out, int64_t B, int64_t T, int64_t s0, int64_t ns, float delta, float lo,
                           float hi, uint64_t seed, uint64_t offset, advstep_stream_t stream);

/* z (S, B) float32: the detector's logits of the slots, S = 1 + 2 n; labels (B) int64; queries (B) int32, read and written.
 * Class 1 is z > 0, as in argmax(cat([-z, z])).  Row b is FOOLED when (z[0, b] > 0) != (labels[b] == 1)  (a NaN z[0, b] is
 * class 0).
 *   fooled row:  out row = adv row, byte for byte; queries[b] unchanged.
 *   otherwise:   sigma = +1 for label 0 and -1 for label 1 (any other label counts as 0): the direction in which the margin loss
 *                rises;  d_j = sigma * fl(z[1 + 2j, b] - z[2 + 2j, b])  (the sign flip is exact);
 *                g_t = (((v_0[t] d_0) + v_1[t] d_1) + ...) + v_{n-1}[t] d_{n-1}   in this order, every v d exact;
 *                out = the move and projection of advstep_pgd_linf_step_f32(adv, g, orig, alpha, eps, lo, hi) — the same
 *                device function;  queries[b] += S.
 *   sign(+-0) = 0: a row whose probes all tie does not move (it is still projected, and its queries are counted).  A NaN in d
 *   behaves as a NaN gradient does in advstep_pgd_linf_step_f32: sign(NaN) = 0.
 * n == 0 (S = 1) is allowed: g = 0.  The estimated gradient is never materialised.
 * Traffic: 12 B per sample plus the (S, B) logits (read once per workgroup, from the cache).
 * out may be adv itself (a thread reads its own samples before it writes them) and otherwise overlaps none of adv, orig, z,
 * labels, queries. */
int advstep_spsa_step_f32(const float *adv, const float *orig, const float *z, const int64_t *labels, int32_t *queries, float *out,
                          int64_t B, int64_t T, int64_t n, float alpha, float eps, float lo, float hi, uint64_t seed,
                          uint64_t offset, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_SPSA_H_ */
