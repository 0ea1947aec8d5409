/*
 * advstep_smooth.h — C ABI of randomized smoothing in libadvstep.so (torchattacks.Smoothing; Cohen, Rosenfeld and Kolter,
 * ICML 2019): the Gaussian-noised copies of a batch and the vote count over their logits.  The smoothed detector classifies
 * many copies x + N(0, sigma^2 I) of an utterance and takes the majority class; a lower confidence bound on that class's
 * probability becomes a certified L2 radius (metrics.py does the statistics on the host).
 *
 * The reference has no such procedure.  The copies of a (B, T) batch are SLOTS, stored slot-major as (ns, B, T) exactly as the
 * probes of include/advstep_spsa.h, so the caller forwards them through the detector in chunks of whole slots:
 *   advstep_smooth_noise_f32    fills slots s0 .. s0 + ns - 1
 *   the detector                z (ns, B): one logit per slot and row
 *   advstep_smooth_tally_i32    counts[b] += the slots of row b whose logit says class 1
 *
 * THE NOISE is a function of (seed, offset, slot s, row b, sample t) and is never written to memory on its own; the mapping is
 * part of this ABI.  With q = t >> 2, k = t & 3 and O = offset + s (a 64-bit sum: it carries into the high counter word),
 *   R = philox4x32_10(c0 = lo32(q), c1 = b, c2 = lo32(O), c3 = hi32(O), k0 = lo32(seed), k1 = hi32(seed))
 *       (Salmon et al., SC'11: the generator of the library's random starts),
 *   u_i = ((R.v[i] >> 8) + 1) * 2^-24 in (0, 1] for i = 0, 2 and u_i = (R.v[i] >> 8) * 2^-24 in [0, 1) for i = 1, 3,
 *   r0 = sqrt(-2 ln u_0), r1 = sqrt(-2 ln u_2), t0 = 2 pi u_1, t1 = 2 pi u_3      (Box-Muller on two uniform pairs),
 *   z[k] = (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1)[k]
 * in float32 with the hardware logarithm, sine and cosine (about 1e-6 absolute): the normals of advstep_pgd_l2_init_philox_f32,
 * the same device function.  |z| <= sqrt(-2 ln 2^-24) = 5.77.  A slot consumes one offset, so a caller that wants fresh noise
 * for its next ns copies passes offset + ns.
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes, nothing
 * thrown, no state in the library; float32 expression by expression, no FMA contraction; 16-byte accesses when T % 4 == 0 and
 * every base is 16-byte aligned, sample by sample otherwise, with the same bits either way.  One launch each; no atomics, no
 * LDS, no workgroup waits on another; reruns are bit-identical on any stream; safe under stream capture.
 */
#ifndef ADVSTEP_SMOOTH_H_
#define ADVSTEP_SMOOTH_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[s - s0, b, t] = fl(x[b, t] + fl(sigma * z)), s = s0 .. s0 + ns - 1, z as above at counter offset + s.  There is no clamp
 * (the waveform domain has no box) and a NaN in x propagates.  `out` holds (ns, B, T) floats and does not overlap x.  A fill in
 * chunks gives the same bytes as a whole one: a slot depends on (x, s, sigma, seed, offset) alone.  On the (4096-sample tile,
 * row) grid a thread keeps its samples of x in registers and loops over the slots.
 * Traffic: 4 B read and 4 * ns B written per sample.
 * ADVSTEP_EINVAL for a negative size, B > 65535, a null pointer with non-zero sizes, out overlapping x, or a sigma that is
 * negative or not finite; B == 0, T == 0 or ns == 0 returns ADVSTEP_OK, launches nothing and writes nothing. */
int advstep_smooth_noise_f32(const float *x, float *out, int64_t B, int64_t T, int64_t s0, int64_t ns, float sigma, uint64_t seed,
                             uint64_t offset, advstep_stream_t stream);

/* counts[b] += #{s : z[s, b] > 0} for z (ns, B) float32 and counts (B) int32, read and written.  Class 1 is z > 0, as in
 * argmax(cat([-z, z])); a NaN logit is class 0, the convention of advstep_spsa_step_f32.  One thread per row walks its ns logits.
 * ADVSTEP_EINVAL for a negative size, a null pointer with non-zero sizes or counts overlapping z; B == 0 or ns == 0 returns
 * ADVSTEP_OK, launches nothing and writes nothing. */
int advstep_smooth_tally_i32(const float *z, int32_t *counts, int64_t B, int64_t ns, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_SMOOTH_H_ */
