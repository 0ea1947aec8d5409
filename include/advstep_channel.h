/*
 * advstep_channel.h — C ABI of the simulated audio channel of libadvstep.so (torchattacks.Channel, torchattacks.EOTPGD and the
 * `channel/*` figures of evaluation.generate_attacks): a batched short FIR with a delay, a gain and a noise floor per (draw, row),
 * K draws per launch, and its adjoint summed over the draws, alone or fused with the PGD L-inf step.
 *
 * The reference has no such thing: its EOTPGD averages gradients of a deterministic model.  THE ARITHMETIC IS PART OF THIS ABI.
 * For a batch x (B, T) and K draws, draw j of row b has taps h[j, b, 0 .. L-1], an integer delay s[j, b], a gain g[j, b] and a
 * noise amplitude a[j, b]; row b has a centre c[b], the value that means silence in the row's units (-mn / (mx - mn) in the
 * attacks' min-max domain, 0 for a waveform).
 *
 *   xc[b, u]   = x[b, u] - c[b]  for 0 <= u < T,  0 otherwise                         (silence outside the utterance)
 *   acc        = 0;  for i = 0 .. L-1 in this order:  acc = acc + h[j,b,i] * xc[b, t - s[j,b] - i]
 *   y[j, b, t] = (c[b] + g[j,b] * acc) + a[j,b] * n[j,b,t]
 *   n[j,b,t]   = 2 * u01(R.v[t & 3]) - 1,
 *   R          = philox4x32_10(c0 = lo32(t >> 2), c1 = b, c2 = lo32(O), c3 = hi32(O), k0 = lo32(seed), k1 = hi32(seed)),
 *   O          = offset + j,   u01(w) = (float)(w >> 8) * 2^-24         (the generator and mapping of the library's random starts)
 *
 * and the adjoint, summed over the draws, with the same out-of-row rule (gy = 0 outside 0 .. T-1):
 *
 *   accj       = 0;  for i = 0 .. L-1 in this order:  accj = accj + h[j,b,i] * gy[j, b, u + s[j,b] + i]
 *   G[b, u]    = 0;  for j = 0 .. K-1 in this order:  G = G + g[j,b] * accj
 *
 * Every product and every sum is rounded to float32 on its own (no FMA contraction), so a float32 restatement in this order gives
 * the same BYTES.  Indices are computed in 64 bits: any int32 delay is legal, and a draw whose window lies wholly outside the row
 * gives c + a n (finite taps).  The output is not clamped: the channel is affine in x and its adjoint is exact.  a n is added also
 * where a = 0.
 *
 * taps, shift, gain, noise and center are device data the host cannot validate: the kernels are memory-safe for any values in
 * them (a delay only ever offsets a bounds-checked read; a NaN or infinite tap reaches the samples whose window holds it and
 * nothing else).
 *
 * Conventions are those of include/advstep.h: raw device pointers, int64_t sizes, stream-ordered launches, status codes, nothing
 * thrown, no state in the library, safe under stream capture, reruns bit-identical on any stream.  One launch each on the
 * (4096-sample tile, row) grid; the bytes do not depend on the alignment of any base or on T % 4.
 *
 * All entry points: ADVSTEP_EINVAL for a negative size, B > 65535, L < 1, L > ADVSTEP_CHANNEL_MAX_TAPS,
 * K > ADVSTEP_CHANNEL_MAX_DRAWS, a null pointer with non-zero sizes or a forbidden overlap; B == 0, T == 0 or K == 0 returns
 * ADVSTEP_OK, launches nothing and writes nothing.
 */
#ifndef ADVSTEP_CHANNEL_H_
#define ADVSTEP_CHANNEL_H_

#include <stddef.h>
#include <stdint.h>

#include "advstep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADVSTEP_CHANNEL_MAX_TAPS 256  /* 16 ms at 16 kHz */
#define ADVSTEP_CHANNEL_MAX_DRAWS 64

/* out[j, b, t] = y[j, b, t] above.  x (B, T), center (B), taps (K, B, L), shift (K, B) int32, gain (K, B), noise (K, B),
 * out (K, B, T), which overlaps none of the inputs.  A K-draw call equals K one-draw calls with offset + j.
 * Traffic: 4 B read and 4 K B written per sample (the K - 1 re-reads of a tile's window come from the cache). */
int advstep_channel_apply_f32(const float *x, const float *center, const float *taps, const int32_t *shift, const float *gain,
                              const float *noise, float *out, int64_t B, int64_t T, int64_t K, int64_t L, uint64_t seed,
                              uint64_t offset, advstep_stream_t stream);

/* out[b, u] = G[b, u] above.  grads (K, B, T), out (B, T), which overlaps none of the inputs.
 * Traffic: 4 K B read and 4 B written per sample. */
int advstep_channel_adjoint_f32(const float *grads, const float *taps, const int32_t *shift, const float *gain, float *out,
                                int64_t B, int64_t T, int64_t K, int64_t L, advstep_stream_t stream);

/* out = the move and projection of advstep_pgd_linf_step_f32(adv, G, orig, alpha, eps, lo, hi) — the same device function — with
 * G as advstep_channel_adjoint_f32 computes it, kept in registers: the averaged gradient never exists in memory.  out may be adv
 * itself (a thread reads its own samples before it writes them) and otherwise overlaps none of adv, orig, grads, taps, shift, gain.
 * Traffic: 4 K + 12 B per sample. */
int advstep_channel_eot_step_f32(const float *adv, const float *orig, const float *grads, const float *taps, const int32_t *shift,
                                 const float *gain, float *out, int64_t B, int64_t T, int64_t K, int64_t L, float alpha, float eps,
                                 float lo, float hi, advstep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ADVSTEP_CHANNEL_H_ */
