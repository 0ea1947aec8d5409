// direction_bits.h — the Rademacher directions of the black-box attacks (spsa.hip, hsj.hip), regenerated from Philox and never
// stored (internal, like advstep_common.h).  The mapping is part of the C ABI: include/advstep_spsa.h states it, and
// include/advstep_hsj.h refers to it.  One Philox call per quad of samples carries 32 directions: bit 4 * (j & 31) + k of its 128
// bits is direction j's sign at sample k of the quad, so word w of a call holds the 8 directions 8 w .. 8 w + 7, direction i of
// them at bits 4 i .. 4 i + 3.

#ifndef ADVSTEP_DIRECTION_BITS_H
#define ADVSTEP_DIRECTION_BITS_H

#include "advstep_common.h"

namespace {

// The 128 sign bits of quad q of row b for directions 32 * call .. 32 * call + 31.
__device__ __forceinline__ Quad direction_bits(int64_t q, int64_t b, uint64_t seed, uint64_t offset, int call) {
    const uint64_t o = offset + (uint64_t)call;
    return philox4x32_10((uint32_t)q, (uint32_t)b, (uint32_t)o, (uint32_t)(o >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Direction j's 4 sign bits of the quad (bit k: sample k).  j is uniform over the workgroup, so the word is chosen by scalar
// selects, not by an indexed read of the register array.
__device__ __forceinline__ uint32_t direction_nibble(const Quad &r, int j) {
    const int w = (j & 31) >> 3;
    const uint32_t word = w == 0 ? r.v[0] : w == 1 ? r.v[1] : w == 2 ? r.v[2] : r.v[3];
    return (word >> (4 * (j & 7))) & 15u;
}

// +-m by sign bit `bit` of `nib`: a set bit is v = -1.
__device__ __forceinline__ float signed_by(float m, uint32_t nib, int bit) { return ((nib >> bit) & 1u) ? -m : m; }

}  // namespace

#endif  // ADVSTEP_DIRECTION_BITS_H
