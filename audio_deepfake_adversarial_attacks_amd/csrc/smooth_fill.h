// smooth_fill.h — the one body of the Gaussian-noised slots that smooth.hip (advstep_smooth_noise_f32) and smoothadv.hip
// (advstep_smoothadv_fill_f32) both launch (internal, like row_tiles.h).  The noise mapping is part of the ABI of
// include/advstep_smooth.h, and the attack on the smoothed detector must see the copies the certifier's fill would make of the
// same waveform, so the two kernels are instantiations of this function and cannot drift apart.

#ifndef ADVSTEP_SMOOTH_FILL_H
#define ADVSTEP_SMOOTH_FILL_H

#include "row_tiles.h"

namespace {

// Slots 0 .. ns - 1 of `out` (ns, B, T) for the workgroup's (tile, row): out[i, b, t] = fl(v + fl(sigma * z)), z =
// philox_normal4 at counter offset0 + i, and v = x[b, t], or with AFFINE v = fl(shift[b] + fl(scale[b] * x[b, t])).  A thread
// keeps its 16 values of v in registers and loops over the slots: 4 B read and 4 * ns B written per sample.  Inside a slot the
// thread's 4 quads are independent chains of Philox rounds and transcendentals for the scheduler to interleave.  No barrier.
template <bool VEC, bool AFFINE>
__device__ __forceinline__ void noised_slots(const float *__restrict__ x, const float *__restrict__ scale,
                                             const float *__restrict__ shift, float *__restrict__ out, int64_t B, int64_t T,
                                             int64_t ns, float sigma, uint64_t seed, uint64_t offset0) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    float4 a[kVecs];
    load_tile<VEC>(x + b * T, T, tile, 0.0f, a);
    if (AFFINE) {
        const float sc = scale[b], sh = shift[b];
        for_each_lane(a, [&](float &e) { e = sh + sc * e; });
    }
    for (int64_t i = 0; i < ns; ++i) {
        const uint64_t O = offset0 + (uint64_t)i;  // offset + s, carried into the high counter word
        float *slot = out + (i * B + b) * T;
#pragma unroll
        for (int v = 0; v < kVecs; ++v) {
            const int64_t q = quad_of(tile, v);
            if (!in_row(T, q, 0)) continue;
            const float4 z = philox_normal4((uint32_t)q, (uint32_t)b, seed, O);
            store4<VEC>(slot, T, q, make_float4(a[v].x + sigma * z.x, a[v].y + sigma * z.y, a[v].z + sigma * z.z, a[v].w + sigma * z.w));
        }
    }
}

}  // namespace

#endif  // ADVSTEP_SMOOTH_FILL_H
