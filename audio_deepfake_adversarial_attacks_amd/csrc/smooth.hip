// smooth.hip — gfx950 (MI355X / CDNA4) kernels of randomized smoothing (torchattacks.Smoothing) + the C ABI declared in
// include/advstep_smooth.h: the fill of Gaussian-noised copies of a batch and the vote count over their logits.
//
// The fill is a row-independent streaming pass on the (4096-sample tile, row) grid of row_tiles.h, shaped like spsa.hip's probe
// kernel: a thread keeps its 16 samples of x in registers and loops over the slots, so it reads 4 B and writes 4 * ns B per
// sample.  The noise is regenerated from Philox per (slot, row, quad) and never stored on its own: one philox_normal4 call —
// advstep_common.h's, the normals of the PGD-L2 random start, unchanged — gives the 4 normals of a quad (the header fixes the
// mapping).  Inside a slot the thread's 4 quads are independent chains of Philox rounds and transcendentals, so the unrolled
// quad loop gives the scheduler 4 of them to interleave.  The tally gives a row to one thread: ns * B logits is a few kilobytes.
//
// Built with -ffp-contract=off: out = fl(x + fl(sigma * z)), two roundings.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_smooth.h"
#include "advstep_common.h"
#include "row_tiles.h"
#include "smooth_fill.h"

namespace {

// ---- a. the noised copies -------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void smooth_noise_kernel(const float *__restrict__ x, float *__restrict__ out, int64_t B,
                                                                  int64_t T, int64_t ns, float sigma, uint64_t seed,
                                                                  uint64_t offset0) {
    noised_slots<VEC, false>(x, nullptr, nullptr, out, B, T, ns, sigma, seed, offset0);  // smooth_fill.h: smoothadv.hip's fill too
}

// ---- b. the votes -----------------------------------------------------------------------------------------------------------------

constexpr int kTallyThreads = 64;

__global__ __launch_bounds__(kTallyThreads) void smooth_tally_kernel(const float *__restrict__ z, int32_t *__restrict__ counts,
                                                                     int64_t B, int64_t ns) {
    const int64_t b = (int64_t)blockIdx.x * kTallyThreads + threadIdx.x;
    if (b >= B) return;
    int32_t c = 0;
    for (int64_t s = 0; s < ns; ++s) c += z[s * B + b] > 0.0f;  // NaN is class 0
    counts[b] += c;
}

}  // namespace

extern "C" {

int advstep_smooth_noise_f32(const float *x, float *out, int64_t B, int64_t T, int64_t s0, int64_t ns, float sigma, uint64_t seed,
                             uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && s0 >= 0 && ns >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(sigma >= 0.0f && sigma <= 3.402823466e+38f);  // finite and not negative: false for NaN
    if (B == 0 || T == 0 || ns == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && out);
    const size_t rows = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(out, (size_t)ns * rows, x, rows));
    launch_tiles(ROW_KERNEL_PAIR(smooth_noise_kernel), rows_vec(T, {x, out}), B, T, as_stream(stream), x, out, B, T, ns, sigma, seed,
                 offset + (uint64_t)s0);
    return status_after_launch();
}

int advstep_smooth_tally_i32(const float *z, int32_t *counts, int64_t B, int64_t ns, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && ns >= 0);
    if (B == 0 || ns == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(z && counts);
    ADVSTEP_REQUIRE(!overlap2(counts, (size_t)B * sizeof(int32_t), z, (size_t)ns * B * sizeof(float)));
    hipLaunchKernelGGL(smooth_tally_kernel, dim3((unsigned)ceil_div(B, kTallyThreads)), dim3(kTallyThreads), 0, as_stream(stream), z,
                       counts, B, ns);
    return status_after_launch();
}

}  // extern "C"
