// channel.hip — gfx950 (MI355X / CDNA4) kernels of the simulated audio channel (torchattacks.Channel, torchattacks.EOTPGD, the
// channel/* figures of the evaluation loop) + the C ABI declared in include/advstep_channel.h: a batched FIR of up to 256 taps with
// a delay, a gain and Philox noise per (draw, row), K draws per launch, and its adjoint summed over the draws, alone or with the PGD
// L-inf step as its epilogue.
//
// Unlike the streaming attack kernels this one is not bound by HBM: at L taps and K draws a sample costs 2 K L unfused float32
// operations against 4 + 4 K bytes (1 024 operations against 36 B at L = 64, K = 8).  The geometry serves the vector ALUs
// (the window, its staging, the tap loop and a thread's run are fir_window.h's, which filter.hip instantiates as well):
//
//   * grid = row_tiles.h's (4096-sample tile, row), 256 threads; a thread owns a CONTIGUOUS run of kRun = 16 outputs, not the
//     strided quads of row_tiles.h, whose neighbours in time sit in other lanes.
//   * per draw the workgroup stages the tile plus its halo of L - 1 samples of x - c (or of the draw's gradient) in LDS.  The
//     delay is an address offset that is uniform over the workgroup: it moves the window's first sample, nothing else, and every
//     global read is bounds-checked against the row in 64-bit arithmetic, so any int32 delay is safe.  Reads are one dword per
//     lane at consecutive addresses: the bytes cannot depend on alignment or on T % 4.
//   * the tap loop slides over registers: a thread holds 2 kRun - 1 consecutive window samples, applies kRun taps to its kRun
//     outputs from them (kRun^2 products with compile-time register indices), then moves kRun - 1 of them up (or down) and reads
//     kRun new ones.  LDS is read (run + L - 1) / run times per output, not L times; a tap is a scalar load (uniform address)
//     and enters the product as a scalar operand.
//   * a thread's window starts kRun floats after its neighbour's: 16 dwords apart is a 16-way bank conflict for ds_read_b32, so
//     logical slot q lives at q + (q >> 4) (lane stride 17 dwords: conflict-free), also for the staging writes.
//
// Built with -ffp-contract=off: every product and sum rounds on its own, in the order the header fixes.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_channel.h"
#include "advstep_common.h"
#include "fir_window.h"
#include "row_tiles.h"

namespace {

constexpr int kMaxTaps = ADVSTEP_CHANNEL_MAX_TAPS;
constexpr int kMaxDraws = ADVSTEP_CHANNEL_MAX_DRAWS;
constexpr int kLdsFloats = fir_lds_floats(kMaxTaps);      // the window of fir_window.h at the channel's capacity

// ---- a. the channel -------------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void channel_apply_kernel(const float *__restrict__ x, const float *__restrict__ center,
                                                                   const float *__restrict__ taps, const int32_t *__restrict__ shift,
                                                                   const float *__restrict__ gain, const float *__restrict__ noise,
                                                                   float *__restrict__ out, int64_t B, int64_t T, int K, int L,
                                                                   uint64_t seed, uint64_t offset) {
    __shared__ float lds[kLdsFloats];
    const int64_t b = blockIdx.y, tile0 = (int64_t)blockIdx.x * kTile, t0 = tile0 + threadIdx.x * kRun;
    const int n_out = T - tile0 < kTile ? (int)(T - tile0) : kTile;
    const float c = center[b];
    for (int j = 0; j < K; ++j) {
        const int64_t jb = (int64_t)j * B + b;
        const int64_t s = shift[jb];
        const float g = gain[jb], amp = noise[jb];
        if (j > 0) __syncthreads();  // every thread has read the previous draw's window
        stage_window<true>(x + b * T, T, tile0 - s - (L - 1), n_out + L - 1, c, lds);
        __syncthreads();
        if (t0 >= T) continue;       // (the barriers above are outside this branch)
        float acc[kRun];
        fir_run<true>(lds, taps + jb * L, L, acc);
        const uint64_t o = offset + (uint64_t)j;
#pragma unroll
        for (int q = 0; q < kRun / 4; ++q) {
            const Quad r = philox4x32_10((uint32_t)((t0 >> 2) + q), (uint32_t)b, (uint32_t)o, (uint32_t)(o >> 32), (uint32_t)seed,
                                         (uint32_t)(seed >> 32));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float n = 2.0f * u01(r.v[k]) - 1.0f;
                acc[4 * q + k] = (c + g * acc[4 * q + k]) + amp * n;
            }
        }
        store_run<VEC>(out + jb * T, T, t0, acc);
    }
}

// ---- b. the adjoint, summed over the draws; STEP: the PGD L-inf step as its epilogue ------------------------------------------------

// out may be adv (STEP): a thread reads its own samples of adv before it writes them, and the windows come from grads.
template <bool VEC, bool STEP>
__global__ __launch_bounds__(kWgThreads) void channel_adjoint_kernel(const float *adv, const float *__restrict__ orig,
                                                                     const float *__restrict__ grads, const float *__restrict__ taps,
                                                                     const int32_t *__restrict__ shift,
                                                                     const float *__restrict__ gain, float *out, int64_t B, int64_t T,
                                                                     int K, int L, float alpha, float eps, float lo, float hi) {
    __shared__ float lds[kLdsFloats];
    const int64_t b = blockIdx.y, tile0 = (int64_t)blockIdx.x * kTile, t0 = tile0 + threadIdx.x * kRun;
    const int n_out = T - tile0 < kTile ? (int)(T - tile0) : kTile;
    float G[kRun];
#pragma unroll
    for (int r = 0; r < kRun; ++r) G[r] = 0.0f;
    for (int j = 0; j < K; ++j) {
        const int64_t jb = (int64_t)j * B + b;
        const int64_t s = shift[jb];
        const float g = gain[jb];
        if (j > 0) __syncthreads();
        stage_window<false>(grads + jb * T, T, tile0 + s, n_out + L - 1, 0.0f, lds);
        __syncthreads();
        if (t0 >= T) continue;
        float acc[kRun];
        fir_run<false>(lds, taps + jb * L, L, acc);
#pragma unroll
        for (int r = 0; r < kRun; ++r) G[r] = G[r] + g * acc[r];
    }
    if (t0 >= T) return;
    if (STEP) {
        float a[kRun], x[kRun];
        load_run<VEC>(adv + b * T, T, t0, a);
        load_run<VEC>(orig + b * T, T, t0, x);
#pragma unroll
        for (int r = 0; r < kRun; ++r) G[r] = pgd_linf_elem(a[r], G[r], x[r], alpha, eps, lo, hi);
    }
    store_run<VEC>(out + b * T, T, t0, G);
}

bool sizes_ok(int64_t B, int64_t T, int64_t K, int64_t L) {
    return B >= 0 && T >= 0 && K >= 0 && B <= kMaxGridY && L >= 1 && L <= kMaxTaps && K <= kMaxDraws;
}

// Does `out` (out_bytes) overlap one of the per-draw parameter arrays?
bool overlaps_params(const void *out, size_t out_bytes, const float *taps, const int32_t *shift, const float *gain, int64_t B,
                     int64_t K, int64_t L) {
    const size_t kb = (size_t)K * B;
    return overlap2(out, out_bytes, taps, kb * L * sizeof(float)) || overlap2(out, out_bytes, shift, kb * sizeof(int32_t)) ||
           overlap2(out, out_bytes, gain, kb * sizeof(float));
}

}  // namespace

extern "C" {

int advstep_channel_apply_f32(const float *x, const float *center, const float *taps, const int32_t *shift, const float *gain,
                              const float *noise, float *out, int64_t B, int64_t T, int64_t K, int64_t L, uint64_t seed,
                              uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(sizes_ok(B, T, K, L));
    if (B == 0 || T == 0 || K == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && center && taps && shift && gain && noise && out);
    const size_t rows = (size_t)B * T * sizeof(float), outs = (size_t)K * rows;
    ADVSTEP_REQUIRE(!overlap2(out, outs, x, rows) && !overlap2(out, outs, center, (size_t)B * sizeof(float)));
    ADVSTEP_REQUIRE(!overlaps_params(out, outs, taps, shift, gain, B, K, L));
    ADVSTEP_REQUIRE(!overlap2(out, outs, noise, (size_t)K * B * sizeof(float)));
    launch_tiles(ROW_KERNEL_PAIR(channel_apply_kernel), rows_vec(T, {out}), B, T, as_stream(stream), x, center, taps, shift, gain,
                 noise, out, B, T, (int)K, (int)L, seed, offset);
    return status_after_launch();
}

int advstep_channel_adjoint_f32(const float *grads, const float *taps, const int32_t *shift, const float *gain, float *out,
                                int64_t B, int64_t T, int64_t K, int64_t L, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(sizes_ok(B, T, K, L));
    if (B == 0 || T == 0 || K == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(grads && taps && shift && gain && out);
    const size_t rows = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(out, rows, grads, (size_t)K * rows) && !overlaps_params(out, rows, taps, shift, gain, B, K, L));
    launch_tiles(ROW_KERNEL_PAIR(channel_adjoint_kernel, false), rows_vec(T, {out}), B, T, as_stream(stream),
                 (const float *)nullptr, (const float *)nullptr, grads, taps, shift, gain, out, B, T, (int)K, (int)L, 0.0f, 0.0f, 0.0f,
                 0.0f);
    return status_after_launch();
}

int advstep_channel_eot_step_f32(const float *adv, const float *orig, const float *grads, const float *taps, const int32_t *shift,
                                 const float *gain, float *out, int64_t B, int64_t T, int64_t K, int64_t L, float alpha, float eps,
                                 float lo, float hi, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(sizes_ok(B, T, K, L));
    if (B == 0 || T == 0 || K == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && orig && grads && taps && shift && gain && out);
    const size_t rows = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(out == adv || !overlaps(out, adv, rows));
    ADVSTEP_REQUIRE(!overlaps(out, orig, rows) && !overlap2(out, rows, grads, (size_t)K * rows));
    ADVSTEP_REQUIRE(!overlaps_params(out, rows, taps, shift, gain, B, K, L));
    launch_tiles(ROW_KERNEL_PAIR(channel_adjoint_kernel, true), rows_vec(T, {adv, orig, out}), B, T, as_stream(stream), adv, orig,
                 grads, taps, shift, gain, out, B, T, (int)K, (int)L, alpha, eps, lo, hi);
    return status_after_launch();
}

}  // extern "C"
