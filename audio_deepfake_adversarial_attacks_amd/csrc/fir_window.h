// fir_window.h — the register-sliding FIR over an LDS window that channel.hip (up to 256 taps per (draw, row)) and filter.hip (one
// filter of up to 1025 taps for the batch) both instantiate: the padded window, its staging from a row, the tap loop and a
// thread's run of outputs (internal, like row_tiles.h, whose (4096-sample tile, row) grid the kernels run on).
//
//   * a thread owns a CONTIGUOUS run of kRun = 16 outputs, not the strided quads of row_tiles.h, whose neighbours in time sit in
//     other lanes.
//   * the workgroup stages the tile plus its halo of L - 1 samples in LDS.  Reads are one dword per lane at consecutive addresses
//     and every one is bounds-checked against the row in 64-bit arithmetic: the bytes cannot depend on alignment or on T % 4.
//   * the tap loop slides over registers: a thread holds 2 kRun - 1 consecutive window samples, applies kRun taps to its kRun
//     outputs from them (kRun^2 products with compile-time register indices), then moves kRun - 1 of them up (or down) and reads
//     kRun new ones.  LDS is read (run + L - 1) / run times per output, not L times; a tap is a scalar load (uniform address)
//     and enters the product as a scalar operand.
//   * a thread's window starts kRun floats after its neighbour's: 16 dwords apart is a 16-way bank conflict for ds_read_b32, so
//     logical slot q lives at q + (q >> 4) (lane stride 17 dwords: conflict-free), also for the staging writes.
//
// The window's capacity is the includer's: fir_lds_floats(max_taps) floats of LDS hold a tile and the halo of max_taps taps.
// Every product and sum rounds on its own (the library is built with -ffp-contract=off), in the order the ABI headers fix.

#ifndef ADVSTEP_FIR_WINDOW_H
#define ADVSTEP_FIR_WINDOW_H

#include "advstep_common.h"

namespace {

constexpr int kRun = 16;                                  // outputs per thread
constexpr int kTile = kWgThreads * kRun;                  // outputs per workgroup
static_assert(kTile == kWsRowTile, "the tile of row_tiles.h's launcher");

// logical window slots: kRun before the window (the forward's last, partial chunk of taps reads below it), the tile, its halo,
// and kRun after it (the adjoint's last chunk reads above it); what lies outside the staged part is read but never used
constexpr int fir_slots(int max_taps) { return kRun + kTile + (max_taps - 1) + kRun; }
constexpr int fir_lds_floats(int max_taps) { return fir_slots(max_taps) + (fir_slots(max_taps) >> 4) + 1; }

__device__ __forceinline__ int slot(int p) {              // window position p (>= -kRun) -> LDS index
    const int q = p + kRun;
    return q + (q >> 4);
}

// win[p] = src[first + p] (- c when CENTRED) inside the row, 0 outside it, p = 0 .. n - 1.  first may be any int64.
template <bool CENTRED>
__device__ __forceinline__ void stage_window(const float *__restrict__ src, int64_t T, int64_t first, int n, float c, float *lds) {
    for (int p = threadIdx.x; p < n; p += kWgThreads) {
        const int64_t u = first + p;
        float v = 0.0f;
        if (u >= 0 && u < T) v = CENTRED ? src[u] - c : src[u];
        lds[slot(p)] = v;
    }
}

// kRun taps h[0 .. kRun-1] (GUARD: only the first `left` of them) on the thread's kRun outputs from its 2 kRun - 1 window samples.
// FWD: tap u of output r reads a[kRun - 1 + r - u]; adjoint: a[r + u].
template <bool FWD, bool GUARD>
__device__ __forceinline__ void tap_chunk(const float (&a)[2 * kRun - 1], const float *__restrict__ h, int left, float (&acc)[kRun]) {
#pragma unroll
    for (int u = 0; u < kRun; ++u) {
        if (GUARD && u >= left) break;
        const float hv = h[u];
#pragma unroll
        for (int r = 0; r < kRun; ++r) acc[r] = acc[r] + hv * a[FWD ? kRun - 1 + r - u : r + u];
    }
}

// acc[r] = sum over i = 0 .. L-1, in this order, of h[i] * win[o + (L - 1) - i] (FWD) or h[i] * win[o + i] (adjoint),
// o = kRun * threadIdx.x + r, starting from +0.
template <bool FWD>
__device__ __forceinline__ void fir_run(const float *lds, const float *__restrict__ h, int L, float (&acc)[kRun]) {
    const int o0 = threadIdx.x * kRun;
    float a[2 * kRun - 1];
#pragma unroll
    for (int r = 0; r < kRun; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int m = 0; m < 2 * kRun - 1; ++m) a[m] = lds[slot(FWD ? o0 + (L - 1) - (kRun - 1) + m : o0 + m)];
    for (int i0 = 0; i0 < L; i0 += kRun) {
        if (i0 > 0) {
            if (FWD) {  // the window moves down by kRun: a[m + kRun] = a[m], kRun new samples below
#pragma unroll
                for (int m = 2 * kRun - 2; m >= kRun; --m) a[m] = a[m - kRun];
#pragma unroll
                for (int m = 0; m < kRun; ++m) a[m] = lds[slot(o0 + (L - 1) - i0 - (kRun - 1) + m)];
            } else {    // up by kRun
#pragma unroll
                for (int m = 0; m < kRun - 1; ++m) a[m] = a[m + kRun];
#pragma unroll
                for (int m = kRun - 1; m < 2 * kRun - 1; ++m) a[m] = lds[slot(o0 + i0 + m)];
            }
        }
        if (i0 + kRun <= L)
            tap_chunk<FWD, false>(a, h + i0, kRun, acc);
        else
            tap_chunk<FWD, true>(a, h + i0, L - i0, acc);
    }
}

// A thread's run of kRun samples starting at sample t0 of a row (t0 % kRun == 0); VEC = the rows are float4-addressable.
template <bool VEC>
__device__ __forceinline__ void load_run(const float *row, int64_t T, int64_t t0, float (&v)[kRun]) {
#pragma unroll
    for (int q = 0; q < kRun / 4; ++q) {
        if (VEC) {
            float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (t0 + 4 * q < T) f = *reinterpret_cast<const float4 *>(row + t0 + 4 * q);
            v[4 * q + 0] = f.x, v[4 * q + 1] = f.y, v[4 * q + 2] = f.z, v[4 * q + 3] = f.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[4 * q + k] = t0 + 4 * q + k < T ? row[t0 + 4 * q + k] : 0.0f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void store_run(float *row, int64_t T, int64_t t0, const float (&v)[kRun]) {
#pragma unroll
    for (int q = 0; q < kRun / 4; ++q) {
        if (VEC) {
            if (t0 + 4 * q < T)
                *reinterpret_cast<float4 *>(row + t0 + 4 * q) = make_float4(v[4 * q + 0], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t0 + 4 * q + k < T) row[t0 + 4 * q + k] = v[4 * q + k];
        }
    }
}

}  // namespace

#endif  // ADVSTEP_FIR_WINDOW_H
