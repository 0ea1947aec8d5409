// filter.hip — gfx950 (MI355X / CDNA4) kernels of the universal adversarial FIR filter (torchattacks.UniversalFilter) + the C ABI
// declared in include/advstep_filter.h: ONE filter of up to 1025 taps for the whole batch with a row mask and the attack domain's
// clamp, the gradient of a loss with respect to its taps — the library's only reduction over rows AND time — and the fold of that
// gradient with an Adam step on the taps.
//
//   * filter_apply is channel.hip's forward with fewer loads: fir_window.h's window (here with room for 1025 taps), staged once
//     per tile, and its register-sliding tap loop; the taps are one array for every row.  A masked row's workgroup copies its tile.
//   * filter_tap_grad is that loop with the roles swapped.  A tile's partial of tap i is a correlation over the tile's samples,
//     p[i] = sum_t gm[t] xc[t + P - i]: with j = L - 1 - i and the window win[q] = xc[tile0 - P + q] it is sum_o gm[o] win[o + j],
//     the adjoint form of fir_window.h with gm in the place of the taps and the taps in the place of the outputs.  "Thread owns
//     samples" would need L workgroup-wide reductions per tile; here a thread owns 16 consecutive taps j (16 accumulators) and a
//     SEGMENT of the tile's samples, holds 31 consecutive window samples in registers, takes 16 samples of gm from LDS — 256
//     fused multiply-adds per 32 LDS reads — and slides the window up by 16.  The 256 threads are (segment, tap lane) pairs: TL =
//     ceil(L / 16) tap lanes and NS = floor(256 / TL) segments, so 252 threads work at L = 129, 256 at 255, 255 at 257 and 195 at
//     1025 (a mapping of one wave per segment with 16 taps per lane would leave 55 of 64 lanes idle at L = 129).  Lanes of one
//     segment read the same gm (an LDS broadcast); lanes whose segment + tap offset coincide share their window reads, and all
//     others are 17 dwords apart under the q + (q >> 4) padding, which gm's staging uses as well.  The NS segment sums of a tap
//     are folded through LDS in segment order.
//   * filter_tap_update: one thread per tap walks the (tile, row) partials in the order the header fixes and takes the Adam step.
//
// The forward rounds every product and sum on its own (-ffp-contract=off); the tap gradient uses explicit fmaf (the header says
// why that is allowed there).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_filter.h"
#include "advstep_common.h"
#include "fir_window.h"
#include "row_tiles.h"

namespace {

constexpr int kMaxTaps = ADVSTEP_FILTER_MAX_TAPS;
constexpr int kGroupRows = ADVSTEP_FILTER_GROUP_ROWS;
constexpr int kLdsFloats = fir_lds_floats(kMaxTaps);      // the window of fir_window.h with room for 1025 taps: 21.4 KiB
constexpr int kGmFloats = kTile + (kTile >> 4) + 1;       // a tile of gm, then the threads' 16 sums each, both padded: 17 KiB
constexpr int kUpdateThreads = 64;

static_assert(((kMaxTaps + kRun - 1) / kRun - 1) * kRun + (kTile - kRun) + 2 * kRun - 2 < fir_slots(kMaxTaps) - kRun,
              "the last tap lane's last window read lies inside the window");

__device__ __forceinline__ int pad16(int q) { return q + (q >> 4); }

// ---- a. the filter ------------------------------------------------------------------------------------------------------------------

// out may be x where the host allows it (one tile per row, or L == 1): the workgroup has staged what it reads before it writes.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void filter_apply_kernel(const float *x, const float *__restrict__ center,
                                                                  const float *__restrict__ row_mask,
                                                                  const float *__restrict__ taps, float *out, int64_t T, int L,
                                                                  float lo, float hi) {
    __shared__ float lds[kLdsFloats];
    const int64_t b = blockIdx.y, tile0 = (int64_t)blockIdx.x * kTile, t0 = tile0 + threadIdx.x * kRun;
    const int n_out = T - tile0 < kTile ? (int)(T - tile0) : kTile;
    float acc[kRun];
    if (row_mask && row_mask[b] == 0.0f) {  // uniform over the workgroup: no barrier is skipped by a part of it
        if (t0 >= T) return;
        load_run<VEC>(x + b * T, T, t0, acc);
        store_run<VEC>(out + b * T, T, t0, acc);
        return;
    }
    const float c = center[b];
    stage_window<true>(x + b * T, T, tile0 - (L - 1) / 2, n_out + L - 1, c, lds);
    __syncthreads();
    if (t0 >= T) return;
    fir_run<true>(lds, taps, L, acc);
#pragma unroll
    for (int r = 0; r < kRun; ++r) acc[r] = clampf(c + acc[r], lo, hi);
    store_run<VEC>(out + b * T, T, t0, acc);
}

// ---- b. the tap gradient: per-(tile, row) partials ----------------------------------------------------------------------------------

__global__ __launch_bounds__(kWgThreads) void filter_tap_grad_kernel(const float *__restrict__ x, const float *__restrict__ center,
                                                                     const float *__restrict__ row_mask,
                                                                     const float *__restrict__ grad,
                                                                     const float *__restrict__ out_adv, float *__restrict__ part,
                                                                     int64_t T, int L, float lo, float hi) {
    __shared__ float win[kLdsFloats];
    __shared__ float gml[kGmFloats];
    const int64_t b = blockIdx.y, tile0 = (int64_t)blockIdx.x * kTile;
    float *dst = part + (b * gridDim.x + blockIdx.x) * (int64_t)L;
    if (row_mask && row_mask[b] == 0.0f) {  // uniform over the workgroup; zeros, not nothing: the fold reads every slot
        for (int i = threadIdx.x; i < L; i += kWgThreads) dst[i] = 0.0f;
        return;
    }
    const int n_out = T - tile0 < kTile ? (int)(T - tile0) : kTile;
    const int chunks = (n_out + kRun - 1) / kRun, n16 = chunks * kRun;
    const int TL = (L + kRun - 1) / kRun, NS = kWgThreads / TL, CPS = (chunks + NS - 1) / NS;
    // every window position a tap lane reads, the lanes of taps >= L included: finite samples of the row, or zeros
    stage_window<true>(x + b * T, T, tile0 - (L - 1) / 2, n16 + TL * kRun - 1, center[b], win);
    for (int o = threadIdx.x; o < n16; o += kWgThreads) {
        float g = 0.0f;
        if (o < n_out) {
            const float y = out_adv[b * T + tile0 + o];
            if (lo < y && y < hi) g = grad[b * T + tile0 + o];
        }
        gml[pad16(o)] = g;
    }
    __syncthreads();
    const int sg = threadIdx.x / TL, tl = threadIdx.x - sg * TL, j0 = tl * kRun;
    const int c_begin = sg * CPS, c_end = (sg + 1) * CPS < chunks ? (sg + 1) * CPS : chunks;
    float acc[kRun];
#pragma unroll
    for (int r = 0; r < kRun; ++r) acc[r] = 0.0f;
    if (sg < NS && c_begin < c_end) {
        float a[2 * kRun - 1];
#pragma unroll
        for (int m = 0; m < 2 * kRun - 1; ++m) a[m] = win[slot(c_begin * kRun + j0 + m)];
        for (int ch = c_begin; ch < c_end; ++ch) {
            const int o0 = ch * kRun;
            if (ch > c_begin) {  // the window moves up by kRun
#pragma unroll
                for (int m = 0; m < kRun - 1; ++m) a[m] = a[m + kRun];
#pragma unroll
                for (int m = kRun - 1; m < 2 * kRun - 1; ++m) a[m] = win[slot(o0 + j0 + m)];
            }
#pragma unroll
            for (int u = 0; u < kRun; ++u) {
                const float g = gml[pad16(o0 + u)];
#pragma unroll
                for (int r = 0; r < kRun; ++r) acc[r] = fmaf(g, a[r + u], acc[r]);
            }
        }
    }
    __syncthreads();  // every thread has read gm: its LDS now takes the threads' sums, (segment, reversed tap) -> sg TL 16 + j
    if (sg < NS) {
#pragma unroll
        for (int r = 0; r < kRun; ++r) gml[pad16((sg * TL + tl) * kRun + r)] = acc[r];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < L; i += kWgThreads) {
        const int j = L - 1 - i;
        float p = 0.0f;
        for (int s = 0; s < NS; ++s) p = p + gml[pad16(s * TL * kRun + j)];
        dst[i] = p;
    }
}

// ---- c. the fold over tiles, rows and row groups + the Adam step --------------------------------------------------------------------

struct AdamScalars {  // advstep.hip's, for cw_adam_step's arithmetic
    float w1;        // 1 - beta1           (lerp weight)
    float beta2;     // beta2
    float omb2;      // 1 - beta2
    float neg_step;  // -(lr / (1 - beta1^t))
    float bc2_sqrt;  // sqrt(1 - beta2^t)
    float eps;
};

__global__ __launch_bounds__(kUpdateThreads) void filter_tap_update_kernel(const float *__restrict__ part, float *taps, float *am,
                                                                           float *av, float *__restrict__ dh_out, int64_t B, int C,
                                                                           int L, AdamScalars s, int ascend) {
    const int i = blockIdx.x * kUpdateThreads + threadIdx.x;
    if (i >= L) return;  // no barrier below
    float dh = 0.0f;
    for (int64_t g0 = 0; g0 < B; g0 += kGroupRows) {
        const int64_t g1 = g0 + kGroupRows < B ? g0 + kGroupRows : B;
        float P = 0.0f;
        for (int64_t b = g0; b < g1; ++b) {
            const float *row = part + b * C * (int64_t)L + i;
            float r = 0.0f;
#pragma unroll 8
            for (int c = 0; c < C; ++c) r = r + row[(int64_t)c * L];
            P = P + r;
        }
        dh = dh + P;
    }
    if (dh_out) dh_out[i] = dh;
    const float g = ascend ? -dh : dh;
    float h = taps[i], m = am[i], v = av[i];
    m = m + s.w1 * (g - m);
    v = v * s.beta2 + (s.omb2 * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    h = h + s.neg_step * (m / denom);
    taps[i] = h;
    am[i] = m;
    av[i] = v;
}

bool sizes_ok(int64_t B, int64_t T, int64_t L) {
    return B >= 0 && T >= 0 && B <= kMaxGridY && L >= 1 && L <= kMaxTaps && (L & 1) == 1;
}

size_t partial_bytes(int64_t B, int64_t T, int64_t L) {
    return (size_t)B * (size_t)ws_tiles_per_row(T) * (size_t)L * sizeof(float);
}

}  // namespace

extern "C" {

int advstep_filter_apply_f32(const float *x, const float *center, const float *row_mask, const float *taps, float *out, int64_t B,
                             int64_t T, int64_t L, float lo, float hi, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(sizes_ok(B, T, L));
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && center && taps && out);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float);
    if (out == x)
        ADVSTEP_REQUIRE(T <= kTile || L == 1);  // otherwise a tile's halo is what its neighbours' workgroups write
    else
        ADVSTEP_REQUIRE(!overlaps(out, x, rows));
    ADVSTEP_REQUIRE(!overlap2(out, rows, center, per_row) && !overlap2(out, rows, taps, (size_t)L * sizeof(float)));
    ADVSTEP_REQUIRE(!row_mask || !overlap2(out, rows, row_mask, per_row));
    launch_tiles(ROW_KERNEL_PAIR(filter_apply_kernel), rows_vec(T, {x, out}), B, T, as_stream(stream), x, center, row_mask, taps,
                 out, T, (int)L, lo, hi);
    return status_after_launch();
}

size_t advstep_filter_workspace_bytes(int64_t B, int64_t T, int64_t L) {
    if (!sizes_ok(B, T, L) || B == 0 || T == 0) return 0;
    return partial_bytes(B, T, L);
}

int advstep_filter_tap_grad_f32(const float *x, const float *center, const float *row_mask, const float *grad, const float *out_adv,
                                void *partials_ws, size_t ws_bytes, int64_t B, int64_t T, int64_t L, float lo, float hi,
                                advstep_stream_t stream) {
    ADVSTEP_REQUIRE(sizes_ok(B, T, L));
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && center && grad && out_adv);
    const size_t need = partial_bytes(B, T, L);
    if (!partials_ws || ws_bytes < need) return ADVSTEP_EWORKSPACE;
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(partials_ws, need, x, rows) && !overlap2(partials_ws, need, grad, rows) &&
                    !overlap2(partials_ws, need, out_adv, rows) && !overlap2(partials_ws, need, center, per_row));
    ADVSTEP_REQUIRE(!row_mask || !overlap2(partials_ws, need, row_mask, per_row));
    hipLaunchKernelGGL(filter_tap_grad_kernel, row_grid(B, T), dim3(kWgThreads), 0, as_stream(stream), x, center, row_mask, grad,
                       out_adv, static_cast<float *>(partials_ws), T, (int)L, lo, hi);
    return status_after_launch();
}

int advstep_filter_tap_update_f32(const void *partials_ws, float *taps, float *adam_m, float *adam_v, float *dh_out, int64_t B,
                                  int64_t T, int64_t L, int64_t step, double lr, double beta1, double beta2, double adam_eps,
                                  int ascend, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(sizes_ok(B, T, L) && step >= 1);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(partials_ws && taps && adam_m && adam_v);
    const size_t need = partial_bytes(B, T, L), row = (size_t)L * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(taps, adam_m, row) && !overlaps(taps, adam_v, row) && !overlaps(adam_m, adam_v, row));
    ADVSTEP_REQUIRE(!overlap2(partials_ws, need, taps, row) && !overlap2(partials_ws, need, adam_m, row) &&
                    !overlap2(partials_ws, need, adam_v, row));
    ADVSTEP_REQUIRE(!dh_out || (!overlap2(partials_ws, need, dh_out, row) && !overlaps(dh_out, taps, row) &&
                                !overlaps(dh_out, adam_m, row) && !overlaps(dh_out, adam_v, row)));
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    AdamScalars s;
    s.w1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.omb2 = (float)(1.0 - beta2);
    s.neg_step = (float)(-(lr / bc1));
    s.bc2_sqrt = (float)sqrt(bc2);
    s.eps = (float)adam_eps;
    hipLaunchKernelGGL(filter_tap_update_kernel, dim3((unsigned)ceil_div(L, kUpdateThreads)), dim3(kUpdateThreads), 0,
                       as_stream(stream), static_cast<const float *>(partials_ws), taps, adam_m, adam_v, dh_out, B,
                       ws_tiles_per_row(T), (int)L, s, ascend);
    return status_after_launch();
}

}  // extern "C"
