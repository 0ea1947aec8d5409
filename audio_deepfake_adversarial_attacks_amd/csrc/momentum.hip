// momentum.hip — gfx950 (MI355X / CDNA4) kernels of the momentum attacks + the C ABI declared in include/advstep_momentum.h:
// the fused MI-FGSM / NI-FGSM update and the variance-tuning helpers of VMI-FGSM / VNI-FGSM (reference:
// adversarial_attacks/torchattacks/attacks/{mifgsm,nifgsm,vmifgsm,vnifgsm}.py).
//
// The update is two launches over grid = (C tiles of 4096 samples, B rows), 256 threads, 4 float4 per thread and stream:
// the partial sums of |a| per (row, tile) into a float plane of the caller's workspace, then the apply pass, whose every
// workgroup re-reduces the C partials of its row in a fixed order (no atomics: reruns are bit-identical; no workgroup waits
// on another).  The variance-tuning helpers are flat one-pass kernels over the same tiles (the buffer as one row).
// Built with -ffp-contract=off; divisions are IEEE; clamps propagate NaN (see include/advstep.h).
//
// Summation order of mu_b (tests derive their bound from it): a thread adds its 4 quads, each as (|x| + |y|) + (|z| + |w|),
// one after the other (2 + 4 additions deep); a wave adds in 6 xor-shuffle levels; the 4 waves add in 3; the re-reduction adds
// ceil(C / 256) partials per thread, then 6 + 3 again: 24 + ceil(C / 256) additions on the longest chain.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_momentum.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ---- the update ---------------------------------------------------------------------------------------------------------

// pass 1: partial sum of |a| of (row, tile), a = grad (+ v).  Out-of-row lanes load 0.
template <bool VEC, bool HASV>
__global__ __launch_bounds__(kWgThreads) void mi_abs_sum_kernel(const float *__restrict__ grad, const float *__restrict__ v,
                                                                int64_t T, float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y, o = b * T;
    float4 g[kVecs];
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        g[j] = load4<VEC>(grad + o, T, quad_of(tile, j), 0.0f);
        if (HASV) g[j] = add4(g[j], load4<VEC>(v + o, T, quad_of(tile, j), 0.0f));
    }
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) s += (fabsf(g[j].x) + fabsf(g[j].y)) + (fabsf(g[j].z) + fabsf(g[j].w));
    s = wg_sum(s, lds);
    if (threadIdx.x == 0) part[b * C + tile] = s;
}

// pass 2: everything after mu_b.  out may be adv: a thread reads its own samples before it writes them.
template <bool VEC, bool HASV, bool NES>
__global__ __launch_bounds__(kWgThreads) void mi_apply_kernel(const float *adv, const float *__restrict__ grad,
                                                              const float *__restrict__ v, const float *__restrict__ orig,
                                                              float *__restrict__ momentum, float *out,
                                                              float *__restrict__ nes_out, int64_t T, float alpha, float eps,
                                                              float decay, float nes_scale, float lo, float hi,
                                                              float *__restrict__ gmean, const float *__restrict__ part) {
    __shared__ float lds[4];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y, o = b * T;
    float4 a[kVecs], g[kVecs], x[kVecs], m[kVecs];
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {  // issued before the re-reduction's barrier: the loads overlap it
        const int64_t q = quad_of(tile, j);
        g[j] = load4<VEC>(grad + o, T, q, 0.0f);
        if (HASV) g[j] = add4(g[j], load4<VEC>(v + o, T, q, 0.0f));
        m[j] = load4<VEC>(momentum + o, T, q, 0.0f);
        a[j] = load4<VEC>(adv + o, T, q, 0.0f);
        x[j] = load4<VEC>(orig + o, T, q, 0.0f);
    }
    const float mu = row_sum(part + b * C, C, lds) / (float)T;
    if (gmean && tile == 0 && threadIdx.x == 0) gmean[b] = mu;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const int64_t q = quad_of(tile, j);
        float4 nes;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float mm = lane(g[j], k) / mu + lane(m[j], k) * decay;
            const float xx = lane(x[j], k);
            const float x1 = lane(a[j], k) + alpha * sgn(mm);
            const float res = clampf(xx + clampf(x1 - xx, -eps, eps), lo, hi);
            lane(m[j], k) = mm;
            lane(a[j], k) = res;
            if (NES) lane(nes, k) = res + nes_scale * mm;
        }
        store4<VEC>(momentum + o, T, q, m[j]);
        store4<VEC>(out + o, T, q, a[j]);
        if (NES) store4<VEC>(nes_out + o, T, q, nes);
    }
}

// ---- variance tuning: flat kernels, the buffer of n samples as one row of n ----------------------------------------------

struct NeighborNoise {   // out = adv + draw
    __device__ __forceinline__ float4 operator()(float4 a, float4 d, int64_t) const { return add4(a, d); }
};
struct NeighborPhilox {  // out = adv + U(-bound, bound), quad q of the flat buffer = counter q
    float bound;
    uint64_t seed, offset;
    __device__ __forceinline__ float4 operator()(float4 a, float4, int64_t q) const {
        return add4(a, philox_uniform4((uint64_t)q, seed, offset, bound));
    }
};
struct Accumulate {      // gv = gv + g
    __device__ __forceinline__ float4 operator()(float4 gv, float4 g, int64_t) const { return add4(gv, g); }
};
struct Variance {        // v = gv / N - adv_grad
    float N;
    __device__ __forceinline__ float4 operator()(float4 gv, float4 ag, int64_t) const {
        return make_float4(gv.x / N - ag.x, gv.y / N - ag.y, gv.z / N - ag.z, gv.w / N - ag.w);
    }
};

// NIN input streams (in1 unused when NIN == 1); out may be in0 or in1 (elementwise)
template <bool VEC, int NIN, class Op>
__global__ __launch_bounds__(kWgThreads) void flat_kernel(const float *in0, const float *in1, float *out, int64_t n, Op op) {
    const int tile = blockIdx.x;
    float4 a[kVecs], b[kVecs];
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        a[j] = load4<VEC>(in0, n, quad_of(tile, j), 0.0f);
        b[j] = NIN > 1 ? load4<VEC>(in1, n, quad_of(tile, j), 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int j = 0; j < kVecs; ++j) store4<VEC>(out, n, quad_of(tile, j), op(a[j], b[j], quad_of(tile, j)));
}

template <int NIN, class Op>
int launch_flat(const float *in0, const float *in1, float *out, int64_t n, Op op, hipStream_t st) {
    // the buffer as one row of n samples: grid = (tiles, 1)
    launch_tiles(ROW_KERNEL_PAIR(flat_kernel, NIN, Op), rows_vec(n, {in0, in1, out}), 1, n, st, in0, in1, out, n, op);
    return status_after_launch();
}

constexpr int64_t kMaxFlat = (int64_t)0x7fffffff * kWsRowTile;  // grid.x is 31 bits of tiles

}  // namespace

extern "C" {

int advstep_mi_step_f32(const float *adv, const float *grad, const float *v, const float *orig, float *momentum, float *out,
                        float *nes_out, int64_t B, int64_t T, float alpha, float eps, float decay, float nes_scale, float lo,
                        float hi, float *gmean, void *ws, size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && grad && orig && momentum && out);
    const size_t bytes = (size_t)B * T * sizeof(float);
    for (const float *r : {adv, grad, v, orig}) {
        if (!r) continue;
        ADVSTEP_REQUIRE(!overlaps(momentum, r, bytes));
        ADVSTEP_REQUIRE(!nes_out || !overlaps(nes_out, r, bytes));
        ADVSTEP_REQUIRE(r == adv ? (out == adv || !overlaps(out, adv, bytes)) : !overlaps(out, r, bytes));
    }
    ADVSTEP_REQUIRE(!overlaps(out, momentum, bytes));
    ADVSTEP_REQUIRE(!nes_out || (!overlaps(nes_out, momentum, bytes) && !overlaps(nes_out, out, bytes)));
    RowWs w;
    if (!carve_ws(ws, ws_bytes, B, T, &w)) return ADVSTEP_EWORKSPACE;
    hipStream_t st = as_stream(stream);
    const bool vec = rows_vec(T, {adv, grad, v, orig, momentum, out, nes_out});
    // [v given] and [v given][nes_out given]
    static constexpr decltype(&mi_abs_sum_kernel<true, true>) abs_sum[2][2] = {ROW_KERNEL_PAIR(mi_abs_sum_kernel, false),
                                                                               ROW_KERNEL_PAIR(mi_abs_sum_kernel, true)};
    static constexpr decltype(&mi_apply_kernel<true, true, true>) apply[2][2][2] = {
        {ROW_KERNEL_PAIR(mi_apply_kernel, false, false), ROW_KERNEL_PAIR(mi_apply_kernel, false, true)},
        {ROW_KERNEL_PAIR(mi_apply_kernel, true, false), ROW_KERNEL_PAIR(mi_apply_kernel, true, true)}};
    launch_tiles(abs_sum[v != nullptr], vec, B, T, st, grad, v, T, w.p0);
    launch_tiles(apply[v != nullptr][nes_out != nullptr], vec, B, T, st, adv, grad, v, orig, momentum, out, nes_out, T, alpha, eps,
                 decay, nes_scale, lo, hi, gmean, w.p0);
    return status_after_launch();
}

int advstep_vt_neighbor_noise_f32(const float *adv, const float *draw, float *out, int64_t n, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0 && n <= kMaxFlat);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && draw && out);
    return launch_flat<2>(adv, draw, out, n, NeighborNoise{}, as_stream(stream));
}

int advstep_vt_neighbor_philox_f32(const float *adv, float *out, int64_t n, float bound, uint64_t seed, uint64_t offset,
                                   advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0 && n <= kMaxFlat);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && out);
    return launch_flat<1>(adv, nullptr, out, n, NeighborPhilox{bound, seed, offset}, as_stream(stream));
}

int advstep_vt_accumulate_f32(float *gv, const float *g, int64_t n, int first, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0 && n <= kMaxFlat);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(gv && g && gv != g);
    // first: gv = 0 + g, which is g (a -0 in g becomes +0, as adding it to the reference's zero-filled accumulator does)
    if (first) return launch_flat<1>(g, nullptr, gv, n, Accumulate{}, as_stream(stream));
    return launch_flat<2>(gv, g, gv, n, Accumulate{}, as_stream(stream));
}

int advstep_vt_variance_f32(const float *gv, const float *adv_grad, float *v, int64_t n, int64_t N, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0 && n <= kMaxFlat && N >= 1);
    if (n == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(gv && adv_grad && v);
    return launch_flat<2>(gv, adv_grad, v, n, Variance{(float)N}, as_stream(stream));
}

}  // extern "C"
