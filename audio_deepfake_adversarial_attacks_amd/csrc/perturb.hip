// perturb.hip — gfx950 (MI355X / CDNA4) kernels of the per-utterance perturbation report + the C ABI declared in
// include/advstep_perturb.h: L-inf, mean L1, L2, signal energy, SNR and segmental SNR of adv - x per row.
//
// Two launches.  The first runs on the (tile, row) grid of row_tiles.h: a workgroup loads its 4096-sample tile of x and of adv
// once (8 B per sample) and writes five float partials — sum x^2, sum d^2, sum |d|, max |d|, sum of the clamped segment SNRs —
// into the caller's workspace, plane p at ws[p * B * C + b * C + tile].  The second is one workgroup per row that re-reduces
// the C partials of each plane in the fixed order of row_sum / row_max and writes the six values.  No atomics, no workgroup
// waits on another, no host synchronisation: reruns are bit-identical and the pair may be captured into a graph.
//
// The segment of the segmental SNR is 256 samples (16 ms at 16 kHz) because that is what one wavefront loads for one j of a
// tile: quad_of(tile, j) = tile * 1024 + j * 256 + threadIdx.x gives the 64 lanes of wave w the 64 consecutive float4 of
// samples [256 s, 256 s + 256), s = tile * 16 + j * 4 + w, in the float4 path and in the sample-by-sample path alike.  A
// segment's two energies are therefore four products per lane plus one wave_reduce each; no segment straddles a wave, a tile
// or a workgroup.
//
// Built with -ffp-contract=off; division and sqrt are IEEE, log10f is the device library's.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_perturb.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

constexpr int kSegment = 256;                   // samples per segment of the segmental SNR
constexpr float kSegLoDb = -10.0f, kSegHiDb = 35.0f;
constexpr int kPlanes = 5;                      // workspace planes, in this order:
enum { kEx = 0, kEd = 1, kL1 = 2, kMax = 3, kSeg = 4 };

static_assert(64 * 4 == kSegment, "a segment is one wavefront's float4 load: 64 lanes of 4 samples");
static_assert(kWgThreads % 64 == 0 && (kWgThreads * 4) % kSegment == 0, "one j of a tile is a whole number of segments");
static_assert(kWsRowTile % kSegment == 0, "no segment straddles a tile");

// 10 log10(ex / ed): +inf for ed == 0 < ex, -inf for ex == 0 < ed, NaN for 0 / 0 and for NaN
__device__ __forceinline__ float ratio_db(float ex, float ed) { return 10.0f * log10f(ex / ed); }

// One segment's term: 35 when nothing moved (also in silence), else the ratio clamped to [-10, 35]; NaN propagates (a NaN in x
// makes d NaN, so ed == 0 implies that ex is a number).
__device__ __forceinline__ float segment_db(float ex, float ed) {
    return ed == 0.0f ? kSegHiDb : clampf(ratio_db(ex, ed), kSegLoDb, kSegHiDb);
}

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void perturb_partials_kernel(const float *__restrict__ x,
                                                                      const float *__restrict__ adv, int64_t T,
                                                                      float *__restrict__ part, int64_t plane) {
    __shared__ float lds[4 * kPlanes];
    const int tile = blockIdx.x, C = gridDim.x;
    const int64_t b = blockIdx.y;
    const int lane_id = threadIdx.x & 63;
    float4 rx[kVecs], ra[kVecs];
    load_tile<VEC>(x + b * T, T, tile, 0.0f, rx);   // out-of-row samples: x = adv = 0, so d = 0 is neutral for all five
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, ra);
    float ex = 0.0f, ed = 0.0f, l1 = 0.0f, mx = 0.0f, seg = 0.0f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        const float4 v = rx[j];
        const float4 d = make_float4(ra[j].x - v.x, ra[j].y - v.y, ra[j].z - v.z, ra[j].w - v.w);
        const float ex_j = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        const float ed_j = (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        ex += ex_j;
        ed += ed_j;
        l1 += (fabsf(d.x) + fabsf(d.y)) + (fabsf(d.z) + fabsf(d.w));
        mx = max_nan(mx, max_nan(max_nan(fabsf(d.x), fabsf(d.y)), max_nan(fabsf(d.z), fabsf(d.w))));
        // this wave's segment of this j: full when the last sample of the wave's last quad is inside the row (wave-uniform)
        const float sx = wave_reduce(ex_j, SumOp()), sd = wave_reduce(ed_j, SumOp());
        if (in_row(T, quad_of(tile, j) - lane_id + 63, 3)) seg += segment_db(sx, sd);
    }
    ex = wg_sum(ex, lds + 4 * kEx);
    ed = wg_sum(ed, lds + 4 * kEd);
    l1 = wg_sum(l1, lds + 4 * kL1);
    mx = wg_max_nan(mx, lds + 4 * kMax);
    seg = wg_sum(lane_id == 0 ? seg : 0.0f, lds + 4 * kSeg);  // every lane of a wave holds the wave's sum: count it once
    if (threadIdx.x == 0) {
        const int64_t i = b * C + tile;
        part[kEx * plane + i] = ex;
        part[kEd * plane + i] = ed;
        part[kL1 * plane + i] = l1;
        part[kMax * plane + i] = mx;
        part[kSeg * plane + i] = seg;
    }
}

// One workgroup per row.  C == 0 (T == 0) reads nothing: the sums are empty and there is no first partial to take a max from.
__global__ __launch_bounds__(kWgThreads) void perturb_finish_kernel(const float *__restrict__ part, int64_t plane, int C,
                                                                    int64_t T, float *__restrict__ stats) {
    __shared__ float lds[4 * kPlanes];
    const int64_t b = blockIdx.x, B = gridDim.x;
    const float *p = part + b * C;
    const float ex = row_sum(p + kEx * plane, C, lds + 4 * kEx);
    const float ed = row_sum(p + kEd * plane, C, lds + 4 * kEd);
    const float l1 = row_sum(p + kL1 * plane, C, lds + 4 * kL1);
    const float mx = C > 0 ? row_max(p + kMax * plane, C, lds + 4 * kMax) : 0.0f;
    const float seg = row_sum(p + kSeg * plane, C, lds + 4 * kSeg);
    if (threadIdx.x != 0) return;
    const int64_t S = T / kSegment;
    stats[0 * B + b] = mx;
    stats[1 * B + b] = l1 / (float)T;
    stats[2 * B + b] = sqrtf(ed);
    stats[3 * B + b] = ex;
    stats[4 * B + b] = ratio_db(ex, ed);
    stats[5 * B + b] = S > 0 ? seg / (float)S : NAN;
}

inline size_t plane_floats(int64_t B, int64_t T) { return (size_t)B * (size_t)ws_tiles_per_row(T); }

// [a, a + a_bytes) and [b, b + b_bytes) share a byte (advstep_common.h's overlaps is for two ranges of one size)
inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + b_bytes && q < p + a_bytes;
}

}  // namespace

extern "C" size_t advstep_perturb_stats_workspace_bytes(int64_t B, int64_t T) {
    if (B <= 0 || T <= 0) return 0;
    return align16(kPlanes * plane_floats(B, T) * sizeof(float));
}

extern "C" int advstep_perturb_stats_f32(const float *x, const float *adv, float *stats, void *ws, size_t ws_bytes, int64_t B,
                                         int64_t T, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(stats);
    hipStream_t st = as_stream(stream);
    const int C = ws_tiles_per_row(T);
    const int64_t plane = (int64_t)plane_floats(B, T);
    if (T > 0) {
        ADVSTEP_REQUIRE(x && adv && ws);
        const size_t need = advstep_perturb_stats_workspace_bytes(B, T);
        const size_t rows = (size_t)B * T * sizeof(float), out = (size_t)6 * B * sizeof(float);
        ADVSTEP_REQUIRE(!ranges_overlap(stats, out, x, rows) && !ranges_overlap(stats, out, adv, rows));
        ADVSTEP_REQUIRE(!ranges_overlap(ws, need, x, rows) && !ranges_overlap(ws, need, adv, rows));
        ADVSTEP_REQUIRE(!ranges_overlap(ws, need, stats, out));
        if (!aligned16(ws) || ws_bytes < need) return ADVSTEP_EWORKSPACE;
        float *part = static_cast<float *>(ws);
        launch_tiles(ROW_KERNEL_PAIR(perturb_partials_kernel), rows_vec(T, {x, adv}), B, T, st, x, adv, T, part, plane);
    }
    hipLaunchKernelGGL(perturb_finish_kernel, dim3((unsigned)B), dim3(kWgThreads), 0, st, (const float *)ws, plane, C, T, stats);
    return status_after_launch();
}
