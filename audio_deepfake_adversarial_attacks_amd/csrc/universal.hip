// universal.hip — gfx950 (MI355X / CDNA4) kernels of the universal perturbation (torchattacks.UniversalPGD) + the C ABI declared
// in include/advstep_universal.h: the column sum of a batch of gradients, (B, T) -> (T), and the broadcast of one delta over a
// batch.  The update of delta itself is advstep.hip's PGD step on a (1, T) row (the header says why).
//
// The column sum is the library's only reduction ACROSS rows.  A thread owns 4 adjacent columns (quad q of every row) and adds
// down the rows, so there is no cross-lane step, no LDS and no barrier; a grid over column tiles alone would be 64 workgroups at
// T = 64 600, so the rows are cut into groups of kGroupRows and grid = (column tile, row group): 512 workgroups at B = 128, each
// thread with kGroupRows independent 16-byte loads in flight.  Group g leaves its partial in plane g of the workspace and a
// second launch folds the planes in order; with one group the first launch writes `out` itself.  The order of a column's
// additions is fixed by (B, T) — rows in order inside a group, groups in order — and is the same in the float4 and in the
// sample-by-sample path, so the two give the same bits.
//
// Built with -ffp-contract=off: w * g rounds before it is added.  Clamps propagate NaN (include/advstep.h).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_universal.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

constexpr int kGroupRows = ADVSTEP_UNIVERSAL_GROUP_ROWS;  // R: rows per group = loads a thread has in flight
constexpr int64_t kColTile = kWgThreads * 4;              // columns per workgroup: one quad per thread

inline int64_t row_groups(int64_t B) { return ceil_div(B, kGroupRows); }
inline int64_t plane_floats(int64_t T) { return ceil_div(T, 4) * 4; }  // every plane starts 16-byte aligned
inline size_t colsum_ws_bytes(int64_t B, int64_t T) {
    return row_groups(B) > 1 ? (size_t)row_groups(B) * (size_t)plane_floats(T) * sizeof(float) : 0;
}

__device__ __forceinline__ float4 add_scaled4(float4 acc, float w, float4 v) {
    return make_float4(acc.x + w * v.x, acc.y + w * v.y, acc.z + w * v.z, acc.w + w * v.w);
}

// ---- a. the column sum ----------------------------------------------------------------------------------------------------------

// Group blockIdx.y's partial of quad q: dst + blockIdx.y * dst_stride (a workspace plane, or `out` when there is one group).
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void colsum_group_kernel(const float *__restrict__ grad,
                                                                  const float *__restrict__ row_weight, float *__restrict__ dst,
                                                                  int64_t dst_stride, int64_t B, int64_t T) {
    const int64_t q = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (q * 4 >= T) return;  // no barrier below: a thread without a column leaves
    const int64_t b0 = (int64_t)blockIdx.y * kGroupRows;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (b0 + kGroupRows <= B) {
        float4 v[kGroupRows];
#pragma unroll
        for (int k = 0; k < kGroupRows; ++k) v[k] = load4<VEC>(grad + (b0 + k) * T, T, q, 0.0f);
#pragma unroll
        for (int k = 0; k < kGroupRows; ++k) acc = add_scaled4(acc, row_weight ? row_weight[b0 + k] : 1.0f, v[k]);
    } else {  // the last, partial group: the same order, row by row
#pragma unroll 4
        for (int64_t b = b0; b < B; ++b) acc = add_scaled4(acc, row_weight ? row_weight[b] : 1.0f, load4<VEC>(grad + b * T, T, q, 0.0f));
    }
    store4<VEC>(dst + (int64_t)blockIdx.y * dst_stride, T, q, acc);
}

// out = ((0 + P_0) + P_1) + ... over the G planes.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void colsum_fold_kernel(const float *__restrict__ planes, int64_t stride, int64_t G,
                                                                 float *__restrict__ out, int64_t T) {
    const int64_t q = (int64_t)blockIdx.x * kWgThreads + threadIdx.x;
    if (q * 4 >= T) return;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 8
    for (int64_t g = 0; g < G; ++g) acc = add_scaled4(acc, 1.0f, load4<VEC>(planes + g * stride, T, q, 0.0f));
    store4<VEC>(out, T, q, acc);
}

// ---- b. the broadcast ---------------------------------------------------------------------------------------------------------------

// out may be x: a thread reads its own samples before it writes them.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void universal_apply_kernel(const float *x, const float *__restrict__ delta,
                                                                     const float *__restrict__ row_weight, float *out, int64_t T,
                                                                     float lo, float hi) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y, o = b * T;
    float4 a[kVecs], d[kVecs];
    load_tile<VEC>(x + o, T, tile, 0.0f, a);
    load_tile<VEC>(delta, T, tile, 0.0f, d);  // delta is a row of its own
    const float w = row_weight ? row_weight[b] : 1.0f;  // uniform over the workgroup
#pragma unroll
    for (int j = 0; j < kVecs; ++j) {
        a[j].x = clampf(a[j].x + w * d[j].x, lo, hi);
        a[j].y = clampf(a[j].y + w * d[j].y, lo, hi);
        a[j].z = clampf(a[j].z + w * d[j].z, lo, hi);
        a[j].w = clampf(a[j].w + w * d[j].w, lo, hi);
    }
    store_tile<VEC>(out + o, T, tile, a);
}

}  // namespace

extern "C" {

size_t advstep_universal_workspace_bytes(int64_t B, int64_t T) {
    if (B <= 0 || T <= 0) return 0;
    return colsum_ws_bytes(B, T);
}

int advstep_universal_colsum_f32(const float *grad, const float *row_weight, float *out, int64_t B, int64_t T, void *ws,
                                 size_t ws_bytes, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(grad && out);
    const size_t rows = (size_t)B * T * sizeof(float), row = (size_t)T * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(out, row, grad, rows));
    ADVSTEP_REQUIRE(!row_weight || !overlap2(out, row, row_weight, (size_t)B * sizeof(float)));
    const int64_t G = row_groups(B);
    const size_t need = colsum_ws_bytes(B, T);
    if (G > 1) {
        if (!ws || !aligned16(ws) || ws_bytes < need) return ADVSTEP_EWORKSPACE;
        ADVSTEP_REQUIRE(!overlap2(ws, need, out, row) && !overlap2(ws, need, grad, rows));
        ADVSTEP_REQUIRE(!row_weight || !overlap2(ws, need, row_weight, (size_t)B * sizeof(float)));
    }
    hipStream_t st = as_stream(stream);
    float *dst = G > 1 ? static_cast<float *>(ws) : out;
    const int64_t stride = plane_floats(T);
    const dim3 cols((unsigned)ceil_div(T, kColTile));
    void (*const group[2])(const float *, const float *, float *, int64_t, int64_t, int64_t) = ROW_KERNEL_PAIR(colsum_group_kernel);
    hipLaunchKernelGGL(group[rows_vec(T, {grad, dst})], dim3(cols.x, (unsigned)G), dim3(kWgThreads), 0, st, grad, row_weight, dst,
                       stride, B, T);
    if (G > 1) {
        void (*const fold[2])(const float *, int64_t, int64_t, float *, int64_t) = ROW_KERNEL_PAIR(colsum_fold_kernel);
        hipLaunchKernelGGL(fold[rows_vec(T, {dst, out})], cols, dim3(kWgThreads), 0, st, (const float *)dst, stride, G, out, T);
    }
    return status_after_launch();
}

int advstep_universal_apply_f32(const float *x, const float *delta, const float *row_weight, float *out, int64_t B, int64_t T,
                                float lo, float hi, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(x && delta && out);
    const size_t rows = (size_t)B * T * sizeof(float), row = (size_t)T * sizeof(float);
    ADVSTEP_REQUIRE(out == x || !overlaps(out, x, rows));
    ADVSTEP_REQUIRE(!overlap2(out, rows, delta, row));
    ADVSTEP_REQUIRE(!row_weight || !overlap2(out, rows, row_weight, (size_t)B * sizeof(float)));
    launch_tiles(ROW_KERNEL_PAIR(universal_apply_kernel), rows_vec(T, {x, delta, out}), B, T, as_stream(stream), x, delta,
                 row_weight, out, T, lo, hi);
    return status_after_launch();
}

}  // extern "C"
