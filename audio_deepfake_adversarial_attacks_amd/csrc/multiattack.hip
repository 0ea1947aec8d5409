// multiattack.hip — gfx950 (MI355X / CDNA4) kernels of the MultiAttack row router + the C ABI declared in
// include/advstep_multi.h (reference: adversarial_attacks/torchattacks/attacks/multiattack.py:55-66).
//
// One stage is two launches.  The select is one wave: an ordered ballot compaction (as qual_select_kernel, wave_prep.hip) that
// judges every row and writes its destination into the caller's int32 scratch — the row of `final` for a wrong row, ~k for the
// k-th kept row — together with next_y, next_rows and the two counts.  The copy pass runs on the (tile, row) grid of
// row_tiles.h: a workgroup reads its row's destination and moves one 4096-sample tile, adv -> final or x -> next_x, so every
// sample is read once and written once (8 B per sample).  No atomics, no workgroup waits on another, and nothing but copies:
// reruns are bit-identical.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_multi.h"
#include "advstep_common.h"
#include "row_tiles.h"

namespace {

constexpr int32_t kSkip = INT32_MIN;  // a wrong row whose index is outside [0, B): counted, never copied

__global__ __launch_bounds__(64) void multi_select_kernel(const float *__restrict__ z, const int64_t *__restrict__ labels,
                                                          const int32_t *__restrict__ rows, int64_t n, int64_t B,
                                                          int32_t *__restrict__ dest, int64_t *__restrict__ next_y,
                                                          int32_t *__restrict__ next_rows, int32_t *__restrict__ counts) {
    const int lane = threadIdx.x;
    int32_t wrongs = 0, kept = 0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t i = base + lane;
        bool wrong = false, keep = false;
        int64_t y = 0;
        int32_t r = 0;
        if (i < n) {
            y = labels[i];
            r = rows[i];
            wrong = (int64_t)(z[i] > 0.0f) != y;  // torch.max(cat([-z, z], 1), 1): the first maximal index
            keep = !wrong;
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long mw = __ballot(wrong), mk = __ballot(keep);
        if (wrong) dest[i] = (r >= 0 && r < B) ? r : kSkip;
        if (keep) {
            const int32_t k = kept + __popcll(mk & below);
            dest[i] = ~k;
            next_y[k] = y;
            next_rows[k] = r;
        }
        wrongs += __popcll(mw);
        kept += __popcll(mk);
    }
    if (lane == 0) {
        counts[0] = wrongs;
        counts[1] = kept;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void multi_copy_kernel(const float *__restrict__ adv, const float *__restrict__ x,
                                                                const int32_t *__restrict__ dest,
                                                                float *__restrict__ final_rows, float *__restrict__ next_x,
                                                                int64_t T) {
    const int tile = blockIdx.x;
    const int64_t i = blockIdx.y;
    const int32_t d = dest[i];  // uniform over the workgroup
    if (d == kSkip) return;
    const float *src = (d >= 0 ? adv : x) + i * T;
    float *dst = d >= 0 ? final_rows + (int64_t)d * T : next_x + (int64_t)(~d) * T;
    float4 r[kVecs];
    load_tile<VEC>(src, T, tile, 0.0f, r);
    store_tile<VEC>(dst, T, tile, r);
}

}  // namespace

extern "C" int advstep_multi_route_f32(const float *adv, const float *x, const float *z, const int64_t *labels,
                                       const int32_t *rows, float *final_rows, float *next_x, int64_t *next_y,
                                       int32_t *next_rows, int32_t *counts, int32_t *scratch, int64_t n, int64_t B, int64_t T,
                                       advstep_stream_t stream) {
    ADVSTEP_REQUIRE(n >= 0 && B >= 0 && T >= 0 && n <= kMaxGridY && B >= n && B <= INT32_MAX);
    if (n == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && x && z && labels && rows && final_rows && next_x && next_y && next_rows && counts && scratch);
    const size_t sub = (size_t)n * T * sizeof(float), full = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(next_x, sub, x, sub) && !overlap2(next_x, sub, adv, sub) && !overlap2(next_x, sub, final_rows, full));
    ADVSTEP_REQUIRE(!overlap2(final_rows, full, adv, sub) && !overlap2(final_rows, full, x, sub));
    ADVSTEP_REQUIRE(!overlaps(next_y, labels, (size_t)n * sizeof(int64_t)) && !overlaps(next_rows, rows, (size_t)n * sizeof(int32_t)));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(multi_select_kernel, dim3(1), dim3(64), 0, st, z, labels, rows, n, B, scratch, next_y, next_rows, counts);
    launch_tiles(ROW_KERNEL_PAIR(multi_copy_kernel), rows_vec(T, {adv, x, final_rows, next_x}), n, T, st, adv, x, scratch, final_rows,
                 next_x, T);
    return status_after_launch();
}
