// spsa.hip — gfx950 (MI355X / CDNA4) kernels of the score-based black-box attack (torchattacks.SPSA) + the C ABI declared in
// include/advstep_spsa.h: the fill of an iteration's probe slots and the sign step along the estimated gradient.
//
// Both are row-independent streaming passes on the (4096-sample tile, row) grid of row_tiles.h.  The Rademacher directions are
// regenerated from Philox in both kernels and never stored: one call per quad of samples carries 32 directions (bit
// 4 * (j & 31) + k of its 128 bits is direction j's sign at sample k of the quad; the header fixes the mapping).  The probe kernel
// keeps a thread's samples of adv in registers and loops over the slots, so it reads 4 B and writes 4 * ns B per sample; the step
// kernel adds +-d_j into 16 accumulators per thread and hands them to the PGD L-inf step's own device function, so the estimated
// gradient never exists in memory: 12 B per sample.  A row's logits and label are uniform over its workgroups: scalar loads.
//
// Built with -ffp-contract=off.  Clamps propagate NaN (include/advstep.h).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_spsa.h"
#include "advstep_common.h"
#include "direction_bits.h"
#include "row_tiles.h"

namespace {

constexpr int64_t kMaxDirections = ADVSTEP_SPSA_MAX_DIRECTIONS;

// direction_bits / direction_nibble / signed_by: direction_bits.h (hsj.hip draws the same directions)

// ---- a. the probe slots ---------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void spsa_probe_kernel(const float *__restrict__ adv, float *__restrict__ out, int64_t B,
                                                                int64_t T, int s0, int ns, float delta, float lo, float hi,
                                                                uint64_t seed, uint64_t offset) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    float4 a[kVecs];
    load_tile<VEC>(adv + b * T, T, tile, 0.0f, a);
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
        const int64_t q = quad_of(tile, v);
        if (!in_row(T, q, 0)) continue;  // no barrier in this kernel
        Quad r = {};
        int call = -1;
        for (int s = s0; s < s0 + ns; ++s) {
            float4 o = a[v];  // slot 0: adv's bytes
            if (s > 0) {
                const int j = (s - 1) >> 1;
                if ((j >> 5) != call) {
                    call = j >> 5;
                    r = direction_bits(q, b, seed, offset, call);
                }
                const uint32_t nib = direction_nibble(r, j);
                const float m = (s & 1) ? delta : -delta;  // slot 1 + 2j adds delta * v, slot 2 + 2j subtracts it
                o.x = clampf(a[v].x + signed_by(m, nib, 0), lo, hi);
                o.y = clampf(a[v].y + signed_by(m, nib, 1), lo, hi);
                o.z = clampf(a[v].z + signed_by(m, nib, 2), lo, hi);
                o.w = clampf(a[v].w + signed_by(m, nib, 3), lo, hi);
            }
            store4<VEC>(out + ((int64_t)(s - s0) * B + b) * T, T, q, o);
        }
    }
}

// ---- b. the step ------------------------------------------------------------------------------------------------------------------

// out may be adv: a thread reads its own samples before it writes them.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void spsa_step_kernel(const float *adv, const float *__restrict__ orig,
                                                               const float *__restrict__ z, const int64_t *__restrict__ labels,
                                                               int32_t *__restrict__ queries, float *out, int64_t B, int64_t T,
                                                               int n, float alpha, float eps, float lo, float hi, uint64_t seed,
                                                               uint64_t offset) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y, o = b * T;
    float4 a[kVecs];
    load_tile<VEC>(adv + o, T, tile, 0.0f, a);
    const bool is_one = labels[b] == 1;
    if ((z[b] > 0.0f) != is_one) {  // fooled (uniform over the row): the row as it is, no query counted
        if (out != adv) store_tile<VEC>(out + o, T, tile, a);
        return;
    }
    float4 x[kVecs], g[kVecs];
    load_tile<VEC>(orig + o, T, tile, 0.0f, x);
#pragma unroll
    for (int v = 0; v < kVecs; ++v) g[v] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int c = 0; c * 32 < n; ++c) {
        Quad r[kVecs];
#pragma unroll
        for (int v = 0; v < kVecs; ++v) r[v] = direction_bits(quad_of(tile, v), b, seed, offset, c);
        const int j1 = (c + 1) * 32 < n ? (c + 1) * 32 : n;
        for (int j = c * 32; j < j1; ++j) {
            const float diff = z[(int64_t)(1 + 2 * j) * B + b] - z[(int64_t)(2 + 2 * j) * B + b];
            const float d = is_one ? -diff : diff;
#pragma unroll
            for (int v = 0; v < kVecs; ++v) {
                const uint32_t nib = direction_nibble(r[v], j);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float t = signed_by(d, nib, k);
                    lane(g[v], k) = j == 0 ? t : lane(g[v], k) + t;  // g = ((+-d_0) +- d_1) +- ...
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) lane(a[v], k) = pgd_linf_elem(lane(a[v], k), lane(g[v], k), lane(x[v], k), alpha, eps, lo, hi);
    }
    store_tile<VEC>(out + o, T, tile, a);
    if (tile == 0 && threadIdx.x == 0) queries[b] += 1 + 2 * n;
}

}  // namespace

extern "C" {

int advstep_spsa_probe_f32(const float *adv, float *out, int64_t B, int64_t T, int64_t s0, int64_t ns, float delta, float lo,
                           float hi, uint64_t seed, uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(s0 >= 0 && ns >= 0 && s0 <= 1 + 2 * kMaxDirections && ns <= 1 + 2 * kMaxDirections - s0);
    if (B == 0 || T == 0 || ns == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && out);
    const size_t rows = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(out, (size_t)ns * rows, adv, rows));
    launch_tiles(ROW_KERNEL_PAIR(spsa_probe_kernel), rows_vec(T, {adv, out}), B, T, as_stream(stream), adv, out, B, T, (int)s0,
                 (int)ns, delta, lo, hi, seed, offset);
    return status_after_launch();
}

int advstep_spsa_step_f32(const float *adv, const float *orig, const float *z, const int64_t *labels, int32_t *queries, float *out,
                          int64_t B, int64_t T, int64_t n, float alpha, float eps, float lo, float hi, uint64_t seed,
                          uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(n >= 0 && n <= kMaxDirections);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && orig && z && labels && queries && out);
    const size_t rows = (size_t)B * T * sizeof(float), zs = (size_t)(1 + 2 * n) * B * sizeof(float);
    ADVSTEP_REQUIRE(out == adv || !overlaps(out, adv, rows));
    ADVSTEP_REQUIRE(!overlaps(out, orig, rows) && !overlap2(out, rows, z, zs));
    ADVSTEP_REQUIRE(!overlap2(out, rows, labels, (size_t)B * sizeof(int64_t)));
    ADVSTEP_REQUIRE(!overlap2(out, rows, queries, (size_t)B * sizeof(int32_t)));
    ADVSTEP_REQUIRE(!overlap2(queries, (size_t)B * sizeof(int32_t), adv, rows));
    ADVSTEP_REQUIRE(!overlap2(queries, (size_t)B * sizeof(int32_t), orig, rows));
    ADVSTEP_REQUIRE(!overlap2(queries, (size_t)B * sizeof(int32_t), z, zs));
    ADVSTEP_REQUIRE(!overlap2(queries, (size_t)B * sizeof(int32_t), labels, (size_t)B * sizeof(int64_t)));
    launch_tiles(ROW_KERNEL_PAIR(spsa_step_kernel), rows_vec(T, {adv, orig, out}), B, T, as_stream(stream), adv, orig, z, labels,
                 queries, out, B, T, (int)n, alpha, eps, lo, hi, seed, offset);
    return status_after_launch();
}

}  // extern "C"
