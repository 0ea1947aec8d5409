// hsj.hip — gfx950 (MI355X / CDNA4) kernels of the label-only black-box attack (torchattacks.HopSkipJump) + the C ABI declared in
// include/advstep_hsj.h: the per-row bisection towards the decision boundary, the probe slots of a normal estimate, the candidate
// steps along the estimated normal's sign, and the choice among them.
//
// All are row-independent passes on the (4096-sample tile, row) grid of row_tiles.h.  A row's state, logits, label and flags are
// uniform over its workgroups: scalar loads.  The Rademacher directions are direction_bits.h's (SPSA's), regenerated and never
// stored.  The search, probe and take kernels are HBM-bound streaming passes.  The candidates kernel is bound by the vector ALUs
// at n of a few hundred: per quad and 32 directions one Philox call (~100 instructions), and per sample and 8 directions two
// v_and_b32 and two accumulating v_bcnt_u32_b32 against two row-uniform masks (the adversarial and the other decisions, one bit
// per direction at the positions of sample 0, shifted by the sample's index in its quad on the scalar unit).  The counts are
// integers, so the step direction does not depend on any order of summation.
//
// Built with -ffp-contract=off.  Clamps propagate NaN (include/advstep.h).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_hsj.h"
#include "advstep_common.h"
#include "direction_bits.h"
#include "row_tiles.h"

namespace {

constexpr int64_t kMaxDirections = ADVSTEP_HSJ_MAX_DIRECTIONS;
constexpr int64_t kMaxTrials = ADVSTEP_HSJ_MAX_TRIALS;
constexpr int kMaskWords = (int)(kMaxDirections / 8);  // 8 directions per Philox word

// SPSA's rule: +-0 and NaN are class 0.
__device__ __forceinline__ bool adversarial(float z, bool is_one) { return (z > 0.0f) != is_one; }

// point(r) of one sample.
__device__ __forceinline__ float point_elem(float c, float x, float r, float lo, float hi) {
    return clampf(x + clampf(c - x, -r, r), lo, hi);
}

// ---- a. the boundary search ---------------------------------------------------------------------------------------------------

enum SearchMode { kOpen = 0, kNext = 1, kClose = 2 };

// out may be cur in kClose only: a thread reads its own samples before it writes them.
template <bool VEC, int MODE>
__global__ __launch_bounds__(kWgThreads) void hsj_search_kernel(const float *cur, const float *__restrict__ orig,
                                                                const float *__restrict__ z, const int64_t *__restrict__ labels,
                                                                const float *__restrict__ dist, const int32_t *__restrict__ active,
                                                                const float *__restrict__ state, float *__restrict__ state_out,
                                                                int32_t *__restrict__ queries, int rounds, float *out, int64_t B,
                                                                int64_t T, float lo, float hi) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y, o = b * T;
    const bool lead = tile == 0 && threadIdx.x == 0;
    float4 c[kVecs];
    if (active[b] == 0) {  // uniform over the row: its bytes, every plane its dist, no query
        if (MODE != kClose && lead) {
#pragma unroll
            for (int p = 0; p < 4; ++p) state_out[p * B + b] = MODE == kOpen ? dist[b] : state[p * B + b];
        }
        if (out == cur) return;
        load_tile<VEC>(cur + o, T, tile, 0.0f, c);
        store_tile<VEC>(out + o, T, tile, c);
        return;
    }
    float blo, bhi, d0;
    if (MODE == kOpen) {
        blo = 0.0f;
        bhi = d0 = dist[b];
    } else {
        blo = state[0 * B + b];
        bhi = state[1 * B + b];
        d0 = state[3 * B + b];
        const float mid = state[2 * B + b];
        if (adversarial(z[b], labels[b] == 1)) bhi = mid;
        else blo = mid;
    }
    float r;
    bool move = true;
    if (MODE == kClose) {
        r = bhi;
        move = bhi < d0;  // hi was judged adversarial; hi == dist0 (or a NaN) keeps cur's bytes
        if (lead) queries[b] += rounds;
    } else {
        r = (blo + bhi) * 0.5f;
        if (lead) {
            state_out[0 * B + b] = blo;
            state_out[1 * B + b] = bhi;
            state_out[2 * B + b] = r;
            state_out[3 * B + b] = d0;
        }
    }
    if (!move && out == cur) return;
    load_tile<VEC>(cur + o, T, tile, 0.0f, c);
    if (move) {
        float4 x[kVecs];
        load_tile<VEC>(orig + o, T, tile, 0.0f, x);
#pragma unroll
        for (int v = 0; v < kVecs; ++v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) lane(c[v], k) = point_elem(lane(c[v], k), lane(x[v], k), r, lo, hi);
        }
    }
    store_tile<VEC>(out + o, T, tile, c);
}

// ---- b. the probe slots ---------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void hsj_probe_kernel(const float *__restrict__ cur, const float *__restrict__ mag,
                                                               const int32_t *__restrict__ active, float *__restrict__ out,
                                                               int64_t B, int64_t T, int s0, int ns, float lo, float hi,
                                                               uint64_t seed, uint64_t offset) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    float4 a[kVecs];
    load_tile<VEC>(cur + b * T, T, tile, 0.0f, a);
    const bool moves = active[b] != 0;
    const float m = mag[b];
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
        const int64_t q = quad_of(tile, v);
        if (!in_row(T, q, 0)) continue;  // no barrier in this kernel
        Quad r = {};
        int call = -1;
        for (int j = s0; j < s0 + ns; ++j) {
            float4 p = a[v];  // an inactive row: cur's bytes in every slot
            if (moves) {
                if ((j >> 5) != call) {
                    call = j >> 5;
                    r = direction_bits(q, b, seed, offset, call);
                }
                const uint32_t nib = direction_nibble(r, j);
                p.x = clampf(a[v].x + signed_by(m, nib, 0), lo, hi);
                p.y = clampf(a[v].y + signed_by(m, nib, 1), lo, hi);
                p.z = clampf(a[v].z + signed_by(m, nib, 2), lo, hi);
                p.w = clampf(a[v].w + signed_by(m, nib, 3), lo, hi);
            }
            store4<VEC>(out + ((int64_t)(j - s0) * B + b) * T, T, q, p);
        }
    }
}

// ---- c. the candidates ------------------------------------------------------------------------------------------------------------

template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void hsj_candidates_kernel(const float *__restrict__ cur, const float *__restrict__ z,
                                                                    const int64_t *__restrict__ labels,
                                                                    const float *__restrict__ dist,
                                                                    const int32_t *__restrict__ active, float *__restrict__ out,
                                                                    int64_t B, int64_t T, int n, int trials, float xi_rel, float lo,
                                                                    float hi, uint64_t seed, uint64_t offset) {
    // decisions of directions 8 w .. 8 w + 7 at bits 0, 4, .. 28 of word w: [0] the adversarial probes, [1] the others
    __shared__ uint32_t masks[2][kMaskWords];
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    float4 a[kVecs];
    load_tile<VEC>(cur + b * T, T, tile, 0.0f, a);
    if (active[b] == 0) {  // uniform over the row, before the barrier
        for (int k = 0; k < trials; ++k) store_tile<VEC>(out + ((int64_t)k * B + b) * T, T, tile, a);
        return;
    }
    const bool is_one = labels[b] == 1;
    const int words = (n + 7) >> 3;
    for (int w = threadIdx.x; w < words; w += kWgThreads) {
        uint32_t adv = 0, rest = 0;
        for (int i = 0; i < 8 && 8 * w + i < n; ++i) {
            if (adversarial(z[(int64_t)(8 * w + i) * B + b], is_one)) adv |= 1u << (4 * i);
            else rest |= 1u << (4 * i);
        }
        masks[0][w] = adv;
        masks[1][w] = rest;
    }
    __syncthreads();
    int na[kVecs][4], ne[kVecs][4], c = 0;
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) na[v][k] = ne[v][k] = 0;
    }
    for (int call = 0; call * 32 < n; ++call) {
        Quad r[kVecs];
#pragma unroll
        for (int v = 0; v < kVecs; ++v) r[v] = direction_bits(quad_of(tile, v), b, seed, offset, call);
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4) {
            const int w = call * 4 + w4;
            if (w >= words) break;  // uniform
            const uint32_t adv = masks[0][w], rest = masks[1][w];
            c += __popc(adv);
#pragma unroll
            for (int v = 0; v < kVecs; ++v) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    na[v][k] += __popc(r[v].v[w4] & (adv << k));
                    ne[v][k] += __popc(r[v].v[w4] & (rest << k));
                }
            }
        }
    }
    const float xi = dist[b] * xi_rel;
    float4 s[kVecs];
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int val = c == n ? n - 2 * na[v][k] : c == 0 ? 2 * ne[v][k] - n : c * ne[v][k] - (n - c) * na[v][k];
            lane(s[v], k) = (float)(val > 0) - (float)(val < 0);
        }
    }
    float scale = 1.0f;
    for (int t = 0; t < trials; ++t) {
        const float step = xi * scale;
        float4 p[kVecs];
#pragma unroll
        for (int v = 0; v < kVecs; ++v) {
#pragma unroll
            for (int k = 0; k < 4; ++k) lane(p[v], k) = clampf(lane(a[v], k) + step * lane(s[v], k), lo, hi);
        }
        store_tile<VEC>(out + ((int64_t)t * B + b) * T, T, tile, p);
        scale *= 0.5f;
    }
}

// ---- d. the choice ------------------------------------------------------------------------------------------------------------------

// out may be cur: a row that stays is then not written at all, and a row that moves is read from cand.
template <bool VEC>
__global__ __launch_bounds__(kWgThreads) void hsj_take_kernel(const float *cur, const float *__restrict__ cand,
                                                              const float *__restrict__ zc, const int64_t *__restrict__ labels,
                                                              const int32_t *__restrict__ active, int32_t *__restrict__ queries,
                                                              float *out, int64_t B, int64_t T, int n, int trials) {
    const int tile = blockIdx.x;
    const int64_t b = blockIdx.y;
    const float *src = cur + b * T;
    if (active[b] != 0) {
        const bool is_one = labels[b] == 1;
        int used = trials;
        for (int k = 0; k < trials; ++k) {
            if (adversarial(zc[(int64_t)k * B + b], is_one)) {  // the first adversarial slot: the largest step
                src = cand + ((int64_t)k * B + b) * T;
                used = k + 1;
                break;
            }
        }
        if (tile == 0 && threadIdx.x == 0) queries[b] += n + used;
    }
    if (src == cur + b * T && out == cur) return;  // uniform over the row
    float4 r[kVecs];
    load_tile<VEC>(src, T, tile, 0.0f, r);
    store_tile<VEC>(out + b * T, T, tile, r);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------

struct Span {
    const void *p;
    size_t bytes;
};

// Does [w, w + w_bytes) — something a launch writes — lie outside every other (non-null) operand?
inline bool writes_apart(const void *w, size_t w_bytes, std::initializer_list<Span> others) {
    for (const Span &s : others)
        if (s.p && overlap2(w, w_bytes, s.p, s.bytes)) return false;
    return true;
}

}  // namespace

extern "C" {

int advstep_hsj_search_open_f32(const float *cur, const float *orig, const float *dist, const int32_t *active, float *state,
                                float *out, int64_t B, int64_t T, float lo, float hi, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && orig && dist && active && state && out);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float), planes = 4 * per_row;
    ADVSTEP_REQUIRE(writes_apart(out, rows, {{cur, rows}, {orig, rows}, {dist, per_row}, {active, per_row}, {state, planes}}));
    ADVSTEP_REQUIRE(writes_apart(state, planes, {{cur, rows}, {orig, rows}, {dist, per_row}, {active, per_row}}));
    launch_tiles(ROW_KERNEL_PAIR(hsj_search_kernel, kOpen), rows_vec(T, {cur, orig, out}), B, T, as_stream(stream), cur, orig,
                 (const float *)nullptr, (const int64_t *)nullptr, dist, active, (const float *)nullptr, state, (int32_t *)nullptr, 0,
                 out, B, T, lo, hi);
    return status_after_launch();
}

int advstep_hsj_search_next_f32(const float *cur, const float *orig, const float *z, const int64_t *labels, const int32_t *active,
                                const float *state, float *state_out, float *out, int64_t B, int64_t T, float lo, float hi,
                                advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && orig && z && labels && active && state && state_out && out);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float), planes = 4 * per_row;
    const size_t label_bytes = (size_t)B * sizeof(int64_t);
    ADVSTEP_REQUIRE(writes_apart(out, rows, {{cur, rows}, {orig, rows}, {z, per_row}, {labels, label_bytes}, {active, per_row},
                                             {state, planes}, {state_out, planes}}));
    ADVSTEP_REQUIRE(writes_apart(state_out, planes, {{cur, rows}, {orig, rows}, {z, per_row}, {labels, label_bytes},
                                                     {active, per_row}, {state, planes}}));  // ping-pong: never reads what it writes
    launch_tiles(ROW_KERNEL_PAIR(hsj_search_kernel, kNext), rows_vec(T, {cur, orig, out}), B, T, as_stream(stream), cur, orig, z,
                 labels, (const float *)nullptr, active, state, state_out, (int32_t *)nullptr, 0, out, B, T, lo, hi);
    return status_after_launch();
}

int advstep_hsj_search_close_f32(const float *cur, const float *orig, const float *z, const int64_t *labels, const int32_t *active,
                                 const float *state, int32_t *queries, int64_t rounds, float *out, int64_t B, int64_t T, float lo,
                                 float hi, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(rounds >= 0 && rounds <= INT32_MAX);
    if (B == 0 || T == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && orig && z && labels && active && state && queries && out);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float), planes = 4 * per_row;
    const size_t label_bytes = (size_t)B * sizeof(int64_t);
    ADVSTEP_REQUIRE(out == cur || !overlaps(out, cur, rows));
    ADVSTEP_REQUIRE(writes_apart(out, rows, {{orig, rows}, {z, per_row}, {labels, label_bytes}, {active, per_row}, {state, planes},
                                             {queries, per_row}}));
    ADVSTEP_REQUIRE(writes_apart(queries, per_row, {{cur, rows}, {orig, rows}, {z, per_row}, {labels, label_bytes},
                                                    {active, per_row}, {state, planes}}));
    launch_tiles(ROW_KERNEL_PAIR(hsj_search_kernel, kClose), rows_vec(T, {cur, orig, out}), B, T, as_stream(stream), cur, orig, z,
                 labels, (const float *)nullptr, active, state, (float *)nullptr, queries, (int)rounds, out, B, T, lo, hi);
    return status_after_launch();
}

int advstep_hsj_probe_f32(const float *cur, const float *mag, const int32_t *active, float *out, int64_t B, int64_t T, int64_t s0,
                          int64_t ns, float lo, float hi, uint64_t seed, uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(s0 >= 0 && ns >= 0 && s0 <= kMaxDirections && ns <= kMaxDirections - s0);
    if (B == 0 || T == 0 || ns == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && mag && active && out);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float);
    ADVSTEP_REQUIRE(writes_apart(out, (size_t)ns * rows, {{cur, rows}, {mag, per_row}, {active, per_row}}));
    launch_tiles(ROW_KERNEL_PAIR(hsj_probe_kernel), rows_vec(T, {cur, out}), B, T, as_stream(stream), cur, mag, active, out, B, T,
                 (int)s0, (int)ns, lo, hi, seed, offset);
    return status_after_launch();
}

int advstep_hsj_candidates_f32(const float *cur, const float *z, const int64_t *labels, const float *dist, const int32_t *active,
                               float *out, int64_t B, int64_t T, int64_t n, int64_t trials, float xi_rel, float lo, float hi,
                               uint64_t seed, uint64_t offset, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(n >= 0 && n <= kMaxDirections && trials >= 0 && trials <= kMaxTrials);
    if (B == 0 || T == 0 || trials == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && labels && dist && active && out && (z || n == 0));
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float);
    ADVSTEP_REQUIRE(writes_apart(out, (size_t)trials * rows, {{cur, rows}, {z, (size_t)n * per_row},
                                                              {labels, (size_t)B * sizeof(int64_t)}, {dist, per_row},
                                                              {active, per_row}}));
    launch_tiles(ROW_KERNEL_PAIR(hsj_candidates_kernel), rows_vec(T, {cur, out}), B, T, as_stream(stream), cur, z, labels, dist,
                 active, out, B, T, (int)n, (int)trials, xi_rel, lo, hi, seed, offset);
    return status_after_launch();
}

int advstep_hsj_take_f32(const float *cur, const float *cand, const float *zc, const int64_t *labels, const int32_t *active,
                         int32_t *queries, float *out, int64_t B, int64_t T, int64_t n, int64_t trials, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && B <= kMaxGridY);
    ADVSTEP_REQUIRE(n >= 0 && n <= kMaxDirections && trials >= 0 && trials <= kMaxTrials);
    if (B == 0 || T == 0 || trials == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(cur && cand && zc && labels && active && queries && out);
    const size_t rows = (size_t)B * T * sizeof(float), per_row = (size_t)B * sizeof(float);
    const size_t label_bytes = (size_t)B * sizeof(int64_t);
    ADVSTEP_REQUIRE(out == cur || !overlaps(out, cur, rows));
    ADVSTEP_REQUIRE(writes_apart(out, rows, {{cand, (size_t)trials * rows}, {zc, (size_t)trials * per_row}, {labels, label_bytes},
                                             {active, per_row}, {queries, per_row}}));
    ADVSTEP_REQUIRE(writes_apart(queries, per_row, {{cur, rows}, {cand, (size_t)trials * rows}, {zc, (size_t)trials * per_row},
                                                    {labels, label_bytes}, {active, per_row}}));
    launch_tiles(ROW_KERNEL_PAIR(hsj_take_kernel), rows_vec(T, {cur, cand, out}), B, T, as_stream(stream), cur, cand, zc, labels,
                 active, queries, out, B, T, (int)n, (int)trials);
    return status_after_launch();
}

}  // extern "C"
