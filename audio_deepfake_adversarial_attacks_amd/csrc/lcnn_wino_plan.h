// lcnn_wino_plan.h — the host-side half of lcnn_wino.hip: what the Winograd 3x3 kernel can read (Src) and do with the result
// (Epi), and which launches one convolution becomes (plan_wino).  Plain C++, no device code; included by lcnn_wino.hip only.
#pragma once

#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "advstep_common.h"

namespace {

constexpr int kWaves = 8, kThreads = kWaves * 64;
constexpr int kChunkCin = 16;                         // input channels per LDS chunk
constexpr int kChunkFloats = 16 * kChunkCin * 32;     // [xi][cin][16 j][2 m] = 32 KB
constexpr int kMaxResident = 4;                       // chunks kept in LDS when K <= 64
constexpr int kComputeUnits = 256;                    // of the MI355X: what a persistent grid is sized to

// ---- what the convolution kernel reads and what it does with the result -----------------------------------------------
// The enumerators' values are the template arguments the kernels have always had (they are in the mangled names).
enum class Src : int {
    Dense = 0,      // a dense tensor x (N, K, H, W)
    MfmPooled = 1,  // d(conv out) of a max-feature-map + 2x2 pool block, given in its compact form — the pooled gradient
                    // gy (N, C, H/2, W/2) and the selection bytes (advstep_mfm_pool2_forward_f32's encoding), K = 2C: channel k of
                    // half k / C at conv position (h, w) carries gy[k % C][h/2][w/2] if that position of that half won, else 0.  The
                    // 4x4 patch of a lane is expanded from the 3x3 pooled cells around its tile; the dense gradient never exists.
    Pooled = 2,     // the same for a plain MaxPool2d(2) (no halves): gy (N, K, H/2, W/2) and ATen-order selection bytes (2 * dh + dw):
                    // channel k at (h, w) carries gy[k][h/2][w/2] if that position won its window, else 0 (odd trailing row / column: 0)
};

enum class Epi : int {
    Store = 0,          // plain store of min(32, Cout - slice * 32) channels per slice (the input-gradient convolution)
    MfmPoolBn = 1,      // bias + max-feature-map + 2x2 pool [+ BatchNorm]; Cout = number of max-feature-map channels C
    MfmBn = 2,          // bias + max-feature-map [+ BatchNorm] without the pool; one selection byte per 2x2 tile
    ShiftLrelu = 3,     // + shift[ch], LeakyReLU(slope), plain store (the residual blocks of SpecRNet, advstep_detector.h); with a
                        // byte plane to fill, also the activation's sign bytes (see LreluGradBytes)
    BiasPool = 4,       // + bias[ch], MaxPool2d(2) with ATen's selection byte (detector_elem.hip::pool4): the conv output never exists
    LreluGradH = 5,     // * (h > 0 ? 1 : slope) with the activation's OUTPUT h (N, Cout, H, W) — LeakyReLU's backward (h has the sign
                        // of the activation's input for slope > 0) — plain store
    LreluGradBytes = 6, // the same from the activation's SIGN BYTES (read only): one byte per (n, channel, 2x2 tile), bit 2 i + j =
                        // h > 0 at tile position (i, j), (N, Cout, TH, TW) — what ShiftLrelu writes next to h.  At SpecRNet's first
                        // block that is 21 MB in the epilogue instead of 331 MB of h: 476 -> 3xx us (round 3)
    BiasPoolFew = 7,    // BiasPool plus a 1x1 convolution over the ga.few (1 or 2) channels of ga.x2 added to the convolution output on
                        // the vector ALUs before the pool, weights (Cout, few): SpecRNet's block0, whose downsample convolution has two
                        // input channels — as part of the reduction (GEN's x2) those two channels cost a whole k-step of six, 32 matrix
                        // instructions per wave and tile group for 8 useful rows of K; here they are 64 fused multiply-adds per lane
};

// each property of an epilogue, stated once
constexpr bool is_mfm(Epi e) { return e == Epi::MfmPoolBn || e == Epi::MfmBn; }           // 16 channel PAIRS per slice
constexpr bool adds_few(Epi e) { return e == Epi::BiasPoolFew; }                          // the few-channel 1x1 before the pool
constexpr bool pools(Epi e) { return e == Epi::MfmPoolBn || e == Epi::BiasPool || adds_few(e); }
constexpr bool reads_sign_bytes(Epi e) { return e == Epi::LreluGradBytes; }
constexpr bool has_constants(Epi e) { return is_mfm(e) || e == Epi::ShiftLrelu || e == Epi::BiasPool || adds_few(e); }
// 2x2 tiles of 32 rows per slice go out as they are (times a factor): these may run a last slice as ONE accumulator tile
constexpr bool plain_store(Epi e) { return !is_mfm(e) && !pools(e); }

// The STREAM kernels copy weight chunks global -> LDS by LDS-DMA rather than through registers (WeightChunks::copy); by default
// only the compact max-feature-map source's do.  -DWINO_GLDS=0 / 1 (tools/build_variant.sh): none / all of them.
constexpr bool chunks_by_dma(Src s) {
#ifdef WINO_GLDS
    return WINO_GLDS;
#else
    return s == Src::MfmPooled;
#endif
}

// The kernel's byte plane `idx` is the selection output (MfmPoolBn, MfmBn, BiasPool, BiasPoolFew), the sign-byte output
// (ShiftLrelu, optional) or — read only — LreluGradBytes' sign-byte input.
template <Epi EPI>
using EpiBytes = std::conditional_t<reads_sign_bytes(EPI), const uint8_t, uint8_t>;

// ---- what is launched ----------------------------------------------------------------------------------------------------
// The four environment knobs, read at every call (tests and tools/coresidency_probe.py flip them inside one process); all are
// A/B switches for measurements.
struct WinoKnobs {
    bool half_slice;    // ADVSTEP_WINO_HALF_SLICE=0: keep the single launch that multiplies a half-empty last slice's zero rows
    bool halves;        // ADVSTEP_WINO_HALVES=0: a one-slice compact backward as one launch (see GenArgs::halves)
    bool xcd;           // ADVSTEP_WINO_XCD=0: round-robin slices instead of one XCD per tile range
    int range_mult;     // ADVSTEP_WINO_RANGE_MULT=k (1..8, default 1): k times the workgroups, each walking 1 / k of the tile groups
                        // - a grid that is NOT persistent, so that workgroups of another stream's launch find compute units while this
                        // one runs (round 6 experiment; the weights are staged once per workgroup, i.e. k times as often)
};

inline WinoKnobs read_wino_knobs() {
    auto not_off = [](const char *name) {
        const char *e = getenv(name);
        return !(e && e[0] == '0');
    };
    const char *em = getenv("ADVSTEP_WINO_RANGE_MULT");
    return {not_off("ADVSTEP_WINO_HALF_SLICE"), not_off("ADVSTEP_WINO_HALVES"), not_off("ADVSTEP_WINO_XCD"),
            em && em[0] >= '1' && em[0] <= '8' ? em[0] - '0' : 1};
}

struct WinoLaunch {
    int NT;
    bool stream, wodd;
    int halves, n_slices, slice0, ranges, xcd;
    size_t lds;
};
struct WinoPlan {
    int count = 0;
    WinoLaunch launch[2];
};

// Which launches one convolution is: the full slices as two-tile kernels, and before them a half-empty last slice on its own,
// or the two halves of a single slice.
inline WinoPlan plan_wino(Epi epi, Src src, bool gen, int64_t N, int64_t K, int64_t H, int64_t W, int64_t Cout, int slices,
                          const WinoKnobs &knobs) {
    const int chunks = (int)ceil_div(K, kChunkCin);
    const bool stream = chunks > kMaxResident;
    const int64_t groups = ceil_div(N * ((H + 1) / 2) * ((W + 1) / 2), 16);
    const size_t lds = (size_t)(stream ? (src == Src::MfmPooled ? 4 : 2) : chunks) * kChunkFloats * sizeof(float);
    const bool wodd = src == Src::Dense && (W & 1);
    WinoPlan plan;
    auto add = [&](int NT, int halves, int n_slices, int slice0) {
        int ranges = knobs.range_mult * kComputeUnits / n_slices;
        if ((int64_t)ranges * kWaves > groups) ranges = (int)ceil_div(groups, kWaves);
        if (ranges < 1) ranges = 1;
        // the slices of one tile range read the same input tiles at the same time: put them on ONE XCD (workgroups b, b + 8, ...
        // share an L2) so all but one of the reads hit it: 2-3 % on L13 forward and SpecRNet's block2 — only where rounding
        // the ranges down to a multiple of 8 does not add a pass over the tile groups
        int xcd = 0;
        const int ranges8 = ranges & ~7;
        if (knobs.xcd && n_slices > 1 && ranges8 >= 8 &&
            ceil_div(groups, (int64_t)ranges8 * kWaves) == ceil_div(groups, (int64_t)ranges * kWaves)) {
            ranges = ranges8;
            xcd = 1;
        }
        plan.launch[plan.count++] = {NT, stream, wodd, halves, n_slices, slice0, ranges, xcd, lds};
    };
    // plain-store epilogues with a half-empty last slice (Cout % 32 in 1..16): that slice on its own, one accumulator tile
    int full = slices;
    if (plain_store(epi) && Cout - (int64_t)(slices - 1) * 32 <= 16 && knobs.half_slice) {
        full = slices - 1;
        add(1, 0, 1, slices - 1);
    }
    // a ONE-slice layer whose tile groups do not fill the chip's 2 048 wave slots even once: the slice as its two 16-row
    // halves, one accumulator tile each - twice the workgroups, half the matrix instructions per wave (the patch loads and
    // input transforms are done twice, on compute units that would have idled)
    if (epi == Epi::Store && src == Src::MfmPooled && !gen && full == 1 && slices == 1 && Cout == 32 &&
        groups <= (int64_t)kComputeUnits * kWaves / 2 && knobs.halves) {
        add(1, 1, 2, 0);
        return plan;
    }
    if (full > 0) add(2, 0, full, 0);
    return plan;
}

// ---- what the C-ABI wrappers check once -----------------------------------------------------------------------------------
// The kernel's 32-bit addressing: a dense source's raw buffer (`dense_ch` channels: the larger of x and x2) is sized in
// bytes, a compact source's (`pooled_ch` channels on the pooled grid) in elements that are shifted left by 2, the output
// (`out_rows` rows; the LCNN wrappers pass 0, they leave it unbounded as they always have) in elements, tiles in an int.
// A channel count of 0: no such tensor, nothing to check.
inline bool wino_sizes_ok(int64_t N, int64_t H, int64_t W, int64_t dense_ch, int64_t pooled_ch, int64_t out_rows) {
    return (uint64_t)N * dense_ch * H * W * 4 < (1ull << 31) && (uint64_t)N * pooled_ch * (H / 2) * (W / 2) < (1ull << 29) &&
           (uint64_t)N * out_rows * H * W * 4 < (1ull << 33) && (uint64_t)N * ((H + 1) / 2) * ((W + 1) / 2) < (1ull << 31);
}

// the reduction length a general (GEN) launch runs: whole k-steps of 4 channels, at least two of them; an odd count is fine
inline int64_t padded_k(int64_t K) { return K <= 8 ? 8 : ceil_div(K, 4) * 4; }

}  // namespace
