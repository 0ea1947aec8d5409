// stft_reg.h — the register-resident 512-point real transform of the frontend's framing, shared by lfcc_stft.hip and masking.hip
// (internal: not part of the C ABI in include/).
//
// masking.hip transforms the same frames as the LFCC frontend (n_fft 512, centre framing, reflect padding) and sends a spectrum
// gradient back through the same inverse, window and overlap-add.  These device functions were moved here from lfcc_stft.hip
// unchanged (its device assembly is byte-identical before and after the move; its "round 4" comments explain each of them at
// length; pack_real_reg and fill_twiddle_rows are new and only masking.hip's):
//   fft4 / fft16 / fft256_reg       the 256-point complex transform as 16 x 16: a frame on 16 lanes, 16 points per lane, one
//                                   transposition through the frame's LDS block (pitch 17: conflict-free)
//   park_vector / mirror_of         a frame's 256-vector in its block so that every lane finds element (N - k) mod N
//   unpack_real_reg                 Z -> 2 X[k] of the real 512-point transform (the factor 2 is left in)
//   overlap_add_frames              a group's windowed frame gradients -> the waveform gradient, every sample summed in frame
//                                   order and added with ONE float atomic per group and sample onto a zeroed row
// and stft_tables.inc (the twiddle constants).  Include after advstep_common.h.

#ifndef ADVSTEP_STFT_REG_H
#define ADVSTEP_STFT_REG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "advstep_common.h"

namespace {

constexpr int kN = 256;            // complex FFT length (n_fft = 512 real samples)
constexpr int kNfft = 2 * kN;
constexpr int kBins = kN + 1;      // one-sided spectrum
constexpr int kGroup = 4;          // frames per wave at a time (16 lanes each): the unit of the overlap-add
constexpr int kPitch = 17;                       // float2 slots per row of a frame's 16 x 16 exchange block
constexpr int kFrameSlots = 16 * kPitch;         // 272 float2 per frame (also holds a frame's 512 floats / 257 bins)

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 conjf2(float2 a) { return make_float2(a.x, -a.y); }

#include "stft_tables.inc"

__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {        // fused: 2 mul + 2 fma
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cmulc(float2 a, float cr, float ci) { return cmulf(a, make_float2(cr, ci)); }

// 4-point transform of (a, b, c, d): forward y1 = (a - c) - i (b - d), inverse y1 = (a - c) + i (b - d)
template <bool INV>
__device__ __forceinline__ void fft4(float2 &a, float2 &b, float2 &c, float2 &d) {
    const float2 s02 = cadd(a, c), d02 = csub(a, c), s13 = cadd(b, d), d13 = csub(b, d);
    const float2 r = INV ? make_float2(-d13.y, d13.x) : make_float2(d13.y, -d13.x);
    a = cadd(s02, s13);
    b = cadd(d02, r);
    c = csub(s02, s13);
    d = csub(d02, r);
}

// 16-point transform in place, natural order in and out: x[4 n1 + n2] -> 4-point over n1 -> W16^(n2 k1) -> 4-point over n2.
template <bool INV>
__device__ __forceinline__ void fft16(float2 (&x)[16]) {
    constexpr float C1 = 0.92387953251128674f, S1 = 0.38268343236508977f, H = 0.70710678118654752f;
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) fft4<INV>(x[n2], x[4 + n2], x[8 + n2], x[12 + n2]);      // x[4 k1 + n2] = b[n2][k1]
    // W16^m = (cos, -sin)(2 pi m / 16); INV: conjugate
    const float sg = INV ? 1.0f : -1.0f;
    x[4 + 1] = cmulc(x[4 + 1], C1, sg * S1);       // n2 = 1, k1 = 1: W^1
    x[8 + 1] = cmulc(x[8 + 1], H, sg * H);         // n2 = 1, k1 = 2: W^2
    x[12 + 1] = cmulc(x[12 + 1], S1, sg * C1);     // n2 = 1, k1 = 3: W^3
    x[4 + 2] = cmulc(x[4 + 2], H, sg * H);         // n2 = 2, k1 = 1: W^2
    x[8 + 2] = INV ? make_float2(-x[8 + 2].y, x[8 + 2].x) : make_float2(x[8 + 2].y, -x[8 + 2].x);   // W^4 = -i (forward)
    x[12 + 2] = cmulc(x[12 + 2], -H, sg * H);      // n2 = 2, k1 = 3: W^6
    x[4 + 3] = cmulc(x[4 + 3], S1, sg * C1);       // n2 = 3, k1 = 1: W^3
    x[8 + 3] = cmulc(x[8 + 3], -H, sg * H);        // n2 = 3, k1 = 2: W^6
    x[12 + 3] = cmulc(x[12 + 3], -C1, -sg * S1);   // n2 = 3, k1 = 3: W^9
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) fft4<INV>(x[4 * k1], x[4 * k1 + 1], x[4 * k1 + 2], x[4 * k1 + 3]);   // -> y[k1 + 4 k2] at x[4 k1 + k2]
    // un-transpose the 4 x 4 block: y[k1 + 4 k2] sits at x[4 k1 + k2]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i + 1; j < 4; ++j) {
            const float2 t = x[4 * i + j];
            x[4 * i + j] = x[4 * j + i];
            x[4 * j + i] = t;
        }
}

// An opaque copy of a lane index: loads from the constant tables indexed with it cannot be issued before this point (they are
// invariant loads, which hipcc otherwise hoists to the top of the loop body and holds in registers across everything)
__device__ __forceinline__ int here(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// "These 16 values are complete HERE": an empty asm every one of them passes through, with a memory clobber.  The loads of the
// next phase cannot be issued above it and the arithmetic producing the values cannot sink below it — without it hipcc overlaps
// a phase's loads with the previous phase's arithmetic and the live set of the two (up to 180 registers) costs a wave of occupancy.
__device__ __forceinline__ void phase_done(float2 (&x)[16]) {
    asm volatile("" : "+v"(x[0].x), "+v"(x[0].y), "+v"(x[1].x), "+v"(x[1].y), "+v"(x[2].x), "+v"(x[2].y), "+v"(x[3].x), "+v"(x[3].y),
                      "+v"(x[4].x), "+v"(x[4].y), "+v"(x[5].x), "+v"(x[5].y), "+v"(x[6].x), "+v"(x[6].y), "+v"(x[7].x), "+v"(x[7].y)
                 :: "memory");
    asm volatile("" : "+v"(x[8].x), "+v"(x[8].y), "+v"(x[9].x), "+v"(x[9].y), "+v"(x[10].x), "+v"(x[10].y), "+v"(x[11].x), "+v"(x[11].y),
                      "+v"(x[12].x), "+v"(x[12].y), "+v"(x[13].x), "+v"(x[13].y), "+v"(x[14].x), "+v"(x[14].y), "+v"(x[15].x), "+v"(x[15].y)
                 :: "memory");
}

template <int BASE>
__device__ __forceinline__ void half_done(float2 (&x)[16]) {       // the same for x[BASE .. BASE + 7]
    asm volatile("" : "+v"(x[BASE].x), "+v"(x[BASE].y), "+v"(x[BASE + 1].x), "+v"(x[BASE + 1].y), "+v"(x[BASE + 2].x), "+v"(x[BASE + 2].y),
                      "+v"(x[BASE + 3].x), "+v"(x[BASE + 3].y), "+v"(x[BASE + 4].x), "+v"(x[BASE + 4].y), "+v"(x[BASE + 5].x),
                      "+v"(x[BASE + 5].y), "+v"(x[BASE + 6].x), "+v"(x[BASE + 6].y), "+v"(x[BASE + 7].x), "+v"(x[BASE + 7].y)
                 :: "memory");
}

// LDS-only ordering inside a wave (its LDS instructions execute in order; only the compiler and the counter must agree)
__device__ __forceinline__ void lds_wave_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// [l][j] = W256^(l j), rows at pitch 17: the lane-constant twiddles between the two 16-point passes, one table per workgroup
__device__ __forceinline__ void fill_twiddle_rows(float2 *twl) {
    for (int m = threadIdx.x; m < kN; m += blockDim.x) twl[(m >> 4) * kPitch + (m & 15)] = kTw256[((m >> 4) * (m & 15)) & 255];
}

// 256-point transform of the wave's 4 frames.  Forward: in x[r] = z[16 r + l] (l = lane & 15), out x[r] = Z[l + 16 r].
// Inverse: in x[r] = Z[l + 16 r], out x[r] = z[l + 16 r] (unnormalised).  `blk`: the frame's kFrameSlots float2 of LDS.
template <bool INV>
__device__ __forceinline__ void fft256_reg(float2 (&x)[16], const float2 *twl, float2 *blk, int l) {
    fft16<INV>(x);
    phase_done(x);
    // W256^(l j), j = 1 .. 15: row l of the workgroup's 16 x 16 table in LDS (30 registers per lane if kept: they cost a wave
    // of occupancy; the reads ride under the first 16-point transform)
#pragma unroll
    for (int j = 1; j < 16; ++j) {
        const float2 t = twl[l * kPitch + j];
        x[j] = cmulf(x[j], INV ? conjf2(t) : t);
    }
    lds_wave_fence();                            // whatever the caller last read from `blk` has been delivered
#pragma unroll
    for (int j = 0; j < 16; ++j) blk[j * kPitch + l] = x[j];
    lds_wave_fence();
#pragma unroll
    for (int j = 0; j < 16; ++j) x[j] = blk[l * kPitch + j];
    fft16<INV>(x);
}

// A frame's 256-vector in its block: element k = l + 16 r (lane l, register r) at slot 17 r + l; the elements of lane 0 are
// stored a second time in the spare 17th column of the row before (element 16 r at slot 17 (r - 1) + 16, element 0 at
// 17 . 15 + 16), so that EVERY lane finds its mirror element (N - k) mod N at slot 17 (15 - r) + (16 - l): one lane-constant
// base and compile-time offsets, no index arithmetic.
__device__ __forceinline__ void park_vector(float2 *blk, const float2 (&x)[16], int l) {
#pragma unroll
    for (int r = 0; r < 16; ++r) blk[r * kPitch + l] = x[r];
    if (l == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) blk[((r + 15) & 15) * kPitch + 16] = x[r];
    }
}
__device__ __forceinline__ float2 mirror_of(const float2 *blk, int r, int l) { return blk[(15 - r) * kPitch + (16 - l)]; }

// Z (the transform of the packed frame, lane l register r = Z[l + 16 r]) -> 2 X[l + 16 r] in place and 2 X[256] (real) in `nyq`
// (meaningful on lane l == 0):  2 X[k] = (Z[k] + Z*[N - k]) + W512^k . (-i) (Z[k] - Z*[N - k]).
__device__ __forceinline__ void unpack_real_reg(float2 (&x)[16], float &nyq, float2 *blk, int l) {
    lds_wave_fence();
    park_vector(blk, x, l);
    lds_wave_fence();
    nyq = 2.0f * (x[0].x - x[0].y);
    const int lt = here(l);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (r == 8) half_done<0>(x);               // two batches of 8 mirror + 8 table reads, not one of 16 + 16
        const float2 zc = conjf2(mirror_of(blk, r, l));
        const float2 e = cadd(x[r], zc), d = csub(x[r], zc);
        x[r] = cadd(e, cmulf(kTw512[lt + 16 * r], make_float2(d.y, -d.x)));
    }
}

// The inverse of the un-packing, for a spectrum gradient already scaled for the one-sided inverse (interior bins halved, DC and
// Nyquist real): x[r] = G[l + 16 r], g_nyq = G[256] (read on lane 0) -> the packed input of the unnormalised 256-point inverse,
// Z'[k] = (G[k] + G*[N - k]) + i W512^-k (G[k] - G*[N - k]);  N - 0 is the Nyquist bin.
__device__ __forceinline__ void pack_real_reg(float2 (&x)[16], float g_nyq, float2 *blk, int l) {
    phase_done(x);
    lds_wave_fence();
    park_vector(blk, x, l);
    lds_wave_fence();
    const int lp = here(l);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (r == 8) half_done<0>(x);
        float2 gc = conjf2(mirror_of(blk, r, l));
        if (r == 0 && l == 0) gc = make_float2(g_nyq, 0.0f);
        const float2 e = cadd(x[r], gc), d = csub(x[r], gc);
        const float2 wd = cmulf(conjf2(kTw512[lp + 16 * r]), d);
        x[r] = make_float2(e.x - wd.y, e.y + wd.x);
    }
}

// Overlap-add of a group's kGroup windowed frame gradients (dframe, STRIDE floats apart) into the zeroed dxb: every sample the
// frames touch is summed over (positions that read it) x (frames) in a fixed order and added with one float atomic; positions
// are padded coordinates p = q + nfft / 2.  Reflections only exist next to the two ends of the signal.  With hop >= 128 a sample
// is reached by at most two groups: two operands per address, commutative, so the sum's bits do not depend on their order.
template <int STRIDE>
__device__ __forceinline__ void overlap_add_frames(const float *dframe, float *__restrict__ dxb, int f_base, int NF, int hop, int T,
                                                   int tid, int nthreads) {
    const int p_lo = f_base * hop;                                          // first padded position of the first frame
    const int frames_here = (NF - f_base) < kGroup ? (NF - f_base) : kGroup;
    const int p_hi = p_lo + (frames_here - 1) * hop + kNfft;                // one past the last
    auto add_from = [&](int p, float &acc) {     // frames in ascending order: a fixed summation order
        if (p < p_lo || p >= p_hi) return;
#pragma unroll
        for (int fl = 0; fl < kGroup; ++fl) {
            const int n = p - p_lo - fl * hop;
            if (fl < frames_here && n >= 0 && n < kNfft) acc += dframe[fl * STRIDE + n];
        }
    };
    const bool near_left = p_lo < 2 * kN, near_right = p_hi > T;            // wave-uniform, almost always false
    const int t_first = p_lo - kN, span_all = p_hi - p_lo;
    for (int i = tid; i < span_all; i += nthreads) {
        const int t = t_first + i;
        if (t < 0 || t >= T) continue;            // padded positions outside the signal are reached by reflection below
        float acc = 0.0f;
        add_from(t + kN, acc);
        if (near_left && t >= 1 && t <= kN) add_from(kN - t, acc);                               // left reflection
        if (near_right && t <= T - 2 && t >= T - 1 - kN) add_from(2 * (T - 1) - t + kN, acc);    // right reflection
        if (acc != 0.0f) atomicAdd(dxb + t, acc);
    }
    if (!(near_left || near_right)) return;
    // samples reached ONLY through a reflection from this group's range (their direct position belongs to another group's
    // range or to none): left edge t = pad - p for p < pad, right edge t = 2 (T - 1) - (p - pad) for p - pad >= T
    for (int i = tid; i < span_all; i += nthreads) {
        const int p = p_lo + i, q = p - kN;
        int t = -1;
        if (q < 0) t = -q;
        else if (q >= T) t = 2 * (T - 1) - q;
        if (t < 0 || t >= T) continue;
        const int pd = t + kN;
        if (pd >= p_lo && pd < p_hi) continue;    // the first loop already took this contribution
        float acc = 0.0f;
        add_from(p, acc);
        if (acc != 0.0f) atomicAdd(dxb + t, acc);
    }
}

}  // namespace

#endif  // ADVSTEP_STFT_REG_H
