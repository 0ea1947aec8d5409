// masking.hip — the psychoacoustic-masking kernels (C ABI: include/advstep_masking.h): the short-time power spectrum of a
// difference, the hinge of that spectrum against a threshold with its exact gradient in ONE launch, and the PGD step that
// mixes the classifier's gradient with the hinge's.
//
// Done with library ops the penalty is torch.stft -> |.|^2 -> relu(. - theta).sum() and an autograd pass back through all of
// it: the (B, NF, 257) complex planes written and re-read both ways.  Here the spectrum of a frame never leaves registers: a
// wave transforms 4 frames (stft_reg.h: lfcc_stft.hip's register-resident transform), decides e = P - theta > 0 per bin where
// the spectrum sits, scales the spectrum by s [e > 0] in place — that IS the gradient with respect to the one-sided spectrum —
// and runs the inverse, the window and the overlap-add.  HBM traffic: adv, x, theta read once, grad zero-filled and written.
//
// Two 1024-thread workgroups per row (kRowSplit): the three row statistics (sum, count, maximum) then need no workspace and no
// second launch.  Inside a workgroup their order is fixed (lane partials over the lane's frames, wave butterfly, 16 waves in
// order); the two workgroups of a row meet in the zero-filled stats with ONE atomic each per value — two operands per address,
// the rule of the overlap-add: a float sum of two terms, a sum of two exact integers and a maximum do not depend on the order.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "advstep_masking.h"
#include "advstep_frontend.h"
#include "advstep_common.h"
#include "row_workgroup.h"
#include "stft_reg.h"

namespace {

// x[r] = (w[2n] d[q + 2n], w[2n + 1] d[q + 2n + 1]),  n = 16 r + l,  q = f hop - 256 (reflect padding at the ends),
// d = a - b (DIFF) or a.
template <bool DIFF>
__device__ __forceinline__ void load_diff_frame_reg(const float *__restrict__ ab, const float *__restrict__ bb,
                                                    const float2 *__restrict__ win2, int T, int f, int hop, float2 (&x)[16],
                                                    int l) {
    const int q_first = f * hop - kN;
    const bool al8 = ((reinterpret_cast<uintptr_t>(ab) | (DIFF ? reinterpret_cast<uintptr_t>(bb) : 0)) & 7u) == 0;
    if (q_first >= 0 && q_first + kNfft <= T && ((q_first & 1) == 0) && al8) {
        const float2 *a2 = reinterpret_cast<const float2 *>(ab + q_first);
        const float2 *b2 = reinterpret_cast<const float2 *>(bb + q_first);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float2 v = a2[16 * r + l];
            if (DIFF) {
                const float2 u = b2[16 * r + l];
                v = make_float2(v.x - u.x, v.y - u.y);
            }
            const float2 wv = win2[16 * r + l];
            x[r] = make_float2(wv.x * v.x, wv.y * v.y);
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = 16 * r + l;
        int q0 = q_first + 2 * n, q1 = q0 + 1;
        q0 = q0 < 0 ? -q0 : q0;
        q0 = q0 >= T ? 2 * (T - 1) - q0 : q0;
        q1 = q1 < 0 ? -q1 : q1;
        q1 = q1 >= T ? 2 * (T - 1) - q1 : q1;
        float d0 = ab[q0], d1 = ab[q1];
        if (DIFF) d0 = d0 - bb[q0], d1 = d1 - bb[q1];
        const float2 wv = win2[n];
        x[r] = make_float2(wv.x * d0, wv.y * d1);
    }
}

// |X|^2 from 2 X
__device__ __forceinline__ float power_of(float2 x2) { return 0.25f * (x2.x * x2.x + x2.y * x2.y); }

// ---- the power spectrum: grid (ceil(NF / 32), B), a wave takes 2 groups of 4 frames ---------------------------------------
constexpr int kPowWaves = 4, kPowGroups = 2, kPowFrames = kPowWaves * kPowGroups * kGroup;

struct LdsPow {
    float2 blk[kPowWaves][kGroup][kFrameSlots];
    float2 twl[16 * kPitch];
};

template <bool DIFF>
__global__ __launch_bounds__(kPowWaves * 64) void stft_power_kernel(const float *__restrict__ a, const float *__restrict__ bsub,
                                                                    const float *__restrict__ w, float *__restrict__ power,
                                                                    int T, int NF, int hop) {
    __shared__ LdsPow S;
    fill_twiddle_rows(S.twl);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, fs = lane >> 4, l = lane & 15;
    __syncthreads();
    const int64_t b = blockIdx.y;
    float2 *blk = S.blk[wave][fs];
    for (int g = 0; g < kPowGroups; ++g) {
        const int f0 = blockIdx.x * kPowFrames + (wave * kPowGroups + g) * kGroup;
        if (f0 >= NF) break;                                   // wave-uniform
        const int f = f0 + fs;
        const bool live = f < NF;
        float2 xr[16];
        load_diff_frame_reg<DIFF>(a + b * T, DIFF ? bsub + b * T : nullptr, reinterpret_cast<const float2 *>(w), T,
                                  live ? f : NF - 1, hop, xr, here(l));
        phase_done(xr);
        fft256_reg<false>(xr, S.twl, blk, l);
        float nyq;
        unpack_real_reg(xr, nyq, blk, l);
        phase_done(xr);
        if (live) {
            float *row = power + (b * NF + f) * kBins;
#pragma unroll
            for (int r = 0; r < 16; ++r) row[l + 16 * r] = power_of(xr[r]);
            if (l == 0) row[kN] = 0.25f * (nyq * nyq);
        }
        lds_wave_fence();                                      // the block is rewritten by the next group's exchange
    }
}

// a real call: the overlap-add's index arithmetic stays out of the transform's register allocation
__device__ __attribute__((noinline)) void overlap_add_group(const float *dframe, float *__restrict__ dxb, int f_base, int NF, int hop,
                                                            int T, int lane) {
    overlap_add_frames<2 * kFrameSlots>(dframe, dxb, f_base, NF, hop, T, lane, 64);
}

// ---- the hinge: grid (kRowSplit, rows), kRow threads -----------------------------------------------------------------------
constexpr int kRowSplit = 2;      // workgroups per row: at B = 128 one per row would leave half of the 256 CUs idle

struct LdsHinge {
    float2 blk[kRowWaves][kGroup][kFrameSlots];    // 139 264 B: gfx950's 160 KB of LDS hold one such workgroup per CU
    float2 twl[16 * kPitch];
    float red[3][kRowWaves];
};

__global__ __launch_bounds__(kRow) void masking_hinge_kernel(const float *__restrict__ adv, const float *__restrict__ x,
                                                             const float *__restrict__ w, const float *__restrict__ theta,
                                                             const float *__restrict__ row_scale, float *__restrict__ grad,
                                                             float *__restrict__ stats, int64_t B, int T, int NF, int hop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char raw[];
    LdsHinge &S = *reinterpret_cast<LdsHinge *>(raw);
    fill_twiddle_rows(S.twl);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, fs = lane >> 4, l = lane & 15;
    __syncthreads();
    float2 *blk = S.blk[wave][fs];
    const int groups = (NF + kGroup - 1) / kGroup;
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        const float *ab = adv + b * T, *xb = x + b * T;
        const float s = row_scale[b];
        float loss = 0.0f, worst = 0.0f;
        int count = 0;
        for (int g = blockIdx.x * kRowWaves + wave; g < groups; g += kRowSplit * kRowWaves) {       // wave-uniform
            const int f0 = g * kGroup, f = f0 + fs;
            const bool live = f < NF;
            const int fc = live ? f : NF - 1;
            float2 xr[16];
            load_diff_frame_reg<true>(ab, xb, reinterpret_cast<const float2 *>(w), T, fc, hop, xr, here(l));
            phase_done(xr);
            fft256_reg<false>(xr, S.twl, blk, l);
            float nyq;
            unpack_real_reg(xr, nyq, blk, l);
            phase_done(xr);
            // xr = 2 X.  e = P - theta decides the hinge; the gradient w.r.t. the one-sided spectrum is 2 s [e > 0] X, which the
            // one-sided inverse wants halved in the interior bins and real at DC / Nyquist: (s / 2) (2 X), resp. s Re(2 X) / 1
            const float *th = theta + (b * NF + fc) * kBins;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float t[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) t[i] = th[l + 16 * (4 * q + i)];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 4 * q + i;
                    const float p = power_of(xr[r]);
                    const float e = p - t[i];
                    const bool act = live && e > 0.0f;
                    if (live) worst = max_nan(worst, p / t[i]);
                    loss += act ? e : 0.0f;
                    count += act ? 1 : 0;
                    const bool dc = r == 0 && l == 0;
                    const float c = dc ? s : 0.5f * s;
                    xr[r] = act ? make_float2(c * xr[r].x, dc ? 0.0f : c * xr[r].y) : make_float2(0.0f, 0.0f);
                }
            }
            float g_nyq = 0.0f;
            if (l == 0) {
                const float tn = th[kN];
                const float p = 0.25f * (nyq * nyq);
                const float e = p - tn;
                const bool act = live && e > 0.0f;
                if (live) worst = max_nan(worst, p / tn);
                loss += act ? e : 0.0f;
                count += act ? 1 : 0;
                g_nyq = act ? s * nyq : 0.0f;
            }
            pack_real_reg(xr, g_nyq, blk, l);
            fft256_reg<true>(xr, S.twl, blk, l);
            // z'[n] = dframe[2n] + i dframe[2n + 1], n = l + 16 r: window, park the frame's 512 floats in its block
            lds_wave_fence();
            const int lp = here(l);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float2 wv = reinterpret_cast<const float2 *>(w)[lp + 16 * r];
                blk[l + 16 * r] = live ? make_float2(wv.x * xr[r].x, wv.y * xr[r].y) : make_float2(0.0f, 0.0f);
            }
            lds_wave_fence();
            overlap_add_group(reinterpret_cast<const float *>(S.blk[wave][0]), grad + b * T, f0, NF, hop, T, lane);
            lds_wave_fence();
        }
        // the workgroup's share of the row's statistics: lanes, then waves in order, then one atomic per value
        loss = wave_reduce(loss, SumOp());
        worst = wave_reduce(worst, MaxNanOp());
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
        if (lane == 0) {
            S.red[0][wave] = loss;
            S.red[1][wave] = (float)count;
            S.red[2][wave] = worst;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float ls = S.red[0][0], cn = S.red[1][0], wr = S.red[2][0];
            for (int i = 1; i < kRowWaves; ++i) {
                ls += S.red[0][i];
                cn += S.red[1][i];
                wr = max_nan(wr, S.red[2][i]);
            }
            // wr >= 0 or NaN: non-negative floats order like their bit patterns, and a NaN's pattern is above every number's
            atomicAdd(stats + 3 * b, s * ls);
            atomicAdd(stats + 3 * b + 1, cn);
            atomicMax(reinterpret_cast<unsigned *>(stats) + 3 * b + 2, __float_as_uint(wr));
        }
        __syncthreads();                                       // red is rewritten by the workgroup's next row
    }
}

// ---- the mixed step ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kRow) void psy_step_kernel(const float *cur, const float *__restrict__ g_ce,
                                                        const float *__restrict__ g_mask, const float *__restrict__ x, float *out,
                                                        int64_t B, int64_t T, float lambda, float step, float eps) {
    __shared__ float lds[2 * kRowWaves];
    for (int64_t row = blockIdx.x; row < B; row += gridDim.x) {
        const float *cr = cur + row * T, *gc = g_ce + row * T, *xr = x + row * T;
        float *orow = out + row * T;
        if (lambda == 0.0f) {                                  // launch-uniform: plain PGD
            map_rows<VEC>({cr, gc, xr}, orow, T,
                          [&](float c, float g, float xi) { return pgd_linf_elem(c, g, xi, step, eps, 0.0f, 1.0f); });
            continue;
        }
        const float *gm = g_mask + row * T;
        float m[2] = {0.0f, 0.0f};
        visit_rows<VEC>({gc, gm}, T, [&](float a, float bm) {
            m[0] += fabsf(a);
            m[1] += fabsf(bm);
        });
        row_reduce<2>(m, SumOp(), lds);
        const float m1 = m[0] / (float)T, m2 = m[1] / (float)T;
        map_rows<VEC>({cr, gc, gm, xr}, orow, T, [&](float c, float a, float bm, float xi) {
            float u = 0.0f;
            if (m1 != 0.0f) u = a / m1;
            if (m2 != 0.0f) u = u - lambda * (bm / m2);
            return pgd_linf_elem(c, u, xi, step, eps, 0.0f, 1.0f);
        });
    }
}

inline bool framing_ok(int64_t B, int64_t T, int64_t NF, int64_t hop, int64_t nfft) {
    return advstep_stft_bands_supported(nfft, hop, T) && NF == 1 + T / hop && T < (int64_t(1) << 30) &&
           B * NF <= (int64_t(1) << 40);
}

}  // namespace

extern "C" {

int advstep_stft_power_f32(const float *a, const float *b, const float *window, float *power, int64_t B, int64_t T, int64_t NF,
                           int64_t hop, int64_t nfft, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && NF >= 0);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(a && window && power && B <= kMaxGridY && framing_ok(B, T, NF, hop, nfft));
    const size_t in_bytes = (size_t)B * T * sizeof(float), out_bytes = (size_t)B * NF * kBins * sizeof(float);
    ADVSTEP_REQUIRE(!overlap2(power, out_bytes, a, in_bytes) && (!b || !overlap2(power, out_bytes, b, in_bytes)));
    const dim3 grid((unsigned)ceil_div(NF, kPowFrames), (unsigned)B);
    if (b)
        hipLaunchKernelGGL(stft_power_kernel<true>, grid, dim3(kPowWaves * 64), 0, as_stream(stream), a, b, window, power, (int)T,
                           (int)NF, (int)hop);
    else
        hipLaunchKernelGGL(stft_power_kernel<false>, grid, dim3(kPowWaves * 64), 0, as_stream(stream), a, b, window, power, (int)T,
                           (int)NF, (int)hop);
    return status_after_launch();
}

int advstep_masking_hinge_grad_f32(const float *adv, const float *x, const float *window, const float *theta,
                                   const float *row_scale, float *grad, float *stats, int64_t B, int64_t T, int64_t NF,
                                   int64_t hop, int64_t nfft, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && NF >= 0);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(adv && x && window && theta && row_scale && grad && stats && framing_ok(B, T, NF, hop, nfft));
    const size_t bytes = (size_t)B * T * sizeof(float), th_bytes = (size_t)B * NF * kBins * sizeof(float);
    const size_t st_bytes = (size_t)B * 3 * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(grad, adv, bytes) && !overlaps(grad, x, bytes) && !overlap2(grad, bytes, theta, th_bytes) &&
                    !overlap2(grad, bytes, stats, st_bytes) && !overlap2(stats, st_bytes, adv, bytes) &&
                    !overlap2(stats, st_bytes, x, bytes) && !overlap2(stats, st_bytes, theta, th_bytes));
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(grad, 0, bytes, st) != hipSuccess || hipMemsetAsync(stats, 0, st_bytes, st) != hipSuccess)
        return ADVSTEP_ELAUNCH;
    const size_t lds = sizeof(LdsHinge);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(masking_hinge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return ADVSTEP_ELAUNCH;
    hipLaunchKernelGGL(masking_hinge_kernel, dim3(kRowSplit, grid_rows(B)), dim3(kRow), lds, st, adv, x, window, theta, row_scale, grad, stats,
                       B, (int)T, (int)NF, (int)hop);
    return status_after_launch();
}

int advstep_psy_step_f32(const float *cur, const float *g_ce, const float *g_mask, const float *x, float lambda, float step,
                         float eps, float *out, int64_t B, int64_t T, advstep_stream_t stream) {
    ADVSTEP_REQUIRE(B >= 0 && T >= 0 && T < kMaxRowLength && lambda >= 0.0f && step >= 0.0f && eps >= 0.0f);
    if (B == 0) return ADVSTEP_OK;
    ADVSTEP_REQUIRE(T >= 1 && cur && g_ce && x && out && (g_mask || lambda == 0.0f));
    const size_t bytes = (size_t)B * T * sizeof(float);
    ADVSTEP_REQUIRE(!overlaps(out, g_ce, bytes) && !overlaps(out, x, bytes) && (!g_mask || !overlaps(out, g_mask, bytes)));
    return launch_rows(ROW_KERNEL_PAIR(psy_step_kernel), rows_vec(T, {cur, g_ce, g_mask, x, out}), B, stream, cur, g_ce, g_mask, x,
                       out, B, T, lambda, step, eps);
}

}  // extern "C"
