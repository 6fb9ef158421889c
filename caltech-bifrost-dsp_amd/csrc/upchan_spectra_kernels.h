// Per-input fine-channel spectra (xengUpchanSpectra*, upchan_spectra.hip): 4+4-bit voltages -> nupchan-point FFT per frame,
// coarse channel and input -> |X|^2 and |X|^4 summed over the frames of a window, per input and fine channel.  The cheap
// diagnostic product next to UpchanBeamform's beams and UpchanCorr's visibilities: the fine-resolution bandpass of every input
// (S1) and, with S2, the spectral-kurtosis estimator (blocks/spectral_kurtosis.py).  The channelised data lives in registers only.
//
// Contract (include/xeng.h, "Per-input fine-channel spectra"):
//   in     u8 [ntime][nchan][ninput] (high nibble real, low nibble imaginary, two's complement; oracle.xeng_oracle.decode)
//   frame f = samples [f*N, f*N + N) of the gulp, N = nupchan in {1, 2, 4, 8, 16, 32, 64}
//   X[f,c,i,k] = sum_n x[f*N+n, c, i] exp(-2 pi i k n / N) (ucc_fft: forward, unnormalised, the twiddles 1 and -i exact); fine
//   channel j = (k + N/2) mod N
//   p = fmaf(re X, re X, im X * im X);  S1 = sum_f p,  S2 = sum_f p * p  over the W = nframe_sum frames of a window
//   out    f32 [nwin][2][nchan][N][ninput], plane 0 = S1, plane 1 = S2
//
// Decomposition: one work-group per (window, coarse channel, run of 64 consecutive inputs); wave s of its nslot waves is
// frame slot s, lane l is input l of the run, so the byte loads of a wave are 64 contiguous bytes per sample.  A thread walks
// the frames s, s + nslot, ... of the window: N byte loads, decode, radix-2 FFT in registers (ucc_fft, upchan_corr_kernels.h),
// S1[k] += p, S2[k] = fmaf(p, p, S2[k]) in 2N registers beside the FFT's 2N.  The slots are then added to slot 0 in slot order
// through LDS, and wave 0 writes S1 and S2 with stores contiguous over inputs.  With the PFB front end (a UcPfb argument) the
// frame's N samples are the PFB's y[n] (uc_pfb_frame, upchan_kernels.h), then the same FFT.
// Numerics: each output is one fixed sum -- per slot an fp32 chain over its frames in ascending order, the slots added as
// ((s0 + s1) + s2) + s3, nslot = min(US_DEFSLOT, frames per chain) -- that depends on the data and the configuration only: no atomics,
// nothing split across work-groups.  A window of several gulps: the same sum per gulp, the gulps' sums added in order in the
// context's accumulator (mode below), which round-trips through memory exactly.
//
// upchan_spectra.hip is compiled with -fno-slp-vectorize (Makefile), as upchan.hip is: the FFT is complex fp32 arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define UCC_FFT_ONLY            // ucc_fft without the correlator's kernels (their host stubs belong to upchan_corr.o)
#include "upchan_corr_kernels.h"

namespace xeng {

constexpr int US_LANES = 64;    // consecutive inputs per work-group: one wave per frame slot
constexpr int US_DEFSLOT = 4;   // frame slots (waves) per work-group unless the window has fewer frames
// the most slots a launch may have: 8 waves at up to 256 registers each (N = 64 holds 4N values per thread: 4 waves at up to 512)
constexpr int us_maxslot(int n) { return n <= 32 ? 8 : 4; }
constexpr size_t US_MAXROW = (size_t)1 << 24;   // bytes per sample, nchan * ninput, at most (Initialize refuses more): 32-bit sample offsets

// what a launch does with its sums: a window within the gulp goes straight to out; a window of G gulps is carried in acc
enum UsMode { US_OUT = 0, US_ASSIGN = 1, US_ADD = 2, US_FINISH = 3 };     // out = s | acc = s | acc = acc + s | out = acc + s

// grid: nwin * nchan * nxb work-groups of 64 * nslot threads, nxb = ninput / 64 rounded up; window w of the launch is frames
// [w * wf, (w + 1) * wf) of the gulp.  in1 / ntime0: samples [ntime0, ntime) are at in1 (a gulp in two spans; ntime0 % N == 0);
// one part: in1 = in0, ntime0 = ntime.  Modes other than US_OUT have nwin = 1 (wf = the gulp's frames) and address acc as out.
// Inputs i >= ninput are neither read nor written.  Pfb: empty (the plain FFT) or one UcPfb.
template <int N, typename... Pfb>
__global__ __launch_bounds__(US_LANES * us_maxslot(N)) void upchan_spectra_kernel(const uint8_t* __restrict__ in0, const uint8_t* __restrict__ in1,
                                                                                 int ntime0, float* __restrict__ out, float* __restrict__ acc, int nchan,
                                                                                 int ninput, int wf, int mode, Pfb... pfb) {
    constexpr bool PFB = sizeof...(Pfb) > 0;
    static_assert(sizeof...(Pfb) <= 1, "one UcPfb at most");
    __shared__ float2 tw[32];
    __shared__ float red[2 * N * US_LANES];                     // one slot's S1[N], S2[N] per lane: [2N][64]
    const int tid = threadIdx.x, lane = tid & (US_LANES - 1), slot = tid / US_LANES, nslot = blockDim.x / US_LANES;
    if (N >= 8 && tid < 32) {
        float s, co;
        sincospif(-(float)tid / 32.0f, &s, &co);
        tw[tid] = make_float2(co, s);
    }
    __syncthreads();
    const int nxb = (ninput + US_LANES - 1) / US_LANES;
    const int lid = uc_logical_block(blockIdx.x, gridDim.x);   // (the runs of one channel next to each other on one XCD: they share cache lines)
    const int xb = lid % nxb, rest = lid / nxb;
    const int c = rest % nchan, w = rest / nchan;
    const int i = xb * US_LANES + lane;
    const bool live = i < ninput;
    float s1[N], s2[N];                                         // indexed by the FFT's k
#pragma unroll
    for (int k = 0; k < N; k++) s1[k] = s2[k] = 0.f;
    if (live) {
        const size_t row = (size_t)nchan * ninput;              // bytes per sample
        const size_t off = (size_t)c * ninput + i;
        __builtin_assume(row <= US_MAXROW);                     // (n * row stays 32-bit: without it the N sample offsets take 2N SGPRs)
        const int f1 = (w + 1) * wf;
        for (int f = w * wf + slot; f < f1; f += nslot) {
            float2 v[N];
            if constexpr (PFB) {
                uc_pfb_frame<N>(v, in0, in1, ntime0, f, row, off, pfb...);
            } else {
                const int t0 = f * N;
                const uint8_t* p = (t0 < ntime0 ? in0 + (size_t)t0 * row : in1 + (size_t)(t0 - ntime0) * row) + off;
#pragma unroll
                for (int n = 0; n < N; n++) {
                    const uint32_t u = p[(size_t)n * row];
                    v[uc_bitrev<N>(n)] = make_float2(uc_hi(u), uc_lo(u));
                }
            }
            ucc_fft<N>(v, tw);
#pragma unroll
            for (int k = 0; k < N; k++) {
                const float p = __builtin_fmaf(v[k].x, v[k].x, v[k].y * v[k].y);
                s1[k] += p;
                s2[k] = __builtin_fmaf(p, p, s2[k]);
            }
        }
    }
    // slots 1 .. nslot-1 into slot 0, in slot order (the barriers are reached by every thread)
    for (int s = 1; s < nslot; s++) {
        if (slot == s) {
#pragma unroll
            for (int k = 0; k < N; k++) {
                red[k * US_LANES + lane] = s1[k];
                red[(N + k) * US_LANES + lane] = s2[k];
            }
        }
        __syncthreads();
        if (slot == 0) {
#pragma unroll
            for (int k = 0; k < N; k++) {
                s1[k] += red[k * US_LANES + lane];
                s2[k] += red[(N + k) * US_LANES + lane];
            }
        }
        __syncthreads();
    }
    if (slot != 0 || !live) return;
    const size_t plane = (size_t)nchan * N * ninput;
    float* dst = (mode == US_OUT || mode == US_FINISH) ? out : acc;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const int k = (j + N / 2) % N;
        const size_t o = (((size_t)w * 2 * nchan + c) * N + j) * ninput + i;
        float a1 = s1[k], a2 = s2[k];
        if (mode >= US_ADD) {
            a1 = acc[o] + a1;
            a2 = acc[o + plane] + a2;
        }
        dst[o] = a1;
        dst[o + plane] = a2;
    }
}

}  // namespace xeng
