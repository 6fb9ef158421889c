// Upchannelising beamformer (xengUpchan*, upchan.hip): 4+4-bit voltages -> nupchan-point FFT per coarse channel and input ->
// per-fine-channel weights -> sum over inputs -> voltage beams, or their power summed over frames, in ONE kernel.  The
// channelised data lives in registers and LDS only (lwa352-upchan-bf.py:94-113 with beamform_offline_block.py:211-245 do the
// same in five bifrost blocks with the FFT output in device memory).
//
// Contract (include/xeng.h, "Upchannelising beamformer"):
//   in   u8 [ntime][nchan][ninput] (high nibble real, low nibble imaginary, two's complement; oracle.xeng_oracle.decode)
//   frame f = samples [f*N, f*N + N) of the gulp, N = nupchan
//   X[f,c,i,k] = sum_n x[f*N+n, c, i] exp(-2 pi i k n / N)     (forward, unnormalised), fine channel j = (k + N/2) mod N
//   w    cf32[nchan][N][nbeam][ninput]  (indexed by j)
//   voltage: out cf32[nframe][nbeam][nchan][N],        v[f,b,c,j] = sum_i w[c,j,b,i] X[f,c,i,j]
//   power:   out f32 [nframe/nframe_sum][nbeam][nchan][N], sum of |v|^2 over nframe_sum consecutive frames
//   dual-pol: out f32 [nframe/nframe_sum][nbeam/2][nchan][N][4], [XX, YY, Re(XY*), Im(XY*)] of X = v[.,2p,.], Y = v[.,2p+1,.]
//
// Decomposition: one work-group per (coarse channel c, run of frames).  It walks the inputs in chunks of UC_IC:
//   phase A  one thread per (frame, input) of the chunk: N byte loads, decode, radix-2 FFT in registers, the N outputs to LDS
//            in fine-channel order (xs[frame][input][j], rows padded by one word against bank conflicts); with the PFB front end
//            (a UcPfb argument, xengUpchanSetPfb) ntap * N byte loads, the tap frames weighted into the FFT's input (uc_pfb_frame)
//   phase B  thread t owns fine channel j = t % N and beams b = t / N + q * (blockDim / N), q < PPT, for UC_FT frames: its
//            accumulators stay in registers across all chunks, its weights w[c][j][b][chunk] come straight from memory (16 B
//            loads, each weight read once per work-group), X[f][i][j] from LDS (one read serves every beam of the thread);
//            dual-pol (DUAL): PPT / 2 whole pairs instead, beams 2p and 2p+1 of p = t / N + q * (blockDim / N), q < PPT / 2, so the
//            2x2 products of a pair are formed in the registers that hold both voltages
// The sum over inputs is a fixed-order fp32 FMA chain per output (chunk by chunk, input by input): no atomics, no
// scheduling-dependent order, so results are bit-identical from run to run.  A work-group's run of frames is a whole
// number of power windows (the host picks it), so detection and integration finish in the same registers.  The voltage chain
// and the |v|^2 chain of a beam do not depend on the thread that owns it, so XX / YY of pair p are the power mode's outputs of
// beams 2p / 2p+1, bit for bit; the cross terms are a fixed-order chain of their own (BeamformSumBeams's convention,
// oracle orc_beamform_integrate: Re += xr*yr + xi*yi, Im += xi*yr - xr*yi, frame by frame).
//
// upchan.hip is compiled with -fno-slp-vectorize (Makefile): otherwise hipcc packs the complex products into the
// op_sel:[0,1] VOP3P form of DESIGN.md 4.10, which tests/test_isa_rules.py refuses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

constexpr int UC_FT = 8;        // frames per sub-tile (accumulators per beam and thread)
constexpr int UC_IC = 16;       // inputs per chunk (phase A items = UC_FT * UC_IC = 128)
constexpr int UC_MAXB = 1024;   // nbeam * nupchan per work-group: blockDim <= 256 threads x PPT <= 4
constexpr int UC_MAXTAP = 8;    // PFB taps (xengUpchanSetPfb, xengUpchanCorrSetPfb)

// twiddles exp(-2 pi i k / 64), k < 32: every N in {8, 16, 32, 64} reads its own as tw[k * 64 / N]
__device__ __forceinline__ float2 uc_tw(const float2* tw, int k64) { return tw[k64]; }

template <int N>
__device__ __forceinline__ void uc_fft(float2 (&v)[N], const float2* tw) {
    // iterative radix-2 decimation in time on bit-reversed input; indices are compile-time after unrolling
#pragma unroll
    for (int len = 2; len <= N; len <<= 1) {
        const int half = len >> 1;
#pragma unroll
        for (int s = 0; s < N; s += len) {
#pragma unroll
            for (int k = 0; k < half; k++) {
                const float2 w = uc_tw(tw, k * (64 / len));
                const float2 a = v[s + k], b = v[s + k + half];
                const float br = __builtin_fmaf(b.x, w.x, -b.y * w.y);
                const float bi = __builtin_fmaf(b.x, w.y, b.y * w.x);
                v[s + k] = make_float2(a.x + br, a.y + bi);
                v[s + k + half] = make_float2(a.x - br, a.y - bi);
            }
        }
    }
}

template <int N>
__host__ __device__ constexpr int uc_bitrev(int n) {
    int r = 0;
    for (int m = 1; m < N; m <<= 1) { r = (r << 1) | (n & 1); n >>= 1; }
    return r;
}

__device__ __forceinline__ float uc_hi(uint32_t u) { return (float)((int32_t)(u << 24) >> 28); }
__device__ __forceinline__ float uc_lo(uint32_t u) { return (float)((int32_t)(u << 28) >> 28); }

// PFB front end (xengUpchanSetPfb, xengUpchanCorrSetPfb): the kernel argument of the PFB instantiations
struct UcPfb {
    const float* h;             // [ntap][N] fp32 coefficients
    const uint8_t* hist;        // u8 [(ntap - 1) * N][nchan][ninput]: the samples right before the gulp (null when ntap = 1)
    int ntap;                   // 1 <= ntap <= UC_MAXTAP
    int hist_valid;             // 0: the samples before the gulp count as zero (hist is not read)
};

// One (frame, input) item through the PFB: v[bitrev(n)] = y[n] = sum_k h[k*N + n] x[(fg - ntap + 1 + k)*N + n], k ascending, one
// fp32 fmaf chain per component from zero.  Tap frames before the gulp (fs < 0) come from hist (frame fs = its samples
// [(ntap - 1 + fs) * N, +N)), or are skipped as zeros without hist_valid.  Gulp frames are N-aligned and each part holds whole
// frames, so every tap frame lies wholly in hist, in0 or in1.  h is read at wave-uniform addresses; `off` is the byte offset of
// (channel, input) within a sample.
template <int N>
__device__ __forceinline__ void uc_pfb_frame(float2 (&v)[N], const uint8_t* __restrict__ in0, const uint8_t* __restrict__ in1, int ntime0,
                                             int fg, size_t row, size_t off, const UcPfb& q) {
#pragma unroll
    for (int n = 0; n < N; n++) v[n] = make_float2(0.f, 0.f);
    for (int k = 0; k < q.ntap; k++) {
        const int fs = fg - q.ntap + 1 + k;
        const uint8_t* p;
        if (fs >= 0) {
            const int t0 = fs * N;
            p = t0 < ntime0 ? in0 + (size_t)t0 * row : in1 + (size_t)(t0 - ntime0) * row;
        } else if (q.hist_valid) {
            p = q.hist + (size_t)((q.ntap - 1 + fs) * N) * row;
        } else {
            continue;
        }
        p += off;
        const float* hk = q.h + k * N;
#pragma unroll
        for (int n = 0; n < N; n++) {
            const uint32_t u = p[(size_t)n * row];
            const float c = hk[n];
            float2& y = v[uc_bitrev<N>(n)];
            y.x = __builtin_fmaf(c, uc_hi(u), y.x);
            y.y = __builtin_fmaf(c, uc_lo(u), y.y);
        }
    }
}

// Work-group -> (channel, frame run) with the runs of one channel on one XCD group, next to each other in time: they read the
// same weights (cdna_hip_programming T1 remap, bijective for any count; a speed choice only).
__device__ __forceinline__ int uc_logical_block(int bid, int nwg) {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, local = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
}

// grid: nchan * ceil(nframe / run) work-groups; blockDim a multiple of 64 and of N, <= 256, with blockDim * PPT >= nbeam * N.
// in1 / ntime0: samples [ntime0, ntime) are at in1 (a gulp in two spans; ntime0 % N == 0); one part: in1 = in0, ntime0 = ntime.
// run: frames per work-group (UC_FT in voltage mode; in power mode a whole number of nframe_sum windows).
// DUAL (nframe_sum > 0, nbeam even, PPT even): PPT / 2 pairs per thread, blockDim * PPT / 2 >= nbeam / 2 * N.
// Pfb: empty -- the plain FFT, with the parameter list (and so the code) the kernel had before the PFB existed -- or one UcPfb,
// the PFB front end: phase A forms y[n] of uc_pfb_frame before the FFT; phase B and the epilogues are the same.
template <int N, int PPT, bool DUAL = false, typename... Pfb>
__global__ __launch_bounds__(256) void upchan_beamform_kernel(const uint8_t* __restrict__ in0, const uint8_t* __restrict__ in1, int ntime0,
                                                              const float2* __restrict__ w, float* __restrict__ out, int nchan, int ninput,
                                                              int nbeam, int nframe, int nframe_sum, int run, Pfb... pfb) {
    constexpr bool PFB = sizeof...(Pfb) > 0;
    static_assert(sizeof...(Pfb) <= 1, "one UcPfb at most");
    constexpr int P = N + 1;                                    // LDS row pitch in float2
    __shared__ float2 xs[UC_FT * UC_IC * P];
    __shared__ float2 tw[32];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int ngrp = (nframe + run - 1) / run;
    const int lid = uc_logical_block(blockIdx.x, nchan * ngrp);
    const int c = lid / ngrp, r0 = (lid % ngrp) * run;
    const int r1 = min(r0 + run, nframe);
    if (tid < 32) {
        float s, co;
        sincospif(-(float)tid / 32.0f, &s, &co);
        tw[tid] = make_float2(co, s);
    }
    static_assert(!DUAL || PPT % 2 == 0, "dual-pol threads own whole pairs");
    const int j = tid % N, b0 = tid / N, bs = nthr / N;
    const size_t row = (size_t)nchan * ninput;                  // bytes per sample
    float pw[PPT];                                              // |v|^2 of beam q (XX / YY of pair q / 2 when DUAL)
    float px[DUAL ? PPT : 1];                                   // Re / Im of X conj(Y) of pair q / 2 (DUAL)
#pragma unroll
    for (int q = 0; q < PPT; q++) pw[q] = 0.f;
#pragma unroll
    for (int q = 0; q < (DUAL ? PPT : 1); q++) px[q] = 0.f;

    for (int s0 = r0; s0 < r1; s0 += UC_FT) {
        float2 acc[PPT][UC_FT];
#pragma unroll
        for (int q = 0; q < PPT; q++)
#pragma unroll
            for (int f = 0; f < UC_FT; f++) acc[q][f] = make_float2(0.f, 0.f);

        for (int i0 = 0; i0 < ninput; i0 += UC_IC) {
            __syncthreads();                                    // (previous chunk's phase B done with xs; tw written)
            // ---- phase A: FFT of (frame, input) items into xs[f][ii][j]
            for (int item = tid; item < UC_FT * UC_IC; item += nthr) {
                const int f = item / UC_IC, ii = item % UC_IC;
                const int fg = s0 + f, i = i0 + ii;
                float2 v[N];
                if (fg < r1 && i < ninput) {
                    if constexpr (PFB) {
                        uc_pfb_frame<N>(v, in0, in1, ntime0, fg, row, (size_t)c * ninput + i, pfb...);
                    } else {
                        const int t0 = fg * N;
                        const uint8_t* p = t0 < ntime0 ? in0 + (size_t)t0 * row : in1 + (size_t)(t0 - ntime0) * row;
                        p += (size_t)c * ninput + i;
#pragma unroll
                        for (int n = 0; n < N; n++) {
                            const uint32_t u = p[(size_t)n * row];
                            v[uc_bitrev<N>(n)] = make_float2(uc_hi(u), uc_lo(u));
                        }
                    }
                    uc_fft<N>(v, tw);
                } else {
#pragma unroll
                    for (int n = 0; n < N; n++) v[n] = make_float2(0.f, 0.f);
                }
                float2* dst = xs + (f * UC_IC + ii) * P;
#pragma unroll
                for (int jj = 0; jj < N; jj++) dst[jj] = v[(jj + N / 2) % N];
            }
            __syncthreads();
            // ---- phase B: acc[q][f] += w[c][j][b_q][i] * X[f][i][j]
            const int nin = min(UC_IC, ninput - i0);            // a multiple of 4 (ninput % 4 == 0)
#pragma unroll
            for (int i2 = 0; i2 < UC_IC; i2 += 2) {
                if (i2 >= nin) break;
                float4 wv[PPT];
#pragma unroll
                for (int q = 0; q < PPT; q++) {
                    const int b = DUAL ? 2 * (b0 + (q >> 1) * bs) + (q & 1) : b0 + q * bs;
                    wv[q] = b < nbeam ? *reinterpret_cast<const float4*>(w + (((size_t)c * N + j) * nbeam + b) * ninput + i0 + i2)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int h = 0; h < 2; h++) {
#pragma unroll
                    for (int f = 0; f < UC_FT; f++) {
                        const float2 x = xs[(f * UC_IC + i2 + h) * P + j];
#pragma unroll
                        for (int q = 0; q < PPT; q++) {
                            const float wr = h ? wv[q].z : wv[q].x, wi = h ? wv[q].w : wv[q].y;
                            acc[q][f].x = __builtin_fmaf(wr, x.x, acc[q][f].x);
                            acc[q][f].x = __builtin_fmaf(-wi, x.y, acc[q][f].x);
                            acc[q][f].y = __builtin_fmaf(wr, x.y, acc[q][f].y);
                            acc[q][f].y = __builtin_fmaf(wi, x.x, acc[q][f].y);
                        }
                    }
                }
            }
        }
        // ---- epilogue of the sub-tile: voltages, or |v|^2 into the window sums
        if constexpr (DUAL) {
#pragma unroll
            for (int q = 0; q < PPT; q += 2) {
                const int p = b0 + (q >> 1) * bs;
                if (2 * p >= nbeam) continue;
#pragma unroll
                for (int f = 0; f < UC_FT; f++) {
                    const int fg = s0 + f;
                    if (fg >= r1) break;
                    const float2 X = acc[q][f], Y = acc[q + 1][f];
                    pw[q] = __builtin_fmaf(X.x, X.x, pw[q]);
                    pw[q] = __builtin_fmaf(X.y, X.y, pw[q]);
                    pw[q + 1] = __builtin_fmaf(Y.x, Y.x, pw[q + 1]);
                    pw[q + 1] = __builtin_fmaf(Y.y, Y.y, pw[q + 1]);
                    px[q] = __builtin_fmaf(X.x, Y.x, px[q]);
                    px[q] = __builtin_fmaf(X.y, Y.y, px[q]);
                    px[q + 1] = __builtin_fmaf(X.y, Y.x, px[q + 1]);
                    px[q + 1] = __builtin_fmaf(-X.x, Y.y, px[q + 1]);
                    if ((fg + 1) % nframe_sum == 0) {
                        reinterpret_cast<float4*>(out)[(((size_t)(fg / nframe_sum) * (nbeam >> 1) + p) * nchan + c) * N + j] =
                            make_float4(pw[q], pw[q + 1], px[q], px[q + 1]);
                        pw[q] = pw[q + 1] = px[q] = px[q + 1] = 0.f;
                    }
                }
            }
            continue;
        }
#pragma unroll
        for (int q = 0; q < PPT; q++) {
            const int b = b0 + q * bs;
            if (b >= nbeam) continue;
#pragma unroll
            for (int f = 0; f < UC_FT; f++) {
                const int fg = s0 + f;
                if (fg >= r1) break;
                if (nframe_sum == 0) {
                    reinterpret_cast<float2*>(out)[(((size_t)fg * nbeam + b) * nchan + c) * N + j] = acc[q][f];
                } else {
                    pw[q] = __builtin_fmaf(acc[q][f].x, acc[q][f].x, pw[q]);
                    pw[q] = __builtin_fmaf(acc[q][f].y, acc[q][f].y, pw[q]);
                    if ((fg + 1) % nframe_sum == 0) {
                        out[(((size_t)(fg / nframe_sum) * nbeam + b) * nchan + c) * N + j] = pw[q];
                        pw[q] = 0.f;
                    }
                }
            }
        }
    }
}

}  // namespace xeng
