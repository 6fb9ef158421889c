// Fine-channel dual-pol power beams from live voltage beams (xengUpchanSumBeams*, upchan_beams.hip): the voltage beams that
// Beamform writes, cf32 [nchan][nbeam][ntime], cut into frames of N samples per (coarse channel, beam), each frame through the
// PFB front end (optional) and the register FFT of upchan_kernels.h, and the 2x2 products of beams 2p / 2p+1 summed over windows
// of frames.  Channelising after the beamformer is what UpchanBeamform computes with the coarse weights copied to every fine
// channel (beamforming, the PFB and the FFT are linear), with one FFT per beam instead of one per input.
//
// Contract (include/xeng.h, "Fine-channel power beams from live beams"):
//   in   cf32[nchan][nbeam][ntime]; pairs p in [pair0, pair0 + npair): X = beam 2p, Y = beam 2p+1
//   frame f = samples [f*N, f*N + N) of the gulp; PFB: y[f,n] = sum_k h[k*N + n] v[(f - P + 1 + k)*N + n], k ascending
//   fine channel j = (k + N/2) mod N of the forward, unnormalised FFT
//   out  f32[nwin][npair][nchan][N][4] = [XX, YY, Re XY*, Im XY*] summed over the frames of each window
//
// Decomposition: one work-group per (coarse channel, pair), all frames of the gulp, in passes of ft = blockDim / 2 frames:
//   stage    (PFB) the two rows' frames [f0 - P + 1, f0 + ft) into LDS, 16-byte loads consecutive across lanes (the taps
//            before the gulp from the history): a lane reading its P tap frames of 8N bytes itself touches 64 cache lines per
//            load instruction, P times over
//   phase A  lane 2f + pol owns frame f0 + f of beam 2p + pol: P tap frames from the stage through the PFB, or (plain FFT) its
//            N samples straight from memory in 16-byte loads; the FFT in registers (uc_fft on bit-reversed input).
//            Partner lanes swap half their spectrum (one xor-1 shuffle per float), so that lane X forms the products of fine
//            channels [0, N/2) and lane Y those of [N/2, N); the float4 products go to LDS, prod[f][j] (rows padded by one).
//   phase B  thread r < 4N owns one (fine channel, component) and adds the pass's frames to its sum in frame order; at the end
//            of a window the sum is written (or, for a window of G > 1 gulps, added to the gulp partials of the accumulator).
// Every sum is a fixed-order fp32 chain: frames in order within a gulp, the gulps' partial sums in order.  No atomics.
// With the PFB, the stage loop also copies the gulp's last P - 1 frames into the other half of a ping-pong history
// (hist_out), which the next gulp reads as hist_in: no D2D copies.
//
// upchan_beams.hip is compiled with -fno-slp-vectorize (Makefile), for the reason upchan.hip is.
#pragma once
#include "upchan_kernels.h"

namespace xeng {

// frames per pass at most: threads = 2 * ft <= 256, LDS (ub_lds_words) within 42 KB
__host__ __device__ constexpr int ub_max_frames(int N) { return N <= 16 ? 128 : 2048 / N; }

// float4 words of LDS before the twiddles: the products prod[ft][N + 1] float4, or (aliased) the stage of the two rows,
// [2][ft + P - 1][N + 2] float2, whichever is larger; the twiddles (32 float2) follow
__host__ __device__ constexpr int ub_lds_words(int N, int ft, int P) {
    return ft * (N + 1) > (ft + P - 1) * (N + 2) ? ft * (N + 1) : (ft + P - 1) * (N + 2);
}

// PFB front end (xengUpchanSumBeamsSetPfb): the kernel argument of the PFB instantiations
struct UbPfb {
    const float* h;             // [ntap][N] fp32 coefficients
    const float2* hist_in;      // [nchan][2 * npair][(ntap - 1) * N]: the samples right before the gulp (read when hist_valid)
    float2* hist_out;           // the same layout: this gulp's last (ntap - 1) * N samples (null when ntap = 1)
    int ntap;                   // 1 <= ntap <= UC_MAXTAP
    int hist_valid;             // 0: the samples before the gulp count as zero (hist_in is not read)
};

// grid: nchan * npair work-groups; blockDim = 2 * ft, a multiple of 64, ft <= ub_max_frames(N); dynamic LDS
// (ub_lds_words(N, ft, P) + 16) * 16 bytes.
// wf: frames per fp32 chain = min(nframe_sum, ntime / N), which divides ntime / N.  gpw: gulps per window (1: ntime / N / wf
// windows in this gulp, written to out); gpw > 1: this gulp is number pos of its window, its partial goes into acc (pos 0:
// acc = partial; then acc + partial), and the last one writes acc + partial to out (out is not touched otherwise).
template <int N, bool PFB>
__global__ __launch_bounds__(256) void upchan_sum_beams_kernel(const float2* __restrict__ in, float* __restrict__ out, float* __restrict__ acc, int nchan,
                                                               int nbeam, int ntime, int pair0, int npair, int wf, int gpw, int pos, UbPfb pfb) {
    extern __shared__ float4 ub_lds[];
    constexpr int NR = (4 * N + 63) / 64;                       // (fine channel, component) sums per thread at 64 threads
    constexpr int SP = N + 2;                                   // stage row pitch in float2 (16 bytes of padding per frame)
    const int tid = threadIdx.x, nthr = blockDim.x, ft = nthr >> 1;
    const int P = PFB ? pfb.ntap : 1, nfl = ft + P - 1;         // frames staged per row and pass: the pass's and the P-1 before
    float4* prod = ub_lds;                                      // [ft][N + 1], aliases stage
    float2* stage = reinterpret_cast<float2*>(ub_lds);          // [2][nfl][SP]
    float2* tw = reinterpret_cast<float2*>(ub_lds + ub_lds_words(N, ft, P));
    const int c = blockIdx.x / npair, p = blockIdx.x % npair;
    const int nframe = ntime / N, pol = tid & 1;
    const size_t nh = (size_t)(P - 1) * N;
    const size_t o0 = ((size_t)p * nchan + c) * N * 4;          // this (pair, channel) in a window of out / in acc
    if (tid < 32) {
        float s, co;
        sincospif(-(float)tid / 32.0f, &s, &co);
        tw[tid] = make_float2(co, s);
    }
    float sum[NR];
#pragma unroll
    for (int q = 0; q < NR; q++) sum[q] = 0.f;

    for (int f0 = 0; f0 < nframe; f0 += ft) {
        __syncthreads();                                        // (tw written; the previous pass's phase B done with prod)
        // ---- stage (PFB): frames [f0 - P + 1, f0 + ft) of beams X and Y, 16-byte loads consecutive across lanes; frames before
        // the gulp from the history (or zeros), frames past it zeros.  The gulp's last P - 1 frames also go to the next history.
        for (int r = 0; PFB && r < 2; r++) {
            const float2* row = in + ((size_t)c * nbeam + 2 * (pair0 + p) + r) * ntime;
            const size_t hrow = ((size_t)c * 2 * npair + 2 * p + r) * nh;
            for (int e = tid; e < nfl * (N / 2); e += nthr) {
                const int fl = e / (N / 2), n = 2 * (e % (N / 2)), fs = f0 - P + 1 + fl;
                float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
                if (fs >= 0 && fs < nframe) {
                    u = *reinterpret_cast<const float4*>(row + (size_t)fs * N + n);
                    if (PFB && fl >= P - 1 && fs >= nframe - (P - 1))
                        *reinterpret_cast<float4*>(pfb.hist_out + hrow + (size_t)(fs - (nframe - P + 1)) * N + n) = u;
                } else if (PFB && fs < 0 && pfb.hist_valid) {
                    u = *reinterpret_cast<const float4*>(pfb.hist_in + hrow + (size_t)(P - 1 + fs) * N + n);
                }
                *reinterpret_cast<float4*>(stage + ((size_t)r * nfl + fl) * SP + n) = u;
            }
        }
        if constexpr (PFB) __syncthreads();
        // ---- phase A: one frame per lane through the PFB (taps of frames outside the stream are staged zeros) and the FFT
        const int fi = tid >> 1, f = f0 + fi;
        float2 v[N];
        if constexpr (PFB) {
#pragma unroll
            for (int n = 0; n < N; n++) v[n] = make_float2(0.f, 0.f);
            for (int k = 0; k < P; k++) {
                const float2* src = stage + ((size_t)pol * nfl + fi + k) * SP;
                const float* hk = pfb.h + k * N;
#pragma unroll
                for (int n = 0; n < N; n += 2) {
                    const float4 u = *reinterpret_cast<const float4*>(src + n);
                    float2& y0 = v[uc_bitrev<N>(n)];
                    float2& y1 = v[uc_bitrev<N>(n + 1)];
                    y0.x = __builtin_fmaf(hk[n], u.x, y0.x);
                    y0.y = __builtin_fmaf(hk[n], u.y, y0.y);
                    y1.x = __builtin_fmaf(hk[n + 1], u.z, y1.x);
                    y1.y = __builtin_fmaf(hk[n + 1], u.w, y1.y);
                }
            }
        } else {
            // (the plain FFT reads each frame once: straight from memory, no stage and no barrier; measured 1.5 us less per gulp)
            const float2* src = in + ((size_t)c * nbeam + 2 * (pair0 + p) + pol) * ntime + (size_t)f * N;
#pragma unroll
            for (int n = 0; n < N; n += 2) {
                const float4 u = f < nframe ? *reinterpret_cast<const float4*>(src + n) : make_float4(0.f, 0.f, 0.f, 0.f);
                v[uc_bitrev<N>(n)] = make_float2(u.x, u.y);
                v[uc_bitrev<N>(n + 1)] = make_float2(u.z, u.w);
            }
        }
        uc_fft<N>(v, tw);
        if constexpr (PFB) __syncthreads();                     // (every lane done with stage: prod aliases it)
        // FFT bin k is fine channel (k + N/2) mod N: lane X keeps bins [N/2, N) (channels [0, N/2)) and sends [0, N/2); lane Y
        // keeps bins [0, N/2) (channels [N/2, N)) and sends [N/2, N)
        float4* dst = prod + fi * (N + 1) + pol * (N / 2);
#pragma unroll
        for (int i = 0; i < N / 2; i++) {
            const float2 mine = pol ? v[i] : v[i + N / 2];
            const float2 send = pol ? v[i + N / 2] : v[i];
            const float2 other = make_float2(__shfl_xor(send.x, 1), __shfl_xor(send.y, 1));
            const float2 X = pol ? other : mine, Y = pol ? mine : other;
            dst[i] = make_float4(__builtin_fmaf(X.x, X.x, X.y * X.y), __builtin_fmaf(Y.x, Y.x, Y.y * Y.y),
                                 __builtin_fmaf(X.x, Y.x, X.y * Y.y), __builtin_fmaf(X.y, Y.x, -(X.x * Y.y)));
        }
        __syncthreads();
        // ---- phase B: thread r = 4 j + component adds the pass's frames in order; windows end inside the pass
        const int f1 = min(f0 + ft, nframe);
        const float* pf = reinterpret_cast<const float*>(prod);
#pragma unroll
        for (int q = 0; q < NR; q++) {
            const int r = tid + q * nthr;
            if (r >= 4 * N) break;
            const float* col = pf + (r >> 2) * 4 + (r & 3);
            for (int fr = f0; fr < f1; fr++) {
                sum[q] += col[(fr - f0) * (N + 1) * 4];
                if ((fr + 1) % wf) continue;
                if (gpw == 1) {
                    out[(size_t)(fr / wf) * npair * nchan * N * 4 + o0 + r] = sum[q];
                } else {
                    const float t = pos > 0 ? acc[o0 + r] + sum[q] : sum[q];
                    if (pos == gpw - 1) out[o0 + r] = t;
                    else acc[o0 + r] = t;
                }
                sum[q] = 0.f;
            }
        }
    }
}

// Prime (xengUpchanSumBeamsPrime): hist_out <- the last nh samples of every selected (channel, beam) row of the gulp
__global__ __launch_bounds__(256) void upchan_sum_beams_prime_kernel(const float2* __restrict__ in, float2* __restrict__ hist_out, int nchan, int nbeam,
                                                                     int ntime, int pair0, int npair, int nh) {
    const long long total = (long long)nchan * 2 * npair * nh;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long rw = e / nh;
        const int t = (int)(e % nh);
        const int c = (int)(rw / (2 * npair)), bl = (int)(rw % (2 * npair));
        hist_out[e] = in[((size_t)c * nbeam + 2 * pair0 + bl) * ntime + (ntime - nh) + t];
    }
}

}  // namespace xeng
