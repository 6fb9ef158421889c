// Upchannelised correlator (xengUpchanCorr*, upchan_corr.hip): 4+4-bit voltages -> nupchan-point FFT per frame, coarse channel
// and input -> a selected range of fine channels -> V[c', i, j] = sum_f X[f, i] conj(X[f, j]) accumulated over frames.  The
// reference does it with blocks.fft, FrequencySelectBlock and blocks.correlate (lwa352-upchan-imag.py:95-106).
//
// Contract (include/xeng.h, "Upchannelised correlator"):
//   in     u8 [ntime][nchan][ninput] (high nibble real, low nibble imaginary, two's complement; oracle.xeng_oracle.decode)
//   frame f = samples [f*N, f*N + N) of the gulp, N = nupchan in {1, 2, 4, 8, 16, 32, 64}
//   X[f,c,i,k] = sum_n x[f*N+n, c, i] exp(-2 pi i k n / N) (forward, unnormalised); fine channel j = (k + N/2) mod N, merged
//   index c*N + j; fine channels [fine_lo, fine_hi) are kept, c' = c*N + j - fine_lo
//   out    cf32 [nfine][ninput][ninput], the full Hermitian matrix
//
// Three kernels, all on one stream:
//   stage     one thread per (coarse channel, frame, input): N byte loads, decode, radix-2 FFT in registers, the selected fine
//             channels to stage[c'][frame][input] (fp32 re/im pairs, inputs padded with zeros to a multiple of 32, frames of a
//             gulp padded with a zero frame to an even count).  A gulp goes to one of nstage slots of frames.  With the PFB front
//             end (xengUpchanCorrSetPfb) ntap * N byte loads weighted into the FFT's input (uc_pfb_frame, upchan_kernels.h).
//   contract  one wave per (fine channel, 32x32 tile pair ti >= tj of inputs): the accumulator tile (Re and Im, 16 registers
//             each) from memory; per staged gulp v_mfma_f32_32x32x2_f32 over its frames two at a time, in frame order, from a
//             zero C: Re += Xr_i Xr_j, Re += Xi_i Xi_j, Im += Xi_i Xr_j, Im += (-Xr_i) Xi_j; that gulp's sum added to the
//             tile; the tile back to memory.
//   dump      one work-group per (fine channel, 32x32 output tile): the lower-triangle tile that holds it through LDS, the
//             upper triangle as its exact conjugate, diagonal imaginary parts written as 0.
// Numerics: an f32-input MFMA is a k-ordered fmaf chain, a zero pad frame adds fma(0, 0, C) = C, the frames of one gulp always
// pair up the same way, and the accumulator round-trips through memory exactly: each visibility is one fixed sum -- per gulp
// an fmaf chain over its frames, the gulps added in order -- whatever the number of gulps staged per contraction.  No
// atomics, nothing split across work-groups.
//
// upchan_corr.hip is compiled with -fno-slp-vectorize (Makefile), as upchan.hip is: the FFT is complex fp32 arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "upchan_kernels.h"

namespace xeng {

constexpr int UCC_T = 32;       // inputs per tile side (the 32x32 MFMA)
constexpr int UCC_SB = 256;     // stage kernel: inputs per work-group
constexpr int UCC_WPB = 4;      // contract kernel: waves (tile pairs) per work-group

typedef float ucc_f32x16 __attribute__((ext_vector_type(16)));

// uc_fft with the twiddles 1 and -i applied exactly (a table's cos(pi/2) is -4.4e-8, not 0): every butterfly of N <= 4 is
// exact on integer data, and the other twiddles come from the table as in uc_fft.
template <int N>
__device__ __forceinline__ void ucc_fft(float2 (&v)[N], const float2* tw) {
#pragma unroll
    for (int len = 2; len <= N; len <<= 1) {
        const int half = len >> 1;
#pragma unroll
        for (int s = 0; s < N; s += len) {
#pragma unroll
            for (int k = 0; k < half; k++) {
                const int k64 = k * (64 / len);
                const float2 a = v[s + k], b = v[s + k + half];
                float br, bi;
                if (k64 == 0) {                 // w = 1
                    br = b.x;
                    bi = b.y;
                } else if (k64 == 16) {         // w = exp(-i pi/2) = -i
                    br = b.y;
                    bi = -b.x;
                } else {
                    const float2 w = uc_tw(tw, k64);
                    br = __builtin_fmaf(b.x, w.x, -b.y * w.y);
                    bi = __builtin_fmaf(b.x, w.y, b.y * w.x);
                }
                v[s + k] = make_float2(a.x + br, a.y + bi);
                v[s + k + half] = make_float2(a.x - br, a.y - bi);
            }
        }
    }
}

#ifndef UCC_FFT_ONLY     // (defined by a translation unit that wants ucc_fft alone: upchan_spectra_kernels.h)
// tile pair index tp = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void ucc_tile_pair(int tp, int& ti, int& tj) {
    int t = (int)((sqrtf(8.0f * (float)tp + 1.0f) - 1.0f) * 0.5f);
    while (t * (t + 1) / 2 > tp) t--;
    while ((t + 1) * (t + 2) / 2 <= tp) t++;
    ti = t;
    tj = tp - t * (t + 1) / 2;
}

// position of element (row, col) of a 32x32 accumulator tile in its [register][lane] image (C/D map of the 32x32 MFMA:
// col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
__device__ __forceinline__ int ucc_acc_index(int row, int col) {
    return ((row & 3) + 4 * (row >> 3)) * 64 + col + 32 * ((row >> 2) & 1);
}

// grid: nxb * nfp * (c_hi - c_lo) work-groups of UCC_SB threads, nxb = npad / UCC_SB rounded up; coarse channels [c_lo, c_hi)
// are those that hold a selected fine channel.  Frame f of the gulp goes to stage frame frame0 + f; frames f >= nframe (the
// pad frame) and inputs i >= ninput are written as zeros.  Pfb: empty (the plain FFT, the kernel as it was before the PFB
// existed) or one UcPfb (upchan_kernels.h): the item's N samples are the PFB's y[n] (uc_pfb_frame), then the same FFT.
template <int N, typename... Pfb>
__global__ __launch_bounds__(UCC_SB) void upchan_corr_stage_kernel(const uint8_t* __restrict__ in0, const uint8_t* __restrict__ in1, int ntime0,
                                                                   float2* __restrict__ stage, int nchan, int ninput, int npad, int nframe, int nfp,
                                                                   size_t fine_stride, int frame0, int fine_lo, int fine_hi, int c_lo, Pfb... pfb) {
    constexpr bool PFB = sizeof...(Pfb) > 0;
    static_assert(sizeof...(Pfb) <= 1, "one UcPfb at most");
    __shared__ float2 tw[32];
    const int tid = threadIdx.x;
    if (N >= 8 && tid < 32) {
        float s, co;
        sincospif(-(float)tid / 32.0f, &s, &co);
        tw[tid] = make_float2(co, s);
    }
    __syncthreads();
    const int nxb = (npad + UCC_SB - 1) / UCC_SB;
    const int xb = blockIdx.x % nxb, rest = blockIdx.x / nxb;
    const int f = rest % nfp, c = c_lo + rest / nfp;
    const int i = xb * UCC_SB + tid;
    if (i >= npad) return;
    float2 v[N];
    if (f < nframe && i < ninput) {
        const size_t row = (size_t)nchan * ninput;               // bytes per sample
        if constexpr (PFB) {
            uc_pfb_frame<N>(v, in0, in1, ntime0, f, row, (size_t)c * ninput + i, pfb...);
        } else {
            const int t0 = f * N;
            const uint8_t* p = t0 < ntime0 ? in0 + (size_t)t0 * row : in1 + (size_t)(t0 - ntime0) * row;
            p += (size_t)c * ninput + i;
#pragma unroll
            for (int n = 0; n < N; n++) {
                const uint32_t u = p[(size_t)n * row];
                v[uc_bitrev<N>(n)] = make_float2(uc_hi(u), uc_lo(u));
            }
        }
        ucc_fft<N>(v, tw);
    } else {
#pragma unroll
        for (int n = 0; n < N; n++) v[n] = make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int jj = 0; jj < N; jj++) {
        const int fine = c * N + jj;
        if (fine >= fine_lo && fine < fine_hi)
            stage[(size_t)(fine - fine_lo) * fine_stride + (size_t)(frame0 + f) * npad + i] = v[(jj + N / 2) % N];
    }
}

// grid: ceil(nfine * ntp / UCC_WPB) work-groups of 64 * UCC_WPB threads; wave w of logical work-group g takes item
// g * UCC_WPB + w = (fine channel, tile pair).  ngulp staged gulps of nfp (even) frames are summed, gulp by gulp, into
// acc[fine][tp][Re, Im][16][64]; with fresh set the sum starts from zero instead of the stored tile.
__global__ __launch_bounds__(64 * UCC_WPB) void upchan_corr_mfma_kernel(const float2* __restrict__ stage, float* __restrict__ acc, int nfine,
                                                                       int ntp, int npad, size_t fine_stride, int ngulp, int nfp, int fresh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int item = uc_logical_block(blockIdx.x, gridDim.x) * UCC_WPB + wave;
    if (item >= nfine * ntp) return;                             // (a whole wave; the kernel has no barrier)
    const int fine = item / ntp, tp = item % ntp;
    int ti, tj;
    ucc_tile_pair(tp, ti, tj);
    const int r = lane & 31, h = lane >> 5;
    // lane (r, h) supplies A[row r][k = h] = X[frame f0 + h][ti*32 + r] and B[k = h][col r] = X[f0 + h][tj*32 + r]
    const float2* xa = stage + (size_t)fine * fine_stride + (size_t)h * npad + ti * UCC_T + r;
    const float2* xb = stage + (size_t)fine * fine_stride + (size_t)h * npad + tj * UCC_T + r;
    const size_t step = 2 * (size_t)npad;                       // two frames
    float* a = acc + ((size_t)fine * ntp + tp) * 2048;
    ucc_f32x16 cre, cim;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        cre[v] = fresh ? 0.f : a[v * 64 + lane];
        cim[v] = fresh ? 0.f : a[1024 + v * 64 + lane];
    }
    for (int g = 0; g < ngulp; g++) {
        // the gulp's frames from zero (tre, tim), then added to the running sum: a gulp-sized fmaf chain per element
        // (sequential chains over thousands of frames lose up to 3e-6 of sum |X_i||X_j|, this 2e-7: DESIGN.md 4.12)
        ucc_f32x16 tre = {}, tim = {};
        int f0 = 0;
        for (; f0 + 8 <= nfp; f0 += 8) {                         // four frame pairs: the loads first, then 16 MFMAs
            float2 pa[4], pb[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                pa[q] = xa[q * step];
                pb[q] = xb[q * step];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                tre = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[q].x, pb[q].x, tre, 0, 0, 0);
                tim = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[q].y, pb[q].x, tim, 0, 0, 0);
                tre = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[q].y, pb[q].y, tre, 0, 0, 0);
                tim = __builtin_amdgcn_mfma_f32_32x32x2f32(-pa[q].x, pb[q].y, tim, 0, 0, 0);
            }
            xa += 4 * step;
            xb += 4 * step;
        }
        for (; f0 < nfp; f0 += 2) {
            const float2 pa = xa[0], pb = xb[0];
            tre = __builtin_amdgcn_mfma_f32_32x32x2f32(pa.x, pb.x, tre, 0, 0, 0);
            tim = __builtin_amdgcn_mfma_f32_32x32x2f32(pa.y, pb.x, tim, 0, 0, 0);
            tre = __builtin_amdgcn_mfma_f32_32x32x2f32(pa.y, pb.y, tre, 0, 0, 0);
            tim = __builtin_amdgcn_mfma_f32_32x32x2f32(-pa.x, pb.y, tim, 0, 0, 0);
            xa += step;
            xb += step;
        }
#pragma unroll
        for (int v = 0; v < 16; v++) {
            cre[v] += tre[v];
            cim[v] += tim[v];
        }
    }
#pragma unroll
    for (int v = 0; v < 16; v++) {
        a[v * 64 + lane] = cre[v];
        a[1024 + v * 64 + lane] = cim[v];
    }
}

// grid: nfine * ntile * ntile work-groups of 256 threads, one per (fine channel, output tile oi, oj).  Output tiles on or below
// the diagonal copy the accumulator tile (oi, oj); those above it read tile (oj, oi) transposed and conjugated.  With fresh
// set (nothing contracted since the last reset) zeros are written.  Rows and columns >= ninput are not written.
__global__ __launch_bounds__(256) void upchan_corr_dump_kernel(const float* __restrict__ acc, float2* __restrict__ out, int ninput, int ntile,
                                                               int ntp, int fresh) {
    __shared__ float s[2048];
    const int tid = threadIdx.x;
    const int per = ntile * ntile;
    const int fine = blockIdx.x / per, rest = blockIdx.x % per;
    const int oi = rest / ntile, oj = rest % ntile;
    const int si = oi >= oj ? oi : oj, sj = oi >= oj ? oj : oi;
    const float* a = acc + ((size_t)fine * ntp + si * (si + 1) / 2 + sj) * 2048;
    for (int e = tid; e < 2048; e += 256) s[e] = fresh ? 0.f : a[e];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int e = tid + 256 * q;
        const int rr = e >> 5, cc = e & 31;
        const int i = oi * UCC_T + rr, j = oj * UCC_T + cc;
        if (i >= ninput || j >= ninput) continue;
        const bool lower = oi > oj || (oi == oj && rr >= cc);
        const int idx = lower ? ucc_acc_index(rr, cc) : ucc_acc_index(cc, rr);
        float re = s[idx], im = s[1024 + idx];
        if (!lower) im = -im;
        if (i == j) im = 0.f;
        out[((size_t)fine * ninput + i) * ninput + j] = make_float2(re, im);
    }
}

#endif  // UCC_FFT_ONLY

}  // namespace xeng
