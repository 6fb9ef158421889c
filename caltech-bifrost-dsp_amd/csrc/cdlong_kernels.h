// Coherent dedispersion with long transforms (xengCdlong*, cdlong.hip): the overlap-save filter of cdedisp_kernels.h for
// NFFT = 2^14 .. 2^20, which no work-group's LDS holds, as a four-step FFT through a scratch buffer in HBM.
//
// Contract (include/xeng.h, "Coherent dedispersion with long transforms"): word for word that of xengCdedisp*.  A row is one
// (channel c, selected beam b), nb = 2 npair, nrow = nchan * nb, row = c * nb + b; N = NFFT = 2^LN, M the overlap (even, <= N/2),
// L = N - M the step.
//
// The split: N = N1 * N2 with N1 = 2^LN1, LN1 = min(LN div 2, 9), and N2 = 2^LN2, LN2 = LN - LN1 (2^7 x 2^7 at 2^14, 2^9 x 2^11
// at 2^20); n = n1 * N2 + n2 and k = k1 + N1 * k2.  A row of the time buffer is the matrix x[n1][n2], n2 fastest.
//   tbuf   cf32[nrow][N]: between two blocks slots [0, fill) hold the samples of the block in progress
//   scr    cf32[nrow][N]: the matrix between the passes, [r][n2] with r = bitrev_LN1(k1) (the order pass A leaves and pass C takes)
//   tab    cf32[npair][nchan][N] in the order pass B meets it: tab[..][r * N2 + j] = T[..][bitrev_LN1(r) + N1 * bitrev_LN2(j)]
//          (permuted by the host at upload), 1/N included
//   tws    float2[N/2], exp(-2 pi i k / N), the step twiddles; tw1 float2[N1/2] and tw2 float2[N2/2], the same for N1 and N2: float64
//          on the host, rounded once
//   out    cf32[nrow][L] of one block: y[M/2 .. M/2 + L)
//
// Per completed block, four launches in stream order behind the ingest (which is cdedisp_kernels.h's, restated here):
//   A  cdlong_cols_fwd_kernel, grid (N2 / 16, nrow): a tile of 16 adjacent columns of x, N1 x 16 elements of LDS; the forward FFT
//      of length N1 down every column, decimation in frequency, natural order in and bit-reversed out;
//      scr[r][n2] = sum_n1 x[n1][n2] exp(-2 pi i n1 k1 / N1).  Every global access is a run of 16 elements = 128 bytes.
//   T  cdlong_tail_kernel, grid (ceil(M / 256), nrow): the overlap, tbuf[row][m] = tbuf[row][L + m] for m < M.  No race: it is
//      launched behind pass A, the only reader of the block's samples, on the same stream; nothing else in flight touches the time
//      buffer (the next ingest comes behind it on the stream); and M <= L keeps the words it reads, [L, N), apart from the words
//      it writes, [0, M), so no thread reads what another writes.
//   B  cdlong_rows_kernel, grid (N1 / R, nrow): a work-group owns R = max(1, 1024 / N2) whole rows of scr (1024 elements of LDS
//      at least, so that 256 threads have a butterfly each) and works in place: each row is loaded times the step twiddle
//      exp(-2 pi i n2 k1 / N), transformed forward over n2 (decimation in frequency), multiplied by the table in the order it lies
//      in, transformed back (decimation in time, conjugate twiddles, the mirrored stages), and stored times
//      exp(+2 pi i n2 k1 / N).  This is cdedisp_filter_kernel steps 3 and 4 with the step twiddle on the load and on the store.
//   C  cdlong_cols_inv_kernel, grid (N2 / 16, nrow): the tile of A again, the inverse FFT of length N1 down every column
//      (bit-reversed in, natural out), y[n1][n2] = sum_k1 scr[r][n2] exp(+2 pi i n1 k1 / N1); only the samples
//      M/2 <= n1 * N2 + n2 < M/2 + L are stored, in runs of up to 16 elements.
// Per block and row: N words of tbuf read and N of scr written (A), M read and written (T), N of scr read and written and N of
// table read (B), N of scr read and L of out written (C).
//
// LDS.  The row layout (pass B): element i of row t lives at t * N2 + cl_sw(i), the XOR swizzle of cdedisp_kernels.h (a copy: that
// file's code objects stay what they are); consecutive lanes take consecutive butterflies of one row.  The column layout (passes A
// and C): element i of column t lives at 16 * (i ^ parity(i >> 1)) + t, consecutive lanes take the 16 columns of one butterfly and
// the next 16 lanes the next butterfly: the 16 columns of an element are one run of 128 bytes, half a bank row, and the two
// butterflies that share a group of 32 lanes differ in one bit of their element index, so in parity, so in the half they take.
// DESIGN.md 4.30 has the argument pass by pass.
//
// fp32, contracts freely (held to a tolerance); no atomics, no scalar memory writes, no printf; every word has one owner; index
// arithmetic that spans rows is size_t.  The result is a fixed function of the row's samples and the table.
//
// cdlong.hip is compiled with -fno-slp-vectorize (Makefile): complex fp32 arithmetic, as cdedisp_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int CL_THREADS = 256;
constexpr int CL_LTC = 4, CL_TC = 1 << CL_LTC;      // columns per tile of passes A and C: runs of 16 * 8 = 128 bytes
constexpr int CL_LN1_MAX = 9;                       // N1 <= 512: 64 KiB of LDS for a tile

constexpr int cl_ln1(int LN) { return (LN >> 1) < CL_LN1_MAX ? (LN >> 1) : CL_LN1_MAX; }
// log2 of the rows a work-group of pass B owns: 2^10 elements of LDS at least
constexpr int cl_lrows(int LN2) { return LN2 < 10 ? 10 - LN2 : 0; }

// grid (ceil(n / 256), nrow), 256 threads: samples [t0, t0 + n) of the call into slots [slot0, slot0 + n) of every row;
// t0 + n <= ntime and slot0 + n <= N (the host's arithmetic)
__global__ __launch_bounds__(256) void cdlong_ingest_kernel(const float2* __restrict__ in, float2* __restrict__ tbuf, int nbeam, int ntime, int beam0,
                                                            int nb, int N, int t0, int slot0, int n) {
    const int t = blockIdx.x * CL_THREADS + threadIdx.x;
    if (t >= n) return;
    const int row = blockIdx.y, c = row / nb, b = row - c * nb;
    tbuf[(size_t)row * N + slot0 + t] = in[((size_t)c * nbeam + beam0 + b) * ntime + t0 + t];
}

// T: grid (ceil(M / 256), nrow), 256 threads.  See "no race" above: launched behind pass A; [L, N) and [0, M) do not meet.
__global__ __launch_bounds__(256) void cdlong_tail_kernel(float2* tbuf, int N, int M) {
    const int m = blockIdx.x * CL_THREADS + threadIdx.x;
    if (m >= M) return;
    float2* const row = tbuf + (size_t)blockIdx.y * N;
    row[m] = row[N - M + m];
}

// cd_sw of cdedisp_kernels.h below its fold of 2^12 points (N2 <= 2^11): a bijection of every aligned block of 32
__device__ __forceinline__ int cl_sw(int i) { return i ^ ((i & 32) ? 21 : 0) ^ ((i & 64) ? 31 : 0); }

// where element i of transform t lives: COL, the tiles of passes A and C (i < 512); else the rows of pass B
template <bool COL> __device__ __forceinline__ int cl_at(int i, int t, int ln) {
    if (COL) {
        int p = i >> 1;
        p ^= p >> 4;
        p ^= p >> 2;
        p ^= p >> 1;
        return ((i ^ (p & 1)) << CL_LTC) | t;
    }
    return (t << ln) | cl_sw(i);
}

// work item w of a pass with 2^lg items per transform: COL, the columns fastest; else the items of one row fastest
template <bool COL> __device__ __forceinline__ void cl_item(int w, int lg, int& q, int& t) {
    if (COL) {
        t = w & (CL_TC - 1);
        q = w >> CL_LTC;
    } else {
        q = w & ((1 << lg) - 1);
        t = w >> lg;
    }
}

__device__ __forceinline__ float2 cl_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
// a * conj(w)
__device__ __forceinline__ float2 cl_cmulc(float2 a, float2 w) { return make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y); }

// exp(-2 pi i k / n) for 0 <= k < n from the half table: tw[k + n/2] = -tw[k]
__device__ __forceinline__ float2 cl_twf(const float2* __restrict__ tw, int k, int n) {
    const int hi = k >= (n >> 1);
    const float2 w = tw[k - (hi ? (n >> 1) : 0)];
    return hi ? make_float2(-w.x, -w.y) : w;
}

// 2^lt transforms of 2^ln points in LDS, forward, in place, decimation in frequency: natural order in, bit-reversed out.  The
// stages are cdedisp_filter_kernel's step 3: two radix-2 stages fused per pass, W_2h^3p from the table, a last radix-2 stage
// where ln is odd.  tw: float2[2^ln / 2].  Every thread of the work-group calls it; it ends behind a barrier.
template <bool COL> __device__ __forceinline__ void cl_fft_fwd(float2* lds, const float2* __restrict__ tw, int ln, int lt) {
    const int n = 1 << ln, tid = threadIdx.x;
    int lh = ln - 1;                                // log2 of the half-size h
    for (; lh >= 1; lh -= 2) {
        const int lq = lh - 1, hh = 1 << lq;        // hh = h / 2
        for (int w = tid; w < (n >> 2) << lt; w += CL_THREADS) {
            int q, t;
            cl_item<COL>(w, ln - 2, q, t);
            const int p = q & (hh - 1), a = ((q >> lq) << (lq + 2)) | p;
            const int i0 = cl_at<COL>(a, t, ln), i1 = cl_at<COL>(a + hh, t, ln), i2 = cl_at<COL>(a + 2 * hh, t, ln), i3 = cl_at<COL>(a + 3 * hh, t, ln);
            const float2 x0 = lds[i0], x1 = lds[i1], x2 = lds[i2], x3 = lds[i3];
            const float2 w1 = tw[p << (ln - 1 - lh)], w2 = tw[p << (ln - lh)], w3 = cl_twf(tw, 3 * p << (ln - 1 - lh), n);
            const float2 u0 = make_float2(x0.x + x2.x, x0.y + x2.y), d0 = make_float2(x0.x - x2.x, x0.y - x2.y);
            const float2 u1 = make_float2(x1.x + x3.x, x1.y + x3.y), d1 = make_float2(x1.x - x3.x, x1.y - x3.y);
            lds[i0] = make_float2(u0.x + u1.x, u0.y + u1.y);
            lds[i1] = cl_cmul(make_float2(u0.x - u1.x, u0.y - u1.y), w2);
            lds[i2] = cl_cmul(make_float2(d0.x + d1.y, d0.y - d1.x), w1);     // d0 - i d1
            lds[i3] = cl_cmul(make_float2(d0.x - d1.y, d0.y + d1.x), w3);     // d0 + i d1
        }
        __syncthreads();
    }
    if (lh == 0) {                                  // ln odd: the last stage, half-size 1, twiddle 1
        for (int w = tid; w < (n >> 1) << lt; w += CL_THREADS) {
            int q, t;
            cl_item<COL>(w, ln - 1, q, t);
            const int i0 = cl_at<COL>(2 * q, t, ln), i1 = cl_at<COL>(2 * q + 1, t, ln);
            const float2 x0 = lds[i0], x1 = lds[i1];
            lds[i0] = make_float2(x0.x + x1.x, x0.y + x1.y);
            lds[i1] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        __syncthreads();
    }
}

// ... inverse, decimation in time with conjugate twiddles, the stages of cl_fft_fwd mirrored: bit-reversed order in, natural out
// (cdedisp_filter_kernel's step 4).  T non-null: the first pass multiplies element i of transform t by T[t * 2^ln + i] as it loads.
template <bool COL> __device__ __forceinline__ void cl_fft_inv(float2* lds, const float2* __restrict__ tw, int ln, int lt, const float2* __restrict__ T) {
    const int n = 1 << ln, tid = threadIdx.x;
    bool mul = T != nullptr;
    if (ln & 1) {                                   // half-size 1, twiddle 1
        for (int w = tid; w < (n >> 1) << lt; w += CL_THREADS) {
            int q, t;
            cl_item<COL>(w, ln - 1, q, t);
            const int i0 = cl_at<COL>(2 * q, t, ln), i1 = cl_at<COL>(2 * q + 1, t, ln);
            float2 x0 = lds[i0], x1 = lds[i1];
            if (mul) {
                x0 = cl_cmul(x0, T[(t << ln) + 2 * q]);
                x1 = cl_cmul(x1, T[(t << ln) + 2 * q + 1]);
            }
            lds[i0] = make_float2(x0.x + x1.x, x0.y + x1.y);
            lds[i1] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        __syncthreads();
        mul = false;
    }
    for (int lh = (ln & 1) ? 2 : 1; lh <= ln - 1; lh += 2) {
        const int lq = lh - 1, hh = 1 << lq;
        for (int w = tid; w < (n >> 2) << lt; w += CL_THREADS) {
            int q, t;
            cl_item<COL>(w, ln - 2, q, t);
            const int p = q & (hh - 1), a = ((q >> lq) << (lq + 2)) | p;
            const int i0 = cl_at<COL>(a, t, ln), i1 = cl_at<COL>(a + hh, t, ln), i2 = cl_at<COL>(a + 2 * hh, t, ln), i3 = cl_at<COL>(a + 3 * hh, t, ln);
            float2 x0 = lds[i0], x1 = lds[i1], x2 = lds[i2], x3 = lds[i3];
            if (mul) {
                const float2* const Tt = T + (t << ln) + a;
                x0 = cl_cmul(x0, Tt[0]);
                x1 = cl_cmul(x1, Tt[hh]);
                x2 = cl_cmul(x2, Tt[2 * hh]);
                x3 = cl_cmul(x3, Tt[3 * hh]);
            }
            const float2 w1 = tw[p << (ln - 1 - lh)], w2 = tw[p << (ln - lh)], w3 = cl_twf(tw, 3 * p << (ln - 1 - lh), n);
            const float2 a1 = cl_cmulc(x1, w2), a2 = cl_cmulc(x2, w1), a3 = cl_cmulc(x3, w3);
            const float2 u0 = make_float2(x0.x + a1.x, x0.y + a1.y), u1 = make_float2(x0.x - a1.x, x0.y - a1.y);
            const float2 s0 = make_float2(a2.x + a3.x, a2.y + a3.y), s1 = make_float2(a3.y - a2.y, a2.x - a3.x);      // i (a2 - a3)
            lds[i0] = make_float2(u0.x + s0.x, u0.y + s0.y);
            lds[i2] = make_float2(u0.x - s0.x, u0.y - s0.y);
            lds[i1] = make_float2(u1.x + s1.x, u1.y + s1.y);
            lds[i3] = make_float2(u1.x - s1.x, u1.y - s1.y);
        }
        __syncthreads();
        mul = false;
    }
}

// A: grid (N2 / 16, nrow), 256 threads, N1 * 16 * 8 bytes of dynamic LDS
__global__ __launch_bounds__(256) void cdlong_cols_fwd_kernel(const float2* __restrict__ tbuf, float2* __restrict__ scr, const float2* __restrict__ tw1,
                                                              int LN1, int LN2) {
    extern __shared__ float2 cl_lds[];
    const int N1 = 1 << LN1, tid = threadIdx.x;
    const size_t base = ((size_t)blockIdx.y << (LN1 + LN2)) + (size_t)blockIdx.x * CL_TC;
    const float2* const src = tbuf + base;
    float2* const dst = scr + base;
    for (int w = tid; w < N1 * CL_TC; w += CL_THREADS) {
        const int t = w & (CL_TC - 1), i = w >> CL_LTC;
        cl_lds[cl_at<true>(i, t, LN1)] = src[((size_t)i << LN2) + t];
    }
    __syncthreads();
    cl_fft_fwd<true>(cl_lds, tw1, LN1, CL_LTC);
    for (int w = tid; w < N1 * CL_TC; w += CL_THREADS) {
        const int t = w & (CL_TC - 1), i = w >> CL_LTC;
        dst[((size_t)i << LN2) + t] = cl_lds[cl_at<true>(i, t, LN1)];
    }
}

// B: grid (N1 >> cl_lrows(LN2), nrow), 256 threads, (N2 << cl_lrows(LN2)) * 8 bytes of dynamic LDS; in place in scr
__global__ __launch_bounds__(256) void cdlong_rows_kernel(float2* __restrict__ scr, const float2* __restrict__ tab, const float2* __restrict__ tws,
                                                          const float2* __restrict__ tw2, int LN1, int LN2, int nb, int nchan) {
    extern __shared__ float2 cl_lds[];
    const int LN = LN1 + LN2, N = 1 << LN, N2 = 1 << LN2, lr = cl_lrows(LN2), tid = threadIdx.x;
    const int row = blockIdx.y, c = row / nb, b = row - c * nb, r0 = blockIdx.x << lr;
    float2* const src = scr + ((size_t)row << LN) + ((size_t)r0 << LN2);
    const float2* const T = tab + (((size_t)(b >> 1) * nchan + c) << LN) + ((size_t)r0 << LN2);
    for (int w = tid; w < N2 << lr; w += CL_THREADS) {
        const int m = w & (N2 - 1), t = w >> LN2;
        const int k1 = (int)(__brev((unsigned)(r0 + t)) >> (32 - LN1));
        cl_lds[cl_at<false>(m, t, LN2)] = cl_cmul(src[w], cl_twf(tws, m * k1, N));
    }
    __syncthreads();
    cl_fft_fwd<false>(cl_lds, tw2, LN2, lr);
    cl_fft_inv<false>(cl_lds, tw2, LN2, lr, T);
    for (int w = tid; w < N2 << lr; w += CL_THREADS) {
        const int m = w & (N2 - 1), t = w >> LN2;
        const int k1 = (int)(__brev((unsigned)(r0 + t)) >> (32 - LN1));
        src[w] = cl_cmulc(cl_lds[cl_at<false>(m, t, LN2)], cl_twf(tws, m * k1, N));
    }
}

// C: grid (N2 / 16, nrow), 256 threads, N1 * 16 * 8 bytes of dynamic LDS.  out is the block's unit, cf32[nrow][N - M].
__global__ __launch_bounds__(256) void cdlong_cols_inv_kernel(const float2* __restrict__ scr, float2* __restrict__ out, const float2* __restrict__ tw1,
                                                              int LN1, int LN2, int M) {
    extern __shared__ float2 cl_lds[];
    const int N1 = 1 << LN1, N = 1 << (LN1 + LN2), Lstep = N - M, h0 = M >> 1, tid = threadIdx.x;
    const int c0 = blockIdx.x * CL_TC;
    const float2* const src = scr + ((size_t)blockIdx.y << (LN1 + LN2)) + c0;
    for (int w = tid; w < N1 * CL_TC; w += CL_THREADS) {
        const int t = w & (CL_TC - 1), i = w >> CL_LTC;
        cl_lds[cl_at<true>(i, t, LN1)] = src[((size_t)i << LN2) + t];
    }
    __syncthreads();
    cl_fft_inv<true>(cl_lds, tw1, LN1, CL_LTC, nullptr);
    float2* const dst = out + (size_t)blockIdx.y * Lstep;
    for (int w = tid; w < N1 * CL_TC; w += CL_THREADS) {
        const int t = w & (CL_TC - 1), i = w >> CL_LTC;
        const int n = (i << LN2) + c0 + t - h0;     // (n1 * N2 + n2 < 2^20)
        if (n >= 0 && n < Lstep) dst[n] = cl_lds[cl_at<true>(i, t, LN1)];
    }
}

}  // namespace xeng
