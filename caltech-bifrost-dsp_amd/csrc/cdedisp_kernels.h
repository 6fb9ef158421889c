// Coherent dedispersion of the voltage beams (xengCdedisp*, cdedisp.hip): overlap-save filtering of every (coarse channel, beam) row
// by a table given in the frequency domain.
//
// Contract (include/xeng.h, "Coherent dedispersion of the voltage beams"); a row is one (channel c, selected beam b), nb = 2 npair,
// nrow = nchan * nb, row = c * nb + b; N = NFFT = 2^LN, M the overlap (even, <= N/2), L = N - M the step:
//   in     cf32[nchan][nbeam][ntime], Beamform's output; the selected beams are 2 pair0 + b
//   tbuf   cf32[nrow][N]: between two blocks slots [0, fill) hold the samples of the block in progress
//   tab    cf32[npair][nchan][N], the table in BIT-REVERSED order (tab[..][j] = T[..][bitrev(j)], permuted by the host), 1/N included
//   tw     float2[N/2], tw[k] = exp(-2 pi i k / N): float64 on the host, rounded once
//   out    cf32[nrow][L] of one block: y[M/2 .. M/2 + L)
//
// Ingest, every call (and once more where a call straddles a block boundary): the input is time-fastest already, so a thread moves
// one sample, 8-byte loads and stores consecutive across lanes along time; grid (ceil(n / 256), nrow).
//
// Filter, once per completed block, one work-group of 256 threads per row, float2[N] of dynamic LDS and nothing else:
//   1. coalesced load of the row into LDS.
//   2. the overlap: behind the barrier that follows every load of the row, the last M samples (read back from LDS) are stored over
//      the row's first M slots, for the next block.  M <= L, so source and destination do not meet, and no other work-group touches
//      the row.  (One buffer and a barrier, not two halves.)  A second barrier keeps step 3's LDS writes behind these LDS reads.
//   3. the forward FFT in place, decimation in frequency, natural order in and bit-reversed order out: two radix-2 stages fused in
//      registers per LDS pass (points a, a+h/2, a+h, a+3h/2: the butterflies of half-sizes h and h/2), and where LN is odd a last
//      radix-2 stage (half-size 1, twiddle 1).  W_2h^p = tw[p * N / 2h], and W_2h^(p+h/2) = -i W_2h^p; the element that would pass
//      through two twiddles, W_2h^p and then W_h^p, takes their product W_2h^3p from the table instead: one rounding fewer.
//   4. the inverse FFT in place, decimation in time with conjugate twiddles, the same stages in the mirrored order (the transposed
//      flow graph): bit-reversed order in, natural order out.  Where LN is odd the radix-2 stage comes first.  The first pass
//      multiplies what it loads by the table, element j by tab[j]: X[k] sits at element bitrev(k), and the table is stored that way.
//   5. coalesced store of the L middle samples.
// Per block and row: N global words in, M back, L out; 2 + ceil(LN / 2) * 2 LDS passes (each a read and a write of N elements but
// the first, write only, and the last, read only, and the M elements of step 2).
//
// LDS banks: element i lives at cd_sw(i), the XOR swizzle of period_kernels.h (a copy: that file's code objects stay what they
// are).  A fused pass touches the same four elements per thread in either direction, so the forward argument holds
// for the mirrored order stage by stage; steps 1 and 5 read or write runs of consecutive elements (step 5 from the offset M/2,
// which need not be a multiple of 32).  All of it is re-enumerated in DESIGN.md 4.21.
//
// fp32, contracts freely (held to a tolerance); no atomics, no scalar memory writes, no printf; every word has one owner; the
// result is a fixed function of the row's samples and the table.
//
// cdedisp.hip is compiled with -fno-slp-vectorize (Makefile): complex fp32 arithmetic, as upchan_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int CD_THREADS = 256;

// grid (ceil(n / 256), nrow), 256 threads: samples [t0, t0 + n) of the call into slots [slot0, slot0 + n) of every row;
// t0 + n <= ntime and slot0 + n <= N (the host's arithmetic)
__global__ __launch_bounds__(256) void cdedisp_ingest_kernel(const float2* __restrict__ in, float2* __restrict__ tbuf, int nbeam, int ntime, int beam0,
                                                             int nb, int N, int t0, int slot0, int n) {
    const int t = blockIdx.x * CD_THREADS + threadIdx.x;
    if (t >= n) return;
    const int row = blockIdx.y, c = row / nb, b = row - c * nb;
    tbuf[(size_t)row * N + slot0 + t] = in[((size_t)c * nbeam + beam0 + b) * ntime + t0 + t];
}

// where element i of the work-group's float2[N] lives (see "LDS banks" above); a bijection of every aligned block of 32
__device__ __forceinline__ int cd_sw(int i, int LN) {
    int p = i ^ ((i & 32) ? 21 : 0) ^ ((i & 64) ? 31 : 0);
    if (LN >= 12) p ^= (int)(__brev((unsigned)i >> (LN - 5)) >> 27);
    return p;
}

__device__ __forceinline__ float2 cd_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
// a * conj(w)
__device__ __forceinline__ float2 cd_cmulc(float2 a, float2 w) { return make_float2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y); }

// tw[k] for 0 <= k < 3N/4 from the half table: tw[k + N/2] = -tw[k]
__device__ __forceinline__ float2 cd_tw3(const float2* __restrict__ tw, int k, int N) {
    const int hi = k >= (N >> 1);
    const float2 w = tw[k - (hi ? (N >> 1) : 0)];
    return hi ? make_float2(-w.x, -w.y) : w;
}

// grid nrow, 256 threads, N * 8 bytes of dynamic LDS.  LN = log2 N; out is the block's unit, cf32[nrow][N - M].
__global__ __launch_bounds__(256) void cdedisp_filter_kernel(float2* __restrict__ tbuf, const float2* __restrict__ tab, const float2* __restrict__ tw,
                                                             float2* __restrict__ out, int LN, int M, int nb, int nchan) {
    extern __shared__ float2 cd_lds[];
    const int N = 1 << LN, Lstep = N - M, tid = threadIdx.x;
    const int row = blockIdx.x, c = row / nb, b = row - c * nb;
    float2* const src = tbuf + (size_t)row * N;
    const float2* const T = tab + ((size_t)(b >> 1) * nchan + c) * N;

    // 1. load
    for (int m = tid; m < N; m += CD_THREADS) cd_lds[cd_sw(m, LN)] = src[m];
    __syncthreads();                                // (every load of the row is done: the stores of step 2 come behind it)

    // 2. the overlap, for the next block
    for (int m = Lstep + tid; m < N; m += CD_THREADS) src[m - Lstep] = cd_lds[cd_sw(m, LN)];
    if (M) __syncthreads();                         // (those reads come before the first pass of step 3 writes the elements)

    // 3. forward FFT, decimation in frequency
    int lh = LN - 1;                                // log2 of the half-size h
    for (; lh >= 1; lh -= 2) {
        const int lq = lh - 1, hh = 1 << lq;        // hh = h / 2
        for (int q = tid; q < N / 4; q += CD_THREADS) {
            const int p = q & (hh - 1), a = ((q >> lq) << (lq + 2)) | p;
            const int i0 = cd_sw(a, LN), i1 = cd_sw(a + hh, LN), i2 = cd_sw(a + 2 * hh, LN), i3 = cd_sw(a + 3 * hh, LN);
            const float2 x0 = cd_lds[i0], x1 = cd_lds[i1], x2 = cd_lds[i2], x3 = cd_lds[i3];
            const float2 w1 = tw[p << (LN - 1 - lh)], w2 = tw[p << (LN - lh)], w3 = cd_tw3(tw, 3 * p << (LN - 1 - lh), N);
            // half-size h: (a, a+h) with W_2h^p, (a+h/2, a+3h/2) with W_2h^(p+h/2) = -i W_2h^p; half-size h/2: (a, a+h/2) and
            // (a+h, a+3h/2), both with W_h^p = W_2h^2p.  The two twiddles of the last element are taken as one, W_2h^3p.
            const float2 u0 = make_float2(x0.x + x2.x, x0.y + x2.y), d0 = make_float2(x0.x - x2.x, x0.y - x2.y);
            const float2 u1 = make_float2(x1.x + x3.x, x1.y + x3.y), d1 = make_float2(x1.x - x3.x, x1.y - x3.y);
            cd_lds[i0] = make_float2(u0.x + u1.x, u0.y + u1.y);
            cd_lds[i1] = cd_cmul(make_float2(u0.x - u1.x, u0.y - u1.y), w2);
            cd_lds[i2] = cd_cmul(make_float2(d0.x + d1.y, d0.y - d1.x), w1);     // d0 - i d1
            cd_lds[i3] = cd_cmul(make_float2(d0.x - d1.y, d0.y + d1.x), w3);     // d0 + i d1
        }
        __syncthreads();
    }
    if (lh == 0) {                                  // LN odd: the last stage, half-size 1, twiddle 1
        for (int q = tid; q < N / 2; q += CD_THREADS) {
            const int i0 = cd_sw(2 * q, LN), i1 = cd_sw(2 * q + 1, LN);
            const float2 x0 = cd_lds[i0], x1 = cd_lds[i1];
            cd_lds[i0] = make_float2(x0.x + x1.x, x0.y + x1.y);
            cd_lds[i1] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        __syncthreads();
    }

    // 4. inverse FFT, decimation in time, conjugate twiddles, the stages of step 3 mirrored; the first pass applies the table
    bool mul = true;
    if (LN & 1) {                                   // half-size 1, twiddle 1
        for (int q = tid; q < N / 2; q += CD_THREADS) {
            const int i0 = cd_sw(2 * q, LN), i1 = cd_sw(2 * q + 1, LN);
            const float2 x0 = cd_cmul(cd_lds[i0], T[2 * q]), x1 = cd_cmul(cd_lds[i1], T[2 * q + 1]);
            cd_lds[i0] = make_float2(x0.x + x1.x, x0.y + x1.y);
            cd_lds[i1] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        __syncthreads();
        mul = false;
    }
    for (lh = (LN & 1) ? 2 : 1; lh <= LN - 1; lh += 2) {
        const int lq = lh - 1, hh = 1 << lq;
        for (int q = tid; q < N / 4; q += CD_THREADS) {
            const int p = q & (hh - 1), a = ((q >> lq) << (lq + 2)) | p;
            const int i0 = cd_sw(a, LN), i1 = cd_sw(a + hh, LN), i2 = cd_sw(a + 2 * hh, LN), i3 = cd_sw(a + 3 * hh, LN);
            float2 x0 = cd_lds[i0], x1 = cd_lds[i1], x2 = cd_lds[i2], x3 = cd_lds[i3];
            if (mul) {
                x0 = cd_cmul(x0, T[a]);
                x1 = cd_cmul(x1, T[a + hh]);
                x2 = cd_cmul(x2, T[a + 2 * hh]);
                x3 = cd_cmul(x3, T[a + 3 * hh]);
            }
            const float2 w1 = tw[p << (LN - 1 - lh)], w2 = tw[p << (LN - lh)], w3 = cd_tw3(tw, 3 * p << (LN - 1 - lh), N);
            // half-size h/2: (a, a+h/2) and (a+h, a+3h/2), both with conj W_h^p; half-size h: (a, a+h) with conj W_2h^p,
            // (a+h/2, a+3h/2) with conj W_2h^(p+h/2) = +i conj W_2h^p.  The two twiddles of the last element are taken as one.
            const float2 a1 = cd_cmulc(x1, w2), a2 = cd_cmulc(x2, w1), a3 = cd_cmulc(x3, w3);
            const float2 u0 = make_float2(x0.x + a1.x, x0.y + a1.y), u1 = make_float2(x0.x - a1.x, x0.y - a1.y);
            const float2 s0 = make_float2(a2.x + a3.x, a2.y + a3.y), s1 = make_float2(a3.y - a2.y, a2.x - a3.x);      // i (a2 - a3)
            cd_lds[i0] = make_float2(u0.x + s0.x, u0.y + s0.y);
            cd_lds[i2] = make_float2(u0.x - s0.x, u0.y - s0.y);
            cd_lds[i1] = make_float2(u1.x + s1.x, u1.y + s1.y);
            cd_lds[i3] = make_float2(u1.x - s1.x, u1.y - s1.y);
        }
        __syncthreads();
        mul = false;
    }

    // 5. the L middle samples
    float2* const dst = out + (size_t)row * Lstep;
    const int h0 = M >> 1;
    for (int n = tid; n < Lstep; n += CD_THREADS) dst[n] = cd_lds[cd_sw(n + h0, LN)];
}

}  // namespace xeng
