// Acceleration search of the long-segment spectra (xengAccel*, accel.hip): the search of plong_kernels.h repeated per trial
// acceleration on the segment read through a quadratic index map (time-domain resampling, nearest sample).
//
// Contract (include/xeng.h, "Acceleration search of the long-segment spectra").  Series, segments, N = NT/2 = 2^LN, the split
// N = N1 * N2 and every buffer named below are those of plong_kernels.h.  Trial a of ntrial <= 256 searches
//   z_a[n] = z[n + s_a(n)],  s_a(n) = (long long) rint(alpha[a] * (double)(n * (n - NT))),  n = 0 .. NT - 1
// the product formed exactly in 64-bit integers (|n (n - NT)| <= NT^2 / 4 = 2^38, exact as a float64 too), one float64 multiply,
// rounding to nearest even (__double2ll_rn).  |alpha| * NT <= 0.5 (Initialize), so the map is non-decreasing and stays inside
// [0, NT - 1]: no clamp.  The records of trial a are bit for bit those of xengPlongRun (nstack = 1) fed z_a.
//
// Per completed segment, in stream order behind the ingest (plong_ingest_kernel) of its last window: per batch of SB series, and
// inside the batch per trial (a batch of tbuf stays warm in L2 / Infinity Cache over its trials),
//   M' accel_mean_kernel, grid SB: plong_mean_kernel with the points loaded through the gather, into the batch-local mv
//   C' accel_cols_kernel, grid (N2 / 16, SB): plong_cols_kernel with the points loaded through the gather
//      Each thread forms the indices of z_a[2m] and z_a[2m + 1] in float64 and loads two words in place of one float2 (the map
//      steps by 0, 1 or 2 windows, by 1 nearly everywhere: the two are neighbours, the same word, or one word apart).  The
//      resampled series is never stored: tbuf is read twice per trial.  Everything behind the load is plong's
//      arithmetic in plong's order -- the same inlined pl_fft_fwd, the same sums of the mean's tree.
//   R U W S D  plong_rows_kernel, plong_power_kernel, plong_whiten_kernel, plong_sums_kernel and plong_reduce_kernel as they are,
//      on batch-local buffers: ser0 = 0, the batch-local mv, a batch-local S f32[SB][N] in the place of A with first = 1, and
//      out = the trial records {f32 H, i32 k}[ntrial][nser][nlevel][nband] at (trial, the batch's first series).
// and behind the last batch
//   B  accel_best_kernel, one thread per record of the plane: the trials in ascending order, larger H wins (so among equal H the
//      smaller ia, and within a trial the smaller k already); {f32 H, i32 k, i32 ia, f32 H0} in one 16-byte store, H0 the H of
//      the first trial with alpha == 0.0 (izero; +0 without one).  An empty record is {+0, -1, -1, H0}.
//
// No atomics, no printf; every word has one owner; index arithmetic that spans series is size_t.  accel.hip is compiled with
// -fno-slp-vectorize, as plong.hip (Makefile).
#pragma once
#include <hip/hip_runtime.h>

// plong_kernels.h defines its kernels as external symbols and plong.o has them already.  This translation unit's copy -- the same
// source under the same flags -- is compiled inside a namespace of its own, so that its symbols have other names; xeng sees them
// through a using-directive.  (hip_runtime.h is included above: inside the namespace its include guard keeps it out.)
namespace accel_plong {
#include "plong_kernels.h"
}
namespace xeng {
using namespace accel_plong::xeng;
}

namespace xeng {

constexpr int AC_MAX_TRIAL = 256;

struct alignas(16) AccelRecord {
    float H;
    int k;
    int ia;
    float H0;
};

// n + s_a(n): where window n of trial alpha's series lies in the segment
__device__ __forceinline__ int ac_index(int n, int NT, double alpha) {
    const long long q = (long long)n * (long long)(n - NT);
    return n + (int)__double2ll_rn(alpha * (double)q);
}

// the complex point c[m] = (z_a[2m], z_a[2m + 1]) of a series whose segment begins at src
__device__ __forceinline__ float2 ac_point(const float* __restrict__ src, int m, int NT, double alpha) {
    return make_float2(src[ac_index(2 * m, NT, alpha)], src[ac_index(2 * m + 1, NT, alpha)]);
}

// M': grid SB (the series ser0 + blockIdx.x; mv is the batch's), 256 threads.  N >= 1024.
__global__ __launch_bounds__(256) void accel_mean_kernel(const float* __restrict__ tbuf, PlongMean* __restrict__ mv, int LN, int ser0, double alpha) {
    __shared__ float wsum[4];
    const int N = 1 << LN, NT = N << 1, tid = threadIdx.x;
    const float* const src = tbuf + (((size_t)ser0 + blockIdx.x) << (LN + 1));
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int m = tid; m < N; m += 4 * PL_THREADS) {
        const float2 c0 = ac_point(src, m, NT, alpha), c1 = ac_point(src, m + PL_THREADS, NT, alpha), c2 = ac_point(src, m + 2 * PL_THREADS, NT, alpha),
                     c3 = ac_point(src, m + 3 * PL_THREADS, NT, alpha);
        a0 += c0.x + c0.y;
        a1 += c1.x + c1.y;
        a2 += c2.x + c2.y;
        a3 += c3.x + c3.y;
    }
    float part = (a0 + a1) + (a2 + a3);
    for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        PlongMean r;
        r.mean = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) * (0.5f / (float)N);
        r.valid = (__float_as_uint(r.mean) & 0x7f800000u) != 0x7f800000u;
        mv[blockIdx.x] = r;
    }
}

// C': grid (N2 / 16, SB), 256 threads, N1 * 16 * 8 bytes of dynamic LDS; ser0 is the batch's first series, mv and scr the batch's
__global__ __launch_bounds__(256) void accel_cols_kernel(const float* __restrict__ tbuf, const PlongMean* __restrict__ mv, float2* __restrict__ scr,
                                                         const float2* __restrict__ tw1, int LN1, int LN2, int ser0, double alpha) {
    extern __shared__ float2 pl_lds[];
    const int N1 = 1 << LN1, NT = 2 << (LN1 + LN2), tid = threadIdx.x;
    const float* const src = tbuf + (((size_t)ser0 + blockIdx.y) << (LN1 + LN2 + 1));
    const int m0 = blockIdx.x * PL_TC;
    float2* const dst = scr + ((size_t)blockIdx.y << (LN1 + LN2)) + (size_t)blockIdx.x * PL_TC;
    const float mean = mv[blockIdx.y].mean;
    for (int w = tid; w < N1 * PL_TC; w += PL_THREADS) {
        const int t = w & (PL_TC - 1), i = w >> PL_LTC;
        const float2 c = ac_point(src, m0 + (i << LN2) + t, NT, alpha);
        pl_lds[pl_at<true>(i, t, LN1)] = make_float2(c.x - mean, c.y - mean);
    }
    __syncthreads();
    pl_fft_fwd<true>(pl_lds, tw1, LN1, PL_LTC);
    for (int w = tid; w < N1 * PL_TC; w += PL_THREADS) {
        const int t = w & (PL_TC - 1), i = w >> PL_LTC;
        dst[((size_t)i << LN2) + t] = pl_lds[pl_at<true>(i, t, LN1)];
    }
}

// B: grid ceil(nrec / 256), 256 threads: record i of the plane from trec {H, k}[ntrial][nrec]
__global__ __launch_bounds__(256) void accel_best_kernel(const PlongRecord* __restrict__ trec, AccelRecord* __restrict__ out, long long nrec, int ntrial,
                                                         int izero) {
    const long long i = (long long)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= nrec) return;
    float H = 0.f, H0 = 0.f;
    int k = -1, ia = -1;
    for (int a = 0; a < ntrial; a++) {
        const PlongRecord p = trec[(size_t)a * (size_t)nrec + (size_t)i];
        if (p.k < 0 || p.H != p.H) continue;
        if (a == izero) H0 = p.H;
        if (k < 0 || p.H > H) {
            H = p.H;
            k = p.k;
            ia = a;
        }
    }
    ((float4*)out)[i] = make_float4(H, __int_as_float(k), __int_as_float(ia), H0);
}

}  // namespace xeng
