// FFT periodicity search with long segments (xengPlong*, plong.hip): the search of period_kernels.h for NT = 2^15 .. 2^20 windows,
// whose NT/2 complex points no work-group's LDS holds, as a four-step FFT through a scratch buffer in HBM (the split of
// cdlong_kernels.h), and with one peak record per series, level and BAND of fundamental frequency.
//
// Contract (include/xeng.h, "FFT periodicity search with long segments"); a series is one (pair, trial), nser = npair*ndm; the real
// segment is packed as N = NT/2 = 2^LN complex points c[m] = (z[2m], z[2m+1]); SB series make a batch, sl is a series' place in it:
//   in     f32[nc][nser][NPROD], z = word 0 (NPROD = 1) or word 0 + word 1 (NPROD = 4)
//   tbuf   f32[nser][NT], window n of a series at slot n mod NT
//   mv     {f32 mean, i32 valid}[nser] of the segment that completed last
//   scr    cf32[SB][N], the matrix between the passes; P f32[SB][N], the power spectrum in natural order
//   A      f32[nser][N], the stack
//   keep   u8[N] (0 = zapped) and cnt f32[N/B], the bins of each whitening block that count (k >= 1, kept): both from the host
//   tw     float2[N], exp(-2 pi i k / NT) (the untangle); tws float2[N/2], exp(-2 pi i k / N) (the step twiddles); tw1 float2[N1/2]
//          and tw2 float2[N2/2], the same for N1 and N2: float64 on the host, rounded once
//   kedge  i32[nband + 1]; part {f32 H, i32 k}[SB][nlevel][nband][16], one partial record per tile of N/16 bins
//   out    {f32 H, i32 k}[nser][nlevel][nband], one 8-byte store each
//
// The split is cdlong_kernels.h's: N = N1 * N2, N1 = 2^LN1, LN1 = min(LN div 2, 9), N2 = 2^LN2, LN2 = LN - LN1 (2^7 x 2^7 at
// NT = 2^15, 2^7 x 2^8 at 2^16, 2^9 x 2^10 at 2^20); m = n1 * N2 + n2 and k = k1 + N1 * k2.  A row of the time buffer, read as
// float2, is the matrix c[n1][n2], n2 fastest.
//
// Every call: plong_ingest_kernel, period_ingest_kernel restated (a tile of 32 series x 32 windows through LDS).  Per completed
// segment, in stream order behind the ingest of its last window:
//   M  plong_mean_kernel, grid nser: the mean of the whole segment in a fixed tree (per thread four running sums over a stride of
//      256 points, the wave by shuffles, the four waves in order) and whether it is finite.  It is a function of the segment alone,
//      never of how the calls cut it.
//   then, per batch of SB series (scr, P and part hold one batch; the batches follow one another on the stream):
//   C  plong_cols_kernel, grid (N2 / 16, SB): a tile of 16 adjacent columns, N1 x 16 elements of LDS; the mean is subtracted as the
//      points are loaded; the forward FFT of length N1 down every column, decimation in frequency, natural order in and
//      bit-reversed out: scr[r][n2], r = bitrev_LN1(k1).  Every global access is a run of 16 elements = 128 bytes.
//   R  plong_rows_kernel, grid (N1 / R, SB), R = max(1, 1024 / N2) whole rows: each row is loaded times the step twiddle
//      exp(-2 pi i n2 k1 / N), transformed over n2 (decimation in frequency) and stored in place.
//      The permutation the two passes leave: scr[r][j] = Z[k1 + N1 * k2] with r = bitrev_LN1(k1) and j = bitrev_LN2(k2), Z the
//      N-point transform of c.
//   U  plong_power_kernel, grid (N2 / 16, SB): the untangle.  A work-group takes the 16 adjacent columns j = 16 bx + jj of every
//      row: bins k = k1 + N1 * bitrev_LN2(j), all k1.  The mirror partner Z[N - k] of bin k is at k1' = (N1 - k1) mod N1 and
//      k2' = N2 - 1 - k2 (k1 != 0; the complement of k2, so j' = N2 - 1 - j: the mirrored tile, read backwards) or
//      k2' = (N2 - k2) mod N2 (k1 = 0); the kernel forms k' = (N - k) mod N and splits it.  Both loads are runs of 128 bytes.
//      X[k] = E + W^k O, E = (Z[k] + conj Z[N-k]) / 2, O = (Z[k] - conj Z[N-k]) / 2i, W^k = tw[k]; P[k] = |X[k]|^2 goes through
//      an LDS tile f32[16][N1 + 2] and out in NATURAL k order, in runs of N1 words.  (P[0] is the DC power; nothing reads it.)
//   W  plong_whiten_kernel, grid (N / Wd, SB), Wd = max(B, 1024) bins: a work-group owns whole blocks.  Block sums by a pairwise
//      tree in LDS (level 1 applies k >= 1 and keep), mu_b = sum / cnt[b], S, then A = S (the stack's first segment) or A + S.
// On the call that completes a stack, per batch:
//   S  plong_sums_kernel, grid (16, SB): a tile of N/16 top-harmonic bins of one series.  Per level and band the bins of the band
//      that lie in the tile are shared out over the threads, H_h[k] by gathers from A (plain adds, j ascending, contraction off),
//      (H, k) reduced per wave by shuffles and over the four waves through LDS: one partial record per (level, band, tile), {+0, -1}
//      where the band misses the tile.
//   D  plong_reduce_kernel, one thread per record: the 16 partials in tile order under the same rule (larger H, then smaller k).
//
// LDS banks.  Passes C and R use the two layouts of cdlong_kernels.h (restated below: that file's code objects stay what they
// are): the column layout, element i of column t at 16 * (i ^ parity(i >> 1)) + t, and the row layout, element i of row t at
// t * N2 + sw(i).  DESIGN.md 4.30 has the argument stage by stage; 4.32 that of the P tile (row stride N1 + 2 words = 2 mod 32:
// the 16 columns x 2 values of k1 of a 32-lane group of ds_write_b32 fall on 32 different banks) and of the whitening tree.
//
// fp32.  Everything up to A is held to a tolerance and contracts freely; the harmonic sums are plain adds.  No atomics, no printf;
// every word has one owner; index arithmetic that spans series is size_t.  A and the records are a fixed function of the series,
// the mask and the edges, whatever SB is.
//
// plong.hip is compiled with -fno-slp-vectorize (Makefile): complex fp32 arithmetic, as cdlong_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int PL_THREADS = 256;
constexpr int PL_TILE = 32;                         // ingest tile: series x windows
constexpr int PL_MAX_LEVEL = 5;
constexpr int PL_MAX_BAND = 32;
constexpr int PL_LTC = 4, PL_TC = 1 << PL_LTC;      // columns per tile of passes C and U: runs of 16 * 8 = 128 bytes
constexpr int PL_LN1_MAX = 9;                       // N1 <= 512: 64 KiB of LDS for a tile of pass C
constexpr int PL_LNTILE = 4, PL_NTILE = 1 << PL_LNTILE;     // tiles of the sums per series
constexpr int PL_PPAD = 2;                          // the P tile's row stride is N1 + 2 words

constexpr int pl_ln1(int LN) { return (LN >> 1) < PL_LN1_MAX ? (LN >> 1) : PL_LN1_MAX; }
// log2 of the rows a work-group of pass R owns: 2^10 elements of LDS at least
constexpr int pl_lrows(int LN2) { return LN2 < 10 ? 10 - LN2 : 0; }
// log2 of the bins a work-group of pass W owns: whole blocks, 2^10 bins at least
constexpr int pl_lwhite(int lb) { return lb < 10 ? 10 : lb; }

struct alignas(8) PlongRecord {
    float H;
    int k;
};
struct alignas(8) PlongMean {
    float mean;
    int valid;
};

// grid (ceil(nser / 32), ceil(nc / 32)), 256 threads; slot0 = slot of the call's first window, slot0 + nc <= NT
template <int NPROD>
__global__ __launch_bounds__(256) void plong_ingest_kernel(const float* __restrict__ in, float* __restrict__ tbuf, int nser, int NT, int slot0, int nc) {
    __shared__ float tile[PL_TILE][PL_TILE + 1];
    const int s0 = blockIdx.x * PL_TILE, t0 = blockIdx.y * PL_TILE;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    for (int i = 0; i < PL_TILE / 8; i++) {
        const int tt = hi + 8 * i, t = t0 + tt, s = s0 + lo;
        if (t < nc && s < nser) {
            if constexpr (NPROD == 4) {
                const float4 v = ((const float4*)in)[(size_t)t * nser + s];
                tile[lo][tt] = v.x + v.y;
            } else {
                tile[lo][tt] = in[(size_t)t * nser + s];
            }
        }
    }
    __syncthreads();
    const int t = t0 + lo;
    if (t >= nc) return;
    for (int i = 0; i < PL_TILE / 8; i++) {
        const int ss = hi + 8 * i, s = s0 + ss;
        if (s >= nser) break;
        tbuf[(size_t)s * NT + slot0 + t] = tile[ss][lo];
    }
}

// M: grid nser, 256 threads.  N >= 1024.
__global__ __launch_bounds__(256) void plong_mean_kernel(const float* __restrict__ tbuf, PlongMean* __restrict__ mv, int LN) {
    __shared__ float wsum[4];
    const int N = 1 << LN, tid = threadIdx.x;
    const float2* const src = (const float2*)tbuf + ((size_t)blockIdx.x << LN);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int m = tid; m < N; m += 4 * PL_THREADS) {
        const float2 c0 = src[m], c1 = src[m + PL_THREADS], c2 = src[m + 2 * PL_THREADS], c3 = src[m + 3 * PL_THREADS];
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

// cl_sw of cdlong_kernels.h: a bijection of every aligned block of 32
__device__ __forceinline__ int pl_sw(int i) { return i ^ ((i & 32) ? 21 : 0) ^ ((i & 64) ? 31 : 0); }

// where element i of transform t lives: COL, the tiles of pass C (i < 512); else the rows of pass R
template <bool COL> __device__ __forceinline__ int pl_at(int i, int t, int ln) {
    if (COL) {
        int p = i >> 1;
        p ^= p >> 4;
        p ^= p >> 2;
        p ^= p >> 1;
        return ((i ^ (p & 1)) << PL_LTC) | t;
    }
    return (t << ln) | pl_sw(i);
}

// work item w of a pass with 2^lg items per transform: COL, the columns fastest; else the items of one row fastest
template <bool COL> __device__ __forceinline__ void pl_item(int w, int lg, int& q, int& t) {
    if (COL) {
        t = w & (PL_TC - 1);
        q = w >> PL_LTC;
    } else {
        q = w & ((1 << lg) - 1);
        t = w >> lg;
    }
}

__device__ __forceinline__ float2 pl_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// exp(-2 pi i k / n) for 0 <= k < n from the half table: tw[k + n/2] = -tw[k]
__device__ __forceinline__ float2 pl_twf(const float2* __restrict__ tw, int k, int n) {
    const int hi = k >= (n >> 1);
    const float2 w = tw[k - (hi ? (n >> 1) : 0)];
    return hi ? make_float2(-w.x, -w.y) : w;
}

// cl_fft_fwd of cdlong_kernels.h: 2^lt transforms of 2^ln points in LDS, forward, in place, decimation in frequency, natural
// order in and bit-reversed out; two radix-2 stages fused per pass, a last radix-2 stage where ln is odd.  tw: float2[2^ln / 2].
// Every thread of the work-group calls it; it ends behind a barrier.
template <bool COL> __device__ __forceinline__ void pl_fft_fwd(float2* lds, const float2* __restrict__ tw, int ln, int lt) {
    const int n = 1 << ln, tid = threadIdx.x;
    int lh = ln - 1;                                // log2 of the half-size h
    for (; lh >= 1; lh -= 2) {
        const int lq = lh - 1, hh = 1 << lq;        // hh = h / 2
        for (int w = tid; w < (n >> 2) << lt; w += PL_THREADS) {
            int q, t;
            pl_item<COL>(w, ln - 2, q, t);
            const int p = q & (hh - 1), a = ((q >> lq) << (lq + 2)) | p;
            const int i0 = pl_at<COL>(a, t, ln), i1 = pl_at<COL>(a + hh, t, ln), i2 = pl_at<COL>(a + 2 * hh, t, ln), i3 = pl_at<COL>(a + 3 * hh, t, ln);
            const float2 x0 = lds[i0], x1 = lds[i1], x2 = lds[i2], x3 = lds[i3];
            const float2 w1 = tw[p << (ln - 1 - lh)], w2 = tw[p << (ln - lh)], w3 = pl_twf(tw, 3 * p << (ln - 1 - lh), n);
            const float2 u0 = make_float2(x0.x + x2.x, x0.y + x2.y), d0 = make_float2(x0.x - x2.x, x0.y - x2.y);
            const float2 u1 = make_float2(x1.x + x3.x, x1.y + x3.y), d1 = make_float2(x1.x - x3.x, x1.y - x3.y);
            lds[i0] = make_float2(u0.x + u1.x, u0.y + u1.y);
            lds[i1] = pl_cmul(make_float2(u0.x - u1.x, u0.y - u1.y), w2);
            lds[i2] = pl_cmul(make_float2(d0.x + d1.y, d0.y - d1.x), w1);     // d0 - i d1
            lds[i3] = pl_cmul(make_float2(d0.x - d1.y, d0.y + d1.x), w3);     // d0 + i d1
        }
        __syncthreads();
    }
    if (lh == 0) {                                  // ln odd: the last stage, half-size 1, twiddle 1
        for (int w = tid; w < (n >> 1) << lt; w += PL_THREADS) {
            int q, t;
            pl_item<COL>(w, ln - 1, q, t);
            const int i0 = pl_at<COL>(2 * q, t, ln), i1 = pl_at<COL>(2 * q + 1, t, ln);
            const float2 x0 = lds[i0], x1 = lds[i1];
            lds[i0] = make_float2(x0.x + x1.x, x0.y + x1.y);
            lds[i1] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        __syncthreads();
    }
}

// C: grid (N2 / 16, SB), 256 threads, N1 * 16 * 8 bytes of dynamic LDS; ser0 is the batch's first series
__global__ __launch_bounds__(256) void plong_cols_kernel(const float* __restrict__ tbuf, const PlongMean* __restrict__ mv, float2* __restrict__ scr,
                                                         const float2* __restrict__ tw1, int LN1, int LN2, int ser0) {
    extern __shared__ float2 pl_lds[];
    const int N1 = 1 << LN1, tid = threadIdx.x;
    const size_t ser = (size_t)ser0 + blockIdx.y;
    const float2* const src = (const float2*)tbuf + (ser << (LN1 + LN2)) + (size_t)blockIdx.x * PL_TC;
    float2* const dst = scr + ((size_t)blockIdx.y << (LN1 + LN2)) + (size_t)blockIdx.x * PL_TC;
    const float mean = mv[ser].mean;
    for (int w = tid; w < N1 * PL_TC; w += PL_THREADS) {
        const int t = w & (PL_TC - 1), i = w >> PL_LTC;
        const float2 c = src[((size_t)i << LN2) + t];
        pl_lds[pl_at<true>(i, t, LN1)] = make_float2(c.x - mean, c.y - mean);
    }
    __syncthreads();
    pl_fft_fwd<true>(pl_lds, tw1, LN1, PL_LTC);
    for (int w = tid; w < N1 * PL_TC; w += PL_THREADS) {
        const int t = w & (PL_TC - 1), i = w >> PL_LTC;
        dst[((size_t)i << LN2) + t] = pl_lds[pl_at<true>(i, t, LN1)];
    }
}

// R: grid (N1 >> pl_lrows(LN2), SB), 256 threads, (N2 << pl_lrows(LN2)) * 8 bytes of dynamic LDS; in place in scr
__global__ __launch_bounds__(256) void plong_rows_kernel(float2* __restrict__ scr, const float2* __restrict__ tws, const float2* __restrict__ tw2, int LN1,
                                                         int LN2) {
    extern __shared__ float2 pl_lds[];
    const int LN = LN1 + LN2, N = 1 << LN, N2 = 1 << LN2, lr = pl_lrows(LN2), tid = threadIdx.x;
    const int r0 = blockIdx.x << lr;
    float2* const src = scr + ((size_t)blockIdx.y << LN) + ((size_t)r0 << LN2);
    for (int w = tid; w < N2 << lr; w += PL_THREADS) {
        const int m = w & (N2 - 1), t = w >> LN2;
        const int k1 = (int)(__brev((unsigned)(r0 + t)) >> (32 - LN1));
        pl_lds[pl_at<false>(m, t, LN2)] = pl_cmul(src[w], pl_twf(tws, m * k1, N));
    }
    __syncthreads();
    pl_fft_fwd<false>(pl_lds, tw2, LN2, lr);
    for (int w = tid; w < N2 << lr; w += PL_THREADS) {
        const int m = w & (N2 - 1), t = w >> LN2;
        src[w] = pl_lds[pl_at<false>(m, t, LN2)];
    }
}

// U: grid (N2 / 16, SB), 256 threads, 16 * (N1 + 2) * 4 bytes of dynamic LDS
__global__ __launch_bounds__(256) void plong_power_kernel(const float2* __restrict__ scr, const float2* __restrict__ tw, float* __restrict__ P, int LN1,
                                                          int LN2) {
    extern __shared__ float2 pl_lds[];
    float* const ldsf = (float*)pl_lds;
    const int LN = LN1 + LN2, N = 1 << LN, N1 = 1 << LN1, tid = threadIdx.x;
    const int j0 = blockIdx.x * PL_TC;
    const float2* const Z = scr + ((size_t)blockIdx.y << LN);
    for (int w = tid; w < N1 * PL_TC; w += PL_THREADS) {
        const int jj = w & (PL_TC - 1), k1 = w >> PL_LTC, j = j0 + jj;
        const int r = (int)(__brev((unsigned)k1) >> (32 - LN1)), k2 = (int)(__brev((unsigned)j) >> (32 - LN2));
        const int k = k1 | (k2 << LN1), kp = (N - k) & (N - 1);
        const int rp = (int)(__brev((unsigned)(kp & (N1 - 1))) >> (32 - LN1)), jp = (int)(__brev((unsigned)(kp >> LN1)) >> (32 - LN2));
        const float2 za = Z[((size_t)r << LN2) + j], zb = Z[((size_t)rp << LN2) + jp], wk = tw[k];
        const float2 E = make_float2(0.5f * (za.x + zb.x), 0.5f * (za.y - zb.y));
        const float2 O = make_float2(0.5f * (za.y + zb.y), -0.5f * (za.x - zb.x));
        const float2 wo = pl_cmul(O, wk);
        const float2 xa = make_float2(E.x + wo.x, E.y + wo.y);
        ldsf[jj * (N1 + PL_PPAD) + k1] = xa.x * xa.x + xa.y * xa.y;
    }
    __syncthreads();
    float* const dst = P + ((size_t)blockIdx.y << LN);
    for (int w = tid; w < N1 * PL_TC; w += PL_THREADS) {
        const int k1 = w & (N1 - 1), jj = w >> LN1;
        const int k2 = (int)(__brev((unsigned)(j0 + jj)) >> (32 - LN2));
        dst[k1 | (k2 << LN1)] = ldsf[jj * (N1 + PL_PPAD) + k1];
    }
}

// W: grid (N >> pl_lwhite(lb), SB), 256 threads, (4 << pl_lwhite(lb)) bytes of dynamic LDS.  lb = log2 B.  first: the segment
// opens its stack (A is stored, not added to).
__global__ __launch_bounds__(256) void plong_whiten_kernel(const float* __restrict__ P, float* __restrict__ A, const unsigned char* __restrict__ keep,
                                                           const float* __restrict__ cnt, const PlongMean* __restrict__ mv, int LN, int lb, int first,
                                                           int ser0) {
    extern __shared__ float2 pl_lds[];
    float* const tree = (float*)pl_lds;
    const int lw = pl_lwhite(lb), W = 1 << lw, tid = threadIdx.x;
    const int k00 = blockIdx.x << lw;
    const size_t ser = (size_t)ser0 + blockIdx.y;
    const float* const Prow = P + ((size_t)blockIdx.y << LN) + k00;
    float* const Arow = A + (ser << LN) + k00;
    const unsigned char* const kp = keep + k00;
    // block sums: a pairwise tree, level by level behind one another
    for (int i = tid; i < W / 2; i += PL_THREADS) {
        const float2 p = ((const float2*)Prow)[i];
        const float a = (k00 + 2 * i >= 1 && kp[2 * i]) ? p.x : 0.f;
        const float b = kp[2 * i + 1] ? p.y : 0.f;
        tree[i] = a + b;
    }
    int off = 0, n = W / 2;
    for (int l = 1; l < lb; l++) {
        __syncthreads();
        const int dst = off + n;
        for (int i = tid; i < n / 2; i += PL_THREADS) {
            const float2 v = ((const float2*)(tree + off))[i];      // (off is even: one 8-byte read, every bank once)
            tree[dst + i] = v.x + v.y;
        }
        off = dst;
        n >>= 1;
    }
    __syncthreads();                                // block b of the run: tree[off + b]
    const bool whole = mv[ser].valid != 0;          // a finite mean: otherwise the series is NaN from here on
    const float* const crow = cnt + (k00 >> lb);
    for (int k = tid; k < W; k += PL_THREADS) {
        const int b = k >> lb;
        const float c = crow[b], mu = tree[off + b] / c;
        float S = 1.0f;
        if (c > 0.f && mu > 0.f && mu < __int_as_float(0x7f800000) && kp[k]) S = Prow[k] / mu;
        if (!whole) S = __int_as_float(0x7fc00000);
        if (k00 + k == 0) S = 0.f;
        Arow[k] = first ? S : Arow[k] + S;
    }
}

// larger H, then smaller k; a NaN never enters
__device__ __forceinline__ void pl_take(PlongRecord& b, float H, int k) {
    if (H != H) return;
    if (b.k < 0 || H > b.H || (H == b.H && k < b.k)) {
        b.H = H;
        b.k = k;
    }
}

// S: grid (16, SB), 256 threads.  part: [SB][nlevel][nband][16]
__global__ __launch_bounds__(256) void plong_sums_kernel(const float* __restrict__ A, const int* __restrict__ kedge, PlongRecord* __restrict__ part, int LN,
                                                         int nlevel, int nband, int ser0) {
    __shared__ int edge[PL_MAX_BAND + 1];
    __shared__ PlongRecord mail[PL_MAX_LEVEL][PL_MAX_BAND][4];
    const int N = 1 << LN, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = N >> PL_LNTILE, t0 = blockIdx.x * T, t1 = t0 + T;
    const float* const Arow = A + (((size_t)ser0 + blockIdx.y) << LN);
    if (tid <= nband) edge[tid] = kedge[tid];
    __syncthreads();
    {
#pragma clang fp contract(off)
        for (int l = 0; l < nlevel; l++) {
            const int h = 1 << l;
            for (int b = 0; b < nband; b++) {
                int lo = edge[b] << l, hi = edge[b + 1] << l;       // (16 * 2^19 at most)
                if (lo < t0) lo = t0;
                if (hi > t1) hi = t1;
                PlongRecord best = {0.f, -1};
                if (lo < hi) {                      // (the same for every thread of the work-group)
                    for (int k = lo + tid; k < hi; k += PL_THREADS) {
                        float H = Arow[(k + (h >> 1)) >> l];
                        for (int j = 2; j <= h; j++) H = H + Arow[(j * k + (h >> 1)) >> l];
                        pl_take(best, H, k);
                    }
                    for (int o = 32; o; o >>= 1) {
                        const float oH = __shfl_xor(best.H, o);
                        const int ok = __shfl_xor(best.k, o);
                        if (ok >= 0) pl_take(best, oH, ok);
                    }
                }
                if (lane == 0) mail[l][b][wave] = best;
            }
        }
    }
    __syncthreads();
    PlongRecord* const dst = part + (((size_t)blockIdx.y * nlevel * nband) << PL_LNTILE) + blockIdx.x;
    for (int i = tid; i < nlevel * nband; i += PL_THREADS) {
        const int l = i / nband, b = i - l * nband;
        PlongRecord best = {0.f, -1};
        for (int w = 0; w < 4; w++)
            if (mail[l][b][w].k >= 0) pl_take(best, mail[l][b][w].H, mail[l][b][w].k);
        dst[(size_t)i << PL_LNTILE] = best;
    }
}

// D: grid ceil(nrec / 256), 256 threads: record i of the batch from its 16 partials; out is the batch's first record
__global__ __launch_bounds__(256) void plong_reduce_kernel(const PlongRecord* __restrict__ part, PlongRecord* __restrict__ out, long long nrec) {
    const long long i = (long long)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= nrec) return;
    PlongRecord best = {0.f, -1};
    for (int t = 0; t < PL_NTILE; t++) {
        const PlongRecord p = part[((size_t)i << PL_LNTILE) + t];
        if (p.k >= 0) pl_take(best, p.H, p.k);
    }
    out[i] = best;
}

}  // namespace xeng
