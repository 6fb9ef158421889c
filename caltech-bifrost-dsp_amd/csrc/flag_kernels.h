// Robust outlier flags from the fine-channel visibilities (xengFlag*, flag.hip): one pass over UpchanCorr's matrix for per-(channel,
// polarisation, stand) statistics, then median / MAD tests over the stands of each (channel, pol) and over the channels of each pol.
//
// Contract (include/xeng.h, "Outlier flags from the fine-channel visibilities"); ninput = 2 nstand, row i = 2 s + p, column j = 2 t + q:
//   vis    cf32[nfine][nstand][2][nstand][2], UpchanCorr's span V[c][s p][t q]; only the words i >= j with p = q are used; never written
//   w      f32[nstand] (the context's state): on / off.  A word of a stand with w = 0 is not loaded.
//   zero   16 bytes of zeros (state): where a lane that has no word to load reads
//   part   f32[nfine][2][nstand][ntile] (state): part[c][p][s][K] = sum over the stands t of tile K, ascending, t != s, of |V[c][s p][t p]|^2
//   autos  f32[nfine][2][nstand] (state): Re V[c][s p][s p]
//   stats  f32[nfine][2][nstand][2] = {R, A}, mask u8[nfine][2][nstand], chan f32[nfine][2][4] = {med_R, mad_R, b, n}
//
// flag_stats_kernel: one work-group of ONE wave per (fine channel, pair of 32-stand tiles I >= J), grid (ntile (ntile + 1) / 2, nfine):
// calapply_kernel's grid.  The bound is HBM: every 128-byte line of the lower triangle is fetched exactly once, 32 KiB per
// work-group, and 8.5 KiB of LDS per work-group leaves room for 18 waves per CU with 16 KiB of loads in flight each.
//   1. lane (r, h) reads, of the rows of the stands s0 + 8 g + 4 h + u (g, u = 0 .. 3) and both p, the word q = p at column stand
//      t0 + r: 32 loads of 8 bytes, all issued before the first is used.  (The parallel hand is every other 8-byte word of a row, so
//      a 16-byte load of the pair [t][q = 0, 1] carries one word that a select drops; with p known at compile time the compiler
//      narrows such a load to these 8 bytes anyway.  The 128-byte lines that come from HBM are the same: all of the lower
//      triangle, once.  The cross hands are never loaded.)  A word that is not needed -- a stand of weight 0, past the matrix,
//      above the diagonal of a diagonal tile -- is not loaded: the lane's address is turned to 16 bytes of zeros in the context's
//      state (`zero`), so that the loads are unconditional instructions in flight together; behind branches they went out one at
//      a time.  m = fma(re, re, im * im) goes to the LDS image M[p][s][t] of the tile (pitch FL_PITCH = 33), +0 where the word
//      was left out.  In a diagonal tile only t <= s is loaded: m of t < s is written to M[p][s][t] and to M[p][t][s] (|V[s][t]|^2
//      = |V[t][s]|^2 of a Hermitian matrix: every unordered pair counts once for each of its two stands), M[p][s][s] is +0 and
//      the auto's real part is split off into its own 64 words.
//   2. after one barrier lane l = 32 p + x adds row x of M[p] in ascending column order from +0: the partial of stand s0 + x from
//      tile J; and, off the diagonal, column x in ascending row order: the partial of stand t0 + x from tile I.  One owner per
//      word of part; no atomics.
// So R[c][p][s] = sum over the tiles K ascending of (sum over the stands t of tile K ascending of m), both from +0 by plain fp32 adds
// (flag_test_kernel does the outer sum), the words left out adding +0.  Tiles are 32 stands whatever nstand: R does not depend on
// nstand, on the other channels or on anything else that runs.
// LDS banks: the image is written along r (consecutive dwords) and, mirrored, at stride 33; it is read along a row at stride 33
// across the lanes and along a column at consecutive dwords: no conflicts.  24 KiB of LDS traffic beside 32 KiB of HBM traffic.
//
// flag_test_kernel: one work-group of 512 threads per (c, p), grid (2, nfine).  Thread s owns stand s: adds its partials in ascending
// tile order, writes stats, then the medians by exact selection: a live value's rank is the count of live values below it (ties by
// stand index), and the values of rank (n - 1) / 2 and n / 2 are the median's.  Two selections, each for two tables at once (R and A,
// then |R - med| and |A - med|), of nstand^2 compares per table, on sortable integer keys of the values (fl_key; a stand that is not
// live holds a key above all others), read from LDS 16 bytes at a time: one compare and one add per pair.  Writes stats, the bits 0, 1, 3, 4 of mask and chan[0, 1, 3].  The compares are this kernel's time: 4 nstand^2 of
// them on one CU.
//
// flag_chan_kernel: one work-group of 1024 threads per p, grid (2).  The keys of y = med_R of up to FL_MAX_NFINE channels in LDS;
// the baseline b per channel (a selection within the window, one thread per channel; or one selection over all channels), |y - b|
// over y in place, its median by the same selection, then bit 2 into mask (a byte read-modify-write by one owner, after
// flag_test_kernel on the same stream) and chan[2].  The selections over all channels are nfine^2 compares: nothing at the hundreds
// of channels of a dump, milliseconds at FL_MAX_NFINE.
// No atomics, no scalar memory writes, no printf.
//
// flag.hip is compiled with -fno-slp-vectorize (Makefile) with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int FL_T = 32;             // stands per tile
constexpr int FL_THREADS = 64;       // one wave
constexpr int FL_PITCH = 33;         // floats per row of the tile's image
constexpr int FL_MAX_NSTAND = 512;
constexpr int FL_MAX_NFINE = 8192;
constexpr int FL_MAX_WCHAN = 64;
constexpr int FL_TEST_THREADS = FL_MAX_NSTAND;              // flag_test_kernel: one stand per thread
constexpr int FL_CHAN_THREADS = 1024;
constexpr int FL_CPER = FL_MAX_NFINE / FL_CHAN_THREADS;     // channels per thread of flag_chan_kernel
constexpr float FL_FLT_MAX = 3.40282346638528859812e+38f;

__host__ __device__ constexpr size_t flag_stats_lds_bytes() { return (size_t)(2 * FL_T * FL_PITCH + 2 * FL_T) * sizeof(float); }
__host__ __device__ constexpr size_t flag_test_lds_bytes() { return (size_t)FL_MAX_NSTAND * 2 * sizeof(float) + 4 * sizeof(float); }
__host__ __device__ constexpr size_t flag_chan_lds_bytes() { return (size_t)FL_MAX_NFINE * (sizeof(float) + 1) + 2 * sizeof(float); }

__device__ __forceinline__ bool fl_finite(float x) { return __builtin_fabsf(x) <= FL_FLT_MAX; }     // false for NaN and Inf

// grid (ntile (ntile + 1) / 2, nfine) with ntile = ceil(nstand / FL_T), FL_THREADS threads; vis 16-byte aligned
__global__ __launch_bounds__(FL_THREADS) void flag_stats_kernel(const float2* __restrict__ vis, const float* __restrict__ w, const float2* __restrict__ zero,
                                                                float* __restrict__ part, float* __restrict__ autos, int nstand) {
    __shared__ __attribute__((aligned(16))) float fl_m[2 * FL_T * FL_PITCH + 2 * FL_T];
    float* fl_a = fl_m + 2 * FL_T * FL_PITCH;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int c = blockIdx.y;
    int S = 0, T = blockIdx.x;                                   // blockIdx.x = S (S + 1) / 2 + T, T <= S
    while (T > S) {
        T -= S + 1;
        S++;
    }
    const int s0 = S * FL_T, t0 = T * FL_T;
    const bool diag = S == T;
    const size_t ninput = 2 * (size_t)nstand;
    const int ntile = (nstand + FL_T - 1) / FL_T;
    const int t = t0 + r;
    // the weights of the tile's row stands go through LDS (one load per lane, not one per row): fl_a is free until the image is written
    const float wt = t < nstand ? w[t] : 0.f, ws = s0 + r < nstand ? w[s0 + r] : 0.f;
    const bool tl = wt > 0.f;
    if (h == 0) fl_a[r] = ws;
    __syncthreads();
    float wrow[16];
#pragma unroll
    for (int k = 0; k < 16; k++) wrow[k] = fl_a[8 * (k >> 2) + 4 * h + (k & 3)];
    __syncthreads();
    const float2* vc = vis + (size_t)c * ninput * ninput;

    // every load of the tile is issued before the first word is used: 32 loads of 8 bytes per lane in flight
    float2 v[32];
    bool lv[32];
#pragma unroll
    for (int e = 0; e < 32; e++) {
        const int g = e >> 3, u = (e >> 1) & 3, p = e & 1;
        const int s = s0 + 8 * g + 4 * h + u;
        lv[e] = tl && wrow[e >> 1] > 0.f && (!diag || t <= s);
        v[e] = *(lv[e] ? vc + (size_t)(2 * s + p) * ninput + 2 * t + p : zero);
    }
#pragma unroll
    for (int e = 0; e < 32; e++) {
        const int g = e >> 3, u = (e >> 1) & 3, p = e & 1;
        const int x = 8 * g + 4 * h + u, s = s0 + x;
        const float re = v[e].x, im = v[e].y;
        const float m = lv[e] ? __builtin_fmaf(re, re, im * im) : 0.f;
        if (!diag) {
            fl_m[(p * FL_T + x) * FL_PITCH + r] = m;
        } else if (t < s) {
            fl_m[(p * FL_T + x) * FL_PITCH + r] = m;
            fl_m[(p * FL_T + r) * FL_PITCH + x] = m;
        } else if (t == s) {
            fl_m[(p * FL_T + x) * FL_PITCH + r] = 0.f;
            fl_a[p * FL_T + x] = lv[e] ? re : 0.f;
        }
    }
    __syncthreads();
    const int p = lane >> 5, x = lane & 31;
    float row = 0.f;
#pragma unroll
    for (int k = 0; k < FL_T; k++) row += fl_m[(p * FL_T + x) * FL_PITCH + k];
    const size_t cp = ((size_t)c * 2 + p) * nstand;
    if (s0 + x < nstand) part[(cp + s0 + x) * ntile + T] = row;
    if (!diag) {
        float col = 0.f;
#pragma unroll
        for (int k = 0; k < FL_T; k++) col += fl_m[(p * FL_T + k) * FL_PITCH + x];
        if (t0 + x < nstand) part[(cp + t0 + x) * ntile + S] = col;
    } else if (s0 + x < nstand) {
        autos[cp + s0 + x] = fl_a[p * FL_T + x];
    }
}

// The selections compare sortable keys, not floats: fl_key is monotonic over the finite floats (-0 taken as +0), and FL_DEAD, above
// every key, marks an entry that takes no part.
constexpr unsigned FL_DEAD = 0xFFFFFFFFu;
__device__ __forceinline__ unsigned fl_key(float v) {
    const unsigned u = __float_as_uint(v + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The rank of key kv, which sits at index `at`, among k[0 .. 4 n4): the count of keys below it, ties by index.  Chunks of four keys
// before the one that holds `at` count their keys <= kv (< kv + 1), the others their keys < kv: one compare and one add per key;
// the keys of kv's own chunk that sit before it and equal it are added at the end.  fl_rank(k, n4, FL_DEAD, 0) counts the live keys.
__device__ __forceinline__ int fl_rank(const unsigned* k, int n4, unsigned kv, int at) {
    const int qs = at >> 2, j = at & 3;
    int rank = 0;
    for (int q = 0; q < n4; q++) {
        const uint4 x = ((const uint4*)k)[q];
        const unsigned thr = q < qs ? kv + 1u : kv;
        rank += (x.x < thr ? 1 : 0) + (x.y < thr ? 1 : 0) + (x.z < thr ? 1 : 0) + (x.w < thr ? 1 : 0);
    }
    const uint4 x = ((const uint4*)k)[qs];
    rank += (j > 0 && x.x == kv ? 1 : 0) + (j > 1 && x.y == kv ? 1 : 0) + (j > 2 && x.z == kv ? 1 : 0);
    return rank;
}

// The medians of two tables at once (R and A, then their deviations): thread s brings its stand's two values, or live = false.  The
// keys go to LDS, FL_DEAD at every stand that is not live (and up to the next multiple of 4).  n, the number of live stands, is
// counted when it comes in negative.  The threads whose rank is (n - 1) / 2 or n / 2 leave their value, and the median is v[n / 2]
// for odd n and 0.5f * (v[(n - 1) / 2] + v[n / 2]) for even n.  With n = 0 the medians are not defined (the caller takes none below
// n = 4).  Every thread of the work-group calls it.
__device__ __forceinline__ void fl_median2(unsigned (*fl_k)[FL_MAX_NSTAND], float* fl_sel, float v0, float v1, bool live, int nstand, int* n_io, float* m0,
                                           float* m1) {
    const int s = threadIdx.x, n4 = (nstand + 3) >> 2;
    const unsigned k0 = live ? fl_key(v0) : FL_DEAD, k1 = live ? fl_key(v1) : FL_DEAD;
    fl_k[0][s] = k0;
    fl_k[1][s] = k1;
    __syncthreads();
    const int n = *n_io < 0 ? fl_rank(fl_k[0], n4, FL_DEAD, 0) : *n_io;
    if (live) {
        const int r0 = fl_rank(fl_k[0], n4, k0, s), r1 = fl_rank(fl_k[1], n4, k1, s);
        if (r0 == (n - 1) / 2) fl_sel[0] = v0;
        if (r0 == n / 2) fl_sel[1] = v0;
        if (r1 == (n - 1) / 2) fl_sel[2] = v1;
        if (r1 == n / 2) fl_sel[3] = v1;
    }
    __syncthreads();
    *m0 = (n & 1) ? fl_sel[1] : 0.5f * (fl_sel[0] + fl_sel[1]);
    *m1 = (n & 1) ? fl_sel[3] : 0.5f * (fl_sel[2] + fl_sel[3]);
    *n_io = n;
    __syncthreads();                                             // (fl_k and fl_sel are free for the next selection)
}

// grid (2, nfine), FL_TEST_THREADS threads: thread s owns stand s
__global__ __launch_bounds__(FL_TEST_THREADS) void flag_test_kernel(const float* __restrict__ part, const float* __restrict__ autos, const float* __restrict__ w,
                                                                    unsigned char* __restrict__ mask, float* __restrict__ stats, float* __restrict__ chan, int nstand,
                                                                    float k_cross, float k_auto) {
    __shared__ __attribute__((aligned(16))) unsigned fl_k[2][FL_MAX_NSTAND];
    __shared__ float fl_sel[4];
    const int s = threadIdx.x, p = blockIdx.x, c = blockIdx.y;
    const int ntile = (nstand + FL_T - 1) / FL_T;
    const size_t cp = ((size_t)c * 2 + p) * nstand;
    float R = 0.f, A = 0.f;
    bool live = false;
    unsigned bits = 0;
    if (s < nstand) {
        const bool on = w[s] > 0.f;
        if (on) {
            for (int K = 0; K < ntile; K++) R += part[(cp + s) * ntile + K];
            A = autos[cp + s];
        }
        stats[(cp + s) * 2] = R;
        stats[(cp + s) * 2 + 1] = A;
        const bool fin = fl_finite(R) && fl_finite(A);
        live = on && fin;
        bits = on ? (fin ? 0u : 8u) : 16u;
    }
    int n = -1;
    float med_r, med_a, mad_r = 0.f, mad_a;
    fl_median2(fl_k, fl_sel, R, A, live, nstand, &n, &med_r, &med_a);
    if (n >= 4) {                                                // (uniform)
        const float dr = __builtin_fabsf(R - med_r), da = __builtin_fabsf(A - med_a);
        fl_median2(fl_k, fl_sel, dr, da, live, nstand, &n, &mad_r, &mad_a);
        if (k_cross > 0.f && live && dr > k_cross * mad_r) bits |= 1u;
        if (k_auto > 0.f && live && da > k_auto * mad_a) bits |= 2u;
    } else {
        med_r = 0.f;
    }
    if (s < nstand) mask[cp + s] = (unsigned char)bits;
    if (s == 0) {
        float* ch = chan + ((size_t)c * 2 + p) * 4;
        ch[0] = med_r;
        ch[1] = mad_r;
        ch[3] = (float)n;
    }
}

// The median of the values whose keys in fl_k[0 .. 4 n4) are not FL_DEAD, the definition of fl_median2; +0 if there is none.  val[e]
// is the value of channel tid + e FL_CHAN_THREADS.  Every thread calls it.
__device__ __forceinline__ float fl_median_all(const unsigned* fl_k, float* fl_cs, const float* val, int nfine) {
    const int n4 = (nfine + 3) >> 2;
    const int n = fl_rank(fl_k, n4, FL_DEAD, 0);
#pragma unroll
    for (int e = 0; e < FL_CPER; e++) {
        const int c = (int)threadIdx.x + e * FL_CHAN_THREADS;
        if (c < nfine && fl_k[c] != FL_DEAD) {
            const int rank = fl_rank(fl_k, n4, fl_k[c], c);
            if (rank == (n - 1) / 2) fl_cs[0] = val[e];
            if (rank == n / 2) fl_cs[1] = val[e];
        }
    }
    __syncthreads();
    const float lo = fl_cs[0], hi = fl_cs[1];
    __syncthreads();
    return n == 0 ? 0.f : (n & 1) ? hi : 0.5f * (lo + hi);
}

// grid (2), FL_CHAN_THREADS threads; after flag_test_kernel on the same stream
__global__ __launch_bounds__(FL_CHAN_THREADS) void flag_chan_kernel(unsigned char* __restrict__ mask, float* __restrict__ chan, int nstand, int nfine, float k_chan,
                                                                    int wchan) {
    __shared__ __attribute__((aligned(16))) unsigned fl_k[FL_MAX_NFINE];    // the keys of y, then of |r|; FL_DEAD for a channel without a y
    __shared__ unsigned char fl_f[FL_MAX_NFINE];                            // channel flagged
    __shared__ float fl_cs[2];
    const int tid = threadIdx.x, p = blockIdx.x;
    float y[FL_CPER], b[FL_CPER], ar[FL_CPER];
    bool has[FL_CPER];
#pragma unroll
    for (int e = 0; e < FL_CPER; e++) {
        const int c = tid + e * FL_CHAN_THREADS;
        y[e] = b[e] = ar[e] = 0.f;
        has[e] = false;
        if (c < nfine) {
            const float* ch = chan + ((size_t)c * 2 + p) * 4;
            has[e] = ch[3] >= 4.f;
            y[e] = ch[0];
        }
        if (c < ((nfine + 3) & ~3)) fl_k[c] = has[e] ? fl_key(y[e]) : FL_DEAD;
    }
    __syncthreads();
    if (wchan == 0) {                                            // (uniform)
        const float all = fl_median_all(fl_k, fl_cs, y, nfine);
#pragma unroll
        for (int e = 0; e < FL_CPER; e++) b[e] = all;
    } else {
#pragma unroll
        for (int e = 0; e < FL_CPER; e++) {
            const int c = tid + e * FL_CHAN_THREADS;
            if (c < nfine && has[e]) {
                const int lo = c - wchan < 0 ? 0 : c - wchan, hi = c + wchan > nfine - 1 ? nfine - 1 : c + wchan;
                int nw = 0;
                for (int a = lo; a <= hi; a++) nw += fl_k[a] != FL_DEAD ? 1 : 0;
                unsigned klo = 0, khi = 0;
                for (int a = lo; a <= hi; a++) {
                    const unsigned kv = fl_k[a];
                    if (kv == FL_DEAD) continue;
                    int rank = 0;
                    for (int t = lo; t <= hi; t++) rank += (fl_k[t] < kv || (fl_k[t] == kv && t < a)) ? 1 : 0;
                    if (rank == (nw - 1) / 2) klo = kv;
                    if (rank == nw / 2) khi = kv;
                }
                // (y >= +0: the key of a value that is not negative is its bits with the sign set)
                const float vlo = __uint_as_float(klo & 0x7FFFFFFFu), vhi = __uint_as_float(khi & 0x7FFFFFFFu);
                b[e] = (nw & 1) ? vhi : 0.5f * (vlo + vhi);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < FL_CPER; e++) {
        const int c = tid + e * FL_CHAN_THREADS;
        if (c < nfine) {
            if (has[e])
                ar[e] = __builtin_fabsf(y[e] - b[e]);
            else
                b[e] = 0.f;
            chan[((size_t)c * 2 + p) * 4 + 2] = b[e];
        }
    }
    __syncthreads();                                             // (every key of y has been read)
#pragma unroll
    for (int e = 0; e < FL_CPER; e++) {
        const int c = tid + e * FL_CHAN_THREADS;
        if (c < nfine) fl_k[c] = has[e] ? fl_key(ar[e]) : FL_DEAD;
    }
    __syncthreads();
    const float thr = k_chan * fl_median_all(fl_k, fl_cs, ar, nfine);
#pragma unroll
    for (int e = 0; e < FL_CPER; e++) {
        const int c = tid + e * FL_CHAN_THREADS;
        if (c < nfine) fl_f[c] = (!has[e] || (k_chan > 0.f && ar[e] > thr)) ? 1 : 0;
    }
    __syncthreads();
    const unsigned total = (unsigned)nfine * (unsigned)nstand;
    for (unsigned idx = tid; idx < total; idx += FL_CHAN_THREADS) {
        const unsigned c = idx / (unsigned)nstand, s = idx - c * (unsigned)nstand;
        if (fl_f[c]) {
            unsigned char* mp = mask + ((size_t)c * 2 + p) * nstand + s;
            *mp = (unsigned char)(*mp | 4u);
        }
    }
}

}  // namespace xeng
