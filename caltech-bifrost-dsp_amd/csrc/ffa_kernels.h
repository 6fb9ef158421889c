// Fast-folding search of the dedispersed beams (xengFfa*, ffa.hip): per series a segment of NT downsampled samples is folded at every
// integer base period p in pmin..pmax and at the M fractional periods between p and p + 1 that the fast folding algorithm gives for
// free, in noct octaves of the time resolution; a circular boxcar matched filter runs over every folded profile, and one peak record
// per series, octave and boxcar width comes out.
//
// Contract (include/xeng.h, "Fast-folding search of the dedispersed beams"); a series is one (pair, trial), nser = npair*ndm,
// N_o = NT >> o, XW = N_0 + ... + N_{noct-1} < 2 NT:
//   in     f32[nc][nser][NPROD], z = word 0 (NPROD = 1) or word 0 + word 1 (NPROD = 4)
//   tbuf   f32[nser][NT], sample k = the sequential sum of the windows [k*nds, (k+1)*nds) at slot k
//   part   f32[2][nser], the running sum of a sample whose windows a call has cut: a call reads one half and writes the other
//   xbuf   f32[nser][XW], octave o at the offset N_0 + ... + N_{o-1}: first u_o, then x_o in its place
//   stats  f32[nser][noct][4] = {c, m, v, g}
//   rho    f32[FA_MAX_WIDTH][FA_RHO_STRIDE], rho[iw][log2 M] = (float)(1 / sqrt(2^iw * M)), float64 on the host, rounded once
//   table  FfaRecord[nser][noct][np][nwidth], np = pmax - pmin + 1: the best of one base period
//   out    FfaRecord[nser][noct][nwidth], one 16-byte store each
//
// Ingest, every call: a work-group moves a tile of 32 series x 32 samples through LDS (rows padded by one word): loads consecutive
// across lanes along the series, one per window of the sample in ascending window order (the downsample chain), 4-byte stores
// consecutive across lanes along time.  A sample whose first windows came with an earlier call starts from part; one whose last
// windows are still to come goes to the other half of part instead of tbuf.
//
// Prepare, once per completed segment, one work-group per series: the octave pyramid into xbuf, then per octave the pivoted sums a
// and q (per thread, per wave by shuffles, the four waves through LDS), {c, m, v, g}, and x_o over u_o.
//
// Fold, once per completed segment and octave, one work-group per (series, base period): M*p words of x_o come into LDS and the
// log2 M stages run between two buffers of M*p words, one barrier a stage; every output word is one add of two words of the stage
// before.  Then the boxcar tree between the same two buffers; each thread keeps its best (S, i*p + j) per width in registers, and
// after the last width the work-group's best per width is reduced through 16 KiB of static LDS and five shuffles and stored in the
// table.  Lanes run along j: consecutive words apart from one wrap per row.  Two buffers rather than the in-place schedule:
// DESIGN.md 4.31.
//
// Reduce: one thread per (series, octave, width) takes the maximum of the table in ascending p.
//
// No atomics; every word has one owner; no work-group waits for another.  The only products are the two of the score and the ones
// of the statistics, written as fmaf where they are fused.
//
// ffa.hip is compiled with -fno-slp-vectorize (Makefile), with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int FA_THREADS = 256;
constexpr int FA_TILE = 32;         // ingest tile: series x samples
constexpr int FA_MAX_OCT = 6;
constexpr int FA_MAX_WIDTH = 8;
constexpr int FA_RHO_STRIDE = 16;   // log2 M <= 10 (M*p <= 2^14, p >= 16)

struct alignas(16) FfaRecord {
    float snr;
    int p, i, j;
};

struct FfaRinv {
    float r[FA_MAX_OCT];            // 1 / N_o, float64 on the host, rounded once
};

// grid (ceil(nser / 32), ceil(nk / 32)), 256 threads.  The call's windows are [w0, w0 + nc) of the segment, w0 + nc <= NT * nds; nk
// is the number of samples they touch.
template <int NPROD>
__global__ __launch_bounds__(256) void ffa_ingest_kernel(const float* __restrict__ in, float* __restrict__ tbuf, const float* __restrict__ part_in,
                                                         float* __restrict__ part_out, int nser, int NT, int nds, int w0, int nc) {
    __shared__ float tile[FA_TILE][FA_TILE + 1];
    const int s0 = blockIdx.x * FA_TILE, t0 = blockIdx.y * FA_TILE;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    const int k0 = w0 / nds, wend = w0 + nc, nk = (wend - 1) / nds - k0 + 1;
    for (int i = 0; i < FA_TILE / 8; i++) {
        const int tt = hi + 8 * i, t = t0 + tt, s = s0 + lo;
        if (t < nk && s < nser) {
            int wa = (k0 + t) * nds, wb = wa + nds;
            const bool cont = wa < w0, open = wb > wend;    // begun by an earlier call; to be finished by a later one
            if (cont) wa = w0;
            if (open) wb = wend;
            float acc = 0.f;
            for (int w = wa; w < wb; w++) {
                float z;
                if constexpr (NPROD == 4) {
                    const float4 v = ((const float4*)in)[(size_t)(w - w0) * nser + s];
                    z = v.x + v.y;
                } else {
                    z = in[(size_t)(w - w0) * nser + s];
                }
                if (w == wa)
                    acc = cont ? part_in[s] + z : z;
                else
                    acc = acc + z;
            }
            if (open)
                part_out[s] = acc;
            else
                tile[lo][tt] = acc;
        }
    }
    __syncthreads();
    const int t = t0 + lo;
    if (t >= nk || (k0 + t + 1) * nds > wend) return;
    for (int i = 0; i < FA_TILE / 8; i++) {
        const int ss = hi + 8 * i, s = s0 + ss;
        if (s >= nser) break;
        tbuf[(size_t)s * NT + k0 + t] = tile[ss][lo];
    }
}

// grid nser, 256 threads
__global__ __launch_bounds__(256) void ffa_prepare_kernel(const float* __restrict__ tbuf, float* xbuf, float* __restrict__ stats, FfaRinv rinv, int NT,
                                                          int noct) {
    __shared__ float mail[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ser = blockIdx.x;
    int XW = 0;
    for (int o = 0; o < noct; o++) XW += NT >> o;
    const float* src = tbuf + ser * NT;
    float* const x = xbuf + ser * XW;

    // the pyramid
    for (int k = tid; k < NT; k += FA_THREADS) x[k] = src[k];
    int off = 0;
    for (int o = 1; o < noct; o++) {
        __syncthreads();
        const float* below = x + off;
        off += NT >> (o - 1);
        float* u = x + off;
        for (int k = tid; k < (NT >> o); k += FA_THREADS) u[k] = below[2 * k] + below[2 * k + 1];
    }
    __syncthreads();

    // per octave the statistics, then x_o in place of u_o (each thread its own words)
    off = 0;
    for (int o = 0; o < noct; o++) {
        const int n = NT >> o;
        float* u = x + off;
        const float c = u[0];
        float a = 0.f, q = 0.f;
        for (int k = tid; k < n; k += FA_THREADS) {
            const float d = u[k] - c;
            a += d;
            q = fmaf(d, d, q);
        }
        for (int s = 32; s; s >>= 1) {
            a += __shfl_xor(a, s);
            q += __shfl_xor(q, s);
        }
        if (lane == 0) {
            mail[wave] = a;
            mail[4 + wave] = q;
        }
        __syncthreads();                            // (also: every thread has read c before thread 0 writes x_o[0] over it)
        a = ((mail[0] + mail[1]) + mail[2]) + mail[3];
        q = ((mail[4] + mail[5]) + mail[6]) + mail[7];
        __syncthreads();
        const float r = rinv.r[o];
        const float m = a * r;
        const float qr = q * r;
        const float v = fmaf(-m, m, qr);
        const float g = 1.0f / sqrtf(v);
        if (tid == 0) {
            float* st = stats + (ser * noct + o) * 4;
            st[0] = c;
            st[1] = m;
            st[2] = v;
            st[3] = g;
        }
        for (int k = tid; k < n; k += FA_THREADS) u[k] = (u[k] - c) - m;
        off += n;
    }
}

// larger S, then smaller e; a NaN never enters
__device__ __forceinline__ void fa_take(float& bS, int& bE, float S, int e) {
    if (S != S) return;
    if (bE < 0 || S > bS || (S == bS && e < bE)) {
        bS = S;
        bE = e;
    }
}

// grid (nser, np), 256 threads, 2 * (the octave's largest M * p) words of dynamic LDS; o is the octave
__global__ __launch_bounds__(256) void ffa_fold_kernel(const float* __restrict__ xbuf, const float* __restrict__ stats, const float* __restrict__ rho,
                                                       FfaRecord* __restrict__ table, int NT, int noct, int o, int pmin, int np, int nwidth) {
    extern __shared__ float fa_lds[];
    __shared__ float mailS[FA_MAX_WIDTH][FA_THREADS];
    __shared__ int mailE[FA_MAX_WIDTH][FA_THREADS];
    const int tid = threadIdx.x;
    const size_t ser = blockIdx.x;
    const int p = pmin + (int)blockIdx.y, N = NT >> o;
    int lm = 1;
    while ((p << (lm + 1)) <= N) lm++;              // M = 2^lm, the largest power of two with M * p <= N
    const int W = p << lm;
    FfaRecord* dst = table + ((ser * noct + o) * np + blockIdx.y) * nwidth;
    const float* st = stats + (ser * noct + o) * 4;
    const float m = st[1], v = st[2], g = st[3];
    const float inf = __int_as_float(0x7f800000);
    if (!(m == m && m < inf && m > -inf && v > 0.f && v < inf)) {
        if (tid < nwidth) dst[tid] = FfaRecord{0.f, -1, -1, -1};
        return;
    }
    int XW = 0, off = 0;
    for (int k = 0; k < noct; k++) {
        if (k < o) off += NT >> k;
        XW += NT >> k;
    }
    const float* x = xbuf + ser * XW + off;
    float* a = fa_lds;
    float* b = fa_lds + W;
    for (int e = tid; e < W; e += FA_THREADS) a[e] = x[e];
    __syncthreads();

    // word e = r * p + j of a buffer is column j of row r; a thread steps through its words without dividing
    const int dr = FA_THREADS / p, dj = FA_THREADS - dr * p;
    const int r0 = tid / p, j0 = tid - r0 * p;
    for (int l = 1; l <= lm; l++) {
        const int L = 1 << l;
        int r = r0, j = j0;
        for (int e = tid; e < W; e += FA_THREADS) {
            const int i = r & (L - 1), base = r - i, h = i >> 1;
            int jj = j + (int)((unsigned)((i + 1) >> 1) % (unsigned)p);
            if (jj >= p) jj -= p;
            b[e] = a[(base + h) * p + j] + a[(base + (L >> 1) + h) * p + jj];
            j += dj;
            r += dr;
            if (j >= p) {
                j -= p;
                r++;
            }
        }
        __syncthreads();
        float* t = a;
        a = b;
        b = t;
    }

    // boxcars and scores: a holds B_w, b takes B_2w
    float bS[FA_MAX_WIDTH];
    int bE[FA_MAX_WIDTH];
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int iw = 0; iw < FA_MAX_WIDTH; iw++) {
            bS[iw] = 0.f;
            bE[iw] = -1;
            if (iw < nwidth) {
                const float rh = rho[iw * FA_RHO_STRIDE + lm];
                const int w = 1 << iw;
                const bool more = iw + 1 < nwidth;
                int r = r0, j = j0;
                for (int e = tid; e < W; e += FA_THREADS) {
                    const float B = a[e];
                    const float Bg = B * g;
                    fa_take(bS[iw], bE[iw], Bg * rh, e);
                    if (more) {
                        int jj = j + w;
                        if (jj >= p) jj -= p;
                        b[e] = B + a[r * p + jj];
                        j += dj;
                        r += dr;
                        if (j >= p) {
                            j -= p;
                            r++;
                        }
                    }
                }
                if (more) {
                    __syncthreads();
                    float* t = a;
                    a = b;
                    b = t;
                }
            }
        }
    }

    // the work-group's best per width: every thread's into LDS, then 32 threads a width, each over 8 words and the 32 by shuffles
#pragma unroll
    for (int iw = 0; iw < FA_MAX_WIDTH; iw++) {
        if (iw < nwidth) {
            mailS[iw][tid] = bS[iw];
            mailE[iw][tid] = bE[iw];
        }
    }
    __syncthreads();
    const int mw = tid >> 5, ml = tid & 31;
    float S = 0.f;
    int E = -1;
    if (mw < nwidth)
        for (int k = 0; k < FA_THREADS / 32; k++)
            if (mailE[mw][ml + 32 * k] >= 0) fa_take(S, E, mailS[mw][ml + 32 * k], mailE[mw][ml + 32 * k]);
    for (int s = 16; s; s >>= 1) {                  // (xor below 32: a wave's two widths stay apart)
        const float oS = __shfl_xor(S, s);
        const int oE = __shfl_xor(E, s);
        if (oE >= 0) fa_take(S, E, oS, oE);
    }
    if (ml == 0 && mw < nwidth) dst[mw] = E < 0 ? FfaRecord{0.f, -1, -1, -1} : FfaRecord{S, p, E / p, E - (E / p) * p};
}

// one thread per (series, octave, width): the largest snr of the table in ascending p (among equals the first, the smallest p)
__global__ __launch_bounds__(256) void ffa_reduce_kernel(const FfaRecord* __restrict__ table, FfaRecord* __restrict__ out, long long nrec, int np,
                                                         int nwidth) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nrec) return;
    const long long so = t / nwidth;
    const int iw = (int)(t - so * nwidth);
    FfaRecord best = {0.f, -1, -1, -1};
    for (int pi = 0; pi < np; pi++) {
        const FfaRecord c = table[(so * np + pi) * nwidth + iw];
        if (c.p < 0 || c.snr != c.snr) continue;
        if (best.p < 0 || c.snr > best.snr) best = c;
    }
    out[t] = best;
}

}  // namespace xeng
