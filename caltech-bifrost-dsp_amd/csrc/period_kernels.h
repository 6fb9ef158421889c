// FFT periodicity search of the dedispersed beams (xengPeriod*, period.hip): per series a segment of NT windows is transformed,
// whitened and stacked into A; when a stack is complete the harmonic sums of A give one peak record per series and level.
//
// Contract (include/xeng.h, "FFT periodicity search of the dedispersed beams"); a series is one (pair, trial), nser = npair*ndm,
// N = NT/2:
//   in     f32[nc][nser][NPROD], z = word 0 (NPROD = 1) or word 0 + word 1 (NPROD = 4)
//   tbuf   f32[nser][NT], window n of a series at slot n mod NT
//   A      f32[nser][N], the stack
//   keep   u8[N] (0 = zapped) and cnt f32[N/B], the bins of each whitening block that count (k >= 1, kept): both from the host
//   tw     float2[N], tw[k] = exp(-2 pi i k / NT), and twu float2[N/2], twu[t] = tw[bitrev(2t)]: float64 on the host, rounded once
//   out    {f32 H, i32 k}[nser][nlevel], one 8-byte store each
//
// Ingest, every call: a work-group moves a tile of 32 series x 32 windows through LDS (rows padded by one word): loads consecutive
// across lanes along the series, 4-byte stores consecutive across lanes along time; I is formed here.
//
// Spectrum, once per completed segment, one work-group of 256 threads per series, float2[N] of dynamic LDS and nothing else:
//   1. coalesced load of the series as N complex points c[m] = (z[2m], z[2m+1]); the mean: per thread, per wave by shuffles, the
//      four waves through four LDS words borrowed from the buffer (read out, used as a mailbox, put back), then subtracted.
//   2. the N-point complex FFT in place, decimation in frequency, natural order in and bit-reversed order out.  Two radix-2
//      stages are fused in registers (a thread takes the points a, a+h/2, a+h, a+3h/2 and does the butterflies of half-sizes h and
//      h/2: one LDS pass and one barrier for two stages, the arithmetic of plain radix 2); where log2 N is odd a last radix-2
//      stage (twiddle 1) follows.  Twiddles come from tw: W_2h^p = tw[p*N/h], W_h^p = tw[2p*N/h], and W_2h^(p+h/2) = -i W_2h^p.
//   3. the real-input untangle in the bit-reversed domain: thread t owns the element at 2t (bin k = bitrev(2t) < N/2) and the one
//      holding bin N-k, forms |E +- W^k O|^2 with W^k = twu[t] and writes both powers over the .x words of the two elements.
//   4. bit-reversed to natural: P[k] from the .x word of element bitrev(k) into the .y word of element k.
//   5. block sums by a pairwise tree over the .x words (level 1 applies k >= 1 and keep), mu_b = sum / cnt[b].
//   6. S, then A = S (the stack's first segment) or A + S, coalesced; on the stack's last segment A also replaces P in the .y words.
//   7. on the last segment the harmonic sums by gathers from those words, (H, k) reduced per wave by shuffles and over the four
//      waves by thread 0, which stores the nlevel records.
// LDS banks: element i lives at pr_sw(i), an XOR swizzle of the low five bits.  In a fused stage with hh = h/2 >= 32 the lanes of a
// 32-lane group read 32 consecutive elements: every bank once.  With hh < 32 the group's elements are runs of hh with a stride of
// 4 hh, which unswizzled fall on 32 / 4 = 8 element slots mod 32 (4-way); bits 5 and 6 of the index, the only ones the five lane
// bits reach beyond bit 4, are folded back by the masks 10101b and 11111b, whose projections on the bit pairs {j, j+1} are
// independent for every j, so that for each hh the map lane -> slot mod 32 is a bijection: no conflict in ds_read_b64 (two
// 32-lane groups, 64 banks).  ds_write_b64 works in 16-lane groups on 32 banks and stays at most 2-way.  For log2 N >= 12 the top
// five bits, reversed, are folded in as well, so that step 4, whose lanes differ in exactly those bits, reads 32 different slots
// instead of one (32-way); below that the top bits overlap bits 5 and 6 and step 4 is left conflicted (sizes for tests).
//
// Everything up to A is held to a tolerance and contracts freely; the harmonic sums are plain fp32 adds in ascending j, with
// contraction off.  No atomics; every word has one owner; the result is a fixed function of the series and the mask.
//
// period.hip is compiled with -fno-slp-vectorize (Makefile): complex fp32 arithmetic, as upchan_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int PR_THREADS = 256;
constexpr int PR_TILE = 32;         // ingest tile: series x windows
constexpr int PR_MAX_LEVEL = 5;

struct PeriodRecord {
    float H;
    int k;
};

// grid (ceil(nser / 32), ceil(nc / 32)), 256 threads; slot0 = slot of the call's first window, slot0 + nc <= NT
template <int NPROD>
__global__ __launch_bounds__(256) void period_ingest_kernel(const float* __restrict__ in, float* __restrict__ tbuf, int nser, int NT, int slot0,
                                                            int nc) {
    __shared__ float tile[PR_TILE][PR_TILE + 1];
    const int s0 = blockIdx.x * PR_TILE, t0 = blockIdx.y * PR_TILE;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    for (int i = 0; i < PR_TILE / 8; i++) {
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
    for (int i = 0; i < PR_TILE / 8; i++) {
        const int ss = hi + 8 * i, s = s0 + ss;
        if (s >= nser) break;
        tbuf[(size_t)s * NT + slot0 + t] = tile[ss][lo];
    }
}

// where element i of the work-group's float2[N] lives (see "LDS banks" above); a bijection of every aligned block of 32
__device__ __forceinline__ int pr_sw(int i, int L) {
    int p = i ^ ((i & 32) ? 21 : 0) ^ ((i & 64) ? 31 : 0);
    if (L >= 12) p ^= (int)(__brev((unsigned)i >> (L - 5)) >> 27);
    return p;
}

__device__ __forceinline__ float2 pr_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// larger H, then smaller k; a NaN never enters
__device__ __forceinline__ void pr_take(PeriodRecord& b, float H, int k) {
    if (H != H) return;
    if (b.k < 0 || H > b.H || (H == b.H && k < b.k)) {
        b.H = H;
        b.k = k;
    }
}

// grid nser, 256 threads, N * 8 bytes of dynamic LDS.  L = log2 N, lb = log2 B.  first: the segment opens its stack (A is stored,
// not added to); last: it completes it (records are written to out, which is not touched otherwise).
__global__ __launch_bounds__(256) void period_spectrum_kernel(const float* __restrict__ tbuf, float* __restrict__ A, const unsigned char* __restrict__ keep,
                                                              const float* __restrict__ cnt, const float2* __restrict__ tw,
                                                              const float2* __restrict__ twu, PeriodRecord* __restrict__ out, int L, int lb, int nlevel,
                                                              int kmin, int first, int last) {
    extern __shared__ float2 pr_lds[];
    float* const ldsf = (float*)pr_lds;
    const int N = 1 << L, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ser = blockIdx.x;
    const float2* src = (const float2*)(tbuf + ser * 2 * N);

    // 1. load, mean
    float part = 0.f;
    for (int m = tid; m < N; m += PR_THREADS) {
        const float2 c = src[m];
        pr_lds[pr_sw(m, L)] = c;
        part += c.x + c.y;
    }
    for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
    __syncthreads();
    float borrowed = 0.f;
    if (lane == 0) borrowed = ldsf[wave];
    __syncthreads();
    if (lane == 0) ldsf[wave] = part;
    __syncthreads();
    const float mean = (((ldsf[0] + ldsf[1]) + ldsf[2]) + ldsf[3]) * (0.5f / (float)N);
    __syncthreads();
    if (lane == 0) ldsf[wave] = borrowed;
    __syncthreads();
    for (int m = tid; m < N; m += PR_THREADS) {     // (its own elements: no barrier between the load and this)
        float2 c = pr_lds[pr_sw(m, L)];
        c.x -= mean;
        c.y -= mean;
        pr_lds[pr_sw(m, L)] = c;
    }
    __syncthreads();

    // 2. FFT, decimation in frequency
    int lh = L - 1;                                 // log2 of the half-size h
    for (; lh >= 1; lh -= 2) {
        const int lq = lh - 1, hh = 1 << lq;        // hh = h / 2
        for (int q = tid; q < N / 4; q += PR_THREADS) {
            const int p = q & (hh - 1), a = ((q >> lq) << (lq + 2)) | p;
            const int i0 = pr_sw(a, L), i1 = pr_sw(a + hh, L), i2 = pr_sw(a + 2 * hh, L), i3 = pr_sw(a + 3 * hh, L);
            const float2 x0 = pr_lds[i0], x1 = pr_lds[i1], x2 = pr_lds[i2], x3 = pr_lds[i3];
            const float2 w1 = tw[(size_t)p << (L - lh)], w2 = tw[(size_t)p << (L - lh + 1)];
            // half-size h: (a, a+h) with W_2h^p, (a+h/2, a+3h/2) with W_2h^(p+h/2) = -i W_2h^p
            const float2 u0 = make_float2(x0.x + x2.x, x0.y + x2.y), d0 = make_float2(x0.x - x2.x, x0.y - x2.y);
            const float2 u1 = make_float2(x1.x + x3.x, x1.y + x3.y), d1 = make_float2(x1.x - x3.x, x1.y - x3.y);
            const float2 v0 = pr_cmul(d0, w1), v1 = pr_cmul(d1, make_float2(w1.y, -w1.x));
            // half-size h/2: (a, a+h/2) and (a+h, a+3h/2), both with W_h^p
            pr_lds[i0] = make_float2(u0.x + u1.x, u0.y + u1.y);
            pr_lds[i1] = pr_cmul(make_float2(u0.x - u1.x, u0.y - u1.y), w2);
            pr_lds[i2] = make_float2(v0.x + v1.x, v0.y + v1.y);
            pr_lds[i3] = pr_cmul(make_float2(v0.x - v1.x, v0.y - v1.y), w2);
        }
        __syncthreads();
    }
    if (lh == 0) {                                  // log2 N odd: the last stage, half-size 1, twiddle 1
        for (int q = tid; q < N / 2; q += PR_THREADS) {
            const int i0 = pr_sw(2 * q, L), i1 = pr_sw(2 * q + 1, L);
            const float2 x0 = pr_lds[i0], x1 = pr_lds[i1];
            pr_lds[i0] = make_float2(x0.x + x1.x, x0.y + x1.y);
            pr_lds[i1] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        __syncthreads();
    }

    // 3. untangle: Z[k] at element bitrev(k).  X[k] = E + W^k O, X[N-k] = conj(E - W^k O), E = (Z[k] + conj Z[N-k]) / 2,
    //    O = (Z[k] - conj Z[N-k]) / 2i
    for (int t = tid; t < N / 2; t += PR_THREADS) {
        const int j = 2 * t, k = (int)(__brev((unsigned)j) >> (32 - L));
        const int jp = (int)(__brev((unsigned)((N - k) & (N - 1))) >> (32 - L));
        const int ia = pr_sw(j, L), ib = pr_sw(jp, L);
        const float2 za = pr_lds[ia], zb = pr_lds[ib], w = twu[t];
        const float2 E = make_float2(0.5f * (za.x + zb.x), 0.5f * (za.y - zb.y));
        const float2 O = make_float2(0.5f * (za.y + zb.y), -0.5f * (za.x - zb.x));
        const float2 wo = pr_cmul(O, w);
        const float2 xa = make_float2(E.x + wo.x, E.y + wo.y), xb = make_float2(E.x - wo.x, E.y - wo.y);
        ldsf[2 * ib] = xb.x * xb.x + xb.y * xb.y;   // (k = 0: both are element 0, whose power is never read)
        ldsf[2 * ia] = xa.x * xa.x + xa.y * xa.y;
        if (t == 0) {                               // bin N/2, its own partner, at element 1: X = conj Z
            const int ic = pr_sw(1, L);
            const float2 zc = pr_lds[ic];
            ldsf[2 * ic] = zc.x * zc.x + zc.y * zc.y;
        }
    }
    __syncthreads();

    // 4. P[k] into the .y word of element k
    for (int k = tid; k < N; k += PR_THREADS) ldsf[2 * pr_sw(k, L) + 1] = ldsf[2 * pr_sw((int)(__brev((unsigned)k) >> (32 - L)), L)];
    __syncthreads();

    // 5. block sums: a pairwise tree over the .x words, level by level behind one another
    for (int i = tid; i < N / 2; i += PR_THREADS) {
        const int k0 = 2 * i, k1 = 2 * i + 1;
        const float a = (k0 >= 1 && keep[k0]) ? ldsf[2 * pr_sw(k0, L) + 1] : 0.f;
        const float b = keep[k1] ? ldsf[2 * pr_sw(k1, L) + 1] : 0.f;
        ldsf[2 * pr_sw(i, L)] = a + b;
    }
    int off = 0, n = N / 2;
    for (int l = 1; l < lb; l++) {
        __syncthreads();
        const int dst = off + n;
        for (int i = tid; i < n / 2; i += PR_THREADS)
            ldsf[2 * pr_sw(dst + i, L)] = ldsf[2 * pr_sw(off + 2 * i, L)] + ldsf[2 * pr_sw(off + 2 * i + 1, L)];
        off = dst;
        n >>= 1;
    }
    __syncthreads();                                // block b's sum is the .x word of element off + b

    // 6. S and A
    const bool whole = (__float_as_uint(mean) & 0x7f800000u) != 0x7f800000u;    // a finite mean: otherwise the series is NaN from here on
    float* Arow = A + ser * N;
    for (int k = tid; k < N; k += PR_THREADS) {
        const int b = k >> lb, ik = 2 * pr_sw(k, L) + 1;
        const float c = cnt[b], mu = ldsf[2 * pr_sw(off + b, L)] / c;
        float S = 1.0f;
        if (c > 0.f && mu > 0.f && mu < __int_as_float(0x7f800000) && keep[k]) S = ldsf[ik] / mu;
        if (!whole) S = __int_as_float(0x7fc00000);
        if (k == 0) S = 0.f;
        const float a = first ? S : Arow[k] + S;
        Arow[k] = a;
        ldsf[ik] = a;
    }
    if (!last) return;
    __syncthreads();

    // 7. harmonic sums and records
    {
#pragma clang fp contract(off)
        PeriodRecord mine[PR_MAX_LEVEL];
#pragma unroll
        for (int l = 0; l < PR_MAX_LEVEL; l++) {
            PeriodRecord best = {0.f, -1};
            if (l < nlevel) {
                const int h = 1 << l;
                for (int k = (kmin << l) + tid; k < N; k += PR_THREADS) {
                    float H = ldsf[2 * pr_sw((k + (h >> 1)) >> l, L) + 1];
                    for (int j = 2; j <= h; j++) H = H + ldsf[2 * pr_sw((j * k + (h >> 1)) >> l, L) + 1];
                    pr_take(best, H, k);
                }
                for (int o = 32; o; o >>= 1) {
                    const float oH = __shfl_xor(best.H, o);
                    const int ok = __shfl_xor(best.k, o);
                    if (ok >= 0) pr_take(best, oH, ok);
                }
            }
            mine[l] = best;
        }
        // the waves meet in .x words (physical elements 0..55: the block sums there are dead, and the gathers read .y words only)
        float* const mail = ldsf;
        if (lane == 0) {
#pragma unroll
            for (int l = 0; l < PR_MAX_LEVEL; l++)
                if (l < nlevel) {
                    mail[2 * (l * 4 + wave)] = mine[l].H;
                    mail[2 * (l * 4 + wave + 32)] = __int_as_float(mine[l].k);
                }
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int l = 0; l < PR_MAX_LEVEL; l++)
                if (l < nlevel) {
                    PeriodRecord best = {0.f, -1};
                    for (int w = 0; w < 4; w++) {
                        const int wk = __float_as_int(mail[2 * (l * 4 + w + 32)]);
                        if (wk >= 0) pr_take(best, mail[2 * (l * 4 + w)], wk);
                    }
                    out[ser * nlevel + l] = best;
                }
        }
    }
}

}  // namespace xeng
