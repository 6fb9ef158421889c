// Template-matched arrival phases of folded profiles (xengToa*, toa.hip): out of one folded cube the sub-band profiles of every beam
// pair, their harmonics, and their correlation with a template on a grid of lags with the lag of its peak.
//
// Contract (include/xeng.h, "Template-matched arrival phases of folded profiles"):
//   X      f32[npair][nprod][nchg][nbin], bin the fastest (xengFoldDump's cube), nprod 1 or 4, never written
//   w      f32[nchg]; gl i32[nused]: the groups with w != 0 inside the sub-bands, ascending; gs i32[nsub + 1]: sub-band r's groups are
//          gl[gs[r]] .. gl[gs[r + 1] - 1] (both formed on the host when the bands are set: a group of weight 0 is never looked at)
//   D      f32[nbin][nharm][2], L f32[nharm][nlag][2], S f32[nrow][nharm][2] with nrow = npair (nsub + 1), row = p (nsub + 1) + r
//   off    u8[npair][nbin], active u8[npair], cnt i32[npair] = n_off, counted on the host when the mask is set
//   state  bv f32[nrow][2] = (base, var)
//   out    rec ToaRecord[nrow], P f32[nrow][nbin], PH f32[nrow][nharm][2], ccf f32[nrow][nlag]
//
// Scrunch, grid (ceil(nbin / 1024), nsub, npair): a thread owns 4 consecutive bins (one 16-byte load a group and plane where nbin is
// a multiple of 4, else word by word) and walks its sub-band's used groups in order, TOA_PU = 8 groups' loads issued together ahead of
// their steps of the chain; gl and w are the same in every thread of the work-group.  The cube's used rows are read exactly once.
// Band, grid (ceil(nbin / 256), npair): thread = bin, the rows r = 0 .. nsub - 1 of P added in order, TOA_PU fetched together.
// Base, grid ceil(nrow / 4): one wave per row, lane j keeps the chain of the off-pulse bins b = j mod 64 in ascending b; the 64
// partials go through LDS and every lane sums them in ascending j and divides (the mean); a second pass of the same shape over
// fl(d d), d = P - base.
// DFT, grid (ceil(nrow / 8), ceil(nharm / 256)): thread = harmonic, TOA_ROWS = 8 rows' (re, im) in registers; d = P - base of 256
// bins x 8 rows goes through LDS (read as two 16-byte broadcasts a bin), D[b][.] is 8 consecutive bytes a lane.
// Correlate, grid (ceil(nrow / 8), ceil(nlag / 256)): thread = lag, 8 rows' words in registers; the cross-spectrum of 256 harmonics x
// 8 rows is formed while it is staged in LDS (four 16-byte broadcasts a harmonic), L[k][.] is 8 consecutive bytes a lane.
// Pick, grid nrow: an ordered arg-max of the row's ccf (a thread keeps the first strictly greater word of its ascending walk; the
// work-group reduces by larger value, then smaller l) and the record.
// Words outside nbin, nharm, nlag or nrow are fetched as +0, computed and dropped, or guarded.
//
// No float atomics, no packed fp32, no MFMA; no transcendental function and no data-dependent iteration; no work-group waits for
// another; size_t index arithmetic; nothing contracted (fp contract(off); every fmaf is written).  Division is correctly rounded in
// hipcc's default build.  toa.hip is compiled with -fno-slp-vectorize (Makefile), with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

#pragma clang fp contract(off)

constexpr int TOA_THREADS = 256;
constexpr int TOA_PU = 8;                       // groups (scrunch) or rows (band) fetched together
constexpr int TOA_ROWS = 8;                     // rows of a DFT or correlation tile
constexpr int TOA_CHUNK = 256;                  // bins (DFT) or harmonics (correlation) staged in LDS at a time
constexpr size_t TOA_BASE_LDS_BYTES = 2 * 4 * 64 * sizeof(float);
constexpr size_t TOA_DFT_LDS_BYTES = (size_t)TOA_CHUNK * TOA_ROWS * sizeof(float);
constexpr size_t TOA_CORR_LDS_BYTES = (size_t)TOA_CHUNK * TOA_ROWS * 2 * sizeof(float);
constexpr size_t TOA_PICK_LDS_BYTES = 2 * TOA_THREADS * sizeof(float);

struct ToaRecord {
    int l;
    float peak, base, var;
};

// one rounding each: this file's operators are not contracted (the pragma above)
__device__ __forceinline__ float toa_add(float a, float b) { return a + b; }
__device__ __forceinline__ float toa_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float toa_mul(float a, float b) { return a * b; }

// four consecutive bins from q (bin b of a row of nbin): one 16-byte load, or the words inside the row, the rest +0
__device__ __forceinline__ float4 toa_load4(const float* q, int b, int nbin, bool vec) {
    if (vec) return *(const float4*)q;
    float4 v = make_float4(q[0], 0.f, 0.f, 0.f);
    if (b + 1 < nbin) v.y = q[1];
    if (b + 2 < nbin) v.z = q[2];
    if (b + 3 < nbin) v.w = q[3];
    return v;
}

// grid (ceil(nbin / (4 * 256)), nsub, npair), 256 threads, no LDS
template <int NPROD>
__global__ __launch_bounds__(256) void toa_scrunch_kernel(const float* __restrict__ X, const float* __restrict__ w, const int* __restrict__ gl,
                                                          const int* __restrict__ gs, const unsigned char* __restrict__ active, float* __restrict__ P, int nchg,
                                                          int nbin, int nsub) {
    const int p = blockIdx.z, r = blockIdx.y, b = (blockIdx.x * TOA_THREADS + threadIdx.x) * 4;
    if (b >= nbin) return;
    const bool vec = (nbin & 3) == 0;                               // (b and nbin multiples of 4: b + 3 < nbin, 16-byte aligned)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active[p] != 0) {                                           // (the same in every thread)
        const size_t plane = (size_t)nchg * nbin;
        const float* x = X + (size_t)p * NPROD * plane + b;
        const int i1 = gs[r + 1];
        for (int i0 = gs[r]; i0 < i1; i0 += TOA_PU) {
            float4 x0[TOA_PU], x1[TOA_PU];
            float wg[TOA_PU];
#pragma unroll
            for (int u = 0; u < TOA_PU; u++) {
                const int g = gl[i0 + u < i1 ? i0 + u : i1 - 1];    // (past the sub-band's list: its last group again, fetched and dropped)
                const size_t at = (size_t)g * nbin;
                wg[u] = w[g];
                x0[u] = toa_load4(x + at, b, nbin, vec);
                if (NPROD == 4) x1[u] = toa_load4(x + plane + at, b, nbin, vec);
            }
#pragma unroll
            for (int u = 0; u < TOA_PU; u++) {
                if (i0 + u >= i1) break;
                float4 v = x0[u];
                if (NPROD == 4) {
                    v.x = toa_add(v.x, x1[u].x);
                    v.y = toa_add(v.y, x1[u].y);
                    v.z = toa_add(v.z, x1[u].z);
                    v.w = toa_add(v.w, x1[u].w);
                }
                acc.x = fmaf(wg[u], v.x, acc.x);
                acc.y = fmaf(wg[u], v.y, acc.y);
                acc.z = fmaf(wg[u], v.z, acc.z);
                acc.w = fmaf(wg[u], v.w, acc.w);
            }
        }
    }
    float* o = P + ((size_t)p * (nsub + 1) + r) * nbin + b;
    if (vec) {
        *(float4*)o = acc;
    } else {
        o[0] = acc.x;
        if (b + 1 < nbin) o[1] = acc.y;
        if (b + 2 < nbin) o[2] = acc.z;
        if (b + 3 < nbin) o[3] = acc.w;
    }
}

// grid (ceil(nbin / 256), npair), 256 threads, no LDS; after the scrunch on the same stream.  P is read (rows < nsub) and written
// (row nsub) through the one pointer.
__global__ __launch_bounds__(256) void toa_band_kernel(const unsigned char* __restrict__ active, float* P, int nbin, int nsub) {
    const int p = blockIdx.y, b = blockIdx.x * TOA_THREADS + threadIdx.x;
    if (b >= nbin) return;
    float* rows = P + (size_t)p * (nsub + 1) * nbin + b;
    float s = 0.f;
    if (active[p] != 0) {                                           // (the same in every thread)
        for (int r0 = 0; r0 < nsub; r0 += TOA_PU) {
            float v[TOA_PU];
#pragma unroll
            for (int u = 0; u < TOA_PU; u++) v[u] = rows[(size_t)(r0 + u < nsub ? r0 + u : nsub - 1) * nbin];
#pragma unroll
            for (int u = 0; u < TOA_PU; u++) {
                if (r0 + u >= nsub) break;
                s = toa_add(s, v[u]);
            }
        }
    }
    rows[(size_t)nsub * nbin] = s;
}

// grid ceil(nrow / 4), 256 threads, TOA_BASE_LDS_BYTES of dynamic LDS; after the band kernel on the same stream
__global__ __launch_bounds__(256) void toa_base_kernel(const float* __restrict__ P, const unsigned char* __restrict__ off, const unsigned char* __restrict__ active,
                                                       const int* __restrict__ cnt, float* __restrict__ bv, int nrow, int nbin, int nsub) {
    extern __shared__ float toa_lds[];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const long long row = (long long)blockIdx.x * 4 + wv;
    const bool live = row < nrow;
    const int p = live ? (int)(row / (nsub + 1)) : 0;
    const int n = live && active[p] != 0 ? cnt[p] : 0;              // (the same in every lane of the wave)
    const float* x = P + (size_t)(live ? row : 0) * nbin;
    const unsigned char* o = off + (size_t)p * nbin;
    float* l1 = toa_lds + wv * 128;                                 // [2 sums][64 lanes] of this wave
    float* l2 = l1 + 64;
    float a = 0.f;
    if (n > 0)
        for (int b = j; b < nbin; b += 64)
            if (o[b] != 0) a = toa_add(a, x[b]);
    l1[j] = a;
    __syncthreads();
    float base = 0.f;
    if (n > 0) {                                                    // every lane sums the 64 partials in ascending j
        for (int jj = 0; jj < 64; jj++) base = toa_add(base, l1[jj]);
        base = base / (float)n;
    }
    a = 0.f;
    if (n > 0)
        for (int b = j; b < nbin; b += 64)
            if (o[b] != 0) {
                const float d = toa_sub(x[b], base);
                a = toa_add(a, toa_mul(d, d));
            }
    l2[j] = a;
    __syncthreads();
    if (live && j == 0) {
        float var = 0.f;
        if (n > 0) {
            for (int jj = 0; jj < 64; jj++) var = toa_add(var, l2[jj]);
            var = var / (float)n;
        }
        bv[2 * (size_t)row] = base;
        bv[2 * (size_t)row + 1] = var;
    }
}

// grid (ceil(nrow / 8), ceil(nharm / 256)), 256 threads, TOA_DFT_LDS_BYTES of dynamic LDS; after the base kernel on the same stream
__global__ __launch_bounds__(256) void toa_dft_kernel(const float* __restrict__ P, const float* __restrict__ bv, const float* __restrict__ D,
                                                      const unsigned char* __restrict__ active, float* __restrict__ PH, int nrow, int nbin, int nsub, int nharm) {
    extern __shared__ float toa_lds[];                              // d[256 bins][8 rows]
    const int tid = threadIdx.x, k = blockIdx.y * TOA_THREADS + tid;
    const size_t row0 = (size_t)blockIdx.x * TOA_ROWS;
    float re[TOA_ROWS], im[TOA_ROWS], bs[TOA_ROWS];
    bool rd[TOA_ROWS];
#pragma unroll
    for (int u = 0; u < TOA_ROWS; u++) {
        re[u] = im[u] = 0.f;
        rd[u] = row0 + u < (size_t)nrow && active[(row0 + u) / (nsub + 1)] != 0;
        bs[u] = rd[u] ? bv[2 * (row0 + u)] : 0.f;
    }
    const float2* D2 = (const float2*)D;
    for (int b0 = 0; b0 < nbin; b0 += TOA_CHUNK) {
        const int b = b0 + tid;
#pragma unroll
        for (int u = 0; u < TOA_ROWS; u++) toa_lds[tid * TOA_ROWS + u] = rd[u] && b < nbin ? toa_sub(P[(row0 + u) * nbin + b], bs[u]) : 0.f;
        __syncthreads();
        const int nb = nbin - b0 < TOA_CHUNK ? nbin - b0 : TOA_CHUNK;
        if (k < nharm) {
#pragma unroll 4
            for (int bb = 0; bb < nb; bb++) {
                const float2 t = D2[(size_t)(b0 + bb) * nharm + k];
                const float4 d0 = *(const float4*)(toa_lds + bb * TOA_ROWS), d1 = *(const float4*)(toa_lds + bb * TOA_ROWS + 4);
                const float d[TOA_ROWS] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
                for (int u = 0; u < TOA_ROWS; u++) {
                    re[u] = fmaf(d[u], t.x, re[u]);
                    im[u] = fmaf(d[u], t.y, im[u]);
                }
            }
        }
        __syncthreads();
    }
    if (k < nharm) {
#pragma unroll
        for (int u = 0; u < TOA_ROWS; u++)
            if (row0 + u < (size_t)nrow) ((float2*)PH)[(row0 + u) * nharm + k] = make_float2(re[u], im[u]);
    }
}

// grid (ceil(nrow / 8), ceil(nlag / 256)), 256 threads, TOA_CORR_LDS_BYTES of dynamic LDS; after the DFT on the same stream
__global__ __launch_bounds__(256) void toa_corr_kernel(const float* __restrict__ PH, const float* __restrict__ S, const float* __restrict__ L,
                                                       const unsigned char* __restrict__ active, float* __restrict__ ccf, int nrow, int nsub, int nharm, int nlag) {
    extern __shared__ float toa_lds[];                              // c[256 harmonics][8 rows][2] = (cr, ci)
    const int tid = threadIdx.x, l = blockIdx.y * TOA_THREADS + tid;
    const size_t row0 = (size_t)blockIdx.x * TOA_ROWS;
    float acc[TOA_ROWS];
    bool rd[TOA_ROWS];
#pragma unroll
    for (int u = 0; u < TOA_ROWS; u++) {
        acc[u] = 0.f;
        rd[u] = row0 + u < (size_t)nrow && active[(row0 + u) / (nsub + 1)] != 0;
    }
    const float2* L2 = (const float2*)L;
    const float2* PH2 = (const float2*)PH;
    const float2* S2 = (const float2*)S;
    for (int k0 = 0; k0 < nharm; k0 += TOA_CHUNK) {
        const int k = k0 + tid;
#pragma unroll
        for (int u = 0; u < TOA_ROWS; u++) {
            float cr = 0.f, ci = 0.f;
            if (rd[u] && k < nharm) {
                const float2 ph = PH2[(row0 + u) * nharm + k], s = S2[(row0 + u) * nharm + k];
                cr = fmaf(ph.x, s.x, toa_mul(ph.y, s.y));
                ci = fmaf(ph.y, s.x, -toa_mul(ph.x, s.y));
            }
            toa_lds[(tid * TOA_ROWS + u) * 2] = cr;
            toa_lds[(tid * TOA_ROWS + u) * 2 + 1] = ci;
        }
        __syncthreads();
        const int nk = nharm - k0 < TOA_CHUNK ? nharm - k0 : TOA_CHUNK;
        if (l < nlag) {
#pragma unroll 4
            for (int kk = 0; kk < nk; kk++) {
                const float2 t = L2[(size_t)(k0 + kk) * nlag + l];
                const float4* c4 = (const float4*)(toa_lds + kk * TOA_ROWS * 2);
                const float4 c0 = c4[0], c1 = c4[1], c2 = c4[2], c3 = c4[3];
                const float c[2 * TOA_ROWS] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w, c3.x, c3.y, c3.z, c3.w};
#pragma unroll
                for (int u = 0; u < TOA_ROWS; u++) {
                    acc[u] = fmaf(c[2 * u], t.x, acc[u]);
                    acc[u] = fmaf(c[2 * u + 1], t.y, acc[u]);
                }
            }
        }
        __syncthreads();
    }
    if (l < nlag) {
#pragma unroll
        for (int u = 0; u < TOA_ROWS; u++)
            if (row0 + u < (size_t)nrow) ccf[(row0 + u) * nlag + l] = acc[u];
    }
}

// grid nrow, 256 threads, TOA_PICK_LDS_BYTES of dynamic LDS; after the correlation on the same stream
__global__ __launch_bounds__(256) void toa_pick_kernel(const float* __restrict__ ccf, const float* __restrict__ bv, const int* __restrict__ gs,
                                                       const unsigned char* __restrict__ active, ToaRecord* __restrict__ rec, int nsub, int nlag) {
    extern __shared__ float toa_lds[];
    float* rc = toa_lds;                            // [256]
    int* rl = (int*)(toa_lds + TOA_THREADS);        // [256]
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const int p = (int)(row / (nsub + 1)), r = (int)(row % (nsub + 1));
    const bool act = active[p] != 0;
    const int nu = r < nsub ? gs[r + 1] - gs[r] : gs[nsub];         // the row's used groups
    float bc = 0.f;
    int bl = -1;
    for (int l = tid; l < nlag; l += TOA_THREADS) {
        const float s = ccf[row * nlag + l];
        if (s == s && (bl < 0 || s > bc)) {
            bc = s;
            bl = l;
        }
    }
    rc[tid] = bc;
    rl[tid] = bl;
    __syncthreads();
    for (int h = TOA_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h && rl[tid + h] >= 0 && (rl[tid] < 0 || rc[tid + h] > rc[tid] || (rc[tid + h] == rc[tid] && rl[tid + h] < rl[tid]))) {
            rc[tid] = rc[tid + h];
            rl[tid] = rl[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        ToaRecord o = {-1, 0.f, 0.f, 0.f};
        if (act) {
            o.base = bv[2 * row];
            o.var = bv[2 * row + 1];
            if (nu > 0 && rl[0] >= 0) {
                o.l = rl[0];
                o.peak = rc[0];
            }
        }
        rec[row] = o;
    }
}

}  // namespace xeng
