// Faraday rotation-measure synthesis of folded profiles (xengRmsynth*, rmsynth.hip): out of one folded dual-pol cube the Faraday
// spectrum of every beam pair over a grid of depths, the depth of its peak, and the band-summed I, Q, U, V profile de-rotated there.
//
// Contract (include/xeng.h, "Faraday rotation-measure synthesis of folded profiles"):
//   X      f32[npair][4][nchg][nbin], bin the fastest (xengFoldDump's cube at nprod = 4), never written
//   T      f32[nchg][nphi][2] = (Tc, Ts), w f32[nchg], gl i32[nused]: the channels with use != 0 in ascending order (formed on the
//          host when the table is set: a channel left out is never looked at), off / on u8[npair][nbin], active u8[npair],
//          cnt i32[npair][2] = (n_on, n_off), counted on the host when the masks are set
//   state  base f32[npair][4][nchg], part f32[npair][nrun][nphi] (nrun = ceil(nbin / 64)), spec f32[npair][nphi], kbest i32[npair]
//
// Base, grid ceil(npair nchg / 4): one wave per (p, g), lane j keeps the four chains of the bins b = j mod 64 in ascending b (a wave
// reads 256 consecutive bytes of each of the four rows per step); the 64 partials go through LDS and lanes 0..3 sum one word each
// in ascending j, then divide.
// Contract, grid (ceil(nphi / 64), ceil(nbin / 64), npair), 256 threads = 16 x 16, a thread owns 4 bins x 4 depths (32
// accumulators re, im).  Channels come in chunks of RM_GC = 8 through LDS, two buffers taken in turn, one barrier a chunk:
// threads 0..127 fetch 4 bins of one channel each (the words the feeds need, 16 bytes a word plane where nbin is a multiple of 4,
// else word by word) and store y_q, y_u with the baseline subtracted; threads 128..255 fetch 4 depths of (Tc, Ts) of one channel
// each (two 16-byte loads where nphi is even) and store them de-interleaved.  LDS per buffer: yq, yu, tc, ts, each [8][64] f32;
// a thread reads four 16-byte words per channel: the tc / ts words of the 16 threads of a ds_read_b128 lane group are 64
// consecutive dwords (all 64 banks once), the yq / yu words one or two addresses (broadcast).  The next chunk's global loads are
// issued before the current chunk's 64 x 8 fmaf and stored after them.  At the end pw = fmaf(im, im, fl(re re)) of the tile goes
// to LDS as [64 bins][64 depths] (the 16 KiB of the two buffers) and threads 0..63, one per depth, walk the bins in order over
// on != 0 and write one partial per (p, run, k).  The cube F[p][b][k] is never stored.  Words outside nbin or nphi are fetched
// as +0, computed and dropped.
// Pick, grid npair: thread k mod 256 sums the runs of depth k in order and writes spec; an ordered arg-max (a thread keeps the first
// strictly greater word of its ascending walk; the work-group reduces by larger value, then smaller k), the record, kbest.
// Profile, grid (ceil(nbin / 256), npair): thread = bin; it walks the used channels, RM_PU = 16 fetched together, with T[g][kbest]
// and w[g] the same in every thread, and keeps the four chains.  Its re, im are the contraction's operations in the contraction's order.
//
// No float atomics, no packed fp32, no MFMA (its summation order is not a stated one); no work-group waits for another; size_t
// index arithmetic; nothing contracted (fp contract(off); every fmaf is written).  Division is correctly rounded in hipcc's default
// build.  rmsynth.hip is compiled with -fno-slp-vectorize (Makefile), with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

#pragma clang fp contract(off)

constexpr int RM_THREADS = 256;
constexpr int RM_TILE = 64;                     // bins and depths of a contraction tile; the bins of a run
constexpr int RM_GC = 8;                        // channels of a chunk
constexpr int RM_PU = 16;                       // channels the profile kernel fetches together
constexpr int RM_BUF = 4 * RM_GC * RM_TILE;     // floats of one LDS buffer: yq, yu, tc, ts
constexpr size_t RM_BASE_LDS_BYTES = 4 * 4 * 64 * sizeof(float);
constexpr size_t RM_CONTRACT_LDS_BYTES = 2 * RM_BUF * sizeof(float);     // = 64 x 64 floats: the pw tile takes their place
constexpr size_t RM_PICK_LDS_BYTES = 2 * RM_THREADS * sizeof(float);
static_assert(2 * RM_BUF == RM_TILE * RM_TILE, "the pw tile lies in the two chunk buffers");

struct RmRecord {
    int k;
    float peak;
    int n_on, n_off;
};

// one rounding each: this file's operators are not contracted (the pragma above)
__device__ __forceinline__ float rm_add(float a, float b) { return a + b; }
__device__ __forceinline__ float rm_sub(float a, float b) { return a - b; }

// The Stokes words of one (pair, channel, bin): feeds 0 (linear) i = XX + YY, q = XX - YY, u = 2 Re, v = 2 Im; feeds 1 (circular)
// i = XX + YY, q = 2 Re, u = 2 Im, v = XX - YY
__device__ __forceinline__ float rm_q(float x0, float x1, float x2, int feeds) { return feeds ? rm_add(x2, x2) : rm_sub(x0, x1); }
__device__ __forceinline__ float rm_u(float x2, float x3, int feeds) { return feeds ? rm_add(x3, x3) : rm_add(x2, x2); }
__device__ __forceinline__ float rm_v(float x0, float x1, float x3, int feeds) { return feeds ? rm_sub(x0, x1) : rm_add(x3, x3); }

// grid ceil(npair nchg / 4), 256 threads, RM_BASE_LDS_BYTES of dynamic LDS
__global__ __launch_bounds__(256) void rmsynth_base_kernel(const float* __restrict__ X, const unsigned char* __restrict__ off, const unsigned char* __restrict__ use,
                                                           const unsigned char* __restrict__ active, const int* __restrict__ cnt, float* __restrict__ base, int npair,
                                                           int nchg, int nbin, int feeds) {
    extern __shared__ float rm_lds[];
    const int tid = threadIdx.x, wv = tid >> 6, j = tid & 63;
    const long long pg = (long long)blockIdx.x * 4 + wv;
    const bool live = pg < (long long)npair * nchg;
    const int p = live ? (int)(pg / nchg) : 0, g = live ? (int)(pg % nchg) : 0;
    const bool reads = live && active[p] != 0 && use[g] != 0;       // (the same in every lane of the wave)
    float ai = 0.f, aq = 0.f, au = 0.f, av = 0.f;
    if (reads) {
        const size_t plane = (size_t)nchg * nbin;
        const float* x = X + ((size_t)p * 4 * nchg + g) * nbin;
        const unsigned char* o = off + (size_t)p * nbin;
        for (int b = j; b < nbin; b += 64) {
            if (o[b] == 0) continue;
            const float x0 = x[b], x1 = x[plane + b], x2 = x[2 * plane + b], x3 = x[3 * plane + b];
            ai = rm_add(ai, rm_add(x0, x1));
            aq = rm_add(aq, rm_q(x0, x1, x2, feeds));
            au = rm_add(au, rm_u(x2, x3, feeds));
            av = rm_add(av, rm_v(x0, x1, x3, feeds));
        }
    }
    float* l = rm_lds + wv * 256;                                   // [4 words][64 lanes] of this wave
    l[j] = ai;
    l[64 + j] = aq;
    l[128 + j] = au;
    l[192 + j] = av;
    __syncthreads();
    if (live && j < 4) {                                            // lane s sums word s in ascending j
        float t = 0.f;
        const int n = reads ? cnt[2 * p + 1] : 0;
        if (n > 0) {
            for (int jj = 0; jj < 64; jj++) t = rm_add(t, l[j * 64 + jj]);
            t = t / (float)n;
        }
        base[((size_t)p * 4 + j) * nchg + g] = t;
    }
}

struct RmFetch {
    float4 a, b, c;
    float bq, bu;
};

// grid (ceil(nphi / 64), ceil(nbin / 64), npair), 256 threads, RM_CONTRACT_LDS_BYTES of dynamic LDS; after the base kernel on the
// same stream
__global__ __launch_bounds__(256) void rmsynth_contract_kernel(const float* __restrict__ X, const float* __restrict__ T, const int* __restrict__ gl,
                                                               const float* __restrict__ base, const unsigned char* __restrict__ on,
                                                               const unsigned char* __restrict__ active, float* __restrict__ part, int nused, int nchg, int nbin,
                                                               int nphi, int feeds) {
    extern __shared__ float rm_lds[];
    const int tid = threadIdx.x, p = blockIdx.z, b0 = blockIdx.y * RM_TILE, k0 = blockIdx.x * RM_TILE;
    if (active[p] == 0) return;                                     // (the same in every thread)
    const int tx = tid & 15, ty = tid >> 4;                         // depths k0 + 4 tx .., bins b0 + 4 ty ..
    const bool isT = tid >= 128;                                    // (whole waves: 0, 1 fetch the cube, 2, 3 the table)
    const int lg = (tid & 127) >> 4, l4 = (tid & 15) * 4;           // the channel of the chunk and the first of 4 bins / depths
    const bool vecX = (nbin & 3) == 0, vecT = (nphi & 1) == 0;
    const size_t plane = (size_t)nchg * nbin;
    const float* Xp = X + (size_t)p * 4 * plane;
    const float* basep = base + (size_t)p * 4 * nchg;
    const int nchunk = (nused + RM_GC - 1) / RM_GC;

    auto fetch = [&](int c, RmFetch& f) -> bool {
        const int i = c * RM_GC + lg;
        if (i >= nused) return false;
        const int g = gl[i];
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        f.a = z;
        f.b = z;
        f.c = z;
        if (!isT) {
            const int b = b0 + l4;
            const float* r0 = Xp + (feeds ? 2 : 0) * plane + (size_t)g * nbin;      // linear: XX, YY, Re; circular: Re, Im
            const float* r1 = Xp + (feeds ? 3 : 1) * plane + (size_t)g * nbin;
            const float* r2 = Xp + 2 * plane + (size_t)g * nbin;
            if (vecX && b < nbin) {                                 // (b and nbin are multiples of 4: b + 3 < nbin)
                f.a = *(const float4*)(r0 + b);
                f.b = *(const float4*)(r1 + b);
                if (!feeds) f.c = *(const float4*)(r2 + b);
            } else {
                if (b < nbin) { f.a.x = r0[b]; f.b.x = r1[b]; if (!feeds) f.c.x = r2[b]; }
                if (b + 1 < nbin) { f.a.y = r0[b + 1]; f.b.y = r1[b + 1]; if (!feeds) f.c.y = r2[b + 1]; }
                if (b + 2 < nbin) { f.a.z = r0[b + 2]; f.b.z = r1[b + 2]; if (!feeds) f.c.z = r2[b + 2]; }
                if (b + 3 < nbin) { f.a.w = r0[b + 3]; f.b.w = r1[b + 3]; if (!feeds) f.c.w = r2[b + 3]; }
            }
            f.bq = basep[(size_t)nchg + g];
            f.bu = basep[(size_t)2 * nchg + g];
        } else {
            const int k = k0 + l4;
            const float* r = T + ((size_t)g * nphi + k) * 2;
            if (vecT && k + 3 < nphi) {                             // (k is a multiple of 4 and nphi even: 16-byte aligned)
                f.a = *(const float4*)r;
                f.b = *(const float4*)(r + 4);
            } else {
                if (k < nphi) { f.a.x = r[0]; f.a.y = r[1]; }
                if (k + 1 < nphi) { f.a.z = r[2]; f.a.w = r[3]; }
                if (k + 2 < nphi) { f.b.x = r[4]; f.b.y = r[5]; }
                if (k + 3 < nphi) { f.b.z = r[6]; f.b.w = r[7]; }
            }
        }
        return true;
    };
    auto stash = [&](const RmFetch& f, float* buf) {
        float4 s0, s1;
        if (!isT) {
            s0.x = rm_sub(rm_q(f.a.x, f.b.x, f.a.x, feeds), f.bq);    // (circular: a is Re, b is Im; linear: a XX, b YY, c Re)
            s0.y = rm_sub(rm_q(f.a.y, f.b.y, f.a.y, feeds), f.bq);
            s0.z = rm_sub(rm_q(f.a.z, f.b.z, f.a.z, feeds), f.bq);
            s0.w = rm_sub(rm_q(f.a.w, f.b.w, f.a.w, feeds), f.bq);
            s1.x = rm_sub(rm_u(f.c.x, f.b.x, feeds), f.bu);
            s1.y = rm_sub(rm_u(f.c.y, f.b.y, feeds), f.bu);
            s1.z = rm_sub(rm_u(f.c.z, f.b.z, feeds), f.bu);
            s1.w = rm_sub(rm_u(f.c.w, f.b.w, feeds), f.bu);
            *(float4*)(buf + lg * RM_TILE + l4) = s0;                                   // yq
            *(float4*)(buf + RM_GC * RM_TILE + lg * RM_TILE + l4) = s1;                 // yu
        } else {
            s0 = make_float4(f.a.x, f.a.z, f.b.x, f.b.z);
            s1 = make_float4(f.a.y, f.a.w, f.b.y, f.b.w);
            *(float4*)(buf + 2 * RM_GC * RM_TILE + lg * RM_TILE + l4) = s0;             // tc
            *(float4*)(buf + 3 * RM_GC * RM_TILE + lg * RM_TILE + l4) = s1;             // ts
        }
    };

    float re[4][4], im[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) re[i][j] = im[i][j] = 0.f;
    RmFetch f;
    if (nchunk > 0) {
        if (fetch(0, f)) stash(f, rm_lds);
        __syncthreads();
    }
    for (int c = 0; c < nchunk; c++) {
        const bool more = c + 1 < nchunk && fetch(c + 1, f);        // (global loads in flight over the chunk's arithmetic)
        const float* buf = rm_lds + (c & 1) * RM_BUF;
        const int n = nused - c * RM_GC < RM_GC ? nused - c * RM_GC : RM_GC;
        for (int gg = 0; gg < n; gg++) {
            const float4 q4 = *(const float4*)(buf + gg * RM_TILE + ty * 4);
            const float4 u4 = *(const float4*)(buf + RM_GC * RM_TILE + gg * RM_TILE + ty * 4);
            const float4 c4 = *(const float4*)(buf + 2 * RM_GC * RM_TILE + gg * RM_TILE + tx * 4);
            const float4 s4 = *(const float4*)(buf + 3 * RM_GC * RM_TILE + gg * RM_TILE + tx * 4);
            const float yq[4] = {q4.x, q4.y, q4.z, q4.w}, yu[4] = {u4.x, u4.y, u4.z, u4.w};
            const float tc[4] = {c4.x, c4.y, c4.z, c4.w}, ts[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    re[i][j] = fmaf(yq[i], tc[j], re[i][j]);
                    re[i][j] = fmaf(yu[i], ts[j], re[i][j]);
                    im[i][j] = fmaf(yu[i], tc[j], im[i][j]);
                    im[i][j] = fmaf(-yq[i], ts[j], im[i][j]);
                }
        }
        if (more) stash(f, rm_lds + ((c + 1) & 1) * RM_BUF);        // (the buffer of chunk c - 1: its readers passed that chunk's barrier)
        __syncthreads();
    }
    // the tile of pw, [bin][depth]; every thread has passed the last chunk's barrier
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float4 pw;
        pw.x = fmaf(im[i][0], im[i][0], re[i][0] * re[i][0]);
        pw.y = fmaf(im[i][1], im[i][1], re[i][1] * re[i][1]);
        pw.z = fmaf(im[i][2], im[i][2], re[i][2] * re[i][2]);
        pw.w = fmaf(im[i][3], im[i][3], re[i][3] * re[i][3]);
        *(float4*)(rm_lds + (ty * 4 + i) * RM_TILE + tx * 4) = pw;
    }
    __syncthreads();
    if (tid < RM_TILE && k0 + tid < nphi) {
        const unsigned char* o = on + (size_t)p * nbin + b0;
        const int nb = nbin - b0 < RM_TILE ? nbin - b0 : RM_TILE;
        float a = 0.f;
        for (int b = 0; b < nb; b++)
            if (o[b] != 0) a = rm_add(a, rm_lds[b * RM_TILE + tid]);
        part[((size_t)p * gridDim.y + blockIdx.y) * nphi + k0 + tid] = a;
    }
}

// grid npair, 256 threads, RM_PICK_LDS_BYTES of dynamic LDS; after the contraction on the same stream
__global__ __launch_bounds__(256) void rmsynth_pick_kernel(const float* __restrict__ part, const unsigned char* __restrict__ active, const int* __restrict__ cnt,
                                                           float* __restrict__ spec, int* __restrict__ kbest, RmRecord* __restrict__ rec,
                                                           float* __restrict__ spec_out, int nrun, int nphi) {
    extern __shared__ float rm_lds[];
    float* rc = rm_lds;                             // [256]
    int* rk = (int*)(rm_lds + RM_THREADS);          // [256]
    const int tid = threadIdx.x, p = blockIdx.x;
    const bool act = active[p] != 0;
    const int n_on = act ? cnt[2 * p] : 0, n_off = act ? cnt[2 * p + 1] : 0;
    float bc = 0.f;
    int bk = -1;
    for (int k = tid; k < nphi; k += RM_THREADS) {
        float s = 0.f;
        if (act)
            for (int r = 0; r < nrun; r++) s = rm_add(s, part[((size_t)p * nrun + r) * nphi + k]);
        spec[(size_t)p * nphi + k] = s;
        spec_out[(size_t)p * nphi + k] = s;
        if (s == s && (bk < 0 || s > bc)) {
            bc = s;
            bk = k;
        }
    }
    rc[tid] = bc;
    rk[tid] = bk;
    __syncthreads();
    for (int h = RM_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h && rk[tid + h] >= 0 && (rk[tid] < 0 || rc[tid + h] > rc[tid] || (rc[tid + h] == rc[tid] && rk[tid + h] < rk[tid]))) {
            rc[tid] = rc[tid + h];
            rk[tid] = rk[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        RmRecord o = {-1, 0.f, n_on, n_off};
        if (act && n_on > 0 && rk[0] >= 0) {
            o.k = rk[0];
            o.peak = rc[0];
        }
        kbest[p] = o.k;
        rec[p] = o;
    }
}

// grid (ceil(nbin / 256), npair), 256 threads, no LDS; after the pick on the same stream
__global__ __launch_bounds__(256) void rmsynth_profile_kernel(const float* __restrict__ X, const float* __restrict__ T, const float* __restrict__ w,
                                                              const int* __restrict__ gl, const float* __restrict__ base, const unsigned char* __restrict__ active,
                                                              const int* __restrict__ kbest, float* __restrict__ prof, int nused, int nchg, int nbin, int nphi,
                                                              int feeds) {
    const int p = blockIdx.y, b = blockIdx.x * RM_THREADS + threadIdx.x;
    if (b >= nbin) return;
    float* o = prof + (size_t)p * 4 * nbin + b;
    float si = 0.f, sv = 0.f, re = 0.f, im = 0.f;
    if (active[p] != 0) {                                           // (the same in every thread)
        const int k = kbest[p];
        const size_t plane = (size_t)nchg * nbin;
        const float* x = X + (size_t)p * 4 * plane + b;
        const float* basep = base + (size_t)p * 4 * nchg;
        // RM_PU channels at a time: their 4 RM_PU loads are issued together, then the chains take them in order (one load a step
        // would leave every step waiting a memory latency: the chains are sequential and there are only npair nbin threads)
        for (int i0 = 0; i0 < nused; i0 += RM_PU) {
            float x0[RM_PU], x1[RM_PU], x2[RM_PU], x3[RM_PU];
            int gs[RM_PU];
#pragma unroll
            for (int u = 0; u < RM_PU; u++) {
                gs[u] = gl[i0 + u < nused ? i0 + u : nused - 1];     // (past the list: the last channel again, fetched and dropped)
                const size_t at = (size_t)gs[u] * nbin;
                x0[u] = x[at];
                x1[u] = x[plane + at];
                x2[u] = x[2 * plane + at];
                x3[u] = x[3 * plane + at];
            }
#pragma unroll
            for (int u = 0; u < RM_PU; u++) {
                if (i0 + u >= nused) break;
                const int g = gs[u];
                const float wg = w[g];
                si = fmaf(wg, rm_sub(rm_add(x0[u], x1[u]), basep[g]), si);
                sv = fmaf(wg, rm_sub(rm_v(x0[u], x1[u], x3[u], feeds), basep[(size_t)3 * nchg + g]), sv);
                if (k >= 0) {
                    const float yq = rm_sub(rm_q(x0[u], x1[u], x2[u], feeds), basep[(size_t)nchg + g]);
                    const float yu = rm_sub(rm_u(x2[u], x3[u], feeds), basep[(size_t)2 * nchg + g]);
                    const float tc = T[((size_t)g * nphi + k) * 2], ts = T[((size_t)g * nphi + k) * 2 + 1];
                    re = fmaf(yq, tc, re);
                    re = fmaf(yu, ts, re);
                    im = fmaf(yu, tc, im);
                    im = fmaf(-yq, ts, im);
                }
            }
        }
    }
    o[0] = si;
    o[(size_t)nbin] = re;
    o[(size_t)2 * nbin] = im;
    o[(size_t)3 * nbin] = sv;
}

}  // namespace xeng
