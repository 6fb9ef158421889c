// Dedispersed cut-outs and DM refinement of single pulses (xengCutout*, cutout.hip): out of a history of the channelised power
// beams, per request the waterfall of the centre trial, the DM-time plane over ndmc fine trials, and the best boxcar score over
// that plane.
//
// Contract (include/xeng.h, "Dedispersed cut-outs and DM refinement of single pulses"); Q = nfine/nband, ntu = nt tscr, c = ndmc/2:
//   ring   f32[npair][nfine][L], L = nhist + nwin: window n at slot n mod L (dedisp_kernels.h's history at nprod = 1; the ingest
//          IS dedisp_ingest_kernel<1>, launched from cutout.hip)
//   s      i32[ndmf][nfine] forward delays, w f32[nfine]
//   slots  the requests a call serves, by value in the kernel arguments (CutoutSlots): the host has validated pair and ic, and
//          formed slot0 = a(0) mod L (floored) and a0 = min(a(0), 2^30): only the sign of a0 + m + s counts
//   out    W f32[slot][nband][nt], P f32[slot][ndmc][nt], records of 32 bytes
//
// Partials, one launch for all served slots, grid (ceil(ntu / 256), ndmc, r): lane = column m of one (slot, row); for a given q a
// wave reads one contiguous run of a history row (slot0 + m + s < 2L: one conditional subtraction, never a word outside the
// row), and s[d][q] and w[q] are the same for the whole work-group.  The thread walks the bands in order, D in one register
// and B = B + D in another.  The time scrunch is an ordered sum through LDS: the work-group's 256 columns are 256 / tscr whole
// output columns (tscr divides 256, and ntu is a multiple of tscr: an output column is all live lanes or all idle ones), lane t
// of the first 256 / tscr sums words [t tscr, (t+1) tscr) in ascending order.  The centre row does that per band for W, with two
// LDS halves taken in turn (one barrier a band); every present row once for P at the end (a third piece of LDS).  Idle lanes
// (m >= ntu) read what lane ntu - 1 reads and their columns are not stored.  An absent row stores +0 and reads nothing.
//
// Row score, grid (ndmc, r): the row in LDS; median and MAD by the 32-pass key search of detrend_kernels.h (co_key, co_block_sum
// and co_median restate dt_key, dt_block_sum and dt_median: that header defines its kernels too and cannot be included twice in
// one library), then the boxcar tree between two LDS rows and an ordered arg-max: a thread keeps the first strictly
// greater score of its (iw ascending, j ascending) walk, the work-group reduces by (larger C, then smaller iw << 16 | j).
// Pick, grid nreq_max: the rows' records reduced by (larger C, then smaller i, then iw, j); slots past the served ones get the
// empty record.
//
// No float atomics (the one atomic is co_block_sum's integer count word in LDS); no work-group waits for another; size_t index
// arithmetic; nothing contracted (fp contract(off); the fmaf is written).  Division is correctly rounded in hipcc's default build.
//
// cutout.hip is compiled with -fno-slp-vectorize (Makefile), with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dedisp_kernels.h"

namespace xeng {

#pragma clang fp contract(off)

constexpr int CO_THREADS = 256;
constexpr int CO_MAX_REQ = 64;
constexpr int CO_MAX_WIDTH = 10;                // 2^(nwidth-1) <= nt/2 <= 512
constexpr unsigned CO_NONE = 0xFFFFFFFFu;       // a record without a score
constexpr size_t CO_PARTIALS_LDS_BYTES = 3 * CO_THREADS * sizeof(float);
inline size_t cutout_score_lds_bytes(int nt) { return ((size_t)3 * nt + 4 + 2 * CO_THREADS) * sizeof(float); }
constexpr size_t CO_PICK_LDS_BYTES = 3 * CO_THREADS * sizeof(float);

struct CutoutSlots {
    int id[CO_MAX_REQ], pair[CO_MAX_REQ], ic[CO_MAX_REQ], dstep[CO_MAX_REQ];
    int slot0[CO_MAX_REQ];                      // a(0) mod L, floored
    int a0[CO_MAX_REQ];                         // min(a(0), 2^30)
};
struct CutoutRho {
    float rho[CO_MAX_WIDTH];
};
struct CutoutRow {                              // a row's best: pk = iw << 16 | j, CO_NONE without a score (C, M, A then +0)
    float C;
    unsigned pk;
    float M, A;
};
struct CutoutRecord {
    int id, status;
    float S, S0;
    short i, iw, j, pad;
    float M, A;
};

constexpr float CO_FLT_MAX = 3.402823466e+38f;

// one rounding each: this file's operators are not contracted (the pragma above)
__device__ __forceinline__ float co_add(float a, float b) { return a + b; }
__device__ __forceinline__ float co_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float co_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float co_div(float a, float b) { return a / b; }

__device__ __forceinline__ bool co_finite(float x) { return __builtin_fabsf(x) <= CO_FLT_MAX; }     // false for NaN and Inf

// monotonic over the floats that are not NaN, -0 taken as +0 (detrend_kernels.h dt_key), and its inverse
__device__ __forceinline__ unsigned co_key(float v) {
    const unsigned u = __float_as_uint(co_add(v, 0.f));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float co_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// The sum of c over the work-group's 256 threads in an integer counter in LDS: cnt[set] takes the adds of this call, and thread 0
// clears cnt[set + 1 mod 3] for the next one (its last readers passed the barrier of the call before this one; its next adders
// start behind this call's barrier).  Every thread calls it, with set = 0, 1, 2, 0, .. from call to call, cnt[0] cleared and
// published before the first; its barrier also publishes what the threads wrote to LDS before the call.
__device__ __forceinline__ unsigned co_block_sum(unsigned c, unsigned* cnt, int set) {
    if (c) atomicAdd(&cnt[set], c);
    if (threadIdx.x == 0) cnt[set == 2 ? 0 : set + 1] = 0;
    __syncthreads();
    return cnt[set];
}

// The median of the values whose keys are k[0 .. n), n even and at most 1024: fl(0.5f fl(lo + hi)) of the values of ranks n/2 - 1
// and n/2, found together by a search on the key, bit by bit from the top.  The low half of a count word counts the keys below
// the lower rank's trial key, the high half those below the upper one's.  The passes take the count sets set, set + 1, .. mod 3,
// and the next call set + 2 mod 3 (32 passes).
__device__ __forceinline__ float co_median(const unsigned* k, unsigned* cnt, int n, int set) {
    const unsigned rlo = (unsigned)(n / 2 - 1), rhi = (unsigned)(n / 2);
    unsigned klo = 0, khi = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const unsigned tlo = klo | (1u << bit), thi = khi | (1u << bit);
        unsigned c = 0;
        for (int q = threadIdx.x; q < n; q += CO_THREADS) {
            const unsigned x = k[q];
            c += (x < tlo ? 1u : 0u) + (x < thi ? 0x10000u : 0u);
        }
        c = co_block_sum(c, cnt, set);
        set = set == 2 ? 0 : set + 1;
        if ((c & 0xFFFFu) <= rlo) klo = tlo;
        if ((c >> 16) <= rhi) khi = thi;
    }
    return co_mul(0.5f, co_add(co_unkey(klo), co_unkey(khi)));
}

// the fine trial of row i, or -1 for an absent row
__device__ __forceinline__ int co_trial(int ic, int dstep, int i, int c, int ndmf) {
    const long long d = (long long)ic + (long long)(i - c) * dstep;
    return d < 0 || d >= ndmf ? -1 : (int)d;
}

// a beats b: a score against none, the larger score, among equal scores the smaller key
__device__ __forceinline__ bool co_better(float Ca, unsigned ka, float Cb, unsigned kb) {
    if (ka == CO_NONE) return false;
    if (kb == CO_NONE) return true;
    return Ca > Cb || (Ca == Cb && ka < kb);
}

// grid (ceil(ntu / 256), ndmc, r), 256 threads, CO_PARTIALS_LDS_BYTES of dynamic LDS; after the call's ingest on the same stream
__global__ __launch_bounds__(256) void cutout_partials_kernel(const float* __restrict__ ring, const int* __restrict__ s, const float* __restrict__ w, CutoutSlots sl,
                                                              float* __restrict__ W, float* __restrict__ P, int nfine, int L, int ndmf, int nband, int nt,
                                                              int tshift, int ndmc) {
    extern __shared__ float co_lds[];
    const int tid = threadIdx.x, z = blockIdx.z, i = blockIdx.y, m0 = blockIdx.x * CO_THREADS;
    const int c = ndmc >> 1, ntu = nt << tshift, tscr = 1 << tshift;
    const int j = (m0 >> tshift) + tid;                         // the output column this thread sums, if tid < 256 / tscr
    const bool sums = tid < (CO_THREADS >> tshift) && j < nt;
    float* Prow = P + ((size_t)z * ndmc + i) * nt;
    const int d = co_trial(sl.ic[z], sl.dstep[z], i, c, ndmf);
    if (d < 0) {                                                // (the same in every thread)
        if (sums) Prow[j] = 0.f;
        return;
    }
    const int m = m0 + tid, mc = m < ntu ? m : ntu - 1;         // (idle lanes read what a live lane reads)
    const int* srow = s + (size_t)d * nfine;
    const float* rows = ring + (size_t)sl.pair[z] * nfine * L;
    const int base = sl.slot0[z] + mc, arel = sl.a0[z] + mc;
    const bool centre = i == c;
    const int Q = nfine / nband;
    float B = 0.f;
    for (int g = 0; g < nband; g++) {
        float D = 0.f;
        for (int q = g * Q; q < (g + 1) * Q; q++) {
            const int sq = srow[q];
            const float wq = w[q];
            int slot = base + sq;                               // (slot0 < L and mc + sq < ntu + S <= nhist < L)
            slot -= slot >= L ? L : 0;
            const float x = rows[(size_t)q * L + slot];
            const bool ok = wq != 0.f && arel + sq >= 0;
            D = fmaf(wq, ok ? x : 0.f, D);
        }
        B = B + D;
        if (centre) {                                           // (the same in every thread)
            float* buf = co_lds + (g & 1) * CO_THREADS;         // (the half of band g - 2: its readers passed band g - 1's barrier)
            buf[tid] = D;
            __syncthreads();
            if (sums) {
                float a = 0.f;
                for (int u = 0; u < tscr; u++) a = a + buf[(tid << tshift) + u];
                W[((size_t)z * nband + g) * nt + j] = a;
            }
        }
    }
    float* buf = co_lds + 2 * CO_THREADS;
    buf[tid] = B;
    __syncthreads();
    if (sums) {
        float a = 0.f;
        for (int u = 0; u < tscr; u++) a = a + buf[(tid << tshift) + u];
        Prow[j] = a;
    }
}

// grid (ndmc, r), 256 threads, cutout_score_lds_bytes(nt) of dynamic LDS; after the partials on the same stream
__global__ __launch_bounds__(256) void cutout_score_kernel(const float* __restrict__ P, CutoutSlots sl, CutoutRow* __restrict__ rowrec, int ndmf, int ndmc, int nt,
                                                           int nwidth, float k_mad, CutoutRho rho) {
    extern __shared__ float co_lds[];
    unsigned* k = (unsigned*)co_lds;                // [nt]: the keys of P, then of |P - M|
    unsigned* cnt = k + nt;                         // [3] (and a word of padding)
    float* ya = co_lds + nt + 4;                    // [nt]
    float* yb = ya + nt;                            // [nt]
    float* rc = yb + nt;                            // [256]
    unsigned* rp = (unsigned*)(rc + CO_THREADS);    // [256]
    const int tid = threadIdx.x, i = blockIdx.x, z = blockIdx.y;
    CutoutRow* rec = rowrec + (size_t)z * ndmc + i;
    const CutoutRow none = {0.f, CO_NONE, 0.f, 0.f};
    if (co_trial(sl.ic[z], sl.dstep[z], i, ndmc >> 1, ndmf) < 0) {
        if (tid == 0) *rec = none;
        return;
    }
    const float* Prow = P + ((size_t)z * ndmc + i) * nt;
    if (tid == 0) cnt[0] = 0;
    __syncthreads();
    unsigned bad = 0;
    for (int j = tid; j < nt; j += CO_THREADS) {
        const float v = Prow[j];
        bad += co_finite(v) ? 0u : 1u;
        ya[j] = v;
        k[j] = co_key(v);
    }
    bad = co_block_sum(bad, cnt, 0);
    if (bad) {                                      // (the same in every thread)
        if (tid == 0) *rec = none;
        return;
    }
    const float M = co_median(k, cnt, nt, 1);       // (sets 1, 2, 0, .. 2)
    for (int j = tid; j < nt; j += CO_THREADS) k[j] = co_key(__builtin_fabsf(co_sub(co_unkey(k[j]), M)));
    __syncthreads();
    const float A = co_median(k, cnt, nt, 0);
    const float sc = co_mul(k_mad, A);
    if (!(sc > 0.f && sc <= CO_FLT_MAX)) {          // (the same in every thread)
        if (tid == 0) *rec = none;
        return;
    }
    const float G = co_div(1.0f, sc);
    for (int j = tid; j < nt; j += CO_THREADS) ya[j] = co_sub(ya[j], M);        // (each word by the thread that wrote it)
    __syncthreads();
    float bc = 0.f;
    unsigned bp = CO_NONE;
    float *cur = ya, *nxt = yb;
    for (int iw = 0; iw < nwidth; iw++) {
        const int wd = 1 << iw;
        const float r = rho.rho[iw];
        for (int j = tid; j < nt; j += CO_THREADS) {
            if (j < wd - 1) continue;
            const float C = co_mul(co_mul(cur[j], G), r);
            const unsigned pk = ((unsigned)iw << 16) | (unsigned)j;
            if (C == C && (bp == CO_NONE || C > bc)) {
                bc = C;
                bp = pk;
            }
        }
        if (iw + 1 < nwidth) {
            for (int j = tid; j < nt; j += CO_THREADS)
                if (j >= 2 * wd - 1) nxt[j] = co_add(cur[j], cur[j - wd]);
            __syncthreads();
            float* t = cur;
            cur = nxt;
            nxt = t;
        }
    }
    rc[tid] = bc;
    rp[tid] = bp;
    __syncthreads();
    for (int h = CO_THREADS / 2; h >= 1; h >>= 1) {
        if (tid < h && co_better(rc[tid + h], rp[tid + h], rc[tid], rp[tid])) {
            rc[tid] = rc[tid + h];
            rp[tid] = rp[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        CutoutRow o = none;
        if (rp[0] != CO_NONE) {
            o.C = rc[0];
            o.pk = rp[0];
            o.M = M;
            o.A = A;
        }
        *rec = o;
    }
}

// grid nreq_max, 256 threads, CO_PICK_LDS_BYTES of dynamic LDS; after the row scores on the same stream.  r = the slots served.
__global__ __launch_bounds__(256) void cutout_pick_kernel(const CutoutRow* __restrict__ rowrec, CutoutSlots sl, CutoutRecord* __restrict__ out, int ndmc, int r) {
    extern __shared__ float co_lds[];
    float* rc = co_lds;                             // [256]
    unsigned* rp = (unsigned*)(co_lds + CO_THREADS);        // [256]
    unsigned* ri = rp + CO_THREADS;                 // [256]: the row
    const int tid = threadIdx.x, z = blockIdx.x;
    if (z >= r) {
        if (tid == 0) out[z] = CutoutRecord{-1, 0, 0.f, 0.f, -1, -1, -1, 0, 0.f, 0.f};
        return;
    }
    const CutoutRow* rows = rowrec + (size_t)z * ndmc;
    rc[tid] = tid < ndmc ? rows[tid].C : 0.f;
    rp[tid] = tid < ndmc ? rows[tid].pk : CO_NONE;
    ri[tid] = (unsigned)tid;
    __syncthreads();
    for (int h = CO_THREADS / 2; h >= 1; h >>= 1) {
        // (the rows differ, so among equal scores the smaller row decides before the key is looked at)
        if (tid < h && rp[tid + h] != CO_NONE &&
            (rp[tid] == CO_NONE || rc[tid + h] > rc[tid] || (rc[tid + h] == rc[tid] && ri[tid + h] < ri[tid]))) {
            rc[tid] = rc[tid + h];
            rp[tid] = rp[tid + h];
            ri[tid] = ri[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        CutoutRecord o = {sl.id[z], 1, 0.f, 0.f, -1, -1, -1, 0, 0.f, 0.f};
        const CutoutRow ctr = rows[ndmc >> 1];
        if (ctr.pk != CO_NONE) o.S0 = ctr.C;
        if (rp[0] != CO_NONE) {
            const CutoutRow best = rows[ri[0]];
            o.status = 0;
            o.S = best.C;
            o.i = (short)ri[0];
            o.iw = (short)(best.pk >> 16);
            o.j = (short)(best.pk & 0xFFFFu);
            o.M = best.M;
            o.A = best.A;
        }
        out[z] = o;
    }
}

}  // namespace xeng
