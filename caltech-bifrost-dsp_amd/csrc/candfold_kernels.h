// Folding of search candidates (xengCandfold*, candfold.hip): every candidate's own (pair, trial) series of the dedispersed beams
// is folded by an integer oscillator into nsub sub-integrations x nbin phase bins, and at the end of each segment a grid of period /
// period-derivative offsets is searched per candidate on the folded cube: one record and one best profile per candidate come out.
//
// Contract (include/xeng.h, "Folding of search candidates"); W = nsub*nbin <= 8192 words, NT = nsub*nsubwin windows a segment:
//   in     f32[nc][nser][NPROD], z = word 0 (NPROD = 1) or word 0 + word 1 (NPROD = 4); never written
//   cand   CfCand[ncand_max] = {u64 phi0, u64 dphi, i64 ddphi, u32 series, u32 active}; the bin of a window is fold_bin's
//          (fold_kernels.h), m = n - n_ref
//   cube   f32[ncand_max][nsub][nbin], hits u32 the same: the segment in progress; a second pair of the same size keeps the last
//          completed segment for xengCandfoldGetCube
//   rot    i32[ntrial][nsub], r_t(s) mod nbin in 0..nbin-1, from cf_shift on the host
//   g      f32[nwidth]
//   out    CfRecord[ncand_max], then f32[ncand_max][nbin] best profiles
//
// Fold, every call, one work-group per candidate: the call's windows are taken CF_TILE at a time.  Lane i of the tile loads the
// word(s) of window i of the candidate's series -- a strided gather, one word per line; candidates on neighbouring trials share
// lines in L2 -- and writes z and the window's cell s*nbin + bin to LDS.  After a barrier thread b < nbin walks the tile in window
// order and adds the windows of its bin: the running word of cell (s, b) stays in a register while s stays and goes to the cube
// when it changes.  Every cell has one owner and its adds happen in ascending n: the one sequential chain, whatever the period
// (shorter than nbin windows, longer than a call) and however calls cut the run.  The walk's LDS reads, four windows each, are
// the same address in every lane: broadcasts.
//
// Refine, per completed segment, one work-group per candidate: cube and hits come into LDS (2 W words, up to 64 KiB).  The 256
// threads are 256 / nbin groups of nbin lanes; a group takes the trials g, g + 256 / nbin, ...; lane = bin.  Per trial the shifted
// sums over s, the division, then the boxcar tree between two rows of LDS per group, one barrier a width; every thread keeps its
// best (C, key), key = (t * 8 + iw) * 256 + j, and thread 0 takes the best of the 256 through LDS.  A last pass recomputes the
// winning trial's profile and stores it.
//   LDS banks: a 4-byte read serves a wave in two groups of 32 lanes, bank = word address mod 32.  The shifted read is word
//   s*nbin + ((j - r) mod nbin) for consecutive lanes j: consecutive words of one row apart from one wrap.  nbin >= 32: the 32
//   lanes of a group read 32 consecutive words mod nbin of a row that is a multiple of 32 words long and starts at a multiple of
//   32: 32 different banks.  nbin = 16: the group's two trials read the same row of 16 words under different rotations; the row
//   has one word per bank, so lanes that meet in a bank read the same word: a broadcast.  The boxcar rows are 256 words per
//   buffer, the lanes of trial group gi at gi*nbin: the same argument.
//
// Clear: +0 over a cube and its hits, grid-stride.
//
// No atomics; every word has one owner; no work-group waits for another.  No product is contracted into a sum: refine is written in
// __fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn.
//
// candfold.hip is compiled with -fno-slp-vectorize (Makefile), with the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

constexpr int CF_THREADS = 256;
constexpr int CF_TILE = 256;            // fold: windows of a tile, one per thread
constexpr int CF_MAX_WIDTH = 8;         // 2^(nwidth-1) <= nbin/2 <= 128
constexpr int CF_REFINE_EXTRA = 4 * CF_THREADS + 8;     // refine: words of LDS behind cube and hits

struct CfCand {
    uint64_t phi0, dphi;
    int64_t ddphi;
    uint32_t series, active;
};

struct alignas(16) CfRecord {
    float S, S0;
    int16_t it, iw, j, pad;
};

// the bin of the window m windows after the reference one: fold_bin (fold_kernels.h) word for word
__host__ __device__ __forceinline__ uint32_t cf_bin(const CfCand& o, uint64_t m, uint32_t nbin) {
    const uint64_t tri = (m * (m - (m ? 1 : 0))) >> 1;
    const uint64_t phi = o.phi0 + o.dphi * m + (uint64_t)o.ddphi * tri;
    return (uint32_t)(((phi >> 32) * (uint64_t)nbin) >> 32);
}

// r_t(s) = floor((2N + D) / (2D)), N = d1*u*nsub + 2*d2*u^2, u = 2s + 1 - nsub, D = 32 nsub^2 (|d| <= 2^20, nsub <= 64: |N| < 2^40)
__host__ __device__ __forceinline__ long long cf_shift(int d1, int d2, int s, int nsub) {
    const long long u = 2 * (long long)s + 1 - nsub;
    const long long N = (long long)d1 * u * nsub + 2 * (long long)d2 * u * u;
    const long long D = 32LL * nsub * nsub;
    const long long a = 2 * N + D, b = 2 * D;
    long long q = a / b;
    if (a % b != 0 && a < 0) q--;
    return q;
}

// one window of the walk of thread `tid`: its bin's windows go into the running word of their cell, which changes with s
__device__ __forceinline__ void cf_walk(float cbits, float z, int tid, int nbin, int& cur, float& acc, uint32_t& h, float* col, uint32_t* hcol) {
    const int cell = (int)__float_as_uint(cbits);
    if ((cell & (nbin - 1)) != tid) return;
    if (cell != cur) {
        if (cur >= 0) {
            col[cur] = acc;
            hcol[cur] = h;
        }
        acc = col[cell];
        h = hcol[cell];
        cur = cell;
    }
    acc = acc + z;
    h++;
}

// grid ncand_max, 256 threads, 2 * CF_TILE words of dynamic LDS.  The call's windows are [pos, pos + nc) of the segment,
// pos + nc <= NT; m0 = n - n_ref of the first of them.
template <int NPROD>
__global__ __launch_bounds__(256) void candfold_fold_kernel(const float* __restrict__ in, float* __restrict__ cube, uint32_t* __restrict__ hits,
                                                            const CfCand* __restrict__ cand, int nser, int nbin, int W, int nsubwin, int pos, unsigned m0,
                                                            int nc) {
    extern __shared__ float cf_lds[];
    const int tid = threadIdx.x;
    const size_t c = blockIdx.x;
    const CfCand o = cand[c];
    if (!o.active) return;
    float* lz = cf_lds;
    float* lc = cf_lds + CF_TILE;       // the cell s*nbin + bin of a window, as bits
    float* col = cube + c * (size_t)W;
    uint32_t* hcol = hits + c * (size_t)W;
    int cur = -1;                       // the cell whose word `acc` holds (-1: none yet)
    float acc = 0.f;
    uint32_t h = 0;
    for (int i0 = 0; i0 < nc; i0 += CF_TILE) {
        const int n = nc - i0 < CF_TILE ? nc - i0 : CF_TILE;
        if (tid < n) {
            const int i = i0 + tid;
            const float* word = in + ((size_t)i * nser + o.series) * NPROD;
            float z;
            if constexpr (NPROD == 4) {
                const float4 v = *(const float4*)word;
                z = v.x + v.y;
            } else {
                z = *word;
            }
            const uint32_t s = (uint32_t)(pos + i) / (uint32_t)nsubwin;
            const uint32_t b = cf_bin(o, (uint64_t)m0 + (uint64_t)i, (uint32_t)nbin);
            lz[tid] = z;
            lc[tid] = __uint_as_float(s * (uint32_t)nbin + b);
        }
        __syncthreads();
        if (tid < nbin) {
            for (int w = 0; w < n; w += 4) {        // four windows a read (words past n are read and not used), taken in their order
                const float4 c4 = *(const float4*)(lc + w), z4 = *(const float4*)(lz + w);
                cf_walk(c4.x, z4.x, tid, nbin, cur, acc, h, col, hcol);
                if (w + 1 < n) cf_walk(c4.y, z4.y, tid, nbin, cur, acc, h, col, hcol);
                if (w + 2 < n) cf_walk(c4.z, z4.z, tid, nbin, cur, acc, h, col, hcol);
                if (w + 3 < n) cf_walk(c4.w, z4.w, tid, nbin, cur, acc, h, col, hcol);
            }
        }
        __syncthreads();
    }
    if (cur >= 0) {
        col[cur] = acc;
        hcol[cur] = h;
    }
}

// +0 over nwords words, grid-stride
__global__ __launch_bounds__(256) void candfold_clear_kernel(uint32_t* __restrict__ words, size_t nwords) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += stride) words[i] = 0u;
}

// larger C, then the smaller key; a NaN never enters
__device__ __forceinline__ void cf_take(float& bS, int& bK, float S, int k) {
    if (S != S) return;
    if (bK < 0 || S > bS || (S == bS && k < bK)) {
        bS = S;
        bK = k;
    }
}

// the profile word of bin j at the trial whose shifts are r[0..nsub): the shifted sums over s, then the division
__device__ __forceinline__ float cf_profile(const float* lcube, const float* lhits, const int* __restrict__ r, int nsub, int nbin, int j) {
    float P = 0.f;
    uint32_t H = 0;
    for (int s = 0; s < nsub; s++) {
        const int e = s * nbin + ((j - r[s]) & (nbin - 1));
        P = __fadd_rn(P, lcube[e]);
        H += __float_as_uint(lhits[e]);
    }
    return H ? __fdiv_rn(P, (float)H) : 0.f;
}

// grid ncand_max, 256 threads, (2 W + CF_REFINE_EXTRA) words of dynamic LDS.  zrot: nsub zeros.  izero: the first trial with
// d1 = d2 = 0, or -1.
__global__ __launch_bounds__(256) void candfold_refine_kernel(const float* __restrict__ cube, const uint32_t* __restrict__ hits,
                                                              const CfCand* __restrict__ cand, const int* __restrict__ rot, const int* __restrict__ zrot,
                                                              const float* __restrict__ gain, CfRecord* __restrict__ rec, float* __restrict__ prof, int nsub,
                                                              int nbin, int nwidth, int ntrial, int izero) {
    extern __shared__ float cf_lds[];
    const int tid = threadIdx.x;
    const size_t c = blockIdx.x;
    const int W = nsub * nbin;
    float* lcube = cf_lds;
    float* lhits = cf_lds + W;                      // u32, as bits
    float* box = lhits + W;                         // [2][256]
    float* mailS = box + 2 * CF_THREADS;            // [256]
    float* mailK = mailS + CF_THREADS;              // [256], i32 as bits
    float* misc = mailK + CF_THREADS;               // [8]: the winning key; S; S0
    float* pout = prof + c * (size_t)nbin;
    if (!cand[c].active) {
        if (tid == 0) rec[c] = CfRecord{0.f, 0.f, -1, -1, -1, 0};
        if (tid < nbin) pout[tid] = 0.f;
        return;
    }
    for (int e = tid; e < W; e += CF_THREADS) {
        lcube[e] = cube[c * (size_t)W + e];
        lhits[e] = __uint_as_float(hits[c * (size_t)W + e]);
    }
    __syncthreads();
    const int j = tid & (nbin - 1), gi = tid / nbin, ngroup = CF_THREADS / nbin;

    // total_c: the bins of the zero-shift profile in ascending order, by every thread for itself
    if (tid < nbin) box[tid] = cf_profile(lcube, lhits, zrot, nsub, nbin, tid);
    __syncthreads();
    float total = box[0];
    for (int b = 1; b < nbin; b++) total = __fadd_rn(total, box[b]);
    __syncthreads();

    float bS = 0.f, b0 = 0.f;
    int bK = -1, k0 = -1;
    float* mine = box + gi * nbin;
    int cb = 0;                                     // the buffer that takes B_w: the two alternate from width to width and on across
                                                    // the trials, so that one barrier separates a buffer's reads from its next writes
    for (int t0 = 0; t0 < ntrial; t0 += ngroup) {
        const int t = t0 + gi;
        const bool on = t < ntrial;
        float B = 0.f;
        if (on) B = cf_profile(lcube, lhits, rot + (size_t)t * nsub, nsub, nbin, j);
        for (int iw = 0; iw < nwidth; iw++) {
            const int w = 1 << iw;
            if (on) {
                const float base = __fmul_rn(total, __fdiv_rn((float)w, (float)nbin));
                const float C = __fmul_rn(__fsub_rn(B, base), gain[iw]);
                const int key = (t * 8 + iw) * 256 + j;
                cf_take(bS, bK, C, key);
                if (t == izero) cf_take(b0, k0, C, key);
            }
            if (iw + 1 < nwidth) {
                if (on) mine[cb * CF_THREADS + j] = B;
                __syncthreads();
                if (on) B = __fadd_rn(B, mine[cb * CF_THREADS + ((j + w) & (nbin - 1))]);
                cb ^= 1;
            }
        }
    }
    __syncthreads();
    mailS[tid] = bS;
    mailK[tid] = __int_as_float(bK);
    __syncthreads();
    if (tid == 0) {
        float S = 0.f;
        int K = -1;
        for (int i = 0; i < CF_THREADS; i++) {
            const int k = __float_as_int(mailK[i]);
            if (k >= 0) cf_take(S, K, mailS[i], k);
        }
        misc[0] = __int_as_float(K);
        misc[1] = S;
    }
    __syncthreads();
    mailS[tid] = b0;
    mailK[tid] = __int_as_float(k0);
    __syncthreads();
    if (tid == 0) {
        float S0 = 0.f;
        int K0 = -1;
        for (int i = 0; i < CF_THREADS; i++) {
            const int k = __float_as_int(mailK[i]);
            if (k >= 0) cf_take(S0, K0, mailS[i], k);
        }
        const int K = __float_as_int(misc[0]);
        if (K0 < 0) S0 = 0.f;
        rec[c] = K < 0 ? CfRecord{0.f, S0, -1, -1, -1, 0} : CfRecord{misc[1], S0, (int16_t)(K >> 11), (int16_t)((K >> 8) & 7), (int16_t)(K & 255), 0};
    }
    const int K = __float_as_int(misc[0]);
    if (tid < nbin) pout[tid] = K < 0 ? 0.f : cf_profile(lcube, lhits, rot + (size_t)(K >> 11) * nsub, nsub, nbin, tid);
}

}  // namespace xeng
