// Incoherent dedispersion of fine-channel power beams (xengDedisp*, dedisp.hip): a direct sum over a caller-supplied grid of DM
// trials, streaming across calls through a history ring on the device.
//
// Contract (include/xeng.h, "Incoherent dedispersion of fine-channel power beams"):
//   in    f32[nwin_call][npair][nfine][4] = [XX, YY, Re XY*, Im XY*], q ascending in frequency
//   hist  f32[npair][nfine][nprod][L], L = max_delay + nwin: window n of (pair, channel, product) at slot n mod L, unweighted;
//         nprod = 1 keeps I = XX + YY (one f32 add), nprod = 4 the four words
//   bt    i32[nfine][ndm], the back-delays b[d][q] = S - s[d][q] transposed, so that neighbouring trials are neighbouring words
//   out   f32[nwin_call][npair][ndm][nprod]:  y[n][p][d] = sum_q w[q] * x[n - b[d][q]][p][q], a term with n - b < 0 or w[q] = 0
//         left out
//
// Decomposition, two launches per call on one stream:
//   ingest       a work-group moves a tile of 32 channels x 32 windows of one pair: 16-byte loads consecutive across lanes
//                along q, through LDS (rows padded by one word), 4-byte stores consecutive across lanes along time.
//   dedisperse   a work-group of 4 waves owns 64 outputs of one pair, a tile of TT windows x 64/TT trials (TT the power of two
//                >= nwin_call, at most 64): lane = (window, trial).  For one q the lanes of a trial read a contiguous run of the
//                history row and neighbouring trials, whose delays differ by little, read runs that overlap it.  Wave s sums
//                segment s of the channels; the four partial sums meet in LDS.
// Summation order (the same for every nwin_call, tile shape, split of a run over calls and ring position): the channels are cut
// into DD_NSEG = 4 segments of Q = ceil(nfine / 4) consecutive channels, segment s = [s*Q, min((s+1)*Q, nfine)).  A segment's
// partial sum starts from +0 and takes its channels in ascending q, one fmaf(w[q], x, sum) each (a left-out term enters as
// fmaf(w[q], +0, sum)); the output is ((P0 + P1) + P2) + P3.  fp32, no atomics.
//
// dedisp.hip is compiled with -fno-slp-vectorize (Makefile), as the other fine-channel code objects are.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int DD_NSEG = 4;      // channel segments = waves per dedisperse work-group
constexpr int DD_TILE = 32;     // ingest tile: channels x windows

// slot of the window `rel` windows after the one at `head` (-L <= rel, head + rel < 2L)
__device__ __forceinline__ int dd_slot(int head, int rel, int L) {
    int s = head + rel;
    s += s < 0 ? L : 0;
    s -= s >= L ? L : 0;
    return s;
}

// grid (ceil(nfine / 32), npair, ceil(nc / 32)), 256 threads; head = slot of the call's first window
template <int NPROD>
__global__ __launch_bounds__(256) void dedisp_ingest_kernel(const float4* __restrict__ in, float* __restrict__ hist, int npair, int nfine, int L,
                                                            int head, int nc) {
    __shared__ float tile[NPROD][DD_TILE][DD_TILE + 1];
    const int p = blockIdx.y, q0 = blockIdx.x * DD_TILE, t0 = blockIdx.z * DD_TILE;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
    for (int i = 0; i < DD_TILE / 8; i++) {
        const int tt = hi + 8 * i, t = t0 + tt, q = q0 + lo;
        if (t < nc && q < nfine) {
            const float4 v = in[((size_t)t * npair + p) * nfine + q];
            if constexpr (NPROD == 1) {
                tile[0][lo][tt] = v.x + v.y;
            } else {
                tile[0][lo][tt] = v.x;
                tile[1][lo][tt] = v.y;
                tile[2][lo][tt] = v.z;
                tile[3][lo][tt] = v.w;
            }
        }
    }
    __syncthreads();
    const int t = t0 + lo;
    if (t >= nc) return;
    const int slot = dd_slot(head, t, L);
    for (int i = 0; i < DD_TILE / 8; i++) {
        const int qq = hi + 8 * i, q = q0 + qq;
        if (q >= nfine) break;
        float* row = hist + ((size_t)p * nfine + q) * NPROD * L;
#pragma unroll
        for (int k = 0; k < NPROD; k++) row[(size_t)k * L + slot] = tile[k][qq][lo];
    }
}

// grid (ceil(nc / TT) * ceil(ndm / (64 / TT)), npair), 256 threads, TT = 1 << tshift <= 64; head = slot of the call's first
// window (already ingested), n0 = windows since the last reset before this call (clamped: only its sign against a delay counts)
template <int NPROD>
__global__ __launch_bounds__(256) void dedisp_kernel(const float* __restrict__ hist, const int* __restrict__ bt, const float* __restrict__ w,
                                                     float* __restrict__ out, int npair, int nfine, int ndm, int L, int head, int n0, int nc,
                                                     int tshift) {
    __shared__ float part[DD_NSEG - 1][NPROD][64];
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int TT = 1 << tshift, DD = 64 >> tshift;
    const int tiles_t = (nc + TT - 1) >> tshift;
    const int tile_t = blockIdx.x % tiles_t, tile_d = blockIdx.x / tiles_t, p = blockIdx.y;
    const int t = tile_t * TT + (lane & (TT - 1)), d = tile_d * DD + (lane >> tshift);
    const bool live = t < nc && d < ndm;
    const int tc = t < nc ? t : nc - 1, dc = d < ndm ? d : ndm - 1;       // (idle lanes read what a live lane reads)
    const int Q = (nfine + DD_NSEG - 1) / DD_NSEG;
    const int q0 = seg * Q, q1 = q0 + Q < nfine ? q0 + Q : nfine;
    const float* rows = hist + (size_t)p * nfine * NPROD * L;
    float acc[NPROD];
#pragma unroll
    for (int k = 0; k < NPROD; k++) acc[k] = 0.f;
#pragma unroll 4
    for (int q = q0; q < q1; q++) {
        const int rel = tc - bt[(size_t)q * ndm + dc];
        const float wq = w[q];
        const bool ok = wq != 0.f && rel + n0 >= 0;
        const float* row = rows + (size_t)q * NPROD * L + dd_slot(head, rel, L);
#pragma unroll
        for (int k = 0; k < NPROD; k++) {
            const float x = row[(size_t)k * L];
            acc[k] = fmaf(wq, ok ? x : 0.f, acc[k]);
        }
    }
    if (seg) {
#pragma unroll
        for (int k = 0; k < NPROD; k++) part[seg - 1][k][lane] = acc[k];
    }
    __syncthreads();
    if (seg || !live) return;
    float* o = out + (((size_t)t * npair + p) * ndm + d) * NPROD;
#pragma unroll
    for (int k = 0; k < NPROD; k++) o[k] = ((acc[k] + part[0][k][lane]) + part[1][k][lane]) + part[2][k][lane];
}

}  // namespace xeng
