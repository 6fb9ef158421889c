// Phase folding of fine-channel power beams (xengFold*, fold.hip): every window of every (pair, channel, product) is added into
// the profile bin that an integer oscillator names, and a dump rotates the channels against each other and sums them.
//
// Contract (include/xeng.h, "Phase-folded profiles of the fine-channel power beams"):
//   in    f32[nwin_call][npair][nfine][4] = [XX, YY, Re XY*, Im XY*], q ascending in frequency
//   osc   per pair {u64 phi0, u64 dphi, i64 ddphi, active}: with m = n - n_ref windows, in wrapping 64-bit arithmetic
//         Phi(m) = phi0 + dphi*m + ddphi*(m(m-1)/2) turns * 2^64 and bin = ((Phi >> 32) * nbin) >> 32
//   prof  f32[npair][nbin][nfine][nprod], UNROTATED, q (and the product) the fastest axis: the bin of a window is the same for
//         every channel of a pair, so a wave's loads and stores are consecutive words of one profile row
//   out   f32[npair][nprod][nfine / nfscr][nbin] (dump): out[p][k][g][b] = sum over the nfscr channels of group g, ascending q,
//         of w[q] * prof[p][(b + rot[p][q]) mod nbin][q][k], one fmaf(w[q], x, sum) each from +0
//
// Decomposition:
//   fold       one launch per call, grid (ceil(nfine*nprod / 256), npair).  A thread owns ONE profile word position (p, q, k)
//              -- nprod = 4: the four words of a channel go to four neighbouring lanes, so 4-byte accesses are still
//              consecutive across a wave; nprod = 1: a lane reads XX and YY of its channel as one 8-byte load -- and walks
//              the call's windows in ascending order: the running word stays in a register while the bin stays, and is stored
//              and the next bin's word taken when it changes.  That is the one strictly sequential chain of fp32 adds the
//              contract asks for, whatever the split of a run over calls.  The windows are taken FOLD_BATCH at a time: the
//              batch's inputs and the profile words of its bins are loaded up front, independent of the chain; a bin that
//              the batch itself (or the word carried in the register) has written before is read again after the store by the
//              same thread instead, so a period shorter than a call works.  Bins are wave-uniform integer arithmetic.
//   dump       grid (bin tiles * channel blocks, npair), 256 threads.  A work-group owns 64 output bins of one pair and either
//              one channel group (nfscr >= 32: taken in chunks of 32 channels) or as many whole groups as fit 32 channels.
//              Load phase: lane = channel, so reads are consecutive along q wherever neighbouring channels share a rotation
//              (the row index is per channel, the same for all of a channel's products), into LDS [k][q][b] (rows padded by
//              one word).  Sum phase: lane = bin, so LDS reads and the global writes are consecutive along b.  Every profile
//              word is read by exactly one thread, which writes +0 over it when the dump clears.
//
// fold.hip is compiled with -fno-slp-vectorize (Makefile), as the other fine-channel code objects are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace xeng {

constexpr int FOLD_BATCH = 8;       // windows whose loads are in flight together
constexpr int FOLD_QC = 32;         // dump: channels per chunk
constexpr int FOLD_BT = 64;         // dump: output bins per work-group

struct FoldOsc {
    uint64_t phi0, dphi;
    int64_t ddphi;
    uint32_t active, pad;
};

// the bin of the window m windows after the reference one (0 <= m < 2^31: m(m-1)/2 is exact in 64 bits)
__host__ __device__ __forceinline__ uint32_t fold_bin(const FoldOsc& o, uint64_t m, uint32_t nbin) {
    const uint64_t tri = (m * (m - (m ? 1 : 0))) >> 1;
    const uint64_t phi = o.phi0 + o.dphi * m + (uint64_t)o.ddphi * tri;
    return (uint32_t)(((phi >> 32) * (uint64_t)nbin) >> 32);
}

// the folded quantity of word j (= q*NPROD + k) of a window's row of one pair
template <int NPROD>
__device__ __forceinline__ float fold_input(const float* __restrict__ row, int j) {
    if constexpr (NPROD == 1) {
        const float2 v = *(const float2*)(row + (size_t)j * 4);
        return v.x + v.y;
    } else {
        return row[j];
    }
}

// grid (ceil(nfine*NPROD / 256), npair), 256 threads; m0 = n - n_ref of the call's first window
template <int NPROD>
__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ in, float* __restrict__ prof, const FoldOsc* __restrict__ osc,
                                                   int npair, int nfine, int nbin, unsigned m0, int nc) {
    const int p = blockIdx.y;
    const FoldOsc o = osc[p];
    if (!o.active) return;
    const int W = nfine * NPROD;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= W) return;
    const size_t wstride = (size_t)npair * nfine * 4;
    const float* src = in + (size_t)p * nfine * 4;
    float* col = prof + (size_t)p * nbin * W + j;
    int cur = -1;                       // the bin whose word `acc` holds (-1: none yet)
    float acc = 0.f;
    for (int i0 = 0; i0 < nc; i0 += FOLD_BATCH) {
        float x[FOLD_BATCH], pw[FOLD_BATCH];
        int b[FOLD_BATCH];
        const int carried = cur;
#pragma unroll
        for (int u = 0; u < FOLD_BATCH; u++) {
            const int i = i0 + u < nc ? i0 + u : nc - 1;            // (a batch's tail repeats the last window's loads; unused)
            b[u] = (int)fold_bin(o, (uint64_t)m0 + (uint64_t)i, (uint32_t)nbin);
            x[u] = fold_input<NPROD>(src + (size_t)i * wstride, j);
            pw[u] = col[(size_t)b[u] * W];
        }
#pragma unroll
        for (int u = 0; u < FOLD_BATCH; u++) {
            if (i0 + u < nc) {
                if (b[u] != cur) {
                    if (cur >= 0) col[(size_t)cur * W] = acc;
                    bool fresh = b[u] != carried;                   // (wave-uniform) nothing since the batch's loads wrote this bin
#pragma unroll
                    for (int v = 0; v < u; v++) fresh = fresh && b[v] != b[u];
                    acc = fresh ? pw[u] : col[(size_t)b[u] * W];
                    cur = b[u];
                }
                acc = acc + x[u];
            }
        }
    }
    if (cur >= 0) col[(size_t)cur * W] = acc;
}

// +0 over the profile's nwords words (xengFoldReset), grid-stride
__global__ __launch_bounds__(256) void fold_clear_kernel(float* __restrict__ prof, size_t nwords) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += stride) prof[i] = 0.f;
}

// grid (nbt * ngb, npair), 256 threads: nbt = ceil(nbin / 64) bin tiles, ngb = ceil(ngroups / gpw) channel blocks of
// gpw = max(1, 32 / nfscr) groups.  hits: u32[npair][nbin] (read only when normalise).
template <int NPROD>
__global__ __launch_bounds__(256) void fold_dump_kernel(float* __restrict__ prof, const FoldOsc* __restrict__ osc, const int* __restrict__ rot,
                                                        const float* __restrict__ w, const uint32_t* __restrict__ hits, float* __restrict__ out,
                                                        int nfine, int nbin, int nfscr, int gpw, int normalise, int clear) {
    __shared__ float tile[NPROD][FOLD_QC][FOLD_BT + 1];
    __shared__ float wq[FOLD_QC];
    const int t = threadIdx.x, p = blockIdx.y;
    const int nbt = (nbin + FOLD_BT - 1) / FOLD_BT;
    const int b0 = (blockIdx.x % nbt) * FOLD_BT, g0 = (blockIdx.x / nbt) * gpw;
    const int ngroups = nfine / nfscr;
    const int gcount = g0 + gpw < ngroups ? gpw : ngroups - g0;             // groups of this work-group
    const int qa = g0 * nfscr, qb = qa + gcount * nfscr;                    // its channels
    const bool active = osc[p].active != 0;
    const int W = nfine * NPROD;
    float* rows = prof + (size_t)p * nbin * W;
    const int items = NPROD * gcount * FOLD_BT;                             // outputs (k, group, bin); <= 256 when there are several chunks
    float acc = 0.f;
    for (int c0 = qa; c0 < qb; c0 += FOLD_QC) {
        const int cn = qb - c0 < FOLD_QC ? qb - c0 : FOLD_QC;
        // load: lane = channel
        const int ql = t & (FOLD_QC - 1), q = c0 + ql;
        if (t < FOLD_QC) wq[t] = t < cn ? w[c0 + t] : 0.f;
        if (ql < cn) {
            const int r0 = rot[(size_t)p * nfine + q];
            for (int bl = t / FOLD_QC; bl < FOLD_BT; bl += 256 / FOLD_QC) {
                const int b = b0 + bl;
                if (b >= nbin) break;
                int r = b + r0;
                r -= r >= nbin ? nbin : 0;
                float* word = rows + (size_t)r * W + (size_t)q * NPROD;
                float v[NPROD];
#pragma unroll
                for (int k = 0; k < NPROD; k++) v[k] = 0.f;
                if (active) {
                    if constexpr (NPROD == 4) {
                        const float4 f = *(const float4*)word;
                        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                    } else {
                        v[0] = *word;
                    }
                    if (normalise) {
                        const uint32_t h = hits[(size_t)p * nbin + r];
                        const float hf = (float)h;
#pragma unroll
                        for (int k = 0; k < NPROD; k++) v[k] = h ? __fdiv_rn(v[k], hf) : 0.f;
                    }
                }
                if (clear) {
                    if constexpr (NPROD == 4)
                        *(float4*)word = make_float4(0.f, 0.f, 0.f, 0.f);
                    else
                        *word = 0.f;
                }
#pragma unroll
                for (int k = 0; k < NPROD; k++) tile[k][ql][bl] = v[k];
            }
        }
        __syncthreads();
        // sum: lane = bin
        for (int it = t; it < items; it += 256) {
            const int bl = it & (FOLD_BT - 1), rest = it / FOLD_BT, k = rest % NPROD, gl = rest / NPROD;
            const int b = b0 + bl;
            float s = c0 == qa ? 0.f : acc;
            const int qlo = gl * nfscr - (c0 - qa) > 0 ? gl * nfscr - (c0 - qa) : 0;
            const int qhi = (gl + 1) * nfscr - (c0 - qa) < cn ? (gl + 1) * nfscr - (c0 - qa) : cn;
            if (b < nbin) {
                for (int qq = qlo; qq < qhi; qq++) {
                    const float wv = wq[qq];
                    if (wv != 0.f) s = fmaf(wv, tile[k][qq][bl], s);
                }
                if (c0 + FOLD_QC >= qb) out[(((size_t)p * NPROD + k) * ngroups + (g0 + gl)) * nbin + b] = s;
            }
            acc = s;
        }
        __syncthreads();
    }
}

}  // namespace xeng
