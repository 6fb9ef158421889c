// Dirty images of the fine-channel visibilities (xengImage*, image.hip): the direct Fourier sum of UpchanCorr's matrix over a list
// of directions.
//
// Contract (include/xeng.h, "Dirty images of the fine-channel visibilities"); ninput = 2 nstand, group g = channels [g nfavg, (g+1) nfavg):
//   vis    cf32[nfine][nstand][2][nstand][2], UpchanCorr's span, V[c][s p][t q]; 16-byte aligned; never written
//   freq   f64[nfine] Hz, tau f64[npix][nstand] s, w f32[nstand] >= 0 (the context's state)
//   b_s(c,x) = w_s exp(-2 pi i frac(freq[c] tau[x][s])): the product and its fraction of a turn in fp64, sine and cosine of the
//            fraction (sincospif) and everything after them fp32
//   out    f32[nfine / nfavg][4][npix] = [XX, YY, Re(XY), Im(XY)],
//            I_pq[g][x] = norm * sum_{c in g, ascending} sum_{s,t} conj(b_s) V[c][s p][t q] b_t,  XX = Re I_00, YY = Re I_11, XY = I_01
//            A 2x2 block with w_s = 0 or w_t = 0 (and, without autos, s = t) is not loaded: its operand is a zero.
//
// One kernel, one work-group of 256 threads (four waves) per (tile of IMG_PX = 32 pixels, channel group).  Per channel of the group:
//   1. the steering tile b[s][x] into LDS, float2 at pitch IMG_PITCH = 33: thread e takes (x, s) = (e / nsp, e % nsp), so the
//      reads of tau run along s.  Stands s >= nstand (nsp = nstand rounded up to 32) and pixels >= npix get zeros.
//   2. U_pq[x][t] = sum_s conj(b_s[x]) V[s p][t q] on v_mfma_f32_32x32x2_f32, rows = the tile's pixels, columns = a tile of 32 stands
//      t, k = the stands s two at a time in ascending order.  Wave w takes the column tiles w, w + 4, ...  The A operand is the
//      steering tile from LDS (lane (r, h): b[s0 + h][r], one ds_read_b64), the B operand V read ALONG its rows: lane (r, h) loads
//      V[s0 + h, p = 0][t0 + r, q = 0..1] as one 16-byte word and V[s0 + h, 1][t0 + r, 1] as one 8-byte word, consecutive across
//      r.  Twelve MFMAs per k pair: for each of pq = 00, 01, 11
//          Ure += br Vr,  Ure += bi Vi,  Uim += br Vi,  Uim += (-bi) Vr          (the minus is an exact operand negation)
//      into six accumulator tiles.
//   3. per lane (its column t, its 16 rows x): P_pq[x] += U_pq[x][t] b_t[x] (fmaf, b from LDS), real part for XX and YY, both for
//      XY; the 64 partial sums per lane run over the wave's column tiles in ascending order and over the group's channels.
// After the last channel: a butterfly over the 32 lanes of each half (xor 1, 2, 4, 8, 16: one fixed tree, every lane ends with the
// same bits), the four waves' sums through LDS added in wave order, one multiply by norm, one store per word.
//
// A pixel's words depend on its own row of the MFMAs only: which other pixels share the tile, and which row it has, changes no
// bit.  Zero operands add fma(0, 0, C) = C.  No atomics, no scalar memory writes, no printf; one owner per word.
//
// LDS banks: ds_read_b64 takes the lanes 0..31 and 32..63 in one cycle each, bank = (address / 4) mod 64.  Step 2 reads 32
// consecutive float2 per half: 64 distinct banks at any pitch.  Step 3 reads b[t0 + (lane & 31)][x]: a stride of the pitch, 66
// dwords = 2 banks at pitch 33 -- 64 distinct banks again (at pitch 32 all 32 lanes of a half would meet on one pair).  Step 1
// stores along s at the same stride.
//
// image.hip is compiled with -fno-slp-vectorize (Makefile): complex fp32 arithmetic beside MFMA kernels, as upchan_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int IMG_PX = 32;          // pixels per work-group (the rows of the 32x32 MFMA)
constexpr int IMG_T = 32;           // stands per column tile
constexpr int IMG_PITCH = 33;       // float2 per stand of the steering tile
constexpr int IMG_WAVES = 4;
constexpr int IMG_THREADS = 64 * IMG_WAVES;

typedef float img_f32x16 __attribute__((ext_vector_type(16)));

// dynamic LDS of image_kernel: the steering tile, the weights, the waves' sums
__host__ __device__ constexpr size_t image_lds_bytes(int nstand) {
    const size_t nsp = (size_t)(nstand + IMG_T - 1) / IMG_T * IMG_T;
    return nsp * IMG_PITCH * sizeof(float2) + nsp * sizeof(float) + (size_t)IMG_WAVES * 4 * IMG_PX * sizeof(float);
}

// row of accumulator register v in lane half h (C/D map of the 32x32 MFMA: col = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 h)
__device__ __forceinline__ int img_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// grid (ceil(npix / IMG_PX), nfine / nfavg), IMG_THREADS threads, image_lds_bytes(nstand) of dynamic LDS
__global__ __launch_bounds__(IMG_THREADS) void image_kernel(const float2* __restrict__ vis, const double* __restrict__ freq, const double* __restrict__ tau,
                                                            const float* __restrict__ w, float* __restrict__ out, int nstand, int npix, int nfavg,
                                                            int autos, float norm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t img_lds[];
    const int nsp = (nstand + IMG_T - 1) / IMG_T * IMG_T, ntile = nsp / IMG_T;
    float2* bt = (float2*)img_lds;                               // [nsp][IMG_PITCH]
    float* wl = (float*)(bt + (size_t)nsp * IMG_PITCH);          // [nsp]
    float* red = wl + nsp;                                       // [IMG_WAVES][4][IMG_PX]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int x0 = blockIdx.x * IMG_PX, g = blockIdx.y;
    const size_t ninput = 2 * (size_t)nstand;

    for (int s = tid; s < nsp; s += IMG_THREADS) wl[s] = s < nstand ? w[s] : 0.f;
    float pxx[16], pyy[16], pre[16], pim[16];
#pragma unroll
    for (int v = 0; v < 16; v++) pxx[v] = pyy[v] = pre[v] = pim[v] = 0.f;

    for (int cc = 0; cc < nfavg; cc++) {
        const int c = g * nfavg + cc;
        __syncthreads();                                         // (the weights are there; the last channel's tile is done with)
        // 1. the steering tile
        const double f = freq[c];
        for (int e = tid; e < IMG_PX * nsp; e += IMG_THREADS) {
            const int xl = e / nsp, s = e - xl * nsp;
            float2 b = make_float2(0.f, 0.f);
            const float ws = wl[s];
            if (x0 + xl < npix && ws != 0.f) {
                const double turns = __dmul_rn(f, tau[(size_t)(x0 + xl) * nstand + s]);
                const float fr = (float)(turns - rint(turns));   // in [-1/2, 1/2]
                float sn, cs;
                sincospif(2.0f * fr, &sn, &cs);
                b = make_float2(ws * cs, -(ws * sn));
            }
            bt[s * IMG_PITCH + xl] = b;
        }
        __syncthreads();
        const float2* vc = vis + (size_t)c * ninput * ninput;
        for (int tj = wave; tj < ntile; tj += IMG_WAVES) {
            // 2. U_pq[x][t] over the stands s, two per MFMA
            const int t = tj * IMG_T + r;
            const bool tlive = t < nstand && wl[t] != 0.f;
            img_f32x16 u00r = {}, u00i = {}, u01r = {}, u01i = {}, u11r = {}, u11i = {};
            // four k pairs per trip: the loads first, then 48 MFMAs.  s0 + 7 <= nsp - 1, and the rows nstand .. nsp - 1 of the
            // tile are zeros: the pairs past the last stand add fma(0, 0, C) = C
            for (int s0 = 0; s0 < nstand; s0 += 8) {
                float2 b[4], v1[4];
                float4 v0[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int s = s0 + 2 * q + h;
                    b[q] = bt[s * IMG_PITCH + r];
                    v0[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                    v1[q] = make_float2(0.f, 0.f);
                    if (tlive && wl[s] != 0.f && (autos || s != t)) {       // (wl[s] = 0 for s >= nstand)
                        const float2* row = vc + (size_t)(2 * s) * ninput + 2 * t;
                        v0[q] = *(const float4*)row;             // V[s 0][t 0], V[s 0][t 1]
                        v1[q] = row[ninput + 1];                 // V[s 1][t 1]
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float br = b[q].x, bi = b[q].y, nbi = -b[q].y;
                    u00r = __builtin_amdgcn_mfma_f32_32x32x2f32(br, v0[q].x, u00r, 0, 0, 0);
                    u00i = __builtin_amdgcn_mfma_f32_32x32x2f32(br, v0[q].y, u00i, 0, 0, 0);
                    u01r = __builtin_amdgcn_mfma_f32_32x32x2f32(br, v0[q].z, u01r, 0, 0, 0);
                    u01i = __builtin_amdgcn_mfma_f32_32x32x2f32(br, v0[q].w, u01i, 0, 0, 0);
                    u11r = __builtin_amdgcn_mfma_f32_32x32x2f32(br, v1[q].x, u11r, 0, 0, 0);
                    u11i = __builtin_amdgcn_mfma_f32_32x32x2f32(br, v1[q].y, u11i, 0, 0, 0);
                    u00r = __builtin_amdgcn_mfma_f32_32x32x2f32(bi, v0[q].y, u00r, 0, 0, 0);
                    u00i = __builtin_amdgcn_mfma_f32_32x32x2f32(nbi, v0[q].x, u00i, 0, 0, 0);
                    u01r = __builtin_amdgcn_mfma_f32_32x32x2f32(bi, v0[q].w, u01r, 0, 0, 0);
                    u01i = __builtin_amdgcn_mfma_f32_32x32x2f32(nbi, v0[q].z, u01i, 0, 0, 0);
                    u11r = __builtin_amdgcn_mfma_f32_32x32x2f32(bi, v1[q].y, u11r, 0, 0, 0);
                    u11i = __builtin_amdgcn_mfma_f32_32x32x2f32(nbi, v1[q].x, u11i, 0, 0, 0);
                }
            }
            // 3. times b_t[x], into the lane's partial sums
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const float2 b = bt[t * IMG_PITCH + img_row(v, h)];
                pxx[v] = __builtin_fmaf(u00r[v], b.x, __builtin_fmaf(-u00i[v], b.y, pxx[v]));
                pyy[v] = __builtin_fmaf(u11r[v], b.x, __builtin_fmaf(-u11i[v], b.y, pyy[v]));
                pre[v] = __builtin_fmaf(u01r[v], b.x, __builtin_fmaf(-u01i[v], b.y, pre[v]));
                pim[v] = __builtin_fmaf(u01r[v], b.y, __builtin_fmaf(u01i[v], b.x, pim[v]));
            }
        }
    }
    // the 32 columns of each half, then the waves in order
#pragma unroll
    for (int v = 0; v < 16; v++) {
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
            pxx[v] += __shfl_xor(pxx[v], m);
            pyy[v] += __shfl_xor(pyy[v], m);
            pre[v] += __shfl_xor(pre[v], m);
            pim[v] += __shfl_xor(pim[v], m);
        }
        if (r == 0) {
            float* q = red + wave * 4 * IMG_PX + img_row(v, h);
            q[0] = pxx[v];
            q[IMG_PX] = pyy[v];
            q[2 * IMG_PX] = pre[v];
            q[3 * IMG_PX] = pim[v];
        }
    }
    __syncthreads();
    if (tid < 4 * IMG_PX) {
        const int k = tid / IMG_PX, xl = tid - k * IMG_PX;
        if (x0 + xl < npix) {
            float sum = red[tid];
#pragma unroll
            for (int wv = 1; wv < IMG_WAVES; wv++) sum += red[wv * 4 * IMG_PX + tid];
            out[((size_t)g * 4 + k) * npix + x0 + xl] = sum * norm;
        }
    }
}

}  // namespace xeng
