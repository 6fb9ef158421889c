// Hogbom CLEAN of the dirty images (xengClean*, clean.hip): the brightest window pixel of every channel group found, a fraction
// `gain` of it recorded as a component and its exact point-spread function subtracted from every pixel, niter times at the most.
//
// Contract (include/xeng.h, "Hogbom CLEAN of the dirty images"); group g = channels [g nfavg, (g+1) nfavg):
//   image  f32[ngroup][4][npix] = [XX, YY, Re XY, Im XY], UpchanImage's span; 16-byte aligned; never written
//   freq   f64[nfine] Hz, tauT f64[nstand][npix] s (the delays TRANSPOSED by SetGeometry: a wave's reads run along the pixels),
//          w f32[nstand] >= 0, mask u8[npix] (the context's state)
//   PSF_g(x, x0) = norm * sum_{c in g, ascending} ( |S_c|^2 - D ),   S_c = sum_s w_s exp(+2 pi i (fr_c(x,s) - fr_c(x0,s)))
//          fr_c(x,s) = freq[c] tau[x][s] (the fp64 product, rounded) minus its nearest integer; the difference of the two fractions
//          fp64; its conversion to fp32, sincospif and everything after fp32:
//            Re S = fmaf(w_s, cos, Re S), Im S = fmaf(w_s, sin, Im S) over the stands of weight > 0 in ascending order
//            p_c = fmaf(Re S, Re S, Im S * Im S) - D;  acc += p_c over the channels in ascending order;  PSF = norm * acc
//   out    the residual f32[ngroup][4][npix], the component records [ngroup][niter][8] and the stats [ngroup][4]
//
// Decomposition: ONE kernel, clean_step_kernel, one work-group of CLN_PX = 256 threads per (tile of 256 pixels, channel group), one
// pixel per thread, launched niter + 2 times with step = 0 .. niter + 1 (the last launch with one tile per group: it only closes
// the books).  No work-group waits for another: launch boundaries order the iterations, and what one launch hands to the next goes
// through two ping-pong buffers (written at parity step & 1, read at the other), so nothing is read in the launch that writes it:
//   rec    i32[2][ngroup][ntile][8] = {pixel, I, XX, YY, Re, Im, 0, 0}: the tile's peak of the residual it has just written, its
//          four words with it (no work-group ever reads a pixel another one rewrites); pixel -1: the tile has no candidate
//   gstate i32[2][ngroup][4] = {stopped, the first peak |I(x_0)|, 0, 0}
// Launch 0 copies the image, fills the group's records with {-1, +0 ..} and leaves the first peak records.  Launch step >= 1, for
// iteration k = step - 1:
//   0. a group that has stopped returns at once (a uniform branch on gstate, which the launch before wrote)
//   1. every work-group of the group reduces the group's ntile records, all to the same winner: the key (|I|, pixel) is a total
//      order (larger |I| first, then the lower pixel), so the tree's shape changes nothing -- the strict > of an ascending scan
//   2. no winner: reason 2.  |I| <= max(threshold, fraction * |I(x_0)|): reason 1.  k = niter: reason 0.  Tile 0 writes the stats
//      and the stop; everyone returns.  Else tile 0 writes record k: C_j = gain * R_j(x_k)
//   3. per channel of the group: fr_c(x_k, s) into LDS (f64[nstand], thread s), then every thread forms S_c for its own pixel
//   4. R_j(x) = fmaf(-C_j, PSF, R_j(x)) for the thread's pixel, in or out of the window, and the tile's new peak record
// A pixel's residual words depend on its own column of tauT and the component list only.  No atomics, no scalar memory writes, no
// printf, no scratch; one owner per word.
//
// LDS (all dynamic): f64 fr0[nstand], f32 ka[256] and i32 ki[256] for the tree, f32 wl[nstand].  fr0[s] and wl[s] are read at the
// same address by all lanes (a broadcast, no conflict); the tree reads ka[tid], ka[tid + m]: consecutive dwords across a
// 32-lane group (ds_read_b32: banks mod 32 per group), so no two lanes of a group meet on a bank.
//
// clean.hip is compiled with -fno-slp-vectorize (Makefile), as the rest of the fine-channel family.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int CLN_PX = 256;             // pixels per work-group = threads per work-group
constexpr int CLN_REC = 8;              // 32-bit words per record

__host__ __device__ constexpr size_t clean_lds_bytes(int nstand) {
    return (size_t)nstand * (sizeof(double) + sizeof(float)) + (size_t)CLN_PX * (sizeof(float) + sizeof(int));
}

// the best of the work-group's 256 candidates (ka: |I| or -1 for none, ki: pixel) into slot 0; ends with a barrier
__device__ __forceinline__ void cln_best(float* ka, int* ki, int tid) {
    for (int m = CLN_PX / 2; m > 0; m >>= 1) {
        __syncthreads();
        if (tid < m) {
            const float a = ka[tid], b = ka[tid + m];
            const int ia = ki[tid], ib = ki[tid + m];
            if (b > a || (b == a && ib < ia)) {
                ka[tid] = b;
                ki[tid] = ib;
            }
        }
    }
    __syncthreads();
}

// grid (ntile, ngroup) for step <= niter, (1, ngroup) for step = niter + 1; CLN_PX threads; clean_lds_bytes(nstand) of dynamic LDS
__global__ __launch_bounds__(CLN_PX) void clean_step_kernel(const float* __restrict__ image, float* out, int* comp, int* stats,
                                                            const double* __restrict__ freq, const double* __restrict__ tauT,
                                                            const float* __restrict__ w, const uint8_t* __restrict__ mask, int* rec, int* gstate,
                                                            int nstand, int npix, int ntile, int nfavg, int niter, int step, float gain,
                                                            float threshold, float fraction, float norm, float dsum) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cln_lds[];
    double* fr0 = (double*)cln_lds;                     // [nstand]
    float* ka = (float*)(fr0 + nstand);                 // [CLN_PX]
    int* ki = (int*)(ka + CLN_PX);                      // [CLN_PX]
    float* wl = (float*)(ki + CLN_PX);                  // [nstand]
    const int tid = threadIdx.x, tile = blockIdx.x, g = blockIdx.y, ngroup = gridDim.y;
    const int x = tile * CLN_PX + tid, par = step & 1;
    const bool live = x < npix;
    float* res = out + (size_t)g * 4 * npix;
    int* gnow = gstate + ((size_t)par * ngroup + g) * 4;
    float r[4] = {0.f, 0.f, 0.f, 0.f};

    if (step == 0) {
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                r[j] = image[((size_t)g * 4 + j) * npix + x];
                res[(size_t)j * npix + x] = r[j];
            }
        }
        if (tile == 0) {
            for (int e = tid; e < niter * CLN_REC; e += CLN_PX) comp[(size_t)g * niter * CLN_REC + e] = (e % CLN_REC) ? 0 : -1;
            if (tid < 4) gnow[tid] = 0;
        }
    } else {
        const int* gprev = gstate + ((size_t)(par ^ 1) * ngroup + g) * 4;
        if (gprev[0]) {                                 // stopped: uniform over the group
            if (tile == 0 && tid < 4) gnow[tid] = gprev[tid];
            return;
        }
        // 1. the group's peak: the best of the tiles' records
        const int* rprev = rec + ((size_t)(par ^ 1) * ngroup + g) * ntile * CLN_REC;
        float ba = -1.f;
        int bi = 0x7fffffff;
        for (int t = tid; t < ntile; t += CLN_PX) {
            const int px = rprev[(size_t)t * CLN_REC];
            if (px >= 0) {
                const float a = fabsf(__int_as_float(rprev[(size_t)t * CLN_REC + 1]));
                if (a > ba) {                           // (ascending pixels: a tie keeps the lower one)
                    ba = a;
                    bi = px;
                }
            }
        }
        ka[tid] = ba;
        ki[tid] = bi;
        cln_best(ka, ki, tid);
        const bool won = ka[0] >= 0.f;
        const int xk = ki[0], k = step - 1;
        __syncthreads();                                // (ka, ki are written again below)
        const int* rk = rprev + (size_t)(won ? xk / CLN_PX : 0) * CLN_REC;
        const float ik = __int_as_float(rk[1]);
        const float peak0 = k == 0 ? fabsf(ik) : __int_as_float(gprev[1]);
        // 2. stop, or component k
        int reason = -1;
        if (!won) reason = 2;
        else if (fabsf(ik) <= fmaxf(threshold, fraction * peak0)) reason = 1;
        else if (k == niter) reason = 0;
        if (reason >= 0) {
            if (tile == 0 && tid == 0) {
                int* st = stats + (size_t)g * 4;
                st[0] = k;
                st[1] = reason;
                st[2] = won ? __float_as_int(fabsf(ik)) : 0;
                st[3] = 0;
                gnow[0] = 1;
                gnow[1] = __float_as_int(peak0);
                gnow[2] = gnow[3] = 0;
            }
            return;
        }
        float cj[4];
#pragma unroll
        for (int j = 0; j < 4; j++) cj[j] = gain * __int_as_float(rk[2 + j]);
        if (tile == 0 && tid == 0) {
            int* ck = comp + ((size_t)g * niter + k) * CLN_REC;
            ck[0] = xk;
            ck[1] = __float_as_int(ik);
#pragma unroll
            for (int j = 0; j < 4; j++) ck[2 + j] = __float_as_int(cj[j]);
            ck[6] = ck[7] = 0;
            gnow[0] = 0;
            gnow[1] = __float_as_int(peak0);
            gnow[2] = gnow[3] = 0;
        }
        // 3. the point-spread function of x_k at the thread's pixel
        for (int s = tid; s < nstand; s += CLN_PX) wl[s] = w[s];
        float acc = 0.f;
        for (int cc = 0; cc < nfavg; cc++) {
            const double f = freq[g * nfavg + cc];
            __syncthreads();                            // (the weights are there; the last channel's fractions are done with)
            for (int s = tid; s < nstand; s += CLN_PX) {
                double fr = 0.0;
                if (wl[s] != 0.f) {
                    const double turns = __dmul_rn(f, tauT[(size_t)s * npix + xk]);
                    fr = turns - rint(turns);
                }
                fr0[s] = fr;
            }
            __syncthreads();
            if (live) {
                float sr = 0.f, si = 0.f;
                for (int s = 0; s < nstand; s++) {
                    const float ws = wl[s];
                    if (ws != 0.f) {
                        const double turns = __dmul_rn(f, tauT[(size_t)s * npix + x]);
                        const float d = (float)((turns - rint(turns)) - fr0[s]);    // in [-1, 1]
                        float sn, cs;
                        sincospif(2.0f * d, &sn, &cs);
                        sr = __builtin_fmaf(ws, cs, sr);
                        si = __builtin_fmaf(ws, sn, si);
                    }
                }
                acc += __builtin_fmaf(sr, sr, si * si) - dsum;
            }
        }
        // 4. subtract
        if (live) {
            const float psf = norm * acc;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                r[j] = __builtin_fmaf(-cj[j], psf, res[(size_t)j * npix + x]);
                res[(size_t)j * npix + x] = r[j];
            }
        }
    }
    // the tile's peak of what it has just written
    const float iv = r[0] + r[1];
    const bool cand = live && mask[live ? x : 0] != 0 && __builtin_isfinite(iv);
    ka[tid] = cand ? fabsf(iv) : -1.f;
    ki[tid] = cand ? x : 0x7fffffff;
    cln_best(ka, ki, tid);
    int* rn = rec + (((size_t)par * ngroup + g) * ntile + tile) * CLN_REC;
    if (ka[0] < 0.f) {
        if (tid < CLN_REC) rn[tid] = tid ? 0 : -1;
    } else if (x == ki[0]) {
        rn[0] = x;
        rn[1] = __float_as_int(iv);
#pragma unroll
        for (int j = 0; j < 4; j++) rn[2 + j] = __float_as_int(r[j]);
        rn[6] = rn[7] = 0;
    }
}

}  // namespace xeng
