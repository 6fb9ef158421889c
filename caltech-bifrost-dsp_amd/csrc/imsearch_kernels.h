// Dedispersed transient search of the images (xengImsearch*, imsearch.hip): per pixel and channel group a running baseline, per
// pixel and DM trial a dedispersed series and boxcars of 1, 2, 4 ... 2^(nwidth-1) integrations, one record plane per integration,
// streaming across calls with its state on the device.
//
// Contract (include/xeng.h, "Dedispersed transient search of the images"); pixels are the contiguous axis everywhere:
//   in     f32[ngroup][4][npix], words 0 and 1 of a group read: I = fl(XX + YY)
//   state  f32[IS_NSTATE][ngroup][npix]: c, m, v, g of the last complete baseline block and c, a, q of the running one
//   U      f32[S + 1][ngroup][npitch]: u of integration n at slot n mod (S + 1), NaN: "no u"
//   Z      f32[T + 1][ndm][npitch], T = 2^(nwidth-1) - 1: z of integration n at slot n mod (T + 1), NaN: "no z"
//   bk     i32[ndm][nusedp], gk i32[nusedp], wk f32[nusedp]: back-delays, indices and weights of the nused groups with weight != 0,
//          ascending, padded to nusedp = nused rounded up to IS_CHUNK with {0, gk[0], 0}
//   out    {f32 snr, i16 idm, i16 iw}[npix], one 8-byte store each
//
// Decomposition, two launches per integration.  A lane owns 4 consecutive pixels and moves them as one 16-byte access wherever the
// rows are aligned: always in U and Z (npitch is a multiple of 4), in the image and the state when npix is.  Otherwise it takes
// the same four words one by one, so no value depends on which it was.
//   imsearch_ingest_kernel   grid (pixel tiles, groups), one wave a work-group: the statistics chain of the contract for the
//                            integration, u (or NaN) into the U slot of n.
//   imsearch_search_kernel   <nwidth>: a work-group of 4 waves on one tile of IS_TILE pixels, wave w the trials d = w, w + 4 ...  Per
//                            trial: the T earlier z and the used groups' rows of U, in chunks of IS_CHUNK, are loaded ahead of
//                            the adds (two chunks in flight); z goes into the Z slot of n; the tree is built in registers
//                            (B_2w[n] = B_w[n] + the pairwise tree of the w integrations before those), each width scored, the
//                            best key (snr, -d, -iw) kept.  The four waves meet in LDS in wave order; wave 0 stores the records.
// What lies before the live range (before integration 0, before nstat, before the weights were set) is decided from indices the
// host passes, never from what the rings hold: a reset clears nothing.  "No u" and "no z" are NaN, every sum that touches one is
// NaN and a NaN score is not scored, so a boxcar is scored exactly when every z under it exists.  No atomics, no scratch; every
// word is a fixed function of its pixel's words.
//
// imsearch.hip is compiled with -fno-slp-vectorize (Makefile), as the other fine-channel code objects are.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace xeng {

constexpr int IS_TILE = 256;    // pixels per work-group: 64 lanes of 4
constexpr int IS_WAVES = 4;     // waves of the search kernel's work-group
constexpr int IS_CHUNK = 8;     // rows of U in flight ahead of their adds
constexpr int IS_MAX_NWIDTH = 6;
enum { IS_DC = 0, IS_DM = 1, IS_DV = 2, IS_DG = 3, IS_RC = 4, IS_RA = 5, IS_RQ = 6, IS_NSTATE = 7 };
constexpr float IS_RSQRT2 = 0.70710678118654752440f;

struct is_f4 {
    float e[4];
};

// four consecutive words of a row of n, from p0 (a multiple of 4, below n rounded up to 4): one 16-byte load when the row is
// aligned (vec), else one by one, the words past the row's end read as its last
__device__ __forceinline__ is_f4 is_load4(const float* __restrict__ row, int p0, int n, bool vec) {
    is_f4 r;
    if (vec) {
        const float4 v = *(const float4*)(row + p0);
        r.e[0] = v.x; r.e[1] = v.y; r.e[2] = v.z; r.e[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) r.e[i] = row[p0 + i < n ? p0 + i : n - 1];
    }
    return r;
}

__device__ __forceinline__ void is_store4(float* __restrict__ row, int p0, int n, bool vec, const is_f4& r) {
    if (vec) {
        *(float4*)(row + p0) = make_float4(r.e[0], r.e[1], r.e[2], r.e[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (p0 + i < n) row[p0 + i] = r.e[i];
    }
}

__device__ __forceinline__ is_f4 is_fill(float v) {
    is_f4 r;
#pragma unroll
    for (int i = 0; i < 4; i++) r.e[i] = v;
    return r;
}

// grid (ceil(npitch / IS_TILE), ngroup), 64 threads.  pos = n mod nstat, prev = (n >= nstat), uslot = n mod (S + 1),
// r_nstat = 1.0f / (float)nstat.
__global__ __launch_bounds__(64) void imsearch_ingest_kernel(const float* __restrict__ in, float* __restrict__ state, float* __restrict__ U, int npix,
                                                             int npitch, int ngroup, int nstat, float r_nstat, int pos, int prev, int uslot) {
    const int g = blockIdx.y, p0 = blockIdx.x * IS_TILE + threadIdx.x * 4;
    if (p0 >= npitch) return;
    const bool vec = (npix & 3) == 0;
    const size_t plane = (size_t)ngroup * npix;
    const float* w0 = in + (size_t)(4 * g) * npix;
    float* st = state + (size_t)g * npix;
    const float nan = __int_as_float(0x7fc00000), inf = __int_as_float(0x7f800000);
    const is_f4 xx = is_load4(w0, p0, npix, vec), yy = is_load4(w0 + npix, p0, npix, vec);
    const is_f4 dc = is_load4(st + IS_DC * plane, p0, npix, vec), dm = is_load4(st + IS_DM * plane, p0, npix, vec),
                dg = is_load4(st + IS_DG * plane, p0, npix, vec);
    is_f4 rc = is_fill(0.f), ra = is_fill(0.f), rq = is_fill(0.f);
    if (pos != 0) {                                 // (at a block's first integration the running words are set, not read)
        rc = is_load4(st + IS_RC * plane, p0, npix, vec);
        ra = is_load4(st + IS_RA * plane, p0, npix, vec);
        rq = is_load4(st + IS_RQ * plane, p0, npix, vec);
    }
    is_f4 u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float I = xx.e[i] + yy.e[i];
        if (pos == 0) rc.e[i] = I;
        const float delta = I - rc.e[i];
        ra.e[i] = ra.e[i] + delta;
        rq.e[i] = fmaf(delta, delta, rq.e[i]);
        u.e[i] = prev && dg.e[i] > 0.f ? ((I - dc.e[i]) - dm.e[i]) * dg.e[i] : nan;     // (g = 0 marks a block that is not valid)
    }
    *(float4*)(U + ((size_t)uslot * ngroup + g) * npitch + p0) = make_float4(u.e[0], u.e[1], u.e[2], u.e[3]);
    is_store4(st + IS_RC * plane, p0, npix, vec, rc);
    is_store4(st + IS_RA * plane, p0, npix, vec, ra);
    is_store4(st + IS_RQ * plane, p0, npix, vec, rq);
    if (pos + 1 == nstat) {
        is_f4 m, v, gg;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            m.e[i] = ra.e[i] * r_nstat;
            v.e[i] = fmaf(-m.e[i], m.e[i], rq.e[i] * r_nstat);
            gg.e[i] = v.e[i] > 0.f && v.e[i] < inf ? 1.0f / sqrtf(v.e[i]) : 0.f;
        }
        is_store4(st + IS_DC * plane, p0, npix, vec, rc);
        is_store4(st + IS_DM * plane, p0, npix, vec, m);
        is_store4(st + IS_DV * plane, p0, npix, vec, v);
        is_store4(st + IS_DG * plane, p0, npix, vec, gg);
    }
}

// z of the integration j before the current one, four pixels: the Z slot (zslot - j) mod T1; "no z" by index when j > zlive (the
// load is issued either way -- the slot exists -- and what it brings is dropped: a branch per row would put a wait in front of each)
__device__ __forceinline__ is_f4 is_zload(const float* __restrict__ Zd, size_t zstride, int zslot, int T1, int zlive, int j) {
    int s = zslot - j;
    s += s < 0 ? T1 : 0;
    const is_f4 v = is_load4(Zd + (size_t)s * zstride, 0, 4, true);
    return j > zlive ? is_fill(__int_as_float(0x7fc00000)) : v;
}

// IS_CHUNK rows of U from the k0-th group in use on: the row of integration n - b at slot (uslot - b) mod (S + 1); "no u" by index
// when that integration has no block before it (its slot was not written since the reset; loaded and dropped, as above).  The
// tables are padded to whole chunks with entries that name a row that exists, so a chunk's table words come in two scalar loads
// and its rows are requested back to back.
__device__ __forceinline__ void is_uload(is_f4* v, const float* __restrict__ Up, const int* __restrict__ bd, const int* __restrict__ gk, int k0,
                                         size_t npitch, int ngroup, int S, int n, int nstat, int uslot) {
    int b[IS_CHUNK], g[IS_CHUNK];
#pragma unroll
    for (int i = 0; i < IS_CHUNK; i++) {
        b[i] = bd[k0 + i];
        g[i] = gk[k0 + i];
    }
#pragma unroll
    for (int i = 0; i < IS_CHUNK; i++) {
        int s = uslot - b[i];
        s += s < 0 ? S + 1 : 0;
        const is_f4 u = is_load4(Up + ((size_t)s * ngroup + g[i]) * npitch, 0, 4, true);
        v[i] = n - b[i] >= nstat ? u : is_fill(__int_as_float(0x7fc00000));
    }
}

// z = fl(z + fl(w * u)) over the chunk's groups in ascending order; the padding of the last chunk is left out
__device__ __forceinline__ void is_uadd(is_f4& z, const is_f4* v, const float* __restrict__ wk, int k0, int nused) {
    float w[IS_CHUNK];
#pragma unroll
    for (int i = 0; i < IS_CHUNK; i++) w[i] = wk[k0 + i];
#pragma unroll
    for (int i = 0; i < IS_CHUNK; i++)
        if (k0 + i < nused) {
#pragma unroll
            for (int e = 0; e < 4; e++) z.e[e] = z.e[e] + w[i] * v[i].e[e];
        }
}

// a wave meets its keys in ascending (d, iw): the first scored, then strictly greater
__device__ __forceinline__ void is_score(float* bs, int* bkey, const is_f4& B, float kappa, float rho, int key) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float s = (B.e[e] * kappa) * rho;
        if (s == s && (bkey[e] < 0 || s > bs[e])) {
            bs[e] = s;
            bkey[e] = key;
        }
    }
}

// B_2W[n] = B_W[n] + the pairwise tree over the W integrations n - W ... n - 2W + 1 (t[0] ... t[W - 1]), the newer half the left
// operand at every level; t is used up
template <int W>
__device__ __forceinline__ void is_widen(is_f4& B, is_f4* t) {
#pragma unroll
    for (int h = 1; h < W; h *= 2)
#pragma unroll
        for (int i = 0; i < W; i += 2 * h)
#pragma unroll
            for (int e = 0; e < 4; e++) t[i].e[e] = t[i].e[e] + t[i + h].e[e];
#pragma unroll
    for (int e = 0; e < 4; e++) B.e[e] = B.e[e] + t[0].e[e];
}

__device__ __forceinline__ float is_rho(int iw) {      // (float)2^(-iw/2)
    return (iw & 1 ? IS_RSQRT2 : 1.0f) * (1.0f / (float)(1 << (iw >> 1)));
}

// grid ceil(npix / IS_TILE), 256 threads; NW = nwidth.  n = integrations since the reset before this one (clamped to INT_MAX: only
// its order against nstat + S counts), uslot = n mod (S + 1), zslot = n mod (T + 1), zlive = min(n - n_w, T): how many earlier z
// count.  A key is d * 8 + iw: smaller d, then smaller iw.  Per trial every load is issued before the first add: the T earlier z
// and two chunks of U rows, a third chunk while the first is added (one wave per SIMD at 65 536 pixels: latency is all there is to
// hide, and registers are free).
template <int NW>
__global__ __launch_bounds__(64 * IS_WAVES) void imsearch_search_kernel(const float* __restrict__ U, float* __restrict__ Z, const int* __restrict__ bk,
                                                                        const int* __restrict__ gk, const float* __restrict__ wk,
                                                                        float2* __restrict__ out, int npix, int npitch, int ngroup, int ndm, int nused,
                                                                        int nstat, int S, int n, int uslot, int zslot, int zlive, float kappa) {
    __shared__ float4 is_red[(IS_WAVES - 1) * 2 * 64];
    constexpr int T1 = 1 << (NW - 1), T = T1 - 1;
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int p0 = blockIdx.x * IS_TILE + lane * 4;
    const int pc = p0 < npitch ? p0 : npitch - 4;   // (idle lanes read what a live lane reads and store nothing)
    const size_t zstride = (size_t)ndm * npitch;
    const int nusedp = (nused + IS_CHUNK - 1) / IS_CHUNK * IS_CHUNK;
    const float* Up = U + pc;
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    int bkey[4] = {-1, -1, -1, -1};

    for (int d = j; d < ndm; d += IS_WAVES) {
        const int* bd = bk + (size_t)d * nusedp;
        float* Zd = Z + (size_t)d * npitch + pc;
        is_f4 zt[T > 0 ? T : 1];                    // z of n - 1 ... n - T
#pragma unroll
        for (int i = 0; i < T; i++) zt[i] = is_zload(Zd, zstride, zslot, T1, zlive, i + 1);
        is_f4 va[IS_CHUNK], vb[IS_CHUNK];
        is_f4 z = is_fill(0.f);
        is_uload(va, Up, bd, gk, 0, npitch, ngroup, S, n, nstat, uslot);
        for (int k0 = 0;;) {
            if (k0 + IS_CHUNK < nused) is_uload(vb, Up, bd, gk, k0 + IS_CHUNK, npitch, ngroup, S, n, nstat, uslot);
            is_uadd(z, va, wk, k0, nused);
            k0 += IS_CHUNK;
            if (k0 >= nused) break;
            if (k0 + IS_CHUNK < nused) is_uload(va, Up, bd, gk, k0 + IS_CHUNK, npitch, ngroup, S, n, nstat, uslot);
            is_uadd(z, vb, wk, k0, nused);
            k0 += IS_CHUNK;
            if (k0 >= nused) break;
        }
        if (p0 < npitch) *(float4*)(Zd + (size_t)zslot * zstride) = make_float4(z.e[0], z.e[1], z.e[2], z.e[3]);

        is_f4 B = z;
        is_score(bs, bkey, B, kappa, 1.0f, d * 8);
        if constexpr (NW > 1) {
            is_widen<1>(B, zt);
            is_score(bs, bkey, B, kappa, is_rho(1), d * 8 + 1);
        }
        if constexpr (NW > 2) {
            is_widen<2>(B, zt + 1);
            is_score(bs, bkey, B, kappa, is_rho(2), d * 8 + 2);
        }
        if constexpr (NW > 3) {
            is_widen<4>(B, zt + 3);
            is_score(bs, bkey, B, kappa, is_rho(3), d * 8 + 3);
        }
        if constexpr (NW > 4) {
            is_widen<8>(B, zt + 7);
            is_score(bs, bkey, B, kappa, is_rho(4), d * 8 + 4);
        }
        if constexpr (NW > 5) {
            is_widen<16>(B, zt + 15);
            is_score(bs, bkey, B, kappa, is_rho(5), d * 8 + 5);
        }
    }

    if (j) {
        is_red[((j - 1) * 2 + 0) * 64 + lane] = make_float4(bs[0], bs[1], bs[2], bs[3]);
        is_red[((j - 1) * 2 + 1) * 64 + lane] =
            make_float4(__int_as_float(bkey[0]), __int_as_float(bkey[1]), __int_as_float(bkey[2]), __int_as_float(bkey[3]));
    }
    __syncthreads();
    if (j || p0 >= npix) return;
#pragma unroll
    for (int k = 0; k < IS_WAVES - 1; k++) {
        const float4 s4 = is_red[(k * 2 + 0) * 64 + lane], k4 = is_red[(k * 2 + 1) * 64 + lane];
        const float os[4] = {s4.x, s4.y, s4.z, s4.w};
        const int ok[4] = {__float_as_int(k4.x), __float_as_int(k4.y), __float_as_int(k4.z), __float_as_int(k4.w)};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (ok[e] >= 0 && (bkey[e] < 0 || os[e] > bs[e] || (os[e] == bs[e] && ok[e] < bkey[e]))) {
                bs[e] = os[e];
                bkey[e] = ok[e];
            }
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (p0 + e < npix) {                        // {snr, i16 idm, i16 iw}: idm in the low half of the second word
            const int rec = bkey[e] < 0 ? -1 : ((bkey[e] >> 3) & 0xffff) | ((bkey[e] & 7) << 16);
            out[p0 + e] = make_float2(bs[e], __int_as_float(rec));
        }
}

}  // namespace xeng
