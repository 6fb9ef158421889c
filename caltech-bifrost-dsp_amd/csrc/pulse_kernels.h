// Boxcar single-pulse search of the dedispersed beams (xengPulse*, pulse.hip): per series a running baseline, boxcars of widths
// 1, 2, 4 ... 2^(nwidth-1) windows and the peak of the call, streaming across calls with its state on the device.
//
// Contract (include/xeng.h, "Boxcar single-pulse search of the dedispersed beams"); a series is one (pair, trial), nser = npair*ndm:
//   in     f32[nc][nser][NPROD], z = word 0 (NPROD = 1) or word 0 + word 1 (NPROD = 4)
//   state  f32[PS_NSTATE][nser]: c, m, v, g of the last complete baseline block and c, a, q of the running one
//   tail   f32[L][nser], L = T + nwin, T = 2^(nwidth-1) - 1: y of window n at slot n mod L (NaN: the window has no y)
//   rho    f32[nwidth]: (float)2^(-iw/2)
//   out    {f32 snr, i32 n_call, i32 iw, f32 B}[nser], one 16-byte store each
//
// Decomposition, one launch per call: a work-group of 4 waves takes 64 neighbouring series, lane = series.  LDS holds
// Y[T + nc][64] (row r is window n0 - T + r) and G[nc][64] (g of the block before each window's).
//   1. wave 0 walks the call's windows in order: the statistics chain of the contract, y into Y, g into G and into the tail
//      ring; waves 1-3 bring the T windows before the call from the ring into Y.  A window before nstat (before window 0 too)
//      has no y BY INDEX: what the ring holds there is never read, so a reset clears nothing.
//   2. the tree in place, level by level: at width w the rows of a series fall into w residue classes mod w, and one thread
//      walks a class downwards, Y[r] = Y[r] + Y[r - w] -- it reads r - w before anybody writes it, so a level needs one
//      barrier.  On the way it scores the B_w it reads; the widest level is scored in a pass of its own.
//   3. the four threads of a series meet in LDS; the key is (snr, -n, -iw).
// "No y" is a NaN in Y: every boxcar that touches it sums to NaN, a NaN score is not scored, and so a boxcar is scored exactly
// when all its windows have a y.  No atomics; every value is a fixed function of the series.
//
// pulse.hip is compiled with -fno-slp-vectorize (Makefile), as the other fine-channel code objects are.
#pragma once
#include <hip/hip_runtime.h>

namespace xeng {

constexpr int PS_SERIES = 64;   // series per work-group = lanes of a wave
constexpr int PS_WAVES = 4;
enum { PS_DC = 0, PS_DM = 1, PS_DV = 2, PS_DG = 3, PS_RC = 4, PS_RA = 5, PS_RQ = 6, PS_NSTATE = 7 };

struct PulseBest {
    float snr, B;
    int n, iw;                  // n < 0: nothing scored yet
};

// larger snr, then smaller n, then smaller iw; a NaN score never enters
__device__ __forceinline__ void ps_take(PulseBest& b, float snr, float B, int n, int iw) {
    if (snr != snr) return;
    const bool better = b.n < 0 || snr > b.snr || (snr == b.snr && (n < b.n || (n == b.n && iw < b.iw)));
    if (better) {
        b.snr = snr; b.B = B; b.n = n; b.iw = iw;
    }
}

__device__ __forceinline__ int ps_slot(int head, int rel, int L) {     // slot of the window `rel` after the one at `head`, -L <= rel < L
    int s = head + rel;
    s += s < 0 ? L : 0;
    s -= s >= L ? L : 0;
    return s;
}

// grid ceil(nser / 64), 256 threads, (max(T + 2 nc, 16)) * 64 floats of dynamic LDS.  n0 = windows since the reset before this
// call (clamped to 2^30: only its order against nstat + T counts), pos0 = that count mod nstat, head = that count mod L,
// r_nstat = 1.0f / (float)nstat.
template <int NPROD>
__global__ __launch_bounds__(256) void pulse_search_kernel(const float* __restrict__ in, float* __restrict__ state, float* __restrict__ tail,
                                                           const float* __restrict__ rho, float4* __restrict__ out, int nser, int nc, int nwidth,
                                                           int nstat, float r_nstat, int L, int head, int n0, int pos0) {
#pragma clang fp contract(off)
    extern __shared__ float ps_lds[];
    const int lane = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int T = (1 << (nwidth - 1)) - 1, R = T + nc;
    float* Y = ps_lds + lane;                       // Y[r * 64]
    float* G = ps_lds + (size_t)R * PS_SERIES + lane;
    const int s = blockIdx.x * PS_SERIES + lane;
    const bool live = s < nser;
    const int sc = live ? s : nser - 1;             // (idle lanes read the input and the ring where a live lane does and store nothing)
    const float nan = __int_as_float(0x7fc00000);

    if (j == 0) {
        bool prev = n0 >= nstat;                    // the window's block has a block before it
        int pos = pos0;
        // (an idle lane takes no state: a clamped read would take the words the last live lane writes below, with no barrier between)
        float dc = 0.f, dm = 0.f, dv = 0.f, dg = 0.f, rc = 0.f, ra = 0.f, rq = 0.f;
        if (live) {
            dc = state[(size_t)PS_DC * nser + s]; dm = state[(size_t)PS_DM * nser + s]; dv = state[(size_t)PS_DV * nser + s];
            dg = state[(size_t)PS_DG * nser + s];
            rc = state[(size_t)PS_RC * nser + s]; ra = state[(size_t)PS_RA * nser + s]; rq = state[(size_t)PS_RQ * nser + s];
        }
        bool ok = prev && dv > 0.f && dv < __int_as_float(0x7f800000);
#pragma unroll 4
        for (int i = 0; i < nc; i++) {
            float z;
            if constexpr (NPROD == 4) {
                const float4 x = ((const float4*)in)[(size_t)i * nser + sc];
                z = x.x + x.y;
            } else {
                z = in[(size_t)i * nser + sc];
            }
            if (pos == 0) {
                rc = z; ra = 0.f; rq = 0.f;
            }
            const float delta = z - rc;
            ra = ra + delta;
            rq = fmaf(delta, delta, rq);
            const float y = ok ? (z - dc) - dm : nan;
            Y[(size_t)(T + i) * PS_SERIES] = y;
            G[(size_t)i * PS_SERIES] = dg;
            if (live && i >= nc - T) tail[(size_t)ps_slot(head, i, L) * nser + s] = y;
            if (++pos == nstat) {
                dm = ra * r_nstat;
                dv = fmaf(-dm, dm, rq * r_nstat);
                dc = rc;
                ok = dv > 0.f && dv < __int_as_float(0x7f800000);
                dg = ok ? 1.0f / sqrtf(dv) : 0.f;
                pos = 0;
            }
        }
        if (live) {
            state[(size_t)PS_DC * nser + s] = dc; state[(size_t)PS_DM * nser + s] = dm; state[(size_t)PS_DV * nser + s] = dv;
            state[(size_t)PS_DG * nser + s] = dg;
            state[(size_t)PS_RC * nser + s] = rc; state[(size_t)PS_RA * nser + s] = ra; state[(size_t)PS_RQ * nser + s] = rq;
        }
    } else {
        for (int r = j - 1; r < T; r += PS_WAVES - 1) {
            const int rel = r - T;                  // window n0 + rel
            const bool has = n0 + rel >= nstat;
            const float v = tail[(size_t)ps_slot(head, rel, L) * nser + sc];
            Y[(size_t)r * PS_SERIES] = has ? v : nan;
        }
    }
    __syncthreads();

    PulseBest best = {0.f, 0.f, -1, -1};
    for (int iw = 0; iw + 1 < nwidth; iw++) {
        const int w = 1 << iw;
        const float rh = rho[iw];
        for (int cls = j; cls < w; cls += PS_WAVES) {
            if (R - 1 < cls) break;
            int r = cls + (((R - 1 - cls) >> iw) << iw);            // the class's topmost row
            float cur = Y[(size_t)r * PS_SERIES];
            for (; r >= w; r -= w) {
                if (r >= T) ps_take(best, (cur * G[(size_t)(r - T) * PS_SERIES]) * rh, cur, r - T, iw);
                const float old = Y[(size_t)(r - w) * PS_SERIES];
                Y[(size_t)r * PS_SERIES] = cur + old;
                cur = old;
            }
        }
        __syncthreads();
    }
    {
        const int iw = nwidth - 1;
        const float rh = rho[iw];
        for (int r = T + j; r < R; r += PS_WAVES) {
            const float B = Y[(size_t)r * PS_SERIES];
            ps_take(best, (B * G[(size_t)(r - T) * PS_SERIES]) * rh, B, r - T, iw);
        }
    }
    __syncthreads();
    float4* red = (float4*)ps_lds;                  // [3][64]
    if (j) red[(j - 1) * PS_SERIES + lane] = make_float4(best.snr, __int_as_float(best.n), __int_as_float(best.iw), best.B);
    __syncthreads();
    if (j || !live) return;
#pragma unroll
    for (int k = 0; k < PS_WAVES - 1; k++) {
        const float4 o = red[k * PS_SERIES + lane];
        const int n = __float_as_int(o.y);
        if (n >= 0) ps_take(best, o.x, o.w, n, __float_as_int(o.z));
    }
    out[s] = make_float4(best.snr, __int_as_float(best.n), __int_as_float(best.iw), best.B);
}

}  // namespace xeng
