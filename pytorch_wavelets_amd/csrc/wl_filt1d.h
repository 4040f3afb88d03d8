// Single-axis building blocks: one strided / dilated correlation with boundary extension along ANY axis of a dense
// tensor, and the 1-D two-channel synthesis bank.  They carry the parts of the reference's API that are not the fused
// 2-D hot path: DWT1DForward / DWT1DInverse (dwt/transform1d.py:7-115, AFB1D / SFB1D dwt/lowlevel.py:368-424, :697-743),
// the stationary transform's a-trous bank (afb1d_atrous, dwt/lowlevel.py:175-223), and the DTCWT primitives the
// reference exposes and tests on their own (colfilter ... rowifilt, dtcwt/lowlevel.py:70-239).
//
//   correlation:  y[o, q0 + qs*k, i] = sum_{t<nt} h[t0 + ts*t] * ext(x[o, :, i], start + step*k + dstep*t),  k in [0,K)
//                 x is (outer, n, inner) dense, y is (outer, ny, inner) dense; optionally a second tap set / output
//                 (the lo and hi channel of a filter bank share the samples).
//   synthesis:    full[m] = sum_k lo[k] g0[m-2k] + hi[k] g1[m-2k];  y[p] = full[p + L - 2]                (crop), or
//                 z[m] = full[m] + [m < L-2] full[m + 2K],  y[p] = z[(p + L/2 - 1) mod 2K]                (periodization)
// One thread per output sample, samples read straight from global memory (consecutive lanes read consecutive
// addresses along the fastest axis; the L-fold re-reads hit L1/L2).  These are API-completeness kernels, not the
// roofline path.
#pragma once
#include "wl_common.h"

#define WL_EXT_REPLICATE 5   // edge replication (only the stationary transform's 'replicate' padding uses it)
#define WL_EXT_PER_FOLD1 6   // periodization as the reference evaluates it (roll, zero-padded convolution, ONE fold of the
                             // wrapped tail: dwt/lowlevel.py:134-150) - differs from the circular form (WL_EXT_PER) when the
                             // signal is shorter than the filter.  step 2, tap_step 1, start = 1 - ntaps.

WL_HD int wl_ext_any(int i, int n, int ext) {
    if (ext == WL_EXT_REPLICATE) return i < 0 ? 0 : (i >= n ? n - 1 : i);
    if (n >= (1 << 30) && (unsigned)i >= (unsigned)n && (ext == WL_EXT_SYM || ext == WL_EXT_REFL)) {
        // the period of the fold, 2n (2n - 2), is no int: wl_ext would wrap it.  No launcher bounds the length of a single axis
        // (the level-by-level route of every 1-D analysis above 2^30 samples ends here; wl_corr1d bounds the positions it hands in)
        const int s = ext == WL_EXT_SYM ? 1 : 0;
        const int64_t p = 2 * (int64_t)n - 2 + 2 * s;
        int64_t j = i % p;
        if (j < 0) j += p;
        return (int)(j < n ? j : p - s - j);
    }
    return wl_ext(i, n, ext);
}

template <typename T>
struct WlCorr1dArgs {
    typedef typename WlAcc<T>::type A;
    const T* x; T* y0; T* y1;          // y1 may be nullptr
    const A* h0; const A* h1;
    int64_t outer, inner, y_outer_stride;   // y index = o * y_outer_stride + q * inner + i
    int n, K, nt, t0, ts, start, step, dstep, ext, q0, qs;
};

template <typename T>
struct WlCorr1d {
    typedef WlCorr1dArgs<T> Args;
    typedef typename WlAcc<T>::type A;
    static const int kThreads = 256;
    static const int kMinWaves = 1;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t per = (int64_t)a.K * a.inner;
        const int64_t idx = ctx.bid * kThreads + ctx.tid;
        if (idx >= a.outer * per) return;
        int64_t o, i;
        int k;
        if (a.outer * per < (1LL << 31)) {       // (uniform) 32-bit index arithmetic: a 64-bit division costs ~40 instructions
            const unsigned u = (unsigned)idx, up = (unsigned)per, ui = (unsigned)a.inner;
            const unsigned uo = u / up, ur = u - uo * up;
            const unsigned uk = ui == 1 ? ur : ur / ui;
            o = uo; k = (int)uk; i = ur - uk * ui;
        } else {
            o = idx / per;
            const int64_t rem = idx - o * per;
            k = (int)(rem / a.inner);
            i = rem - (int64_t)k * a.inner;
        }
        const T* xp = a.x + o * a.n * a.inner + i;
        A acc0 = 0, acc1 = 0;
        const int p0 = a.start + a.step * k;
        if (a.ext != WL_EXT_PER_FOLD1 && a.dstep > 0 && p0 >= 0 && p0 + a.dstep * (a.nt - 1) < a.n) {
            // interior: every tap meets a sample of the signal (all but the first / last few outputs of a row): no extension
            // arithmetic per tap
            const T* xq = xp + (int64_t)p0 * a.inner;
            const int64_t st = (int64_t)a.dstep * a.inner;
            const A* h0 = a.h0 + a.t0;
            const A* h1 = a.h1 + a.t0;
            if (a.y1) {
                for (int t = 0; t < a.nt; ++t) {
                    const A v = (A)xq[t * st];
                    acc0 += h0[a.ts * t] * v;
                    acc1 += h1[a.ts * t] * v;
                }
            } else {
                for (int t = 0; t < a.nt; ++t) acc0 += h0[a.ts * t] * (A)xq[t * st];
            }
        } else if (a.ext == WL_EXT_PER_FOLD1) {
            const int ne = a.n + (a.n & 1), L2 = a.nt / 2;
            const int nfold = k < (L2 < ne / 2 ? L2 : ne / 2) ? 2 : 1;
            for (int f = 0; f < nfold; ++f)
                for (int t = 0; t < a.nt; ++t) {
                    const int s = wl_per_rolled_src(p0 + t + f * ne, a.n, L2);
                    if (s < 0) continue;
                    const A v = (A)xp[(int64_t)s * a.inner];
                    acc0 += a.h0[a.t0 + a.ts * t] * v;
                    if (a.y1) acc1 += a.h1[a.t0 + a.ts * t] * v;
                }
        } else
        for (int t = 0; t < a.nt; ++t) {
            const int s = wl_ext_any(p0 + a.dstep * t, a.n, a.ext);
            if (s < 0) continue;
            const A v = (A)xp[(int64_t)s * a.inner];
            acc0 += a.h0[a.t0 + a.ts * t] * v;
            if (a.y1) acc1 += a.h1[a.t0 + a.ts * t] * v;
        }
        const int64_t yo = o * a.y_outer_stride + (int64_t)(a.q0 + a.qs * k) * a.inner + i;
        a.y0[yo] = (T)acc0;
        if (a.y1) a.y1[yo] = (T)acc1;
    }
};

// The transpose of the unit-step correlation above (two tap sets): with y_b[k] = sum_t h_b[t] * ext(x, start + k + dstep*t),
// k in [0,K),
//     dx[m] = scale * sum_{e : ext(e) == m, start <= e <= start + K-1 + dstep*(nt-1)} z[e]
//     z[e]  = sum_b sum_t h_b[t] * y_b[e - start - dstep*t]                       (y_b zero outside [0,K))
// One thread per dx sample.  The extended positions e that the rule maps onto m are arithmetic progressions, walked with as
// many folds as the pad is long: zero {m}; periodic m + n q; symmetric m + 2n q and -1-m + 2n q; reflect +-m + (2n-2) q (the two
// coincide at m = 0 and m = n-1: counted once); replicate every e <= 0 for m = 0 and every e >= n-1 for m = n-1.
// This is what autograd derives upstream for afb1d_atrous (dwt/lowlevel.py:175-223: mypad + conv2d), for any axis, dilation
// and K; the fused level kernel (wl_iswt2d.h) hands over what it declines.
template <typename T>
struct WlCorr1dAdjArgs {
    typedef typename WlAcc<T>::type A;
    const T* y0; const T* y1;          // (outer, K, inner) through their outer strides; y1 may be nullptr
    T* dx;                             // (outer, n, inner) dense
    const A* h0; const A* h1;
    A scale;
    int64_t outer, inner, y0_os, y1_os;
    int n, K, nt, start, dstep, ext;
};

template <typename T>
struct WlCorr1dAdj {
    typedef WlCorr1dAdjArgs<T> Args;
    typedef typename WlAcc<T>::type A;
    static const int kThreads = 256;
    static const int kMinWaves = 1;
    static WL_DEV A z(const Args& a, const T* p0, const T* p1, int e) {
        A acc = 0;
        for (int t = 0; t < a.nt; ++t) {
            const int k = e - a.start - a.dstep * t;
            if ((unsigned)k >= (unsigned)a.K) continue;
            acc += a.h0[t] * (A)p0[(int64_t)k * a.inner];
            if (p1) acc += a.h1[t] * (A)p1[(int64_t)k * a.inner];
        }
        return acc;
    }
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t per = (int64_t)a.n * a.inner;
        const int64_t idx = ctx.bid * kThreads + ctx.tid;
        if (idx >= a.outer * per) return;
        const int64_t o = idx / per;
        const int64_t rem = idx - o * per;
        const int m = (int)(rem / a.inner);
        const int64_t i = rem - (int64_t)m * a.inner;
        const T* p0 = a.y0 + o * a.y0_os + i;
        const T* p1 = a.y1 ? a.y1 + o * a.y1_os + i : nullptr;
        const int elo = a.start, ehi = a.start + a.K - 1 + a.dstep * (a.nt - 1);
        // up to two progressions (first, step) up to ehi, or one run [first[0], last] of consecutive positions
        int nf = 1, step = 0, first[2] = {m, 0}, last = m;
        const int n = a.n;
        switch (a.ext) {
            case WL_EXT_PERIODIC: step = n; break;
            case WL_EXT_SYM: step = 2 * n; first[1] = -1 - m; nf = 2; break;
            case WL_EXT_REFL:
                if (n == 1) { first[0] = elo; last = ehi; }
                else { step = 2 * n - 2; first[1] = -m; nf = (m == 0 || m == n - 1) ? 1 : 2; }
                break;
            case WL_EXT_REPLICATE:
                if (m == 0) first[0] = elo;
                if (m == n - 1) last = ehi;
                break;
            default: break;   // zero: the sample itself
        }
        A acc = 0;
        if (step) {
            for (int f = 0; f < nf; ++f)
                for (int e = elo + wl_pmod(first[f] - elo, step); e <= ehi; e += step) acc += z(a, p0, p1, e);
        } else {
            const int e0 = first[0] < elo ? elo : first[0], e1 = last > ehi ? ehi : last;
            for (int e = e0; e <= e1; ++e) acc += z(a, p0, p1, e);
        }
        a.dx[idx] = (T)(a.scale * acc);
    }
};

template <typename T>
struct WlSynth1dArgs {
    typedef typename WlAcc<T>::type A;
    const T* lo; const T* hi; T* y;    // lo / hi: (outer, K, inner); hi may be nullptr (zeros); y: (outer, ny, inner)
    const A* g0; const A* g1;
    int64_t outer, inner;
    int K, ny, L, circ;
};

template <typename T>
struct WlSynth1d {
    typedef WlSynth1dArgs<T> Args;
    typedef typename WlAcc<T>::type A;
    static const int kThreads = 256;
    static const int kMinWaves = 1;
    static WL_DEV A full(const Args& a, const T* lp, const T* hp, int m) {   // full[m] of the header
        A acc = 0;
        int k1 = m / 2;
        if (k1 > a.K - 1) k1 = a.K - 1;
        int k0 = (m - a.L + 2) / 2;          // ceil((m - L + 1) / 2) for m - L + 1 >= 0
        if (m - a.L + 1 < 0) k0 = 0;
        for (int k = k0; k <= k1; ++k) {
            const int t = m - 2 * k;
            if (t < 0 || t >= a.L) continue;
            acc += a.g0[t] * (A)lp[(int64_t)k * a.inner];
            if (hp) acc += a.g1[t] * (A)hp[(int64_t)k * a.inner];
        }
        return acc;
    }
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t per = (int64_t)a.ny * a.inner;
        const int64_t idx = ctx.bid * kThreads + ctx.tid;
        if (idx >= a.outer * per) return;
        int64_t o, i;
        int p;
        if (a.outer * per < (1LL << 31)) {       // (uniform) 32-bit index arithmetic
            const unsigned u = (unsigned)idx, up = (unsigned)per, ui = (unsigned)a.inner;
            const unsigned uo = u / up, ur = u - uo * up;
            const unsigned uq = ui == 1 ? ur : ur / ui;
            o = uo; p = (int)uq; i = ur - uq * ui;
        } else {
            o = idx / per;
            const int64_t rem = idx - o * per;
            p = (int)(rem / a.inner);
            i = rem - (int64_t)p * a.inner;
        }
        const T* lp = a.lo + o * a.K * a.inner + i;
        const T* hp = a.hi ? a.hi + o * a.K * a.inner + i : nullptr;
        A v;
        if (a.circ) {
            const int N = 2 * a.K;
            const int m = (p + (a.L / 2 - 1 < 2 * N ? a.L / 2 - 1 : 0)) % N;   // the reference's roll(): identity from 2N on
            v = full(a, lp, hp, m);
            if (m < a.L - 2) v += full(a, lp, hp, m + N);
        } else {
            v = full(a, lp, hp, p + a.L - 2);
        }
        a.y[idx] = (T)v;
    }
};
