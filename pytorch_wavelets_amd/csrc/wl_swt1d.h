// The 1-D stationary (undecimated, a-trous) wavelet transform along the last axis, periodic, up to three levels per launch, on
// the wave tiles of wl_wave1d.h (the tile scheme, the piece accesses and the fetch are explained there).
//
//   * nothing is decimated, so every level of a periodic signal is periodic with the same period, and a lane holds the same V
//     positions at every level.  With i the register index and D the tap offset, both compile-time, the operand of an output
//     is source i + D of the lane (wl_wave1d_fetch): (L - 1) * d shuffled values per lane and level of dilation d, whatever V;
//   * a level of dilation d eats (L/2 - 1) * d positions of the tile on one side and (L/2) * d on the other (the analysis in
//     front and behind, the adjoint the other way round).  The core is the 64 * V - (L - 1) * (2^J - 1) positions that are
//     left, behind a head of (L/2 - 1)(2^J - 1) (analysis) or (L/2)(2^J - 1) (adjoint) positions; it is odd.  Each highpass is
//     stored from the level that made it, the lowpass at the end.
//
//   analysis, level of dilation d:  lo[p], hi[p] = scale * sum_t h0[t], h1[t] * in[p - (L/2 - 1) d + d t]      (afb1d_atrous,
//                                   stored = reversed taps; d = 1, 2, 4 for levels 1, 2, 3)
//   adjoint:                        out[m] = scale * sum_t (g0[t] lo[m + (L/2 - 1) d - d t] + g1[t] hi[m + (L/2 - 1) d - d t])
//                                   coarsest level first, a missing highpass = zeros
// The two kernels serve four directions: the transform (scale 1), its backward (adjoint, analysis taps, scale 1), the inverse
// (adjoint, synthesis taps, scale 1/2 per level) and the inverse's backward (analysis, synthesis taps, scale 1/2 per level).
#pragma once
#include "wl_wave1d.h"

// One analysis level of dilation D on the lane's registers: the sources M = i + (t - (L/2 - 1)) D in ascending order.
template <int L, int V, int D>
struct WlSwt1dFwdLevel {
    static const int LO = -(L / 2 - 1) * D, HI = V - 1 + (L / 2) * D;
    template <int M>
    static WL_DEV void step(const float (&in)[V], const float (&h0)[L], const float (&h1)[L], int lane, float (&lo)[V], float (&hi)[V]) {
        const float v = wl_wave1d_fetch<V, V, 0, M>(in, lane);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int dl = M - i + (L / 2 - 1) * D;        // = t * D
            if (dl >= 0 && dl % D == 0 && dl / D < L) {
                lo[i] = __builtin_fmaf(h0[dl / D], v, lo[i]);
                hi[i] = __builtin_fmaf(h1[dl / D], v, hi[i]);
            }
        }
    }
    template <int... S>
    static WL_DEV void steps(const float (&in)[V], const float (&h0)[L], const float (&h1)[L], int lane, float (&lo)[V], float (&hi)[V],
                             std::integer_sequence<int, S...>) {
        (step<LO + S>(in, h0, h1, lane, lo, hi), ...);
    }
    static WL_DEV void run(const float (&in)[V], const float (&h0)[L], const float (&h1)[L], int lane, float scale, float (&lo)[V], float (&hi)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) { lo[i] = 0.f; hi[i] = 0.f; }
        steps(in, h0, h1, lane, lo, hi, std::make_integer_sequence<int, HI - LO + 1>());
#pragma unroll
        for (int i = 0; i < V; ++i) { lo[i] *= scale; hi[i] *= scale; }
    }
};

// One level of the transpose: the sources M = i + (L/2 - 1 - t) D in ascending order, the lowpass term in front of the highpass term.
template <int L, int V, int D>
struct WlSwt1dAdjLevel {
    static const int LO = -(L / 2) * D, HI = V - 1 + (L / 2 - 1) * D;
    template <int M>
    static WL_DEV void step(const float (&lo)[V], const float (&hi)[V], const float (&g0)[L], const float (&g1)[L], int lane, float (&out)[V]) {
        const float vl = wl_wave1d_fetch<V, V, 0, M>(lo, lane);
        const float vh = wl_wave1d_fetch<V, V, 0, M>(hi, lane);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int dl = i - M + (L / 2 - 1) * D;        // = t * D
            if (dl >= 0 && dl % D == 0 && dl / D < L) {
                out[i] = __builtin_fmaf(g0[dl / D], vl, out[i]);
                out[i] = __builtin_fmaf(g1[dl / D], vh, out[i]);
            }
        }
    }
    template <int... S>
    static WL_DEV void steps(const float (&lo)[V], const float (&hi)[V], const float (&g0)[L], const float (&g1)[L], int lane, float (&out)[V],
                             std::integer_sequence<int, S...>) {
        (step<LO + S>(lo, hi, g0, g1, lane, out), ...);
    }
    static WL_DEV void run(const float (&lo)[V], const float (&hi)[V], const float (&g0)[L], const float (&g1)[L], int lane, float scale,
                           float (&out)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) out[i] = 0.f;
        steps(lo, hi, g0, g1, lane, out, std::make_integer_sequence<int, HI - LO + 1>());
#pragma unroll
        for (int i = 0; i < V; ++i) out[i] *= scale;
    }
};

template <typename T>
struct WlSwt1dFwdArgs {
    const T* x; T* lo; T* hi[WL_WAVE1D_MAXJ];      // hi[j]: level j + 1, nullptr = not stored
    const float* h0; const float* h1;
    int64_t rows, waves;                           // waves = rows * tiles
    int len, nlev, tiles, core, origin;
    float scale;                                   // per level
};

template <typename T, int L>
struct WlSwt1dFwd {
    typedef WlSwt1dFwdArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = wl_wave1d_wave(ctx);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int len = a.len, J = a.nlev;                 // (read in front of the tile arithmetic: DESIGN.md 4.28)
        WlWave1dTile t;
        wl_wave1d_tile<V>(a, ctx, w, (L / 2 - 1) * ((1 << a.nlev) - 1), t);
        const int lane = t.lane;
        float h0[L], h1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { h0[i] = a.h0[i]; h1[i] = a.h1[i]; }
        float r[V], lo[V], hi[V];
        wl_wave1d_load<T, V, V>(a.x + t.base, wl_pmod(t.p0, len), len, r, 0);
        WlSwt1dFwdLevel<L, V, 1>::run(r, h0, h1, lane, a.scale, lo, hi);
        if (a.hi[0]) wl_wave1d_store<T, V, V>(a.hi[0] + t.base, t.p0, t.c0, t.c1, hi, 0);
        if (J >= 2) {
            WlSwt1dFwdLevel<L, V, 2>::run(lo, h0, h1, lane, a.scale, r, hi);
            if (a.hi[1]) wl_wave1d_store<T, V, V>(a.hi[1] + t.base, t.p0, t.c0, t.c1, hi, 0);
            if (J >= 3) {
                WlSwt1dFwdLevel<L, V, 4>::run(r, h0, h1, lane, a.scale, lo, hi);
                if (a.hi[2]) wl_wave1d_store<T, V, V>(a.hi[2] + t.base, t.p0, t.c0, t.c1, hi, 0);
                wl_wave1d_store<T, V, V>(a.lo + t.base, t.p0, t.c0, t.c1, lo, 0);
            } else {
                wl_wave1d_store<T, V, V>(a.lo + t.base, t.p0, t.c0, t.c1, r, 0);
            }
        } else {
            wl_wave1d_store<T, V, V>(a.lo + t.base, t.p0, t.c0, t.c1, lo, 0);
        }
    }
};

template <typename T>
struct WlSwt1dAdjArgs {
    const T* lo; const T* hi[WL_WAVE1D_MAXJ]; T* y;// hi[j]: level j + 1, nullptr = zeros
    const float* g0; const float* g1;
    int64_t rows, waves;
    int len, nlev, tiles, core, origin;
    float scale;                                   // per level
};

template <typename T, int L>
struct WlSwt1dAdj {
    typedef WlSwt1dAdjArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    static WL_DEV void tile_of(const T* src, int64_t base, int s0, int len, float (&r)[V]) {
        if (src) wl_wave1d_load<T, V, V>(src + base, s0, len, r, 0);
        else {
#pragma unroll
            for (int i = 0; i < V; ++i) r[i] = 0.f;
        }
    }
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = wl_wave1d_wave(ctx);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int len = a.len, J = a.nlev;
        WlWave1dTile t;
        wl_wave1d_tile<V>(a, ctx, w, (L / 2) * ((1 << a.nlev) - 1), t);
        const int lane = t.lane;
        const int s0 = wl_pmod(t.p0, len);
        float g0[L], g1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { g0[i] = a.g0[i]; g1[i] = a.g1[i]; }
        float lo[V], hi[V], out[V];
        wl_wave1d_load<T, V, V>(a.lo + t.base, s0, len, lo, 0);
        if (J >= 3) {
            tile_of(a.hi[2], t.base, s0, len, hi);
            WlSwt1dAdjLevel<L, V, 4>::run(lo, hi, g0, g1, lane, a.scale, out);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = out[i];
        }
        if (J >= 2) {
            tile_of(a.hi[1], t.base, s0, len, hi);
            WlSwt1dAdjLevel<L, V, 2>::run(lo, hi, g0, g1, lane, a.scale, out);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = out[i];
        }
        tile_of(a.hi[0], t.base, s0, len, hi);
        WlSwt1dAdjLevel<L, V, 1>::run(lo, hi, g0, g1, lane, a.scale, out);
        wl_wave1d_store<T, V, V>(a.y + t.base, t.p0, t.c0, t.c1, out, 0);
    }
};
