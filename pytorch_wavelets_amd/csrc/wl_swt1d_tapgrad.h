// The gradient of the 1-D stationary transform (wl_swt1d.h) with respect to its FILTER TAPS, periodic, up to three levels, in ONE
// launch on the wave tiles of wl_wave1d.h: no LDS, no barrier, no atomics.  One kernel serves both directions.
//
//   inputs: a signal s, a top v_J, highs w_1 .. w_J (a null pointer = zeros), taps k0 / k1, the per-level scale sigma; d_j = 2^(j-1)
//   the analysis chain   u_0 = s,   u_j = sigma A0_j(k0) u_{j-1}                              (WlSwt1dFwdLevel, its highpass unused)
//   the adjoint chain    v_{j-1} = sigma (A0_j(k0)^T v_j + A1_j(k1)^T w_j)                    (WlSwt1dAdjLevel, coarsest first)
//   c0[t] = sigma sum_j sum_p u_{j-1}[p + (t - (L/2 - 1)) d_j] v_j[p]
//   c1[t] = sigma sum_j sum_p u_{j-1}[p + (t - (L/2 - 1)) d_j] w_j[p]                         t = 0 .. L - 1
//   * the backward of the transform:  (s, v_J, w, k, sigma) = (x, dlo, dhi, h, 1)    -> (dh0, dh1)
//     the backward of the inverse:    (s, v_J, w, k, sigma) = (dx, lo, hi, g, 1/2)   -> (dg0, dg1)
//   * s, v_J and every w_j are loaded once; u_0 .. u_{J-1} stay fp32 in registers.  At level j the adjoint level first makes
//     v_{j-1} of (v_j, w_j) - level 1 makes none: v_0 is not wanted -, then v_j and w_j are zeroed outside the tile's core cut to
//     the row, [c0, c1), and correlated with u_{j-1}: the sources M = i + (t - (L/2 - 1)) d_j of u_{j-1} in ascending order,
//     each fetched ONCE (wl_wave1d_fetch), every term an explicit fused multiply-add into the lane's 2 L sums.  The cores
//     partition a row, so every (row, p, j) is counted exactly once;
//   * position p of level j needs u_{j-1} on [p - (L/2 - 1) d_j, p + (L/2) d_j] - that is where u_j is valid: (L/2 - 1)(2^j - 1)
//     positions behind the tile's start, (L/2)(2^j - 1) in front of its end - and v_j, which J - j adjoint levels leave valid
//     (L/2)(2^J - 2^j) behind the start and (L/2 - 1)(2^J - 2^j) in front of the end.  Over j = 1 .. J the larger of the two:
//         head = max((L/2 - 1)(2^J - 1), (L/2)(2^J - 2))     (level J's analysis, or level 1's adjoint chain)
//         tail = (L/2)(2^J - 1)                              (level J's analysis)
//     and the core is the 64 V - head - tail positions between (1024 - 63 - 70 = 891 at 20 taps and J = 3; 1011 at 2 taps);
//   * the 2 L sums are reduced across the wave by a fixed butterfly of wl_shfl that every lane takes part in (wl_shrink1d.h's,
//     for the threshold gradient), multiplied by sigma, and lane i < 2 L writes sum i with an ordinary store to
//     part[(row * tiles + tile) * 2 L + b * L + t] (float32).  No atomics: the caller sums over rows and tiles.
#pragma once
#include "wl_swt1d.h"

// positions of the tile in front of its core
WL_HD int wl_swt1d_tapgrad_head(int L, int J) {
    const int a = (L / 2 - 1) * ((1 << J) - 1), b = (L / 2) * ((1 << J) - 2);
    return a > b ? a : b;
}

// the tile's core
WL_HD int wl_swt1d_tapgrad_core(int L, int J) {
    return 64 * WL_WAVE1D_V - wl_swt1d_tapgrad_head(L, J) - (L / 2) * ((1 << J) - 1);
}

// One level of the correlations on the lane's registers: the sources M = i + (t - (L/2 - 1)) D of u in ascending order, v and w
// already zero outside the core.
template <int L, int V, int D>
struct WlSwt1dTapCorr {
    static const int LO = -(L / 2 - 1) * D, HI = V - 1 + (L / 2) * D;
    template <int M>
    static WL_DEV void step(const float (&u)[V], const float (&v)[V], const float (&w)[V], int lane, float (&c0)[L], float (&c1)[L]) {
        const float s = wl_wave1d_fetch<V, V, 0, M>(u, lane);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int dl = M - i + (L / 2 - 1) * D;        // = t * D
            if (dl >= 0 && dl % D == 0 && dl / D < L) {
                c0[dl / D] = __builtin_fmaf(v[i], s, c0[dl / D]);
                c1[dl / D] = __builtin_fmaf(w[i], s, c1[dl / D]);
            }
        }
    }
    template <int... S>
    static WL_DEV void steps(const float (&u)[V], const float (&v)[V], const float (&w)[V], int lane, float (&c0)[L], float (&c1)[L],
                             std::integer_sequence<int, S...>) {
        (step<LO + S>(u, v, w, lane, c0, c1), ...);
    }
    static WL_DEV void run(const float (&u)[V], const float (&v)[V], const float (&w)[V], int lane, float (&c0)[L], float (&c1)[L]) {
        steps(u, v, w, lane, c0, c1, std::make_integer_sequence<int, HI - LO + 1>());
    }
};

template <typename T>
struct WlSwt1dTapGradArgs {
    const T* s; const T* top; const T* hi[WL_WAVE1D_MAXJ];     // hi[j]: level j + 1, nullptr = zeros
    float* part;                                               // [rows][tiles][2][L]
    const float* k0; const float* k1;
    int64_t rows, waves;                                       // waves = rows * tiles
    int len, nlev, tiles, core, origin;
    float scale;                                               // per level
};

template <typename T, int L>
struct WlSwt1dTapGrad {
    typedef WlSwt1dTapGradArgs<T> Args;
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
    // zeros outside the core cut to the row
    static WL_DEV void cut(float (&r)[V], int p0, int c0, int c1) {
#pragma unroll
        for (int i = 0; i < V; ++i) r[i] = (p0 + i >= c0 && p0 + i < c1) ? r[i] : 0.f;
    }
    static WL_DEV float wave_sum(float v, int lane) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) v += wl_shfl(v, lane ^ k);
        return v;
    }
    // level j of dilation D: v <- v_{j-1} (LAST: none), the correlations of (v_j, w_j) with u_{j-1}
    template <int D, bool LAST>
    static WL_DEV void level(const float (&u)[V], float (&v)[V], float (&w)[V], const float (&k0)[L], const float (&k1)[L],
                             const WlWave1dTile& t, float scale, float (&c0)[L], float (&c1)[L]) {
        float out[V];
        if constexpr (!LAST) WlSwt1dAdjLevel<L, V, D>::run(v, w, k0, k1, t.lane, scale, out);
        cut(v, t.p0, t.c0, t.c1);
        cut(w, t.p0, t.c0, t.c1);
        WlSwt1dTapCorr<L, V, D>::run(u, v, w, t.lane, c0, c1);
        if constexpr (!LAST) {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = out[i];
        }
    }
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t wv = wl_wave1d_wave(ctx);
        if (wv >= a.waves) return;                         // (the wave as a whole, before any shuffle)
        const int len = a.len, J = a.nlev;
        WlWave1dTile t;
        wl_wave1d_tile<V>(a, ctx, wv, wl_swt1d_tapgrad_head(L, a.nlev), t);
        const int lane = t.lane;
        const int s0 = wl_pmod(t.p0, len);
        float k0[L], k1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { k0[i] = a.k0[i]; k1[i] = a.k1[i]; }
        float u0[V], u1[V], u2[V], v[V], w[V];
        // down: u_0 .. u_{J-1} (the highpass of a level lands in `w` and is dropped)
        wl_wave1d_load<T, V, V>(a.s + t.base, s0, len, u0, 0);
        if (J >= 2) WlSwt1dFwdLevel<L, V, 1>::run(u0, k0, k1, lane, a.scale, u1, w);
        if (J >= 3) WlSwt1dFwdLevel<L, V, 2>::run(u1, k0, k1, lane, a.scale, u2, w);
        float c0[L], c1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { c0[i] = 0.f; c1[i] = 0.f; }
        // up, coarsest first
        wl_wave1d_load<T, V, V>(a.top + t.base, s0, len, v, 0);
        if (J >= 3) {
            tile_of(a.hi[2], t.base, s0, len, w);
            level<4, false>(u2, v, w, k0, k1, t, a.scale, c0, c1);
        }
        if (J >= 2) {
            tile_of(a.hi[1], t.base, s0, len, w);
            level<2, false>(u1, v, w, k0, k1, t, a.scale, c0, c1);
        }
        tile_of(a.hi[0], t.base, s0, len, w);
        level<1, true>(u0, v, w, k0, k1, t, a.scale, c0, c1);
        // lane i < 2 L keeps sum i of the wave
        float mine = 0.f;
#pragma unroll
        for (int i = 0; i < L; ++i) {
            const float r0 = wave_sum(c0[i], lane) * a.scale, r1 = wave_sum(c1[i], lane) * a.scale;
            mine = lane == i ? r0 : (lane == L + i ? r1 : mine);
        }
        if (lane < 2 * L) a.part[wv * (2 * L) + lane] = mine;
    }
};
