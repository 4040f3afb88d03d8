// The 1-D wavelet packet transform (the full tree: every band is split again) along the last axis, periodization, up to three
// levels per launch, on the wave tiles of wl_wave1d.h (the tile scheme, the piece accesses and the fetch are explained there).
//
//   * rows of a (rows, len) tensor go to / come from the packed (rows, 2^J, len / 2^J) tensor of the J levels of a launch: band b
//     of a row - b = sum_j s_j 2^(J-j), s_j = 1 the highpass taken at level j, level 1 the most significant bit - is one
//     contiguous run of len / 2^J coefficients, so the next launch reads the bands as 2^J times as many rows;
//   * len is a multiple of 2^J, so every level of the periodized tree is periodic on the unfolded coordinates.  After level j a
//     lane holds V / 2^j consecutive coefficients of each of the 2^j bands - V registers at every level - and fetches a
//     band's sources from that band's run of registers: (L - 2) shuffled values per lane and band split, (L - 2)(2^J - 1) per
//     launch.  Synthesis sums the lowpass term in front of the highpass term; the last level rounds once per store;
//   * a level eats at most L/2 positions of its own resolution on either side.  head = (L/2)(2^J - 1) rounded up to a multiple
//     of 2^J covers all J levels in both directions, the core is the 64 * V - 2 * head positions in between.  Tile starts and
//     the core are multiples of 2^J, so every lane decimates on the row's own phase (and `origin` is a multiple of 2^J);
//   * on the band side a lane owns V / 2^J consecutive coefficients of a band: its piece is 16 bytes where it owns that much
//     and its whole run (8 or 4 bytes) where it owns less - consecutive lanes touch consecutive addresses, a band of a tile
//     is one contiguous run of core / 2^J elements.
//
//   analysis of a band of even length m:   lo[k], hi[k] = sum_t h0[t], h1[t] * in[(2k + t - (L/2 - 1)) mod m]
//   synthesis, its exact transpose:        out[i] = sum over (k, t) with 2k + t - (L/2 - 1) = i (mod m) of g0[t] lo[k] + g1[t] hi[k]
// (the periodization bank of wl_corr1d / wl_synth1d with the stored taps, for bands at least as long as the filter).  The two
// kernels serve four directions: the transform (analysis taps), its backward (synthesis kernel, analysis taps), the inverse
// (synthesis taps) and the inverse's backward (analysis kernel, synthesis taps).
#pragma once
#include "wl_wave1d.h"

// One analysis level on the lane's V registers: V / VI bands of VI coefficients each; band B's lowpass becomes band 2B, its
// highpass band 2B + 1, VI / 2 coefficients each.  Per band the sources M = 2k + t - (L/2 - 1) in ascending order.
template <int L, int V, int VI>
struct WlWpt1dAfbLevel {
    static const int NB = V / VI, VO = VI / 2;
    static const int LO = -(L / 2 - 1), HI = VI - 2 + L / 2, NM = HI - LO + 1;
    template <int S>
    static WL_DEV void step(const float (&in)[V], const float (&h0)[L], const float (&h1)[L], int lane, float (&out)[V]) {
        constexpr int B = S / NM, M = LO + S % NM;
        const float v = wl_wave1d_fetch<V, VI, B * VI, M>(in, lane);
#pragma unroll
        for (int k = 0; k < VO; ++k) {
            const int t = M - 2 * k + (L / 2 - 1);
            if (t >= 0 && t < L) {
                out[B * VI + k] = __builtin_fmaf(h0[t], v, out[B * VI + k]);
                out[B * VI + VO + k] = __builtin_fmaf(h1[t], v, out[B * VI + VO + k]);
            }
        }
    }
    template <int... S>
    static WL_DEV void steps(const float (&in)[V], const float (&h0)[L], const float (&h1)[L], int lane, float (&out)[V],
                             std::integer_sequence<int, S...>) {
        (step<S>(in, h0, h1, lane, out), ...);
    }
    static WL_DEV void run(const float (&in)[V], const float (&h0)[L], const float (&h1)[L], int lane, float (&out)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) out[i] = 0.f;
        steps(in, h0, h1, lane, out, std::make_integer_sequence<int, NB * NM>());
    }
};

// One level of the transpose: V / VC bands of VC coefficients each; bands 2B (lowpass) and 2B + 1 (highpass) become band B of
// 2 VC coefficients.  Per band the sources M in ascending order, output i takes tap t = i + (L/2 - 1) - 2M of it.
template <int L, int V, int VC>
struct WlWpt1dSfbLevel {
    static const int NB = V / (2 * VC), VX = 2 * VC;
    static const int LO = -(L / 4), HI = (VX - 1 + L / 2 - 1) / 2, NM = HI - LO + 1;
    template <int S>
    static WL_DEV void step(const float (&in)[V], const float (&g0)[L], const float (&g1)[L], int lane, float (&out)[V]) {
        constexpr int B = S / NM, M = LO + S % NM;
        const float vl = wl_wave1d_fetch<V, VC, B * VX, M>(in, lane);
        const float vh = wl_wave1d_fetch<V, VC, B * VX + VC, M>(in, lane);
#pragma unroll
        for (int i = 0; i < VX; ++i) {
            const int t = i + (L / 2 - 1) - 2 * M;
            if (t >= 0 && t < L) {
                out[B * VX + i] = __builtin_fmaf(g0[t], vl, out[B * VX + i]);
                out[B * VX + i] = __builtin_fmaf(g1[t], vh, out[B * VX + i]);
            }
        }
    }
    template <int... S>
    static WL_DEV void steps(const float (&in)[V], const float (&g0)[L], const float (&g1)[L], int lane, float (&out)[V],
                             std::integer_sequence<int, S...>) {
        (step<S>(in, g0, g1, lane, out), ...);
    }
    static WL_DEV void run(const float (&in)[V], const float (&g0)[L], const float (&g1)[L], int lane, float (&out)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) out[i] = 0.f;
        steps(in, g0, g1, lane, out, std::make_integer_sequence<int, NB * NM>());
    }
};

// x: the (rows, len) side, y: the packed (rows, 2^nlev, len >> nlev) side; f0 / f1: the stored lowpass / highpass taps
template <typename T>
struct WlWpt1dArgs {
    const T* src; T* dst;
    const float* f0; const float* f1;
    int64_t rows, waves;                           // waves = rows * tiles
    int len, nlev, tiles, head, core, origin;
};

// The tile of the wave; false: the wave is past the grid and leaves (as a whole).  Both kernels take the test through this
// function and the stationary kernels write it into their bodies: either family compiled the other's way gets other
// registers ("One tile function, two exits").
template <int V, typename T>
WL_DEV bool wl_wpt1d_tile(const WlWpt1dArgs<T>& a, const WlCtx& ctx, WlWave1dTile& t) {
    const int64_t w = wl_wave1d_wave(ctx);
    if (w >= a.waves) return false;
    wl_wave1d_tile<V>(a, ctx, w, a.head, t);
    return true;
}

// the 2^NL bands of the lane, V >> NL coefficients each, to / from the packed side
template <typename T, int V, int NL>
WL_DEV void wl_wpt1d_store_bands(T* y, const WlWave1dTile& t, int len, const float (&r)[V]) {
    constexpr int VJ = V >> NL;
    const int m = len >> NL;
#pragma unroll
    for (int b = 0; b < (1 << NL); ++b)
        wl_wave1d_store<T, VJ, V>(y + t.base + (int64_t)b * m, t.p0 >> NL, t.c0 >> NL, t.c1 >> NL, r, b * VJ);
}

template <typename T, int V, int NL>
WL_DEV void wl_wpt1d_load_bands(const T* y, const WlWave1dTile& t, int len, float (&r)[V]) {
    constexpr int VJ = V >> NL;
    const int m = len >> NL;
    const int s0 = wl_pmod(t.p0 >> NL, m);             // (p0 is a multiple of 2^NL: the shift is exact)
#pragma unroll
    for (int b = 0; b < (1 << NL); ++b)
        wl_wave1d_load<T, VJ, V>(y + t.base + (int64_t)b * m, s0, m, r, b * VJ);
}

template <typename T, int L>
struct WlWpt1dAfb {
    typedef WlWpt1dArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        WlWave1dTile t;
        if (!wl_wpt1d_tile<V>(a, ctx, t)) return;
        float h0[L], h1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { h0[i] = a.f0[i]; h1[i] = a.f1[i]; }
        float r[V], s[V];
        wl_wave1d_load<T, V, V>(a.src + t.base, wl_pmod(t.p0, a.len), a.len, r, 0);
        WlWpt1dAfbLevel<L, V, V>::run(r, h0, h1, t.lane, s);
        if (a.nlev == 1) {
            wl_wpt1d_store_bands<T, V, 1>(a.dst, t, a.len, s);
            return;
        }
        WlWpt1dAfbLevel<L, V, V / 2>::run(s, h0, h1, t.lane, r);
        if (a.nlev == 2) {
            wl_wpt1d_store_bands<T, V, 2>(a.dst, t, a.len, r);
            return;
        }
        WlWpt1dAfbLevel<L, V, V / 4>::run(r, h0, h1, t.lane, s);
        wl_wpt1d_store_bands<T, V, 3>(a.dst, t, a.len, s);
    }
};

template <typename T, int L>
struct WlWpt1dSfb {
    typedef WlWpt1dArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        WlWave1dTile t;
        if (!wl_wpt1d_tile<V>(a, ctx, t)) return;
        float g0[L], g1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { g0[i] = a.f0[i]; g1[i] = a.f1[i]; }
        float r[V], s[V];
        if (a.nlev == 3) {
            wl_wpt1d_load_bands<T, V, 3>(a.src, t, a.len, s);
            WlWpt1dSfbLevel<L, V, V / 8>::run(s, g0, g1, t.lane, r);
            WlWpt1dSfbLevel<L, V, V / 4>::run(r, g0, g1, t.lane, s);
        } else if (a.nlev == 2) {
            wl_wpt1d_load_bands<T, V, 2>(a.src, t, a.len, r);
            WlWpt1dSfbLevel<L, V, V / 4>::run(r, g0, g1, t.lane, s);
        } else {
            wl_wpt1d_load_bands<T, V, 1>(a.src, t, a.len, s);
        }
        WlWpt1dSfbLevel<L, V, V / 2>::run(s, g0, g1, t.lane, r);
        wl_wave1d_store<T, V, V>(a.dst + t.base, t.p0, t.c0, t.c1, r, 0);
    }
};
