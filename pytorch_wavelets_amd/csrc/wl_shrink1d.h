// Wavelet shrinkage of the 1-D stationary transform along the last axis, periodic, up to three levels, in ONE launch per
// direction on the wave tiles of wl_wave1d.h: analysis (wl_swt1d.h's level bodies, taps h, scale 1), a threshold on every
// highpass, the inverse (the adjoint level bodies, taps g, 1/2 per level) - without leaving registers.  x is read once and y
// written once whatever J; nothing is stored for the backward, which recomputes.
//
//   shrink, t = thr[j * rows + row] (float32, used as given):   soft  w' = sign(w) max(|w| - t, 0)
//                                                               hard  w' = w [|w| > t]              (the mask is strict in both)
//   * the analysis eats (L/2 - 1)(2^J - 1) positions of the tile in front and (L/2)(2^J - 1) behind, the adjoint the mirror image:
//     the head is (L - 1)(2^J - 1) on both sides and the core 64 V - 2 (L - 1)(2^J - 1) positions (758 at 20 taps and J = 3);
//   * backward: the analysis of x is run again - the same level bodies on the same tile, so the same bits as the forward's
//     (an output's bits do not depend on its place in a tile anyway) - and only two bits per coefficient are kept of it, 16-bit
//     fields in one register per level.  Then dy goes through the analysis with g and 1/2 per level, every dhi_j is
//     multiplied by the mask, and the adjoint with h and scale 1 gives dx;
//   * the threshold gradient of soft shrinkage, dt_j = - sum_p sign(hi_j[p]) [|hi_j[p]| > t_j] dhi_j[p] (the unmasked dhi), is
//     summed per lane over CORE positions only - the cores partition a row -, reduced across the wave by a fixed butterfly of
//     wl_shfl that every lane takes part in, and written by lane 0 with ordinary stores to dthr_part[(row * tiles + tile) * J + j].
//     No atomics: the caller sums over tiles.  A null dthr_part skips the reduction; hard shrinkage writes zeros.
#pragma once
#include "wl_swt1d.h"

#define WL_SHRINK_SOFT 0
#define WL_SHRINK_HARD 1

// the two bits of a coefficient w under the threshold t: A = kept and positive, B = kept and negative, A and B = kept and zero
// (a negative t keeps zeros, whose sign is 0).  kept = A | B, sign = A - B.
struct WlShrinkBits {
    template <int V>
    static WL_DEV unsigned pack(const float (&w)[V], float t) {
        static_assert(V <= 16, "two 16-bit fields in one register");
        unsigned bits = 0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const bool keep = __builtin_fabsf(w[i]) > t;
            if (keep && w[i] >= 0.f) bits |= 1u << i;
            if (keep && w[i] <= 0.f) bits |= 1u << (16 + i);
        }
        return bits;
    }
    static WL_DEV bool keep(unsigned bits, int i) { return (((bits >> i) | (bits >> (16 + i))) & 1u) != 0; }
    static WL_DEV float sign(unsigned bits, int i) { return (float)(int)((bits >> i) & 1u) - (float)(int)((bits >> (16 + i)) & 1u); }
};

template <int V>
WL_DEV void wl_shrink1d_apply(float (&w)[V], float t, int kind) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const float a = __builtin_fabsf(w[i]);
        const float s = w[i] > 0.f ? 1.f : (w[i] < 0.f ? -1.f : 0.f);
        const float soft = s * (a - t);
        w[i] = a > t ? (kind == WL_SHRINK_HARD ? w[i] : soft) : 0.f;
    }
}

template <typename T>
struct WlShrink1dFwdArgs {
    const T* x; T* y;
    const float* thr;                              // [nlev][rows]
    const float* h0; const float* h1; const float* g0; const float* g1;
    int64_t rows, waves;                           // waves = rows * tiles
    int len, nlev, tiles, core, origin, kind;
};

template <typename T, int L>
struct WlShrink1dFwd {
    typedef WlShrink1dFwdArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = wl_wave1d_wave(ctx);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int len = a.len, J = a.nlev, kind = a.kind;
        WlWave1dTile t;
        wl_wave1d_tile<V>(a, ctx, w, (L - 1) * ((1 << a.nlev) - 1), t);
        const int lane = t.lane;
        const int64_t row = w / a.tiles;
        float f0[L], f1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { f0[i] = a.h0[i]; f1[i] = a.h1[i]; }
        float r[V], lo[V], hi1[V], hi2[V], hi3[V];
        wl_wave1d_load<T, V, V>(a.x + t.base, wl_pmod(t.p0, len), len, r, 0);
        // down: the lowpass of level J ends in `lo`
        WlSwt1dFwdLevel<L, V, 1>::run(r, f0, f1, lane, 1.f, lo, hi1);
        wl_shrink1d_apply<V>(hi1, a.thr[row], kind);
        if (J >= 2) {
            WlSwt1dFwdLevel<L, V, 2>::run(lo, f0, f1, lane, 1.f, r, hi2);
            wl_shrink1d_apply<V>(hi2, a.thr[a.rows + row], kind);
            if (J >= 3) {
                WlSwt1dFwdLevel<L, V, 4>::run(r, f0, f1, lane, 1.f, lo, hi3);
                wl_shrink1d_apply<V>(hi3, a.thr[2 * a.rows + row], kind);
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) lo[i] = r[i];
            }
        }
        // up, coarsest first
#pragma unroll
        for (int i = 0; i < L; ++i) { f0[i] = a.g0[i]; f1[i] = a.g1[i]; }
        if (J >= 3) {
            WlSwt1dAdjLevel<L, V, 4>::run(lo, hi3, f0, f1, lane, 0.5f, r);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = r[i];
        }
        if (J >= 2) {
            WlSwt1dAdjLevel<L, V, 2>::run(lo, hi2, f0, f1, lane, 0.5f, r);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = r[i];
        }
        WlSwt1dAdjLevel<L, V, 1>::run(lo, hi1, f0, f1, lane, 0.5f, r);
        wl_wave1d_store<T, V, V>(a.y + t.base, t.p0, t.c0, t.c1, r, 0);
    }
};

template <typename T>
struct WlShrink1dBwdArgs {
    const T* x; const T* dy; T* dx;
    const float* thr;                              // [nlev][rows]
    float* dthr_part;                              // [rows][tiles][nlev], nullptr = not wanted
    const float* h0; const float* h1; const float* g0; const float* g1;
    int64_t rows, waves;
    int len, nlev, tiles, core, origin, kind;
};

template <typename T, int L>
struct WlShrink1dBwd {
    typedef WlShrink1dBwdArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    // - sum over the lane's core positions of sign * dhi (the bits are empty where nothing is kept)
    static WL_DEV float partial(const float (&dhi)[V], unsigned bits, int p0, int c0, int c1) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float term = WlShrinkBits::sign(bits, i) * dhi[i];
            s -= (p0 + i >= c0 && p0 + i < c1) ? term : 0.f;
        }
        return s;
    }
    static WL_DEV void mask(float (&dhi)[V], unsigned bits) {
#pragma unroll
        for (int i = 0; i < V; ++i) dhi[i] = WlShrinkBits::keep(bits, i) ? dhi[i] : 0.f;
    }
    static WL_DEV float wave_sum(float v, int lane) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) v += wl_shfl(v, lane ^ k);
        return v;
    }
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = wl_wave1d_wave(ctx);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int len = a.len, J = a.nlev;
        WlWave1dTile t;
        wl_wave1d_tile<V>(a, ctx, w, (L - 1) * ((1 << a.nlev) - 1), t);
        const int lane = t.lane;
        const int64_t row = w / a.tiles;
        const int s0 = wl_pmod(t.p0, len);
        float f0[L], f1[L];
#pragma unroll
        for (int i = 0; i < L; ++i) { f0[i] = a.h0[i]; f1[i] = a.h1[i]; }
        float r[V], lo[V], d1[V], d2[V], d3[V];
        unsigned b1, b2 = 0, b3 = 0;
        // the forward's coefficients again, of which the bits stay
        wl_wave1d_load<T, V, V>(a.x + t.base, s0, len, r, 0);
        WlSwt1dFwdLevel<L, V, 1>::run(r, f0, f1, lane, 1.f, lo, d1);
        b1 = WlShrinkBits::pack<V>(d1, a.thr[row]);
        if (J >= 2) {
            WlSwt1dFwdLevel<L, V, 2>::run(lo, f0, f1, lane, 1.f, r, d2);
            b2 = WlShrinkBits::pack<V>(d2, a.thr[a.rows + row]);
            if (J >= 3) {
                WlSwt1dFwdLevel<L, V, 4>::run(r, f0, f1, lane, 1.f, lo, d3);
                b3 = WlShrinkBits::pack<V>(d3, a.thr[2 * a.rows + row]);
            }
        }
        // dy down the inverse's backward: g, 1/2 per level
#pragma unroll
        for (int i = 0; i < L; ++i) { f0[i] = a.g0[i]; f1[i] = a.g1[i]; }
        wl_wave1d_load<T, V, V>(a.dy + t.base, s0, len, r, 0);
        WlSwt1dFwdLevel<L, V, 1>::run(r, f0, f1, lane, 0.5f, lo, d1);
        if (J >= 2) {
            WlSwt1dFwdLevel<L, V, 2>::run(lo, f0, f1, lane, 0.5f, r, d2);
            if (J >= 3) {
                WlSwt1dFwdLevel<L, V, 4>::run(r, f0, f1, lane, 0.5f, lo, d3);
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) lo[i] = r[i];
            }
        }
        if (a.dthr_part) {
            const bool soft = a.kind == WL_SHRINK_SOFT;
            float* part = a.dthr_part + w * J;
            const float p1 = soft ? wave_sum(partial(d1, b1, t.p0, t.c0, t.c1), lane) : 0.f;
            if (lane == 0) part[0] = p1;
            if (J >= 2) {
                const float p2 = soft ? wave_sum(partial(d2, b2, t.p0, t.c0, t.c1), lane) : 0.f;
                if (lane == 0) part[1] = p2;
            }
            if (J >= 3) {
                const float p3 = soft ? wave_sum(partial(d3, b3, t.p0, t.c0, t.c1), lane) : 0.f;
                if (lane == 0) part[2] = p3;
            }
        }
        // up the forward's backward: h, scale 1
#pragma unroll
        for (int i = 0; i < L; ++i) { f0[i] = a.h0[i]; f1[i] = a.h1[i]; }
        if (J >= 3) {
            mask(d3, b3);
            WlSwt1dAdjLevel<L, V, 4>::run(lo, d3, f0, f1, lane, 1.f, r);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = r[i];
        }
        if (J >= 2) {
            mask(d2, b2);
            WlSwt1dAdjLevel<L, V, 2>::run(lo, d2, f0, f1, lane, 1.f, r);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = r[i];
        }
        mask(d1, b1);
        WlSwt1dAdjLevel<L, V, 1>::run(lo, d1, f0, f1, lane, 1.f, r);
        wl_wave1d_store<T, V, V>(a.dx + t.base, t.p0, t.c0, t.c1, r, 0);
    }
};
