// The 1-D stationary (undecimated, a-trous) wavelet transform along the last axis, periodic, up to three levels per launch, on
// wave tiles: no LDS, no workgroup barrier, no role split.
//
//   * a WAVE owns a tile of 64 * V consecutive UNFOLDED positions of one row: position p is sample p mod len (a true floor-mod:
//     tiles start left of 0, and a row may be shorter than the filter and wrap many times inside one tile).  Nothing is
//     decimated, so every level of a periodic signal is periodic with the same period: the cascade runs on the unfolded
//     coordinates and no level has boundary logic;
//   * lane l holds positions a + l*V .. a + l*V + V - 1 in registers, as float.  With i the register index and D the tap offset,
//     both compile-time, the operand of an output lives in register (i + D) mod V of lane l + floor((i + D) / V): the lane's own
//     register when the quotient is 0, one wl_shfl otherwise.  The sources of a level are walked in ascending position, each
//     fetched ONCE and used by every (output, tap) pair that wants it: (L - 1) * d shuffled values per lane and level of
//     dilation d, whatever V;
//   * the sum of an output runs over its sources in ascending position (analysis: taps ascending), every term an explicit fused
//     multiply-add (wl_dwt3d.h): an output's bits do not depend on where in a tile, or in which tile, it falls;
//   * a level of dilation d eats (L/2 - 1) * d positions of the tile on one side and (L/2) * d on the other; lanes near the tile's
//     ends compute garbage (their shuffles wrap around the wave) that is never stored.  The CORE of a tile is what is still
//     valid after the last level: 64 * V - (L - 1) * (2^J - 1) positions.  Only core positions are stored - each highpass from
//     the level that made it, the lowpass at the end -, tiles advance by the core, the grid is rows x tiles, one tile per wave,
//     WL_SWT1D_WAVES waves per workgroup.  A wave whose tile index is past the grid leaves as a whole; inside the body all 64
//     lanes reach every shuffle;
//   * loads and stores go in 16-byte pieces where a piece lies inside the row (stores: inside the core), element by element where
//     it straddles the wrap or an end of the core.  A piece is addressed as a vector of ELEMENT alignment: a tile's start
//     follows the core, which is odd, and rows whose length is no whole number of pieces shift every later row, so three
//     tiles in four (2-byte data: seven in eight) are off the 16-byte grid - the hardware takes unaligned global accesses, and
//     the compiler emits one global_load_dwordx4 / global_store_dwordx4 for such a vector.
//
//   analysis, level of dilation d:  lo[p], hi[p] = scale * sum_t h0[t], h1[t] * in[p - (L/2 - 1) d + d t]      (afb1d_atrous,
//                                   stored = reversed taps; d = 1, 2, 4 for levels 1, 2, 3)
//   adjoint:                        out[m] = scale * sum_t (g0[t] lo[m + (L/2 - 1) d - d t] + g1[t] hi[m + (L/2 - 1) d - d t])
//                                   coarsest level first, a missing highpass = zeros
// The two kernels serve four directions: the transform (scale 1), its backward (adjoint, analysis taps, scale 1), the inverse
// (adjoint, synthesis taps, scale 1/2 per level) and the inverse's backward (analysis, synthesis taps, scale 1/2 per level).
// `origin` (tests) moves the first tile's core left by that many positions: the seams fall elsewhere, the bits stay.
#pragma once
#include <utility>
#include "wl_common.h"

#define WL_SWT1D_MAXJ 3
#define WL_SWT1D_MAXL 20
#define WL_SWT1D_WAVES 4       // tiles (waves) per workgroup
#define WL_SWT1D_V 16          // positions per lane

// one 16-byte piece as a vector of element alignment (a struct of elements is taken apart into element accesses)
template <typename T> struct WlSwtPiece;
template <> struct WlSwtPiece<float> { typedef float type __attribute__((ext_vector_type(4), aligned(4), may_alias)); };
template <> struct WlSwtPiece<wl_half> { typedef wl_half type __attribute__((ext_vector_type(8), aligned(2), may_alias)); };
template <> struct WlSwtPiece<wl_bf16> { typedef wl_bf16 type __attribute__((ext_vector_type(8), aligned(2), may_alias)); };

// V consecutive unfolded positions, the first one sample s0 (0 <= s0 < len) of `row`
template <typename T, int V>
WL_DEV void wl_swt1d_load(const T* row, int s0, int len, float (&r)[V]) {
    constexpr int E = 16 / (int)sizeof(T);
    static_assert(V % E == 0, "a lane holds whole 16-byte pieces");
#pragma unroll
    for (int k = 0; k < V; k += E) {
        int s = s0 + k;
        if (s >= len) s %= len;
        if (s + E <= len) {
            const typename WlSwtPiece<T>::type v = *reinterpret_cast<const typename WlSwtPiece<T>::type*>(row + s);
#pragma unroll
            for (int e = 0; e < E; ++e) r[k + e] = (float)v[e];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                r[k + e] = (float)row[s];
                s = s + 1 == len ? 0 : s + 1;
            }
        }
    }
}

// positions p0 .. p0 + V - 1 of a lane: those inside [c0, c1) (0 <= c0, c1 <= len: positions that are samples) are stored
template <typename T, int V>
WL_DEV void wl_swt1d_store(T* row, int p0, int c0, int c1, const float (&r)[V]) {
    constexpr int E = 16 / (int)sizeof(T);
#pragma unroll
    for (int k = 0; k < V; k += E) {
        const int p = p0 + k;
        if (p >= c0 && p + E <= c1) {
            typename WlSwtPiece<T>::type v;
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = (T)r[k + e];
            *reinterpret_cast<typename WlSwtPiece<T>::type*>(row + p) = v;
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (p + e >= c0 && p + e < c1) row[p + e] = (T)r[k + e];
        }
    }
}

// tile-relative source position M of a lane (register M mod V of lane + floor(M / V)), fetched once
template <int V, int M>
WL_DEV float wl_swt1d_fetch(const float (&in)[V], int lane) {
    constexpr int Q = (M >= 0 ? M : M - V + 1) / V, K = M - Q * V;
    if constexpr (Q == 0) return in[K];
    else return wl_shfl(in[K], lane + Q);
}

// One analysis level of dilation D on the lane's registers: the sources M = i + (t - (L/2 - 1)) D in ascending order.
template <int L, int V, int D>
struct WlSwt1dFwdLevel {
    static const int LO = -(L / 2 - 1) * D, HI = V - 1 + (L / 2) * D;
    template <int M>
    static WL_DEV void step(const float (&in)[V], const float (&h0)[L], const float (&h1)[L], int lane, float (&lo)[V], float (&hi)[V]) {
        const float v = wl_swt1d_fetch<V, M>(in, lane);
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
        const float vl = wl_swt1d_fetch<V, M>(lo, lane);
        const float vh = wl_swt1d_fetch<V, M>(hi, lane);
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
    const T* x; T* lo; T* hi[WL_SWT1D_MAXJ];       // hi[j]: level j + 1, nullptr = not stored
    const float* h0; const float* h1;
    int64_t rows, waves;                           // waves = rows * tiles
    int len, nlev, tiles, core, origin;
    float scale;                                   // per level
};

template <typename T, int L>
struct WlSwt1dFwd {
    typedef WlSwt1dFwdArgs<T> Args;
    static const int kThreads = 64 * WL_SWT1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_SWT1D_V;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = ctx.bid * WL_SWT1D_WAVES + (ctx.tid >> 6);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int lane = ctx.tid & 63;
        const int64_t row = w / a.tiles;
        const int tile = (int)(w - row * a.tiles);
        const int len = a.len, J = a.nlev;
        const int cs = tile * a.core - a.origin;           // the core: [cs, cs + core) cut to the row
        const int c0 = cs > 0 ? cs : 0, c1 = cs + a.core < len ? cs + a.core : len;
        const int p0 = cs - (L / 2 - 1) * ((1 << J) - 1) + lane * V;
        float h0[L], h1[L];
#pragma unroll
        for (int t = 0; t < L; ++t) { h0[t] = a.h0[t]; h1[t] = a.h1[t]; }
        const int64_t base = row * len;
        float r[V], lo[V], hi[V];
        wl_swt1d_load<T, V>(a.x + base, wl_pmod(p0, len), len, r);
        WlSwt1dFwdLevel<L, V, 1>::run(r, h0, h1, lane, a.scale, lo, hi);
        if (a.hi[0]) wl_swt1d_store<T, V>(a.hi[0] + base, p0, c0, c1, hi);
        if (J >= 2) {
            WlSwt1dFwdLevel<L, V, 2>::run(lo, h0, h1, lane, a.scale, r, hi);
            if (a.hi[1]) wl_swt1d_store<T, V>(a.hi[1] + base, p0, c0, c1, hi);
            if (J >= 3) {
                WlSwt1dFwdLevel<L, V, 4>::run(r, h0, h1, lane, a.scale, lo, hi);
                if (a.hi[2]) wl_swt1d_store<T, V>(a.hi[2] + base, p0, c0, c1, hi);
                wl_swt1d_store<T, V>(a.lo + base, p0, c0, c1, lo);
            } else {
                wl_swt1d_store<T, V>(a.lo + base, p0, c0, c1, r);
            }
        } else {
            wl_swt1d_store<T, V>(a.lo + base, p0, c0, c1, lo);
        }
    }
};

template <typename T>
struct WlSwt1dAdjArgs {
    const T* lo; const T* hi[WL_SWT1D_MAXJ]; T* y; // hi[j]: level j + 1, nullptr = zeros
    const float* g0; const float* g1;
    int64_t rows, waves;
    int len, nlev, tiles, core, origin;
    float scale;                                   // per level
};

template <typename T, int L>
struct WlSwt1dAdj {
    typedef WlSwt1dAdjArgs<T> Args;
    static const int kThreads = 64 * WL_SWT1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_SWT1D_V;
    static WL_DEV void tile_of(const T* src, int64_t base, int s0, int len, float (&r)[V]) {
        if (src) wl_swt1d_load<T, V>(src + base, s0, len, r);
        else {
#pragma unroll
            for (int i = 0; i < V; ++i) r[i] = 0.f;
        }
    }
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = ctx.bid * WL_SWT1D_WAVES + (ctx.tid >> 6);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int lane = ctx.tid & 63;
        const int64_t row = w / a.tiles;
        const int tile = (int)(w - row * a.tiles);
        const int len = a.len, J = a.nlev;
        const int cs = tile * a.core - a.origin;
        const int c0 = cs > 0 ? cs : 0, c1 = cs + a.core < len ? cs + a.core : len;
        const int p0 = cs - (L / 2) * ((1 << J) - 1) + lane * V;
        const int s0 = wl_pmod(p0, len);
        float g0[L], g1[L];
#pragma unroll
        for (int t = 0; t < L; ++t) { g0[t] = a.g0[t]; g1[t] = a.g1[t]; }
        const int64_t base = row * len;
        float lo[V], hi[V], out[V];
        wl_swt1d_load<T, V>(a.lo + base, s0, len, lo);
        if (J >= 3) {
            tile_of(a.hi[2], base, s0, len, hi);
            WlSwt1dAdjLevel<L, V, 4>::run(lo, hi, g0, g1, lane, a.scale, out);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = out[i];
        }
        if (J >= 2) {
            tile_of(a.hi[1], base, s0, len, hi);
            WlSwt1dAdjLevel<L, V, 2>::run(lo, hi, g0, g1, lane, a.scale, out);
#pragma unroll
            for (int i = 0; i < V; ++i) lo[i] = out[i];
        }
        tile_of(a.hi[0], base, s0, len, hi);
        WlSwt1dAdjLevel<L, V, 1>::run(lo, hi, g0, g1, lane, a.scale, out);
        wl_swt1d_store<T, V>(a.y + base, p0, c0, c1, out);
    }
};
