// Wave tiles: what the barrier-free 1-D kernels along the last axis (wl_swt1d.h, wl_wpt1d.h, wl_scat1d.h) share.  No LDS, no
// workgroup barrier, no role split.
//
//   * a WAVE owns a tile of 64 * V consecutive UNFOLDED positions of one row: position p is sample p mod len (a true floor-mod:
//     tiles start left of 0, and a row may be shorter than the filter and wrap many times inside one tile).  The transforms here
//     are periodic with the row's period at every level, so the cascade runs on the unfolded coordinates and no level has
//     boundary logic (the scattering layer: the symmetric extension of a row is periodic, wl_wave1d_load_sym);
//   * lane l holds positions a + l*V .. a + l*V + V - 1 in registers, as float.  A source at compile-time offset M from a run of
//     VJ registers of the lane lives in register M mod VJ of lane l + floor(M / VJ): the lane's own register when the quotient
//     is 0, one wl_shfl otherwise (wl_wave1d_fetch).  The sources of a level are walked in ascending position, each fetched
//     ONCE and used by every (output, tap) pair that wants it;
//   * the sum of an output runs over its sources in ascending position, every term an explicit fused multiply-add (wl_dwt3d.h):
//     an output's bits do not depend on where in a tile, or in which tile, it falls.  Intermediate levels stay fp32 in
//     registers;
//   * every level eats positions at both ends of the tile; lanes near the ends compute garbage (their shuffles wrap around the
//     wave) that is never stored.  The CORE of a tile is what is still valid after the last level, `head` positions behind the
//     tile's start (each kernel header has its formulas).  Only core positions are stored, tiles advance by the core, the grid
//     is rows x tiles, one tile per wave, WL_WAVE1D_WAVES waves per workgroup.  A wave whose tile index is past the grid leaves
//     as a whole (wl_wave1d_wave); inside the body all 64 lanes reach every shuffle;
//   * loads and stores go in 16-byte pieces where a piece lies inside the row (stores: inside the core), element by element where
//     it straddles the wrap or an end of the core.  A piece is addressed as a vector of ELEMENT alignment: a tile's start
//     follows the core, which may be odd, and rows whose length is no whole number of pieces shift every later row, so three
//     tiles in four (2-byte data: seven in eight) are off the 16-byte grid - the hardware takes unaligned global accesses, and
//     the compiler emits one global_load_dwordx4 / global_store_dwordx4 for such a vector.  A lane that owns fewer than 16
//     bytes of a run (the packet kernels' bands) moves its whole run as one piece of 8 or 4 bytes.
// `origin` (tests) moves the first tile's core left by that many positions: the seams fall elsewhere, the bits stay.
#pragma once
#include <utility>
#include "wl_common.h"

#define WL_WAVE1D_MAXJ 3        // levels per launch
#define WL_WAVE1D_MAXL 20       // taps
#define WL_WAVE1D_WAVES 4       // tiles (waves) per workgroup
#define WL_WAVE1D_V 16          // positions per lane

// E elements as one access of element alignment (a struct of elements is taken apart into element accesses)
template <typename T, int E> struct WlWavePiece;
#define WL_WAVE_PIECE(T, E) \
    template <> struct WlWavePiece<T, E> { typedef T type __attribute__((ext_vector_type(E), aligned(sizeof(T)), may_alias)); };
WL_WAVE_PIECE(float, 2) WL_WAVE_PIECE(float, 4)
WL_WAVE_PIECE(wl_half, 2) WL_WAVE_PIECE(wl_half, 4) WL_WAVE_PIECE(wl_half, 8)
WL_WAVE_PIECE(wl_bf16, 2) WL_WAVE_PIECE(wl_bf16, 4) WL_WAVE_PIECE(wl_bf16, 8)
#undef WL_WAVE_PIECE

// elements of a lane's piece: 16 bytes, or all N where N elements are less than that
template <typename T, int N> struct WlWaveRun { static const int E = N * (int)sizeof(T) < 16 ? N : 16 / (int)sizeof(T); };

// N consecutive unfolded positions of a periodic run of `len` elements, the first one element s0 (0 <= s0 < len), into
// r[off .. off + N)
template <typename T, int N, int V>
WL_DEV void wl_wave1d_load(const T* run, int s0, int len, float (&r)[V], int off) {
    constexpr int E = WlWaveRun<T, N>::E;
    static_assert(N % E == 0, "a lane holds whole pieces");
#pragma unroll
    for (int k = 0; k < N; k += E) {
        int s = s0 + k;
        if (s >= len) s %= len;
        if (s + E <= len) {
            const typename WlWavePiece<T, E>::type v = *reinterpret_cast<const typename WlWavePiece<T, E>::type*>(run + s);
#pragma unroll
            for (int e = 0; e < E; ++e) r[off + k + e] = (float)v[e];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                r[off + k + e] = (float)run[s];
                s = s + 1 == len ? 0 : s + 1;
            }
        }
    }
}

// The half-sample symmetric fold of a row of n elements that stands for ne = n + (n & 1) samples (an odd row carries a copy of
// its last sample behind it): q, a position already reduced to the period [0, 2 ne), is element
//     s = q < ne ? q : 2 ne - 1 - q,    s == n -> n - 1.
// A true reflection of period 2 ne: a row may be shorter than the filter and fold many times inside one tile.
WL_DEV int wl_wave1d_fold(int q, int n, int ne) {
    const int s = q < ne ? q : 2 * ne - 1 - q;
    return s < n ? s : n - 1;
}

// The symmetric counterpart of wl_wave1d_load: N consecutive unfolded positions from p0 on (any sign) of a row of n elements
// under that fold, into r[off .. off + N).  A piece whose positions map ascending into [0, n) is one access, any other piece
// goes element by element.  Only the pieces that meet the window [w0, w1) are loaded (what the stored core needs of the tile:
// a row's last tile, or a short row's only one, lies mostly outside it); the others are zeros that no stored output reads.
template <typename T, int N, int V>
WL_DEV void wl_wave1d_load_sym(const T* run, int p0, int n, int ne, int w0, int w1, float (&r)[V], int off) {
    constexpr int E = WlWaveRun<T, N>::E;
    static_assert(N % E == 0, "a lane holds whole pieces");
    const int q0 = wl_pmod(p0, 2 * ne);
#pragma unroll
    for (int k = 0; k < N; k += E) {
        if (p0 + k + E <= w0 || p0 + k >= w1) {
#pragma unroll
            for (int e = 0; e < E; ++e) r[off + k + e] = 0.f;
            continue;
        }
        int q = q0 + k;
        if (q >= 2 * ne) q %= 2 * ne;
        if (q + E <= n) {
            const typename WlWavePiece<T, E>::type v = *reinterpret_cast<const typename WlWavePiece<T, E>::type*>(run + q);
#pragma unroll
            for (int e = 0; e < E; ++e) r[off + k + e] = (float)v[e];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                r[off + k + e] = (float)run[wl_wave1d_fold(q, n, ne)];
                q = q + 1 == 2 * ne ? 0 : q + 1;
            }
        }
    }
}

// positions p0 .. p0 + N - 1 of a lane, held in r[off .. off + N): those inside [c0, c1) (0 <= c0, c1 <= len: positions that
// are elements of the run) are stored
template <typename T, int N, int V>
WL_DEV void wl_wave1d_store(T* run, int p0, int c0, int c1, const float (&r)[V], int off) {
    constexpr int E = WlWaveRun<T, N>::E;
#pragma unroll
    for (int k = 0; k < N; k += E) {
        const int p = p0 + k;
        if (p >= c0 && p + E <= c1) {
            typename WlWavePiece<T, E>::type v;
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = (T)r[off + k + e];
            *reinterpret_cast<typename WlWavePiece<T, E>::type*>(run + p) = v;
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (p + e >= c0 && p + e < c1) run[p + e] = (T)r[off + k + e];
        }
    }
}

// source M of a lane, relative to the VJ consecutive positions it holds in in[O .. O + VJ): register M mod VJ of lane
// + floor(M / VJ), fetched once
template <int V, int VJ, int O, int M>
WL_DEV float wl_wave1d_fetch(const float (&in)[V], int lane) {
    constexpr int Q = (M >= 0 ? M : M - VJ + 1) / VJ, K = M - Q * VJ;
    if constexpr (Q == 0) return in[O + K];
    else return wl_shfl(in[O + K], lane + Q);
}

// what a kernel makes of its wave: the row's first element, the lane, its first position, the core cut to the row
struct WlWave1dTile { int64_t base; int lane, p0, c0, c1; };

// the wave's index in the grid of rows x tiles; one that is not below the launch's `waves` leaves before any shuffle
WL_DEV int64_t wl_wave1d_wave(const WlCtx& ctx) { return ctx.bid * WL_WAVE1D_WAVES + (ctx.tid >> 6); }

// The tile of wave w of the launch `a` (its tiles, core, origin and len), `head` positions of the tile in front of its core.
template <int V, typename A>
WL_DEV void wl_wave1d_tile(const A& a, const WlCtx& ctx, int64_t w, int head, WlWave1dTile& t) {
    t.lane = ctx.tid & 63;
    const int64_t row = w / a.tiles;
    const int tile = (int)(w - row * a.tiles);
    const int cs = tile * a.core - a.origin;           // the core: [cs, cs + core) cut to the row
    t.c0 = cs > 0 ? cs : 0;
    t.c1 = cs + a.core < a.len ? cs + a.core : a.len;
    t.p0 = cs - head + t.lane * V;
    t.base = row * a.len;
}
