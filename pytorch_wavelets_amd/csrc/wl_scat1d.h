// One order of 1-D DTCWT scattering at one scale along the last axis (ScatLayer1D: the ScatLayer of wl_dtcwt_kernels.h on one
// axis), forward and backward in ONE launch each, on the wave tiles of wl_wave1d.h (the tile scheme, the piece accesses and the
// fetch are explained there).  No LDS, no barrier.
//
//   xe = x, an odd row with a copy of its last sample appended (ne samples); with m = L / 2 of the odd tap count L
//   lo[p], hi[p] = sum_j h0o[j], h1o[j] * sym(xe, p + j - m)              (colfilter: half-sample symmetric, stored taps)
//   Z[b, c, k]     = (lo[2k] + lo[2k+1]) / 2
//   Z[b, C + c, k] = r - bias,   r = sqrt(hi[2k]^2 + hi[2k+1]^2 + bias^2)
//   dir[b, c, 2k], dir[b, c, 2k+1] = hi[2k] / r, hi[2k+1] / r             (training only: what the 2-D layer keeps as drdx, drdy)
//   backward (the reference's rule, ScatLayerj1_f.backward on one axis):
//   dlo[s] = dZ[b, c, s >> 1] / 2,   dhi[s] = dZ[b, C + c, s >> 1] * dir[s]
//   dxe[p] = sum_j h0o[j] sym(dlo, p + j - m0) + h1o[j] sym(dhi, p + j - m1);   an odd row: dx[n-1] = dxe[n-1] + dxe[n]
//
//   * the signal is not periodic but its symmetric extension is, with period 2 ne: a tile holds 64 * V unfolded positions of
//     that extension (wl_wave1d_load_sym), and the single level has no boundary logic behind the load;
//   * both filters run in one ascending walk over the sources -M .. V - 1 + M of a lane, M = max(L0, L1) / 2: each source is
//     fetched once and feeds every (output, tap) pair of either filter that wants it;
//   * the level eats M positions either end of the tile.  The head is M rounded up to even, the core 64 * V - 2 * head, the
//     origin even: a lane's V positions are V / 2 whole (2k, 2k+1) pairs and the epilogue stays inside the lane.  A lane stores
//     V / 2 lowpass and V / 2 magnitude values in 16-byte pieces, clipped to the core; nothing here assumes symmetric taps.
#pragma once
#include "wl_wave1d.h"
#include "wl_dtcwt_kernels.h"   // wl_sqrt, wl_rcp

template <int L0, int L1, int V>
struct WlScat1dWalk {
    static const int M0 = L0 / 2, M1 = L1 / 2, M = M0 > M1 ? M0 : M1;
    static const int HEAD = (M + 1) / 2 * 2;
    // one source of the analysis: lo, hi += taps * in[S]
    template <int S>
    static WL_DEV void fwd_step(const float (&in)[V], const float (&h0)[L0], const float (&h1)[L1], int lane, float (&lo)[V], float (&hi)[V]) {
        const float v = wl_wave1d_fetch<V, V, 0, S>(in, lane);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int j0 = S - i + M0, j1 = S - i + M1;
            if (j0 >= 0 && j0 < L0) lo[i] = __builtin_fmaf(h0[j0], v, lo[i]);
            if (j1 >= 0 && j1 < L1) hi[i] = __builtin_fmaf(h1[j1], v, hi[i]);
        }
    }
    template <int... S>
    static WL_DEV void fwd_steps(const float (&in)[V], const float (&h0)[L0], const float (&h1)[L1], int lane, float (&lo)[V], float (&hi)[V],
                                 std::integer_sequence<int, S...>) {
        (fwd_step<S - M>(in, h0, h1, lane, lo, hi), ...);
    }
    static WL_DEV void fwd(const float (&in)[V], const float (&h0)[L0], const float (&h1)[L1], int lane, float (&lo)[V], float (&hi)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) { lo[i] = 0.f; hi[i] = 0.f; }
        fwd_steps(in, h0, h1, lane, lo, hi, std::make_integer_sequence<int, V + 2 * M>());
    }
    // one source of the backward: out += h0 * dlo[S] + h1 * dhi[S], the lowpass term in front (the shorter filter does not
    // fetch the sources only the longer one reaches)
    template <int S>
    static WL_DEV void bwd_step(const float (&dlo)[V], const float (&dhi)[V], const float (&h0)[L0], const float (&h1)[L1], int lane, float (&out)[V]) {
        float vl = 0.f, vh = 0.f;
        if constexpr (S >= -M0 && S <= V - 1 + M0) vl = wl_wave1d_fetch<V, V, 0, S>(dlo, lane);
        if constexpr (S >= -M1 && S <= V - 1 + M1) vh = wl_wave1d_fetch<V, V, 0, S>(dhi, lane);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int j0 = S - i + M0, j1 = S - i + M1;
            if (j0 >= 0 && j0 < L0) out[i] = __builtin_fmaf(h0[j0], vl, out[i]);
            if (j1 >= 0 && j1 < L1) out[i] = __builtin_fmaf(h1[j1], vh, out[i]);
        }
    }
    template <int... S>
    static WL_DEV void bwd_steps(const float (&dlo)[V], const float (&dhi)[V], const float (&h0)[L0], const float (&h1)[L1], int lane, float (&out)[V],
                                 std::integer_sequence<int, S...>) {
        (bwd_step<S - M>(dlo, dhi, h0, h1, lane, out), ...);
    }
    static WL_DEV void bwd(const float (&dlo)[V], const float (&dhi)[V], const float (&h0)[L0], const float (&h1)[L1], int lane, float (&out)[V]) {
#pragma unroll
        for (int i = 0; i < V; ++i) out[i] = 0.f;
        bwd_steps(dlo, dhi, h0, h1, lane, out, std::make_integer_sequence<int, V + 2 * M>());
    }
};

// `len` = ne, the even length the tiles cover; z (batch, 2 C, ne / 2), dir (batch * C, ne), x / dx (batch * C, n)
template <typename T>
struct WlScat1dFwdArgs {
    const T* x; T* z; T* dir;                      // dir: nullptr = not stored (inference)
    const float* h0; const float* h1;
    int64_t rows, waves;                           // rows = batch * C, waves = rows * tiles
    int C, n, len, tiles, core, origin;
    float bias;
};

template <typename T, int L0, int L1>
struct WlScat1dFwd {
    typedef WlScat1dFwdArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    typedef WlScat1dWalk<L0, L1, V> Walk;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = wl_wave1d_wave(ctx);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int n = a.n, ne = a.len, C = a.C;
        WlWave1dTile t;
        wl_wave1d_tile<V>(a, ctx, w, Walk::HEAD, t);
        const int lane = t.lane;
        const int64_t row = w / a.tiles, b = row / C;
        const int no = ne >> 1;
        T* zl = a.z + (row + b * C) * no;                  // Z[b, c]: row b * 2C + c
        T* zm = zl + (int64_t)C * no;                      // Z[b, C + c]
        float h0[L0], h1[L1];
#pragma unroll
        for (int i = 0; i < L0; ++i) h0[i] = a.h0[i];
#pragma unroll
        for (int i = 0; i < L1; ++i) h1[i] = a.h1[i];
        float r[V], lo[V], hi[V];
        wl_wave1d_load_sym<T, V, V>(a.x + row * n, t.p0, n, ne, t.c0 - Walk::M, t.c1 + Walk::M, r, 0);
        Walk::fwd(r, h0, h1, lane, lo, hi);
        const float bias = a.bias, b2 = bias * bias;
        float yl[V / 2], ym[V / 2];
#pragma unroll
        for (int k = 0; k < V / 2; ++k) {
            const float re = hi[2 * k], im = hi[2 * k + 1];
            const float mag = wl_sqrt(__builtin_fmaf(re, re, __builtin_fmaf(im, im, b2)));
            yl[k] = 0.5f * (lo[2 * k] + lo[2 * k + 1]);
            ym[k] = mag - bias;
            const float inv = wl_rcp(mag);
            hi[2 * k] = re * inv;
            hi[2 * k + 1] = im * inv;
        }
        // (p0, c0 and c1 are even: the head, the core, the origin and ne are)
        wl_wave1d_store<T, V / 2, V / 2>(zl, t.p0 >> 1, t.c0 >> 1, t.c1 >> 1, yl, 0);
        wl_wave1d_store<T, V / 2, V / 2>(zm, t.p0 >> 1, t.c0 >> 1, t.c1 >> 1, ym, 0);
        if (a.dir) wl_wave1d_store<T, V, V>(a.dir + t.base, t.p0, t.c0, t.c1, hi, 0);
    }
};

template <typename T>
struct WlScat1dBwdArgs {
    const T* dz; const T* dir; T* dx;
    const float* h0; const float* h1;
    int64_t rows, waves;
    int C, n, len, tiles, core, origin;
};

template <typename T, int L0, int L1>
struct WlScat1dBwd {
    typedef WlScat1dBwdArgs<T> Args;
    static const int kThreads = 64 * WL_WAVE1D_WAVES;
    static const int kMinWaves = 2;
    static const int V = WL_WAVE1D_V;
    typedef WlScat1dWalk<L0, L1, V> Walk;
    // dlo, dhi of V positions from p0 on, through the fold of wl_wave1d_load_sym on the ne positions of dir: a piece of E
    // positions that maps ascending into the row reads E directions and E / 2 of either half of dZ (p0 is even, so is q)
    static WL_DEV void load(const T* zl, const T* zm, const T* dir, int p0, int ne, int w0, int w1, float (&dlo)[V], float (&dhi)[V]) {
        constexpr int E = WlWaveRun<T, V>::E;
        typedef typename WlWavePiece<T, E>::type Piece;
        typedef typename WlWavePiece<T, E / 2>::type Half;
        const int q0 = wl_pmod(p0, 2 * ne);
#pragma unroll
        for (int k = 0; k < V; k += E) {
            if (p0 + k + E <= w0 || p0 + k >= w1) {
#pragma unroll
                for (int e = 0; e < E; ++e) { dlo[k + e] = 0.f; dhi[k + e] = 0.f; }
                continue;
            }
            int q = q0 + k;
            if (q >= 2 * ne) q %= 2 * ne;
            if (q + E <= ne) {
                const Piece d = *reinterpret_cast<const Piece*>(dir + q);
                const Half l = *reinterpret_cast<const Half*>(zl + (q >> 1));
                const Half m = *reinterpret_cast<const Half*>(zm + (q >> 1));
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    dlo[k + e] = 0.5f * (float)l[e >> 1];
                    dhi[k + e] = (float)m[e >> 1] * (float)d[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int s = wl_wave1d_fold(q, ne, ne);
                    dlo[k + e] = 0.5f * (float)zl[s >> 1];
                    dhi[k + e] = (float)zm[s >> 1] * (float)dir[s];
                    q = q + 1 == 2 * ne ? 0 : q + 1;
                }
            }
        }
    }
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int64_t w = wl_wave1d_wave(ctx);
        if (w >= a.waves) return;                          // (the wave as a whole)
        const int n = a.n, ne = a.len, C = a.C;
        WlWave1dTile t;
        wl_wave1d_tile<V>(a, ctx, w, Walk::HEAD, t);
        const int lane = t.lane;
        const int64_t row = w / a.tiles, b = row / C;
        const int no = ne >> 1;
        const T* zl = a.dz + (row + b * C) * no;
        const T* zm = zl + (int64_t)C * no;
        float h0[L0], h1[L1];
#pragma unroll
        for (int i = 0; i < L0; ++i) h0[i] = a.h0[i];
#pragma unroll
        for (int i = 0; i < L1; ++i) h1[i] = a.h1[i];
        float dlo[V], dhi[V], out[V];
        load(zl, zm, a.dir + t.base, t.p0, ne, t.c0 - Walk::M, t.c1 + Walk::M, dlo, dhi);
        Walk::bwd(dlo, dhi, h0, h1, lane, out);
        // an odd row: the appended sample's gradient goes to the one it copies - positions n - 1 and n are a pair of one lane
#pragma unroll
        for (int k = 0; k < V; k += 2)
            if (t.p0 + k == n - 1) out[k] += out[k + 1];   // (p0 + k is even: never true for an even n)
        wl_wave1d_store<T, V, V>(a.dx + row * n, t.p0, t.c0, t.c1 < n ? t.c1 : n, out, 0);
    }
};
