// One level of the 2-D wavelet PACKET transform on packed band blocks: every sub-band is split again, so a level maps
//   analysis :  x (planes, H, W)  ->  y (planes, 4, Kh, Kw)      band s = 2 b_W + b_H (b = 1: highpass), DWTForward's order
//   synthesis:  y (planes, 4, Kh, Kw)  ->  x (planes, OH, OW)    OH / OW at most the natural size (a smaller one crops)
// and the next analysis level reads y as (4 planes, Kh, Kw) planes - a pure view.  The tile kernels of the DWT (wl_dwt_tile.h,
// wl_dwt_tile_syn.h) write ll and the highs to two differently shaped buffers and assume wide planes; these two write / read
// the packed block and take their tile geometry at run time, because the planes of a packet level shrink fourfold per level
// while their number grows fourfold:
//
//   * a workgroup of 256 threads owns one TILE of th x tw coefficients (analysis: of each of the four bands; synthesis: of x)
//     of NP consecutive planes.  The launcher (wl_wpt2d_api.inc) picks th x tw <= 512 - wide planes: 16 x 32, narrow ones
//     taller - and NP = 1 while a plane has more than one tile or more than 256 coefficients ("the wide walk"); planes of at
//     most 256 coefficients are walked NP = 512 / (th tw) at a time ("the plane-run walk"), so that the lanes of a workgroup
//     stay busy on 8 x 8 or 4 x 4 planes.  Neither threshold has been measured;
//   * stage: the input footprint of the tile goes to LDS as fp32 with the boundary extension applied as index math (wl_ext,
//     every mode, any number of folds) - analysis: even and odd columns in two half rows, so that the row bank's lanes read
//     consecutive words; synthesis: the four band tiles, zero (periodization: wrapped) outside the bands;
//   * two banks over LDS with the taps in scalar registers (compile-time tap count, fully unrolled) and fp32 accumulation;
//     the two-bank form throughout: no relation between the taps is used, so nothing has to be verified on the device;
//   * consecutive lanes write consecutive coefficients of a band row (analysis) or of an image row (synthesis).
//
//   analysis :  y[k] = sum_j h[j] ext(x, 2k + base + j)             (ops.afb1d; taps stored reversed), along W, then along H
//   synthesis:  x[n] = sum_u g[(m & 1) + 2u] B((m >> 1) - u),  m = n + s,  s = L - 2, B zero outside [0, K);
//               periodization: s = L/2 - 1 and the band index wraps modulo K      (wl_dwt_tile_syn.h), along H, then along W
// NLEV = 1: one level per launch, every mode.  NLEV = 2 (the end of this file): two levels per launch for periodization with
// every size a multiple of 4 - a workgroup owns a tile of the 16 level-2 bands of one plane and keeps the level-1 bands in LDS.
#pragma once
#include "wl_common.h"

// f / d without a division: m = wl_wpt_magic(d) = ceil(2^32 / d) from the launcher, exact while f d < 2^32 (here both count LDS
// words of one workgroup: below 2^14).  The run-time tile geometry would otherwise cost two ~30-instruction divisions per
// staged element - more than the arithmetic of the banks.
WL_HD unsigned wl_wpt_magic(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d); }
WL_HD int wl_wpt_div(int f, unsigned m) { return m ? (int)(((uint64_t)(unsigned)f * m) >> 32) : f; }

template <typename T>
struct WlWptAfbArgs {
    const T* x;            // (planes, H, W) through x_ps / x_rs
    T* y;                  // (planes, 4, Kh, Kw) dense
    const float* h_w_lo; const float* h_w_hi; const float* h_h_lo; const float* h_h_hi;
    int64_t planes, x_ps;
    int x_rs;
    int H, W, Kh, Kw;
    int base_h, base_w, ext;
    int th, tw, np;        // tile of band coefficients, planes per workgroup
    int tiles_y, tiles_x;
    unsigned m_stage, m_sp, m_tw, m_tile;   // wl_wpt_magic of nr * sp, sp, tw, th * tw (set by the launcher through set_geometry)
};

template <typename T, int LT, int NLEV> struct WlWptAfb;
template <typename T, int LT, int NLEV> struct WlWptSfb;

template <typename T, int LT>
struct WlWptAfb<T, LT, 1> {
    typedef WlWptAfbArgs<T> Args;
    static const int kThreads = 256;
    static const int kMinWaves = 4;      // the launcher budgets LDS for four workgroups per CU: four waves per SIMD
    // floats of LDS for a tile geometry: the staged rows (two half rows of tw + LT/2 - 1 words) + the (lo, hi) rows
    static WL_HD int lds_floats(int th, int tw, int np) { return np * (2 * th + LT - 2) * (2 * (tw + LT / 2 - 1) + 2 * tw); }
    static void set_geometry(Args& a, int th, int tw, int np) {
        a.th = th; a.tw = tw; a.np = np;
        const int nr = 2 * th + LT - 2, sp = 2 * (tw + LT / 2 - 1);
        a.m_stage = wl_wpt_magic(nr * sp); a.m_sp = wl_wpt_magic(sp); a.m_tw = wl_wpt_magic(tw); a.m_tile = wl_wpt_magic(th * tw);
    }

    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int tid = ctx.tid;
        const int tiles = a.tiles_y * a.tiles_x;
        const int64_t grp = ctx.bid / tiles;
        const int tile = (int)(ctx.bid - grp * tiles);
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int th = a.th, tw = a.tw;
        const int kh0 = ty * th, kw0 = tx * tw;
        const int64_t plane0 = grp * a.np;
        const int np = a.planes - plane0 < a.np ? (int)(a.planes - plane0) : a.np;
        const int nr = 2 * th + LT - 2;              // staged rows
        const int hc = tw + LT / 2 - 1;              // staged columns of one parity
        const int sp = 2 * hc;                       // staged row pitch: [even columns | odd columns]
        float* S = reinterpret_cast<float*>(ctx.smem);
        wl_f2* Tm = reinterpret_cast<wl_f2*>(S + a.np * nr * sp);
        // ---- stage ----------------------------------------------------------------------------------------------------
        {
            const int er0 = 2 * kh0 + a.base_h, ec0 = 2 * kw0 + a.base_w;
            const int per_plane = nr * sp;
            for (int f = tid; f < np * per_plane; f += kThreads) {
                const int p = wl_wpt_div(f, a.m_stage), g = f - p * per_plane;
                const int i = wl_wpt_div(g, a.m_sp), c = g - i * sp;
                const int r = wl_ext(er0 + i, a.H, a.ext), cc = wl_ext(ec0 + c, a.W, a.ext);
                float v = 0.f;
                if ((r | cc) >= 0) v = (float)a.x[(plane0 + p) * a.x_ps + (r * a.x_rs + cc)];
                S[p * per_plane + i * sp + (c & 1) * hc + (c >> 1)] = v;
            }
        }
        ctx.sync();
        // ---- row bank (along W): (lo, hi) of every staged row ---------------------------------------------------------
        {
            float h0[LT], h1[LT];
#pragma unroll
            for (int j = 0; j < LT; ++j) { h0[j] = a.h_w_lo[j]; h1[j] = a.h_w_hi[j]; }
            const int rows = np * nr;                // (the staged rows of the np planes lie one after the other)
            for (int f = tid; f < rows * tw; f += kThreads) {
                const int i = wl_wpt_div(f, a.m_tw), k = f - i * tw;
                const float* se = S + i * sp + k;
                float lo = 0.f, hi = 0.f;
#pragma unroll
                for (int j = 0; j < LT; ++j) {       // x[2k + j]: word k + j/2 of the half row of j's parity
                    const float v = se[(j & 1) * hc + (j >> 1)];
                    lo += h0[j] * v;
                    hi += h1[j] * v;
                }
                wl_f2 o; o.x = lo; o.y = hi;
                Tm[f] = o;
            }
        }
        ctx.sync();
        // ---- column bank (along H) + the four band stores ---------------------------------------------------------------
        {
            float h0[LT], h1[LT];
#pragma unroll
            for (int j = 0; j < LT; ++j) { h0[j] = a.h_h_lo[j]; h1[j] = a.h_h_hi[j]; }
            const int per_plane = th * tw;
            const int64_t bplane = (int64_t)a.Kh * a.Kw;
            for (int f = tid; f < np * per_plane; f += kThreads) {
                const int p = wl_wpt_div(f, a.m_tile), g = f - p * per_plane;
                const int kh = wl_wpt_div(g, a.m_tw), kw = g - kh * tw;
                const int k = kh0 + kh, kc = kw0 + kw;
                if (k >= a.Kh || kc >= a.Kw) continue;
                const wl_f2* col = Tm + (p * nr + 2 * kh) * tw + kw;
                float ll = 0.f, lh = 0.f, hl = 0.f, hh = 0.f;
#pragma unroll
                for (int j = 0; j < LT; ++j) {
                    const wl_f2 v = col[j * tw];
                    ll += h0[j] * v.x; lh += h1[j] * v.x;
                    hl += h0[j] * v.y; hh += h1[j] * v.y;
                }
                T* dst = a.y + (plane0 + p) * 4 * bplane + (k * a.Kw + kc);
                dst[0] = (T)ll;                      // s = 2 b_W + b_H
                dst[bplane] = (T)lh;
                dst[2 * bplane] = (T)hl;
                dst[3 * bplane] = (T)hh;
            }
        }
    }
};

template <typename T>
struct WlWptSfbArgs {
    const T* y;            // (planes, 4, Kh, Kw) dense
    T* x;                  // (planes, OH, OW) dense
    const float* g_w_lo; const float* g_w_hi; const float* g_h_lo; const float* g_h_hi;
    int64_t planes;
    int Kh, Kw, OH, OW;
    int s, circ;
    int th, tw, np;        // tile of x, planes per workgroup
    int tiles_y, tiles_x;
    unsigned m_band, m_nkc, m_colb, m_rowb, m_npc;   // wl_wpt_magic of nkr * nkc, nkc, npr * nkc, th * npc, npc
};

template <typename T, int LT>
struct WlWptSfb<T, LT, 1> {
    typedef WlWptSfbArgs<T> Args;
    static const int kThreads = 256;
    static const int kMinWaves = 4;      // the launcher budgets LDS for four workgroups per CU: four waves per SIMD
    static const int HL = LT / 2;                    // taps per phase
    // the four band tiles ((t + 1)/2 + HL band samples cover t outputs of either parity) + the (lo, hi) rows of the H bank
    static WL_HD int lds_floats(int th, int tw, int np) {
        return np * ((tw + 1) / 2 + HL) * (4 * ((th + 1) / 2 + HL) + 2 * th);
    }
    static void set_geometry(Args& a, int th, int tw, int np) {
        a.th = th; a.tw = tw; a.np = np;
        const int nkr = (th + 1) / 2 + HL, nkc = (tw + 1) / 2 + HL, npr = th / 2 + 1, npc = tw / 2 + 1;
        a.m_band = wl_wpt_magic(nkr * nkc); a.m_nkc = wl_wpt_magic(nkc); a.m_colb = wl_wpt_magic(npr * nkc);
        a.m_rowb = wl_wpt_magic(th * npc); a.m_npc = wl_wpt_magic(npc);
    }

    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int tid = ctx.tid;
        const int tiles = a.tiles_y * a.tiles_x;
        const int64_t grp = ctx.bid / tiles;
        const int tile = (int)(ctx.bid - grp * tiles);
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int th = a.th, tw = a.tw;
        const int n0 = ty * th, w0 = tx * tw;
        const int64_t plane0 = grp * a.np;
        const int np = a.planes - plane0 < a.np ? (int)(a.planes - plane0) : a.np;
        const int nkr = (th + 1) / 2 + HL, nkc = (tw + 1) / 2 + HL;
        const int kr0 = ((n0 + a.s) >> 1) - (HL - 1), kc0 = ((w0 + a.s) >> 1) - (HL - 1);   // first staged band row / column
        float* B = reinterpret_cast<float*>(ctx.smem);                   // [np][4][nkr][nkc]
        wl_f2* U = reinterpret_cast<wl_f2*>(B + a.np * 4 * nkr * nkc);     // [np][th][nkc]
        const int64_t bplane = (int64_t)a.Kh * a.Kw;
        // ---- stage the four band tiles ----------------------------------------------------------------------------------
        {
            const int per_band = nkr * nkc;
            for (int f = tid; f < np * 4 * per_band; f += kThreads) {
                const int pb = wl_wpt_div(f, a.m_band), g = f - pb * per_band;   // pb = 4 p + band: the bands of a plane are adjacent
                const int i = wl_wpt_div(g, a.m_nkc), j = g - i * nkc;
                int r = kr0 + i, c = kc0 + j;
                if (a.circ) {
                    if ((unsigned)r >= (unsigned)a.Kh) r = wl_pmod(r, a.Kh);
                    if ((unsigned)c >= (unsigned)a.Kw) c = wl_pmod(c, a.Kw);
                }
                float v = 0.f;
                if ((unsigned)r < (unsigned)a.Kh && (unsigned)c < (unsigned)a.Kw)
                    v = (float)a.y[(plane0 * 4 + pb) * bplane + (r * a.Kw + c)];
                B[f] = v;
            }
        }
        ctx.sync();
        // Both banks work on output PAIRS (m, m + 1), m = n + s even: the two outputs meet the same band samples B(m/2 - u), the
        // even one under the taps g[2u], the odd one under g[2u + 1] - compile-time tap indices (a parity-dependent index would
        // put the taps into scratch) and half the LDS reads.  A tile whose first m is odd starts one output early: skipped.
        // ---- column bank (along H): output rows 2 (cr0 + q) - s, + 1 of (W-lo, W-hi) -----------------------------------------
        {
            float g0[LT], g1[LT];
#pragma unroll
            for (int t = 0; t < LT; ++t) { g0[t] = a.g_h_lo[t]; g1[t] = a.g_h_hi[t]; }
            const int npr = th / 2 + 1;
            const int per_plane = npr * nkc;
            const int nl0 = 2 * ((n0 + a.s) >> 1) - a.s - n0;            // 0 or -1: the tile row of pair 0's even output
            const int bs = nkr * nkc;
            for (int f = tid; f < np * per_plane; f += kThreads) {
                const int p = wl_wpt_div(f, a.m_colb), g = f - p * per_plane;
                const int q = wl_wpt_div(g, a.m_nkc), j = g - q * nkc;
                const float* b = B + (p * 4 * nkr + (q + HL - 1)) * nkc + j;   // band 0, band row cr0 + q
                float le = 0.f, he = 0.f, lo = 0.f, ho = 0.f;
#pragma unroll
                for (int u = 0; u < HL; ++u) {
                    const float* r = b - u * nkc;
                    const float b0 = r[0], b1 = r[bs], b2 = r[2 * bs], b3 = r[3 * bs];
                    le += g0[2 * u] * b0;     le += g1[2 * u] * b1;
                    he += g0[2 * u] * b2;     he += g1[2 * u] * b3;
                    lo += g0[2 * u + 1] * b0; lo += g1[2 * u + 1] * b1;
                    ho += g0[2 * u + 1] * b2; ho += g1[2 * u + 1] * b3;
                }
                const int nl = nl0 + 2 * q;
                const int d = (p * th + nl) * nkc + j;
                if (nl >= 0 && nl < th) { wl_f2 o; o.x = le; o.y = he; U[d] = o; }
                if (nl + 1 < th) { wl_f2 o; o.x = lo; o.y = ho; U[d + nkc] = o; }
            }
        }
        ctx.sync();
        // ---- row bank (along W) + store ---------------------------------------------------------------------------------------
        {
            float g0[LT], g1[LT];
#pragma unroll
            for (int t = 0; t < LT; ++t) { g0[t] = a.g_w_lo[t]; g1[t] = a.g_w_hi[t]; }
            const int npc = tw / 2 + 1;
            const int per_plane = th * npc;
            const int wl0 = 2 * ((w0 + a.s) >> 1) - a.s - w0;            // 0 or -1
            const int64_t oplane = (int64_t)a.OH * a.OW;
            for (int f = tid; f < np * per_plane; f += kThreads) {
                const int p = wl_wpt_div(f, a.m_rowb), g = f - p * per_plane;
                const int nl = wl_wpt_div(g, a.m_npc), q = g - nl * npc;
                const int n = n0 + nl;
                if (n >= a.OH) continue;
                const wl_f2* r = U + (p * th + nl) * nkc + (q + HL - 1);
                float ye = 0.f, yo = 0.f;
#pragma unroll
                for (int u = 0; u < HL; ++u) {
                    const wl_f2 v = r[-u];
                    ye += g0[2 * u] * v.x;     ye += g1[2 * u] * v.y;
                    yo += g0[2 * u + 1] * v.x; yo += g1[2 * u + 1] * v.y;
                }
                const int wl = wl0 + 2 * q;
                T* row = a.x + (plane0 + p) * oplane + n * a.OW;
                const int w = w0 + wl;
                if (wl >= 0 && wl < tw && w < a.OW) row[w] = (T)ye;
                if (wl + 1 < tw && w + 1 < a.OW) row[w + 1] = (T)yo;
            }
        }
    }
};

// ---- two levels per launch: periodization, H % 4 == 0 and W % 4 == 0 -------------------------------------------------------
// With every level even, filtering commutes with the periodic extension: a level-1 sample at a wrapped coordinate is simply
// computed from wrapped input, so the tile works in unwrapped coordinates throughout, only the staging wraps, and no tap tests a
// boundary.  (The mirror modes do not commute: they keep one level per launch.)  The level-1 bands never leave LDS; the 16
// level-2 bands are written (analysis) / read (synthesis) once.  Fixed tiles, compile-time index arithmetic.
//
// Analysis: a tile of TH x TW = 8 x 16 coefficients of each of the 16 bands needs N1 = 2 T + L - 2 samples of each level-1 band
// per axis and N0 = 2 N1 + L - 2 = 4 T + 3 (L - 2) input samples.  LDS: the input footprint, its (lo, hi) rows, the four level-1
// bands; the (lo, hi) rows of level 2 reuse the footprint's words.  15 404 floats at 12 taps: two workgroups per CU.
template <typename T, int LT>
struct WlWptAfb<T, LT, 2> {
    typedef WlWptAfbArgs<T> Args;          // Kh / Kw: the LEVEL-2 band size H / 4, W / 4; y (planes, 16, Kh, Kw)
    static const int kThreads = 256;
    static const int kMinWaves = 2;
    static const int TH = 8, TW = 16;
    static const int N1R = 2 * TH + LT - 2, N1C = 2 * TW + LT - 2;
    static const int N0R = 2 * N1R + LT - 2, N0C = 2 * N1C + LT - 2;
    static const int kS = N0R * N0C, kT2 = 8 * N1R * TW;
    static const int kX = kS > kT2 ? kS : kT2;
    static const int kT1 = 2 * N0R * N1C, kB1 = 4 * N1R * N1C;
    static const int kLdsFloats = kX + kT1 + kB1;

    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int tid = ctx.tid;
        const int tiles = a.tiles_y * a.tiles_x;
        const int64_t plane = ctx.bid / tiles;
        const int tile = (int)(ctx.bid - plane * tiles);
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int kh0 = ty * TH, kw0 = tx * TW;
        const int base = 1 - LT / 2;                               // wl_afb_base of periodization
        const int r0 = 2 * (2 * kh0 + base) + base, c0 = 2 * (2 * kw0 + base) + base;   // input position of the footprint's corner
        float* S = reinterpret_cast<float*>(ctx.smem);             // [N0R][N0C], later T2
        wl_f2* T2 = reinterpret_cast<wl_f2*>(S);                   // [4][N1R][TW]
        wl_f2* T1 = reinterpret_cast<wl_f2*>(S + kX);              // [N0R][N1C]
        float* B1 = S + kX + kT1;                                  // [4][N1R][N1C]
        const T* xp = a.x + plane * a.x_ps;
        for (int f = tid; f < kS; f += kThreads) {
            const int i = f / N0C, c = f - i * N0C;
            S[f] = (float)xp[wl_pmod(r0 + i, a.H) * a.x_rs + wl_pmod(c0 + c, a.W)];
        }
        ctx.sync();
        float hw0[LT], hw1[LT], hh0[LT], hh1[LT];
#pragma unroll
        for (int j = 0; j < LT; ++j) { hw0[j] = a.h_w_lo[j]; hw1[j] = a.h_w_hi[j]; hh0[j] = a.h_h_lo[j]; hh1[j] = a.h_h_hi[j]; }
        // level 1 along W: (lo, hi) of every footprint row
        for (int f = tid; f < N0R * N1C; f += kThreads) {
            const int i = f / N1C, k = f - i * N1C;
            const float* src = S + i * N0C + 2 * k;
            float lo = 0.f, hi = 0.f;
#pragma unroll
            for (int j = 0; j < LT; ++j) { lo += hw0[j] * src[j]; hi += hw1[j] * src[j]; }
            wl_f2 o; o.x = lo; o.y = hi;
            T1[f] = o;
        }
        ctx.sync();
        // level 1 along H: the four level-1 bands
        for (int f = tid; f < N1R * N1C; f += kThreads) {
            const int r = f / N1C, k = f - r * N1C;
            const wl_f2* col = T1 + 2 * r * N1C + k;
            float ll = 0.f, lh = 0.f, hl = 0.f, hh = 0.f;
#pragma unroll
            for (int j = 0; j < LT; ++j) {
                const wl_f2 v = col[j * N1C];
                ll += hh0[j] * v.x; lh += hh1[j] * v.x;
                hl += hh0[j] * v.y; hh += hh1[j] * v.y;
            }
            B1[f] = ll; B1[N1R * N1C + f] = lh; B1[2 * N1R * N1C + f] = hl; B1[3 * N1R * N1C + f] = hh;
        }
        ctx.sync();
        // level 2 along W: (lo, hi) of every row of the four level-1 bands (the rows of the bands lie one after the other)
        for (int f = tid; f < 4 * N1R * TW; f += kThreads) {
            const int i = f / TW, k = f - i * TW;
            const float* src = B1 + i * N1C + 2 * k;
            float lo = 0.f, hi = 0.f;
#pragma unroll
            for (int j = 0; j < LT; ++j) { lo += hw0[j] * src[j]; hi += hw1[j] * src[j]; }
            wl_f2 o; o.x = lo; o.y = hi;
            T2[f] = o;
        }
        ctx.sync();
        // level 2 along H + the 16 band stores: band 4 s1 + s2
        const int64_t bplane = (int64_t)a.Kh * a.Kw;
        for (int f = tid; f < 4 * TH * TW; f += kThreads) {
            const int s1 = f / (TH * TW), g = f - s1 * (TH * TW);
            const int kh = g / TW, kw = g - kh * TW;
            const int k = kh0 + kh, kc = kw0 + kw;
            if (k >= a.Kh || kc >= a.Kw) continue;
            const wl_f2* col = T2 + (s1 * N1R + 2 * kh) * TW + kw;
            float ll = 0.f, lh = 0.f, hl = 0.f, hh = 0.f;
#pragma unroll
            for (int j = 0; j < LT; ++j) {
                const wl_f2 v = col[j * TW];
                ll += hh0[j] * v.x; lh += hh1[j] * v.x;
                hl += hh0[j] * v.y; hh += hh1[j] * v.y;
            }
            T* dst = a.y + (plane * 16 + 4 * s1) * bplane + (k * a.Kw + kc);
            dst[0] = (T)ll; dst[bplane] = (T)lh; dst[2 * bplane] = (T)hl; dst[3 * bplane] = (T)hh;
        }
    }
};

// Synthesis, the mirror image: a tile of XH x XW = 32 x 64 samples of x needs N1 = X / 2 + L / 2 samples of each level-1 band per
// axis (origin A1) and N2 = (N1 + 1) / 2 + L / 2 of each level-2 band (origin A2, wrapped at staging).  Four banks in output pairs,
// as in the one-level kernel.  LDS: the 16 band tiles, the (lo, hi) rows of level 2, the four level-1 bands; the (lo, hi) rows of
// level 1 reuse the band tiles' words.  14 544 floats at 12 taps.
template <typename T, int LT>
struct WlWptSfb<T, LT, 2> {
    typedef WlWptSfbArgs<T> Args;          // Kh / Kw: the LEVEL-2 band size; y (planes, 16, Kh, Kw); OH = 4 Kh, OW = 4 Kw
    static const int kThreads = 256;
    static const int kMinWaves = 2;
    static const int HL = LT / 2, SH = HL - 1;                     // taps per phase, the shift s of periodization
    static const int XH = 32, XW = 64;
    static const int N1R = XH / 2 + HL, N1C = XW / 2 + HL;
    static const int N2R = (N1R + 1) / 2 + HL, N2C = (N1C + 1) / 2 + HL;
    static const int kZ = 16 * N2R * N2C, kU1 = 2 * XH * N1C;
    static const int kX = kZ > kU1 ? kZ : kU1;
    static const int kU2 = 8 * N1R * N2C, kB1 = 4 * N1R * N1C;
    static const int kLdsFloats = kX + kU2 + kB1;

    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int tid = ctx.tid;
        const int tiles = a.tiles_y * a.tiles_x;
        const int64_t plane = ctx.bid / tiles;
        const int tile = (int)(ctx.bid - plane * tiles);
        const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int n0 = ty * XH, w0 = tx * XW;
        const int a1r = ((n0 + SH) >> 1) - (HL - 1), a1c = ((w0 + SH) >> 1) - (HL - 1);     // level-1 origin (>= -(HL - 1))
        const int a2r = ((a1r + SH) >> 1) - (HL - 1), a2c = ((a1c + SH) >> 1) - (HL - 1);   // level-2 origin (may be negative)
        float* Z = reinterpret_cast<float*>(ctx.smem);             // [16][N2R][N2C], later U1
        wl_f2* U1 = reinterpret_cast<wl_f2*>(Z);                   // [XH][N1C]
        wl_f2* U2 = reinterpret_cast<wl_f2*>(Z + kX);              // [4][N1R][N2C]
        float* B1 = Z + kX + kU2;                                  // [4][N1R][N1C]
        const int64_t bplane = (int64_t)a.Kh * a.Kw;
        const T* yp = a.y + plane * 16 * bplane;
        for (int f = tid; f < kZ; f += kThreads) {
            const int b = f / (N2R * N2C), g = f - b * (N2R * N2C);
            const int i = g / N2C, j = g - i * N2C;
            Z[f] = (float)yp[b * bplane + (wl_pmod(a2r + i, a.Kh) * a.Kw + wl_pmod(a2c + j, a.Kw))];
        }
        ctx.sync();
        float gw0[LT], gw1[LT], gh0[LT], gh1[LT];
#pragma unroll
        for (int t = 0; t < LT; ++t) { gw0[t] = a.g_w_lo[t]; gw1[t] = a.g_w_hi[t]; gh0[t] = a.g_h_lo[t]; gh1[t] = a.g_h_hi[t]; }
        // level 2 along H: level-1 rows 2 q + i0, + 1 of (W-lo, W-hi) for each of the four level-1 bands
        {
            const int NPR = N1R / 2 + 1;
            const int i0 = 2 * ((a1r + SH) >> 1) - SH - a1r;          // 0 or -1
            for (int f = tid; f < 4 * NPR * N2C; f += kThreads) {
                const int s1 = f / (NPR * N2C), g = f - s1 * (NPR * N2C);
                const int q = g / N2C, j = g - q * N2C;
                const float* b = Z + ((4 * s1) * N2R + (q + HL - 1)) * N2C + j;
                float le = 0.f, he = 0.f, lo = 0.f, ho = 0.f;
#pragma unroll
                for (int u = 0; u < HL; ++u) {
                    const float* r = b - u * N2C;
                    const float b0 = r[0], b1 = r[N2R * N2C], b2 = r[2 * N2R * N2C], b3 = r[3 * N2R * N2C];
                    le += gh0[2 * u] * b0;     le += gh1[2 * u] * b1;
                    he += gh0[2 * u] * b2;     he += gh1[2 * u] * b3;
                    lo += gh0[2 * u + 1] * b0; lo += gh1[2 * u + 1] * b1;
                    ho += gh0[2 * u + 1] * b2; ho += gh1[2 * u + 1] * b3;
                }
                const int i1 = i0 + 2 * q;
                const int d = (s1 * N1R + i1) * N2C + j;
                if (i1 >= 0 && i1 < N1R) { wl_f2 o; o.x = le; o.y = he; U2[d] = o; }
                if (i1 + 1 < N1R) { wl_f2 o; o.x = lo; o.y = ho; U2[d + N2C] = o; }
            }
        }
        ctx.sync();
        // level 2 along W: the four level-1 bands
        {
            const int NPC = N1C / 2 + 1;
            const int j0 = 2 * ((a1c + SH) >> 1) - SH - a1c;
            for (int f = tid; f < 4 * N1R * NPC; f += kThreads) {
                const int row = f / NPC, q = f - row * NPC;           // row = s1 * N1R + i1
                const wl_f2* r = U2 + row * N2C + (q + HL - 1);
                float ye = 0.f, yo = 0.f;
#pragma unroll
                for (int u = 0; u < HL; ++u) {
                    const wl_f2 v = r[-u];
                    ye += gw0[2 * u] * v.x;     ye += gw1[2 * u] * v.y;
                    yo += gw0[2 * u + 1] * v.x; yo += gw1[2 * u + 1] * v.y;
                }
                const int j1 = j0 + 2 * q;
                if (j1 >= 0 && j1 < N1C) B1[row * N1C + j1] = ye;
                if (j1 + 1 < N1C) B1[row * N1C + j1 + 1] = yo;
            }
        }
        ctx.sync();
        // level 1 along H
        {
            const int NPR = XH / 2 + 1;
            const int nl0 = 2 * ((n0 + SH) >> 1) - SH - n0;
            for (int f = tid; f < NPR * N1C; f += kThreads) {
                const int q = f / N1C, j = f - q * N1C;
                const float* b = B1 + (q + HL - 1) * N1C + j;
                float le = 0.f, he = 0.f, lo = 0.f, ho = 0.f;
#pragma unroll
                for (int u = 0; u < HL; ++u) {
                    const float* r = b - u * N1C;
                    const float b0 = r[0], b1 = r[N1R * N1C], b2 = r[2 * N1R * N1C], b3 = r[3 * N1R * N1C];
                    le += gh0[2 * u] * b0;     le += gh1[2 * u] * b1;
                    he += gh0[2 * u] * b2;     he += gh1[2 * u] * b3;
                    lo += gh0[2 * u + 1] * b0; lo += gh1[2 * u + 1] * b1;
                    ho += gh0[2 * u + 1] * b2; ho += gh1[2 * u + 1] * b3;
                }
                const int nl = nl0 + 2 * q;
                const int d = nl * N1C + j;
                if (nl >= 0 && nl < XH) { wl_f2 o; o.x = le; o.y = he; U1[d] = o; }
                if (nl + 1 < XH) { wl_f2 o; o.x = lo; o.y = ho; U1[d + N1C] = o; }
            }
        }
        ctx.sync();
        // level 1 along W + store
        {
            const int NPC = XW / 2 + 1;
            const int wl0 = 2 * ((w0 + SH) >> 1) - SH - w0;
            T* xp = a.x + plane * ((int64_t)a.OH * a.OW);
            for (int f = tid; f < XH * NPC; f += kThreads) {
                const int nl = f / NPC, q = f - nl * NPC;
                const int n = n0 + nl;
                if (n >= a.OH) continue;
                const wl_f2* r = U1 + nl * N1C + (q + HL - 1);
                float ye = 0.f, yo = 0.f;
#pragma unroll
                for (int u = 0; u < HL; ++u) {
                    const wl_f2 v = r[-u];
                    ye += gw0[2 * u] * v.x;     ye += gw1[2 * u] * v.y;
                    yo += gw0[2 * u + 1] * v.x; yo += gw1[2 * u + 1] * v.y;
                }
                const int wl = wl0 + 2 * q, w = w0 + wl;
                T* row = xp + n * a.OW;
                if (wl >= 0 && wl < XW && w < a.OW) row[w] = (T)ye;
                if (wl + 1 < XW && w + 1 < a.OW) row[w + 1] = (T)yo;
            }
        }
    }
};
