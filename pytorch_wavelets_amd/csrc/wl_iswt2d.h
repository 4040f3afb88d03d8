// The TRANSPOSE of one level of the 2-D stationary analysis bank (wl_swt2d.h) in ONE launch: the four sub-bands of a
// (planes, 4, H, W) tensor are read once, one (planes, H, W) plane is written once.  It is two things at once:
//   * the backward of afb2d_atrous / SWTForward's level (what autograd derives upstream from mypad + conv2d,
//     dwt/lowlevel.py:475-521), scale = 1;
//   * one level of the inverse stationary transform (the intent of dwt/swt_inverse.py, which upstream never finished): with the
//     synthesis taps g as the bank and periodic extension, x = 1/4 sum_{r,b} A_r(g)^T A_b(g)^T y[4c + 2r + b], scale = 1/4.
// With A_b the n x n matrix of the analysis along an axis, y_b[k] = sum_t h_b[t] X(k - s + d t), s = (L d) / 2 - d, the
// transpose of the 'periodic' and of the 'zero' rule is again a correlation with one source sample per tap - every (m, t) has
// exactly one k in [0, n) with ext(k - s + d t) == m, however often the pad wraps round the signal:
//     dx[m] = sum_b sum_t h_b[t] Y_b(m + s - d t)              Y_b = dy_b under the SAME rule (wrap / zeros)
// so the kernel is the forward's mirror image: taps reversed, first sample at m + s - d (L - 1) = m - (L d) / 2.  The mirror
// and replicate rules fold several extended samples onto one and are left to the single-axis kernel (WlCorr1dAdj).
// A workgroup owns a TH x 64 tile of dx.  The bands are staged in turn, by their band along H: for b = 0, 1 the extended
// tiles of the pair (y[2*0 + b], y[2*1 + b]) go to LDS side by side, the filter along W sums them into one value per staged
// row and output column; the filter along H then reads those (b = 0, b = 1) pairs back.  LDS holds two planes' worth of
// halo'd tile plus the pairs - not the four a staging of all bands at once would need.
// The ll band (channel 4c + 0) may come from / be joined by a separate plane `ll` (plane stride ll_ps, rows dense):
//   ll_mode 1 (replace): channel 4c + 0 is read from `ll` - the inverse feeds the reconstructed ll of the coarser level;
//   ll_mode 2 (add):     `ll` is added to channel 4c + 0 - the backward of level j takes dx of level j + 1 this way;
// and y itself may be NULL with ll_mode 1 (the other three bands are zeros: an unused level in a backward).
#pragma once
#include "wl_common.h"
#include "wl_filt1d.h"

template <typename T>
struct WlSwtInvArgs {
    typedef typename WlAcc<T>::type A;
    const T* y;                    // (planes, 4, H, W) through y_ps (the four bands of a plane dense), or nullptr
    const T* ll;                   // (planes, H, W) through ll_ps, or nullptr
    T* x;                          // (planes, H, W) dense
    const A* hw0; const A* hw1;    // taps along W (low, high), Lw each - as the analysis stores them
    const A* hh0; const A* hh1;    // taps along H, Lh each
    A scale;
    int64_t planes, y_ps, ll_ps, nblocks;
    int H, W, Lw, Lh, d, ext, ll_mode;
    int sw, sh;                    // first extended column / row a tile reads relative to its output: -((L d) / 2)
    int TH, tiles_x, tiles_y;
    int in_pitch;                  // pairs per row of the staged tile
    int mid_off;                   // byte offset of the row-filtered pairs in LDS
    int lds_bytes;
};

// LT = compile-time tap count of both axes, 0 = any (Lw, Lh) at run time
template <typename T, int LT>
struct WlSwtInvLevel {
    typedef WlSwtInvArgs<T> Args;
    typedef typename WlAcc<T>::type A;
    static const int kThreads = 256;
    static const int kMinWaves = 2;
    static const int TW = 64;
    struct Pair { A p, q; };
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int tx = ctx.tid & 63, ty = ctx.tid >> 6;
        const int per_plane = a.tiles_x * a.tiles_y;
        const int64_t plane = ctx.bid / per_plane;
        const int rem = (int)(ctx.bid - plane * per_plane);
        const int tyi = rem / a.tiles_x, txi = rem - tyi * a.tiles_x;
        const int r0 = tyi * a.TH, c0 = txi * TW;
        const int Lw = LT ? LT : a.Lw, Lh = LT ? LT : a.Lh, d = a.d;
        const int hw = (Lw - 1) * d, hh = (Lh - 1) * d;
        const int th = r0 + a.TH <= a.H ? a.TH : a.H - r0;
        const int tw = c0 + TW <= a.W ? TW : a.W - c0;
        const int rows = th + hh, cols = tw + hw;
        const size_t per = (size_t)a.H * a.W;
        Pair* const in = reinterpret_cast<Pair*>(ctx.smem);
        Pair* const mid = reinterpret_cast<Pair*>(ctx.smem + a.mid_off);
        const T* const yp = a.y ? a.y + (size_t)plane * a.y_ps : nullptr;
        const T* const lp = a.ll ? a.ll + (size_t)plane * a.ll_ps : nullptr;
        A w0[LT ? LT : 1], w1[LT ? LT : 1];       // reversed: tap u of the mirror-image correlation = stored tap L - 1 - u
        if (LT) {
#pragma unroll
            for (int t = 0; t < (LT ? LT : 1); ++t) { w0[t] = a.hw0[LT - 1 - t]; w1[t] = a.hw1[LT - 1 - t]; }
        }
        for (int b = 0; b < 2; ++b) {
            // ---- the extended tiles of the pair (band 2*0 + b, band 2*1 + b): rows r0 + sh .., columns c0 + sw ..
            // (eight rows of a column at a time: the loads of a batch are in flight together, as in the forward)
            const T* p0 = yp ? yp + (size_t)b * per : nullptr;          // band along W = 0
            const T* const p1 = yp ? yp + (size_t)(2 + b) * per : nullptr;
            const T* padd = nullptr;
            if (b == 0 && a.ll_mode == 1) p0 = lp;
            if (b == 0 && a.ll_mode == 2) padd = lp;
            for (int c = tx; c < cols; c += 64) {
                const int gc = wl_ext_any(c0 + a.sw + c, a.W, a.ext);
                for (int rb = ty; rb < rows; rb += 32) {
                    T v0[8], v1[8], v2[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int r = rb + 4 * u;
                        const int gr = r < rows ? wl_ext_any(r0 + a.sh + r, a.H, a.ext) : -1;
                        const bool off = gr < 0 || gc < 0;
                        const size_t o = off ? 0 : (size_t)gr * a.W + gc;
                        v0[u] = (off || !p0) ? (T)0 : p0[o];
                        v1[u] = (off || !p1) ? (T)0 : p1[o];
                        v2[u] = (off || !padd) ? (T)0 : padd[o];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int r = rb + 4 * u;
                        if (r < rows) {
                            Pair s; s.p = (A)v0[u] + (A)v2[u]; s.q = (A)v1[u];
                            in[r * a.in_pitch + c] = s;
                        }
                    }
                }
            }
            ctx.sync();
            // ---- filter along W: one value per staged row and output column, the two bands along W summed
            if (tx < tw) {
                for (int r = ty; r < rows; r += 4) {
                    const Pair* p = in + r * a.in_pitch + tx;
                    A acc = 0;
                    if (LT) {
#pragma unroll
                        for (int t = 0; t < (LT ? LT : 1); ++t) { const Pair s = p[t * d]; acc += w0[t] * s.p; acc += w1[t] * s.q; }
                    } else {
                        for (int t = 0; t < Lw; ++t) { const Pair s = p[t * d]; acc += a.hw0[Lw - 1 - t] * s.p; acc += a.hw1[Lw - 1 - t] * s.q; }
                    }
                    if (b == 0) mid[r * TW + tx].p = acc; else mid[r * TW + tx].q = acc;
                }
            }
            ctx.sync();      // the staged tile is free for the second pair; after it, the pairs of `mid` are complete
        }
        // ---- filter along H, the two bands along H summed, and the scale
        if (tx < tw) {
            A v0[LT ? LT : 1], v1[LT ? LT : 1];
            if (LT) {
#pragma unroll
                for (int t = 0; t < (LT ? LT : 1); ++t) { v0[t] = a.hh0[LT - 1 - t]; v1[t] = a.hh1[LT - 1 - t]; }
            }
            T* const xp = a.x + (size_t)plane * per + (size_t)c0 + tx;
            for (int r = ty; r < th; r += 4) {
                const Pair* p = mid + r * TW + tx;
                A acc = 0;
                if (LT) {
#pragma unroll
                    for (int t = 0; t < (LT ? LT : 1); ++t) { const Pair s = p[t * d * TW]; acc += v0[t] * s.p; acc += v1[t] * s.q; }
                } else {
                    for (int t = 0; t < Lh; ++t) { const Pair s = p[t * d * TW]; acc += a.hh0[Lh - 1 - t] * s.p; acc += a.hh1[Lh - 1 - t] * s.q; }
                }
                xp[(size_t)(r0 + r) * a.W] = (T)(a.scale * acc);
            }
        }
    }
};
