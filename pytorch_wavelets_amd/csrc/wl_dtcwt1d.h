// 1-D dual-tree complex wavelet transform along the last axis of dense (rows, n) tensors: up to four levels of the analysis
// (WlDt1dFwd) or of the synthesis (WlDt1dInv) in ONE launch, every intermediate lowpass in LDS.  The level structure is the
// 2-D transform's carried to one axis (reference dtcwt/transform2d.py:117-133, :235-236; transform_funcs.py:237-238, :361-488):
//   level 1      lo = colfilter(x, h0o), hi = colfilter(x, h1o) at full rate (odd-length taps), an odd input gets a copy of its
//                last sample first;
//   level j >= 2 (lo, hi) = coldfilt(lo, ..): the pair k = (Ya[k], Yb[k]) of both filters reads the samples 4k + 2t + {2, 3} - m
//                of the lowpass, which is first padded by one replicated sample either side where its length is no multiple of 4.
// The highpass of a level IS the complex band: (hi[2k], hi[2k+1]) = (real, imaginary) - the kernels write / read the
// (rows, L_j, 2) tensors as flat rows.
//
// Cells.  A level buffer in LDS holds float32 "cells" in EXTENDED PADDED coordinates e of the signal it carries: padded
// position p = e inside [0, np), np = n + 2 with end padding (cell p holds sample clamp(p - 1)), and the half-sample
// symmetric images -1 - p and 2 np - 1 - p outside.  Whoever produces a sample stores it into every cell of the chunk's
// range that shows it (the loader through wl_dt1d_src, a level through `put`: at most the cell, its pad twin and one image
// each) - so NO filter tap ever tests a boundary, the padding is an index shift at store time, and the sum of an output runs
// over its taps in one order whatever chunk it falls in: chunk seams do not change a bit.
//
// Layout (q-shift levels, m = 10 / 14 / 18 taps, all with m = 2 mod 4): a buffer's cell 0 sits at a position that is a
// multiple of 4, so the 2m samples of pair k start at the 16-byte aligned cell 4k + 2 - m: m / 2 ds_read_b128 per pair, each
// the (even, odd) samples of two taps for both trees; neighbouring lanes are 16 bytes apart - conflict-free for 16-byte reads
// (4-way for 4-byte, 2-way for 8-byte ones).  The synthesis reads (even, odd) pairs, lanes 8 bytes apart: 8-byte reads.
// Level-1 lanes own single outputs (4-byte reads, lanes 4 bytes apart).
#pragma once
#include "wl_common.h"

#define WL_DT1D_MAXJ 4
#ifndef WL_DT1D_SPAN
#define WL_DT1D_SPAN 4096          // input samples per chunk of the analysis (not measured against other sizes)
#endif
#ifndef WL_DT1D_INV_CHUNK
#define WL_DT1D_INV_CHUNK 2048     // output samples per chunk of the synthesis (not measured against other sizes)
#endif
#define WL_DT1D_MAXL1 20           // level-1 taps (odd lengths up to 19)

// end rules of a level's INPUT in the analysis
#define WL_DT1D_PAD_NONE 0
#define WL_DT1D_PAD_REPL 1         // [x[0], x, x[-1]]     (the forward transform)
#define WL_DT1D_PAD_ZERO 2         // [0, x, 0]            (backward of a synthesis level that cropped)
#define WL_DT1D_PAD_LAST 3         // [x, x[-1]]           (an odd input of level 1)
// end rules of a level's OUTPUT in the synthesis
#define WL_DT1D_RULE_NONE 0
#define WL_DT1D_RULE_CROP 1        // y[1:-1]                                  (the inverse transform)
#define WL_DT1D_RULE_FOLD 2        // y[1:-1] with y[0], y[-1] added to the ends (backward of an analysis level that padded);
                                   // level 1: y[:-1] with y[-1] added to the last sample (backward of the odd input's copy)

WL_HD int wl_dt1d_padded_len(int n, int pad) {
    return n + (pad == WL_DT1D_PAD_REPL || pad == WL_DT1D_PAD_ZERO ? 2 : pad == WL_DT1D_PAD_LAST ? 1 : 0);
}
// source sample of cell e of a signal of n samples under `pad` (-1: a zero)
WL_HD int wl_dt1d_src(int e, int n, int pad) {
    int p = wl_ext(e, wl_dt1d_padded_len(n, pad), WL_EXT_SYM);
    if (pad == WL_DT1D_PAD_REPL) { p -= 1; return p < 0 ? 0 : (p >= n ? n - 1 : p); }
    if (pad == WL_DT1D_PAD_ZERO) { p -= 1; return (unsigned)p < (unsigned)n ? p : -1; }
    if (pad == WL_DT1D_PAD_LAST) return p >= n ? n - 1 : p;
    return p;
}
// the positions [a, b) of a signal of np samples that the cells [ca, cb) show (one fold either side)
WL_HD void wl_dt1d_shown(int ca, int cb, int np, int& a, int& b) {
    a = ca < 0 ? 0 : ca;
    b = cb > np ? np : cb;
    if (ca < 0) { const int m = -ca < np ? -ca : np; if (m > b) b = m; }
    if (cb > np) { const int m = 2 * np - cb > 0 ? 2 * np - cb : 0; if (m < a) a = m; }
}
WL_HD int wl_dt1d_floor4(int v) { return v >= 0 ? v & ~3 : -((-v + 3) & ~3); }
WL_HD int wl_dt1d_min(int a, int b) { return a < b ? a : b; }
WL_HD int wl_dt1d_max(int a, int b) { return a > b ? a : b; }

// one sample into every cell of [clo, chi) that shows padded position p of a signal of np padded samples
WL_DEV void wl_dt1d_put(float* buf, int org, int clo, int chi, int np, int p, float v) {
    if (p >= clo && p < chi) buf[p - org] = v;
    const int e1 = -1 - p, e2 = 2 * np - 1 - p;
    if (e1 >= clo && e1 < chi) buf[e1 - org] = v;
    if (e2 >= clo && e2 < chi) buf[e2 - org] = v;
}

// ---------------------------------------------------------------------------------------------------------------- analysis
struct WlDt1dFwdShape {
    int J, qstart;                     // levels of this launch; qstart: its first level is a q-shift level already
    int M, Mx;                         // q-shift taps; max(L0, L1) / 2 of level 1
    int n[WL_DT1D_MAXJ + 1];           // n[0] = input samples, n[l] = outputs of level l (lowpass = highpass length)
    int pad[WL_DT1D_MAXJ];             // end rule of the input of level l + 1
    int chunk, nchunks;                // pairs of the coarsest level per chunk, chunks per row
};
// per chunk: level l = 1 .. J computes the output pairs [klo, khi) and stores those of [olo, ohi) to memory; buffer b = 0 .. J - 1
// (the input of level b + 1) holds the cells [clo, chi), cell `org` (a multiple of 4) first
struct WlDt1dFwdGeo {
    int klo[WL_DT1D_MAXJ + 1], khi[WL_DT1D_MAXJ + 1], olo[WL_DT1D_MAXJ + 1], ohi[WL_DT1D_MAXJ + 1];
    int clo[WL_DT1D_MAXJ], chi[WL_DT1D_MAXJ], org[WL_DT1D_MAXJ];
};
WL_HD int wl_dt1d_fwd_pairs(const WlDt1dFwdShape& s, int l) {
    const int np = wl_dt1d_padded_len(s.n[l - 1], s.pad[l - 1]);
    return l == 1 && !s.qstart ? np >> 1 : np >> 2;
}
WL_HD void wl_dt1d_fwd_geometry(const WlDt1dFwdShape& s, int c, WlDt1dFwdGeo& g) {
    const bool last = c == s.nchunks - 1;
    for (int l = s.J; l >= 1; --l) {
        const int K = wl_dt1d_fwd_pairs(s, l), sft = s.J - l;
        const int64_t b0 = ((int64_t)c * s.chunk) << sft, b1 = ((int64_t)(c + 1) * s.chunk) << sft;
        const int olo = b0 < K ? (int)b0 : K, ohi = last || b1 > K ? K : (int)b1;
        int klo = olo, khi = ohi;
        if (l < s.J && g.chi[l] > g.clo[l]) {
            // the outputs the cells of the next level's input show
            const int n = s.n[l], pad = s.pad[l], sh = pad == WL_DT1D_PAD_REPL || pad == WL_DT1D_PAD_ZERO ? 1 : 0;
            int a, b;
            wl_dt1d_shown(g.clo[l], g.chi[l], n + 2 * sh, a, b);
            const int tlo = wl_dt1d_min(wl_dt1d_max(a - sh, 0), n - 1), thi = wl_dt1d_min(wl_dt1d_max(b - 1 - sh, 0), n - 1) + 1;
            const int k0 = tlo >> 1, k1 = (thi + 1) >> 1;
            if (khi <= klo) { klo = k0; khi = k1; } else { klo = wl_dt1d_min(klo, k0); khi = wl_dt1d_max(khi, k1); }
        }
        g.klo[l] = klo; g.khi[l] = khi; g.olo[l] = olo; g.ohi[l] = ohi;
        int ca = 0, cb = 0;
        if (khi > klo) {
            if (l == 1 && !s.qstart) { ca = 2 * klo - s.Mx; cb = 2 * khi + s.Mx; }
            else { ca = 4 * klo + 2 - s.M; cb = 4 * (khi - 1) + s.M + 2; }
        }
        g.clo[l - 1] = ca; g.chi[l - 1] = cb; g.org[l - 1] = wl_dt1d_floor4(ca);
    }
}

template <typename T>
struct WlDt1dFwdArgs {
    const T* x;                        // (rows, n[0]) dense
    T* hi[WL_DT1D_MAXJ];               // (rows, n[l]) dense = (rows, n[l] / 2, 2): highpass of level l, or null (skipped)
    T* lo[WL_DT1D_MAXJ];               // (rows, n[l]) dense: lowpass of level l, or null; the last level's is always written
    const float* h0o; const float* h1o; int L0, L1;                        // level 1 (stored taps)
    const float* h0a; const float* h0b; const float* h1a; const float* h1b;   // q-shift levels, M taps each
    int64_t rows, nblocks;
    WlDt1dFwdShape s;
    int buf_off[WL_DT1D_MAXJ], geo_off, lds_bytes;
};

template <typename T, int M>
struct WlDt1dFwd {
    typedef WlDt1dFwdArgs<T> Args;
    static const int kThreads = 256;
    static const int kMinWaves = 2;
    typedef T Pair2 __attribute__((ext_vector_type(2), aligned(sizeof(T)), may_alias));

    // output q of a level -> the cells of the next level's input
    static WL_DEV void emit(float* buf, int org, int clo, int chi, int n, int pad, int q, float v) {
        const int sh = pad == WL_DT1D_PAD_REPL || pad == WL_DT1D_PAD_ZERO ? 1 : 0, np = n + 2 * sh;
        wl_dt1d_put(buf, org, clo, chi, np, q + sh, v);
        if (sh) {
            const float w = pad == WL_DT1D_PAD_REPL ? v : 0.f;
            if (q == 0) wl_dt1d_put(buf, org, clo, chi, np, 0, w);
            if (q == n - 1) wl_dt1d_put(buf, org, clo, chi, np, np - 1, w);
        }
    }

    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int tid = ctx.tid;
        const WlDt1dFwdShape& s = a.s;
        const int64_t row = ctx.bid / s.nchunks;
        const int c = (int)(ctx.bid - row * s.nchunks);
        // the chunk's ranges: worked out once, by one lane, into LDS (arrays indexed by the level: in registers they would be scratch)
        const WlDt1dFwdGeo& g = *reinterpret_cast<const WlDt1dFwdGeo*>(ctx.smem + a.geo_off);
        if (tid == 0) wl_dt1d_fwd_geometry(s, c, *reinterpret_cast<WlDt1dFwdGeo*>(ctx.smem + a.geo_off));
        ctx.sync();
        {   // ---- the input samples the chunk depends on, end rules resolved here
            float* const b0 = reinterpret_cast<float*>(ctx.smem + a.buf_off[0]);
            const int n0 = s.n[0], pad0 = s.pad[0], clo = g.clo[0], chi = g.chi[0], org = g.org[0];
            const int sh = pad0 == WL_DT1D_PAD_REPL || pad0 == WL_DT1D_PAD_ZERO ? 1 : 0;
            const T* const xr = a.x + (size_t)row * n0;
            for (int e = clo + tid; e < chi; e += kThreads) {
                const int q = (unsigned)(e - sh) < (unsigned)n0 ? e - sh : wl_dt1d_src(e, n0, pad0);
                b0[e - org] = q < 0 ? 0.f : (float)xr[q];
            }
        }
        ctx.sync();
        float qa[M], qb[M], ra[M], rb[M];                          // h0a, h0b, h1a, h1b: scalar registers
        const bool qs = s.J > 1 || s.qstart;                       // (a lone level 1 has no q-shift taps)
#pragma unroll
        for (int t = 0; t < M; ++t) {
            qa[t] = wl_uniform_f(qs ? a.h0a[t] : 0.f); qb[t] = wl_uniform_f(qs ? a.h0b[t] : 0.f);
            ra[t] = wl_uniform_f(qs ? a.h1a[t] : 0.f); rb[t] = wl_uniform_f(qs ? a.h1b[t] : 0.f);
        }
        for (int l = 1; l <= s.J; ++l) {
            const float* const src = reinterpret_cast<const float*>(ctx.smem + a.buf_off[l - 1]);
            const int sorg = g.org[l - 1];
            const bool more = l < s.J;
            float* const dst = more ? reinterpret_cast<float*>(ctx.smem + a.buf_off[l]) : nullptr;
            const int dclo = more ? g.clo[l] : 0, dchi = more ? g.chi[l] : 0, dorg = more ? g.org[l] : 0, dpad = more ? s.pad[l] : 0;
            const int nl = s.n[l];
            const int klo = g.klo[l], khi = g.khi[l], olo = g.olo[l], ohi = g.ohi[l];
            T* const hp = a.hi[l - 1] ? a.hi[l - 1] + (size_t)row * nl : nullptr;
            T* const lp = a.lo[l - 1] ? a.lo[l - 1] + (size_t)row * nl : nullptr;
            if (l == 1 && !s.qstart) {
                // the two odd-length filters at full rate: a lane owns single outputs
                const int L0 = a.L0, L1 = a.L1, m0 = L0 >> 1, m1 = L1 >> 1;
                for (int i = 2 * klo + tid; i < 2 * khi; i += kThreads) {
                    const float* p0 = src + (i - m0 - sorg);
                    const float* p1 = src + (i - m1 - sorg);
                    float lo = 0.f, hi = 0.f;
                    for (int t = 0; t < L0; ++t) lo = __builtin_fmaf(a.h0o[t], p0[t], lo);
                    for (int t = 0; t < L1; ++t) hi = __builtin_fmaf(a.h1o[t], p1[t], hi);
                    if (dst) emit(dst, dorg, dclo, dchi, nl, dpad, i, lo);
                    if (i >= 2 * olo && i < 2 * ohi) {
                        if (hp) hp[i] = (T)hi;
                        if (lp) lp[i] = (T)lo;
                    }
                }
            } else {
                for (int k = klo + tid; k < khi; k += kThreads) {
                    const float* p = src + (4 * k + 2 - M - sorg);              // 16-byte aligned: M = 2 (mod 4), sorg = 0 (mod 4)
                    float le = 0.f, lo_ = 0.f, he = 0.f, ho = 0.f;
#pragma unroll
                    for (int u = 0; u < M / 2; ++u) {
                        const wl_vf4 w = *reinterpret_cast<const wl_vf4*>(p + 4 * u);   // (even, odd) samples of taps 2u, 2u + 1
                        le = __builtin_fmaf(qb[2 * u], w.x, le);   ho = __builtin_fmaf(rb[2 * u], w.x, ho);
                        lo_ = __builtin_fmaf(qa[2 * u], w.y, lo_); he = __builtin_fmaf(ra[2 * u], w.y, he);
                        le = __builtin_fmaf(qb[2 * u + 1], w.z, le);   ho = __builtin_fmaf(rb[2 * u + 1], w.z, ho);
                        lo_ = __builtin_fmaf(qa[2 * u + 1], w.w, lo_); he = __builtin_fmaf(ra[2 * u + 1], w.w, he);
                    }
                    if (dst) {
                        emit(dst, dorg, dclo, dchi, nl, dpad, 2 * k, le);
                        emit(dst, dorg, dclo, dchi, nl, dpad, 2 * k + 1, lo_);
                    }
                    if (k >= olo && k < ohi) {
                        if (hp) { Pair2 v; v.x = (T)he; v.y = (T)ho; *reinterpret_cast<Pair2*>(hp + 2 * k) = v; }
                        if (lp) { Pair2 v; v.x = (T)le; v.y = (T)lo_; *reinterpret_cast<Pair2*>(lp + 2 * k) = v; }
                    }
                }
            }
            ctx.sync();
        }
    }
};

// --------------------------------------------------------------------------------------------------------------- synthesis
// Level j >= 2 (colifilt, m / 2 odd):  y[4q + s] = sum_t f_s[t] lo(2(q + t) + 1 - m/2 + {0, 1, 0, 1}[s])
//                                                + sum_t F_s[t] hi(2(q + t) + 1 - m/2 + {1, 0, 1, 0}[s]),
// f = (g0b odd, g0a odd, g0b even, g0a even taps), F likewise of g1b / g1a; hi = the interleaved (real, imaginary) band.
// Level 1: y[i] = sum_t g0o[t] lo(i + t - L0/2) + sum_t g1o[t] hi(i + t - L1/2).
struct WlDt1dInvShape {
    int J, qstart;                     // levels of this launch; qstart: its finest level is a q-shift level
    int M, Mx;
    int n[WL_DT1D_MAXJ + 1];           // n[l] = samples of level l's inputs (lowpass after its end rule = interleaved highpass), l = 1 .. J
    int rule[WL_DT1D_MAXJ + 1];        // rule[l - 1]: end rule of level l's output (rule[0]: of y); rule[J]: CROP = the lowpass in memory has n[J] + 2 samples
    int n_lo, out_len;
    int chunk, nchunks;                // output samples per chunk, chunks per row
};
// per chunk: level l computes the outputs [q0, q1) (level 1: samples; q-shift levels: groups of four) from the cells [ca, cb)
// of its two inputs; the chunk stores the samples [o0, o1) of y
struct WlDt1dInvGeo { int q0[WL_DT1D_MAXJ + 1], q1[WL_DT1D_MAXJ + 1], ca[WL_DT1D_MAXJ + 1], cb[WL_DT1D_MAXJ + 1], o0, o1; };
WL_HD void wl_dt1d_inv_geometry(const WlDt1dInvShape& s, int c, WlDt1dInvGeo& g) {
    const int m2 = s.M >> 1;
    const int64_t e1 = (int64_t)(c + 1) * s.chunk;
    int t0 = c * s.chunk, t1 = e1 < s.out_len ? (int)e1 : s.out_len;     // samples needed of the level's output (after its end rule)
    g.o0 = t0; g.o1 = t1;
    for (int l = 1; l <= s.J; ++l) {
        const int rule = s.rule[l - 1], tn = l == 1 ? s.out_len : s.n[l - 1];
        int q0 = 0, q1 = 0, ca = 0, cb = 0;
        if (t1 > t0) {
            if (l == 1 && !s.qstart) {
                q0 = t0; q1 = t1 + (rule == WL_DT1D_RULE_FOLD && t1 == tn ? 1 : 0);
                ca = q0 - s.Mx; cb = q1 + s.Mx;
            } else {
                const int sh = rule != WL_DT1D_RULE_NONE ? 1 : 0;
                int r0 = t0 + sh, r1 = t1 + sh;
                if (rule == WL_DT1D_RULE_FOLD) { if (t0 == 0) r0 = 0; if (t1 == tn) r1 = 2 * s.n[l]; }
                q0 = r0 >> 2; q1 = (r1 + 3) >> 2;
                ca = 2 * q0 + 1 - m2; cb = 2 * q1 + m2 - 1;
            }
        }
        g.q0[l] = q0; g.q1[l] = q1; g.ca[l] = ca; g.cb[l] = cb;
        if (cb > ca) wl_dt1d_shown(ca, cb, s.n[l], t0, t1); else t0 = t1 = 0;
    }
}

template <typename T>
struct WlDt1dInvArgs {
    const T* lo;                       // (rows, n_lo) dense: the coarsest lowpass
    const T* hi[WL_DT1D_MAXJ];         // (rows, n[l]) dense = (rows, n[l] / 2, 2), or null = zeros
    T* y;                              // (rows, out_len) dense
    const float* g0o; const float* g1o; int L0, L1;
    const float* g0a; const float* g0b; const float* g1a; const float* g1b;
    int64_t rows, nblocks;
    WlDt1dInvShape s;
    int lo_off[WL_DT1D_MAXJ + 1], hi_off[WL_DT1D_MAXJ + 1], geo_off, lds_bytes;
};

template <typename T, int M>
struct WlDt1dInv {
    typedef WlDt1dInvArgs<T> Args;
    static const int kThreads = 256;
    static const int kMinWaves = 2;
    static const int M2 = M / 2;

    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        const int tid = ctx.tid;
        const WlDt1dInvShape& s = a.s;
        const int64_t row = ctx.bid / s.nchunks;
        const int c = (int)(ctx.bid - row * s.nchunks);
        const WlDt1dInvGeo& g = *reinterpret_cast<const WlDt1dInvGeo*>(ctx.smem + a.geo_off);
        if (tid == 0) wl_dt1d_inv_geometry(s, c, *reinterpret_cast<WlDt1dInvGeo*>(ctx.smem + a.geo_off));
        ctx.sync();
        // ---- every coefficient the chunk needs, symmetric images included (null band: zeros)
        for (int l = 1; l <= s.J; ++l) {
            const int ca = g.ca[l], cb = g.cb[l], n = s.n[l];
            float* const hb = reinterpret_cast<float*>(ctx.smem + a.hi_off[l]);
            const T* const hr = a.hi[l - 1] ? a.hi[l - 1] + (size_t)row * n : nullptr;
            for (int e = ca + tid; e < cb; e += kThreads) {
                const int p = (unsigned)e < (unsigned)n ? e : wl_ext(e, n, WL_EXT_SYM);
                hb[e - ca] = hr ? (float)hr[p] : 0.f;
            }
            if (l == s.J) {
                float* const lb = reinterpret_cast<float*>(ctx.smem + a.lo_off[l]);
                const T* const lr = a.lo + (size_t)row * s.n_lo + (s.rule[l] == WL_DT1D_RULE_CROP ? 1 : 0);
                for (int e = ca + tid; e < cb; e += kThreads) {
                    const int p = (unsigned)e < (unsigned)n ? e : wl_ext(e, n, WL_EXT_SYM);
                    lb[e - ca] = (float)lr[p];
                }
            }
        }
        ctx.sync();
        float f0[M], f1[M], F0[M], F1[M];                         // g0b, g0a, g1b, g1a: scalar registers
        const bool qs = s.J > 1 || s.qstart;                      // (a lone level 1 has no q-shift taps)
#pragma unroll
        for (int t = 0; t < M; ++t) {
            f0[t] = wl_uniform_f(qs ? a.g0b[t] : 0.f); f1[t] = wl_uniform_f(qs ? a.g0a[t] : 0.f);
            F0[t] = wl_uniform_f(qs ? a.g1b[t] : 0.f); F1[t] = wl_uniform_f(qs ? a.g1a[t] : 0.f);
        }
        T* const yr = a.y + (size_t)row * s.out_len;
        for (int l = s.J; l >= 1; --l) {
            const float* const lb = reinterpret_cast<const float*>(ctx.smem + a.lo_off[l]);
            const float* const hb = reinterpret_cast<const float*>(ctx.smem + a.hi_off[l]);
            const int ca = g.ca[l], q0 = g.q0[l], q1 = g.q1[l];
            const int rule = s.rule[l - 1];
            const bool more = l > 1;
            float* const dst = more ? reinterpret_cast<float*>(ctx.smem + a.lo_off[l - 1]) : nullptr;
            const int dca = more ? g.ca[l - 1] : 0, dcb = more ? g.cb[l - 1] : 0;
            const int tn = more ? s.n[l - 1] : s.out_len;         // samples of the output after its end rule
            if (l == 1 && !s.qstart) {
                const int L0 = a.L0, L1 = a.L1, m0 = L0 >> 1, m1 = L1 >> 1;
                const bool fold = rule == WL_DT1D_RULE_FOLD;
                for (int i = q0 + tid; i < q1 && i < tn; i += kThreads) {
                    float v = 0.f;
                    for (int r = 0; r < 2; ++r) {                // (r = 1: the sample behind the last one, folded onto it)
                        if (r == 1 && !(fold && i == tn - 1)) break;
                        const float* p0 = lb + (i + r - m0 - ca);
                        const float* p1 = hb + (i + r - m1 - ca);
                        float w = 0.f;
                        for (int t = 0; t < L0; ++t) w = __builtin_fmaf(a.g0o[t], p0[t], w);
                        for (int t = 0; t < L1; ++t) w = __builtin_fmaf(a.g1o[t], p1[t], w);
                        v = r ? v + w : w;
                    }
                    yr[i] = (T)v;
                }
            } else {
                const int sh = rule != WL_DT1D_RULE_NONE ? 1 : 0, R = 2 * s.n[l];
                for (int q = q0 + tid; q < q1; q += kThreads) {
                    const float* pl = lb + (2 * q + 1 - M2 - ca);             // (even cell: 8-byte aligned pairs)
                    const float* ph = hb + (2 * q + 1 - M2 - ca);
                    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
#pragma unroll
                    for (int t = 0; t < M2; ++t) {
                        const wl_f2 x = *reinterpret_cast<const wl_f2*>(pl + 2 * t);
                        const wl_f2 h = *reinterpret_cast<const wl_f2*>(ph + 2 * t);
                        v0 = __builtin_fmaf(f0[2 * t + 1], x.x, v0); v0 = __builtin_fmaf(F0[2 * t + 1], h.y, v0);
                        v1 = __builtin_fmaf(f1[2 * t + 1], x.y, v1); v1 = __builtin_fmaf(F1[2 * t + 1], h.x, v1);
                        v2 = __builtin_fmaf(f0[2 * t], x.x, v2);     v2 = __builtin_fmaf(F0[2 * t], h.y, v2);
                        v3 = __builtin_fmaf(f1[2 * t], x.y, v3);     v3 = __builtin_fmaf(F1[2 * t], h.x, v3);
                    }
                    if (rule == WL_DT1D_RULE_FOLD) {
                        if (q == 0) v1 = v1 + v0;
                        if (4 * q + 4 == R) v2 = v2 + v3;
                    }
                    const float v[4] = {v0, v1, v2, v3};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = 4 * q + k - sh;
                        if ((unsigned)i >= (unsigned)tn) continue;
                        if (dst) wl_dt1d_put(dst, dca, dca, dcb, tn, i, v[k]);
                        else if (i >= g.o0 && i < g.o1) yr[i] = (T)v[k];
                    }
                }
            }
            ctx.sync();
        }
    }
};
