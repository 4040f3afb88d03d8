// C ABI of the fused multi-level 1-D DTCWT kernels (wl_dtcwt1d.h).  Included at the end of wl_dwt1d_api.inc, so compiled in the
// fourth translation unit of the HIP build (wl_dtinv_hip.hip) and in the matching unit of the host emulation.
#include "wl_api_common.h"
#include "wl_dtcwt1d.h"

// chunks whose geometry decides buffer sizes and declines: all of them - but for the long rows of the chunk policy, whose chunks
// are far longer than the halo: there the first and the last three (the ones in between differ by a shift)
static inline bool wl_dt1d_chunk_matters(int c, int nchunks, int forced) { return forced > 0 || nchunks <= 4096 || c < 3 || c >= nchunks - 3; }

template <typename T, int M>
static int wl_dt1d_fwd_launch(WlDt1dFwdArgs<T>& a, int force_chunk, void* stream) {
    WlDt1dFwdShape& s = a.s;
    const int J = s.J, KJ = wl_dt1d_fwd_pairs(s, J);
    int chunk = force_chunk > 0 ? force_chunk : WL_DT1D_SPAN >> (J + (s.qstart ? 1 : 0));
    if (chunk > KJ) chunk = KJ;
    if (chunk < 1) chunk = 1;
    s.chunk = chunk;
    s.nchunks = wl_cdiv(KJ, chunk);
    int cap[WL_DT1D_MAXJ] = {0, 0, 0, 0};
    for (int c = 0; c < s.nchunks; ++c) {
        if (!wl_dt1d_chunk_matters(c, s.nchunks, force_chunk)) continue;
        WlDt1dFwdGeo g;
        wl_dt1d_fwd_geometry(s, c, g);
        for (int b = 0; b < J; ++b) {
            if (g.chi[b] - g.org[b] > cap[b]) cap[b] = g.chi[b] - g.org[b];
            // a level's lowpass is mirrored by one fold at most: shorter levels go to the per-level path
            const int np = wl_dt1d_padded_len(s.n[b], s.pad[b]);
            if (b > 0 && g.chi[b] > g.clo[b] && (g.clo[b] < -np || g.chi[b] > 2 * np)) return WL_ERR_UNSUPPORTED;
        }
    }
    int off = 0;
    for (int b = 0; b < WL_DT1D_MAXJ; ++b) { a.buf_off[b] = off; if (b < J) off += wl_align_up(cap[b] * 4, 16) + 16; }
    a.geo_off = off; off += wl_align_up((int)sizeof(WlDt1dFwdGeo), 16);
    a.lds_bytes = off;
    if (off > 64 * 1024) return WL_ERR_UNSUPPORTED;
    a.nblocks = a.rows * s.nchunks;
    return wl_launch<WlDt1dFwd<T, M> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

static inline bool wl_dt1d_odd_taps(int L) { return L >= 1 && (L & 1) && L < WL_DT1D_MAXL1; }

extern "C" int wl_dtcwt1d_analysis(const void* x, void* const* his, void* const* los, int dtype, int64_t rows, int N, int J, int qstart,
                                   const int* pad, const void* h0o, const void* h1o, int L0, int L1, const void* h0a,
                                   const void* h0b, const void* h1a, const void* h1b, int M, int chunk, void* stream) {
    if (rows < 0 || N < 1 || J < 1 || chunk < 0) return WL_ERR_SHAPE;
    if (J > WL_DT1D_MAXJ || !x || !his || !los || !pad || !los[J - 1]) return WL_ERR_UNSUPPORTED;
    const bool biort = !qstart, qs = J > 1 || qstart;
    if (biort && (!h0o || !h1o || L0 < 1 || L1 < 1)) return WL_ERR_TAPS;
    if (biort && !(wl_dt1d_odd_taps(L0) && wl_dt1d_odd_taps(L1))) return WL_ERR_UNSUPPORTED;
    if (qs && (!h0a || !h0b || !h1a || !h1b || M < 1)) return WL_ERR_TAPS;
    if (qs && M != 10 && M != 14 && M != 18) return WL_ERR_UNSUPPORTED;
    if (!qs) M = 10;
    if (N >= (1 << 30) || (int64_t)rows * N >= (1LL << 40)) return WL_ERR_UNSUPPORTED;
    WlDt1dFwdShape s;
    s.J = J; s.qstart = qstart ? 1 : 0; s.M = M; s.Mx = biort ? (L0 > L1 ? L0 : L1) / 2 : 0; s.chunk = s.nchunks = 0;
    for (int l = 0; l <= WL_DT1D_MAXJ; ++l) s.n[l] = 0;
    for (int l = 0; l < WL_DT1D_MAXJ; ++l) s.pad[l] = 0;
    s.n[0] = N;
    for (int l = 1; l <= J; ++l) {
        int p = pad[l - 1];
        if (l == 1 && biort) { if (p != WL_DT1D_PAD_NONE) return WL_ERR_SHAPE; p = (N & 1) ? WL_DT1D_PAD_LAST : WL_DT1D_PAD_NONE; }
        else if (p != WL_DT1D_PAD_NONE && p != WL_DT1D_PAD_REPL && p != WL_DT1D_PAD_ZERO) return WL_ERR_SHAPE;
        s.pad[l - 1] = p;
        const int np = wl_dt1d_padded_len(s.n[l - 1], p);
        if (l == 1 && biort) s.n[l] = np;
        else { if (np % 4) return WL_ERR_SHAPE; s.n[l] = np / 2; }
    }
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlDt1dFwdArgs<T> a;
        a.x = (const T*)x;
        for (int l = 0; l < WL_DT1D_MAXJ; ++l) { a.hi[l] = l < J ? (T*)his[l] : nullptr; a.lo[l] = l < J ? (T*)los[l] : nullptr; }
        a.h0o = (const float*)h0o; a.h1o = (const float*)h1o; a.L0 = L0; a.L1 = L1;
        a.h0a = (const float*)h0a; a.h0b = (const float*)h0b; a.h1a = (const float*)h1a; a.h1b = (const float*)h1b;
        a.rows = rows; a.s = s;
        switch (M) {
            case 10: return wl_dt1d_fwd_launch<T, 10>(a, chunk, stream);
            case 14: return wl_dt1d_fwd_launch<T, 14>(a, chunk, stream);
            default: return wl_dt1d_fwd_launch<T, 18>(a, chunk, stream);
        }
    });
}

template <typename T, int M>
static int wl_dt1d_inv_launch(WlDt1dInvArgs<T>& a, int force_chunk, void* stream) {
    WlDt1dInvShape& s = a.s;
    const int J = s.J;
    int chunk = force_chunk > 0 ? force_chunk : (J == 1 ? 2 * WL_DT1D_INV_CHUNK : WL_DT1D_INV_CHUNK);
    if (chunk > s.out_len) chunk = s.out_len;
    s.chunk = chunk;
    s.nchunks = wl_cdiv(s.out_len, chunk);
    int cap[WL_DT1D_MAXJ + 1] = {0, 0, 0, 0, 0};
    for (int c = 0; c < s.nchunks; ++c) {
        if (!wl_dt1d_chunk_matters(c, s.nchunks, force_chunk)) continue;
        WlDt1dInvGeo g;
        wl_dt1d_inv_geometry(s, c, g);
        for (int l = 1; l <= J; ++l) {
            if (g.cb[l] - g.ca[l] > cap[l]) cap[l] = g.cb[l] - g.ca[l];
            if (g.cb[l] > g.ca[l] && (g.ca[l] < -s.n[l] || g.cb[l] > 2 * s.n[l])) return WL_ERR_UNSUPPORTED;
        }
    }
    int off = 0;
    for (int l = 0; l <= WL_DT1D_MAXJ; ++l) {
        a.lo_off[l] = off; if (l >= 1 && l <= J) off += wl_align_up(cap[l] * 4, 16) + 16;
        a.hi_off[l] = off; if (l >= 1 && l <= J) off += wl_align_up(cap[l] * 4, 16) + 16;
    }
    a.geo_off = off; off += wl_align_up((int)sizeof(WlDt1dInvGeo), 16);
    a.lds_bytes = off;
    if (off > 64 * 1024) return WL_ERR_UNSUPPORTED;
    a.nblocks = a.rows * s.nchunks;
    return wl_launch<WlDt1dInv<T, M> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

extern "C" int wl_dtcwt1d_synthesis(const void* lo, int n_lo, const void* const* his, const int* n, const int* rule, void* y,
                                    int out_len, int dtype, int64_t rows, int J, int qstart, const void* g0o, const void* g1o,
                                    int L0, int L1, const void* g0a, const void* g0b, const void* g1a, const void* g1b, int M,
                                    int chunk, void* stream) {
    if (rows < 0 || J < 1 || n_lo < 1 || out_len < 1 || chunk < 0) return WL_ERR_SHAPE;
    if (J > WL_DT1D_MAXJ || !lo || !his || !n || !rule || !y) return WL_ERR_UNSUPPORTED;
    const bool biort = !qstart, qs = J > 1 || qstart;
    if (biort && (!g0o || !g1o || L0 < 1 || L1 < 1)) return WL_ERR_TAPS;
    if (biort && !(wl_dt1d_odd_taps(L0) && wl_dt1d_odd_taps(L1))) return WL_ERR_UNSUPPORTED;
    if (qs && (!g0a || !g0b || !g1a || !g1b || M < 1)) return WL_ERR_TAPS;
    if (qs && M != 10 && M != 14 && M != 18) return WL_ERR_UNSUPPORTED;
    if (!qs) M = 10;
    WlDt1dInvShape s;
    s.J = J; s.qstart = qstart ? 1 : 0; s.M = M; s.Mx = biort ? (L0 > L1 ? L0 : L1) / 2 : 0; s.chunk = s.nchunks = 0;
    s.n_lo = n_lo; s.out_len = out_len;
    for (int l = 0; l <= WL_DT1D_MAXJ; ++l) { s.n[l] = 0; s.rule[l] = 0; }
    for (int l = 0; l <= J; ++l) {
        if (rule[l] != WL_DT1D_RULE_NONE && rule[l] != WL_DT1D_RULE_CROP && rule[l] != WL_DT1D_RULE_FOLD) return WL_ERR_SHAPE;
        s.rule[l] = rule[l];
    }
    for (int l = 1; l <= J; ++l) {
        if (n[l - 1] < 2 || (n[l - 1] & 1) || n[l - 1] >= (1 << 29)) return n[l - 1] >= (1 << 29) ? WL_ERR_UNSUPPORTED : WL_ERR_SHAPE;
        s.n[l] = n[l - 1];
    }
    if (rule[J] == WL_DT1D_RULE_FOLD || n_lo != s.n[J] + (rule[J] == WL_DT1D_RULE_CROP ? 2 : 0)) return WL_ERR_SHAPE;
    for (int l = 2; l <= J; ++l)
        if (2 * s.n[l] != s.n[l - 1] + (rule[l - 1] != WL_DT1D_RULE_NONE ? 2 : 0)) return WL_ERR_SHAPE;
    if (biort) {
        if (rule[0] == WL_DT1D_RULE_CROP || out_len != s.n[1] - (rule[0] == WL_DT1D_RULE_FOLD ? 1 : 0)) return WL_ERR_SHAPE;
    } else if (out_len != 2 * s.n[1] - (rule[0] != WL_DT1D_RULE_NONE ? 2 : 0)) return WL_ERR_SHAPE;
    if ((int64_t)rows * out_len >= (1LL << 40)) return WL_ERR_UNSUPPORTED;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlDt1dInvArgs<T> a;
        a.lo = (const T*)lo; a.y = (T*)y;
        for (int l = 0; l < WL_DT1D_MAXJ; ++l) a.hi[l] = l < J ? (const T*)his[l] : nullptr;
        a.g0o = (const float*)g0o; a.g1o = (const float*)g1o; a.L0 = L0; a.L1 = L1;
        a.g0a = (const float*)g0a; a.g0b = (const float*)g0b; a.g1a = (const float*)g1a; a.g1b = (const float*)g1b;
        a.rows = rows; a.s = s;
        switch (M) {
            case 10: return wl_dt1d_inv_launch<T, 10>(a, chunk, stream);
            case 14: return wl_dt1d_inv_launch<T, 14>(a, chunk, stream);
            default: return wl_dt1d_inv_launch<T, 18>(a, chunk, stream);
        }
    });
}
#include "wl_wave1d_api.inc"
