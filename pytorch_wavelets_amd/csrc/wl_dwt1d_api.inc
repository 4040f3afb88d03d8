// C ABI of the fused multi-level 1-D analysis (wl_dwt1d_fused.h).  Compiled in the fourth translation unit of the HIP build
// (wl_dtinv_hip.hip); included after the backend header.
#include "wl_api_common.h"
#include "wl_dwt1d_fused.h"

template <typename T, int LT>
static int wl_dwt1d_fused_launch(WlDwt1dArgs<T>& a, void* stream) {
    typedef WlDwt1dFused<T, LT> K;
    const bool wraps = a.ext == WL_EXT_PERIODIC || a.ext == WL_EXT_PER;
    const int J = a.J;
    for (int j = 0; j < J; ++j) if (a.n[j] < LT) return WL_ERR_UNSUPPORTED;          // (levels shorter than the filter: per-level kernels)
    // chunk: ~4096 input samples per workgroup (31 KB of LDS: five workgroups per CU overlap their load and compute phases;
    // the halo both neighbours also load is (L - 2)(2^J - 1) samples either side, 2 % at db4 J = 3); modes that wrap around
    // need the whole row in one chunk
    int chunk = WL_DWT1D_SPAN >> J;
    if (chunk < 2 * LT) chunk = 2 * LT;
    if (wraps || chunk > a.n[J]) chunk = a.n[J];
    a.chunk = chunk;
    a.nchunks = wl_cdiv(a.n[J], chunk);
    int cap[WL_DWT1D_MAXJ] = {0, 0, 0, 0};
    for (int c = 0; c < a.nchunks; ++c) {
        // (chunks 1 .. nchunks - 2 differ by a shift only: the first two and the last two decide the buffer sizes)
        if (c > 1 && c < a.nchunks - 2) continue;
        const typename K::Geo g = K::geometry(a, c);
        {   // the loader's envelope: MAXV vector groups and one single sample per thread
            const int v_lo = g.clo[0] < 0 ? 0 : (g.clo[0] + 3) & ~3;
            int v_hi = g.chi[0] > a.n[0] ? a.n[0] & ~3 : g.chi[0] & ~3;
            if (v_hi < v_lo) v_hi = v_lo;
            if (v_hi - v_lo > 4 * K::kThreads * K::MAXV || (v_lo - g.clo[0]) + (g.chi[0] - v_hi) > K::kThreads) return WL_ERR_UNSUPPORTED;
            if (a.n[0] < 4) return WL_ERR_UNSUPPORTED;
        }
        for (int j = 0; j < J; ++j) {
            const int need = g.chi[j] - g.org[j] + 4;
            if (need > cap[j]) cap[j] = need;
            if (g.chi[j + 1] <= g.clo[j + 1]) continue;
            if (j == 0) continue;
            // inner levels: every position level j + 1 reads beyond the ends of level j must mirror into the chunk
            for (int e = 0; e < 2; ++e) {
                const int k = e ? g.chi[j + 1] - 1 : g.clo[j + 1];
                for (int t = 0; t < LT; ++t) {
                    const int p = 2 * k + a.base[j] + t;
                    if ((unsigned)p < (unsigned)a.n[j]) { if (p < g.clo[j] || p >= g.chi[j]) return WL_ERR_UNSUPPORTED; continue; }
                    const int sp = wl_ext(p, a.n[j], a.ext);
                    if (sp >= 0 && (sp < g.clo[j] || sp >= g.chi[j])) return WL_ERR_UNSUPPORTED;
                }
            }
        }
    }
    int off = 0;
    for (int j = 0; j < J; ++j) { a.buf_off[j] = off; off += wl_align_up(cap[j] * 4, 16); }
    a.lds_bytes = off;
    if (a.lds_bytes > 64 * 1024) return WL_ERR_UNSUPPORTED;
    // consecutive chunks per workgroup: about two rounds of workgroups over the chip (five of them fit a CU)
    {
        const int64_t total = a.rows * a.nchunks, want = 2 * 5 * (int64_t)wl_num_cus();
        int64_t cpw = total / want;
        if (cpw < 1) cpw = 1;
        if (cpw > a.nchunks) cpw = a.nchunks;
        a.cpw = (int)cpw;
        a.ngroups = wl_cdiv(a.nchunks, a.cpw);
    }
    a.nblocks = a.rows * a.ngroups;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
static int wl_dwt1d_fused_any(WlDwt1dArgs<T>& a, int L, void* stream) {
#define WL_CASE(LT_) case LT_: return wl_dwt1d_fused_launch<T, LT_>(a, stream)
    switch (L) {
        WL_CASE(2); WL_CASE(4); WL_CASE(6); WL_CASE(8); WL_CASE(10); WL_CASE(12); WL_CASE(14); WL_CASE(16); WL_CASE(18); WL_CASE(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASE
}

extern "C" int wl_dwt1d_analysis_fused(const void* x, void* lo, void* const* highs, int dtype, int64_t rows, int N, int J,
                                       const void* h0, const void* h1, int L, int mode, void* stream) {
    const int ext = wl_mode_to_ext(mode);
    if (ext < 0) return WL_ERR_MODE;
    if (rows < 0 || N < 1 || J < 1) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (J > WL_DWT1D_MAXJ || !highs || !lo || !x) return WL_ERR_UNSUPPORTED;
    if (rows == 0) return 0;
    if (mode == 2 && N + (N & 1) < L - 1) return WL_ERR_UNSUPPORTED;       // single-fold corner of the reference: wl_corr1d's literal form
    if ((int64_t)rows * N >= (1LL << 40) || N >= (1 << 30)) return WL_ERR_UNSUPPORTED;   // (wl_ext folds with the period 2N: an int)
    int n[WL_DWT1D_MAXJ + 1], base[WL_DWT1D_MAXJ];
    n[0] = N;
    for (int j = 0; j < J; ++j) {
        n[j + 1] = wl_coeff_len(n[j], L, mode);
        base[j] = wl_afb_base(n[j], L, mode);
        if (mode == 2 && n[j] + (n[j] & 1) < L - 1) return WL_ERR_UNSUPPORTED;
    }
    WL_DISPATCH_FLOAT(dtype, {
        WlDwt1dArgs<T> a;
        a.x = (const T*)x; a.lo = (T*)lo;
        for (int j = 0; j < WL_DWT1D_MAXJ; ++j) a.hi[j] = j < J ? (T*)highs[j] : nullptr;
        a.h0 = (const float*)h0; a.h1 = (const float*)h1; a.rows = rows; a.J = J; a.ext = ext;
        for (int j = 0; j <= WL_DWT1D_MAXJ; ++j) a.n[j] = j <= J ? n[j] : 0;
        for (int j = 0; j < WL_DWT1D_MAXJ; ++j) a.base[j] = j < J ? base[j] : 0;
        return wl_dwt1d_fused_any<T>(a, L, stream);
    });
}

// ---- fused multi-level 1-D synthesis (wl_idwt1d_fused.h) ---------------------------------------------------------------
#include "wl_idwt1d_fused.h"

template <typename T, int LT>
static int wl_idwt1d_fused_launch(WlIdwt1dArgs<T>& a, void* stream) {
    const int J = a.J, HL = LT / 2;
    // outputs per chunk (measured at 64 x 16 x 65536, same box): one level 4096 (0.144 ms against 0.154 at 2048), three levels
    // 2048 (0.182 against 0.224 at 4096, 0.227 at 1024, 0.386 at 8192): more resident workgroups hide the phases' latencies
    int chunk = J == 1 ? WL_IDWT1D_CHUNK : WL_IDWT1D_CHUNK / 2;
    const int unit = 1 << J;
    if (chunk > wl_align_up(a.out_len, unit)) chunk = wl_align_up(a.out_len, unit);
    chunk = wl_align_up(chunk, unit);
    a.chunk = chunk;
    a.nchunks = wl_cdiv(a.out_len, chunk);
    a.span[0] = chunk;
    int off = 0;
    for (int j = 0; j < J; ++j) {
        a.span[j + 1] = wl_align_up(a.span[j] / 2 + HL - 1, 2);
        // (+ one 16-byte group behind every buffer: the loads fill whole groups of four, the two-pair lanes of level 1 read one sample past the span)
        a.hi_off[j] = off; off += wl_align_up(a.span[j + 1] * 4, 16) + 16;
        a.lo_off[j] = off; off += wl_align_up(a.span[j + 1] * 4, 16) + 16;
    }
    for (int j = J; j < WL_IDWT1D_MAXJ; ++j) { a.span[j + 1] = 0; a.hi_off[j] = a.lo_off[j] = 0; }
    a.lds_bytes = off;
    if (off > 64 * 1024) return WL_ERR_UNSUPPORTED;
    a.nblocks = a.rows * a.nchunks;
    return wl_launch<WlIdwt1dFused<T, LT> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
static int wl_idwt1d_fused_any(WlIdwt1dArgs<T>& a, int L, void* stream) {
#define WL_CASE(LT_) case LT_: return wl_idwt1d_fused_launch<T, LT_>(a, stream)
    switch (L) {
        WL_CASE(2); WL_CASE(4); WL_CASE(6); WL_CASE(8); WL_CASE(10); WL_CASE(12); WL_CASE(14); WL_CASE(16); WL_CASE(18); WL_CASE(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASE
}

extern "C" int wl_dwt1d_synthesis_fused(const void* lo, int n_lo, const void* const* highs, const int* n_hi, void* y, int out_len,
                                        int dtype, int64_t rows, int J, const void* g0, const void* g1, int L, int mode,
                                        void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (rows < 0 || J < 1 || n_lo < 1 || out_len < 1) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (J > WL_IDWT1D_MAXJ || !highs || !n_hi || !lo || !y || mode == 2 || (L & 1) || L > 20) return WL_ERR_UNSUPPORTED;
    if (rows == 0) return 0;
    // every level's reconstruction is the next finer level's lowpass: its highpass length or one more (the 'unpad'), the output at
    // most the finest reconstruction
    for (int j = J - 1; j >= 0; --j) {
        if (n_hi[j] < 1) return WL_ERR_SHAPE;
        const int S = 2 * n_hi[j] - L + 2;
        if (S < 1) return WL_ERR_UNSUPPORTED;
        if (j > 0 && !(n_hi[j - 1] <= S && S <= n_hi[j - 1] + 1)) return WL_ERR_UNSUPPORTED;
        if (j == 0 && out_len > S) return WL_ERR_SHAPE;
    }
    if (!(n_hi[J - 1] <= n_lo && n_lo <= n_hi[J - 1] + 1)) return WL_ERR_UNSUPPORTED;
    if ((int64_t)rows * out_len >= (1LL << 40)) return WL_ERR_UNSUPPORTED;
    WL_DISPATCH_FLOAT(dtype, {
        WlIdwt1dArgs<T> a;
        a.lo = (const T*)lo; a.y = (T*)y; a.n_lo = n_lo; a.out_len = out_len;
        for (int j = 0; j < WL_IDWT1D_MAXJ; ++j) { a.hi[j] = j < J ? (const T*)highs[j] : nullptr; a.n_hi[j] = j < J ? n_hi[j] : 0; }
        a.g0 = (const float*)g0; a.g1 = (const float*)g1; a.rows = rows; a.J = J;
        return wl_idwt1d_fused_any<T>(a, L, stream);
    });
}

// ---- fused multi-level 1-D DTCWT (wl_dtcwt1d.h): the same translation unit, in the HIP build and in the host emulation -----
#include "wl_dtcwt1d_api.inc"
