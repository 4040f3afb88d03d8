// C ABI of the wave-tile kernels (wl_wave1d.h): the 1-D stationary transform (wl_swt1d.h), the 1-D wavelet packet transform
// (wl_wpt1d.h), the 1-D scattering layer (wl_scat1d.h), the shrinkage of the stationary transform (wl_shrink1d.h) and the tap
// gradients of the stationary transform (wl_swt1d_tapgrad.h).  Included at the end of wl_dtcwt1d_api.inc, so compiled in the fourth translation unit of the HIP build
// (wl_dtinv_hip.hip) and in the matching unit of the host emulation.
#include "wl_api_common.h"
#include "wl_swt1d.h"
#include "wl_wpt1d.h"
#include "wl_scat1d.h"
#include "wl_shrink1d.h"
#include "wl_swt1d_tapgrad.h"

// the grid of a launch: tiles of `core` positions from -origin on, WL_WAVE1D_WAVES tiles per workgroup
struct WlWave1dGrid { int core, tiles; int64_t waves, nblocks; };

// The checks every entry starts with (their order decides which code wins when several fail); `family_ok`: the transform's own
// mode / extension test, which answers with the same code as the level and tap limits.
static int wl_wave1d_check(int64_t rows, int len, int J, int L, int dtype, bool family_ok, int origin) {
    if (rows < 0 || len < 1 || J < 1 || L < 1 || origin < 0) return WL_ERR_SHAPE;
    if (dtype != WL_F32 && dtype != WL_F16 && dtype != WL_BF16) return dtype == WL_F64 ? WL_ERR_UNSUPPORTED : WL_ERR_DTYPE;
    if (J > WL_WAVE1D_MAXJ || (L & 1) || L > WL_WAVE1D_MAXL || !family_ok || len >= (1 << 30)) return WL_ERR_UNSUPPORTED;
    return 0;
}

// ... and end with, once the transform has worked out its core
static int wl_wave1d_grid(int64_t rows, int len, int origin, int core, WlWave1dGrid& g) {
    if (origin >= core) return WL_ERR_SHAPE;
    g.core = core;
    g.tiles = wl_cdiv(len + origin, core);
    g.waves = rows * g.tiles;
    g.nblocks = wl_cdiv64(g.waves, WL_WAVE1D_WAVES);
    return 0;
}

static int wl_swt1d_grid(int64_t rows, int N, int J, int L, int dtype, int ext, int origin, WlWave1dGrid& g) {
    const int rc = wl_wave1d_check(rows, N, J, L, dtype, ext == WL_EXT_PERIODIC, origin);
    if (rc != 0) return rc;
    return wl_wave1d_grid(rows, N, origin, 64 * WL_WAVE1D_V - (L - 1) * ((1 << J) - 1), g);
}

// `head`: the halo in front of each core
static int wl_wpt1d_grid(int64_t rows, int len, int nlev, int L, int dtype, int mode, int origin, int& head, WlWave1dGrid& g) {
    const int rc = wl_wave1d_check(rows, len, nlev, L, dtype, mode == 2, origin);
    if (rc != 0) return rc;
    const int q = 1 << nlev;
    // every level's band is even and at least as long as the filter (shorter: the reference's single fold is not the circular form)
    if (len % q != 0 || (len >> (nlev - 1)) < L) return WL_ERR_UNSUPPORTED;
    head = ((L / 2) * (q - 1) + q - 1) / q * q;
    if (origin % q != 0) return WL_ERR_SHAPE;
    return wl_wave1d_grid(rows, len, origin, 64 * WL_WAVE1D_V - 2 * head, g);
}

// the fields every argument struct has
#define WL_WAVE1D_FILL(a, g, nrows, n, J, org) \
    a.rows = nrows; a.waves = g.waves; a.len = n; a.nlev = J; a.tiles = g.tiles; a.core = g.core; a.origin = org

#define WL_WAVE1D_BY_TAPS(K, a, g, stream)                                                     \
    switch (L) {                                                                               \
        case 2: return wl_launch<K<T, 2> >(a, g.nblocks, 0, stream);                           \
        case 4: return wl_launch<K<T, 4> >(a, g.nblocks, 0, stream);                           \
        case 6: return wl_launch<K<T, 6> >(a, g.nblocks, 0, stream);                           \
        case 8: return wl_launch<K<T, 8> >(a, g.nblocks, 0, stream);                           \
        case 10: return wl_launch<K<T, 10> >(a, g.nblocks, 0, stream);                         \
        case 12: return wl_launch<K<T, 12> >(a, g.nblocks, 0, stream);                         \
        case 14: return wl_launch<K<T, 14> >(a, g.nblocks, 0, stream);                         \
        case 16: return wl_launch<K<T, 16> >(a, g.nblocks, 0, stream);                         \
        case 18: return wl_launch<K<T, 18> >(a, g.nblocks, 0, stream);                         \
        default: return wl_launch<K<T, 20> >(a, g.nblocks, 0, stream);                         \
    }

extern "C" int wl_swt1d_analysis(const void* x, void* lo, void* const* his, int dtype, int64_t rows, int N, int J, const void* h0,
                                 const void* h1, int L, int ext, double scale, int origin, void* stream) {
    WlWave1dGrid g;
    const int rc = wl_swt1d_grid(rows, N, J, L, dtype, ext, origin, g);
    if (rc != 0) return rc;
    if (!x || !lo || !his) return WL_ERR_SHAPE;
    if (!h0 || !h1) return WL_ERR_TAPS;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlSwt1dFwdArgs<T> a;
        a.x = (const T*)x; a.lo = (T*)lo;
        for (int l = 0; l < WL_WAVE1D_MAXJ; ++l) a.hi[l] = l < J ? (T*)his[l] : nullptr;
        a.h0 = (const float*)h0; a.h1 = (const float*)h1;
        WL_WAVE1D_FILL(a, g, rows, N, J, origin);
        a.scale = (float)scale;
        WL_WAVE1D_BY_TAPS(WlSwt1dFwd, a, g, stream)
    });
}

extern "C" int wl_swt1d_adjoint(const void* lo, const void* const* his, void* y, int dtype, int64_t rows, int N, int J, const void* g0,
                                const void* g1, int L, int ext, double scale, int origin, void* stream) {
    WlWave1dGrid g;
    const int rc = wl_swt1d_grid(rows, N, J, L, dtype, ext, origin, g);
    if (rc != 0) return rc;
    if (!lo || !y || !his) return WL_ERR_SHAPE;
    if (!g0 || !g1) return WL_ERR_TAPS;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlSwt1dAdjArgs<T> a;
        a.lo = (const T*)lo; a.y = (T*)y;
        for (int l = 0; l < WL_WAVE1D_MAXJ; ++l) a.hi[l] = l < J ? (const T*)his[l] : nullptr;
        a.g0 = (const float*)g0; a.g1 = (const float*)g1;
        WL_WAVE1D_FILL(a, g, rows, N, J, origin);
        a.scale = (float)scale;
        WL_WAVE1D_BY_TAPS(WlSwt1dAdj, a, g, stream)
    });
}

// ---- the tap gradients of the 1-D stationary transform: both chains and the 2 L correlations in one launch (wl_swt1d_tapgrad.h)
extern "C" int wl_swt1d_tapgrad(const void* s, const void* top, const void* const* his, void* part, int dtype, int64_t rows, int n,
                                int J, const void* k0, const void* k1, int L, int ext, double scale, int origin, void* stream) {
    WlWave1dGrid g;
    int rc = wl_wave1d_check(rows, n, J, L, dtype, ext == WL_EXT_PERIODIC, origin);
    if (rc == 0) rc = wl_wave1d_grid(rows, n, origin, wl_swt1d_tapgrad_core(L, J), g);
    if (rc != 0) return rc;
    if (!s || !top || !his || !part) return WL_ERR_SHAPE;
    if (!k0 || !k1) return WL_ERR_TAPS;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlSwt1dTapGradArgs<T> a;
        a.s = (const T*)s; a.top = (const T*)top; a.part = (float*)part;
        for (int l = 0; l < WL_WAVE1D_MAXJ; ++l) a.hi[l] = l < J ? (const T*)his[l] : nullptr;
        a.k0 = (const float*)k0; a.k1 = (const float*)k1;
        WL_WAVE1D_FILL(a, g, rows, n, J, origin);
        a.scale = (float)scale;
        WL_WAVE1D_BY_TAPS(WlSwt1dTapGrad, a, g, stream)
    });
}

// ---- shrinkage of the 1-D stationary transform: analysis, threshold and inverse in one launch (wl_shrink1d.h)
static int wl_shrink1d_grid(int64_t rows, int n, int J, int L, int dtype, int kind, int origin, WlWave1dGrid& g) {
    const int rc = wl_wave1d_check(rows, n, J, L, dtype, kind == WL_SHRINK_SOFT || kind == WL_SHRINK_HARD, origin);
    if (rc != 0) return rc;
    return wl_wave1d_grid(rows, n, origin, 64 * WL_WAVE1D_V - 2 * (L - 1) * ((1 << J) - 1), g);
}

#define WL_SHRINK1D_FILL(a, g)                                                                 \
    a.thr = (const float*)thr;                                                                 \
    a.h0 = (const float*)h0; a.h1 = (const float*)h1; a.g0 = (const float*)g0; a.g1 = (const float*)g1; \
    WL_WAVE1D_FILL(a, g, rows, n, J, origin);                                                  \
    a.kind = kind

extern "C" int wl_shrink1d_forward(const void* x, void* y, const void* thr, int dtype, int64_t rows, int n, int J, const void* h0,
                                   const void* h1, const void* g0, const void* g1, int L, int kind, int origin, void* stream) {
    WlWave1dGrid g;
    const int rc = wl_shrink1d_grid(rows, n, J, L, dtype, kind, origin, g);
    if (rc != 0) return rc;
    if (!x || !y || !thr) return WL_ERR_SHAPE;
    if (!h0 || !h1 || !g0 || !g1) return WL_ERR_TAPS;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlShrink1dFwdArgs<T> a;
        a.x = (const T*)x; a.y = (T*)y;
        WL_SHRINK1D_FILL(a, g);
        WL_WAVE1D_BY_TAPS(WlShrink1dFwd, a, g, stream)
    });
}

extern "C" int wl_shrink1d_backward(const void* x, const void* dy, void* dx, const void* thr, void* dthr_part, int dtype, int64_t rows,
                                    int n, int J, const void* h0, const void* h1, const void* g0, const void* g1, int L, int kind,
                                    int origin, void* stream) {
    WlWave1dGrid g;
    const int rc = wl_shrink1d_grid(rows, n, J, L, dtype, kind, origin, g);
    if (rc != 0) return rc;
    if (!x || !dy || !dx || !thr) return WL_ERR_SHAPE;
    if (!h0 || !h1 || !g0 || !g1) return WL_ERR_TAPS;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlShrink1dBwdArgs<T> a;
        a.x = (const T*)x; a.dy = (const T*)dy; a.dx = (T*)dx;
        a.dthr_part = (float*)dthr_part;
        WL_SHRINK1D_FILL(a, g);
        WL_WAVE1D_BY_TAPS(WlShrink1dBwd, a, g, stream)
    });
}
#undef WL_SHRINK1D_FILL

#define WL_WPT1D_ENTRY(K, from, to, t0, t1)                                                                                     \
    WlWave1dGrid g;                                                                                                             \
    int head;                                                                                                                   \
    const int rc = wl_wpt1d_grid(rows, len, nlev, L, dtype, mode, origin, head, g);                                             \
    if (rc != 0) return rc;                                                                                                     \
    if (!from || !to) return WL_ERR_SHAPE;                                                                                      \
    if (!t0 || !t1) return WL_ERR_TAPS;                                                                                         \
    if (rows == 0) return 0;                                                                                                    \
    WL_DISPATCH_FLOAT(dtype, {                                                                                                  \
        WlWpt1dArgs<T> a;                                                                                                       \
        a.src = (const T*)from; a.dst = (T*)to;                                                                                 \
        a.f0 = (const float*)t0; a.f1 = (const float*)t1;                                                                       \
        WL_WAVE1D_FILL(a, g, rows, len, nlev, origin);                                                                          \
        a.head = head;                                                                                                          \
        WL_WAVE1D_BY_TAPS(K, a, g, stream)                                                                                      \
    })

extern "C" int wl_wpt1d_analysis(const void* x, void* y, int dtype, int64_t rows, int len, int nlev, const void* h0, const void* h1,
                                 int L, int mode, int origin, void* stream) {
    WL_WPT1D_ENTRY(WlWpt1dAfb, x, y, h0, h1);
}

extern "C" int wl_wpt1d_synthesis(const void* y, void* x, int dtype, int64_t rows, int len, int nlev, const void* g0, const void* g1,
                                  int L, int mode, int origin, void* stream) {
    WL_WPT1D_ENTRY(WlWpt1dSfb, y, x, g0, g1);
}
#undef WL_WPT1D_ENTRY

// ---- the 1-D scattering layer: two odd tap counts, one level, the symmetric fold.  Its own checks (wl_wave1d_check insists on
// one even L), the same order of the codes.
static bool wl_scat1d_pair(int L0, int L1) {
    return (L0 == 5 && L1 == 7) || (L0 == 5 && L1 == 3) || (L0 == 13 && L1 == 19) || (L0 == 9 && L1 == 7);
}

static int wl_scat1d_grid(int64_t batch, int C, int n, int L0, int L1, int dtype, int origin, WlWave1dGrid& g) {
    if (batch < 0 || C < 0 || n < 1 || L0 < 1 || L1 < 1 || origin < 0) return WL_ERR_SHAPE;
    if (dtype != WL_F32 && dtype != WL_F16 && dtype != WL_BF16) return dtype == WL_F64 ? WL_ERR_UNSUPPORTED : WL_ERR_DTYPE;
    if (!wl_scat1d_pair(L0, L1) || n >= (1 << 29)) return WL_ERR_UNSUPPORTED;      // (the fold's period 2 ne is an int)
    if (origin & 1) return WL_ERR_SHAPE;                                           // a lane holds whole (2k, 2k+1) pairs
    const int M = (L0 > L1 ? L0 : L1) / 2, head = (M + 1) / 2 * 2;
    return wl_wave1d_grid(batch * C, n + (n & 1), origin, 64 * WL_WAVE1D_V - 2 * head, g);
}

#define WL_SCAT1D_BY_TAPS(K, a, g, stream)                                                     \
    switch (L0 * 100 + L1) {                                                                   \
        case 507: return wl_launch<K<T, 5, 7> >(a, g.nblocks, 0, stream);                      \
        case 503: return wl_launch<K<T, 5, 3> >(a, g.nblocks, 0, stream);                      \
        case 1319: return wl_launch<K<T, 13, 19> >(a, g.nblocks, 0, stream);                   \
        default: return wl_launch<K<T, 9, 7> >(a, g.nblocks, 0, stream);                       \
    }

#define WL_SCAT1D_FILL(a, g)                                                                   \
    a.h0 = (const float*)h0o; a.h1 = (const float*)h1o;                                        \
    a.rows = batch * C; a.waves = g.waves; a.C = C; a.n = n; a.len = n + (n & 1);              \
    a.tiles = g.tiles; a.core = g.core; a.origin = origin

extern "C" int wl_scat1d_forward(const void* x, void* z, void* dir, int dtype, int64_t batch, int C, int n, const void* h0o, int L0,
                                 const void* h1o, int L1, double magbias, int origin, void* stream) {
    WlWave1dGrid g;
    const int rc = wl_scat1d_grid(batch, C, n, L0, L1, dtype, origin, g);
    if (rc != 0) return rc;
    if (!x || !z) return WL_ERR_SHAPE;
    if (!h0o || !h1o) return WL_ERR_TAPS;
    if (batch * C == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlScat1dFwdArgs<T> a;
        a.x = (const T*)x; a.z = (T*)z; a.dir = (T*)dir;
        WL_SCAT1D_FILL(a, g);
        a.bias = (float)magbias;
        WL_SCAT1D_BY_TAPS(WlScat1dFwd, a, g, stream)
    });
}

extern "C" int wl_scat1d_backward(const void* dz, const void* dir, void* dx, int dtype, int64_t batch, int C, int n, const void* h0o,
                                  int L0, const void* h1o, int L1, double magbias, int origin, void* stream) {
    (void)magbias;                                      // (the directions carry it)
    WlWave1dGrid g;
    const int rc = wl_scat1d_grid(batch, C, n, L0, L1, dtype, origin, g);
    if (rc != 0) return rc;
    if (!dz || !dir || !dx) return WL_ERR_SHAPE;
    if (!h0o || !h1o) return WL_ERR_TAPS;
    if (batch * C == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlScat1dBwdArgs<T> a;
        a.dz = (const T*)dz; a.dir = (const T*)dir; a.dx = (T*)dx;
        WL_SCAT1D_FILL(a, g);
        WL_SCAT1D_BY_TAPS(WlScat1dBwd, a, g, stream)
    });
}
#undef WL_SCAT1D_FILL
#undef WL_SCAT1D_BY_TAPS
