// C ABI of the wave-tile kernels of the 1-D stationary transform (wl_swt1d.h).  Included at the end of wl_dtcwt1d_api.inc, so
// compiled in the fourth translation unit of the HIP build (wl_dtinv_hip.hip) and in the matching unit of the host emulation.
#include "wl_api_common.h"
#include "wl_swt1d.h"

// the grid of both kernels: tiles of `core` positions from -origin on, WL_SWT1D_WAVES of them per workgroup
struct WlSwt1dGrid { int core, tiles; int64_t waves, nblocks; };

static int wl_swt1d_grid(int64_t rows, int N, int J, int L, int dtype, int ext, int origin, WlSwt1dGrid& g) {
    if (rows < 0 || N < 1 || J < 1 || L < 1 || origin < 0) return WL_ERR_SHAPE;
    if (dtype != WL_F32 && dtype != WL_F16 && dtype != WL_BF16) return dtype == WL_F64 ? WL_ERR_UNSUPPORTED : WL_ERR_DTYPE;
    if (J > WL_SWT1D_MAXJ || (L & 1) || L > WL_SWT1D_MAXL || ext != WL_EXT_PERIODIC || N >= (1 << 30)) return WL_ERR_UNSUPPORTED;
    g.core = 64 * WL_SWT1D_V - (L - 1) * ((1 << J) - 1);
    if (origin >= g.core) return WL_ERR_SHAPE;
    g.tiles = wl_cdiv(N + origin, g.core);
    g.waves = rows * g.tiles;
    g.nblocks = wl_cdiv64(g.waves, WL_SWT1D_WAVES);
    return 0;
}

#define WL_SWT1D_BY_TAPS(K, a, g, stream)                                                      \
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
    WlSwt1dGrid g;
    const int rc = wl_swt1d_grid(rows, N, J, L, dtype, ext, origin, g);
    if (rc != 0) return rc;
    if (!x || !lo || !his) return WL_ERR_SHAPE;
    if (!h0 || !h1) return WL_ERR_TAPS;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlSwt1dFwdArgs<T> a;
        a.x = (const T*)x; a.lo = (T*)lo;
        for (int l = 0; l < WL_SWT1D_MAXJ; ++l) a.hi[l] = l < J ? (T*)his[l] : nullptr;
        a.h0 = (const float*)h0; a.h1 = (const float*)h1;
        a.rows = rows; a.waves = g.waves; a.len = N; a.nlev = J; a.tiles = g.tiles; a.core = g.core; a.origin = origin;
        a.scale = (float)scale;
        WL_SWT1D_BY_TAPS(WlSwt1dFwd, a, g, stream)
    });
}

extern "C" int wl_swt1d_adjoint(const void* lo, const void* const* his, void* y, int dtype, int64_t rows, int N, int J, const void* g0,
                                const void* g1, int L, int ext, double scale, int origin, void* stream) {
    WlSwt1dGrid g;
    const int rc = wl_swt1d_grid(rows, N, J, L, dtype, ext, origin, g);
    if (rc != 0) return rc;
    if (!lo || !y || !his) return WL_ERR_SHAPE;
    if (!g0 || !g1) return WL_ERR_TAPS;
    if (rows == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlSwt1dAdjArgs<T> a;
        a.lo = (const T*)lo; a.y = (T*)y;
        for (int l = 0; l < WL_SWT1D_MAXJ; ++l) a.hi[l] = l < J ? (const T*)his[l] : nullptr;
        a.g0 = (const float*)g0; a.g1 = (const float*)g1;
        a.rows = rows; a.waves = g.waves; a.len = N; a.nlev = J; a.tiles = g.tiles; a.core = g.core; a.origin = origin;
        a.scale = (float)scale;
        WL_SWT1D_BY_TAPS(WlSwt1dAdj, a, g, stream)
    });
}
#include "wl_wpt1d_api.inc"
