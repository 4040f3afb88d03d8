// C ABI of the wave-tile kernels of the 1-D wavelet packet transform (wl_wpt1d.h).  Included at the end of wl_swt1d_api.inc, so
// compiled in the fourth translation unit of the HIP build (wl_dtinv_hip.hip) and in the matching unit of the host emulation.
#include "wl_api_common.h"
#include "wl_wpt1d.h"

// the grid of both kernels: tiles of `core` positions from -origin on, `head` positions of halo in front of each,
// WL_WPT1D_WAVES tiles per workgroup
struct WlWpt1dGrid { int head, core, tiles; int64_t waves, nblocks; };

static int wl_wpt1d_grid(int64_t rows, int len, int nlev, int L, int dtype, int mode, int origin, WlWpt1dGrid& g) {
    if (rows < 0 || len < 1 || nlev < 1 || L < 1 || origin < 0) return WL_ERR_SHAPE;
    if (dtype != WL_F32 && dtype != WL_F16 && dtype != WL_BF16) return dtype == WL_F64 ? WL_ERR_UNSUPPORTED : WL_ERR_DTYPE;
    if (nlev > WL_WPT1D_MAXJ || (L & 1) || L > WL_WPT1D_MAXL || mode != 2 || len >= (1 << 30)) return WL_ERR_UNSUPPORTED;
    const int q = 1 << nlev;
    // every level's band is even and at least as long as the filter (shorter: the reference's single fold is not the circular form)
    if (len % q != 0 || (len >> (nlev - 1)) < L) return WL_ERR_UNSUPPORTED;
    g.head = ((L / 2) * (q - 1) + q - 1) / q * q;
    g.core = 64 * WL_WPT1D_V - 2 * g.head;
    if (origin % q != 0 || origin >= g.core) return WL_ERR_SHAPE;
    g.tiles = wl_cdiv(len + origin, g.core);
    g.waves = rows * g.tiles;
    g.nblocks = wl_cdiv64(g.waves, WL_WPT1D_WAVES);
    return 0;
}

#define WL_WPT1D_BY_TAPS(K, a, g, stream)                                                      \
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

#define WL_WPT1D_ENTRY(K, from, to, t0, t1)                                                                                     \
    WlWpt1dGrid g;                                                                                                              \
    const int rc = wl_wpt1d_grid(rows, len, nlev, L, dtype, mode, origin, g);                                                   \
    if (rc != 0) return rc;                                                                                                     \
    if (!from || !to) return WL_ERR_SHAPE;                                                                                      \
    if (!t0 || !t1) return WL_ERR_TAPS;                                                                                         \
    if (rows == 0) return 0;                                                                                                    \
    WL_DISPATCH_FLOAT(dtype, {                                                                                                  \
        WlWpt1dArgs<T> a;                                                                                                       \
        a.src = (const T*)from; a.dst = (T*)to;                                                                                 \
        a.f0 = (const float*)t0; a.f1 = (const float*)t1;                                                                       \
        a.rows = rows; a.waves = g.waves; a.len = len; a.nlev = nlev; a.tiles = g.tiles; a.head = g.head; a.core = g.core;     \
        a.origin = origin;                                                                                                      \
        WL_WPT1D_BY_TAPS(K, a, g, stream)                                                                                       \
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
