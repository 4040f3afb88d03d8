// ---- the 2-D wavelet packet level on packed band blocks (wl_wpt2d.h): included by wl_api.inc ------------------------------
// Tile geometry of a launch (see the head of wl_wpt2d.h): th x tw <= WL_WPT_TILE coefficients, as wide as the plane up to 32
// columns and then as tall as that allows; shrunk while its LDS exceeds WL_WPT_LDS_FLOATS (long filters on narrow planes).
// Planes of one tile and at most WL_WPT_RUN_MAX coefficients: np = WL_WPT_TILE / (th tw) planes per workgroup, as long as that
// leaves a workgroup per compute unit.  None of the three numbers has been measured.
#define WL_WPT_TILE 512
#define WL_WPT_RUN_MAX 256
#define WL_WPT_LDS_FLOATS 10240      // 40 KB: four workgroups per compute unit

template <typename K>
static void wl_wpt_geometry(typename K::Args& a, int rows, int cols, int64_t planes) {
    int w = cols < 32 ? cols : 32;
    int h = WL_WPT_TILE / w;
    if (h > rows) h = rows;
    while (h > 1 && K::lds_floats(h, w, 1) > WL_WPT_LDS_FLOATS) h = (h + 1) / 2;
    while (w > 1 && K::lds_floats(h, w, 1) > WL_WPT_LDS_FLOATS) w = (w + 1) / 2;
    int n = 1;
    if (h == rows && w == cols && h * w <= WL_WPT_RUN_MAX) {
        n = WL_WPT_TILE / (h * w);
        if (n > planes) n = (int)planes;
        while (n > 1 && (K::lds_floats(h, w, n) > WL_WPT_LDS_FLOATS || wl_cdiv64(planes, n) < (int64_t)wl_num_cus())) n = (n + 1) / 2;
    }
    K::set_geometry(a, h, w, n);
}

template <typename T, int LT>
static int wl_wpt_afb_launch(WlWptAfbArgs<T>& a, void* stream) {
    typedef WlWptAfb<T, LT, 1> K;
    wl_wpt_geometry<K>(a, a.Kh, a.Kw, a.planes);
    a.tiles_y = wl_cdiv(a.Kh, a.th); a.tiles_x = wl_cdiv(a.Kw, a.tw);
    const int64_t grid = wl_cdiv64(a.planes, a.np) * a.tiles_y * a.tiles_x;
    if (grid > 2147483647LL) return WL_ERR_UNSUPPORTED;
    return wl_launch<K>(a, grid, (size_t)K::lds_floats(a.th, a.tw, a.np) * sizeof(float), stream);
}

template <typename T, int LT>
static int wl_wpt_sfb_launch(WlWptSfbArgs<T>& a, void* stream) {
    typedef WlWptSfb<T, LT, 1> K;
    wl_wpt_geometry<K>(a, a.OH, a.OW, a.planes);
    a.tiles_y = wl_cdiv(a.OH, a.th); a.tiles_x = wl_cdiv(a.OW, a.tw);
    const int64_t grid = wl_cdiv64(a.planes, a.np) * a.tiles_y * a.tiles_x;
    if (grid > 2147483647LL) return WL_ERR_UNSUPPORTED;
    return wl_launch<K>(a, grid, (size_t)K::lds_floats(a.th, a.tw, a.np) * sizeof(float), stream);
}

// two levels per launch (periodization, sizes multiples of 4, L <= 12): fixed tiles, one plane per workgroup
template <typename T, int LT>
static int wl_wpt_afb2_launch(WlWptAfbArgs<T>& a, void* stream) {
    typedef WlWptAfb<T, LT, 2> K;
    a.tiles_y = wl_cdiv(a.Kh, K::TH); a.tiles_x = wl_cdiv(a.Kw, K::TW);
    const int64_t grid = a.planes * a.tiles_y * a.tiles_x;
    if (grid > 2147483647LL) return WL_ERR_UNSUPPORTED;
    return wl_launch<K>(a, grid, (size_t)K::kLdsFloats * sizeof(float), stream);
}

template <typename T, int LT>
static int wl_wpt_sfb2_launch(WlWptSfbArgs<T>& a, void* stream) {
    typedef WlWptSfb<T, LT, 2> K;
    a.tiles_y = wl_cdiv(a.OH, K::XH); a.tiles_x = wl_cdiv(a.OW, K::XW);
    const int64_t grid = a.planes * a.tiles_y * a.tiles_x;
    if (grid > 2147483647LL) return WL_ERR_UNSUPPORTED;
    return wl_launch<K>(a, grid, (size_t)K::kLdsFloats * sizeof(float), stream);
}

#define WL_WPT2_CASES(FN, ...)                                                                                         \
    switch (L) {                                                                                                       \
        case 2: return FN<T, 2>(__VA_ARGS__);   case 4: return FN<T, 4>(__VA_ARGS__);   case 6: return FN<T, 6>(__VA_ARGS__);   \
        case 8: return FN<T, 8>(__VA_ARGS__);   case 10: return FN<T, 10>(__VA_ARGS__); case 12: return FN<T, 12>(__VA_ARGS__); \
        default: return WL_ERR_UNSUPPORTED;                                                                            \
    }

#define WL_WPT_CASES(FN, ...)                                                                                          \
    switch (L) {                                                                                                       \
        case 2: return FN<T, 2>(__VA_ARGS__);   case 4: return FN<T, 4>(__VA_ARGS__);   case 6: return FN<T, 6>(__VA_ARGS__);   \
        case 8: return FN<T, 8>(__VA_ARGS__);   case 10: return FN<T, 10>(__VA_ARGS__); case 12: return FN<T, 12>(__VA_ARGS__); \
        case 14: return FN<T, 14>(__VA_ARGS__); case 16: return FN<T, 16>(__VA_ARGS__); case 18: return FN<T, 18>(__VA_ARGS__); \
        case 20: return FN<T, 20>(__VA_ARGS__); default: return WL_ERR_UNSUPPORTED;                                    \
    }

extern "C" int wl_wpt2d_analysis(const void* x, int64_t x_plane_stride, int x_row_stride, void* y, int dtype, int64_t planes,
                                 int H, int W, int nlev, const void* h_w_lo, const void* h_w_hi, const void* h_h_lo,
                                 const void* h_h_hi, int L, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (planes < 0 || H < 1 || W < 1 || nlev < 1 || x_row_stride < W || x_plane_stride < 0) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (nlev > 2) return WL_ERR_UNSUPPORTED;
    if ((L & 1) || L > 20 || wl_options().generic_only) return WL_ERR_UNSUPPORTED;
    if (nlev == 2) {
        // the wrap case only, and level 2 no shorter than the filter (the reference's single fold)
        if (mode != 2 || (H & 3) || (W & 3) || L > 12 || H / 2 < L - 1 || W / 2 < L - 1) return WL_ERR_UNSUPPORTED;
        if ((int64_t)H * W >= (1LL << 29) || (int64_t)H * x_row_stride >= (1LL << 30)) return WL_ERR_UNSUPPORTED;
        if (planes == 0) return 0;
        WL_DISPATCH_FLOAT(dtype, {
            WlWptAfbArgs<T> a;
            memset(&a, 0, sizeof(a));
            a.x = (const T*)x; a.y = (T*)y;
            a.h_w_lo = (const float*)h_w_lo; a.h_w_hi = (const float*)h_w_hi; a.h_h_lo = (const float*)h_h_lo; a.h_h_hi = (const float*)h_h_hi;
            a.planes = planes; a.x_ps = x_plane_stride; a.x_rs = x_row_stride;
            a.H = H; a.W = W; a.Kh = H / 4; a.Kw = W / 4;
            WL_WPT2_CASES(wl_wpt_afb2_launch, a, stream);
        });
    }
    // periodization of a plane shorter than the filter: the reference folds the wrapped tail once (wl_dwt_direct.h)
    if (mode == 2 && (H + (H & 1) < L - 1 || W + (W & 1) < L - 1)) return WL_ERR_UNSUPPORTED;
    // the kernels hold offsets inside a plane in 32 bits
    if ((int64_t)H * W >= (1LL << 29) || (int64_t)H * x_row_stride >= (1LL << 30)) return WL_ERR_UNSUPPORTED;
    if (planes == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlWptAfbArgs<T> a;
        memset(&a, 0, sizeof(a));
        a.x = (const T*)x; a.y = (T*)y;
        a.h_w_lo = (const float*)h_w_lo; a.h_w_hi = (const float*)h_w_hi; a.h_h_lo = (const float*)h_h_lo; a.h_h_hi = (const float*)h_h_hi;
        a.planes = planes; a.x_ps = x_plane_stride; a.x_rs = x_row_stride;
        a.H = H; a.W = W; a.Kh = wl_coeff_len(H, L, mode); a.Kw = wl_coeff_len(W, L, mode);
        a.base_h = wl_afb_base(H, L, mode); a.base_w = wl_afb_base(W, L, mode); a.ext = wl_mode_to_ext(mode);
        WL_WPT_CASES(wl_wpt_afb_launch, a, stream);
    });
}

extern "C" int wl_wpt2d_synthesis(const void* y, void* x_out, int dtype, int64_t planes, int Kh, int Kw, int OH, int OW, int nlev,
                                  const void* g_w_lo, const void* g_w_hi, const void* g_h_lo, const void* g_h_hi, int L,
                                  int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (planes < 0 || Kh < 1 || Kw < 1 || OH < 1 || OW < 1 || nlev < 1) return WL_ERR_SHAPE;
    if (nlev > 2) return WL_ERR_UNSUPPORTED;
    if ((L & 1) || L > 20 || wl_options().generic_only) return WL_ERR_UNSUPPORTED;
    if (nlev == 2) {                                                    // y (planes, 16, Kh, Kw) -> x (planes, 4 Kh, 4 Kw)
        if (OH > 4 * (int64_t)Kh || OW > 4 * (int64_t)Kw) return WL_ERR_SHAPE;
        if (mode != 2 || OH != 4 * Kh || OW != 4 * Kw || L > 12 || 2 * Kh < L - 1 || 2 * Kw < L - 1) return WL_ERR_UNSUPPORTED;
        if ((int64_t)OH * OW >= (1LL << 29)) return WL_ERR_UNSUPPORTED;
        if (planes == 0) return 0;
        WL_DISPATCH_FLOAT(dtype, {
            WlWptSfbArgs<T> a;
            memset(&a, 0, sizeof(a));
            a.y = (const T*)y; a.x = (T*)x_out;
            a.g_w_lo = (const float*)g_w_lo; a.g_w_hi = (const float*)g_w_hi; a.g_h_lo = (const float*)g_h_lo; a.g_h_hi = (const float*)g_h_hi;
            a.planes = planes; a.Kh = Kh; a.Kw = Kw; a.OH = OH; a.OW = OW; a.circ = 1; a.s = L / 2 - 1;
            WL_WPT2_CASES(wl_wpt_sfb2_launch, a, stream);
        });
    }
    if (Kh >= (1 << 29) || Kw >= (1 << 29)) return WL_ERR_UNSUPPORTED;
    const int fullH = mode == 2 ? 2 * Kh : 2 * Kh - L + 2, fullW = mode == 2 ? 2 * Kw : 2 * Kw - L + 2;
    if (OH > fullH || OW > fullW) return WL_ERR_SHAPE;
    if (mode == 2 && (2 * Kh < L - 2 || 2 * Kw < L - 2)) return WL_ERR_UNSUPPORTED;   // fewer outputs than taps: the single fold
    if ((int64_t)Kh * Kw >= (1LL << 29) || (int64_t)OH * OW >= (1LL << 30)) return WL_ERR_UNSUPPORTED;
    if (planes == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlWptSfbArgs<T> a;
        memset(&a, 0, sizeof(a));
        a.y = (const T*)y; a.x = (T*)x_out;
        a.g_w_lo = (const float*)g_w_lo; a.g_w_hi = (const float*)g_w_hi; a.g_h_lo = (const float*)g_h_lo; a.g_h_hi = (const float*)g_h_hi;
        a.planes = planes; a.Kh = Kh; a.Kw = Kw; a.OH = OH; a.OW = OW;
        a.circ = mode == 2;
        a.s = a.circ ? L / 2 - 1 : L - 2;
        WL_WPT_CASES(wl_wpt_sfb_launch, a, stream);
    });
}
#undef WL_WPT_CASES
#undef WL_WPT2_CASES
