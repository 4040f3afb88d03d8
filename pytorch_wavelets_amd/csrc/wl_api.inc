// C ABI implementation (include/wavelets_hip.h).  Included by wl_hip.hip (HIP backend) and by
// tests/emu/wl_emu.cpp (host emulation backend) AFTER the backend header, which provides
//   template <typename K> int wl_launch(const typename K::Args&, int64_t nblocks, size_t lds, void* stream);
// so that the launch-geometry logic below is the same code in both builds.
#include "../../include/wavelets_hip.h"
#include "wl_common.h"
#include "wl_api_common.h"
#include "wl_dt_api.h"
#include <string.h>
#include "wl_dwt_kernels.h"
#include "wl_dwt_tile.h"
#include "wl_dwt_tile_syn.h"
#include "wl_dwt_direct.h"
#include "wl_nonsep.h"
#include "wl_dwt_small.h"
#include "wl_filt1d.h"
#include "wl_swt2d.h"
#include "wl_iswt2d.h"
#include "wl_dwt3d.h"
#include "wl_wpt2d.h"
#include "wl_dtcwt_kernels.h"
#include "wl_dtcwt_tile.h"
#include "wl_dtcwt_rot.h"
#include "wl_dtcwt_small.h"

// ---- kernel functors -------------------------------------------------------------------------
template <typename T>
struct WlAfb2dTile {
    typedef WlAfb2dArgs<T> Args;
    static const int kThreads = 256;
    static const int kMinWaves = 1;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) { wl_afb2d_tile_body<T>(a, ctx); }
};
template <typename T>
struct WlSfb2dTile {
    typedef WlSfb2dArgs<T> Args;
    static const int kThreads = 256;
    static const int kMinWaves = 1;
    static WL_DEV void run(const Args& a, const WlCtx& ctx) { wl_sfb2d_tile_body<T>(a, ctx); }
};

extern "C" int wl_version(void) { return 220; }
extern "C" const char* wl_backend(void) { return WL_BACKEND_NAME; }
extern "C" int wl_dwt_coeff_len(int n, int L, int mode) { return wl_coeff_len(n, L, mode); }

// ---- runtime options ---------------------------------------------------------------------------------------------
// Read from the environment ONCE (first use) and changeable through wl_set_option(); nothing on the launch path calls
// getenv.  generic_only: route every operator to the runtime-L generic kernels (the tests compare the two families).
struct WlOptions {
    int generic_only;
    int no_stream;   // 1: the DTCWT / ScatLayer operators skip their streaming kernels (A/B measurements, tests of the tile kernels)
    int scat_stream; // 1: the ScatLayer forward may use the streaming level-1 kernel too (measured no faster: off)
    WlOptions() {
        const char* v = getenv("WL_GENERIC_ONLY");
        generic_only = (v && *v) ? atoi(v) : 0;
        no_stream = 0;
        scat_stream = 0;
    }
};
static WlOptions& wl_options() { static WlOptions o; return o; }
extern "C" int wl_set_option(const char* name, int value) {
    if (!name) return WL_ERR_SHAPE;
    if (!strcmp(name, "generic_only")) { wl_options().generic_only = value; return 0; }
    if (!strcmp(name, "no_stream")) { wl_options().no_stream = value; return 0; }
    if (!strcmp(name, "scat_stream")) { wl_options().scat_stream = value; return 0; }
    return WL_ERR_UNSUPPORTED;
}
extern "C" int wl_get_option(const char* name) {
    if (!name) return WL_ERR_SHAPE;
    if (!strcmp(name, "generic_only")) return wl_options().generic_only;
    if (!strcmp(name, "no_stream")) return wl_options().no_stream;
    if (!strcmp(name, "scat_stream")) return wl_options().scat_stream;
    return WL_ERR_UNSUPPORTED;
}
extern "C" const char* wl_last_kernel(void) { return wl_last_kernel_name(); }
extern "C" const char* wl_kernel_history(int back) { return wl_kernel_history_name(back); }
extern "C" long long wl_launch_count(void) { return wl_launch_count_value(); }
extern "C" long long wl_last_grid(void) { return wl_last_grid_value(); }
// for the entry points that live in the other translation units: 1 when the streaming kernels are switched off
int wl_streaming_off() { return wl_options().no_stream || wl_options().generic_only; }

// ---- DWT analysis ------------------------------------------------------------------------------
template <typename T>
static int wl_afb2d_generic(const WlAfbReq& r) {
    typedef typename WlAcc<T>::type A;
    const int H = r.H, W = r.W, Lw = r.Lw, Lh = r.Lh, mode = r.mode;
    WlAfb2dArgs<T> a;
    a.x = (const T*)r.x; a.ll = (T*)r.ll; a.highs = (T*)r.highs;
    a.h_w_lo = (const A*)r.taps.w_lo; a.h_w_hi = (const A*)r.taps.w_hi; a.h_h_lo = (const A*)r.taps.h_lo; a.h_h_hi = (const A*)r.taps.h_hi;
    a.NC = r.planes; a.H = H; a.W = W;
    a.x_ps = r.x_ps; a.ll_ps = r.ll_ps; a.x_rs = r.x_rs; a.ll_rs = r.ll_rs;
    a.Kh = wl_dwt_coeff_len(H, Lh, mode); a.Kw = wl_dwt_coeff_len(W, Lw, mode);
    a.Lw = Lw; a.Lh = Lh;
    a.basew = wl_afb_base(W, Lw, mode); a.baseh = wl_afb_base(H, Lh, mode);
    a.extw = a.exth = wl_mode_to_ext(mode);
    // tile: shrink until the LDS budget fits (long filters)
    int TH = 16, TW = 64;
    if (a.Kw <= 32) TW = 32;
    if (a.Kh <= 8) TH = 8;
    for (;;) {
        a.TH = TH; a.TW = TW;
        a.nrows = 2 * TH + Lh - 2; a.ncols = 2 * TW + Lw - 2;
        a.spitch = a.ncols | 1;
        if (wl_afb2d_tile_lds(a) <= 64 * 1024 || (TH <= 4 && TW <= 16)) break;
        if (TW > 16) TW /= 2; else TH /= 2;
    }
    a.tiles_x = wl_cdiv(a.Kw, TW); a.tiles_y = wl_cdiv(a.Kh, TH);
    return wl_launch<WlAfb2dTile<T> >(a, r.planes * a.tiles_x * a.tiles_y, wl_afb2d_tile_lds(a), r.stream);
}

// ---- specialised tile kernel (even tap counts, float / half data) ---------------------------------------

template <typename T, int LT, int TH = 16, int TW = 64, int SH = 0, int V4 = 0>
static int wl_afb_tile_launch(const WlAfbReq& r) {
    typedef WlAfbTile<T, LT, TH, TW, SH, V4> K;
    const int64_t planes = r.planes;
    const int H = r.H, W = r.W, mode = r.mode;
    WlAfbTileArgs<T> a;
    a.x = (const T*)r.x; a.ll = (T*)r.ll; a.highs = (T*)r.highs;
    a.h_w_lo = (const float*)r.taps.w_lo; a.h_w_hi = (const float*)r.taps.w_hi;
    a.h_h_lo = (const float*)r.taps.h_lo; a.h_h_hi = (const float*)r.taps.h_hi;
    a.NC = planes; a.H = H; a.W = W;
    a.x_ps = r.x_ps; a.ll_ps = r.ll_ps; a.x_rs = r.x_rs; a.ll_rs = r.ll_rs;
    a.Kh = wl_dwt_coeff_len(H, LT, mode); a.Kw = wl_dwt_coeff_len(W, LT, mode);
    a.base = wl_afb_base(W, LT, mode);
    a.ext = wl_mode_to_ext(mode);
    a.tiles_x = wl_cdiv(a.Kw, K::TW); a.tiles_y = wl_cdiv(a.Kh, K::TH);
    if (a.tiles_x > 1 && a.Kw - (a.tiles_x - 1) * K::TW <= K::XT) --a.tiles_x;   // the last tile absorbs a short remainder
    a.vec_ok = (r.x_rs % 2 == 0) && (r.x_ps % 2 == 0) && ((uintptr_t)r.x % (2 * sizeof(T)) == 0);
    // tiles per workgroup: whole tile rows unless that leaves too few workgroups to fill the chip
    int run = a.tiles_x;
    while (run > 1 && planes * a.tiles_y * wl_cdiv(a.tiles_x, run) < 2048) run = (run + 1) / 2;
    a.run_len = run; a.runs_x = wl_cdiv(a.tiles_x, run);
    a.nblocks = 0;   // XCD-aware remap measured neutral for this kernel: off
    return wl_launch<K>(a, planes * a.tiles_y * a.runs_x, (size_t)K::kLdsFloats * sizeof(float), r.stream);
}

template <typename T>
static int wl_afb_tile_dispatch(const WlAfbReq& r) {   // (Lw == Lh)
    if ((int64_t)r.H * r.W >= (1LL << 30) || (int64_t)r.H * r.x_rs >= (1LL << 30) || (int64_t)r.H * r.ll_rs >= (1LL << 30))
        return WL_ERR_UNSUPPORTED;
    // float16 rows that allow it are staged with four-element (8-byte) loads: the staged origin 2*kw0 + base - SH is a
    // multiple of four columns when (base - SH) is, and the rows must be 8-byte aligned
    const bool q4 = sizeof(T) == 2 && (r.x_rs % 4 == 0) && (r.x_ps % 4 == 0) && ((uintptr_t)r.x % 8 == 0);
#define WL_CASE(LT_)                                                                                                  \
    case LT_: {                                                                                                       \
        const int base = wl_afb_base(r.W, LT_, r.mode);                                                               \
        const bool v4 = q4 && ((base - (base & 1)) % 4 == 0);                                                         \
        if (base & 1)                                                                                                 \
            return v4 ? wl_afb_tile_launch<T, LT_, 16, 64, 1, sizeof(T) == 2>(r) : wl_afb_tile_launch<T, LT_, 16, 64, 1, 0>(r); \
        return v4 ? wl_afb_tile_launch<T, LT_, 16, 64, 0, sizeof(T) == 2>(r) : wl_afb_tile_launch<T, LT_, 16, 64, 0, 0>(r);     \
    }
    switch (r.Lw) {
        // (14 and 18 taps - db7 / sym7, db9 / sym9 - since round 5: without an instantiation every narrow level of theirs fell to the
        // run-time-tap kernel, 0.73 ms for a 128 x 3 x 512 x 512 db7 forward against 0.31 ms)
        WL_CASE(2); WL_CASE(4); WL_CASE(6); WL_CASE(8); WL_CASE(10); WL_CASE(12); WL_CASE(14); WL_CASE(16); WL_CASE(18); WL_CASE(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASE
}

extern "C" int wl_dwt2d_analysis_strided(const void* x, int64_t x_plane_stride, int x_row_stride, void* ll,
                                         int64_t ll_plane_stride, int ll_row_stride, void* highs, int dtype,
                                         int64_t planes, int H, int W, const void* h_w_lo, const void* h_w_hi, int Lw,
                                 const void* h_h_lo, const void* h_h_hi, int Lh, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (Lw < 1 || Lh < 1 || Lw > WL_MAX_TAPS || Lh > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (x_row_stride < W || ll_row_stride < wl_dwt_coeff_len(W, Lw, mode) || x_plane_stride < 0 || ll_plane_stride < 0)
        return WL_ERR_SHAPE;
    if (planes == 0) return 0;
    const WlAfbReq r = {x, x_plane_stride, x_row_stride, ll, ll_plane_stride, ll_row_stride, highs, planes, H, W,
                        {h_w_lo, h_w_hi, h_h_lo, h_h_hi}, Lw, Lh, mode, 0, nullptr, nullptr, stream};
    if (mode == 2 && (H + (H & 1) < Lh - 1 || W + (W & 1) < Lw - 1)) {
        // a level shorter than the filter: the reference folds the wrapped tail only once (dwt/lowlevel.py:146-150),
        // which is not the circular form of the tile kernels - evaluate its formula literally (tiny planes)
        WL_DISPATCH_DTYPE(dtype, {
            typedef typename WlAcc<T>::type A;
            WlDirectArgs<T> a;
            a.x = (const T*)r.x; a.highs = nullptr; a.ll = (T*)r.ll; a.hout = (T*)r.highs;
            a.w_lo = (const A*)r.taps.w_lo; a.w_hi = (const A*)r.taps.w_hi; a.h_lo = (const A*)r.taps.h_lo; a.h_hi = (const A*)r.taps.h_hi;
            a.NC = r.planes; a.x_ps = r.x_ps; a.ll_ps = r.ll_ps; a.x_rs = r.x_rs; a.ll_rs = r.ll_rs;
            a.H = r.H; a.W = r.W; a.Kh = wl_dwt_coeff_len(r.H, r.Lh, r.mode); a.Kw = wl_dwt_coeff_len(r.W, r.Lw, r.mode);
            a.Lw = r.Lw; a.Lh = r.Lh; a.OH = a.OW = 0;
            return wl_launch<WlAfbDirect<T> >(a, wl_cdiv64(r.planes * a.Kh * a.Kw, 256), 0, r.stream);
        });
    }
    if (Lw == Lh && dtype != WL_F64 && !wl_options().generic_only) {
        int rc = dtype == WL_F32    ? wl_afb_tile_dispatch<float>(r)
                 : dtype == WL_F16  ? wl_afb_tile_dispatch<wl_half>(r)
                 : dtype == WL_BF16 ? wl_afb_tile_dispatch<wl_bf16>(r)
                                    : WL_ERR_DTYPE;
        if (rc != WL_ERR_UNSUPPORTED) return rc;
    }
    WL_DISPATCH_DTYPE(dtype, return wl_afb2d_generic<T>(r));
    return 0;
}

extern "C" int wl_dwt2d_analysis(const void* x, void* ll, void* highs, int dtype, int64_t planes, int H,
                                 int W, const void* h_w_lo, const void* h_w_hi, int Lw,
                                 const void* h_h_lo, const void* h_h_hi, int Lh, int mode, void* stream) {
    // dense layouts; invalid arguments are reported by the strided entry in the usual order (mode, shape, taps)
    const bool ok = H >= 1 && W >= 1 && Lw >= 1 && Lh >= 1;
    const int Kh = ok ? wl_dwt_coeff_len(H, Lh, mode) : 1, Kw = ok ? wl_dwt_coeff_len(W, Lw, mode) : 1;
    return wl_dwt2d_analysis_strided(x, ok ? (int64_t)H * W : 1, ok ? W : 1, ll, (int64_t)Kh * Kw, Kw, highs, dtype, planes, H, W, h_w_lo,
                                     h_w_hi, Lw, h_h_lo, h_h_hi, Lh, mode, stream);
}

// ---- DWT synthesis -----------------------------------------------------------------------------
template <typename T>
static int wl_sfb2d_generic(const WlSfbReq& r) {
    typedef typename WlAcc<T>::type A;
    const int OH = r.OH, OW = r.OW, Lw = r.Lw, Lh = r.Lh;
    WlSfb2dArgs<T> a;
    a.ll = (const T*)r.ll; a.highs = (const T*)r.highs; a.y = (T*)r.y;
    a.g_w_lo = (const A*)r.taps.w_lo; a.g_w_hi = (const A*)r.taps.w_hi; a.g_h_lo = (const A*)r.taps.h_lo; a.g_h_hi = (const A*)r.taps.h_hi;
    a.NC = r.planes; a.ll_plane_stride = r.ll_ps; a.ll_row_stride = r.ll_rs;
    a.Kh = r.Kh; a.Kw = r.Kw; a.OH = OH; a.OW = OW; a.Lw = Lw; a.Lh = Lh;
    a.circ = (r.mode == 2);
    a.sw = a.circ ? Lw / 2 - 1 : Lw - 2;
    a.sh = a.circ ? Lh / 2 - 1 : Lh - 2;
    int TH = 16, TW = 64;
    if (OW <= 32) TW = 32;
    if (OH <= 8) TH = 8;
    for (;;) {
        a.TH = TH; a.TW = TW;
        a.nkr = (TH + Lh) / 2 + 1; a.nkc = (TW + Lw) / 2 + 1;
        if (wl_sfb2d_tile_lds(a) <= 64 * 1024 || (TH <= 4 && TW <= 16)) break;
        if (TW > 16) TW /= 2; else TH /= 2;
    }
    a.tiles_x = wl_cdiv(OW, TW); a.tiles_y = wl_cdiv(OH, TH);
    return wl_launch<WlSfb2dTile<T> >(a, r.planes * a.tiles_x * a.tiles_y, wl_sfb2d_tile_lds(a), r.stream);
}

template <typename T, int LT, int SODD>
static int wl_sfb_tile_launch(const WlSfbReq& r) {
    typedef WlSfbTile<T, LT, SODD> K;
    WlSfbTileArgs<T> a;
    a.ll = (const T*)r.ll; a.highs = (const T*)r.highs; a.y = (T*)r.y;
    a.g_w_lo = (const float*)r.taps.w_lo; a.g_w_hi = (const float*)r.taps.w_hi;
    a.g_h_lo = (const float*)r.taps.h_lo; a.g_h_hi = (const float*)r.taps.h_hi;
    a.NC = r.planes; a.ll_plane_stride = r.ll_ps; a.ll_row_stride = r.ll_rs;
    a.Kh = r.Kh; a.Kw = r.Kw; a.OH = r.OH; a.OW = r.OW;
    a.circ = (r.mode == 2);
    a.s = a.circ ? LT / 2 - 1 : LT - 2;
    a.tiles_x = wl_cdiv(r.OW, K::TW); a.tiles_y = wl_cdiv(r.OH, K::TH);
    a.nblocks = r.planes * a.tiles_x * a.tiles_y;   // XCD-aware remap: halo rows meet in one L2
    return wl_launch<K>(a, r.planes * a.tiles_x * a.tiles_y, (size_t)K::kLdsFloats * sizeof(float), r.stream);
}

template <typename T>
static int wl_sfb_tile_dispatch(const WlSfbReq& r) {   // (Lw == Lh)
    if ((int64_t)r.OH * r.OW >= (1LL << 30) || r.ll_ps >= (1LL << 30) || (int64_t)r.Kh * r.ll_rs >= (1LL << 30))
        return WL_ERR_UNSUPPORTED;
#define WL_CASE(LT_)                                                                                                     \
    case LT_:                                                                                                            \
        return ((r.mode == 2 ? LT_ / 2 - 1 : LT_ - 2) & 1) ? wl_sfb_tile_launch<T, LT_, 1>(r) : wl_sfb_tile_launch<T, LT_, 0>(r)
    switch (r.Lw) {
        // (14 and 18 taps - db7 / sym7, db9 / sym9 - since round 5: without an instantiation every narrow level of theirs fell to the
        // run-time-tap kernel, 0.73 ms for a 128 x 3 x 512 x 512 db7 forward against 0.31 ms)
        WL_CASE(2); WL_CASE(4); WL_CASE(6); WL_CASE(8); WL_CASE(10); WL_CASE(12); WL_CASE(14); WL_CASE(16); WL_CASE(18); WL_CASE(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASE
}

extern "C" int wl_dwt2d_synthesis(const void* ll, int64_t ll_plane_stride, int ll_row_stride,
                                  const void* highs, void* y, int dtype, int64_t planes, int Kh, int Kw,
                                  int OH, int OW, const void* g_w_lo, const void* g_w_hi, int Lw,
                                  const void* g_h_lo, const void* g_h_hi, int Lh, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (Lw < 1 || Lh < 1 || Lw > WL_MAX_TAPS || Lh > WL_MAX_TAPS) return WL_ERR_TAPS;
    const int fullH = mode == 2 ? 2 * Kh : 2 * Kh - Lh + 2;
    const int fullW = mode == 2 ? 2 * Kw : 2 * Kw - Lw + 2;
    if (planes < 0 || Kh < 1 || Kw < 1 || OH < 1 || OW < 1 || OH > fullH || OW > fullW) return WL_ERR_SHAPE;
    if (planes == 0) return 0;
    const WlSfbReq r = {ll, ll_plane_stride, ll_row_stride, highs, y, planes, Kh, Kw, OH, OW,
                        {g_w_lo, g_w_hi, g_h_lo, g_h_hi}, Lw, Lh, mode, 0, nullptr, nullptr, stream};
    if (mode == 2 && (2 * Kh < Lh - 2 || 2 * Kw < Lw - 2)) {
        // fewer outputs than taps: the reference's single fold (dwt/lowlevel.py:256-260), evaluated literally
        WL_DISPATCH_DTYPE(dtype, {
            typedef typename WlAcc<T>::type A;
            WlDirectArgs<T> a;
            a.x = (const T*)r.ll; a.highs = (const T*)r.highs; a.ll = (T*)r.y; a.hout = nullptr;
            a.w_lo = (const A*)r.taps.w_lo; a.w_hi = (const A*)r.taps.w_hi; a.h_lo = (const A*)r.taps.h_lo; a.h_hi = (const A*)r.taps.h_hi;
            a.NC = r.planes; a.x_ps = r.ll_ps; a.ll_ps = 0; a.x_rs = r.ll_rs; a.ll_rs = 0;
            a.H = a.W = 0; a.Kh = r.Kh; a.Kw = r.Kw; a.Lw = r.Lw; a.Lh = r.Lh; a.OH = r.OH; a.OW = r.OW;
            return wl_launch<WlSfbDirect<T> >(a, wl_cdiv64(r.planes * r.OH * r.OW, 256), 0, r.stream);
        });
    }
    if (Lw == Lh && dtype != WL_F64 && !wl_options().generic_only) {
        int rc = dtype == WL_F32    ? wl_sfb_tile_dispatch<float>(r)
                 : dtype == WL_F16  ? wl_sfb_tile_dispatch<wl_half>(r)
                 : dtype == WL_BF16 ? wl_sfb_tile_dispatch<wl_bf16>(r)
                                    : WL_ERR_DTYPE;
        if (rc != WL_ERR_UNSUPPORTED) return rc;
    }
    WL_DISPATCH_DTYPE(dtype, return wl_sfb2d_generic<T>(r));
    return 0;
}

// ---- non-separable one-level analysis / synthesis (wl_nonsep.h; reference dwt/lowlevel.py:524-597, :746-798) ----
extern "C" int wl_dwt2d_analysis_nonsep(const void* x, void* y, int dtype, int64_t planes, int H, int W, const void* f,
                                        int Ly, int Lx, int mode, void* stream) {
    const int ext = wl_mode_to_ext(mode);
    if (ext < 0 || mode == 6) return WL_ERR_MODE;   // the reference's afb2d_nonsep has no 'periodic' branch (:572)
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (Ly < 1 || Lx < 1 || Ly > WL_MAX_TAPS || Lx > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (mode == 2 && (Ly - 1 > H + (H & 1) || Lx - 1 > W + (W & 1))) return WL_ERR_UNSUPPORTED;   // more than one wrap
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        typedef typename WlAcc<T>::type A;
        WlNonsepArgs<T> a;
        a.x = (const T*)x; a.y = (T*)y; a.f = (const A*)f; a.planes = planes;
        a.H = H; a.W = W; a.Ly = Ly; a.Lx = Lx; a.ext = ext; a.per = mode == 2; a.OH = a.OW = 0;
        a.Kh = wl_coeff_len(H, Ly, mode); a.Kw = wl_coeff_len(W, Lx, mode);
        a.oy = mode == 2 ? (Ly + 1) / 2 - (Ly - 1) : -(Ly - 2);
        a.ox = mode == 2 ? (Lx + 1) / 2 - (Lx - 1) : -(Lx - 2);
        return wl_launch<WlAfbNonsep<T> >(a, wl_cdiv64(planes * a.Kh * a.Kw, 256), 0, stream);
    });
    return 0;
}

extern "C" int wl_dwt2d_synthesis_nonsep(const void* coeffs, void* y, int dtype, int64_t planes, int Kh, int Kw,
                                         int OH, int OW, const void* g, int Ly, int Lx, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (Ly < 1 || Lx < 1 || Ly > WL_MAX_TAPS || Lx > WL_MAX_TAPS) return WL_ERR_TAPS;
    const int fullH = mode == 2 ? 2 * Kh : 2 * Kh - Ly + 2, fullW = mode == 2 ? 2 * Kw : 2 * Kw - Lx + 2;
    if (planes < 0 || Kh < 1 || Kw < 1 || OH < 1 || OW < 1 || OH > fullH || OW > fullW) return WL_ERR_SHAPE;
    if (mode == 2 && (Ly - 2 > 2 * Kh || Lx - 2 > 2 * Kw)) return WL_ERR_UNSUPPORTED;             // more than one wrap
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        typedef typename WlAcc<T>::type A;
        WlNonsepArgs<T> a;
        a.x = (const T*)coeffs; a.y = (T*)y; a.f = (const A*)g; a.planes = planes;
        a.H = a.W = 0; a.Kh = Kh; a.Kw = Kw; a.OH = OH; a.OW = OW; a.Ly = Ly; a.Lx = Lx; a.ext = 0; a.per = mode == 2;
        a.oy = mode == 2 ? Ly / 2 - 1 : Ly - 2;
        a.ox = mode == 2 ? Lx / 2 - 1 : Lx - 2;
        return wl_launch<WlSfbNonsep<T> >(a, wl_cdiv64(planes * OH * OW, 256), 0, stream);
    });
    return 0;
}

// gradient of wl_dwt2d_analysis_nonsep with respect to x, every mode (the true adjoint of gather + correlation, as
// autograd gives it upstream): dy (planes,4,Kh,Kw) -> dx (planes,H,W)
extern "C" int wl_dwt2d_analysis_nonsep_bwd(const void* dy, void* dx, int dtype, int64_t planes, int H, int W,
                                            const void* f, int Ly, int Lx, int mode, void* stream) {
    const int ext = wl_mode_to_ext(mode);
    if (ext < 0 || mode == 6) return WL_ERR_MODE;
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (Ly < 1 || Lx < 1 || Ly > WL_MAX_TAPS || Lx > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (mode == 2 && (Ly - 1 > H + (H & 1) || Lx - 1 > W + (W & 1))) return WL_ERR_UNSUPPORTED;   // as the forward
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        typedef typename WlAcc<T>::type A;
        WlNonsepArgs<T> a;
        a.x = (const T*)dy; a.y = (T*)dx; a.f = (const A*)f; a.planes = planes;
        a.H = H; a.W = W; a.Ly = Ly; a.Lx = Lx; a.ext = ext; a.per = mode == 2; a.OH = a.OW = 0;
        a.Kh = wl_coeff_len(H, Ly, mode); a.Kw = wl_coeff_len(W, Lx, mode);
        a.oy = mode == 2 ? (Ly + 1) / 2 - (Ly - 1) : -(Ly - 2);
        a.ox = mode == 2 ? (Lx + 1) / 2 - (Lx - 1) : -(Lx - 2);
        return wl_launch<WlAfbNonsepAdj<T> >(a, wl_cdiv64(planes * H * W, 256), 0, stream);
    });
    return 0;
}

// gradient of wl_dwt2d_synthesis_nonsep with respect to the coefficients: dy (planes,OH,OW) with OH = 2Kh-Ly+2 (2Kh
// for periodization) -> dc (planes,4,Kh,Kw); an analysis of dy with the synthesis point-spread functions
extern "C" int wl_dwt2d_synthesis_nonsep_bwd(const void* dy, void* dc, int dtype, int64_t planes, int Kh, int Kw,
                                             const void* g, int Ly, int Lx, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (Ly < 1 || Lx < 1 || Ly > WL_MAX_TAPS || Lx > WL_MAX_TAPS) return WL_ERR_TAPS;
    const int OH = mode == 2 ? 2 * Kh : 2 * Kh - Ly + 2, OW = mode == 2 ? 2 * Kw : 2 * Kw - Lx + 2;
    if (planes < 0 || Kh < 1 || Kw < 1 || OH < 1 || OW < 1) return WL_ERR_SHAPE;
    if (mode == 2 && (Ly - 2 > 2 * Kh || Lx - 2 > 2 * Kw)) return WL_ERR_UNSUPPORTED;             // as the forward
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        typedef typename WlAcc<T>::type A;
        WlNonsepArgs<T> a;
        a.x = (const T*)dy; a.y = (T*)dc; a.f = (const A*)g; a.planes = planes;
        a.H = OH; a.W = OW; a.Kh = Kh; a.Kw = Kw; a.Ly = Ly; a.Lx = Lx; a.OH = a.OW = 0; a.per = mode == 2;
        a.ext = mode == 2 ? WL_EXT_PERIODIC : WL_EXT_ZERO;
        a.oy = mode == 2 ? -(Ly / 2 - 1) : -(Ly - 2);
        a.ox = mode == 2 ? -(Lx / 2 - 1) : -(Lx - 2);
        return wl_launch<WlAfbNonsep<T> >(a, wl_cdiv64(planes * Kh * Kw, 256), 0, stream);
    });
    return 0;
}

// =================================================================================================
// DTCWT
// =================================================================================================
#define WL_FUNCTOR(NAME, ARGS, BODY)                                                         \
    template <typename T> struct NAME {                                                      \
        typedef ARGS<T> Args;                                                                \
        static const int kThreads = 256;                                                     \
        static const int kMinWaves = 1;                                                      \
        static WL_DEV void run(const Args& a, const WlCtx& ctx) { BODY<T>(a, ctx); }        \
    };
WL_FUNCTOR(WlDtFwd1, WlDtFwd1Args, wl_dtcwt_fwd1_body)
WL_FUNCTOR(WlDtFwd2, WlDtFwd2Args, wl_dtcwt_fwd2_body)
WL_FUNCTOR(WlDtInv1, WlDtInv1Args, wl_dtcwt_inv1_body)
WL_FUNCTOR(WlDtInv2, WlDtInv2Args, wl_dtcwt_inv2_body)
#undef WL_FUNCTOR

// specialised tile kernels (wl_dtcwt_tile.h): float / half data and the reference's filter lengths only
// output tiles of the level >= 2 DTCWT tile kernels
#ifndef WL_INV2_TH
#define WL_INV2_TH 16
#define WL_INV2_TW 64
#endif
#ifndef WL_FWD2_TH
#define WL_FWD2_TH 16
#define WL_FWD2_TW 64
#endif
template <typename T>
struct WlDtTile {
    template <int L0, int L1, int COMB>
    static int fwd1_launch2(WlDtFwd1Args<T>& a, int64_t units, void* stream) {
        typedef WlDtFwd1Tile<T, L0, L1, COMB> K;
        a.TH = K::TH; a.TW = K::TW;
        a.tiles_x = wl_cdiv(a.We, K::TW); a.tiles_y = wl_cdiv(a.He, K::TH);
        int run = a.tiles_x;   // whole tile rows unless that leaves too few workgroups to fill the chip
        while (run > 1 && units * a.tiles_y * wl_cdiv(a.tiles_x, run) < 2048) run = (run + 1) / 2;
        a.run_len = run; a.runs_x = wl_cdiv(a.tiles_x, run);
        a.nblocks = 0;
        return wl_launch<K>(a, units * a.tiles_y * a.runs_x, (size_t)K::kLdsFloats * sizeof(float), stream);
    }
    template <int L0, int L1>
    static int fwd1_launch(WlDtFwd1Args<T>& a, int64_t units, void* stream) {
        return a.combine ? fwd1_launch2<L0, L1, 1>(a, units, stream) : fwd1_launch2<L0, L1, 0>(a, units, stream);
    }
    static int fwd1(WlDtFwd1Args<T>& a, int64_t units, void* stream) {
        if (a.L0 == 5 && a.L1 == 7) return fwd1_launch<5, 7>(a, units, stream);       // near_sym_a
        if (a.L0 == 13 && a.L1 == 19) return fwd1_launch<13, 19>(a, units, stream);   // near_sym_b
        if (a.L0 == 9 && a.L1 == 7) return fwd1_launch<9, 7>(a, units, stream);       // antonini
        if (a.L0 == 5 && a.L1 == 3) return fwd1_launch<5, 3>(a, units, stream);       // legall
        return WL_ERR_UNSUPPORTED;
    }
    template <int L>
    static int fwd2_launch(WlDtFwd2Args<T>& a, void* stream) {
        typedef WlDtFwd2Tile<T, L, WL_FWD2_TH, WL_FWD2_TW> K;
        a.TH = K::THO; a.TW = K::TWO;
        a.tiles_x = wl_cdiv(a.We / 2, K::TWO); a.tiles_y = wl_cdiv(a.He / 2, K::THO);
        a.nblocks = 0;
        return wl_launch<K>(a, a.NC * a.tiles_x * a.tiles_y, (size_t)K::kLdsFloats * sizeof(float), stream);
    }
    static int fwd2(WlDtFwd2Args<T>& a, void* stream) {
        switch (a.L) {
            case 10: return fwd2_launch<10>(a, stream);   // qshift_06, qshift_a
            case 14: return fwd2_launch<14>(a, stream);   // qshift_b
            case 16: return fwd2_launch<16>(a, stream);   // qshift_c
            case 18: return fwd2_launch<18>(a, stream);   // qshift_d
            default: return WL_ERR_UNSUPPORTED;
        }
    }
    template <int L0, int L1, int SCAT>
    static int inv1_launch(WlDtInv1Args<T>& a, void* stream) {
        typedef WlDtInv1Tile<T, L0, L1, SCAT> K;
        a.TH = K::TH; a.TW = K::TW;
        a.tiles_x = wl_cdiv(a.W, K::TW); a.tiles_y = wl_cdiv(a.H, K::TH);
        a.nblocks = a.NC * a.tiles_x * a.tiles_y;
        return wl_launch<K>(a, a.NC * a.tiles_x * a.tiles_y, (size_t)K::kLdsFloats * sizeof(float), stream);
    }
    static int inv1(WlDtInv1Args<T>& a, void* stream) {
        if (a.L0 == 7 && a.L1 == 5) return inv1_launch<7, 5, 0>(a, stream);       // near_sym_a
        if (a.L0 == 19 && a.L1 == 13) return inv1_launch<19, 13, 0>(a, stream);   // near_sym_b
        if (a.L0 == 7 && a.L1 == 9) return inv1_launch<7, 9, 0>(a, stream);       // antonini
        if (a.L0 == 3 && a.L1 == 5) return inv1_launch<3, 5, 0>(a, stream);       // legall
        if (a.L0 == 5 && a.L1 == 7) return inv1_launch<5, 7, 0>(a, stream);       // backward of the forward level 1
        return WL_ERR_UNSUPPORTED;
    }
    static int scat_bwd(WlDtInv1Args<T>& a, void* stream) {   // taps = the FORWARD biort pair
        if (a.L0 == 5 && a.L1 == 7) return inv1_launch<5, 7, 1>(a, stream);       // near_sym_a
        if (a.L0 == 13 && a.L1 == 19) return inv1_launch<13, 19, 1>(a, stream);   // near_sym_b
        return WL_ERR_UNSUPPORTED;
    }
    template <int L>
    static int inv2_launch(WlDtInv2Args<T>& a, void* stream) {
        typedef WlDtInv2Tile<T, L, WL_INV2_TH, WL_INV2_TW> K;
        a.TH = K::TH; a.TW = K::TW;
        a.tiles_x = wl_cdiv(2 * a.w, K::TW); a.tiles_y = wl_cdiv(2 * a.h, K::TH);
        a.nblocks = a.NC * a.tiles_x * a.tiles_y;
        return wl_launch<K>(a, a.NC * a.tiles_x * a.tiles_y, (size_t)K::kLdsFloats * sizeof(float), stream);
    }
    static int inv2(WlDtInv2Args<T>& a, void* stream) {
        switch (a.L) {
            case 10: return inv2_launch<10>(a, stream);
            case 14: return inv2_launch<14>(a, stream);
            case 16: return inv2_launch<16>(a, stream);
            case 18: return inv2_launch<18>(a, stream);
            default: return WL_ERR_UNSUPPORTED;
        }
    }
};
template <>
struct WlDtTile<double> {
    static int fwd1(WlDtFwd1Args<double>&, int64_t, void*) { return WL_ERR_UNSUPPORTED; }
    static int fwd2(WlDtFwd2Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
    static int inv1(WlDtInv1Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
    static int scat_bwd(WlDtInv1Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
    static int inv2(WlDtInv2Args<double>&, void*) { return WL_ERR_UNSUPPORTED; }
};

// small planes, several per workgroup (wl_dtcwt_small.h): even sizes up to 64 x 64, the tabulated level-1 pairs, no colour
// combination, float32 / float16
static unsigned wl_magic(unsigned d) { return d <= 1 ? 0u : (unsigned)((0x100000000ULL + d - 1) / d); }
template <typename T, int LA, int LB>
static int wl_dtfwd1_small_launch(WlDtFwd1Args<T> a, void* stream) {
    const int M = WlDtFwd1Small<T, LA, LB>::M;
    if (M > a.H || M > a.W) return WL_ERR_UNSUPPORTED;             // one fold of the extension
    const int He = a.H + 2 * M, We = a.W + 2 * M;
    const int per_plane = (He * We + 2 * He * a.W) * 4;            // the extended plane + its (lo, hi) rows
    // (measured: at 55 KiB per plane - 64 x 64 - one plane per workgroup and two workgroups per CU lose to the tile kernel,
    // 0.101 against 0.055 ms; 32 x 32 planes win, 0.038 against 0.054)
    if (per_plane > 24 * 1024) return WL_ERR_UNSUPPORTED;
    int G = 40 * 1024 / per_plane;
    if (G < 1) G = 1;
    if (G > 16) G = 16;
    const int64_t want = 2 * (int64_t)wl_num_cus();
    if (a.NC / G < want) G = (int)(a.NC / want);
    if (G < 1) G = 1;
    while (G > 1 && (int64_t)G * He * We >= 65536) --G;
    if ((int64_t)G * He * We >= 65536) return WL_ERR_UNSUPPORTED;
    a.run_len = G;
    a.mg_q = wl_magic((unsigned)(He * We)); a.mg_w = wl_magic((unsigned)We); a.mg_w2 = wl_magic((unsigned)a.W);
    a.nblocks_q = wl_magic((unsigned)((a.H / 2) * (a.W / 2))); a.mg_qc = wl_magic((unsigned)(a.W / 2));
    const size_t lds = 4 * ((size_t)wl_align_up(G * He * We, 4) + 2 * (size_t)G * He * a.W);
    return wl_launch<WlDtFwd1Small<T, LA, LB> >(a, (a.NC + G - 1) / G, lds, stream);
}
template <typename T>
static int wl_dtfwd1_small(const WlDtFwd1Args<T>& a, void* stream) {
    typedef typename WlAcc<T>::type A;
    if (sizeof(A) != 4 || a.combine || a.He != a.H || a.We != a.W || a.H < 2 || a.W < 2 || a.H * a.W > 4096 || a.NC < 16) return WL_ERR_UNSUPPORTED;
    if (wl_options().no_stream) return WL_ERR_UNSUPPORTED;        // (the tests of the tile kernels)
    if (a.L0 == 5 && a.L1 == 7) return wl_dtfwd1_small_launch<T, 5, 7>(a, stream);        // near_sym_a
    if (a.L0 == 13 && a.L1 == 19) return wl_dtfwd1_small_launch<T, 13, 19>(a, stream);    // near_sym_b
    if (a.L0 == 9 && a.L1 == 7) return wl_dtfwd1_small_launch<T, 9, 7>(a, stream);         // antonini
    if (a.L0 == 5 && a.L1 == 3) return wl_dtfwd1_small_launch<T, 5, 3>(a, stream);         // legall
    return WL_ERR_UNSUPPORTED;
}

// Level 1 forward / ScatLayer forward of the struct an entry built (wl_dtfwd1_args + its outputs): the streaming kernels of the strip
// unit (wl_dt_api.h), the small-plane kernel, the tile kernels, the generic kernel - the first that takes the case.
template <typename T>
static int wl_dtfwd1_launch(WlDtFwd1Args<T>& a, void* stream) {
    const int64_t units = a.combine ? a.NC / 3 : a.NC;
    if ((int64_t)a.He * a.We < (1LL << 30) && !wl_options().generic_only) {
        int rc = wl_options().no_stream ? WL_ERR_UNSUPPORTED : wl_dtfwd1_lean(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
        rc = (wl_options().no_stream || (a.z && !wl_options().scat_stream)) ? WL_ERR_UNSUPPORTED : wl_dtfwd1_strip(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
        rc = wl_dtfwd1_small(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
        rc = WlDtTile<T>::fwd1(a, units, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
    }
    a.TH = 16; a.TW = 64;
    while (wl_dtfwd1_lds(a) > 60 * 1024 && a.TW > 16) a.TW /= 2;
    a.tiles_x = wl_cdiv(a.We, a.TW); a.tiles_y = wl_cdiv(a.He, a.TH);
    return wl_launch<WlDtFwd1<T> >(a, units * a.tiles_x * a.tiles_y, wl_dtfwd1_lds(a), stream);
}

static int wl_dt_ext(int mode) { return mode == 1 ? WL_EXT_SYM : WL_EXT_ZERO; }   // dtcwt/lowlevel.py:75-79

extern "C" int wl_dtcwt_fwd_level1(const void* x, void* ll, void* highs, int dtype, int64_t planes, int H, int W,
                                   const void* h0, int L0, const void* h1, int L1, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0 && mode != 3 && mode != 5) return WL_ERR_MODE;
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (!(L0 & 1) || !(L1 & 1)) return WL_ERR_UNSUPPORTED;   // even-length level-1 filters change the output size
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtFwd1Args<T> a = wl_dtfwd1_args<T>(x, planes, 1, H, W, h0, L0, h1, L1, wl_dt_ext(mode));
        a.ll = (T*)ll; a.highs = (T*)highs;
        return wl_dtfwd1_launch(a, stream);
    });
    return 0;
}

extern "C" int wl_scat_fwd_level1(const void* x, void* z, void* drdx, void* drdy, void* ll, int dtype, int64_t N, int C,
                                  int H, int W, const void* h0, int L0, const void* h1, int L1, int mode, double magbias,
                                  int combine_colour, void* stream) {
    if (wl_mode_to_ext(mode) < 0 && mode != 3 && mode != 5) return WL_ERR_MODE;
    if (N < 0 || C < 1 || H < 1 || W < 1 || (combine_colour && C != 3)) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (!(L0 & 1) || !(L1 & 1)) return WL_ERR_UNSUPPORTED;
    if (N == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtFwd1Args<T> a = wl_dtfwd1_args<T>(x, N * C, C, H, W, h0, L0, h1, L1, wl_dt_ext(mode));
        a.ll = (T*)ll; a.z = (T*)z; a.drdx = (T*)drdx; a.drdy = (T*)drdy;
        a.combine = combine_colour; a.magbias = (WlDtFwd1Args<T>::A)magbias;
        return wl_dtfwd1_launch(a, stream);
    });
    return 0;
}

// ScatLayerj2 (reference scatternet/lowlevel.py:205-295) assembles its (N, 49, C, H/4, W/4) output from three transforms; with
// these two entry points every one of them writes its entries where they belong - no concatenation afterwards.
extern "C" int wl_scat_fwd_level1_into(const void* x, void* z, int64_t z_batch_stride, int64_t z_ll_offset, int64_t z_mag_offset,
                                       void* ll, int dtype, int64_t N, int C, int H, int W, const void* h0, int L0, const void* h1,
                                       int L1, int mode, double magbias, void* stream) {
    if (wl_mode_to_ext(mode) < 0 && mode != 3 && mode != 5) return WL_ERR_MODE;
    if (N < 0 || C < 1 || H < 1 || W < 1 || !z) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (!(L0 & 1) || !(L1 & 1)) return WL_ERR_UNSUPPORTED;
    if (N == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtFwd1Args<T> a = wl_dtfwd1_args<T>(x, N * C, C, H, W, h0, L0, h1, L1, wl_dt_ext(mode));
        a.ll = (T*)ll; a.z = (T*)z; a.magbias = (WlDtFwd1Args<T>::A)magbias;
        a.z_bs = z_batch_stride; a.z_ll_off = z_ll_offset; a.z_mag_off = z_mag_offset;   // the caller places the entries
        return wl_dtfwd1_launch(a, stream);
    });
    return 0;
}

extern "C" int wl_scat_fwd_level2_into(const void* x, void* z, int64_t z_batch_stride, int64_t z_ll_offset, int64_t z_mag_offset,
                                       int dtype, int64_t N, int C, int H, int W, const void* h0a, const void* h0b,
                                       const void* h1a, const void* h1b, int L, double magbias, void* stream) {
    if (N < 0 || C < 1 || H < 4 || W < 4 || !z) return WL_ERR_SHAPE;
    if (L < 2 || L > WL_MAX_TAPS || (L & 1)) return WL_ERR_TAPS;
    if ((H & 3) || (W & 3)) return WL_ERR_UNSUPPORTED;               // (ScatLayerj2 pads its input to a multiple of 8)
    if (N == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {                                       // (the streaming kernel or none)
        WlDtFwd2Args<T> a = wl_dtfwd2_args<T>(x, N * C, H, W, h0a, h0b, h1a, h1b, L);
        a.z = (T*)z; a.z_bs = z_batch_stride; a.z_ll_off = z_ll_offset; a.z_mag_off = z_mag_offset;
        a.C = C; a.magbias = (WlDtFwd2Args<T>::A)magbias;
        return wl_streaming_off() ? WL_ERR_UNSUPPORTED : wl_dtfwd2_lean(a, stream);
    });
    return 0;
}

// ---- level 1 with the band-pass diagonal ('near_sym_b_bp'; wl_dtcwt_rot.h; reference dtcwt/transform_funcs.py:124-149,
// scatternet/lowlevel.py:140-182) ----
template <typename T>
static int wl_dtfwd1_rot_run(WlDtRotArgs<T>& a, int scat, void* stream) {
    typedef typename WlAcc<T>::type A;
    if (scat && a.ext == WL_EXT_SYM && !wl_streaming_off() && !(a.H & 1) && !(a.W & 1)) {
        // ScatLayer inference on wide planes that fill the chip: the lean streaming kernel with a third row filter and window
        // (wl_dtcwt_fused.h MODE 6) writes the same (N, 7, C, H/2, W/2) tensor
        WlDtFwd1Args<T> f = wl_dtfwd1_args<T>(a.x, a.planes, a.C, a.H, a.W, a.h0, a.L0, a.h1, a.L1, a.ext);
        f.z = a.re; f.magbias = (A)a.bias;
        const int rc = wl_dtrot_lean(f, a.h2, a.L2, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
    }
    const int M = WlDtFwd1Rot<T, 0>::M;
    a.in_pitch = 64 + 2 * M + 1;
    int TH = 32;
    for (;; TH /= 2) {                                             // (float64: 16 rows)
        if (TH < 8) return WL_ERR_UNSUPPORTED;
        a.mid_off = wl_align_up((TH + 2 * M) * a.in_pitch * (int)sizeof(A), 16);
        a.lds_bytes = a.mid_off + 3 * (TH + 2 * M) * 64 * (int)sizeof(A);
        if (a.lds_bytes <= 64 * 1024) break;
    }
    a.TH = TH;
    a.tiles_x = wl_cdiv(a.W, 64); a.tiles_y = wl_cdiv(a.H, TH);
    a.nblocks = a.planes * a.tiles_x * a.tiles_y;
    if (scat) return wl_launch<WlDtFwd1Rot<T, 1> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
    return wl_launch<WlDtFwd1Rot<T, 0> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

extern "C" int wl_dtcwt_fwd_level1_rot(const void* x, void* ll, void* re, void* im, int dtype, int64_t N, int C, int H, int W,
                                       const void* h0, int L0, const void* h1, int L1, const void* h2, int L2, int mode,
                                       int scat, double magbias, void* stream) {
    if (wl_mode_to_ext(mode) < 0 && mode != 3 && mode != 5) return WL_ERR_MODE;
    if (N < 0 || C < 1 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || L2 < 1 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS || L2 > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (!(L0 & 1) || !(L1 & 1) || !(L2 & 1)) return WL_ERR_UNSUPPORTED;   // even-length level-1 filters change the output size
    if (L0 > 19 || L1 > 19 || L2 > 19) return WL_ERR_UNSUPPORTED;          // (the kernel's unrolled, zero-padded tap window)
    if ((H & 1) || (W & 1)) return WL_ERR_UNSUPPORTED;                     // q2c pairs rows and columns (the modules pad first)
    if ((int64_t)H * W >= (1LL << 30)) return WL_ERR_UNSUPPORTED;
    if (N == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtRotArgs<T> a = wl_dtrot_args<T>(x, ll, re, im, N * C, C, H, W, h0, L0, h1, L1, h2, L2, wl_dt_ext(mode), magbias);
        return wl_dtfwd1_rot_run(a, scat, stream);
    });
    return 0;
}

template <typename T>
static int wl_dtfwd2_launch(WlDtFwd2Args<T>& a, void* stream) {
    if ((int64_t)a.H * a.W < (1LL << 30) && !wl_options().generic_only) {
        int rc = wl_options().no_stream ? WL_ERR_UNSUPPORTED : wl_dtfwd2_lean(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
        rc = WlDtTile<T>::fwd2(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
    }
    a.TH = 16; a.TW = 32;
    while (wl_dtfwd2_lds(a) > 60 * 1024 && a.TW > 8) a.TW /= 2;
    while (wl_dtfwd2_lds(a) > 60 * 1024 && a.TH > 4) a.TH /= 2;
    a.tiles_x = wl_cdiv(a.We / 2, a.TW); a.tiles_y = wl_cdiv(a.He / 2, a.TH);
    return wl_launch<WlDtFwd2<T> >(a, a.NC * a.tiles_x * a.tiles_y, wl_dtfwd2_lds(a), stream);
}

extern "C" int wl_dtcwt_fwd_level2(const void* x, void* ll, void* highs, int dtype, int64_t planes, int H, int W,
                                   const void* h0a, const void* h0b, const void* h1a, const void* h1b, int L,
                                   void* stream) {
    if (planes < 0 || H < 2 || W < 2 || (H & 1) || (W & 1)) return WL_ERR_SHAPE;
    if (L < 2 || L > WL_MAX_TAPS || (L & 1)) return WL_ERR_TAPS;
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtFwd2Args<T> a = wl_dtfwd2_args<T>(x, planes, H, W, h0a, h0b, h1a, h1b, L);
        a.ll = (T*)ll; a.highs = (T*)highs;
        return wl_dtfwd2_launch(a, stream);
    });
    return 0;
}

template <typename T>
static int wl_dtinv1_launch(WlDtInv1Args<T>& a, void* stream) {
    if ((int64_t)a.H * a.W < (1LL << 30) && a.ll_plane_stride < (1LL << 30) && (int64_t)a.H * a.ll_row_stride < (1LL << 30) &&
        !wl_options().generic_only) {
        int rc = wl_options().no_stream ? WL_ERR_UNSUPPORTED : wl_dtinv1_strip(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
        rc = WlDtTile<T>::inv1(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
    }
    a.TH = 16; a.TW = 64;
    while (wl_dtinv1_lds(a) > 60 * 1024 && a.TW > 16) a.TW /= 2;
    while (wl_dtinv1_lds(a) > 60 * 1024 && a.TH > 4) a.TH /= 2;
    a.tiles_x = wl_cdiv(a.W, a.TW); a.tiles_y = wl_cdiv(a.H, a.TH);
    return wl_launch<WlDtInv1<T> >(a, a.NC * a.tiles_x * a.tiles_y, wl_dtinv1_lds(a), stream);
}

extern "C" int wl_dtcwt_inv_level1(const void* ll, int64_t ll_plane_stride, int ll_row_stride, const void* highs,
                                   void* y, int dtype, int64_t planes, int H, int W, const void* g0, int L0,
                                   const void* g1, int L1, int mode, void* stream) {
    if (planes < 0 || H < 2 || W < 2 || (H & 1) || (W & 1)) return WL_ERR_SHAPE;
    if (!ll && !highs) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (!(L0 & 1) || !(L1 & 1)) return WL_ERR_UNSUPPORTED;
    if (planes == 0) return 0;
    // the reference ignores `mode` (always symmetric) when there are no highpass inputs (transform_funcs.py:158-159)
    const int ext = highs ? wl_dt_ext(mode) : WL_EXT_SYM;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtInv1Args<T> a = wl_dtinv1_args<T>(y, planes, 1, H, W, g0, L0, g1, L1, ext);
        a.ll = (const T*)ll; a.highs = (const T*)highs; a.ll_plane_stride = ll_plane_stride; a.ll_row_stride = ll_row_stride;
        return wl_dtinv1_launch(a, stream);
    });
    return 0;
}

template <typename T>
static int wl_scat_bwd_launch(WlDtInv1Args<T>& a, void* stream) {
    if ((int64_t)a.H * a.W >= (1LL << 30)) return WL_ERR_UNSUPPORTED;
    // wide planes that fill the chip: the streaming level-1 inverse with the scattering prologue in its stagers
    const int rc = wl_options().no_stream ? WL_ERR_UNSUPPORTED : wl_dtinv1_strip(a, stream);
    if (rc != WL_ERR_UNSUPPORTED) return rc;
    return WlDtTile<T>::scat_bwd(a, stream);
}

/* ScatLayer backward = ScatLayerj1_f.backward (scatternet/lowlevel.py:114-137) in one launch: dx (N,C,H,W) with H, W
 * the padded-to-even input size, from dz (the gradient of z), and the drdx/drdy saved by wl_scat_fwd_level1.
 * h0/h1 are the FORWARD level-1 taps (the adjoint of fwd_j1 is inv_j1 with the same taps).  Specialised kernels
 * only: returns WL_ERR_UNSUPPORTED for other tap counts / float64 (callers then compose the prologue themselves). */
extern "C" int wl_scat_bwd_level1(const void* dz, const void* drdx, const void* drdy, void* dx, int dtype, int64_t N,
                                  int C, int H, int W, const void* h0, int L0, const void* h1, int L1, int mode,
                                  int combine_colour, void* stream) {
    if (wl_mode_to_ext(mode) < 0 && mode != 3 && mode != 5) return WL_ERR_MODE;
    if (N < 0 || C < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || (combine_colour && C != 3)) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (wl_options().generic_only) return WL_ERR_UNSUPPORTED;
    if (N == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtInv1Args<T> a = wl_dtinv1_args<T>(dx, N * C, C, H, W, h0, L0, h1, L1, wl_dt_ext(mode));
        a.sz = (const T*)dz; a.sdx = (const T*)drdx; a.sdy = (const T*)drdy; a.combine = combine_colour;
        return wl_scat_bwd_launch(a, stream);
    });
    return 0;
}

template <typename T>
static int wl_dtinv2_launch(WlDtInv2Args<T>& a, void* stream) {
    if ((int64_t)a.h * a.w < (1LL << 28) && a.ll_plane_stride < (1LL << 30) && (int64_t)a.h * a.ll_row_stride < (1LL << 30) &&
        !wl_options().generic_only) {
        int rc = wl_options().no_stream ? WL_ERR_UNSUPPORTED : wl_dtinv2_strip(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
        rc = WlDtTile<T>::inv2(a, stream);
        if (rc != WL_ERR_UNSUPPORTED) return rc;
    }
    a.TH = 16; a.TW = 64;
    while (wl_dtinv2_lds(a) > 60 * 1024 && a.TW > 16) a.TW /= 2;
    a.tiles_x = wl_cdiv(2 * a.w, a.TW); a.tiles_y = wl_cdiv(2 * a.h, a.TH);
    return wl_launch<WlDtInv2<T> >(a, a.NC * a.tiles_x * a.tiles_y, wl_dtinv2_lds(a), stream);
}

extern "C" int wl_dtcwt_inv_level2(const void* ll, int64_t ll_plane_stride, int ll_row_stride, const void* highs,
                                   void* y, int dtype, int64_t planes, int h, int w, const void* g0a,
                                   const void* g0b, const void* g1a, const void* g1b, int L, void* stream) {
    if (planes < 0 || h < 2 || w < 2 || (h & 1) || (w & 1)) return WL_ERR_SHAPE;
    if (!ll && !highs) return WL_ERR_SHAPE;
    if (L < 2 || L > WL_MAX_TAPS || (L & 1)) return WL_ERR_TAPS;
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        WlDtInv2Args<T> a = wl_dtinv2_args<T>(ll, ll_plane_stride, ll_row_stride, highs, y, planes, h, w, g0a, g0b, g1a, g1b, L);
        return wl_dtinv2_launch(a, stream);
    });
    return 0;
}

// =================================================================================================
// single-axis building blocks (wl_filt1d.h)
// =================================================================================================
extern "C" int wl_corr1d(const void* x, void* y0, void* y1, int dtype, int64_t outer, int n, int64_t inner,
                         int64_t y_outer_stride, int K, const void* h0, const void* h1, int tap_offset, int tap_stride,
                         int ntaps, int start, int step, int tap_step, int ext, int out_offset, int out_stride,
                         void* stream) {
    if (outer < 0 || n < 1 || inner < 1 || K < 0 || ntaps < 1 || ntaps > WL_MAX_TAPS || tap_stride < 1) return WL_ERR_SHAPE;
    if (ext < 0 || ext > WL_EXT_PER_FOLD1) return WL_ERR_MODE;
    if (ext == WL_EXT_PER_FOLD1 && (step != 2 || tap_step != 1 || start != 1 - ntaps)) return WL_ERR_SHAPE;
    if (outer == 0 || K == 0) return 0;
    {   // the kernel holds extended positions in an int: the last one a thread forms must be one (a row within a filter length of 2^31)
        const int64_t last = (int64_t)start + (int64_t)step * (K - 1) + (int64_t)tap_step * (ntaps - 1) + (ext == WL_EXT_PER_FOLD1 ? (int64_t)n + 1 : 0);
        if (last > 2147483647LL) return WL_ERR_UNSUPPORTED;
    }
    WL_DISPATCH_DTYPE(dtype, {
        typedef typename WlAcc<T>::type A;
        WlCorr1dArgs<T> a;
        a.x = (const T*)x; a.y0 = (T*)y0; a.y1 = (T*)y1; a.h0 = (const A*)h0; a.h1 = (const A*)h1;
        a.outer = outer; a.inner = inner; a.y_outer_stride = y_outer_stride;
        a.n = n; a.K = K; a.nt = ntaps; a.t0 = tap_offset; a.ts = tap_stride;
        a.start = start; a.step = step; a.dstep = tap_step; a.ext = ext; a.q0 = out_offset; a.qs = out_stride;
        return wl_launch<WlCorr1d<T> >(a, wl_cdiv64(outer * K * inner, 256), 0, stream);
    });
    return 0;
}

// ---- multi-level analysis of small planes, several planes per workgroup (wl_dwt_small.h; reference dwt/transform2d.py:63-74) ----
template <typename T, int LT>
static int wl_afb_small_launch(WlSmallArgs<T>& a, void* stream) {
    return wl_launch<WlAfbSmall<T, LT> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
static int wl_afb_small_run(const WlAfbPyrReq& r) {
    const int SZ = (int)sizeof(T);
    const int64_t planes = r.planes;
    const int H = r.H, W = r.W, nlev = r.nlev, L = r.L, mode = r.mode;
    WlSmallArgs<T> a;
    a.x = (const T*)r.x; a.yl = (T*)r.yl;
    for (int j = 0; j < WL_SMALL_MAXLEV; ++j) a.yh[j] = j < nlev ? (T*)r.yh[j] : nullptr;
    a.hw_lo = (const float*)r.taps.w_lo; a.hw_hi = (const float*)r.taps.w_hi; a.hh_lo = (const float*)r.taps.h_lo; a.hh_hi = (const float*)r.taps.h_hi;
    a.planes = planes; a.nlev = nlev; a.L = L; a.ext = wl_mode_to_ext(mode);
    a.h[0] = H; a.w[0] = W;
    for (int j = 0; j < WL_SMALL_MAXLEV; ++j) {
        a.base_h[j] = a.base_w[j] = 0; a.mg_k[j] = 0;
        a.kf_w[j] = a.ki_w[j] = a.kf_h[j] = a.ki_h[j] = 0;
        a.mg_r1[j] = a.mg_k1[j] = a.mg_r2[j] = a.mg_k2[j] = a.mg_c1[j] = a.mg_c2[j] = 0;
        if (j >= nlev) { a.h[j + 1] = a.h[j]; a.w[j + 1] = a.w[j]; continue; }
        // periodization of a level shorter than the filter: the reference folds the wrapped tail once (dwt/lowlevel.py:146-150),
        // which is not the circular form this kernel evaluates - the per-level kernels reproduce it
        if (mode == 2 && (a.h[j] + (a.h[j] & 1) < L - 1 || a.w[j] + (a.w[j] & 1) < L - 1)) return WL_ERR_UNSUPPORTED;
        a.h[j + 1] = wl_coeff_len(a.h[j], L, mode); a.w[j + 1] = wl_coeff_len(a.w[j], L, mode);
        a.base_h[j] = wl_afb_base(a.h[j], L, mode); a.base_w[j] = wl_afb_base(a.w[j], L, mode);
    }
    // one fold / wrap reaches every sample a level reads?  (positions base .. 2 (K - 1) + base + L - 1 of a length-n signal)
    int fold1 = 1;
    for (int j = 0; j < nlev; ++j) {
        const int nn[2] = {a.h[j], a.w[j]}, kk[2] = {a.h[j + 1], a.w[j + 1]}, bb[2] = {a.base_h[j], a.base_w[j]};
        for (int d = 0; d < 2; ++d) {
            const int lo = bb[d], hi = 2 * (kk[d] - 1) + bb[d] + L - 1, n = nn[d];
            const int reach = a.ext == WL_EXT_REFL ? n - 1 : n;     // how far beyond either end one fold reaches
            if (a.ext != WL_EXT_ZERO && (lo < -reach || hi > n - 1 + reach)) fold1 = 0;
        }
    }
    if (!fold1) return WL_ERR_UNSUPPORTED;                          // a filter longer than a level: the per-level kernels
    // LDS per plane: the two buffers the levels ping-pong between (the plane and ll_2, ll_1 and ll_3) and the (lo, hi) rows of a
    // level - the largest of each over the levels (a level of a short signal under a long filter is LARGER than its input)
    int b0 = H * W, b1 = 1, mid0 = 1;
    for (int j = 0; j < nlev; ++j) {
        const int out = a.h[j + 1] * a.w[j + 1], m = a.h[j] * a.w[j + 1] * 2;
        if (j + 1 < nlev) { if ((j + 1) & 1) { if (out > b1) b1 = out; } else if (out > b0) b0 = out; }
        if (m > mid0) mid0 = m;
    }
    const int in0 = b0, ll1 = b1;
    const int per_plane = (in0 + ll1 + mid0) * 4;
    if (per_plane > 56 * 1024) return WL_ERR_UNSUPPORTED;          // planes beyond ~72 x 72: the streaming kernels
    if (H * W > 4 * 256 * WlAfbSmall<T, 0>::PRE) return WL_ERR_UNSUPPORTED;   // (the planes of a group travel through PRE 16-byte registers per thread)
    int G = 40 * 1024 / per_plane;
    if (G < 1) G = 1;
    if (G > 16) G = 16;
    while (G > 1 && G * H * W > 4 * 256 * WlAfbSmall<T, 0>::PRE) --G;
    const int64_t want = 2 * (int64_t)wl_num_cus();                 // workgroups for every CU before more planes per workgroup
    if (planes / G < want) G = (int)(planes / want);
    if (G < 1) G = 1;
    int most = 1;                                                   // elements a pass of a level indexes per plane
    for (int j = 0; j < nlev; ++j) {
        if (a.h[j] * a.w[j + 1] > most) most = a.h[j] * a.w[j + 1];
        if (a.h[j + 1] * a.w[j + 1] > most) most = a.h[j + 1] * a.w[j + 1];
    }
    while (G > 1 && (int64_t)G * most >= 65536) --G;                // (the index arithmetic divides by multiplication: 16-bit range)
    if ((int64_t)G * most >= 65536) return WL_ERR_UNSUPPORTED;
    a.G = G;
    for (int j = 0; j < nlev; ++j) {
        a.mg_k[j] = wl_magic((unsigned)a.w[j + 1]);
        // interior outputs of either axis: 2k + base >= 0 and 2k + base + L <= n
        const int nn[2] = {a.w[j], a.h[j]}, kk[2] = {a.w[j + 1], a.h[j + 1]}, bb[2] = {a.base_w[j], a.base_h[j]};
        int kf[2], ki[2];
        for (int d = 0; d < 2; ++d) {
            kf[d] = bb[d] < 0 ? (-bb[d] + 1) / 2 : 0;
            int kl = nn[d] - L - bb[d];                              // 2 k <= kl
            kl = kl >= 0 ? kl / 2 : -1;
            if (kl > kk[d] - 1) kl = kk[d] - 1;
            ki[d] = kl >= kf[d] ? kl - kf[d] + 1 : 0;
            if (ki[d] == 0) kf[d] = 0;
        }
        a.kf_w[j] = kf[0]; a.ki_w[j] = ki[0]; a.kf_h[j] = kf[1]; a.ki_h[j] = ki[1];
        a.mg_r1[j] = wl_magic((unsigned)(a.h[j] * ki[0])); a.mg_k1[j] = wl_magic((unsigned)ki[0]);
        a.mg_r2[j] = wl_magic((unsigned)(a.h[j] * (a.w[j + 1] - ki[0]))); a.mg_k2[j] = wl_magic((unsigned)(a.w[j + 1] - ki[0]));
        a.mg_c1[j] = wl_magic((unsigned)(ki[1] * a.w[j + 1])); a.mg_c2[j] = wl_magic((unsigned)((a.h[j + 1] - ki[1]) * a.w[j + 1]));
    }
    a.buf_off[0] = 0;
    a.buf_off[1] = wl_align_up(G * in0 * 4, 16);
    a.mid_off = a.buf_off[1] + wl_align_up(G * ll1 * 4, 16);
    a.tap_off = a.mid_off + wl_align_up(G * mid0 * 4, 16);
    a.lds_bytes = a.tap_off + 4 * L * 4;
    a.vec_ok = ((H * W) % 4 == 0) && ((int64_t)G * H * W * SZ) % 16 == 0 && (uintptr_t)r.x % 16 == 0;
    a.nblocks = (planes + G - 1) / G;                               // groups; a workgroup walks over several when the chip is full
    int per_cu = 160 * 1024 / a.lds_bytes;
    if (per_cu > 8) per_cu = 8;
    const int64_t resident = (int64_t)per_cu * wl_num_cus();
    if (a.nblocks > resident) a.nblocks = resident;
    switch (L) {
        case 2: return wl_afb_small_launch<T, 2>(a, r.stream);
        case 4: return wl_afb_small_launch<T, 4>(a, r.stream);
        case 6: return wl_afb_small_launch<T, 6>(a, r.stream);
        case 8: return wl_afb_small_launch<T, 8>(a, r.stream);
        default: return wl_afb_small_launch<T, 0>(a, r.stream);
    }
}

extern "C" int wl_dwt2d_analysis_small(const void* x, void* yl, void* const* yh, int dtype, int64_t planes, int H, int W,
                                       int nlev, const void* h_w_lo, const void* h_w_hi, const void* h_h_lo,
                                       const void* h_h_hi, int L, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (nlev < 1 || nlev > WL_SMALL_MAXLEV || L > 20) return WL_ERR_UNSUPPORTED;
    if (planes == 0) return 0;
    const WlAfbPyrReq r = {x, (int64_t)H * W, W, yl, yh, planes, H, W, nlev, {h_w_lo, h_w_hi, h_h_lo, h_h_hi}, L, mode,
                           0, 0, nullptr, nullptr, stream};
    WL_DISPATCH_FLOAT(dtype, return wl_afb_small_run<T>(r));
}

template <typename T>
static int wl_sfb_small_run(const WlSfbPyrReq& r) {
    const int64_t planes = r.planes;
    const int yl_h = r.yl_h, yl_w = r.yl_w, nlev = r.nlev, L = r.L, mode = r.mode;
    const int* const Kh = r.Kh; const int* const Kw = r.Kw;
    void* const stream = r.stream;
    WlSmallSynArgs<T> a;
    a.yl = (const T*)r.yl; a.y = (T*)r.y; a.planes = planes; a.nlev = nlev; a.L = L; a.per = mode == 2;
    a.gw_lo = (const float*)r.taps.w_lo; a.gw_hi = (const float*)r.taps.w_hi; a.gh_lo = (const float*)r.taps.h_lo; a.gh_hi = (const float*)r.taps.h_hi;
    a.llh = yl_h; a.llw = yl_w;
    int hsum = 0, b[2] = {yl_h * yl_w, 1}, mid0 = 1, most = 1;
    int sh = yl_h, sw = yl_w;                                       // size of the ll a level receives
    for (int j = 0; j < WL_SMALL_MAXLEV; ++j) { a.yh[j] = nullptr; a.Kh[j] = a.Kw[j] = a.OH[j] = a.OW[j] = 1; a.mg_pk[j] = a.mg_k[j] = a.mg_pq[j] = a.mg_q[j] = 0; a.h_off[j] = 0; }
    for (int j = nlev - 1; j >= 0; --j) {
        a.yh[j] = (const T*)r.yh[j];
        a.Kh[j] = Kh[j]; a.Kw[j] = Kw[j];
        if (Kh[j] < 1 || Kw[j] < 1) return WL_ERR_SHAPE;
        // the lowpass a level receives is its high-pass size or one larger (then the surplus row / column is dropped: 'unpad')
        if (!(Kh[j] <= sh && sh <= Kh[j] + 1 && Kw[j] <= sw && sw <= Kw[j] + 1)) return WL_ERR_UNSUPPORTED;
        a.OH[j] = mode == 2 ? 2 * Kh[j] : 2 * Kh[j] - L + 2;
        a.OW[j] = mode == 2 ? 2 * Kw[j] : 2 * Kw[j] - L + 2;
        if (a.OH[j] < 1 || a.OW[j] < 1) return WL_ERR_UNSUPPORTED;
        sh = a.OH[j]; sw = a.OW[j];
        hsum += 3 * Kh[j] * Kw[j];
        const int out = a.OH[j] * a.OW[j], m = a.OH[j] * Kw[j] * 2;
        if (j > 0) { const int which = (nlev - j) & 1; if (out > b[which]) b[which] = out; }
        if (m > mid0) mid0 = m;
        if (out > most) most = out;
        if (a.OH[j] * Kw[j] > most) most = a.OH[j] * Kw[j];
    }
    const int per_plane = (hsum + b[0] + b[1] + mid0) * 4;
    if (per_plane > 56 * 1024) return WL_ERR_UNSUPPORTED;
    int G = 40 * 1024 / per_plane;
    if (G < 1) G = 1;
    if (G > 16) G = 16;
    const int64_t want = 2 * (int64_t)wl_num_cus();
    if (planes / G < want) G = (int)(planes / want);
    if (G < 1) G = 1;
    while (G > 1 && (int64_t)G * most >= 65536) --G;
    if ((int64_t)G * most >= 65536) return WL_ERR_UNSUPPORTED;
    a.G = G;
    int off = 0;
    for (int j = 0; j < nlev; ++j) {
        a.h_off[j] = off; off += wl_align_up(G * 3 * Kh[j] * Kw[j] * 4, 16);
        a.mg_pk[j] = a.OH[j] * Kw[j] == 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)(a.OH[j] * Kw[j]) - 1) / (unsigned)(a.OH[j] * Kw[j]));
        a.mg_k[j] = Kw[j] == 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)Kw[j] - 1) / (unsigned)Kw[j]);
        a.mg_pq[j] = a.OH[j] * a.OW[j] == 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)(a.OH[j] * a.OW[j]) - 1) / (unsigned)(a.OH[j] * a.OW[j]));
        a.mg_q[j] = a.OW[j] == 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)a.OW[j] - 1) / (unsigned)a.OW[j]);
        a.mg2_pk[j] = wl_magic((unsigned)(((a.OH[j] + 1) / 2) * Kw[j]));
        a.mg2_pq[j] = wl_magic((unsigned)(a.OH[j] * ((a.OW[j] + 1) / 2)));
        a.mg2_q[j] = wl_magic((unsigned)((a.OW[j] + 1) / 2));
    }
    a.ll_off[0] = off; off += wl_align_up(G * b[0] * 4, 16);
    a.ll_off[1] = off; off += wl_align_up(G * b[1] * 4, 16);
    a.mid_off = off; off += wl_align_up(G * mid0 * 4, 16);
    a.tap_off = off; off += 4 * L * 4;
    a.lds_bytes = off;
    a.nblocks = (planes + G - 1) / G;
    if (mode != 2) switch (L) {                                    // the pair form with compile-time taps
        case 2: return wl_launch<WlSfbSmall<T, 2> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
        case 4: return wl_launch<WlSfbSmall<T, 4> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
        case 6: return wl_launch<WlSfbSmall<T, 6> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
        case 8: return wl_launch<WlSfbSmall<T, 8> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
        default: break;
    }
    return wl_launch<WlSfbSmall<T, 0> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

extern "C" int wl_dwt2d_synthesis_small(const void* yl, int yl_h, int yl_w, const void* const* yh, const int* Kh, const int* Kw,
                                        void* y, int dtype, int64_t planes, int nlev, const void* g_w_lo, const void* g_w_hi,
                                        const void* g_h_lo, const void* g_h_hi, int L, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (planes < 0 || yl_h < 1 || yl_w < 1) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (nlev < 1 || nlev > WL_SMALL_MAXLEV || L > 20 || (L & 1)) return WL_ERR_UNSUPPORTED;
    if (planes == 0) return 0;
    const WlSfbPyrReq r = {yl, (int64_t)yl_h * yl_w, yl_w, yl_h, yl_w, yh, Kh, Kw, y, planes, nlev,
                           {g_w_lo, g_w_hi, g_h_lo, g_h_hi}, L, mode, 0, 0, nullptr, nullptr, stream};
    WL_DISPATCH_FLOAT(dtype, return wl_sfb_small_run<T>(r));
}

// ---- one level of the stationary transform (wl_swt2d.h; reference dwt/lowlevel.py:475-521, :175-223) ----
template <typename T, int LT>
static int wl_swt2d_launch(WlSwtArgs<T>& a, void* stream) {
    return wl_launch<WlSwtLevel<T, LT> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
static int wl_swt2d_run(const void* x, int64_t x_ps, void* y, int64_t planes, int H, int W, const void* h_w_lo, const void* h_w_hi,
                        const void* h_h_lo, const void* h_h_hi, int Lw, int Lh, int dilation, int ext, void* stream) {
    typedef typename WlAcc<T>::type A;
    WlSwtArgs<T> a;
    a.x = (const T*)x; a.y = (T*)y; a.x_ps = x_ps; a.planes = planes;
    a.hw0 = (const A*)h_w_lo; a.hw1 = (const A*)h_w_hi; a.hh0 = (const A*)h_h_lo; a.hh1 = (const A*)h_h_hi;
    a.H = H; a.W = W; a.Lw = Lw; a.Lh = Lh; a.d = dilation; a.ext = ext;
    a.sw = -((Lw * dilation) / 2 - dilation); a.sh = -((Lh * dilation) / 2 - dilation);
    const int hw = (Lw - 1) * dilation;
    const int hh = (Lh - 1) * dilation;
    // the tallest tile whose staged rows fit 64 KiB of LDS (two workgroups per CU)
    a.in_pitch = 64 + hw + 1;
    int TH = 32;
    for (;; TH /= 2) {
        if (TH < 4) return WL_ERR_UNSUPPORTED;                     // long dilated filters: the single-axis kernels
        a.mid_off = wl_align_up((TH + hh) * a.in_pitch * (int)sizeof(A), 16);
        a.lds_bytes = a.mid_off + (TH + hh) * 64 * 2 * (int)sizeof(A);
        if (a.lds_bytes <= 64 * 1024) break;
    }
    a.TH = TH;
    a.tiles_x = wl_cdiv(W, 64); a.tiles_y = wl_cdiv(H, TH);
    a.nblocks = planes * a.tiles_x * a.tiles_y;
    if (Lw == Lh) switch (Lw) {
        case 2: return wl_swt2d_launch<T, 2>(a, stream);
        case 4: return wl_swt2d_launch<T, 4>(a, stream);
        case 6: return wl_swt2d_launch<T, 6>(a, stream);
        case 8: return wl_swt2d_launch<T, 8>(a, stream);
        case 10: return wl_swt2d_launch<T, 10>(a, stream);
        case 12: return wl_swt2d_launch<T, 12>(a, stream);
        case 16: return wl_swt2d_launch<T, 16>(a, stream);
        case 20: return wl_swt2d_launch<T, 20>(a, stream);
        default: break;
    }
    return wl_swt2d_launch<T, 0>(a, stream);
}

extern "C" int wl_swt2d_level(const void* x, int64_t x_ps, void* y, int dtype, int64_t planes, int H, int W,
                              const void* h_w_lo, const void* h_w_hi, const void* h_h_lo, const void* h_h_hi, int Lw, int Lh,
                              int dilation, int ext, void* stream) {
    if (planes < 0 || H < 1 || W < 1 || dilation < 1) return WL_ERR_SHAPE;
    if (Lw < 1 || Lh < 1 || Lw > WL_MAX_TAPS || Lh > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (ext < 0 || ext > WL_EXT_REPLICATE || ext == WL_EXT_PER) return WL_ERR_MODE;   // (the reference's mypad has no 'periodization')
    // the output keeps the input size only for even products L d (every even L): n + 2 ((L d) / 2) - d - d (L - 1) == n
    if ((Lw * dilation) % 2 || (Lh * dilation) % 2) return WL_ERR_UNSUPPORTED;
    if ((int64_t)H * W >= (1LL << 30)) return WL_ERR_UNSUPPORTED;
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, return wl_swt2d_run<T>(x, x_ps, y, planes, H, W, h_w_lo, h_w_hi, h_h_lo, h_h_hi, Lw, Lh, dilation, ext, stream));
    return 0;
}

// ---- the transpose of that level: backward of the stationary transform and one level of its inverse (wl_iswt2d.h) ----
template <typename T, int LT>
static int wl_iswt2d_launch(WlSwtInvArgs<T>& a, void* stream) {
    return wl_launch<WlSwtInvLevel<T, LT> >(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
static int wl_iswt2d_run(const void* y, int64_t y_ps, const void* ll, int64_t ll_ps, int ll_mode, void* x, int64_t planes, int H, int W,
                         const void* h_w_lo, const void* h_w_hi, const void* h_h_lo, const void* h_h_hi, int Lw, int Lh, int dilation,
                         int ext, double scale, void* stream) {
    typedef typename WlAcc<T>::type A;
    WlSwtInvArgs<T> a;
    a.y = (const T*)y; a.ll = (const T*)ll; a.x = (T*)x; a.y_ps = y_ps; a.ll_ps = ll_ps; a.ll_mode = ll_mode; a.planes = planes;
    a.hw0 = (const A*)h_w_lo; a.hw1 = (const A*)h_w_hi; a.hh0 = (const A*)h_h_lo; a.hh1 = (const A*)h_h_hi;
    a.scale = (A)scale;
    a.H = H; a.W = W; a.Lw = Lw; a.Lh = Lh; a.d = dilation; a.ext = ext;
    a.sw = -((Lw * dilation) / 2); a.sh = -((Lh * dilation) / 2);
    const int hw = (Lw - 1) * dilation;
    const int hh = (Lh - 1) * dilation;
    // the tallest tile whose staged pair of bands and row-filtered pairs fit 64 KiB of LDS (two workgroups per CU); what fits
    // no tile of four rows so (the staged pair is twice the forward's input tile) may take a CU's whole 160 KiB: one
    // workgroup per CU is still one pass over the data, where the single-axis kernel needs three
    if (hw > 4096 || hh > 4096) return WL_ERR_UNSUPPORTED;         // (and the byte counts below stay far from 2^31)
    a.in_pitch = 64 + hw + 1;
    int TH = 32, budget = 64 * 1024;
    for (;; TH /= 2) {
        if (TH < 4) {
            if (budget > 64 * 1024) return WL_ERR_UNSUPPORTED;     // long dilated filters: the single-axis kernel
            TH = 32; budget = 160 * 1024;
        }
        a.mid_off = wl_align_up((TH + hh) * a.in_pitch * 2 * (int)sizeof(A), 16);
        a.lds_bytes = a.mid_off + (TH + hh) * 64 * 2 * (int)sizeof(A);
        if (a.lds_bytes <= budget) break;
    }
    a.TH = TH;
    a.tiles_x = wl_cdiv(W, 64); a.tiles_y = wl_cdiv(H, TH);
    a.nblocks = planes * a.tiles_x * a.tiles_y;
    if (Lw == Lh) switch (Lw) {
        case 2: return wl_iswt2d_launch<T, 2>(a, stream);
        case 4: return wl_iswt2d_launch<T, 4>(a, stream);
        case 6: return wl_iswt2d_launch<T, 6>(a, stream);
        case 8: return wl_iswt2d_launch<T, 8>(a, stream);
        case 10: return wl_iswt2d_launch<T, 10>(a, stream);
        case 12: return wl_iswt2d_launch<T, 12>(a, stream);
        case 16: return wl_iswt2d_launch<T, 16>(a, stream);
        case 20: return wl_iswt2d_launch<T, 20>(a, stream);
        default: break;
    }
    return wl_iswt2d_launch<T, 0>(a, stream);
}

extern "C" int wl_iswt2d_level(const void* y, int64_t y_ps, const void* ll, int64_t ll_ps, int ll_mode, void* x, int dtype,
                               int64_t planes, int H, int W, const void* h_w_lo, const void* h_w_hi, const void* h_h_lo,
                               const void* h_h_hi, int Lw, int Lh, int dilation, int ext, double scale, void* stream) {
    if (planes < 0 || H < 1 || W < 1 || dilation < 1) return WL_ERR_SHAPE;
    if (Lw < 1 || Lh < 1 || Lw > WL_MAX_TAPS || Lh > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (ext < 0 || ext > WL_EXT_REPLICATE || ext == WL_EXT_PER) return WL_ERR_MODE;
    if (ll_mode < 0 || ll_mode > 2 || (ll_mode != 0) != (ll != nullptr) || (!y && ll_mode != 1)) return WL_ERR_SHAPE;
    // the mirror and replicate rules fold several extended samples onto one: the single-axis kernel walks them
    if (ext != WL_EXT_ZERO && ext != WL_EXT_PERIODIC) return WL_ERR_UNSUPPORTED;
    if ((Lw * dilation) % 2 || (Lh * dilation) % 2) return WL_ERR_UNSUPPORTED;   // (the level changes size: not square)
    if ((int64_t)H * W >= (1LL << 30)) return WL_ERR_UNSUPPORTED;
    if (planes == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, return wl_iswt2d_run<T>(y, y_ps, ll, ll_ps, ll_mode, x, planes, H, W, h_w_lo, h_w_hi, h_h_lo, h_h_hi, Lw, Lh,
                                                     dilation, ext, scale, stream));
    return 0;
}

extern "C" int wl_corr1d_adj(const void* y0, int64_t y0_outer_stride, const void* y1, int64_t y1_outer_stride, void* dx, int dtype,
                             int64_t outer, int n, int64_t inner, int K, const void* h0, const void* h1, int ntaps, int start,
                             int tap_step, int ext, double scale, void* stream) {
    if (outer < 0 || n < 1 || inner < 1 || K < 0 || ntaps < 1 || ntaps > WL_MAX_TAPS || tap_step < 1 || !y0) return WL_ERR_SHAPE;
    if (y1 && !h1) return WL_ERR_SHAPE;
    if (ext < 0 || ext > WL_EXT_REPLICATE || ext == WL_EXT_PER) return WL_ERR_MODE;
    // the kernel walks extended positions up to 2n + the pad in an int
    if (n >= (1 << 30)) return WL_ERR_UNSUPPORTED;
    if (outer == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        typedef typename WlAcc<T>::type A;
        WlCorr1dAdjArgs<T> a;
        a.y0 = (const T*)y0; a.y1 = (const T*)y1; a.dx = (T*)dx; a.h0 = (const A*)h0; a.h1 = (const A*)h1; a.scale = (A)scale;
        a.outer = outer; a.inner = inner; a.y0_os = y0_outer_stride; a.y1_os = y1_outer_stride;
        a.n = n; a.K = K; a.nt = ntaps; a.start = start; a.dstep = tap_step; a.ext = ext;
        return wl_launch<WlCorr1dAdj<T> >(a, wl_cdiv64(outer * n * inner, 256), 0, stream);
    });
    return 0;
}

extern "C" int wl_synth1d(const void* lo, const void* hi, void* y, int dtype, int64_t outer, int K, int64_t inner,
                          int ny, const void* g0, const void* g1, int L, int mode, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (outer < 0 || K < 1 || inner < 1 || L < 1 || L > WL_MAX_TAPS) return WL_ERR_SHAPE;
    const int full = mode == 2 ? 2 * K : 2 * K - L + 2;
    if (ny < 1 || ny > full) return WL_ERR_SHAPE;
    if (outer == 0) return 0;
    WL_DISPATCH_DTYPE(dtype, {
        typedef typename WlAcc<T>::type A;
        WlSynth1dArgs<T> a;
        a.lo = (const T*)lo; a.hi = (const T*)hi; a.y = (T*)y; a.g0 = (const A*)g0; a.g1 = (const A*)g1;
        a.outer = outer; a.inner = inner; a.K = K; a.ny = ny; a.L = L; a.circ = mode == 2;
        return wl_launch<WlSynth1d<T> >(a, wl_cdiv64(outer * ny * inner, 256), 0, stream);
    });
    return 0;
}

#include "wl_dwt3d_api.inc"
#include "wl_wpt2d_api.inc"
