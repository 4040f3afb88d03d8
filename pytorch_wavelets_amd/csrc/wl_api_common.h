// Host-side helpers shared by the translation units of the C ABI (wl_api.inc, wl_rows_api.inc, wl_strip_api.inc, ...): included
// after the backend header, which provides wl_launch<K>() / wl_launch_aux<K>().
#pragma once
#include <stdlib.h>
#include "../../include/wavelets_hip.h"
#include "wl_common.h"
#include "wl_lattice.h"   // WlTapPrep, wl_tap_examined / wl_tap_mark

// ---- helpers ---------------------------------------------------------------------------------
static int wl_mode_to_ext(int mode) {
    switch (mode) {
        case 0: return WL_EXT_ZERO;
        case 1: return WL_EXT_SYM;
        case 2: return WL_EXT_PER;
        case 4: return WL_EXT_REFL;
        case 6: return WL_EXT_PERIODIC;
        default: return -1;
    }
}

static inline int wl_coeff_len(int n, int L, int mode) { return mode == 2 ? (n + 1) / 2 : (n + L - 1) / 2; }

// base of  y[k] = sum_j h[j] * ext(x, 2k + base + j)   (stored taps h; see wl_dwt_kernels.h)
static int wl_afb_base(int n, int L, int mode) {
    if (mode == 2) return L / 2 - L + 1;
    const int K = (n + L - 1) / 2;
    const int p = 2 * (K - 1) - n + L;
    return -(p / 2);
}

// ---- requests of the 2-D DWT ---------------------------------------------------------------------
// What an extern "C" entry was handed: validated and filled there, once, and passed down by reference - every launcher below an
// entry takes `const Req&` plus what is its own (lat, guard, what).  Strides in elements.
struct WlBanks { const void* w_lo; const void* w_hi; const void* h_lo; const void* h_hi; };   // row lo / hi, column lo / hi
// One level of analysis: x (planes, H, W) -> ll (planes, Kh, Kw) + highs (planes, 3, Kh, Kw).
struct WlAfbReq {
    const void* x; int64_t x_ps; int x_rs;
    void* ll; int64_t ll_ps; int ll_rs; void* highs;
    int64_t planes; int H, W;
    WlBanks taps; int Lw, Lh, mode;
    int policy; float* scratch; int* tstate; void* stream;      // the streaming entries: see wl_dwt2d_analysis_stream_ex
};
// One level of synthesis: ll + highs -> y (planes, OH, OW).
struct WlSfbReq {
    const void* ll; int64_t ll_ps; int ll_rs; const void* highs; void* y;
    int64_t planes; int Kh, Kw, OH, OW;
    WlBanks taps; int Lw, Lh, mode;
    int policy; float* scratch; int* tstate; void* stream;
};
// All levels of an analysis in one launch.  The input planes: (planes, H, W) through a plane stride and a row pitch (elements).  The
// loaders of the fused kernel bring a row in as 16-byte pieces, so rows start on 16-byte addresses (pitch and plane stride whole
// pieces); a row whose WIDTH is no whole number of pieces (the odd-width LL of a strip-kernel level: 515 columns below a 1024-wide
// image) ends inside its last piece - the cells behind it land in the ring's right halo cells and are overwritten there (mirrored
// samples, or zeros in zero mode) before any lane reads them.  The caller owns pitch - W readable elements behind every row
// (ops.afb2d_stream pads its ll for that).
struct WlAfbPyrReq {
    const void* x; int64_t x_ps; int x_rs;
    void* yl; void* const* yh;
    int64_t planes; int H, W, nlev;
    WlBanks taps; int L, mode;
    int strips, hints; float* scratch; int* tstate; void* stream;
};
// All levels of a synthesis in one launch: yl (yl_h x yl_w) and yh[j] (3 x Kh[j] x Kw[j]), finest level first -> y.
struct WlSfbPyrReq {
    const void* yl; int64_t yl_ps; int yl_rs; int yl_h, yl_w;
    const void* const* yh; const int* Kh; const int* Kw; void* y;
    int64_t planes; int nlev;
    WlBanks taps; int L, mode;
    int strips, hints; float* scratch; int* tstate; void* stream;
};

// ---- dtype dispatch --------------------------------------------------------------------------------
// A statement with T = the element type of `dtype`: every dtype of the ABI ...
#define WL_DISPATCH_DTYPE(dtype, ...)                      \
    switch (dtype) {                                       \
        case WL_F32: { typedef float T; __VA_ARGS__; } break;    \
        case WL_F16: { typedef wl_half T; __VA_ARGS__; } break;  \
        case WL_BF16: { typedef wl_bf16 T; __VA_ARGS__; } break; \
        case WL_F64: { typedef double T; __VA_ARGS__; } break;   \
        default: return WL_ERR_DTYPE;                      \
    }
// ... or, for the kernels without a float64 form, a statement that returns: float64 is valid but not this kernel's
// (WL_ERR_UNSUPPORTED), anything else is no dtype
#define WL_DISPATCH_FLOAT(dtype, ...)                                      \
    do {                                                                   \
        if ((dtype) == WL_F32) { typedef float T; __VA_ARGS__; }           \
        if ((dtype) == WL_F16) { typedef wl_half T; __VA_ARGS__; }         \
        if ((dtype) == WL_BF16) { typedef wl_bf16 T; __VA_ARGS__; }        \
        return (dtype) == WL_F64 ? WL_ERR_UNSUPPORTED : WL_ERR_DTYPE;      \
    } while (0)

// ---- hinted launches ---------------------------------------------------------------------------------
// A launch of the variant HINT that relies on a relation between the filter banks, guarded on the device (wl_common.h), with
// the plain variant PLAIN queued behind it as its armed fallback: exactly one of the two does the work.  The fallback's own
// checks run first (dry), so that it cannot decline behind a hinted variant that is already on the stream.
#define WL_GUARDED_PAIR(HINT, PLAIN, ...)                         \
    do {                                                          \
        int rc_ = PLAIN(__VA_ARGS__, 2, 1);                       \
        if (rc_ != 0) return rc_;                                 \
        rc_ = HINT(__VA_ARGS__, 1, 0);                            \
        if (rc_ != 0) return rc_;                                 \
        return PLAIN(__VA_ARGS__, 2, 2);                          \
    } while (0)

// The lattice variant of a kernel (wl_lattice.h): WlTapPrep leaves its verdict on the banks + the column lattice in the caller's
// device scratch, the lattice kernel runs if the verdict is good, the two-bank kernel behind it if not.  `plain` and `lattice`
// are the two launchers as (guard, what) -> rc.  `same`: the kernels hold ONE bank for both axes (the fused multi-level kernels).
// *tstate: the scratch already holds the verdict on exactly these banks - an earlier level of the same transform, which THIS
// library examined (bit 0; bit 1: WITH the same-banks check): the launcher that runs WlTapPrep sets the bits, nobody else.
// `bits` is what this caller needs examined and what it marks: 1 for the strip kernels (same = 0), 3 for the fused ones (same = 1).
template <int LT, typename Plain, typename Lattice>
static int wl_lattice_launch(Plain plain, Lattice lattice, const WlBanks& b, int syn, int same, size_t elem_size,
                             float* scratch, int* tstate, int bits, void* stream) {
    int rc = plain(2, 1);                               // the fallback's own checks first (it must not decline later)
    if (rc != 0) return rc;
    rc = lattice(1, 1);
    if (rc != 0) return rc;
    WlTapPrepArgs p;
    p.h_w_lo = (const float*)b.w_lo; p.h_w_hi = (const float*)b.w_hi; p.h_h_lo = (const float*)b.h_lo; p.h_h_hi = (const float*)b.h_hi;
    p.out = scratch; p.L = LT; p.syn = syn; p.same = same;
    p.tol = elem_size == 2 ? 0x1p-12f : 0x1p-22f;       // a quarter unit in the last place of float16 storage / float32: wl_lattice.h
    rc = wl_tap_examined(tstate, bits) ? 0 : wl_launch_aux<WlTapPrep<LT> >(p, 1, 0, stream);
    if (rc != 0) return rc;
    wl_tap_mark(tstate, bits);
    rc = lattice(1, 0);
    if (rc != 0) return rc;
    return plain(2, 2);
}
