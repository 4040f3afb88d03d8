// C ABI of the one-level streaming analysis over column strips (wl_dwt_strip.h).  Its own translation unit in the HIP
// build (wl_strip_hip.hip, -fno-slp-vectorize like the other streaming kernels); included after the backend header.
#include "wl_api_common.h"
#include "wl_dt_api.h"      // wl_streaming_off, the launchers of part 4 that wl_api.inc calls
#include "wl_dwt_strip.h"

// planes of WL_FOUR_MIN .. 128 columns go four to a workgroup of the lean DTCWT / ScatLayer kernels (forward and inverse)
#ifndef WL_FOUR_MIN
#define WL_FOUR_MIN 64
#endif

// Row segments of a strip kernel: `rows` output rows per (plane, strip), `units` = planes x strips, `wgs_per_cu` resident
// workgroups per CU, every segment re-processes `halo` rows.  A launch runs in whole rounds of the chip's workgroup slots,
// so the time is about rounds x (rows per segment + halo): the number of segments (each of at least 64 rows, a multiple of
// `align`) that minimises it, preferring fewer segments on a tie.
// (min_rows = 32 with `partial` rounds, the lean DTCWT kernels: with few planes - ScatLayerj2 on 64 images - segments of 32 rows
// fill the chip where 64-row segments left it half empty, 0.042 -> 0.037 ms and 0.057 -> 0.052 ms for its two ScatLayer
// launches; the workgroups of a partly filled last round run faster, so rounds count fractionally above one.)
// Planes per workgroup of a one-level DWT strip kernel (K::run): `nact` = compute waves one plane's strip keeps busy, `rows` = the
// rows row segments are cut from, `ngl_max` >= 4-cell groups per stager lane and row (the stager holds pp x that many in registers:
// <= lim2 with two planes, <= lim4 with four - the instantiations the kernel has).  More than one only when the strip is the whole row, the
// workgroup has its four compute and four stager waves and the chip still gets a workgroup for every slot.
#ifndef WL_STRIP_MINSEG
#define WL_STRIP_MINSEG 32      // shortest row segment of the one-level DWT strip kernels.  A workgroup's cadence is one half-batch per
#endif                          // ~3000 cycles whatever else the chip does: a small level (config 5's fourth: 512 planes of 256 x 256) is
                                // over soonest with MANY short workgroups - four planes each, four segments of 32 rows - not few long ones
static int wl_strip_planes_per_wg(int nact, int nstrips, int64_t planes, int rows, int ngl_max, int st_off, int ring, int lim2, int lim4) {
    if (WL_STRIP_CWAVES != 4 || WL_STRIP_SWAVES != 4 || nstrips != 1) return 1;
    int pp = nact == 1 ? 4 : nact == 2 ? 2 : 1;
    int maxseg = rows / WL_STRIP_MINSEG;
    maxseg = maxseg < 1 ? 1 : maxseg;
    while (pp > 1 && ((planes + pp - 1) / pp * maxseg < 2 * (int64_t)wl_num_cus() || st_off + pp * ring > 80 * 1024 || ngl_max > (pp == 2 ? lim2 : lim4))) pp >>= 1;
    return pp;
}

#ifndef WL_STRIP_WGS
#define WL_STRIP_WGS 2     // workgroups per CU the one-level DWT strip kernels are cut for
#endif
static void wl_pick_segments(int rows, int64_t units, int wgs_per_cu, int halo, int align, int* seg_rows, int* nseg,
                             int min_rows = 64, bool partial = false) {
    const int64_t slots = (int64_t)wgs_per_cu * wl_num_cus();
    int maxseg = rows / min_rows;
    if (maxseg < 1) maxseg = 1;
    if (maxseg > 64) maxseg = 64;
    int64_t best = -1;
    for (int n = 1; n <= maxseg; ++n) {
        const int sr = wl_align_up(wl_cdiv(rows, n), align);
        const int ns = wl_cdiv(rows, sr);
        const int64_t rounds = wl_cdiv64(units * ns, slots);
        int64_t cost = rounds * (sr + halo + 8);         // (+8: pipeline fill and LDS clearing of a workgroup)
        if (partial) cost = (units * ns > slots ? units * ns : slots) * (sr + halo + 8);   // (the same scale: x slots)
        if (best < 0 || cost < best) { best = cost; *seg_rows = sr; *nseg = ns; }
    }
}

// Round 6: THREE translation units (WL_STRIP_PARTS: bit 0 = the analysis strip kernels, wl_strip_hip.hip; bit 1 = the synthesis strip kernels,
// wl_istrip_hip.hip; bit 2 = the streaming DTCWT / ScatLayer kernels, wl_dtstrip_hip.hip - together they were the build's longest unit by far;
// without the macro the file is whole).
#ifndef WL_STRIP_PARTS
#define WL_STRIP_PARTS 7
#endif
#if WL_STRIP_PARTS & 1
// Strip width, row segments and the LDS layout; declines (WL_ERR_UNSUPPORTED) what the kernel does not cover.
// policy: 0 = the engine decides whether the launch pays, 1 = force.
template <typename T, int LT, int QMF = 0, int LAT = 0>
static int wl_afb_strip_launch(const WlAfbReq& r, const float* lat, int guard = 0, int what = 0) {
    // what: 0 = launch, 1 = dry run (every check, no launch), 2 = launch as the armed fallback of a hinted launch
    // lat: device scratch with WlTapPrep's verdict (+ the column lattice for LAT = 1), or null (the guard reads the taps)
    typedef WlAfbStrip<T, LT, QMF, LAT> K;
    const int SZ = (int)sizeof(T), A = K::A;
    const int64_t planes = r.planes, x_ps = r.x_ps, ll_ps = r.ll_ps;
    const int H = r.H, W = r.W, x_rs = r.x_rs, ll_rs = r.ll_rs;
    WlStripArgs<T> a;
    a.ext = wl_mode_to_ext(r.mode);
    a.H = H; a.W = W;
    a.Kh = wl_coeff_len(H, LT, r.mode); a.Kw = wl_coeff_len(W, LT, r.mode);
    a.base = wl_afb_base(W, LT, r.mode);
    // the stagers load 4-cell groups at element alignment: any row width and pitch; wrapped groups (periodic /
    // periodization) must be whole groups.
    if (K::wraps(a.ext) && W % 4) return WL_ERR_UNSUPPORTED;
    if ((uintptr_t)r.x % SZ) return WL_ERR_UNSUPPORTED;
    if ((int64_t)H * x_rs >= (1LL << 29) || (int64_t)a.Kh * a.Kw >= (1LL << 29) || (int64_t)a.Kh * ll_rs >= (1LL << 29)) return WL_ERR_UNSUPPORTED;
    if (W < 2 * LT || H < 2) return WL_ERR_UNSUPPORTED;       // a mirrored / wrapped halo must come from inside the row, once
    if (a.ext == WL_EXT_SYM || a.ext == WL_EXT_REFL || a.ext == WL_EXT_PERIODIC) {
        // rows above / below the plane are fetched through the extension rule: any number of folds is fine
    }
    // the widest strip the LDS takes at two workgroups per CU: 128 output columns per compute wave
    int ncw = WL_STRIP_CWAVES, ng_worst = 0;
    for (;; --ncw) {
        if (ncw < 1) return WL_ERR_UNSUPPORTED;
        const int smax = 128 * ncw;
        a.nstrips = wl_cdiv(a.Kw, smax);
        a.strip_cols = (wl_cdiv(a.Kw, a.nstrips) + 1) & ~1;
        a.nstrips = wl_cdiv(a.Kw, a.strip_cols);
        const int np = (2 * a.strip_cols + LT + 1 + 2 * A) / A + 1;              // pieces per row, worst alignment
        const int ng = np * A / 4;
        ng_worst = ng;
        a.dma_pitch = wl_align_up(np * 16, 16);                   // (host only: the bytes of a row as 16-byte pieces, bounded below)
        a.st_pitch = wl_align_up((4 * ng + 8 + 4 * K::NV4) * 4, 16);
        a.dma_off = 0;
        a.st_off = 0;                                              // (the staged ring is all of the LDS)
        a.lds_bytes = a.st_off + 2 * 4 * a.st_pitch;
        if (wl_cdiv(np, 64) <= WL_STRIP_MAXPPR && a.lds_bytes <= 80 * 1024 && wl_cdiv(ng, 64) <= K::MAXG) break;
    }
    // a narrow level (one strip that needs two / one of the four compute waves): two / four planes per workgroup (K::run) when
    // that still leaves workgroups for every slot of the chip
    a.ring = 2 * 4 * a.st_pitch;
    a.pp = wl_strip_planes_per_wg(wl_cdiv(wl_cdiv(a.Kw, 2), 64), a.nstrips, planes, a.Kh, wl_cdiv(ng_worst, 64), a.st_off, a.ring, 3, 2);
    a.lds_bytes = a.st_off + a.pp * a.ring;
    // row segments (two workgroups of 8 waves per CU)
    wl_pick_segments(a.Kh, wl_cdiv64(planes, a.pp) * a.nstrips, WL_STRIP_WGS, K::WARM, 1, &a.seg_rows, &a.nseg, WL_STRIP_MINSEG);
    // every strip must find its mirrored halo inside the columns it loads; the limits on np / ppr / dma_pitch and the "no run of 64
    // pieces that lies outside the row" loop below are limits of the accepted geometry inherited from the layout of the retired DMA
    // ring (rows of at most WL_STRIP_MAXPPR KiB as 16-byte pieces): they decide which shapes this kernel takes
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        if (s.np < 1 || s.ppr > WL_STRIP_MAXPPR || s.np * 16 > a.dma_pitch) return WL_ERR_UNSUPPORTED;
        if ((K::staged_of(s, 0) + 4 * s.ng) * 4 > a.st_pitch) return WL_ERR_UNSUPPORTED;
        const int npairs = wl_cdiv(s.k1 - s.k0, 2);
        if (s.lane_off + 16 * (npairs - 1) + 16 * K::NV4 > a.st_pitch) return WL_ERR_UNSUPPORTED;
        if (a.ext == WL_EXT_SYM || a.ext == WL_EXT_REFL) {
            const int e_hi = 2 * (s.k1 - 1) + a.base + LT - 1 + 2;
            const int last = e_hi > W - 1 ? W - 1 : e_hi;
            for (int e = s.e_lo; e <= e_hi; ++e) {
                if ((unsigned)e < (unsigned)W) { e = W - 1; continue; }          // (skip the interior)
                const int src = wl_ext(e, W, a.ext);
                if (src < s.c0a || src > last || src < 0) return WL_ERR_UNSUPPORTED;
            }
            const int nl = s.e_lo < 0 ? -s.e_lo : 0, nr = e_hi > W - 1 ? e_hi - (W - 1) : 0;
            if (K::LROWS * (nl + nr) > 128) return WL_ERR_UNSUPPORTED;
        }
        // every run of 64 pieces of a row must hold a piece that is loaded (inherited from the ring layout, where such a run was one
        // DMA instruction): pieces 0, 64, 128, .. lie left of the row only in the first run
        for (int q = 0; q < s.ppr; ++q) {
            bool any = false;
            for (int l = 0; l < 64 && !any; ++l) {
                const int p = q * 64 + l;
                if (p >= s.np) break;
                const int col = s.c0a + p * A;
                any = K::wraps(a.ext) || (unsigned)col < (unsigned)W;
            }
            if (!any) return WL_ERR_UNSUPPORTED;
        }
    }
    if (a.pp > 1 && wl_cdiv(K::geometry(a, 0, 0).ng, 64) > (a.pp == 2 ? 3 : 2)) return WL_ERR_UNSUPPORTED;   // (wl_strip_planes_per_wg's bound on the stager's groups)
    const int64_t nblocks = wl_cdiv64(planes, a.pp) * a.nstrips * a.nseg;
    // the engine's own policy (measured against the per-level tile kernels, tools/gpu_strip_probe.py): the strip kernel
    // pays from rows of 2 KiB up (512 float32 / 1024 float16 columns: three or four compute waves per strip) when there are
    // workgroups for every CU; narrower levels of a pyramid stay on the tile kernels
#ifndef WL_STRIP_MINW
#define WL_STRIP_MINW 256        // the narrowest float16 level (columns) the strip kernel takes (0: 2 KiB rows as for float32); config 5 on
                                 // levels of 512 and 256 columns: 2.840 -> 2.800 ms (tools/gpu_cfg5_minw_ab.sh); the synthesis at 256: no gain
#endif
    // Round 5: narrower levels too (from 128 columns) when the launch packs planes so that all four compute waves of a workgroup
    // work (tools/gpu_r5p_policy.py, periodization, J = 1, against the tile kernels: float16 128 columns 0.19-0.27 -> 0.16-0.23 ms,
    // float32 256 columns 0.24-0.34 -> 0.19-0.21 ms)
    const bool wide = WL_STRIP_MINW && SZ == 2 ? W >= WL_STRIP_MINW : W * SZ >= 2048;
    // (rows of 1 KiB with half the compute waves busy: 384 planes of 256 x 256 float32 0.048 -> 0.036 ms, tools/gpu_r5p_small.py;
    // at 128 columns and few planes the tile kernels stay ahead, 0.016 against 0.027 ms)
    const int busy = a.pp * wl_cdiv(wl_cdiv(a.Kw, 2), 64);
    const bool packed = (busy >= WL_STRIP_CWAVES && W >= 128) || (2 * busy >= WL_STRIP_CWAVES && W * SZ >= 1024);
    if (!(r.policy & 1) && (nblocks < wl_num_cus() || !(wide || packed))) return WL_ERR_UNSUPPORTED;
    a.x = (const T*)r.x; a.ll = (T*)r.ll; a.highs = (T*)r.highs;
    a.h_w_lo = (const float*)r.taps.w_lo; a.h_w_hi = (const float*)r.taps.w_hi; a.h_h_lo = (const float*)r.taps.h_lo; a.h_h_hi = (const float*)r.taps.h_hi;
    a.NC = planes; a.x_ps = x_ps; a.ll_ps = ll_ps; a.x_rs = x_rs; a.ll_rs = ll_rs;
    a.nblocks = nblocks;
    a.pair_ok = a.Kw % 2 == 0 && ll_rs % 2 == 0 && ll_ps % 2 == 0 && (uintptr_t)r.ll % (2 * SZ) == 0 && (uintptr_t)r.highs % (2 * SZ) == 0;
    a.guard = guard;
    a.lat = lat;
    if (what == 1) return 0;
    return what == 2 ? wl_launch_armed<K>(a, nblocks, (size_t)a.lds_bytes, r.stream) : wl_launch<K>(a, nblocks, (size_t)a.lds_bytes, r.stream);
}

// The lattice variant (wl_lattice_launch): the lattice kernel behind WlTapPrep, the two-bank kernel armed behind it.
template <typename T, int LT>
static int wl_afb_strip_lattice(const WlAfbReq& r) {
    return wl_lattice_launch<LT>([&](int guard, int what) { return wl_afb_strip_launch<T, LT, 0, 0>(r, r.scratch, guard, what); },
                                 [&](int guard, int what) { return wl_afb_strip_launch<T, LT, 1, 1>(r, r.scratch, guard, what); },
                                 r.taps, 0, 0, sizeof(T), r.scratch, r.tstate, 1, r.stream);
}

template <typename T>
static int wl_afb_strip_dispatch(const WlAfbReq& r) {   // (Lw == Lh)
    const float* const none = nullptr;
#define WL_CASE(LT_) case LT_: return wl_afb_strip_launch<T, LT_>(r, none)
    // policy bit 1 (value 2): the caller vouches for quadrature-mirror highpass banks; from 12 taps on the kernel then derives
    // the (lo, hi) tap pairs from the lowpass bank alone (below that the scalar file holds both banks)
    // (a hint, not a promise: the variant verifies the relation on the device and the two-bank variant stands by behind it)
    // With device scratch from the caller the hinted variant is the LATTICE kernel (WL_STRIP_LAT_MIN taps and more; not 18: the
    // compiler does not unroll the nine half-batches after which nine delay slots are back in place, and with run-time slots
    // the state leaves the registers - the QMF variant stays there).
#ifndef WL_STRIP_LAT_MIN
#define WL_STRIP_LAT_MIN 12
#endif
#define WL_CASEQ(LT_) case LT_: if (!(r.policy & 2)) return wl_afb_strip_launch<T, LT_>(r, none); \
                                 if constexpr (LT_ >= WL_STRIP_LAT_MIN && LT_ != 18) { if (r.scratch) return wl_afb_strip_lattice<T, LT_>(r); } \
                                 WL_GUARDED_PAIR((wl_afb_strip_launch<T, LT_, 1>), (wl_afb_strip_launch<T, LT_, 0>), r, none)
    switch (r.Lw) {
        WL_CASE(2); WL_CASE(4); WL_CASE(6); WL_CASE(8); WL_CASE(10); WL_CASEQ(12); WL_CASEQ(14); WL_CASEQ(16); WL_CASEQ(18); WL_CASEQ(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASEQ
#undef WL_CASE
}

extern "C" int wl_dwt2d_analysis_stream_ex(const void* x, int64_t x_plane_stride, int x_row_stride, void* ll,
                                           int64_t ll_plane_stride, int ll_row_stride, void* highs, int dtype,
                                           int64_t planes, int H, int W, const void* h_w_lo, const void* h_w_hi,
                                           const void* h_h_lo, const void* h_h_hi, int L, int mode, int policy, void* tap_scratch,
                                           int* tap_state, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (x_row_stride < W || ll_row_stride < wl_coeff_len(W, L, mode) || x_plane_stride < 0 || ll_plane_stride < 0) return WL_ERR_SHAPE;
    if (policy < 0 || policy > 3) return WL_ERR_UNSUPPORTED;
    if (!tap_scratch) tap_state = nullptr;               // (no scratch: nothing to remember)
    if (wl_streaming_off()) return WL_ERR_UNSUPPORTED;   // generic_only / no_stream: the callers fall back to the tile / generic kernels
    if (mode == 2 && (H + (H & 1) < L - 1 || W + (W & 1) < L - 1)) return WL_ERR_UNSUPPORTED;   // single-fold corner: direct kernels
    if (planes == 0) return 0;
    const WlAfbReq r = {x, x_plane_stride, x_row_stride, ll, ll_plane_stride, ll_row_stride, highs, planes, H, W,
                        {h_w_lo, h_w_hi, h_h_lo, h_h_hi}, L, L, mode, policy, (float*)tap_scratch, tap_state, stream};
    WL_DISPATCH_FLOAT(dtype, return wl_afb_strip_dispatch<T>(r));
}

// (the entry point of library versions up to 1.x: no device scratch, so the hinted variant of 12 taps and more is the QMF kernel)
extern "C" int wl_dwt2d_analysis_stream(const void* x, int64_t x_plane_stride, int x_row_stride, void* ll,
                                        int64_t ll_plane_stride, int ll_row_stride, void* highs, int dtype,
                                        int64_t planes, int H, int W, const void* h_w_lo, const void* h_w_hi,
                                        const void* h_h_lo, const void* h_h_hi, int L, int mode, int policy, void* stream) {
    return wl_dwt2d_analysis_stream_ex(x, x_plane_stride, x_row_stride, ll, ll_plane_stride, ll_row_stride, highs, dtype, planes, H, W,
                                       h_w_lo, h_w_hi, h_h_lo, h_h_hi, L, mode, policy, nullptr, nullptr, stream);
}

#endif   // WL_STRIP_PARTS & 1

#if WL_STRIP_PARTS & 2
// ---- one-level streaming synthesis over column strips (wl_idwt_strip.h) ---------------------------------------------
#include "wl_idwt_strip.h"

template <typename T, int LT, int SODD, int QMF = 0, int LAT = 0>
static int wl_sfb_strip_launch(const WlSfbReq& r, const float* lat, int guard = 0, int what = 0) {
    typedef WlSfbStrip<T, LT, SODD, QMF, LAT> K;
    const int SZ = (int)sizeof(T), A = K::A, HL = LT / 2;
    const int64_t planes = r.planes, ll_ps = r.ll_ps;
    const int ll_rs = r.ll_rs, Kh = r.Kh, Kw = r.Kw, OH = r.OH, OW = r.OW;
    WlIStripArgs<T> a;
    a.per = r.mode == 2;
    a.Kh = Kh; a.Kw = Kw; a.OH = OH; a.OW = OW;
    a.sw = a.per ? HL - 1 : LT - 2;
    a.sh = a.sw;
    if ((a.sw & 1) != SODD) return WL_ERR_UNSUPPORTED;
    // the stagers load 4-cell groups at element alignment: any row width and pitch; wrapped groups (periodization) must be
    // whole groups.
    if (a.per && Kw % 4) return WL_ERR_UNSUPPORTED;
    if ((uintptr_t)r.ll % SZ || (uintptr_t)r.highs % SZ) return WL_ERR_UNSUPPORTED;
    if ((int64_t)Kh * Kw >= (1LL << 28) || (int64_t)OH * OW >= (1LL << 29) || (int64_t)Kh * ll_rs >= (1LL << 29)) return WL_ERR_UNSUPPORTED;
    if (Kw < LT || Kh < HL) return WL_ERR_UNSUPPORTED;
    // z-row pairs that hold output rows: all of them under periodization, from L/2-1 on otherwise; the crop drops the rest
    a.m_first = a.per ? 0 : HL - 1;
    a.m_end = Kh;
    if (!a.per) { const int need = (OH + a.sh + 1) / 2; if (need < a.m_end) a.m_end = need; }
    if (a.m_end <= a.m_first) return WL_ERR_UNSUPPORTED;
    const int units = (OW + 3) / 4;
    int cap = 64 * WL_STRIP_CWAVES, ng_worst = 0;
    for (;; cap -= 64) {
        if (cap < 64) return WL_ERR_UNSUPPORTED;
        a.nstrips = wl_cdiv(units, cap);
        a.strip_units = wl_cdiv(units, a.nstrips);
        a.nstrips = wl_cdiv(units, a.strip_units);
        const int np = (2 * a.strip_units + K::NT + 1 + 2 * A) / A + 1;
        const int ng = np * A / 4;
        ng_worst = ng;
        a.dma_pitch = np * 16;                                     // (host only: the bytes of a row as 16-byte pieces, bounded below)
        a.st_pitch = wl_align_up((4 * ng + 2 + A + 2 * K::NC2) * 4, 16);
        a.dma_off = 0;
        a.st_off = 0;                                              // (the staged ring is all of the LDS)
        a.lds_bytes = a.st_off + 2 * 8 * a.st_pitch;
        if (wl_cdiv(np, 64) <= WL_STRIP_MAXPPR && a.lds_bytes <= 80 * 1024 && wl_cdiv(ng, 64) <= K::MAXG) break;
    }
    // a narrow level: two / four planes per workgroup (WlAfbStrip::run) when that still leaves workgroups for every slot of the chip
    a.ring = 2 * 8 * a.st_pitch;
    a.pp = wl_strip_planes_per_wg(wl_cdiv(units, 64), a.nstrips, planes, a.m_end - a.m_first, wl_cdiv(ng_worst, 64), a.st_off, a.ring, 2, 1);
    a.lds_bytes = a.st_off + a.pp * a.ring;
    wl_pick_segments(a.m_end - a.m_first, wl_cdiv64(planes, a.pp) * a.nstrips, WL_STRIP_WGS, HL - 1, 1, &a.seg_pairs, &a.nseg, WL_STRIP_MINSEG);
    // (np / ppr / dma_pitch and the loop over runs of 64 pieces: limits of the accepted geometry inherited from the layout of the retired
    // DMA ring, as in wl_afb_strip_launch)
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        if (s.np < 1 || s.ppr > WL_STRIP_MAXPPR || s.np * 16 > a.dma_pitch) return WL_ERR_UNSUPPORTED;
        if ((4 * s.ng + s.dm) * 4 > a.st_pitch) return WL_ERR_UNSUPPORTED;
        if (s.lane_off + 8 * (s.u1 - s.u0 - 1) + 8 * K::NC2 > a.st_pitch) return WL_ERR_UNSUPPORTED;
        if (!a.per && s.q_lo < 0) return WL_ERR_UNSUPPORTED;
        for (int q = 0; q < s.ppr; ++q) {     // no run of 64 pieces that lies outside the row
            bool any = false;
            for (int l = 0; l < 64 && !any; ++l) {
                const int p = q * 64 + l;
                if (p >= s.np) break;
                any = a.per || (unsigned)(s.c0a + p * A) < (unsigned)Kw;
            }
            if (!any) return WL_ERR_UNSUPPORTED;
        }
    }
    if (a.pp > 1 && wl_cdiv(K::geometry(a, 0, 0).ng, 64) > (a.pp == 2 ? 2 : 1)) return WL_ERR_UNSUPPORTED;   // (wl_strip_planes_per_wg's bound on the stager's groups)
    const int64_t nblocks = wl_cdiv64(planes, a.pp) * a.nstrips * a.nseg;
    // the engine's own policy (tools/gpu_istrip_probe.py against the tile kernels): output rows of 1 KiB and more that leave
    // as aligned 4-column stores, workgroups for every CU
#ifndef WL_ISTRIP_MINW
#define WL_ISTRIP_MINW 0
#endif
    // Round 5: narrower levels too (from 128 columns) when the launch packs planes so that all four compute waves work (float16
    // 256 columns, periodization, against the tile kernel: 0.23-0.30 -> 0.14-0.16 ms; tools/gpu_r5p_policy.py)
    const bool wide = WL_ISTRIP_MINW && SZ == 2 ? OW >= WL_ISTRIP_MINW : OW * SZ >= 1024;
    const bool packed = a.pp * wl_cdiv(units, 64) >= WL_STRIP_CWAVES && OW >= 128;
    if (!(r.policy & 1) && (nblocks < wl_num_cus() || !(wide || packed) || OW % 4 || (uintptr_t)r.y % (4 * SZ))) return WL_ERR_UNSUPPORTED;
    a.ll = (const T*)r.ll; a.highs = (const T*)r.highs; a.y = (T*)r.y;
    a.g_w_lo = (const float*)r.taps.w_lo; a.g_w_hi = (const float*)r.taps.w_hi; a.g_h_lo = (const float*)r.taps.h_lo; a.g_h_hi = (const float*)r.taps.h_hi;
    a.NC = planes; a.ll_ps = ll_ps; a.ll_rs = ll_rs; a.nblocks = nblocks;
    a.quad_ok = OW % 4 == 0 && (uintptr_t)r.y % (4 * SZ) == 0;
    a.guard = guard;
    a.lat = lat;
    if (what == 1) return 0;
    return what == 2 ? wl_launch_armed<K>(a, nblocks, (size_t)a.lds_bytes, r.stream) : wl_launch<K>(a, nblocks, (size_t)a.lds_bytes, r.stream);
}

// The lattice variant (wl_lattice_launch): the lattice kernel behind WlTapPrep, the two-bank kernel armed behind it.
template <typename T, int LT, int SODD>
static int wl_sfb_strip_lattice(const WlSfbReq& r) {
    return wl_lattice_launch<LT>([&](int guard, int what) { return wl_sfb_strip_launch<T, LT, SODD, 0, 0>(r, r.scratch, guard, what); },
                                 [&](int guard, int what) { return wl_sfb_strip_launch<T, LT, SODD, 1, 1>(r, r.scratch, guard, what); },
                                 r.taps, 1, 0, sizeof(T), r.scratch, r.tstate, 1, r.stream);
}

template <typename T>
static int wl_sfb_strip_dispatch(const WlSfbReq& r) {   // (Lw == Lh)
    const int sodd = (r.mode == 2 ? r.Lw / 2 - 1 : r.Lw - 2) & 1;
    const float* const none = nullptr;
    // policy bit 1 (value 2): the caller vouches for quadrature-mirror highpass banks; from 12 taps on the kernel then derives
    // the highpass tap pairs from the lowpass ones (below that the scalar file holds both).  NOT at 14 taps: that instantiation
    // needs 19 more vector registers than four waves per SIMD leave it and spills them - measured 0.434 against 0.332 ms
    // (float32) and 1.85 against 1.04 ms (float16) for the two-bank kernel with its 13 spilled scalars (tools/gpu_qmf_probe.py)
    const bool qmf = (r.policy & 2) != 0;
#define WL_CASE0(LT_) case LT_: return sodd ? WL_ERR_UNSUPPORTED : wl_sfb_strip_launch<T, LT_, 0>(r, none)
#define WL_CASE2(LT_) case LT_: return sodd ? wl_sfb_strip_launch<T, LT_, 1>(r, none) : wl_sfb_strip_launch<T, LT_, 0>(r, none)
    // (a hint, not a promise: the QMF variant verifies the relation on the device, the two-bank variant stands by behind it)
    // With device scratch from the caller the hinted variant is the LATTICE kernel (wl_lattice.h), also at 14 taps where the
    // QMF variant alone does not pay.
#define WL_CASE0Q(LT_) case LT_: if (sodd) return WL_ERR_UNSUPPORTED;                                  \
                                  if (!qmf) return wl_sfb_strip_launch<T, LT_, 0>(r, none);             \
                                  if constexpr (LT_ != 18) { if (r.scratch) return wl_sfb_strip_lattice<T, LT_, 0>(r); }   /* (18: see the analysis) */ \
                                  WL_GUARDED_PAIR((wl_sfb_strip_launch<T, LT_, 0, 1>), (wl_sfb_strip_launch<T, LT_, 0, 0>), r, none)
#define WL_CASE0L(LT_) case LT_: if (sodd) return WL_ERR_UNSUPPORTED;                                  \
                                  if (qmf && r.scratch) return wl_sfb_strip_lattice<T, LT_, 0>(r); \
                                  return wl_sfb_strip_launch<T, LT_, 0>(r, none)
#define WL_CASE2Q(LT_) case LT_: if (!qmf) return sodd ? wl_sfb_strip_launch<T, LT_, 1>(r, none) : wl_sfb_strip_launch<T, LT_, 0>(r, none); \
                                  if (r.scratch) return sodd ? wl_sfb_strip_lattice<T, LT_, 1>(r) : wl_sfb_strip_lattice<T, LT_, 0>(r); \
                                  if (sodd) WL_GUARDED_PAIR((wl_sfb_strip_launch<T, LT_, 1, 1>), (wl_sfb_strip_launch<T, LT_, 1, 0>), r, none); \
                                  WL_GUARDED_PAIR((wl_sfb_strip_launch<T, LT_, 0, 1>), (wl_sfb_strip_launch<T, LT_, 0, 0>), r, none)
    switch (r.Lw) {   // an odd roll (SODD) only exists for periodization with L % 4 == 0
        WL_CASE0(2); WL_CASE2(4); WL_CASE0(6); WL_CASE2(8); WL_CASE0(10); WL_CASE2Q(12); WL_CASE0L(14); WL_CASE2Q(16); WL_CASE0Q(18); WL_CASE2Q(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASE0Q
#undef WL_CASE0L
#undef WL_CASE2Q
#undef WL_CASE0
#undef WL_CASE2
}

extern "C" int wl_dwt2d_synthesis_stream_ex(const void* ll, int64_t ll_plane_stride, int ll_row_stride, const void* highs,
                                            void* y, int dtype, int64_t planes, int Kh, int Kw, int OH, int OW,
                                            const void* g_w_lo, const void* g_w_hi, const void* g_h_lo, const void* g_h_hi,
                                            int L, int mode, int policy, void* tap_scratch, int* tap_state, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    const int fullH = mode == 2 ? 2 * Kh : 2 * Kh - L + 2, fullW = mode == 2 ? 2 * Kw : 2 * Kw - L + 2;
    if (planes < 0 || Kh < 1 || Kw < 1 || OH < 1 || OW < 1 || OH > fullH || OW > fullW) return WL_ERR_SHAPE;
    if (policy < 0 || policy > 3 || !highs) return WL_ERR_UNSUPPORTED;
    if (!tap_scratch) tap_state = nullptr;
    if (wl_streaming_off()) return WL_ERR_UNSUPPORTED;
    if (mode == 2 && (2 * Kh < L - 2 || 2 * Kw < L - 2)) return WL_ERR_UNSUPPORTED;   // single-fold corner: direct kernels
    if (planes == 0) return 0;
    const WlSfbReq r = {ll, ll_plane_stride, ll_row_stride, highs, y, planes, Kh, Kw, OH, OW,
                        {g_w_lo, g_w_hi, g_h_lo, g_h_hi}, L, L, mode, policy, (float*)tap_scratch, tap_state, stream};
    WL_DISPATCH_FLOAT(dtype, return wl_sfb_strip_dispatch<T>(r));
}

extern "C" int wl_dwt2d_synthesis_stream(const void* ll, int64_t ll_plane_stride, int ll_row_stride, const void* highs,
                                         void* y, int dtype, int64_t planes, int Kh, int Kw, int OH, int OW,
                                         const void* g_w_lo, const void* g_w_hi, const void* g_h_lo, const void* g_h_hi,
                                         int L, int mode, int policy, void* stream) {
    return wl_dwt2d_synthesis_stream_ex(ll, ll_plane_stride, ll_row_stride, highs, y, dtype, planes, Kh, Kw, OH, OW, g_w_lo, g_w_hi,
                                        g_h_lo, g_h_hi, L, mode, policy, nullptr, nullptr, stream);
}

#endif   // WL_STRIP_PARTS & 2

#if WL_STRIP_PARTS & 4
// ---- streaming level-1 DTCWT forward / ScatLayer over column strips (wl_dtcwt_strip.h) ------------------------------
#include "wl_dtcwt_strip.h"

// The launchers of this part that wl_api.inc calls are declared in wl_dt_api.h and defined here once, as templates over the element
// type: this instantiates one of them for the three types with streaming kernels (float64 is declined in the header).
#define WL_DT_INSTANTIATE(NAME, ARGS, ...)                             \
    template int NAME<float>(const ARGS<float>&, __VA_ARGS__);         \
    template int NAME<wl_half>(const ARGS<wl_half>&, __VA_ARGS__);     \
    template int NAME<wl_bf16>(const ARGS<wl_bf16>&, __VA_ARGS__);

template <typename T, int L0, int L1>
static int wl_dtfwd1_strip_launch(const WlDtFwd1Args<T>& f, void* stream) {
    typedef WlDtFwd1Strip<T, L0, L1> K;
    const int A = K::A, M = K::M;
    WlDtStripArgs<T> a = {};
    a.f = f;
    const int quads = f.We / 2;
    int cap = 64 * WL_STRIP_CWAVES;
    for (;; cap -= 64) {
        if (cap < 64) return WL_ERR_UNSUPPORTED;
        a.nstrips = wl_cdiv(quads, cap);
        a.strip_quads = wl_cdiv(quads, a.nstrips);
        a.nstrips = wl_cdiv(quads, a.strip_quads);
        const int np = (2 * a.strip_quads + 2 * M + 2 * A) / A + 1;
        const int ng = np * A / 4;
        a.dma_pitch = np * 16;
        a.st_pitch = wl_align_up((4 * ng + 2 + A + 2 * K::NC2 + 2) * 4, 16);
        a.dma_off = 0;
        a.st_off = K::D * 4 * a.dma_pitch;
        a.lds_bytes = a.st_off + 2 * 4 * a.st_pitch;
        if (wl_cdiv(np, 64) <= WL_STRIP_MAXPPR && a.lds_bytes <= 64 * 1024) break;
    }
    wl_pick_segments(f.He, f.NC * a.nstrips, a.lds_bytes <= 53 * 1024 ? 3 : 2, 2 * M, 4, &a.seg_rows, &a.nseg);
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        if (s.np < 1 || s.ppr > WL_STRIP_MAXPPR || s.np * 16 > a.dma_pitch) return WL_ERR_UNSUPPORTED;
        if ((4 * s.ng + s.dm) * 4 > a.st_pitch) return WL_ERR_UNSUPPORTED;
        if (s.lane_off + 8 * (s.q1 - s.q0 - 1) + 8 * K::NC2 > a.st_pitch) return WL_ERR_UNSUPPORTED;
        const int e_hi = 2 * s.q1 - 1 + M;
        const int last = e_hi > f.W - 1 ? f.W - 1 : e_hi;
        const int nl = s.e_lo < 0 ? -s.e_lo : 0, nr = e_hi > f.W - 1 ? e_hi - (f.W - 1) : 0;
        if (nl + nr > 64) return WL_ERR_UNSUPPORTED;
        if (f.ext != WL_EXT_ZERO)
            for (int c = 0; c < nl + nr; ++c) {   // the mirrored halo comes from inside the columns the strip loads
                const int e = c < nl ? s.e_lo + c : f.W + (c - nl);
                const int src = wl_ext_padded(e, f.W, 0, f.We - f.W, f.ext);
                if (src < s.c0a || src > last || src < 0) return WL_ERR_UNSUPPORTED;
            }
        for (int q = 0; q < s.ppr; ++q) {     // no DMA instruction whose lanes are all off
            bool any = false;
            for (int l = 0; l < 64 && !any; ++l) {
                const int p = q * 64 + l;
                if (p >= s.np) break;
                any = (unsigned)(s.c0a + p * A) < (unsigned)f.W;
            }
            if (!any) return WL_ERR_UNSUPPORTED;
        }
    }
    a.nblocks = f.NC * a.nstrips * a.nseg;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

// Called by wl_dtfwd1_launch (wl_api.inc) before the tile kernels; WL_ERR_UNSUPPORTED = not this kernel's case.
template <typename T>
int wl_dtfwd1_strip(const WlDtFwd1Args<T>& f, void* stream) {
    const int SZ = (int)sizeof(T);
    if (f.combine || (f.ext != WL_EXT_SYM && f.ext != WL_EXT_ZERO)) return WL_ERR_UNSUPPORTED;
    if ((f.W * SZ) % 16 || (uintptr_t)f.x % 16 || f.W < 32 || f.H < 8 || (int64_t)f.He * f.We >= (1LL << 28)) return WL_ERR_UNSUPPORTED;
    if (f.NC * (int64_t)wl_cdiv(f.He, 64) < wl_num_cus() || f.W * SZ < 1024) return WL_ERR_UNSUPPORTED;   // small work: tile kernels
    // Measured against the tile kernels (tools/gpu_dt_probe.py, 64x3x512x512 / 16x3x1024x1024): the DTCWT level 1 reaches
    // the practical HBM ceiling here (0.61 / 0.67 of peak against 0.58 / 0.60); the ScatLayer epilogue is bound by its
    // instruction stream, not by bytes, and is no faster (0.18 ms either way, slower on 256-wide planes): the caller keeps
    // it on the tile kernels unless wl_set_option("scat_stream", 1);
    // the 13 / 19-tap pair does not fit its two register windows into 128 registers: tile kernels.
    if (f.L0 == 5 && f.L1 == 7) return wl_dtfwd1_strip_launch<T, 5, 7>(f, stream);       // near_sym_a
    if (f.L0 == 9 && f.L1 == 7) return wl_dtfwd1_strip_launch<T, 9, 7>(f, stream);       // antonini
    if (f.L0 == 5 && f.L1 == 3) return wl_dtfwd1_strip_launch<T, 5, 3>(f, stream);       // legall
    return WL_ERR_UNSUPPORTED;
}
WL_DT_INSTANTIATE(wl_dtfwd1_strip, WlDtFwd1Args, void*)

// ---- streaming level-1 DTCWT inverse over column strips ---------------------------------------------------------------
template <typename T, int L0, int L1, int SCAT = 0, int PP = 1>
static int wl_dtinv1_strip_launch1(const WlDtInv1Args<T>& f, void* stream) {
    typedef WlDtInv1Strip<T, L0, L1, SCAT, PP> K;
    const int M = K::M;
    WlDtIStripArgs<T> a = {};
    a.f = f;
    const int W2 = f.W / 2;
    // one quad per stager lane: at most 256 quads (a strip's own and its neighbours' halo quads) are staged per quad row
    int cap = 64 * K::CW / PP;
    if (cap > 256 - 2 * ((M + 1) / 2)) cap = W2 <= 256 ? 256 : 256 - 2 * ((M + 1) / 2);   // (a single strip has no neighbours)
    a.nstrips = wl_cdiv(W2, cap);
    a.strip_quads = wl_cdiv(W2, a.nstrips);
    a.nstrips = wl_cdiv(W2, a.strip_quads);
    if (PP > 1 && a.nstrips != 1) return WL_ERR_UNSUPPORTED;     // (PP whole planes per workgroup)
    a.st_pitch = PP * (2 * a.strip_quads + 2 * M + 4) * 16;      // (PP = 2: the two planes' rows side by side)
    a.st_off = 0;
    a.lds_bytes = 2 * 2 * a.st_pitch;
    wl_pick_segments(f.H, wl_cdiv64(f.NC, PP) * a.nstrips, a.lds_bytes <= 40 * 1024 && !K::PAIRS ? 3 : 2, 2 * M + 1, 4, &a.seg_rows, &a.nseg, 32, true);   // (PAIRS: 127 registers)
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        const int e_hi = 2 * s.q1 - 1 + M;
        if (s.nq < 1 || s.nq > 256 / PP || (e_hi - s.px0 + 1) * 16 > a.st_pitch / PP || s.e_lo < s.px0) return WL_ERR_UNSUPPORTED;
        // the mirrored pixels of either edge must belong to quads this strip stages
        if (f.ext != WL_EXT_ZERO) {
            if (s.e_lo < 0 && (-1 - s.e_lo) / 2 > s.Qa + s.nq - 1) return WL_ERR_UNSUPPORTED;
            if (e_hi > f.W - 1 && (2 * f.W - 1 - e_hi) / 2 < s.Qa) return WL_ERR_UNSUPPORTED;
        }
    }
    a.nblocks = wl_cdiv64(f.NC, PP) * a.nstrips * a.nseg;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}
// planes of up to 256 columns (128 quad columns): two planes per workgroup
template <typename T, int L0, int L1, int SCAT = 0>
static int wl_dtinv1_strip_launch(const WlDtInv1Args<T>& f, void* stream) {
#ifndef WL_DTI1_PAIRS
#define WL_DTI1_PAIRS 1
#endif
    if (f.W <= 128 && f.NC >= 4) return wl_dtinv1_strip_launch1<T, L0, L1, SCAT, 4>(f, stream);   // (64 .. 128 columns: four)
    if (WL_DTI1_PAIRS && f.W <= 256 && f.NC >= 2) return wl_dtinv1_strip_launch1<T, L0, L1, SCAT, 2>(f, stream);
    return wl_dtinv1_strip_launch1<T, L0, L1, SCAT, 1>(f, stream);
}

template <typename T>
int wl_dtinv1_strip(const WlDtInv1Args<T>& f, void* stream) {
    const int SZ = (int)sizeof(T);
    if (f.ext != WL_EXT_SYM && f.ext != WL_EXT_ZERO) return WL_ERR_UNSUPPORTED;
    if ((f.W & 1) || (f.H & 1) || f.W < 32 || f.H < 4 * f.M + 4 || (int64_t)f.H * f.W >= (1LL << 28) || (uintptr_t)f.y % (2 * SZ)) return WL_ERR_UNSUPPORTED;
    if (f.NC * (int64_t)wl_cdiv(f.H, 64) < wl_num_cus() || f.W < WL_FOUR_MIN) return WL_ERR_UNSUPPORTED;   // small work: tile kernels
    if (f.sz) {
        // the fused ScatLayer backward (dZ, re / r, im / r instead of ll / highs): the near_sym_a forward pair, one channel set
        // per image (combine_colour shares the magnitudes between the colours: tile kernel)
        if (f.combine || !f.sdx || !f.sdy) return WL_ERR_UNSUPPORTED;
        if (f.L0 == 5 && f.L1 == 7) return wl_dtinv1_strip_launch<T, 5, 7, 1>(f, stream);
        if (f.L0 == 13 && f.L1 == 19) return wl_dtinv1_strip_launch<T, 13, 19, 1>(f, stream);   // near_sym_b
        return WL_ERR_UNSUPPORTED;
    }
    if (!f.ll || !f.highs) return WL_ERR_UNSUPPORTED;
    // 8-byte loads of ll pixel pairs and (re, im) pairs
    if ((uintptr_t)f.ll % (2 * SZ) || (uintptr_t)f.highs % (2 * SZ) || (f.ll_row_stride & 1) || (f.ll_plane_stride & 1)) return WL_ERR_UNSUPPORTED;
    if (f.L0 == 7 && f.L1 == 5) return wl_dtinv1_strip_launch<T, 7, 5>(f, stream);       // near_sym_a
    if (f.L0 == 7 && f.L1 == 9) return wl_dtinv1_strip_launch<T, 7, 9>(f, stream);       // antonini
    if (f.L0 == 3 && f.L1 == 5) return wl_dtinv1_strip_launch<T, 3, 5>(f, stream);       // legall
    if (f.L0 == 19 && f.L1 == 13) return wl_dtinv1_strip_launch<T, 19, 13>(f, stream);    // near_sym_b
    // backward passes of the level-1 forward: an inverse with the forward taps
    if (f.L0 == 5 && f.L1 == 7) return wl_dtinv1_strip_launch<T, 5, 7>(f, stream);       // near_sym_a
    if (f.L0 == 9 && f.L1 == 7) return wl_dtinv1_strip_launch<T, 9, 7>(f, stream);       // antonini
    if (f.L0 == 5 && f.L1 == 3) return wl_dtinv1_strip_launch<T, 5, 3>(f, stream);       // legall
    if (f.L0 == 13 && f.L1 == 19) return wl_dtinv1_strip_launch<T, 13, 19>(f, stream);    // near_sym_b
    return WL_ERR_UNSUPPORTED;
}
WL_DT_INSTANTIATE(wl_dtinv1_strip, WlDtInv1Args, void*)

// ---- levels 1 + 2 of the DTCWT forward in one streaming launch (wl_dtcwt_fused.h) ----------------------------------------
#include "wl_dtcwt_fused.h"

template <typename T, int L0, int L1, int LQ>
static int wl_dtfwd12_launch(WlDtFusedArgs<T>& a, void* stream) {
    typedef WlDtFwd12Strip<T, L0, L1, LQ> K;
    const WlDtFwd1Args<T>& f = a.f;
    const int Q = f.W / 2, HH = K::HQ / 2;
    // 256 level-1 lanes per strip: a strip's own quad columns and, towards a neighbouring strip, the HQ / 2 quad columns
    // of it that level 2 reads (the plane's edges are mirrored copies, not lanes)
    if (Q <= 64 * K::CW) { a.nstrips = 1; a.strip_quads = Q; }
    else {
        const int cap = 64 * K::CW - 2 * HH;
        a.nstrips = wl_cdiv(Q, cap);
        a.strip_quads = wl_align_up(wl_cdiv(Q, a.nstrips), 2);
        a.nstrips = wl_cdiv(Q, a.strip_quads);
    }
    int cells = 0;
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        if (s.qb - s.qa > 64 * K::CW || (s.q1 - s.q0) > 64 * K::QW || ((s.q1 - s.q0) & 1) || (s.q0 & 1)) return WL_ERR_UNSUPPORTED;
        if (s.ng > 64 * K::MAXG || s.nl + s.nr > 64 || s.nl > f.W || s.nr > f.W) return WL_ERR_UNSUPPORTED;
        const int c = 2 * (s.qb - s.qa) + 2 * K::M + 8;
        if (c > cells) cells = c;
    }
    a.st_pitch = wl_align_up(cells * 4, 16);
    a.l1_pitch = (2 * a.strip_quads + 2 * K::HQ) * 4;
    a.st_off = 0;
    a.l1_off = a.st_off + 2 * 4 * a.st_pitch;
    a.w2_off = a.l1_off + 2 * 4 * a.l1_pitch;
    a.lds_bytes = a.w2_off + (K::NW2 / 2) * 64 * K::QW * 16;
    if (a.lds_bytes > 80 * 1024) return WL_ERR_UNSUPPORTED;
    int seg_rows = f.H, nseg = 1;
    wl_pick_segments(f.H, f.NC * a.nstrips, 2, 4 * (K::WARM1 + 2 * K::HG + 1), 4, &seg_rows, &nseg);
#ifdef WL_DT12_NSEG
    seg_rows = wl_align_up(wl_cdiv(f.H, WL_DT12_NSEG), 4);
#endif
    a.seg_groups = seg_rows / 4;
    a.nseg = wl_cdiv(f.H / 4, a.seg_groups);
    a.nblocks = f.NC * a.nstrips * a.nseg;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
static int wl_dtfwd12_any(WlDtFusedArgs<T>& a, int LQ, int policy, void* stream) {
    const int SZ = (int)sizeof(T);
    const WlDtFwd1Args<T>& f = a.f;
    const int64_t planes = f.NC;
    const int H = f.H, W = f.W, L0 = f.L0, L1 = f.L1;
    if ((H % 4) || (W % 4) || H < 32 || W < 32 || (int64_t)H * W >= (1LL << 28)) return WL_ERR_UNSUPPORTED;
    if ((uintptr_t)f.x % SZ || (uintptr_t)f.highs % (2 * SZ) || (uintptr_t)a.ll2 % (2 * SZ) || (uintptr_t)a.highs2 % (2 * SZ)) return WL_ERR_UNSUPPORTED;
    // small work: per-level kernels.  (224-column planes only in numbers: 256x3x224^2 J = 2 forward 0.232 -> 0.190 ms, 128x3x224^2 0.111 -> 0.112,
    // 64x3x224^2 0.053 -> 0.059 - tools/gpu_r5z.py)
    if (!policy && (planes * (int64_t)wl_cdiv(H, 64) < wl_num_cus() || (W < 256 && !(W >= 224 && planes >= 3 * (int64_t)wl_num_cus())))) return WL_ERR_UNSUPPORTED;
    if (LQ != 10) return WL_ERR_UNSUPPORTED;                                                    // qshift_a, qshift_06
    if (L0 == 5 && L1 == 7) return wl_dtfwd12_launch<T, 5, 7, 10>(a, stream);                   // near_sym_a
    // (antonini's 9 / 7 pair needs more than the 96 registers of five waves per SIMD: per-level kernels)
    if (L0 == 5 && L1 == 3) return wl_dtfwd12_launch<T, 5, 3, 10>(a, stream);                   // legall
    return WL_ERR_UNSUPPORTED;
}

extern "C" int wl_dtcwt_fwd_level12(const void* x, void* highs1, void* ll2, void* highs2, int dtype, int64_t planes, int H,
                                    int W, const void* h0o, int L0, const void* h1o, int L1, const void* h0a,
                                    const void* h0b, const void* h1a, const void* h1b, int LQ, int mode, int policy,
                                    void* stream) {
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || LQ < 2 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS || LQ > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (policy < 0 || policy > 1) return WL_ERR_UNSUPPORTED;
    if (mode != 1) return WL_ERR_UNSUPPORTED;                   // symmetric (coldfilt / rowdfilt know nothing else)
    if (planes == 0) return 0;
    if (wl_streaming_off()) return WL_ERR_UNSUPPORTED;
    WL_DISPATCH_FLOAT(dtype, {
        WlDtFwd1Args<T> f = wl_dtfwd1_args<T>(x, planes, 1, H, W, h0o, L0, h1o, L1, WL_EXT_SYM);
        f.highs = (T*)highs1;
        WlDtFusedArgs<T> a = wl_dtfused_args<T>(f, (T*)ll2, (T*)highs2, h0a, h0b, h1a, h1b);
        return wl_dtfwd12_any(a, LQ, policy, stream);
    });
}

// ---- lean level-1 forward / ScatLayer forward on the stagers and level-1 lanes of the fused kernel (MODE 0 / 1) ----------
template <typename T, int L0, int L1, int MODE, int CW, int PP = 1>
static int wl_dtlean1_launch(const WlDtFwd1Args<T>& f, void* stream, const float* h2 = nullptr, int L2 = 0) {
    typedef WlDtFwd12Strip<T, L0, L1, 10, MODE, CW, PP> K;
    WlDtFusedArgs<T> a = wl_dtfused_args<T>(f);
    a.h2 = h2; a.L2 = L2;                                       // (MODE 6)
    const int Q = f.W / 2;
    a.nstrips = wl_cdiv(Q, 64 * CW / PP);
    a.strip_quads = wl_align_up(wl_cdiv(Q, a.nstrips), 2);
    a.nstrips = wl_cdiv(Q, a.strip_quads);
    if (PP > 1 && a.nstrips != 1) return WL_ERR_UNSUPPORTED;      // (PP whole planes per workgroup)
    int cells = 0;
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        if (s.qb - s.qa > 64 * CW / PP || PP * s.ng > 64 * K::MAXG || s.nl + s.nr > 64 / PP) return WL_ERR_UNSUPPORTED;
        const int c = 2 * (s.qb - s.qa) + 2 * K::M + 8;
        if (c > cells) cells = c;
    }
    a.st_pitch = PP * wl_align_up(cells * 4, 16);              // (PP = 2: the two planes' rows side by side)
    a.l1_pitch = 0;
    a.st_off = 0;
    a.l1_off = a.w2_off = a.lds_bytes = 2 * 4 * a.st_pitch;
    int seg_rows = f.H, nseg = 1;
    int per_cu = 4 * K::kMinWaves / K::kWaves;                 // resident workgroups per CU: registers, then LDS
    if (K::kLong) per_cu = MODE == 3 || MODE == 6 ? 1 : 2;     // (13 / 19 taps: 115-119 registers, the training forward 142, the band-pass variant 206)
    if (per_cu > 160 * 1024 / a.lds_bytes) per_cu = 160 * 1024 / a.lds_bytes;
    // (one workgroup per CU - the 13 / 19-tap training forward and band-pass kernels: a partly filled last round costs a whole one,
    // whole rounds are counted; with several workgroups per CU the workgroups of a partly filled round run faster: fractional rounds)
    wl_pick_segments(f.H, wl_cdiv64(f.NC, PP) * a.nstrips, per_cu, 4 * K::WARM1 + 2, 4, &seg_rows, &nseg, 32, per_cu > 1);
    a.seg_groups = seg_rows / 4;
    a.nseg = wl_cdiv(f.H / 4, a.seg_groups);
    a.nblocks = wl_cdiv64(f.NC, PP) * a.nstrips * a.nseg;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
int wl_dtfwd1_lean(const WlDtFwd1Args<T>& f, void* stream) {
    const int SZ = (int)sizeof(T);
    if (f.combine || f.ext != WL_EXT_SYM || f.He != f.H || f.We != f.W || (f.H % 4) || (f.W % 4)) return WL_ERR_UNSUPPORTED;
    if (f.H < 32 || f.W < 32 || (int64_t)f.H * f.W >= (1LL << 28) || (uintptr_t)f.x % SZ) return WL_ERR_UNSUPPORTED;
    if ((uintptr_t)f.ll % (2 * SZ) || (uintptr_t)f.highs % (2 * SZ)) return WL_ERR_UNSUPPORTED;
    // planes of 64 .. 128 columns: four per workgroup, one per level-1 wave (tools/gpu_four_probe.py: 1.6-1.9x the tile kernels at
    // 72-88 columns, equal at 64)
    // (a plane's 16 stager lanes for mirrored cells: 2 M <= 16 - the 13 / 19-tap pair goes two planes to a workgroup)
    const bool four = f.W <= 128 && f.W >= WL_FOUR_MIN && f.NC >= 4 && f.L0 <= 17 && f.L1 <= 17;
    if (f.NC * (int64_t)wl_cdiv(f.H, 64) < wl_num_cus() || f.W < WL_FOUR_MIN) return WL_ERR_UNSUPPORTED;   // small work: tile kernels
    const bool narrow = f.W <= 256;
    // planes of up to 256 columns: two planes per workgroup of the wide-plane kernel (WL_DT12_PAIRS, default on) or one per
    // workgroup of two level-1 waves + two stagers
#ifndef WL_DT12_PAIRS
#define WL_DT12_PAIRS 1
#endif
#define WL_NARROW(l0, l1, mode_) (four ? wl_dtlean1_launch<T, l0, l1, mode_, 4, 4>(f, stream) : WL_DT12_PAIRS && f.NC >= 2 ? wl_dtlean1_launch<T, l0, l1, mode_, 4, 2>(f, stream) : wl_dtlean1_launch<T, l0, l1, mode_, 2>(f, stream))
#define WL_LEAN(l0, l1)                                                                              \
    if (f.L0 == l0 && f.L1 == l1) {                                                                  \
        if (f.z && f.drdx) return narrow ? WL_NARROW(l0, l1, 3) : wl_dtlean1_launch<T, l0, l1, 3, 4>(f, stream); \
        if (f.z) return narrow ? WL_NARROW(l0, l1, 1) : wl_dtlean1_launch<T, l0, l1, 1, 4>(f, stream); \
        return narrow ? WL_NARROW(l0, l1, 0) : wl_dtlean1_launch<T, l0, l1, 0, 4>(f, stream); \
    }
    WL_LEAN(5, 7)        // near_sym_a
    WL_LEAN(5, 3)        // legall
    WL_LEAN(13, 19)      // near_sym_b (round 6: tap pairs shared between the row and column filters, windows of 20 rows)
#undef WL_LEAN
#undef WL_NARROW
    return WL_ERR_UNSUPPORTED;
}
// ScatLayer inference with the rotationally symmetric level-1 filters ('near_sym_b_bp': 13 / 19 / 19 taps, a third band-pass filter for the
// diagonal sub-band) on the lean kernel (MODE 6); called by wl_dtfwd1_rot_run (wl_api.inc) before the tile kernel WlDtFwd1Rot.
template <typename T>
int wl_dtrot_lean(const WlDtFwd1Args<T>& f, const void* h2, int L2, void* stream) {
    const int SZ = (int)sizeof(T);
    if (!f.z || f.ll || f.highs || f.drdx || f.drdy || f.combine || f.ext != WL_EXT_SYM || f.He != f.H || f.We != f.W || (f.H % 4) || (f.W % 4)) return WL_ERR_UNSUPPORTED;
    if (f.H < 40 || f.W < 128 || (int64_t)f.H * f.W >= (1LL << 28) || (uintptr_t)f.x % SZ || !h2) return WL_ERR_UNSUPPORTED;
    if (f.L0 != 13 || f.L1 != 19 || L2 < 1 || L2 > 19 || !(L2 & 1)) return WL_ERR_UNSUPPORTED;
    if (f.NC * (int64_t)wl_cdiv(f.H, 64) < wl_num_cus()) return WL_ERR_UNSUPPORTED;        // small work: tile kernel
    if (f.W <= 256 && f.NC >= 2) return wl_dtlean1_launch<T, 13, 19, 6, 4, 2>(f, stream, (const float*)h2, L2);
    return wl_dtlean1_launch<T, 13, 19, 6, 4, 1>(f, stream, (const float*)h2, L2);
}
WL_DT_INSTANTIATE(wl_dtrot_lean, WlDtFwd1Args, const void*, int, void*)
WL_DT_INSTANTIATE(wl_dtfwd1_lean, WlDtFwd1Args, void*)

// ---- streaming level >= 2 DTCWT inverse over column strips (wl_dtcwt_fused.h) ----------------------------------------------
template <typename T, int LQ>
static int wl_dtinv2_strip_launch(const WlDtInv2Args<T>& f, void* stream) {
    typedef WlDtInv2Strip<T, LQ> K;
    WlDtI2StripArgs<T> a = {};
    a.f = f;
    const int W2 = f.w / 2, H2 = f.h / 2;
    // one quad per stager lane: a strip's own quad columns and, towards a neighbouring strip, D2 of its quad columns
    const int cap = W2 <= K::QCAP ? K::QCAP : (64 * K::SW - 2 * K::D2 < K::QCAP ? 64 * K::SW - 2 * K::D2 : K::QCAP);
    a.nstrips = wl_cdiv(W2, cap);
    a.strip_quads = wl_cdiv(W2, a.nstrips);
    a.nstrips = wl_cdiv(W2, a.strip_quads);
    a.st_pitch = (a.strip_quads + 2 * K::D2) * 32;
    a.st_off = 0;
    a.lds_bytes = 2 * 2 * a.st_pitch;
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        if (s.nq < 1 || s.nq > 64 * K::SW || s.q1 - s.q0 > K::QCAP) return WL_ERR_UNSUPPORTED;
    }
    int seg_rows = 4 * H2, nseg = 1;
    wl_pick_segments(4 * H2, f.NC * a.nstrips, 4 * K::kMinWaves / K::kWaves, 4 * (2 * K::D2 + 1), 4, &seg_rows, &nseg);
    a.seg_groups = seg_rows / 4;
    a.nseg = wl_cdiv(H2, a.seg_groups);
    a.nblocks = f.NC * a.nstrips * a.nseg;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
int wl_dtinv2_strip(const WlDtInv2Args<T>& f, void* stream) {
    const int SZ = (int)sizeof(T);
    if (!f.ll || !f.highs) return WL_ERR_UNSUPPORTED;
    if ((f.w & 1) || (f.h & 1) || (uintptr_t)f.ll % (2 * SZ) || (uintptr_t)f.highs % (2 * SZ) || (uintptr_t)f.y % (2 * SZ) ||
        (f.ll_row_stride & 1) || (f.ll_plane_stride & 1) || f.w < 16 || f.h < 16 || (int64_t)f.h * f.w >= (1LL << 26)) return WL_ERR_UNSUPPORTED;
    #ifndef WL_DTINV2_MINW
#define WL_DTINV2_MINW 192    // (tools/gpu_lean_f16_probe.py: from 192 output columns the strip kernel wins, at 128 the tile kernel)
#endif
    if (f.NC * (int64_t)wl_cdiv(2 * f.h, 64) < wl_num_cus() || 2 * f.w < WL_DTINV2_MINW) return WL_ERR_UNSUPPORTED;   // small work: tile kernels
    if (f.L == 10) return wl_dtinv2_strip_launch<T, 10>(f, stream);       // qshift_a, qshift_06
    if (f.L == 14) return wl_dtinv2_strip_launch<T, 14>(f, stream);       // qshift_b
    if (f.L == 18) return wl_dtinv2_strip_launch<T, 18>(f, stream);       // qshift_d
    return WL_ERR_UNSUPPORTED;
}
WL_DT_INSTANTIATE(wl_dtinv2_strip, WlDtInv2Args, void*)

// ---- level >= 2 forward alone on the stagers and level-2 lanes of the fused kernel (MODE 4) ------------------------------------
template <typename T, int CW, int MODE = 4, int LQ = 10>
static int wl_dtfwd2_lean_launch(const WlDtFwd2Args<T>& g, void* stream) {
    typedef WlDtFwd12Strip<T, 5, 7, LQ, MODE, CW> K;
    // this launch has no level 1: of the level-1 struct its kernel reads the input, the sizes and - MODE 5 - where ScatLayerj2's second
    // scale puts its entries; there are no level-1 taps to pass (the tap counts are the kernel's template arguments), so L0 = L1 = 1, M = 0
    WlDtFwd1Args<T> f = wl_dtfwd1_args<T>(g.x, g.NC, 1, g.H, g.W, nullptr, 1, nullptr, 1, WL_EXT_SYM);
    if (MODE == 5) { f.z = g.z; f.z_bs = g.z_bs; f.z_ll_off = g.z_ll_off; f.z_mag_off = g.z_mag_off; f.C = g.C; f.magbias = g.magbias; }
    WlDtFusedArgs<T> a = wl_dtfused_args<T>(f, g.ll, g.highs, g.h0a, g.h0b, g.h1a, g.h1b);
    const int Q = g.W / 2;
    a.nstrips = wl_cdiv(Q, 64 * CW);
    a.strip_quads = wl_align_up(wl_cdiv(Q, a.nstrips), 2);
    a.nstrips = wl_cdiv(Q, a.strip_quads);
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Strip s = K::geometry(a, st, 0);
        if ((s.q1 - s.q0) > 64 * K::QW || ((s.q1 - s.q0) & 1) || (s.q0 & 1) || s.ng > 64 * K::MAXG || s.nl + s.nr > 64) return WL_ERR_UNSUPPORTED;
    }
    a.st_pitch = 0; a.st_off = 0;
    a.l1_pitch = (2 * a.strip_quads + 2 * K::HQ) * 4;
    a.l1_off = 0;
    a.w2_off = a.l1_off + 2 * 4 * a.l1_pitch;
    a.lds_bytes = a.w2_off + (K::NW2 / 2) * 64 * K::QW * 16;
    int per_cu = 4 * K::kMinWaves / K::kWaves;
    if (per_cu > 160 * 1024 / a.lds_bytes) per_cu = 160 * 1024 / a.lds_bytes;
    int seg_rows = g.H, nseg = 1;
    wl_pick_segments(g.H, g.NC * a.nstrips, per_cu, 4 * (2 * K::HG + 1), 4, &seg_rows, &nseg, 32, true);
    a.seg_groups = seg_rows / 4;
    a.nseg = wl_cdiv(g.H / 4, a.seg_groups);
    a.nblocks = g.NC * a.nstrips * a.nseg;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
int wl_dtfwd2_lean(const WlDtFwd2Args<T>& g, void* stream) {
    const int SZ = (int)sizeof(T);
    if ((!g.highs && !g.z) || (g.L != 10 && g.L != 14) || g.padr || g.padc || (g.H % 4) || (g.W % 4) || g.H < 32 || g.W < 32) return WL_ERR_UNSUPPORTED;
    if ((int64_t)g.H * g.W >= (1LL << 28) || (uintptr_t)g.x % SZ || (uintptr_t)g.ll % (2 * SZ) || (uintptr_t)g.highs % (2 * SZ)) return WL_ERR_UNSUPPORTED;
    #ifndef WL_DTFWD2_MINW
#define WL_DTFWD2_MINW 128   // (tools/gpu_lean_f16_probe.py: 160 .. 224 columns 1.07-1.25x float32, 1.4-2x float16; neutral at 128)
#endif
    if (g.NC * (int64_t)wl_cdiv(g.H, 64) < wl_num_cus() || g.W < WL_DTFWD2_MINW) return WL_ERR_UNSUPPORTED;   // small work: tile kernels
    if (g.L == 14) {                                              // qshift_b (14 taps; ScatLayerj2 is built on qshift_a)
        if (g.z) return WL_ERR_UNSUPPORTED;
        return g.W <= 256 ? wl_dtfwd2_lean_launch<T, 2, 4, 14>(g, stream) : wl_dtfwd2_lean_launch<T, 4, 4, 14>(g, stream);
    }
    // (qshift_d, 18 taps: instantiated and measured in round 6 - 34 spilled scalars, one workgroup per CU - no faster than the tile kernel:
    // 64x3x512^2 J = 3 forward 0.454 / 0.459 ms; the level >= 2 INVERSE of 18 taps is on its strip kernel, 0.65 -> 0.47 ms)
    if (g.z) return g.W <= 256 ? wl_dtfwd2_lean_launch<T, 2, 5>(g, stream) : wl_dtfwd2_lean_launch<T, 4, 5>(g, stream);
    return g.W <= 256 ? wl_dtfwd2_lean_launch<T, 2>(g, stream) : wl_dtfwd2_lean_launch<T, 4>(g, stream);
}
WL_DT_INSTANTIATE(wl_dtfwd2_lean, WlDtFwd2Args, void*)
#undef WL_DT_INSTANTIATE
#endif   // WL_STRIP_PARTS & 4
