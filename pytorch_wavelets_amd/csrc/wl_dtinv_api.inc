// C ABI of the fused DTCWT inverse (levels 2 + 1 in one streaming launch, wl_dtcwt_inv_fused.h).  Its own translation unit in
// the HIP build (wl_dtinv_hip.hip, -fno-slp-vectorize like the other streaming kernels); included after the backend header.
#include "wl_api_common.h"
#include "wl_dt_api.h"      // wl_streaming_off
#include "wl_dtcwt_inv_fused.h"

template <typename T, int L0, int L1, int LQ>
static int wl_dtinv21_launch(WlDtInv21Args<T>& a, void* stream) {
    typedef WlDtInv21Strip<T, L0, L1, LQ> K;
    const int M = K::M, D2 = K::D2, NG = K::NG;
    const int W1q = a.W / 2, H1q = a.H / 2;
    if (H1q <= K::ME || a.H / 4 <= D2 || a.W / 4 <= D2 || a.W <= 2 * M) return WL_ERR_UNSUPPORTED;   // (single folds only)
    // strips: at most 256 level-1 quads (its own + halo quads towards a neighbouring strip) are staged per quad row, and the
    // in-plane lowpass columns they read must come from at most 128 level-2 quad columns (two waves per column phase)
    int cap = W1q <= 64 * K::CW1 ? 64 * K::CW1 : 64 * K::CW1 - 2 * ((M + 1) / 2) - 2;
    cap &= ~1;
    a.nstrips = wl_cdiv(W1q, cap);
    a.strip_quads = wl_align_up(wl_cdiv(W1q, a.nstrips), 2);
    a.nstrips = wl_cdiv(W1q, a.strip_quads);
    a.seg_rows = a.H; a.nseg = 1; a.P1 = 0;
    int cells2 = 0, nk2 = 0;
    for (int st = 0; st < a.nstrips; ++st) {
        const typename K::Geo s = K::geometry(a, st, 0);
        const int e_hi = 2 * s.q1 - 1 + M;
        if (s.nq < 1 || s.nq > 64 * K::SW1 || s.q1 - s.q0 > 64 * K::CW1 || s.e_lo < s.px0) return WL_ERR_UNSUPPORTED;
        if ((e_hi - s.px0 + 1) * 16 > (2 * a.strip_quads + 2 * M + 4) * 16) return WL_ERR_UNSUPPORTED;
        // the mirrored pixels of either edge must belong to quads this strip stages
        if (s.e_lo < 0 && (-1 - s.e_lo) / 2 > s.Qa + s.nq - 1) return WL_ERR_UNSUPPORTED;
        if (e_hi > a.W - 1 && (2 * a.W - 1 - e_hi) / 2 < s.Qa) return WL_ERR_UNSUPPORTED;
        if (s.kb - s.ka + 1 > 32 * K::CW2 || s.nq2 < 1 || s.nq2 > 64 * K::SW2) return WL_ERR_UNSUPPORTED;
        if (s.kb - s.ka + 1 > nk2) nk2 = s.kb - s.ka + 1;
        if (s.kb - s.ka + 1 + 2 * D2 > cells2) cells2 = s.kb - s.ka + 1 + 2 * D2;
    }
    a.st1_pitch = (2 * a.strip_quads + 2 * M + 4) * 16;
    a.st2_pitch = cells2 * 32;
    a.l1_pitch = nk2 * 16;
    a.st1_off = 0;
    a.st2_off = a.st1_off + 2 * 4 * a.st1_pitch;
    a.l1_off = a.st2_off + 2 * 2 * a.st2_pitch;
    a.lds_bytes = a.l1_off + 4 * NG * a.l1_pitch;
    if (a.lds_bytes > 160 * 1024) return WL_ERR_UNSUPPORTED;
    // row segments: whole rounds of one workgroup per CU; a segment costs its phases (pipeline fill + halo group included)
    {
        const int64_t units = a.NC * a.nstrips, slots = wl_num_cus();
        int64_t best = -1;
        int maxseg = a.H / 32;
        if (maxseg < 1) maxseg = 1;
        if (maxseg > 64) maxseg = 64;
        for (int n = 1; n <= maxseg; ++n) {
            const int sr = wl_align_up(wl_cdiv(a.H, n), 4 * K::PF1);   // (whole sets of the level-1 stagers' registers)
            const int ns = wl_cdiv(a.H, sr);
            const int64_t rounds = wl_cdiv64(units * ns, slots);
            const int64_t cost = rounds * (4 * (sr / 4 + 2) + 2 * D2 + 4);   // (fill phases cost about a quarter of a working one)
            if (best < 0 || cost < best) { best = cost; a.seg_rows = sr; a.nseg = ns; }
        }
    }
    // P1: every LL1 group must have been written in an earlier phase than the level-1 stagers read it
    const int HG = a.H / 4;
    auto wphase = [&](const typename K::Geo& s, int g) { return g - s.G_lo + 2 * D2 + 1; };
    int P1 = 0;
    for (int sg = 0; sg < a.nseg; ++sg) {
        const typename K::Geo s = K::geometry(a, 0, sg);
        for (int h = 0; h < K::real_n1(s.r_lo, s.r_hi); ++h) {
            const int need = wphase(s, K::group_of(s.ge_first + h, HG)) + 1 - h;
            if (need > P1) P1 = need;
        }
    }
    a.P1 = P1;
    // ... and must still be there at its last read: the ring holds NG groups
    for (int sg = 0; sg < a.nseg; ++sg) {
        const typename K::Geo s = K::geometry(a, 0, sg);
        for (int h = 0; h < K::real_n1(s.r_lo, s.r_hi); ++h) {
            const int g = K::group_of(s.ge_first + h, HG);
            if (g < s.G_lo || g > s.G_hi) return WL_ERR_UNSUPPORTED;
            if (g + NG <= s.G_hi && a.P1 + h >= wphase(s, g + NG)) return WL_ERR_UNSUPPORTED;
        }
    }
    a.nblocks = a.NC * a.nstrips * a.nseg;
    return wl_launch<K>(a, a.nblocks, (size_t)a.lds_bytes, stream);
}

template <typename T>
static int wl_dtinv21_any(WlDtInv21Args<T>& a, int L0, int L1, int LQ, int policy, void* stream) {
    const int SZ = (int)sizeof(T);
    const int64_t planes = a.NC;
    const int H = a.H, W = a.W;
    if ((H % 4) || (W % 4) || H < 32 || W < 32 || (int64_t)H * W >= (1LL << 28)) return WL_ERR_UNSUPPORTED;
    // 8-byte loads of ll2 pixel pairs and (re, im) pairs, 8-byte stores of y
    if ((uintptr_t)a.ll2 % (2 * SZ) || (uintptr_t)a.highs2 % (2 * SZ) || (uintptr_t)a.highs1 % (2 * SZ) || (uintptr_t)a.y % (2 * SZ) ||
        (a.ll2_rs & 1) || (a.ll2_ps & 1)) return WL_ERR_UNSUPPORTED;
    // small work: per-level kernels (224-column planes only in numbers: 256x3x224^2 J = 2 inverse 0.246 -> 0.227 ms, 128x3x224^2 0.117 -> 0.129)
    if (!policy && (planes * (int64_t)wl_cdiv(H, 64) < wl_num_cus() || (W < 256 && !(W >= 224 && planes >= 3 * (int64_t)wl_num_cus())))) return WL_ERR_UNSUPPORTED;
    if (LQ != 10) return WL_ERR_UNSUPPORTED;                                                       // qshift_a, qshift_06
    if (L0 == 7 && L1 == 5) return wl_dtinv21_launch<T, 7, 5, 10>(a, stream);                      // near_sym_a
    if (L0 == 5 && L1 == 7) return wl_dtinv21_launch<T, 5, 7, 10>(a, stream);                      // backward of the near_sym_a forward
    return WL_ERR_UNSUPPORTED;
}

extern "C" int wl_dtcwt_inv_level21(const void* ll2, int64_t ll2_plane_stride, int ll2_row_stride, const void* highs2,
                                    const void* highs1, void* y, int dtype, int64_t planes, int H, int W, const void* g0o,
                                    int L0, const void* g1o, int L1, const void* g0a, const void* g0b, const void* g1a,
                                    const void* g1b, int LQ, int mode, int policy, void* stream) {
    if (planes < 0 || H < 1 || W < 1) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || LQ < 2 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS || LQ > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (ll2_row_stride < W / 2 || ll2_plane_stride < 0) return WL_ERR_SHAPE;
    if (policy < 0 || policy > 1 || !ll2 || !highs2 || !highs1) return WL_ERR_UNSUPPORTED;
    if (mode != 1) return WL_ERR_UNSUPPORTED;                   // symmetric (level 1 of the other modes pads with zeros: per-level kernels)
    if (planes == 0) return 0;
    if (wl_streaming_off()) return WL_ERR_UNSUPPORTED;
    WL_DISPATCH_FLOAT(dtype, {
        WlDtInv21Args<T> a = wl_dtinv21_args<T>(ll2, ll2_plane_stride, ll2_row_stride, highs2, highs1, y, planes, H, W, g0o, g1o,
                                                g0a, g0b, g1a, g1b);
        return wl_dtinv21_any(a, L0, L1, LQ, policy, stream);
    });
}
