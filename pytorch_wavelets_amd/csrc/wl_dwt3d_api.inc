// ---- the depth axis of the 3-D DWT (wl_dwt3d.h): included by wl_api.inc ----------------------------------------------
// Depth chunks of a launch: the fewest that give every CU work - WL_DEPTH_WG_PER_CU workgroups per compute unit before the
// depth axis is cut at all (a guess: nobody has measured this threshold), never chunks shorter than the filter's halo (a cut
// re-reads LT - 2 planes), `forced` > 0 as the caller says.  Returns the chunk length; *chunks = how many there are.
#ifndef WL_DEPTH_WG_PER_CU
#define WL_DEPTH_WG_PER_CU 4
#endif
static int wl_depth_chunks(int64_t blocks, int steps, int min_len, int forced, unsigned* chunks) {
    int64_t c = 1;
    if (forced > 0) c = forced;
    else {
        const int64_t want = (int64_t)WL_DEPTH_WG_PER_CU * wl_num_cus();
        if (blocks < want) c = wl_cdiv64(want, blocks);
        const int most = steps / (min_len < 1 ? 1 : min_len);
        if (c > most) c = most;
    }
    if (c > steps) c = steps;
    if (c < 1) c = 1;
    const int len = wl_cdiv(steps, (int)c);
    *chunks = (unsigned)wl_cdiv(steps, len);               // (no empty chunk)
    return len;
}

// elements per access of the vector body: 16 bytes, but 8 for 2-byte data under 14 taps and more (a ring of 16-byte pieces, which
// the compiler also keeps converted to fp32, does not fit the registers: profiles/dwt3d_kernel_regs.txt)
template <typename T, int LT> struct WlDepthVec { static const int value = sizeof(T) == 2 ? (LT >= 14 ? 4 : 8) : 4; };
static int wl_depth_vec_of(size_t elem, int L) { return elem == 2 ? (L >= 14 ? 4 : 8) : 4; }

static bool wl_depth_vec_ok(const void* const* p, const int64_t* os, const int64_t* as, int nsrc, int vec, size_t elem) {
    for (int s = 0; s < nsrc; ++s) {
        if (!p[s]) continue;
        if ((uintptr_t)p[s] % (vec * elem) || os[s] % vec || as[s] % vec) return false;
    }
    return true;
}

template <typename T, int LT, int VEC>
static int wl_afb_depth_launch(WlAfbDepthArgs<T>& a, int64_t outer, int forced, void* stream) {
    typedef WlAfbDepth<T, LT, VEC> K;
    const int64_t tiles = wl_cdiv64(a.inner, (int64_t)K::kThreads * VEC);
    a.tiles = (unsigned)tiles;
    a.chunk_len = wl_depth_chunks(tiles * outer * a.nsrc, a.K, LT / 2, forced, &a.chunks);
    const int64_t grid = tiles * outer * a.nsrc * a.chunks;
    if (grid > 2147483647LL) return WL_ERR_UNSUPPORTED;    // (the block index is taken apart in 32 bits)
    return wl_launch<K>(a, grid, 0, stream);
}

template <typename T, int LT>
static int wl_afb_depth_vec(WlAfbDepthArgs<T>& a, int64_t outer, int forced, bool vec, void* stream) {
    const int VEC = WlDepthVec<T, LT>::value;
    return vec ? wl_afb_depth_launch<T, LT, VEC>(a, outer, forced, stream) : wl_afb_depth_launch<T, LT, 1>(a, outer, forced, stream);
}

template <typename T, int LT, int VEC>
static int wl_sfb_depth_launch(WlSfbDepthArgs<T>& a, int64_t outer, int forced, void* stream) {
    typedef WlSfbDepth<T, LT, VEC> K;
    const int64_t tiles = wl_cdiv64(a.inner, (int64_t)K::kThreads * VEC);
    a.tiles = (unsigned)tiles;
    a.chunk_len = wl_depth_chunks(tiles * outer * a.nsrc, a.nq, LT / 2, forced, &a.chunks);
    const int64_t grid = tiles * outer * a.nsrc * a.chunks;
    if (grid > 2147483647LL) return WL_ERR_UNSUPPORTED;
    return wl_launch<K>(a, grid, 0, stream);
}

template <typename T, int LT>
static int wl_sfb_depth_vec(WlSfbDepthArgs<T>& a, int64_t outer, int forced, bool vec, void* stream) {
    const int VEC = WlDepthVec<T, LT>::value;
    return vec ? wl_sfb_depth_launch<T, LT, VEC>(a, outer, forced, stream) : wl_sfb_depth_launch<T, LT, 1>(a, outer, forced, stream);
}

#define WL_DEPTH_CASES(FN, ...)                                                                                        \
    switch (L) {                                                                                                       \
        case 2: return FN<T, 2>(__VA_ARGS__);   case 4: return FN<T, 4>(__VA_ARGS__);   case 6: return FN<T, 6>(__VA_ARGS__);   \
        case 8: return FN<T, 8>(__VA_ARGS__);   case 10: return FN<T, 10>(__VA_ARGS__); case 12: return FN<T, 12>(__VA_ARGS__); \
        case 14: return FN<T, 14>(__VA_ARGS__); case 16: return FN<T, 16>(__VA_ARGS__); case 18: return FN<T, 18>(__VA_ARGS__); \
        case 20: return FN<T, 20>(__VA_ARGS__); default: return WL_ERR_UNSUPPORTED;                                    \
    }

static int wl_depth_check(int nsrc, int64_t outer, int n, int64_t inner, int L0, int L1, int mode) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (nsrc < 1 || nsrc > WL_DEPTH_MAX_SRC || outer < 0 || n < 1 || inner < 1) return WL_ERR_SHAPE;
    if (L0 < 1 || L1 < 1 || L0 > WL_MAX_TAPS || L1 > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (L0 != L1 || (L0 & 1) || L0 > 20) return WL_ERR_UNSUPPORTED;
    // the kernels hold positions along the axis in 32 bits and a thread's offset into a plane in 31
    if (n >= (1 << 29) || inner >= (1LL << 29)) return WL_ERR_UNSUPPORTED;
    return 0;
}

extern "C" int wl_dwt3d_depth_analysis(const void* const* src, const int64_t* src_outer_stride, const int64_t* src_axis_stride,
                                       void* const* lo, const int64_t* lo_outer_stride, const int64_t* lo_axis_stride,
                                       void* const* hi, const int64_t* hi_outer_stride, const int64_t* hi_axis_stride, int nsrc,
                                       int dtype, int64_t outer, int n, int64_t inner, const void* h0, int L0, const void* h1,
                                       int L1, int mode, int chunks, void* stream) {
    const int rc = wl_depth_check(nsrc, outer, n, inner, L0, L1, mode);
    if (rc != 0) return rc;
    if (chunks < 0) return WL_ERR_SHAPE;
    for (int s = 0; s < nsrc; ++s) {
        if (!src[s] || !lo[s] || !hi[s]) return WL_ERR_SHAPE;
        if (src_outer_stride[s] < 0 || src_axis_stride[s] < 0 || lo_outer_stride[s] < 0 || hi_outer_stride[s] < 0 ||
            lo_axis_stride[s] < inner || hi_axis_stride[s] < inner)
            return WL_ERR_SHAPE;
    }
    const int L = L0;
    if (mode == 2 && n + (n & 1) < L - 1) return WL_ERR_UNSUPPORTED;   // the reference's single fold (wl_filt1d.h, WL_EXT_PER_FOLD1)
    if (wl_options().generic_only) return WL_ERR_UNSUPPORTED;
    if (outer == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlAfbDepthArgs<T> a;
        memset(&a, 0, sizeof(a));
        for (int s = 0; s < WL_DEPTH_MAX_SRC; ++s) {
            const int r = s < nsrc ? s : 0;                        // (unused slots repeat the first: the selects read them)
            a.src[s] = (const T*)src[r]; a.src_os[s] = src_outer_stride[r]; a.src_as[s] = src_axis_stride[r];
            a.lo[s] = (T*)lo[r]; a.lo_os[s] = lo_outer_stride[r]; a.lo_as[s] = lo_axis_stride[r];
            a.hi[s] = (T*)hi[r]; a.hi_os[s] = hi_outer_stride[r]; a.hi_as[s] = hi_axis_stride[r];
        }
        a.h0 = (const float*)h0; a.h1 = (const float*)h1;
        a.inner = inner; a.nsrc = (unsigned)nsrc;
        a.n = n; a.K = wl_coeff_len(n, L, mode); a.base = wl_afb_base(n, L, mode); a.ext = wl_mode_to_ext(mode);
        const int VEC = wl_depth_vec_of(sizeof(T), L);
        const bool vec = inner % VEC == 0 && wl_depth_vec_ok(src, src_outer_stride, src_axis_stride, nsrc, VEC, sizeof(T)) &&
                         wl_depth_vec_ok((const void* const*)lo, lo_outer_stride, lo_axis_stride, nsrc, VEC, sizeof(T)) &&
                         wl_depth_vec_ok((const void* const*)hi, hi_outer_stride, hi_axis_stride, nsrc, VEC, sizeof(T));
        WL_DEPTH_CASES(wl_afb_depth_vec, a, outer, chunks, vec, stream);
    });
}

extern "C" int wl_dwt3d_depth_synthesis(const void* const* lo, const int64_t* lo_outer_stride, const int64_t* lo_axis_stride,
                                        const void* const* hi, const int64_t* hi_outer_stride, const int64_t* hi_axis_stride,
                                        void* const* y, const int64_t* y_outer_stride, const int64_t* y_axis_stride, int nsrc,
                                        int dtype, int64_t outer, int K, int64_t inner, int ny, const void* g0, int L0,
                                        const void* g1, int L1, int mode, int chunks, void* stream) {
    const int rc = wl_depth_check(nsrc, outer, K, inner, L0, L1, mode);
    if (rc != 0) return rc;
    const int L = L0;
    const int full = mode == 2 ? 2 * K : 2 * K - L + 2;
    if (ny < 1 || ny > full || chunks < 0) return WL_ERR_SHAPE;
    for (int s = 0; s < nsrc; ++s) {
        if (!lo[s] || !y[s]) return WL_ERR_SHAPE;
        if (lo_outer_stride[s] < 0 || lo_axis_stride[s] < 0 || y_outer_stride[s] < 0 || y_axis_stride[s] < inner ||
            (hi[s] && (hi_outer_stride[s] < 0 || hi_axis_stride[s] < 0)))
            return WL_ERR_SHAPE;
    }
    if (mode == 2 && 2 * K < L - 2) return WL_ERR_UNSUPPORTED;        // more taps than outputs: the reference's single fold
    if (wl_options().generic_only) return WL_ERR_UNSUPPORTED;
    if (outer == 0) return 0;
    WL_DISPATCH_FLOAT(dtype, {
        WlSfbDepthArgs<T> a;
        memset(&a, 0, sizeof(a));
        for (int s = 0; s < WL_DEPTH_MAX_SRC; ++s) {
            const int r = s < nsrc ? s : 0;
            a.lo[s] = (const T*)lo[r]; a.lo_os[s] = lo_outer_stride[r]; a.lo_as[s] = lo_axis_stride[r];
            a.hi[s] = (const T*)hi[r]; a.hi_os[s] = hi[r] ? hi_outer_stride[r] : 0; a.hi_as[s] = hi[r] ? hi_axis_stride[r] : 0;
            a.y[s] = (T*)y[r]; a.y_os[s] = y_outer_stride[r]; a.y_as[s] = y_axis_stride[r];
        }
        a.g0 = (const float*)g0; a.g1 = (const float*)g1;
        a.inner = inner; a.nsrc = (unsigned)nsrc;
        a.K = K; a.ny = ny;
        a.shift = mode == 2 ? L / 2 - 1 : L - 2;
        a.ext = mode == 2 ? WL_EXT_PERIODIC : WL_EXT_ZERO;
        a.q_first = a.shift / 2;
        a.nq = (ny - 1 + a.shift) / 2 - a.q_first + 1;
        const int VEC = wl_depth_vec_of(sizeof(T), L);
        const bool vec = inner % VEC == 0 && wl_depth_vec_ok(lo, lo_outer_stride, lo_axis_stride, nsrc, VEC, sizeof(T)) &&
                         wl_depth_vec_ok(hi, hi_outer_stride, hi_axis_stride, nsrc, VEC, sizeof(T)) &&
                         wl_depth_vec_ok((const void* const*)y, y_outer_stride, y_axis_stride, nsrc, VEC, sizeof(T));
        WL_DEPTH_CASES(wl_sfb_depth_vec, a, outer, chunks, vec, stream);
    });
}
#undef WL_DEPTH_CASES
