// The depth axis of the 3-D DWT: one analysis / synthesis level along the MIDDLE axis of (outer, n, inner) data, streamed.
//
// The H and W axes of a volume go through the 2-D engine (the N*C*D planes of an (N,C,D,H,W) tensor are planes like any other);
// what is left is a two-channel bank along D, where neighbouring samples of a signal lie a whole plane apart.  These kernels
// march along that axis instead of gathering across it:
//
//   * a thread owns VEC contiguous `inner` elements (16 bytes when VEC > 1: 4 floats, 8 halves - 4 halves from 14 taps on, where
//     the wider body would spill) and one CHUNK of output indices;
//   * it keeps a sliding window of input planes in registers (analysis: LT planes, synthesis: LT/2 planes of lo and of hi),
//     loads per step what slides in (analysis: two planes; synthesis: one of each) and emits one lo + one hi plane (analysis) or
//     two output planes (synthesis), accumulated in fp32;
//   * the window is a ring of one step more than it needs, so that the loads of step k+1 are issued before the arithmetic of
//     step k; the ring slots are compile-time (the step loop is unrolled over one turn of the ring): no register is moved;
//   * the depth index is wave-uniform (it comes from the block index alone), so the boundary extension - wl_ext, the closed
//     forms every kernel here uses - is scalar arithmetic, and a plane that the extension maps to zero is not loaded;
//   * every input plane is read from HBM once per chunk, plus LT - 2 (synthesis: LT/2 - 1 per band) halo planes where two
//     chunks meet; no LDS, no barriers.
//
// Up to four sources per launch, each with its own base pointer, outer stride and axis stride, and the same for each output:
// the analysis reads the 2-D engine's dense ll (P,H',W') and highs (P,3,H',W') and writes the final (N,C,7,D',H',W') /
// (N,C,D',H',W') tensors, the synthesis reads those and writes the dense buffers the 2-D synthesis wants.  The `inner` elements
// of a plane are contiguous.  VEC = 1 is the same body for data whose inner size, strides or bases are no 16-byte multiples.
//
//   analysis:   lo[k], hi[k] = sum_{j<LT} h0[j], h1[j] * ext(x, 2k + base + j)          (ops.afb1d; taps stored reversed)
//   synthesis:  y[p] = sum_{t<LT, t = m mod 2} g0[t] lo[(m-t)/2] + g1[t] hi[(m-t)/2],   m = p + LT - 2, samples outside [0,K) zero
//               periodization: m = p + LT/2 - 1 and the coefficient index wraps modulo K - the reference's fold of the wrapped
//               tail (wl_filt1d.h) whenever that tail is no longer than the signal (2K >= LT - 2; the launcher declines the rest)
// The sum of an output runs over the taps in the same order whatever chunk it falls into, every term an explicit fused
// multiply-add: a result does not depend on the cut.  (With `a += h * v` the compiler is free to contract a term or not, and it
// chose differently in different phases of the unrolled ring - packed multiplies and separate adds in some, fused multiply-adds
// in others -, so an output's last bit depended on the phase, that is on the chunk, it fell into: DESIGN.md 4.25.)
#pragma once
#include "wl_common.h"

#define WL_DEPTH_MAX_SRC 4

template <typename T, int VEC>
struct __attribute__((may_alias)) alignas(sizeof(T) * VEC) WlPack { T e[VEC]; };

// Waves per SIMD the compiler has to leave room for (its register budget is 512 / that): without a bound it spends registers on
// lookahead - 246 for the 20-tap float kernel whose ring is 88.  Rings of up to 64 registers: 4 waves (128 registers); up to 96:
// 3 (168); beyond (12 taps of 2-byte data in 16-byte pieces): 2.  (2-byte data of 14 taps and more takes VEC = 4.)
template <typename T, int LT, int VEC>
struct WlDepthWaves {
    static const int ring = (LT + 2) * VEC;    // registers of the ring as fp32 (the compiler converts 2-byte planes once, at the load)
    static const int value = VEC == 1 ? 4 : ring <= 64 ? 4 : ring <= 96 ? 3 : 2;
};

template <typename X> WL_DEV X wl_pick4(const X* v, unsigned s) {   // (selects: a run-time index into kernel arguments costs scratch)
    X r = v[0];
    if (s == 1) r = v[1];
    if (s == 2) r = v[2];
    if (s == 3) r = v[3];
    return r;
}

// plane `p` (-1: zeros) of a source: base + p * axis stride, this thread's VEC elements
template <typename T, int VEC>
WL_DEV WlPack<T, VEC> wl_depth_load(const T* base, int64_t as, int64_t i0, int p) {
    typedef WlPack<T, VEC> V;
    V v = *reinterpret_cast<const V*>(base + (int64_t)(p < 0 ? 0 : p) * as + i0);
    if (p < 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v.e[e] = (T)0.f;
    }
    return v;
}

template <typename T>
struct WlAfbDepthArgs {
    const T* src[WL_DEPTH_MAX_SRC]; int64_t src_os[WL_DEPTH_MAX_SRC], src_as[WL_DEPTH_MAX_SRC];
    T* lo[WL_DEPTH_MAX_SRC]; int64_t lo_os[WL_DEPTH_MAX_SRC], lo_as[WL_DEPTH_MAX_SRC];
    T* hi[WL_DEPTH_MAX_SRC]; int64_t hi_os[WL_DEPTH_MAX_SRC], hi_as[WL_DEPTH_MAX_SRC];
    const float* h0; const float* h1;
    int64_t inner;
    unsigned tiles, chunks, nsrc;      // the grid: (inner tiles) x chunks x sources x outer
    int chunk_len;                     // outputs per chunk
    int n, K, base, ext;
};

template <typename T, int LT, int VEC>
struct WlAfbDepth {
    typedef WlAfbDepthArgs<T> Args;
    typedef WlPack<T, VEC> V;
    static const int kThreads = 256;
    static const int kMinWaves = WlDepthWaves<T, LT, VEC>::value;
    static const int R = LT + 2;       // ring slots: the window and the two planes of the next step
    static const int PH = R / 2;       // steps per turn of the ring
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        unsigned b = (unsigned)ctx.bid;
        const unsigned it = b % a.tiles; b /= a.tiles;
        const unsigned c = b % a.chunks; b /= a.chunks;
        const unsigned s = b % a.nsrc;
        const int64_t o = b / a.nsrc;
        const int64_t i0 = ((int64_t)it * kThreads + ctx.tid) * VEC;
        if (i0 >= a.inner) return;
        const int k0 = (int)c * a.chunk_len;
        const int k1 = k0 + a.chunk_len < a.K ? k0 + a.chunk_len : a.K;
        const int64_t xas = wl_pick4(a.src_as, s), las = wl_pick4(a.lo_as, s), has = wl_pick4(a.hi_as, s);
        const T* x = wl_pick4(a.src, s) + o * wl_pick4(a.src_os, s);
        T* lo = wl_pick4(a.lo, s) + o * wl_pick4(a.lo_os, s);
        T* hi = wl_pick4(a.hi, s) + o * wl_pick4(a.hi_os, s);
        const int n = a.n, ext = a.ext;
        float h0[LT], h1[LT];
#pragma unroll
        for (int j = 0; j < LT; ++j) { h0[j] = a.h0[j]; h1[j] = a.h1[j]; }
        V win[R];
        const int q0 = 2 * k0 + a.base;                    // extended position of ring slot 0
#pragma unroll
        for (int j = 0; j < LT; ++j) win[j] = wl_depth_load<T, VEC>(x, xas, i0, wl_ext(q0 + j, n, ext));
        for (int k = k0; k < k1; k += PH) turn<0>(win, h0, h1, x, xas, lo, las, hi, has, i0, k, k0, k1, q0, n, ext);
    }
    // the steps k + PHASE .. of one turn of the ring: the ring slots are compile-time constants
    template <int PHASE>
    static WL_DEV void turn(V (&win)[R], const float (&h0)[LT], const float (&h1)[LT], const T* x, int64_t xas, T* lo, int64_t las, T* hi, int64_t has,
                            int64_t i0, int k, int k0, int k1, int q0, int n, int ext) {
        if constexpr (PHASE < PH) {
            const int kk = k + PHASE;
            if (kk >= k1) return;
            if (kk + 1 < k1) {                             // what slides in for the next step
                const int q = q0 + 2 * (kk - k0) + LT;
                win[(2 * PHASE + LT) % R] = wl_depth_load<T, VEC>(x, xas, i0, wl_ext(q, n, ext));
                win[(2 * PHASE + LT + 1) % R] = wl_depth_load<T, VEC>(x, xas, i0, wl_ext(q + 1, n, ext));
            }
            // (one accumulator per band and element, not a packed pair: the pair form keeps every window value twice)
            float alo[VEC], ahi[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) { alo[e] = 0.f; ahi[e] = 0.f; }
#pragma unroll
            for (int j = 0; j < LT; ++j) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float v = (float)win[(2 * PHASE + j) % R].e[e];
                    alo[e] = __builtin_fmaf(h0[j], v, alo[e]);
                    ahi[e] = __builtin_fmaf(h1[j], v, ahi[e]);
                }
            }
            V ylo, yhi;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { ylo.e[e] = (T)alo[e]; yhi.e[e] = (T)ahi[e]; }
            *reinterpret_cast<V*>(lo + (int64_t)kk * las + i0) = ylo;
            *reinterpret_cast<V*>(hi + (int64_t)kk * has + i0) = yhi;
            turn<PHASE + 1>(win, h0, h1, x, xas, lo, las, hi, has, i0, k, k0, k1, q0, n, ext);
        }
    }
};

template <typename T>
struct WlSfbDepthArgs {
    const T* lo[WL_DEPTH_MAX_SRC]; int64_t lo_os[WL_DEPTH_MAX_SRC], lo_as[WL_DEPTH_MAX_SRC];
    const T* hi[WL_DEPTH_MAX_SRC]; int64_t hi_os[WL_DEPTH_MAX_SRC], hi_as[WL_DEPTH_MAX_SRC];   // hi[s] may be nullptr: zeros
    T* y[WL_DEPTH_MAX_SRC]; int64_t y_os[WL_DEPTH_MAX_SRC], y_as[WL_DEPTH_MAX_SRC];
    const float* g0; const float* g1;
    int64_t inner;
    unsigned tiles, chunks, nsrc;
    int chunk_len;                     // steps (output pairs) per chunk
    int K, ny, shift, ext;             // y[p] = full[p + shift]; ext: WL_EXT_ZERO (crop) or WL_EXT_PERIODIC (periodization)
    int q_first, nq;                   // step q makes full[2q], full[2q + 1]; q_first .. q_first + nq - 1 cover the outputs
};

template <typename T, int LT, int VEC>
struct WlSfbDepth {
    typedef WlSfbDepthArgs<T> Args;
    typedef WlPack<T, VEC> V;
    static const int kThreads = 256;
    static const int kMinWaves = WlDepthWaves<T, LT, VEC>::value;
    static const int HT = LT / 2;      // coefficients under the filter
    static const int R = HT + 1;       // ring slots per band: the window and the plane of the next step
    static WL_DEV void run(const Args& a, const WlCtx& ctx) {
        unsigned b = (unsigned)ctx.bid;
        const unsigned it = b % a.tiles; b /= a.tiles;
        const unsigned c = b % a.chunks; b /= a.chunks;
        const unsigned s = b % a.nsrc;
        const int64_t o = b / a.nsrc;
        const int64_t i0 = ((int64_t)it * kThreads + ctx.tid) * VEC;
        if (i0 >= a.inner) return;
        const int s0 = (int)c * a.chunk_len;
        const int s1 = s0 + a.chunk_len < a.nq ? s0 + a.chunk_len : a.nq;
        const int64_t las = wl_pick4(a.lo_as, s), has = wl_pick4(a.hi_as, s), yas = wl_pick4(a.y_as, s);
        const T* lo = wl_pick4(a.lo, s) + o * wl_pick4(a.lo_os, s);
        const T* hp = wl_pick4(a.hi, s);
        const bool has_hi = hp != nullptr;
        const T* hi = has_hi ? hp + o * wl_pick4(a.hi_os, s) : lo;
        T* y = wl_pick4(a.y, s) + o * wl_pick4(a.y_os, s);
        const int K = a.K, ext = a.ext, ny = a.ny;
        float g0[LT], g1[LT];
#pragma unroll
        for (int t = 0; t < LT; ++t) { g0[t] = a.g0[t]; g1[t] = a.g1[t]; }
        V wl[R], wh[R];
        const int kb = a.q_first + s0 - HT + 1;            // coefficient index of ring slot 0
#pragma unroll
        for (int u = 0; u < HT; ++u) {
            const int p = wl_ext(kb + u, K, ext);
            wl[u] = wl_depth_load<T, VEC>(lo, las, i0, p);
            wh[u] = wl_depth_load<T, VEC>(hi, has, i0, has_hi ? p : -1);
        }
        for (int st = s0; st < s1; st += R)
            turn<0>(wl, wh, g0, g1, lo, las, hi, has, has_hi, y, yas, i0, st, s0, s1, kb, a.q_first, a.shift, K, ny, ext);
    }
    template <int PHASE>
    static WL_DEV void turn(V (&wl)[R], V (&wh)[R], const float (&g0)[LT], const float (&g1)[LT], const T* lo, int64_t las,
                            const T* hi, int64_t has, bool has_hi, T* y, int64_t yas, int64_t i0, int st, int s0, int s1, int kb,
                            int q_first, int shift, int K, int ny, int ext) {
        if constexpr (PHASE < R) {
            const int sq = st + PHASE;
            if (sq >= s1) return;
            if (sq + 1 < s1) {                             // what slides in for the next step
                const int p = wl_ext(kb + (sq - s0) + HT, K, ext);
                wl[(PHASE + HT) % R] = wl_depth_load<T, VEC>(lo, las, i0, p);
                wh[(PHASE + HT) % R] = wl_depth_load<T, VEC>(hi, has, i0, has_hi ? p : -1);
            }
            float ae[VEC], ao[VEC];                        // full[2q], full[2q + 1]
#pragma unroll
            for (int e = 0; e < VEC; ++e) { ae[e] = 0.f; ao[e] = 0.f; }
#pragma unroll
            for (int u = 0; u < HT; ++u) {                 // taps 2u, 2u + 1 meet coefficient q - u
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float vl = (float)wl[(PHASE + HT - 1 - u) % R].e[e];
                    const float vh = (float)wh[(PHASE + HT - 1 - u) % R].e[e];
                    ae[e] = __builtin_fmaf(g0[2 * u], vl, ae[e]);
                    ae[e] = __builtin_fmaf(g1[2 * u], vh, ae[e]);
                    ao[e] = __builtin_fmaf(g0[2 * u + 1], vl, ao[e]);
                    ao[e] = __builtin_fmaf(g1[2 * u + 1], vh, ao[e]);
                }
            }
            const int p0 = 2 * (q_first + sq) - shift;     // output index of full[2q]
            V ye, yo;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { ye.e[e] = (T)ae[e]; yo.e[e] = (T)ao[e]; }
            if (p0 >= 0 && p0 < ny) *reinterpret_cast<V*>(y + (int64_t)p0 * yas + i0) = ye;
            if (p0 + 1 >= 0 && p0 + 1 < ny) *reinterpret_cast<V*>(y + (int64_t)(p0 + 1) * yas + i0) = yo;
            turn<PHASE + 1>(wl, wh, g0, g1, lo, las, hi, has, has_hi, y, yas, i0, st, s0, s1, kb, q_first, shift, K, ny, ext);
        }
    }
};
