// C ABI of the two streaming multi-level kernels (analysis: wl_dwt_rows.h, synthesis: wl_idwt_rows.h).  Their own
// translation unit in the HIP build (wl_rows_hip.hip, compiled with -fno-slp-vectorize: the packed FMAs are written
// out by hand with their operand selects, and the SLP vectoriser would re-pack the rest into register shuffles);
// included after the backend header, which provides wl_launch<K>() and wl_num_cus().  Round 6: TWO translation units (wl_rows_hip.hip defines
// WL_ROWS_UNIT_ANALYSIS, wl_irows_hip.hip WL_ROWS_UNIT_SYNTHESIS: the halves compile side by side; with neither macro the file is whole).
#include "wl_api_common.h"
#include "wl_dwt_rows.h"

// Narrow planes, too few of them for the packing rule of the fused kernels ("no more planes per workgroup than leaves a workgroup
// for every CU") to pack at all: pack AND cut.  A workgroup's time is the rows it walks - its cadence does not depend on how many of
// its waves have columns (§4.6 of DESIGN.md) - so 384 planes of 224 x 224 as 384 + 384 half planes in two rounds, or as 256 whole + 256 half
// planes in one, take a whole plane's time; as 128 workgroups x 2 halves of THREE planes they take half of it.  Returns the planes
// per workgroup (> 1) when packing `pp_cap` or fewer planes and cutting every unit in two beats `cost_now` (rounds x rows of the
// launcher's own choice) by a tenth, else 0.  `max_wgs`: the analysis kernel only with at most ONE such workgroup per CU (its waves
// are bound by what a SIMD issues: 128x3x256^2 as 384 workgroups of two half planes ran 0.045 ms against 0.041, 128x3x224^2 as 256
// of three 0.029 against 0.035; three levels with 384 workgroups 0.049 against 0.045), the synthesis kernel two (128x3x224^2 J = 2 as
// 384 workgroups 0.064 against 0.080 ms; J = 1 as 256: 0.030 against 0.064): tools/gpu_r5w.py, same box.
static int wl_rows_pack_and_cut(int64_t planes, int pp_cap, int lds_plane, int rows, int halo, int64_t cost_now, int64_t max_wgs) {
    const int64_t cus = wl_num_cus(), slots = 2 * cus;
    int p2 = pp_cap < planes ? pp_cap : (int)planes;
    // (workgroups for three quarters of the CUs at least: half planes of a packed unit still beat whole planes on every CU)
    while (p2 > 1 && (p2 * lds_plane > 80 * 1024 || 8 * ((planes + p2 - 1) / p2) < 3 * cus)) --p2;
    if (p2 <= 1) return 0;
    const int64_t wgs = 2 * ((planes + p2 - 1) / p2);
    if (wgs > max_wgs) return 0;
    const int64_t cost = ((wgs + slots - 1) / slots) * (rows / 2 + halo + 8);
    return cost * 10 < cost_now * 9 ? p2 : 0;
}

#if !defined(WL_ROWS_UNIT_SYNTHESIS)
// ---- fused multi-level streaming analysis (wl_dwt_rows.h) -------------------------------------------
// Simulate the schedule of one segment (feeds [f0, fend) per level) exactly as the waves will follow it: fills
// sg.sched / sg.nhb and reports how many rows of each LL ring are ever in use at once (need[j]: the source ring of level j - the ring is
// overrun if it has fewer rows).
template <typename T>
static int wl_rows_plan_segment(const WlRowsArgs<T>& a, WlRowsSeg& sg, int LT, int* need) {
    const int nlev = a.nlev;
    WlRowsSched sc;
    sc.init(sg);
    for (int j = 0; j < WL_ROWS_MAXLEV; ++j) need[j] = 0;
    int nhb = 0;
    for (;; ++nhb) {
        int nn[WL_ROWS_MAXLEV], todo = 0;
        for (int j = 0; j < nlev; ++j) { nn[j] = sc.feeds_now(a, sg, j, LT); todo += sg.fend[j] - sc.fed[j]; }
        if (todo == 0) break;
        if (nhb >= WL_ROWS_MAXHB) return WL_ERR_UNSUPPORTED;   // taller than the schedule table (or not draining)
        if ((nhb & 3) == 0) sg.sched[nhb >> 2] = 0;
        int any = 0;
        for (int j = 0; j < nlev; ++j) { sg.sched[nhb >> 2] |= (unsigned)nn[j] << (8 * (nhb & 3) + 2 * j); any += nn[j]; }
        if (!any) return WL_ERR_UNSUPPORTED;                   // a level waits for rows nobody will produce
        for (int j = 0; j + 1 < nlev; ++j) {
            // rows level j writes into the ring of level j+1 in this half-batch must not evict a row that level j+1
            // still has to read (now or later): its oldest outstanding source row
            const int wr_hi = sc.avail(sg, j, LT) + nn[j];   // one past the newest row written (upper bound)
            const int e_next = a.base + 2 * sc.fed[j + 1];
            const int e_last = a.base + 2 * sg.fend[j + 1] - 1;
            int oldest = a.g[j + 1].Hs;
            if (a.ext == WL_EXT_PER) oldest = e_next <= e_last ? e_next : 0x3fffffff;   // (unfolded row numbers: monotone)
            else if (e_next <= e_last) {
                // the source row index is monotone in e except at the two folds: check both ends and the folds
                const int cand[4] = {e_next, e_last, e_next < 0 ? -1 : e_next, e_next < 0 ? 0 : e_next};
                for (int c = 0; c < 4; ++c) {
                    if (cand[c] < e_next || cand[c] > e_last) continue;
                    const int r = wl_ext1(cand[c], a.g[j + 1].Hs, a.ext);
                    if (r >= 0 && r < oldest) oldest = r;
                }
            }
            if (wr_hi - oldest > need[j + 1]) need[j + 1] = wr_hi - oldest;
        }
        for (int j = 0; j < nlev; ++j) sc.fed[j] += nn[j];
    }
    sg.nhb = nhb;
    return 0;
}

// Geometry, LDS layout and wave roles of the streaming kernel, the segments the planes are processed in, and a host
// simulation of each segment's schedule.  strips: 0 = cut as many planes in two as it takes to fill whole rounds of
// the chip, 1 = whole planes only, 2 = cut every plane (tests).
// (host emulation only: WL_EMU_TRACE=1 in the environment names the check of wl_afb_rows_launch that declined a configuration)
#if defined(__HIPCC__)
#define WL_DECLINE(n) WL_ERR_UNSUPPORTED
#else
#include <stdio.h>
static int wl_decline_trace(int n, int line) {
    if (getenv("WL_EMU_TRACE")) fprintf(stderr, "[wl] fused analysis declined at check %d (wl_rows_api.inc:%d)\n", n, line);
    return WL_ERR_UNSUPPORTED;
}
#define WL_DECLINE(n) wl_decline_trace(n, __LINE__)
#endif
template <typename T, int LT, int PPR, int SAME = 0, int LAT = 0, int ODD = 0, int NP2 = 0>
static int wl_afb_rows_launch(const WlAfbPyrReq& r, const float* lat, int guard = 0, int what = 0) {
    // what: 0 = launch, 1 = dry run (every check, no launch), 2 = launch as the armed fallback of a hinted launch
    // lat: device scratch with WlTapPrep's verdict (+ the column lattice for LAT = 1), or null (the guard compares the taps)
    typedef WlAfbRows<T, LT, PPR, WL_ROWS_DEPTH, SAME, LAT, ODD, NP2> K;
    const int WARM = (LT - 2) / 2;
    const int64_t planes = r.planes;
    const int H = r.H, W = r.W, nlev = r.nlev, mode = r.mode, strips = r.strips;
    WlRowsArgs<T> a;
    a.ext = wl_mode_to_ext(mode);
    const bool per = a.ext == WL_EXT_PER;
    if (nlev < 1 || nlev > WL_ROWS_MAXLEV) return WL_DECLINE(1);
    // several levels: zero / symmetric / reflect (single-fold rows above / below the plane) and, round 6, periodization (those rows
    // are computed: see WlRowsSched::src_row); `periodic` (mode 6: the wrap of an EXPANSIVE transform) stays level by level
    if (nlev > 1 && !(a.ext == WL_EXT_ZERO || a.ext == WL_EXT_SYM || a.ext == WL_EXT_REFL || per)) return WL_DECLINE(2);
    if ((int64_t)H * r.x_rs >= (1LL << 30) || r.x_rs < W) return WL_DECLINE(3);   // 32-bit in-plane offsets
    // level-1 rows arrive by 16-byte LDS-DMA pieces: every row starts on a 16-byte address (see WlAfbPyrReq for a ragged last piece)
    if ((r.x_rs * sizeof(T)) % 16 != 0 || (r.x_ps * sizeof(T)) % 16 != 0 || (uintptr_t)r.x % 16 != 0 || wl_cdiv(W * (int)sizeof(T), 1024) != PPR) return WL_DECLINE(4);
    if ((W * sizeof(T)) % 16 != 0 && wl_align_up(W * (int)sizeof(T), 16) > r.x_rs * (int)sizeof(T)) return WL_DECLINE(5);   // the last piece must lie inside the pitch
    a.base = wl_afb_base(W, LT, mode);   // the same for every level and both axes (depends on L and mode only)
    if ((a.base & 1) != ODD) return WL_DECLINE(6);   // periodization with L % 4 == 0: the samples sit on odd cells (the ODD instantiations)
    a.nlev = nlev;
    // geometry + wave counts
    int compute_waves = 0;
    {
        int h = H, w = W, wave = 0;
        for (int j = 0; j < nlev; ++j) {
            WlRowsLevel& g = a.g[j];
            g.Hs = h; g.Ws = w;
            // (a periodized level shorter than the filter is NOT a periodic convolution in the reference - its wrap-add folds once,
            // dwt/lowlevel.py:134-150: the direct kernels restate that corner, like the entry point's check of level 1)
            if (per && (h + (h & 1) < LT - 1 || w + (w & 1) < LT - 1)) return WL_DECLINE(7);
            g.Kh = wl_coeff_len(h, LT, mode); g.Kw = wl_coeff_len(w, LT, mode);
            g.nwaves = wl_cdiv(g.Kw, 64); wave += g.nwaves;
            // ring row = [left halo | w samples | right halo]: the cells the row filter reads beyond the samples
            g.hl = (a.base < 0 ? -a.base : 0) + ODD;                      // (ODD: the lanes read one cell earlier and one later)
            const int e_max = 2 * (g.Kw - 1) + a.base + LT - 1 + ODD;
            g.hr = e_max > w - 1 ? e_max - (w - 1) : 0;
            if (g.hl > w || g.hr > w || (4 / WL_ROWS_LOADERS) * (g.hl + g.hr) > 128) return WL_DECLINE(8);   // rows shorter than the filter
            g.pad = wl_align_up(g.hl * (int)sizeof(T), 16);
            g.ring_pitch = wl_align_up(g.pad + (w + g.hr) * (int)sizeof(T), 16);
            if (j > 0) {
                // levels >= 2 resolve their source rows with the single-fold extension (wl_ext1)
                const int e_last = a.base + 2 * (g.Kh + WARM) - 1;
                if (-a.base > h || e_last >= 2 * h - 1 || h < 2) return WL_DECLINE(9);
                // an odd periodized level repeats its last row / column (a lane would be the source of two halo cells on one side;
                // the rows above the plane would not be the rows at its bottom): level by level
                if (per && ((h & 1) || (w & 1))) return WL_DECLINE(10);
            }
            h = g.Kh; w = g.Kw;
        }
        for (int j = nlev; j < WL_ROWS_MAXLEV; ++j) { a.g[j] = a.g[nlev - 1]; a.g[j].nwaves = 0; a.yh[j] = nullptr; }
        if (wave + WL_ROWS_LOADERS > WL_ROWS_WAVES) return WL_DECLINE(11);   // rows wider than the compute waves cover
        compute_waves = wave;
    }
    // segments: whole plane; top / bottom half, cut at row m of the coarsest level.  The bottom half of level j starts
    // at the first row its next level needs (m_j = base + 2 m_{j+1}); the top half computes (without storing) the L-2
    // rows beyond the cut that its own next level reads.
    for (int t = 0; t < 3; ++t)
        for (int j = 0; j < WL_ROWS_MAXLEV; ++j) { a.seg[t].f0[j] = a.seg[t].fend[j] = a.seg[t].own_lo[j] = a.seg[t].own_hi[j] = 0; }
    bool can_split = true;
    {
        // the whole plane: feeds [F0, FEND) of every level.  Periodization: a level also COMPUTES the rows above / below its plane
        // that the level below reads (rows base + 2 F0[j+1] .. base + 2 FEND[j+1] - 1 of its periodic output - its loader / the level
        // above wrap around for it), exactly like the halves of a cut plane compute the rows beyond the cut
        int F0[WL_ROWS_MAXLEV], FEND[WL_ROWS_MAXLEV];
        for (int j = nlev - 1; j >= 0; --j) {
            F0[j] = 0; FEND[j] = a.g[j].Kh + WARM;
            if (per && j + 1 < nlev) { F0[j] = a.base + 2 * F0[j + 1]; FEND[j] = a.base + 2 * FEND[j + 1] + WARM; }
        }
        int m[WL_ROWS_MAXLEV];
        m[nlev - 1] = a.g[nlev - 1].Kh / 2;
        for (int j = nlev - 2; j >= 0; --j) m[j] = a.base + 2 * m[j + 1];
        for (int j = 0; j < nlev; ++j) if (m[j] < 1 || m[j] >= a.g[j].Kh - 1) can_split = false;
        for (int j = 0; j < nlev; ++j) {
            const int Kh = a.g[j].Kh;
            a.seg[0].f0[j] = F0[j]; a.seg[0].fend[j] = FEND[j]; a.seg[0].own_lo[j] = 0; a.seg[0].own_hi[j] = Kh;
            if (!can_split) continue;
            a.seg[2].f0[j] = m[j]; a.seg[2].fend[j] = FEND[j]; a.seg[2].own_lo[j] = m[j]; a.seg[2].own_hi[j] = Kh;
            a.seg[1].f0[j] = F0[j]; a.seg[1].own_lo[j] = 0; a.seg[1].own_hi[j] = m[j];
        }
        if (can_split)
            for (int j = nlev - 1; j >= 0; --j) {   // rows the top half must produce: its own, and what level j+1 reads
                int rows = a.seg[1].own_hi[j];
                if (j + 1 < nlev) {
                    const int need = a.base + 2 * a.seg[1].fend[j + 1];   // one past the last extended row level j+1 reads
                    if (need > rows) rows = need;
                }
                if (rows > FEND[j] - WARM) rows = FEND[j] - WARM;
                a.seg[1].fend[j] = rows + WARM;
            }
    }
    if (strips == 2 && !can_split) return WL_DECLINE(12);
    // the smallest power-of-two LL ring none of the schedules overruns, and the LDS layout for it
    int off = 0;
    {
        int r0 = 8;
        while (r0 < LT) r0 *= 2;
        if (NP2) r0 = 2;                                       // (grown to exactly what the simulated schedule needs)
        for (int j = 0; j < WL_ROWS_MAXLEV; ++j) a.g[j].ring_rows = r0;
    }
    for (;;) {
        bool bad = false;
        for (int t = 0; t < (can_split ? 3 : 1) && !bad; ++t) {
            int need[WL_ROWS_MAXLEV];
            const int rc = wl_rows_plan_segment<T>(a, a.seg[t], LT, need);
            if (rc) { if (t == 0) return rc; can_split = false; break; }   // a cut that does not schedule: whole planes only
            for (int j = 1; j < nlev; ++j)
                if (need[j] > a.g[j].ring_rows) {          // (the schedule does not depend on the ring sizes: only the overrun ring grows)
                    if (NP2) a.g[j].ring_rows = need[j];   // exactly what the schedule needs (wl_dwt_rows.h: NP2)
                    else a.g[j].ring_rows *= 2;
                    bad = true;
                    if (a.g[j].ring_rows > 64) return WL_DECLINE(13);
                }
        }
        if (!bad) break;
    }
    for (int j = 0; j < WL_ROWS_MAXLEV; ++j) a.g[j].ring_magic = (unsigned)(0x100000000ull / (unsigned)a.g[j].ring_rows);
    if (NP2)
        for (int j = 1; j < nlev; ++j) {
            // the rows live at once in a ring (at most ring_rows consecutive row numbers) must sit in distinct slots:
            // slot(r + rows) == slot(r) over every row number the levels address - the reader's from base up, the producer's
            // from -hl up (periodization: rows -hl .. -1 are the wrapped bottom rows, wl_dwt_rows.h) - and one period is a permutation
            const int rows = a.g[j].ring_rows, hi = a.g[j].Hs + 2 * LT + rows;
            int lo = a.base < 0 ? a.base : 0;
            if (-a.g[j].hl < lo) lo = -a.g[j].hl;
            if (-a.g[j - 1].hl < lo) lo = -a.g[j - 1].hl;
            unsigned long long seen = 0;
            for (int r = lo; r < lo + rows; ++r) seen |= 1ull << wl_ring_slot(r, rows, a.g[j].ring_magic);
            if (seen != (rows == 64 ? ~0ull : (1ull << rows) - 1)) return WL_DECLINE(16);
            for (int r = lo; r + rows <= hi; ++r)
                if (wl_ring_slot(r + rows, rows, a.g[j].ring_magic) != wl_ring_slot(r, rows, a.g[j].ring_magic)) return WL_DECLINE(16);
        }
    if (strips == 2 && !can_split) return WL_DECLINE(14);
    {
        int zero_bytes = 0;
        off = 0;
        for (int j = 0; j < nlev; ++j) {
            a.g[j].ring_off = off;
            off += (j == 0 ? 4 * K::NSLOT : a.g[j].ring_rows) * a.g[j].ring_pitch;
            if (a.g[j].ring_pitch > zero_bytes) zero_bytes = a.g[j].ring_pitch;
        }
        for (int j = nlev; j < WL_ROWS_MAXLEV; ++j) a.g[j].ring_off = a.g[nlev - 1].ring_off;
        a.zero_off = off; off += zero_bytes;
#if !defined(__HIPCC__)
        if (off > 80 * 1024 && getenv("WL_EMU_TRACE"))
            for (int j = 0; j < nlev; ++j) fprintf(stderr, "[wl]   level %d: ring rows %d pitch %d\n", j, j == 0 ? 4 * K::NSLOT : a.g[j].ring_rows, a.g[j].ring_pitch);
#endif
        // over the 80 KiB of two workgroups per CU with power-of-two rings: the long orthogonal filters have an instantiation whose rings are sized
        // exactly (NP2: the lattice variants of 12 taps and more and their armed two-bank fallbacks, even `base`)
        if constexpr (!NP2 && !ODD && LT >= 12 && ((SAME && LAT) || (!SAME && !LAT))) {
            if (off > 80 * 1024 && nlev > 1)
                return wl_afb_rows_launch<T, LT, PPR, SAME, LAT, ODD, 1>(r, lat, guard, what);
        }
        if (off > 80 * 1024) return WL_DECLINE(15);            // two workgroups per CU
    }
    // narrow planes leave most of the 12 waves idle (one compute wave per 64 coefficient columns and level): several planes
    // per workgroup - what the waves and 80 KiB of LDS allow, and no more than leaves a workgroup for every CU
    const int pp_cap = WL_ROWS_WAVES / (compute_waves + WL_ROWS_LOADERS);
    int pp = pp_cap;
    a.lds_plane = wl_align_up(off, 16);
    while (pp > 1 && (pp * a.lds_plane > 80 * 1024 || (planes + pp - 1) / pp < (int64_t)wl_num_cus())) --pp;
    if (strips == 2) pp = 1;
    bool pack_cut = false;
    if (strips == 0 && can_split && pp == 1 && pp_cap > 1) {
        // what the rules below would do with whole planes (+ halves to fill the last round): rounds x a whole plane's rows
        const int64_t slots = 2 * (int64_t)wl_num_cus();
        const int p2 = wl_rows_pack_and_cut(planes, pp_cap, a.lds_plane, a.g[0].Kh, WARM, ((planes + slots - 1) / slots) * (int64_t)(a.g[0].Kh + 8), wl_num_cus());
        if (p2) { pp = p2; pack_cut = true; }
    }
    a.pp = pp;
    if (pp > 1) off = pp * a.lds_plane;
    a.lds_bytes = off;
    const int64_t units = (planes + pp - 1) / pp;
    // how many planes to cut: workgroups = planes + cut planes should fill whole rounds of 2 workgroups per CU
    int64_t ncut = 0;
    if (can_split && strips == 2) ncut = planes;
    else if (pack_cut) ncut = units;                                // (wl_rows_pack_and_cut: every unit of pp planes as two halves)
    else if (can_split && strips == 0 && pp == 1) {
        const int64_t cus = wl_num_cus(), slots = 2 * cus;
        const int64_t rounds = (planes + slots - 1) / slots;        // rounds the whole planes alone would need
        ncut = rounds * slots - planes;                             // fill the last round with halves
        if (ncut > planes) ncut = planes;
        if (rounds > 1 && ncut * 4 > planes) ncut = 0;              // many rounds: the tail matters little, the halo does
        // fewer planes than compute units: a workgroup alone on its CU is issue-bound at ~0.11 ms per 512x512 plane, so
        // halves on CUs of their own (0.06-0.07 ms) as long as there are CUs for them, never two workgroups per CU
        if (planes <= cus) ncut = cus - planes < planes ? cus - planes : planes;
    }
    a.nwhole = (int)(units - ncut);
    {   // deal the roles out to the waves: waves w and w+4 share a SIMD; a SIMD issues about one instruction per four
        // cycles for all its waves together, so what counts is the instruction load per SIMD.  Greedy, heaviest first:
        // a level-j chunk runs 2 / 1 / 0.5 feeds per half-batch, a loader issues about as much as half a feed.
        int load[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
        const int cap[4] = {(WL_ROWS_WAVES + 3) / 4, (WL_ROWS_WAVES + 2) / 4, (WL_ROWS_WAVES + 1) / 4, WL_ROWS_WAVES / 4};
        for (int w = 0; w < WL_ROWS_WAVES; ++w) { a.role_level[w] = -2; a.role_col0[w] = 0; a.role_sub[w] = 0; }
        int sub = 0;
        auto place = [&](int level, int col0, int cost) {
            int best = -1;
            for (int b = 0; b < 4; ++b)
                if (cnt[b] < cap[b] && (best < 0 || load[b] < load[best])) best = b;
            const int w = best + 4 * cnt[best];
            a.role_level[w] = (signed char)level; a.role_col0[w] = (short)col0; a.role_sub[w] = (signed char)sub;
            load[best] += cost; ++cnt[best];
        };
        for (sub = 0; sub < pp; ++sub)
            for (int j = 0; j < nlev; ++j)
                for (int c = 0; c < a.g[j].nwaves; ++c) place(j, 64 * c, 8 >> j);
        for (sub = 0; sub < pp; ++sub)
            for (int l = 0; l < WL_ROWS_LOADERS; ++l) place(-1, l, 4 / WL_ROWS_LOADERS);
    }
    a.x = (const T*)r.x; a.ll = (T*)r.yl;
    for (int j = 0; j < nlev; ++j) a.yh[j] = (T*)r.yh[j];
    a.h_w_lo = (const float*)r.taps.w_lo; a.h_w_hi = (const float*)r.taps.w_hi;
    a.h_h_lo = (const float*)r.taps.h_lo; a.h_h_hi = (const float*)r.taps.h_hi;
    a.NC = planes; a.x_ps = r.x_ps; a.x_rs = r.x_rs;
    a.ll_ps = (int64_t)a.g[nlev - 1].Kh * a.g[nlev - 1].Kw; a.ll_rs = a.g[nlev - 1].Kw;
    a.guard = guard;
    a.lat = lat;
    if (what == 1) return 0;
    return what == 2 ? wl_launch_armed<K>(a, units + ncut, (size_t)off, r.stream) : wl_launch<K>(a, units + ncut, (size_t)off, r.stream);
}

// One tap count.  Up to 12 taps: the one-bank variant (SAME) when both axes are handed the same device buffers (proven: no check),
// or when the caller HINTS that the two banks hold the same taps - then the variant verifies that on the device and the two-bank
// variant stands by behind it (wl_common.h, tap-relation guards); else the two-bank variant.  From WL_ROWS_LAT_MIN taps on, with
// BOTH hints (same banks, quadrature-mirror highpass) and device scratch from the caller: the LATTICE variant (wl_lattice.h) behind
// the one-thread examination WlTapPrep, the two-bank variant armed behind it - the only fused form of 14-20 taps (the two-bank
// kernel of those lengths spills its window and exists as the fallback alone).
#ifndef WL_ROWS_LAT_MIN
#define WL_ROWS_LAT_MIN 10
#endif
// ODD = 1: the instantiations for an odd `base` (periodization with L % 4 == 0, wl_dwt_rows.h): the two-bank direct form up to 12
// taps, the lattice variant from 12 taps on (no SAME-only variant: one more instantiation per shape for biorthogonal 12-tap banks).
template <typename T, int LT, int PPR, int ODD = 0>
static int wl_afb_rows_pick(const WlAfbPyrReq& r) {
    const bool same_hint = (r.hints & 1) != 0, qmf_hint = (r.hints & 2) != 0;
    const float* const none = nullptr;
    if constexpr (LT >= WL_ROWS_LAT_MIN) {
        if (same_hint && qmf_hint && r.scratch)
            return wl_lattice_launch<LT>([&](int guard, int what) { return wl_afb_rows_launch<T, LT, PPR, 0, 0, ODD>(r, r.scratch, guard, what); },
                                         [&](int guard, int what) { return wl_afb_rows_launch<T, LT, PPR, 1, 1, ODD>(r, r.scratch, guard, what); },
                                         r.taps, 0, 1, sizeof(T), r.scratch, r.tstate, 3, r.stream);
    }
    if constexpr (LT > 12) return WL_ERR_UNSUPPORTED;          // (no direct-form fused kernel above 12 taps)
    else {
        if constexpr (LT >= WL_ROWS_SAME_MIN && !ODD) {
            if (r.taps.w_lo == r.taps.h_lo && r.taps.w_hi == r.taps.h_hi) return wl_afb_rows_launch<T, LT, PPR, 1>(r, none);
            if (same_hint) WL_GUARDED_PAIR((wl_afb_rows_launch<T, LT, PPR, 1>), (wl_afb_rows_launch<T, LT, PPR, 0>), r, none);
        }
        return wl_afb_rows_launch<T, LT, PPR, 0, 0, ODD>(r, none);
    }
}

template <typename T>
static int wl_afb_rows_dispatch(const WlAfbPyrReq& r) {
    const int ppr = wl_cdiv(r.W * (int)sizeof(T), 1024);
    const bool odd = (wl_afb_base(r.W, r.L, r.mode) & 1) != 0;      // periodization with L % 4 == 0
#define WL_PICK(LT_, P_)                                                               \
    do {                                                                               \
        if constexpr (LT_ % 4 == 0) { if (odd) return wl_afb_rows_pick<T, LT_, P_, 1>(r); } \
        return wl_afb_rows_pick<T, LT_, P_, 0>(r);                                     \
    } while (0)
#define WL_CASE(LT_)                                                                   \
    case LT_:                                                                          \
        if (ppr == 1) WL_PICK(LT_, 1);                                                 \
        if (ppr == 2) WL_PICK(LT_, 2);                                                 \
        if constexpr (sizeof(T) == 4) {    /* rows of 2-3 KiB: the 515-column ll below a 1024-wide float32 image (its 5 + 3 compute waves fit; float16 rows that long need more waves than a workgroup has) */ \
            if (ppr == 3) WL_PICK(LT_, 3);                                             \
        }                                                                              \
        return WL_ERR_UNSUPPORTED
    switch (r.L) {
        WL_CASE(2); WL_CASE(4); WL_CASE(6); WL_CASE(8); WL_CASE(10); WL_CASE(12); WL_CASE(14); WL_CASE(16); WL_CASE(18); WL_CASE(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASE
#undef WL_PICK
}

extern "C" int wl_dwt2d_analysis_fused_ex(const void* xp, int64_t x_plane_stride, int x_row_stride, void* yl, void* const* yh,
                                          int dtype, int64_t planes, int H, int W, int nlev, const void* h_w_lo,
                                          const void* h_w_hi, const void* h_h_lo, const void* h_h_hi, int L, int mode,
                                          int strips, void* tap_scratch, int* tap_state, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (planes < 0 || H < 1 || W < 1 || x_row_stride < W || x_plane_stride < 0) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    if (mode == 2 && (H + (H & 1) < L - 1 || W + (W & 1) < L - 1)) return WL_ERR_UNSUPPORTED;
    // strips bit 2 (value 4): the caller believes that the row and the column banks hold the same taps (a hint: verified on the
    // device, see wl_afb_rows_pick)
    // bit 3 (value 8): a HINT that each highpass bank is the quadrature mirror of its lowpass bank; with both hints and tap_scratch
    // the lattice variant runs (10-20 taps).  *tap_state (wl_lattice.h): what this library has already examined into tap_scratch
    if (strips > 15) return WL_ERR_UNSUPPORTED;
    const int hints = strips < 0 ? 0 : ((strips & 4) ? 1 : 0) | ((strips & 8) ? 2 : 0);
    if (!tap_scratch) tap_state = nullptr;
    if (strips >= 0) strips &= 3;
    if (strips < 0 || strips > 2) return WL_ERR_UNSUPPORTED;
    // one workgroup per plane (or half plane): pays from about 3/8 of the compute units up (strips == 1 forces the kernel)
    if (strips == 0 && 8 * planes < 3 * wl_num_cus()) return WL_ERR_UNSUPPORTED;   // measured break-even against the tile kernels: 96 planes
    const WlAfbPyrReq r = {xp, x_plane_stride, x_row_stride, yl, yh, planes, H, W, nlev, {h_w_lo, h_w_hi, h_h_lo, h_h_hi}, L, mode,
                           strips, hints, (float*)tap_scratch, tap_state, stream};
    // (no planes: nothing to do for a dtype the kernel has, the usual codes for the others)
    WL_DISPATCH_FLOAT(dtype, return planes == 0 ? 0 : wl_afb_rows_dispatch<T>(r));
}

// (the entry point of library versions up to 1.x: dense x, no device scratch - so no lattice variant: 14, 16, 20 taps decline)
extern "C" int wl_dwt2d_analysis_fused(const void* x, void* yl, void* const* yh, int dtype, int64_t planes,
                                       int H, int W, int nlev, const void* h_w_lo, const void* h_w_hi,
                                       const void* h_h_lo, const void* h_h_hi, int L, int mode, int strips, void* stream) {
    return wl_dwt2d_analysis_fused_ex(x, (int64_t)H * W, W, yl, yh, dtype, planes, H, W, nlev, h_w_lo, h_w_hi, h_h_lo, h_h_hi,
                                      L, mode, strips, nullptr, nullptr, stream);
}


#endif   // !WL_ROWS_UNIT_SYNTHESIS

#if !defined(WL_ROWS_UNIT_ANALYSIS)
// ---- fused multi-level streaming synthesis (wl_idwt_rows.h) -----------------------------------------
#include "wl_idwt_rows.h"

// Simulate one segment's schedule exactly as the waves will follow it: fills sg.sched / sg.nhb.
template <typename T>
static int wl_irows_plan_segment(const WlIRowsArgs<T>& a, WlIRowsSeg& sg, int LT) {
    WlIRowsSched sc;
    sc.init(sg);
    int nhb = 0;
    for (;; ++nhb) {
        int nn[WL_IROWS_MAXLEV], todo = 0, any = 0;
        for (int j = 0; j < a.nlev; ++j) { nn[j] = sc.feeds_now(a, sg, j, LT); todo += sg.fend[j] - sc.fed[j]; any += nn[j]; }
        if (todo == 0) break;
        if (nhb >= WL_IROWS_MAXHB || !any) return WL_ERR_UNSUPPORTED;   // taller than the table, or a level starves
        if ((nhb & 3) == 0) sg.sched[nhb >> 2] = 0;
        for (int j = 0; j < a.nlev; ++j) sg.sched[nhb >> 2] |= (unsigned)nn[j] << (8 * (nhb & 3) + 2 * j);
        for (int j = 0; j < a.nlev; ++j) sc.fed[j] += nn[j];
    }
    sg.nhb = nhb;
    return 0;
}

// Geometry, LDS layout, wave roles, segments and their schedules.  strips as for the analysis kernel.
template <typename T, int LT, int LAT = 0, int PER = 0>
static int wl_sfb_rows_launch(const WlSfbPyrReq& r, const float* lat = nullptr, int guard = 0, int what = 0) {
    // what: 0 = launch, 1 = dry run (every check, no launch), 2 = launch as the armed fallback of a lattice launch
    // PER: periodization (wl_idwt_rows.h): every level exactly twice the size of the level above, all 2K outputs kept
    typedef WlSfbRows<T, LT, LAT, PER> K;
    const int SZ = (int)sizeof(T), WARM = K::WARM;
    const int64_t planes = r.planes, ll_ps = r.yl_ps;
    const int ll_rs = r.yl_rs, yl_h = r.yl_h, yl_w = r.yl_w, nlev = r.nlev, strips = r.strips;
    const void* const yl = r.yl; const void* const* const yh = r.yh;
    const int* const Kh = r.Kh; const int* const Kw = r.Kw;
    WlIRowsArgs<T> a;
    if (nlev < 1 || nlev > WL_IROWS_MAXLEV) return WL_ERR_UNSUPPORTED;
    a.nlev = nlev;
    a.per = PER;
    // geometry, coarsest level first: the low-pass source of level j is yl / the output of level j+1, which may be
    // one row / column larger than yh[j] (the reference drops the surplus: dwt/transform2d.py:141-146)
    int compute_waves = 0;
    {
        int sh = yl_h, sw = yl_w;
        for (int j = nlev - 1; j >= 0; --j) {
            WlIRowsLevel& g = a.g[j];
            g.Kh = Kh[j]; g.Kw = Kw[j];
            if (g.Kh < LT / 2 || g.Kw < LT / 2) return WL_ERR_UNSUPPORTED;          // no output at all / degenerate
            if (sh < g.Kh || sh > g.Kh + 1 || sw < g.Kw || sw > g.Kw + 1) return WL_ERR_SHAPE;
            if (PER && (sh != g.Kh || sw != g.Kw)) return WL_ERR_UNSUPPORTED;          // (an odd periodized level: the caller's 'unpad' - level by level)
            g.OH = PER ? 2 * g.Kh : 2 * g.Kh - LT + 2; g.OW = PER ? 2 * g.Kw : 2 * g.Kw - LT + 2;
            g.per_d0 = 0; g.head_off = -1;
            if ((int64_t)g.Kh * g.Kw >= (1LL << 28)) return WL_ERR_UNSUPPORTED;     // 32-bit in-plane byte offsets
            // planes are copied as 16-byte pieces (+ a dword tail) from 4-byte aligned addresses
            g.rbytes = g.Kw * SZ;
            if (g.rbytes % 4 != 0 || ((int64_t)g.Kh * g.rbytes) % 4 != 0 || (uintptr_t)yh[j] % 4 != 0) return WL_ERR_UNSUPPORTED;
            // the ring holds a chunk's worth of rows more than the rows in use (see the loader)
#ifndef WL_IROWS_R0
#define WL_IROWS_R0 8
#endif
            g.dma_rows = j == 0 ? WL_IROWS_R0 : 8; g.dma_shift = j == 0 && WL_IROWS_R0 == 16 ? 4 : 3;
            if (PER) {   // rows of a 16-byte pitch with WARM wrapped cells in front of the coefficients
                g.per_d0 = wl_align_up(WARM * SZ, 16);
                g.rbytes = wl_align_up(g.per_d0 + g.Kw * SZ, 16);
                // short rows of whole 16-byte pieces: G ring rows per DMA instruction (wl_idwt_rows.h), a ring of four groups
                g.per_grp = 1;
#ifndef WL_IROWS_PER_GRP
#define WL_IROWS_PER_GRP 8
#endif
                if ((g.Kw * SZ) % 16 == 0)
                    while (g.per_grp < WL_IROWS_PER_GRP && 2 * g.per_grp * g.rbytes <= WL_IROWS_CHUNK) g.per_grp *= 2;
                while (g.dma_rows < 4 * g.per_grp) { g.dma_rows *= 2; ++g.dma_shift; }
            } else g.per_grp = 1;
            while (!PER && (g.dma_rows < wl_cdiv(WL_IROWS_CHUNK, g.rbytes) + 4 || (g.dma_rows * g.rbytes) % 16)) { g.dma_rows *= 2; ++g.dma_shift; }
            g.cpr = wl_cdiv(g.dma_rows * g.rbytes, WL_IROWS_CHUNK);
            g.nwaves = wl_cdiv(wl_cdiv(g.OW, 2), 64);
            compute_waves += g.nwaves;
            sh = g.OH; sw = g.OW;
        }
        // the coarsest low-pass is copied like a band plane: dense rows of exactly Kw
        if (ll_rs != a.g[nlev - 1].Kw || (ll_ps * SZ) % 4 != 0 || (uintptr_t)yl % 4 != 0) return WL_ERR_UNSUPPORTED;
        if (PER && (yl_h != a.g[nlev - 1].Kh || yl_w != a.g[nlev - 1].Kw)) return WL_ERR_UNSUPPORTED;
        if ((int64_t)a.g[0].OH * a.g[0].OW >= (1LL << 28)) return WL_ERR_UNSUPPORTED;
    }
    // wave roles: the finest level has one loader per band (all four sources when it is also the coarsest), every
    // coarser level one loader for all its sources
    struct Ld { int level, s0, ns; } ld[8];
    int nld = 0;
    // Narrow planes leave most of the 14 waves idle (one compute wave per 128 output columns and level): several planes per
    // workgroup, every one with its compute waves and loaders (a single level on up to 256 columns: ONE loader for its four
    // sources, so that up to seven planes fit).  pp is settled below, once the LDS of a plane is known.
    const bool one_loader = nlev == 1 && compute_waves <= 2;
    if (one_loader) ld[nld++] = Ld{0, 0, 4};
    else if (nlev == 1) for (int s = 0; s < 4; ++s) ld[nld++] = Ld{0, s, 1};
    else {
        // (round 5) narrow planes - one compute wave per level (WL_IROWS_NARROW_ML = 2: up to two at the finest) - where it lets another
        // plane into the workgroup: the finest level's three bands through ONE loader like every coarser level's, nlev loader waves per
        // plane instead of nlev + 2 (with three loaders at the finest level three levels of a 128-column plane left no waves for a
        // second plane: 512x3x128^2 J = 3 0.146 -> 0.083 ms, 1024x3x112^2 0.217 -> 0.120 ms, same box)
#ifndef WL_IROWS_NARROW_ML
#define WL_IROWS_NARROW_ML 2
#endif
        const bool narrow_ml = WL_IROWS_NARROW_ML && strips != 2 && compute_waves <= nlev + WL_IROWS_NARROW_ML - 1 &&
                               WL_IROWS_WAVES / (compute_waves + nlev) > WL_IROWS_WAVES / (compute_waves + nlev + 2);
        if (narrow_ml) ld[nld++] = Ld{0, 1, 3};
        else for (int s = 1; s < 4; ++s) ld[nld++] = Ld{0, s, 1};
        for (int j = 1; j < nlev; ++j) ld[nld++] = Ld{j, j == nlev - 1 ? 0 : 1, j == nlev - 1 ? 4 : 3};
    }
    if (compute_waves + nld > WL_IROWS_WAVES) return WL_ERR_UNSUPPORTED;            // rows wider than the waves cover
    for (int l = 0; l < nld; ++l) {   // the steps under two rows must fit into the loader's DMA instructions in flight
        if (PER) {                      // (a step = one row of every source: at least four rows in flight)
            const int rowb = a.g[ld[l].level].Kw * SZ;
            const int per_row = a.g[ld[l].level].per_grp > 1 ? ld[l].ns : ld[l].ns * (wl_cdiv(rowb & ~15, WL_IROWS_CHUNK) + ((rowb & 15) ? 1 : 0));
            if (WL_IROWS_MAX_VM / per_row - 1 < 4) return WL_ERR_UNSUPPORTED;
        } else if (2 * wl_cdiv(a.g[ld[l].level].rbytes, WL_IROWS_CHUNK) + 2 > WL_IROWS_MAX_VM / ld[l].ns - 1) return WL_ERR_UNSUPPORTED;
    }
    int pp_waves = WL_IROWS_WAVES / (compute_waves + nld);                          // planes the waves allow
#ifdef WL_IROWS_PP_MAX
    if (pp_waves > WL_IROWS_PP_MAX) pp_waves = WL_IROWS_PP_MAX;
#endif
    // segments: the whole plane; rows [0, M) and [M, OH) of x
    for (int t = 0; t < 3; ++t) {
        a.seg[t].own_lo = a.seg[t].own_hi = a.seg[t].nhb = 0;
        for (int j = 0; j < WL_IROWS_MAXLEV; ++j) a.seg[t].f0[j] = a.seg[t].fend[j] = 0;
    }
    const int OH0 = a.g[0].OH;
    int M = (OH0 / 2) & ~1;
    if (PER) M &= ~((2 << nlev) - 1);   // (the rotation of the second half must be whole coefficient rows at every level: 2 rho_0 = M)
    bool can_split = M >= 2 && M + 2 <= OH0;
    for (int t = 0; t < 3; ++t)
        for (int j = 0; j < WL_IROWS_MAXLEV; ++j) a.seg[t].rho[j] = 0;
    for (int t = 0; t < (can_split ? 3 : 1); ++t) {
        WlIRowsSeg& sg = a.seg[t];
        sg.own_lo = t == 2 ? M : 0;
        sg.own_hi = t == 1 ? M : OH0;
        if (PER) {
            // periodization: a segment is z rows [0, len) of the plane ROTATED by rho (wl_idwt_rows.h): the whole plane rho = 0, len = OH; the
            // halves rho = 0 / M/2 (coefficient rows of level 0, halved per level), len = M / OH - M - neither meets its own wrap, both start
            // at feed 0.  Level j makes the low-pass rows [0, fend[j-1]) the level below reads (those beyond its ring's last row: head copies)
            const int len = sg.own_hi - sg.own_lo;
            for (int j = 0; j < nlev; ++j) sg.rho[j] = (sg.own_lo / 2) >> j;
            sg.own_lo = 0; sg.own_hi = len;
            sg.f0[0] = 0;
            sg.fend[0] = len / 2 + WARM;
            for (int j = 1; j < nlev; ++j) {
                sg.f0[j] = 0;
                int rows = sg.fend[j - 1];                         // ring rows [0, rows) of level j-1's low-pass
                if (rows > a.g[j - 1].Kh) rows = a.g[j - 1].Kh;   // (the feeds past the plane's bottom read the head copies)
                sg.fend[j] = (rows + 1) / 2 + WARM;
            }
            continue;
        }
        // feeds of level 0: output rows 2(k - WARM), +1 come out of feed k, whose window holds coefficient rows k-WARM..k
        sg.f0[0] = sg.own_lo / 2;
        sg.fend[0] = (sg.own_hi + 1) / 2 + WARM;
        if (sg.fend[0] > a.g[0].Kh) sg.fend[0] = a.g[0].Kh;
        for (int j = 1; j < nlev; ++j) {   // level j makes the low-pass rows [f0, fend) of level j-1
            sg.f0[j] = sg.f0[j - 1] / 2;
            sg.fend[j] = (sg.fend[j - 1] - 1) / 2 + WARM + 1;
            if (sg.fend[j] > a.g[j].Kh) sg.fend[j] = a.g[j].Kh;
        }
    }
    // LDS: per level four source rings; the LDS-fed low-pass rings get the smallest power-of-two depth that does not
    // slow the schedule down
    int off = 0;
    for (int rr = 4;; rr *= 2) {
        off = 0;
        for (int j = 0; j < nlev; ++j) {
            WlIRowsLevel& g = a.g[j];
            if (j + 1 < nlev) {
                int cols = g.Kw;
                if (2 * wl_cdiv(a.g[j + 1].OW, 2) > cols) cols = 2 * wl_cdiv(a.g[j + 1].OW, 2);
                if (PER) cols += WARM;                             // the wrapped cells behind the row
                g.ll_rows = rr; g.ll_pitch = wl_align_up(cols * SZ, 16);
            } else { g.ll_rows = g.dma_rows; g.ll_pitch = g.rbytes; }
            for (int s = 0; s < 4; ++s) {
                g.src_off[s] = off;
                off += s == 0 ? g.ll_rows * g.ll_pitch : wl_align_up(g.dma_rows * g.rbytes, 16);
                if (PER && s == 0 && j + 1 < nlev) { g.head_off = off; off += (WARM > 0 ? WARM : 1) * g.ll_pitch; }   // copies of the ring's first rows
            }
        }
        bool ok = true;
        for (int t = 0; t < (can_split ? 3 : 1); ++t) {
            const int rc = wl_irows_plan_segment<T>(a, a.seg[t], LT);
            if (rc) { if (t == 0) return rc; can_split = false; break; }
            // the same with rings nothing ever waits for
            WlIRowsArgs<T> b = a;
            for (int j = 0; j < nlev; ++j) b.g[j].ll_rows = 1 << 20;
            wl_irows_plan_segment<T>(b, b.seg[t], LT);
            if (a.seg[t].nhb > b.seg[t].nhb + 2) ok = false;
        }
        if (ok || nlev == 1) break;
        if (rr >= 64) return WL_ERR_UNSUPPORTED;
    }
    for (int j = nlev; j < WL_IROWS_MAXLEV; ++j) { a.g[j] = a.g[nlev - 1]; a.g[j].nwaves = 0; a.yh[j] = nullptr; }
    if (off > 80 * 1024) return WL_ERR_UNSUPPORTED;                                  // two workgroups per CU
    // planes per workgroup: what the waves and 80 KiB of LDS allow, and no more than leaves a workgroup for every CU
    int pp = pp_waves;
    a.lds_plane = wl_align_up(off, 16);
    while (pp > 1 && (pp * a.lds_plane > 80 * 1024 || (planes + pp - 1) / pp < (int64_t)wl_num_cus())) --pp;
    if (strips == 2) pp = 1;
    bool pack_cut = false;
    if (strips == 0 && can_split && pp == 1 && pp_waves > 1) {
        // what the rules below do with one plane per workgroup: a single partly filled round -> halves of every plane (rounds of
        // half planes), else rounds of whole planes
        const int64_t slots = 2 * (int64_t)wl_num_cus();
        const int64_t r1 = (planes + slots - 1) / slots;
        const bool halves = r1 == 1 && r1 * slots - planes > 0 && planes > wl_num_cus();
        const int64_t cost_now = halves ? ((2 * planes + slots - 1) / slots) * (int64_t)(OH0 / 4 + LT / 2 + 8) : r1 * (int64_t)(OH0 / 2 + 8);
        const int p2 = wl_rows_pack_and_cut(planes, pp_waves, a.lds_plane, OH0 / 2, LT / 2, cost_now, slots);
        if (p2) { pp = p2; pack_cut = true; }
    }
    a.pp = pp;
    if (pp > 1) off = pp * a.lds_plane;
    a.lds_bytes = off;
    {
        int load[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
        const int cap[4] = {(WL_IROWS_WAVES + 3) / 4, (WL_IROWS_WAVES + 2) / 4, (WL_IROWS_WAVES + 1) / 4, WL_IROWS_WAVES / 4};
        for (int w = 0; w < WL_IROWS_WAVES; ++w) { a.role_level[w] = -2; a.role_arg[w] = 0; a.role_sub[w] = 0; }
        int sub = 0;
        auto place = [&](int level, int arg, int cost) {   // waves w and w+4 share a SIMD: balance the issue load
            int best = -1;
            for (int b = 0; b < 4; ++b)
                if (cnt[b] < cap[b] && (best < 0 || load[b] < load[best])) best = b;
            const int w = best + 4 * cnt[best];
            a.role_level[w] = (signed char)level; a.role_arg[w] = (short)arg; a.role_sub[w] = (signed char)sub;
            load[best] += cost; ++cnt[best];
        };
        for (sub = 0; sub < pp; ++sub)
            for (int j = 0; j < nlev; ++j)
                for (int c = 0; c < a.g[j].nwaves; ++c) place(j, 64 * c, 16 >> j);
        for (sub = 0; sub < pp; ++sub)
            for (int l = 0; l < nld; ++l) place(-1, ld[l].level * 16 + ld[l].s0 * 4 + (ld[l].ns - 1), ld[l].level == 0 ? 3 : 2);
    }
    if (strips == 2 && !can_split) return WL_ERR_UNSUPPORTED;
    const int64_t units = (planes + pp - 1) / pp;                                   // workgroups' worth of planes
    int64_t ncut = 0;
    if (can_split && strips == 2) ncut = planes;
    else if (pack_cut) ncut = units;                                                // (wl_rows_pack_and_cut)
    else if (can_split && strips == 0 && pp == 1) {
        const int64_t cus = wl_num_cus(), slots = 2 * cus;
        const int64_t rounds = (planes + slots - 1) / slots;
        ncut = rounds * slots - planes;
        if (ncut > planes) ncut = planes;
        if (rounds > 1 && ncut * 4 > planes) ncut = 0;
        // a single, partly filled round: halves of every plane spread better than a mix of wholes and halves whose time
        // is that of a whole (measured at 384 planes / 512 slots: 0.194 ms against 0.213 ms)
        if (rounds == 1 && ncut > 0) ncut = planes;
        // fewer planes than compute units: halves on CUs of their own as long as there are CUs for them (see the analysis)
        if (planes <= cus) ncut = cus - planes < planes ? cus - planes : planes;
    }
    a.nwhole = (int)(units - ncut);
    a.yl = (const T*)yl; a.ll_ps = ll_ps;
    for (int j = 0; j < nlev; ++j) a.yh[j] = (const T*)yh[j];
    a.y = (T*)r.y;
    a.g_w_lo = (const float*)r.taps.w_lo; a.g_w_hi = (const float*)r.taps.w_hi;
    a.g_h_lo = (const float*)r.taps.h_lo; a.g_h_hi = (const float*)r.taps.h_hi;
    a.NC = planes;
    a.guard = guard; a.lat = lat;
    if (what == 1) return 0;
    return what == 2 ? wl_launch_armed<K>(a, units + ncut, (size_t)off, r.stream) : wl_launch<K>(a, units + ncut, (size_t)off, r.stream);
}

// One tap count of the fused synthesis: from WL_IROWS_LAT_MIN taps on (8: the metric's inverse), with both hints (one bank for both axes, quadrature-mirror
// highpass banks) and device scratch, the LATTICE variant (wl_lattice.h, the transposed recurrence) behind the one-thread
// examination of the banks, the four-bank direct form armed behind it (above 12 taps that form exists as this fallback alone:
// its four banks of tap pairs do not fit the scalar registers); else the direct form up to 12 taps.
template <typename T, int LT, int PER = 0>
static int wl_sfb_rows_pick(const WlSfbPyrReq& r) {
    if constexpr (LT >= WL_IROWS_LAT_MIN) {
        if ((r.hints & 3) == 3 && r.scratch)
            return wl_lattice_launch<LT>([&](int guard, int what) { return wl_sfb_rows_launch<T, LT, 0, PER>(r, r.scratch, guard, what); },
                                         [&](int guard, int what) { return wl_sfb_rows_launch<T, LT, 1, PER>(r, r.scratch, guard, what); },
                                         r.taps, 1, 1, sizeof(T), r.scratch, r.tstate, 3, r.stream);
    }
    if constexpr (LT > 12) return WL_ERR_UNSUPPORTED;
    else return wl_sfb_rows_launch<T, LT, 0, PER>(r);
}

template <typename T>
static int wl_sfb_rows_dispatch(const WlSfbPyrReq& r) {
#define WL_CASE(LT_) case LT_: return r.mode == 2 ? wl_sfb_rows_pick<T, LT_, 1>(r) : wl_sfb_rows_pick<T, LT_, 0>(r)   // periodization: the PER instantiations (round 6)
    switch (r.L) {
        WL_CASE(2); WL_CASE(4); WL_CASE(6); WL_CASE(8); WL_CASE(10); WL_CASE(12); WL_CASE(14); WL_CASE(16); WL_CASE(18); WL_CASE(20);
        default: return WL_ERR_UNSUPPORTED;
    }
#undef WL_CASE
}

extern "C" int wl_dwt2d_synthesis_fused_ex(const void* yl, int64_t yl_plane_stride, int yl_row_stride, int yl_h, int yl_w,
                                           const void* const* yh, const int* Kh, const int* Kw, void* y, int dtype,
                                           int64_t planes, int nlev, const void* g_w_lo, const void* g_w_hi,
                                           const void* g_h_lo, const void* g_h_hi, int L, int mode, int strips,
                                           void* tap_scratch, int* tap_state, void* stream) {
    if (wl_mode_to_ext(mode) < 0) return WL_ERR_MODE;
    if (planes < 0 || yl_h < 1 || yl_w < 1) return WL_ERR_SHAPE;
    if (L < 1 || L > WL_MAX_TAPS) return WL_ERR_TAPS;
    // strips bits 2-3, tap_scratch and tap_state as for wl_dwt2d_analysis_fused_ex: the hints (same bank on both axes,
    // quadrature-mirror highpass banks) that select the lattice variant, what the scratch already holds
    if (strips > 15) return WL_ERR_UNSUPPORTED;
    const int hints = strips < 0 ? 0 : ((strips & 4) ? 1 : 0) | ((strips & 8) ? 2 : 0);
    if (!tap_scratch) tap_state = nullptr;
    if (strips >= 0) strips &= 3;
    if (strips < 0 || strips > 2) return WL_ERR_UNSUPPORTED;
    if (strips == 0 && 8 * planes < 3 * wl_num_cus()) return WL_ERR_UNSUPPORTED;   // measured break-even against the tile kernels: 96 planes
    if (planes == 0) return 0;
    const WlSfbPyrReq r = {yl, yl_plane_stride, yl_row_stride, yl_h, yl_w, yh, Kh, Kw, y, planes, nlev,
                           {g_w_lo, g_w_hi, g_h_lo, g_h_hi}, L, mode, strips, hints, (float*)tap_scratch, tap_state, stream};
    WL_DISPATCH_FLOAT(dtype, return wl_sfb_rows_dispatch<T>(r));
}

extern "C" int wl_dwt2d_synthesis_fused(const void* yl, int64_t yl_plane_stride, int yl_row_stride, int yl_h, int yl_w,
                                        const void* const* yh, const int* Kh, const int* Kw, void* y, int dtype,
                                        int64_t planes, int nlev, const void* g_w_lo, const void* g_w_hi,
                                        const void* g_h_lo, const void* g_h_hi, int L, int mode, int strips, void* stream) {
    return wl_dwt2d_synthesis_fused_ex(yl, yl_plane_stride, yl_row_stride, yl_h, yl_w, yh, Kh, Kw, y, dtype, planes, nlev,
                                       g_w_lo, g_w_hi, g_h_lo, g_h_hi, L, mode, strips, nullptr, nullptr, stream);
}
#endif   // !WL_ROWS_UNIT_ANALYSIS
