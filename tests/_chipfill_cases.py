"""Shared checks of the work-sharing walks the launchers take once a launch fills the chip, run by the emulator (CPU) and the
GPU test modules.  Every check takes (dev, cus): the row and plane counts come from `cus` through the launchers' own formulas,
mirrored below, so the same case enters the same branch on the emulator's 2 / 8 / 256-CU chips and on the 256-CU device.

  WlDwt1dFused (csrc/wl_dwt1d_api.inc)   cpw = rows * nchunks / (10 CUs) consecutive chunks per workgroup: a workgroup streams
                                         over them through ONE set of LDS buffers, the next chunk's samples in registers.
  WlAfbSmall   (csrc/wl_api.inc)         the grid is capped at min(8, 160 KiB / lds) workgroups per CU; a workgroup walks over
                                         the groups bid, bid + nblocks, .. with a register prefetch.
  WlDtFwd1Small (csrc/wl_api.inc)        run_len G > 1 planes per workgroup only when NC / G >= 2 CUs.

Every case asserts
  * the launch's grid (wl_last_grid) - the witness that the branch was entered: strictly fewer workgroups than chunks / groups;
  * the result against the float64 oracle on a sample: the first and the last unit and the units on either side of every
    group / run boundary, the short last one included (for the 1-D kernel, where a workgroup never leaves its row: whole rows);
  * BITWISE equality with the same rows / planes run again in batches small enough for one unit per workgroup (witnessed by
    the grid again): rows and planes are independent, and the arithmetic of an output depends on the chunk geometry, never on
    how chunks are shared - a difference is a race or a stale LDS cell, not rounding;
  * the kernel names (pw.kernels_since).

Bounds (relative to the band's maximum): 1e-5 float32, 4e-3 float16 (tests/_ext_cases.py::check_dwt1d_fused), _wpt1d_cases.REL
for bfloat16; 3e-6 / 5e-3 against the tile kernels (the small-plane DTCWT tests).  A device whose derived shape would exceed
MAX_BYTES is the one permitted skip."""
import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters as F, ops
from pytorch_wavelets_amd.dtcwt import lowlevel as dl
from _wpt1d_cases import REL

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TOL = {F32: 1e-5, F16: 4e-3, BF16: REL[BF16]}
TILE_TOL = {F32: 3e-6, F16: 5e-3}
TNAME = {F32: 'float', F16: '_Float16', BF16: '__bf16'}
MAX_BYTES = 256 << 20
DWT1D_SPAN = 4096        # WL_DWT1D_SPAN of csrc/wl_dwt1d_fused.h


def cdiv(a, b):
    return -(-a // b)


def last_grid():
    """Workgroups of the engine's last launch."""
    return int(ops._backend().wl_last_grid())


def npy(t):
    return t.detach().cpu().double().numpy()


def fits(nbytes, what):
    """The one permitted skip: a device so large that the derived shape would exceed MAX_BYTES."""
    if nbytes > MAX_BYTES:
        pytest.skip('%s: the shape derived from the CU count holds %d bytes, more than %d' % (what, nbytes, MAX_BYTES))


def close(got, want, tol, what):
    err, bound = float(np.abs(npy(got) - want).max()), tol * max(float(np.abs(want).max()), 1e-30)
    print('%s: max err %.3e, bound %.3e' % (what, err, bound))
    assert tuple(got.shape) == want.shape and err <= bound, (what, err, bound)


def same(a, b, what):
    """Bit for bit, and which rows / planes differ if not."""
    if not torch.equal(a, b):
        bad = (a != b).flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError('%s: %d of %d units differ from the one-unit-per-workgroup run, first %s' % (what, len(bad), a.shape[0], bad[:8]))


def batches(n, limit):
    """[(lo, hi)]: n units in the fewest runs of at most `limit`, as even as possible."""
    k = cdiv(n, limit)
    cuts = [n * i // k for i in range(k + 1)]
    return list(zip(cuts[:-1], cuts[1:]))


def boundary_sample(n, G):
    """The first and last unit, and the units either side of every boundary between groups of G."""
    s = {0, n - 1}
    for b in range(G, n, G):
        s.update((b - 1, b))
    return sorted(s)


# ---- WlDwt1dFused ---------------------------------------------------------------------------------------------------------------
def dwt1d_plan(cus, rows, N, L, J, mode):
    """(nchunks, cpw, grid) of wl_dwt1d_fused_launch for a mode that does not wrap."""
    n = N
    for _ in range(J):
        n = ops.coeff_len(n, L, mode)
    chunk = min(max(DWT1D_SPAN >> J, 2 * L), n)
    nchunks = cdiv(n, chunk)
    cpw = min(max(rows * nchunks // (10 * cus), 1), nchunks)
    return nchunks, cpw, rows * cdiv(nchunks, cpw)


def dwt1d_grad_ref(dlo, dhis, lens, h0, h1, mode):
    """The reference's backward of the level chain: the synthesis with the ANALYSIS taps, each level cropped to its input."""
    d = dlo
    for dh, n in zip(dhis[::-1], lens[::-1]):
        d = wo.sfb1d(d, dh, h0, h1, mode, axis=-1)[..., :n]
    return d


def check_dwt1d_walk(dev, cus, wave, mode, J, N, dtype, cpw, nchunks, grad=False):
    """rows = ceil(cpw * 10 * cus / nchunks) rows of N samples: `cpw` consecutive chunks per workgroup, the last workgroup of a
    row fewer.  The comparison runs hold at most (20 cus - 1) / nchunks rows: one chunk per workgroup."""
    from pytorch_wavelets_amd.dwt import lowlevel
    h0, h1 = F.dwt_analysis_taps(wave)
    L, m = len(h0), lowlevel.mode_to_int(mode)
    rows = cdiv(cpw * 10 * cus, nchunks)
    fits(rows * N * torch.empty(0, dtype=dtype).element_size(), 'WlDwt1dFused')
    plan = dwt1d_plan(cus, rows, N, L, J, m)
    assert plan[:2] == (nchunks, cpw) and plan[2] < rows * nchunks, plan
    torch.manual_seed(41)
    x = torch.randn(rows, 1, N).to(dtype).to(dev)
    xfm = pw.DWT1DForward(J=J, wave=wave, mode=mode).to(dev).to(dtype)
    name = 'WlDwt1dFused<%s, %d>' % (TNAME[dtype], L)

    def run(xs, want_grid):
        xs = xs.clone().requires_grad_(grad)
        c0 = pw.launch_count()
        yl, yh = xfm(xs)
        ks, g = pw.kernels_since(c0), last_grid()
        assert ks == [name] and g == want_grid, (ks, g, want_grid)
        outs = [yl.detach()] + [h.detach() for h in yh]
        if grad:
            cots = [torch.ones_like(yl)] + [h.detach().sign() for h in yh]     # (a function of the row alone: any batch gives the same)
            c0 = pw.launch_count()
            dx, = torch.autograd.grad([yl] + list(yh), xs, cots)
            assert pw.kernels_since(c0) == ['WlIdwt1dFused<%s, %d>' % (TNAME[dtype], L)], pw.kernels_since(c0)
            outs.append(dx)
        return outs

    full = run(x, rows * cdiv(nchunks, cpw))
    print('WlDwt1dFused %s %s J=%d N=%d %s on %d CUs: %d rows x %d chunks, cpw %d, grid %d'
          % (wave, mode, J, N, TNAME[dtype], cus, rows, nchunks, cpw, plan[2]))
    # ---- one chunk per workgroup
    parts = []
    for lo, hi in batches(rows, (20 * cus - 1) // nchunks):
        assert dwt1d_plan(cus, hi - lo, N, L, J, m)[1] == 1
        parts.append(run(x[lo:hi], (hi - lo) * nchunks))
    for i, a in enumerate(full):
        same(a, torch.cat([p[i] for p in parts]), 'WlDwt1dFused %s J=%d output %d' % (wave, J, i))
    # ---- the oracle: whole rows (a workgroup never leaves its row: every chunk boundary of a row is inside it)
    sel = sorted({0, 1, rows // 2, rows - 1})
    xs = npy(x[sel])
    oyl, oyh = wo.dwt1d_forward(xs, J, h0, h1, mode)
    close(full[0][sel], oyl, TOL[dtype], 'yl')
    for j in range(J):
        close(full[1 + j][sel], oyh[j], TOL[dtype], 'yh[%d]' % j)
    if grad:
        lens = [N] + [h.shape[-1] for h in oyh[:-1]]
        want = dwt1d_grad_ref(np.ones_like(oyl), [np.sign(npy(full[1 + j][sel])) for j in range(J)], lens, h0, h1, mode)
        close(full[-1][sel], want, TOL[dtype], 'dx')


# ---- WlAfbSmall -----------------------------------------------------------------------------------------------------------------
def align16(v):
    return (v + 15) & ~15


def afb_small_plan(cus, planes, H, W, L, J, mode):
    """(G, groups, resident, grid) of wl_afb_small_run."""
    h, w = [H], [W]
    for _ in range(J):
        h.append(ops.coeff_len(h[-1], L, mode))
        w.append(ops.coeff_len(w[-1], L, mode))
    b0, b1, mid0, most = H * W, 1, 1, 1
    for j in range(J):
        out, m = h[j + 1] * w[j + 1], h[j] * w[j + 1] * 2
        if j + 1 < J:
            if (j + 1) & 1:
                b1 = max(b1, out)
            else:
                b0 = max(b0, out)
        mid0 = max(mid0, m)
        most = max(most, h[j] * w[j + 1], out)
    G = min(max(40 * 1024 // ((b0 + b1 + mid0) * 4), 1), 16)
    while G > 1 and G * H * W > 4 * 256 * 6:
        G -= 1
    if planes // G < 2 * cus:
        G = max(planes // (2 * cus), 1)
    while G > 1 and G * most >= 65536:
        G -= 1
    lds = align16(G * b0 * 4) + align16(G * b1 * 4) + align16(G * mid0 * 4) + 16 * L
    resident = min(160 * 1024 // lds, 8) * cus
    groups = cdiv(planes, G)
    return G, groups, resident, min(groups, resident)


def check_afb_small_walk(dev, cus, wave, mode, J, hw, per_cu, extra, dtype, want_G=None, inverse=False):
    """planes = per_cu * G * cus + extra planes of hw x hw (G = the launcher's planes per group on a full chip; `extra`: whole
    groups and a short last one): more groups than the residency cap, so a workgroup walks over several, group k + nblocks
    prefetched while group k runs out of LDS.  inverse: also WlSfbSmall on the same pyramid, and the gradient (float32)."""
    from pytorch_wavelets_amd.dwt import lowlevel
    h0, h1 = F.dwt_analysis_taps(wave)
    L, m = len(h0), lowlevel.mode_to_int(mode)
    G = afb_small_plan(cus, 1 << 24, hw, hw, L, J, m)[0]
    if want_G is not None:
        assert G == want_G, (G, want_G)
    planes = per_cu * G * cus + extra(G)
    fits(planes * hw * hw * torch.empty(0, dtype=dtype).element_size(), 'WlAfbSmall')
    g_, groups, resident, grid = afb_small_plan(cus, planes, hw, hw, L, J, m)
    assert g_ == G and planes % G and grid == resident < groups, (g_, G, planes, groups, resident)
    torch.manual_seed(43)
    x = torch.randn(planes, 1, hw, hw).to(dtype).to(dev)
    xfm = pw.DWTForward(J=J, wave=wave, mode=mode).to(dev).to(dtype)
    ifm = pw.DWTInverse(wave=wave, mode=mode).to(dev).to(dtype)
    grad = inverse and dtype == F32
    LT = L if L in (2, 4, 6, 8) else 0
    A = 'WlAfbSmall<%s, %d>' % (TNAME[dtype], LT)
    S = 'WlSfbSmall<%s, %d>' % (TNAME[dtype], 0 if m == 2 else LT)

    def run(xs, want_grid):
        xs = xs.clone().requires_grad_(grad)
        c0 = pw.launch_count()
        yl, yh = xfm(xs)
        ks, g = pw.kernels_since(c0), last_grid()
        assert ks == [A] and g == want_grid, (ks, g, want_grid)
        outs = [yl.detach()] + [h.detach() for h in yh]
        if inverse:
            c0 = pw.launch_count()
            outs.append(ifm((outs[0], outs[1:])))
            assert pw.kernels_since(c0) == [S], pw.kernels_since(c0)
        if grad:
            c0 = pw.launch_count()
            dx, = torch.autograd.grad([yl] + list(yh), xs, [torch.ones_like(yl)] + [h.detach().sign() for h in yh])
            assert pw.kernels_since(c0) == [S], pw.kernels_since(c0)
            outs.append(dx)
        return outs

    full = run(x, resident)
    print('WlAfbSmall %s %s J=%d %dx%d %s on %d CUs: %d planes, G %d, %d groups, grid %d'
          % (wave, mode, J, hw, hw, TNAME[dtype], cus, planes, G, groups, resident))
    # ---- one group per workgroup
    parts = []
    for lo, hi in batches(planes, resident * G):
        pg = afb_small_plan(cus, hi - lo, hw, hw, L, J, m)
        assert pg[1] <= pg[2], pg
        parts.append(run(x[lo:hi], pg[1]))
    for i, a in enumerate(full):
        same(a, torch.cat([p[i] for p in parts]), 'WlAfbSmall %s J=%d output %d' % (wave, J, i))
    # ---- the oracle
    sel = boundary_sample(planes, G)
    assert planes - planes % G - 1 in sel and planes - planes % G in sel
    oyl, oyh = wo.dwt_forward(npy(x[sel]), J, h0, h1, h0, h1, mode)
    close(full[0][sel], oyl, TOL[dtype], 'yl')
    for j in range(J):
        close(full[1 + j][sel], oyh[j], TOL[dtype], 'yh[%d]' % j)
    if inverse:
        g0, g1 = F.dwt_synthesis_taps(wave)
        want = wo.dwt_inverse(npy(full[0][sel]), [npy(full[1 + j][sel]) for j in range(J)], g0, g1, g0, g1, mode)
        close(full[1 + J][sel], want, TOL[dtype], 'rec')
    if grad:
        # the reference's backward: the synthesis with the analysis taps, every level cropped to its input
        d = np.ones_like(oyl)
        sizes = [(hw, hw)] + [tuple(h.shape[-2:]) for h in oyh[:-1]]
        for j in range(J - 1, -1, -1):
            d = wo.afb2d_level_backward(d, np.sign(npy(full[1 + j][sel])), h0, h1, h0, h1, mode, sizes[j])
        close(full[-1][sel], d, TOL[dtype], 'dx')


# ---- WlDtFwd1Small --------------------------------------------------------------------------------------------------------------
def dt_small_plan(cus, NC, H, W, M):
    """(G, grid) of wl_dtfwd1_small_launch."""
    He, We = H + 2 * M, W + 2 * M
    G = min(max(40 * 1024 // ((He * We + 2 * He * W) * 4), 1), 16)
    if NC // G < 2 * cus:
        G = max(NC // (2 * cus), 1)
    while G > 1 and G * He * We >= 65536:
        G -= 1
    return G, cdiv(NC, G)


def check_dt_small_runs(dev, cus, biort, mode, hw, planes_of, want_G, last_run, dtype):
    """NC = planes_of(cus) planes of hw x hw behind ScatLayer and DTCWTForward(J=1): runs of want_G planes per workgroup and a
    short last run of `last_run`.  Against the tile kernels on every plane (option no_stream), bitwise against runs of one
    plane per workgroup where the chip has a plane count that gives them (the launcher takes 16 planes and more, and keeps
    runs of one below 4 planes per CU: from 5 CUs on), against the oracle on the planes either side of every run boundary."""
    h0o, _, h1o, _ = F.biort(biort)
    M = max(len(h0o), len(h1o)) // 2
    NC = planes_of(cus)
    fits(NC * hw * hw * torch.empty(0, dtype=dtype).element_size() * 8, 'WlDtFwd1Small')
    G, grid = dt_small_plan(cus, NC, hw, hw, M)
    assert G == want_G and NC % G == last_run and grid < NC, (G, NC, grid)
    torch.manual_seed(47)
    x = torch.randn(NC, 1, hw, hw).to(dtype).to(dev)
    sl = pw.ScatLayer(biort=biort, mode=mode).to(dev).to(dtype)
    xf = pw.DTCWTForward(J=1, biort=biort, mode=mode).to(dev).to(dtype)
    name = 'WlDtFwd1Small<%s, %d, %d' % (TNAME[dtype], len(h0o), len(h1o))

    def run(xs, want_grid):
        with torch.no_grad():
            c0 = pw.launch_count()
            z = sl(xs)
            ks, g1 = pw.kernels_since(c0), last_grid()
            c0 = pw.launch_count()
            yl, yh = xf(xs)
            ks += pw.kernels_since(c0)
            g2 = last_grid()
        if want_grid is None:
            assert not any('Small' in k for k in ks), ks
        else:
            assert len(ks) == 2 and all(k.startswith(name) for k in ks) and (g1, g2) == (want_grid, want_grid), (ks, g1, g2, want_grid)
        return [z, yl, yh[0]]

    full = run(x, grid)
    print('WlDtFwd1Small %s %s %dx%d %s on %d CUs: %d planes, G %d, grid %d' % (biort, mode, hw, hw, TNAME[dtype], cus, NC, G, grid))
    lib = ops._backend()
    lib.wl_set_option(b'no_stream', 1)
    try:
        tile = run(x, None)
    finally:
        lib.wl_set_option(b'no_stream', 0)
    for u, v in zip(full, tile):
        assert u.shape == v.shape
        assert float((u.float() - v.float()).abs().max()) <= TILE_TOL[dtype] * max(1.0, float(v.float().abs().max()))
    # ---- one plane per workgroup
    if 4 * cus - 1 >= 16:
        parts = []
        for lo, hi in batches(NC, 4 * cus - 1):
            assert dt_small_plan(cus, hi - lo, hw, hw, M) == (1, hi - lo)
            parts.append(run(x[lo:hi], hi - lo))
        for i, a in enumerate(full):
            same(a, torch.cat([p[i] for p in parts]), 'WlDtFwd1Small %s output %d' % (biort, i))
    # ---- the oracle
    sel = boundary_sample(NC, G)
    hp = [dl.prep_filt(v, 1).numpy().ravel() for v in (h0o, h1o)]
    xs = npy(x[sel])
    close(full[0][sel], wo.scat_layer_forward(xs, hp[0], hp[1], mode), TOL[dtype], 'ScatLayer')
    oyl, oyh = wo.dtcwt_forward(xs, 1, *F.dtcwt_forward_taps(biort, 'qshift_a'), mode=mode)
    close(full[1][sel], oyl, TOL[dtype], 'yl')
    close(full[2][sel], oyh[0], TOL[dtype], 'yh[0]')


# ---- the cases ------------------------------------------------------------------------------------------------------------------
DWT1D_CASES = {
    # three chunks per row: workgroups of 2 + 1 chunks
    'db4_J1_cpw2': dict(wave='db4', mode='symmetric', J=1, N=8400, dtype=F32, cpw=2, nchunks=3),
    # four chunks, the last of five outputs: workgroups of 3 + 1 chunks; the backward on WlIdwt1dFused
    'db4_J2_cpw3_grad': dict(wave='db4', mode='symmetric', J=2, N=12289, dtype=F32, cpw=3, nchunks=4, grad=True),
    # 20 taps in the 2-byte types: four chunks, workgroups of 2 + 2
    'db10_J3_f16': dict(wave='db10', mode='zero', J=3, N=12289, dtype=F16, cpw=2, nchunks=4),
    'db10_J2_bf16': dict(wave='db10', mode='zero', J=2, N=12289, dtype=BF16, cpw=2, nchunks=4),
}
AFB_SMALL_CASES = {
    # six groups of four planes per CU and a last group of three, on a grid of four workgroups per CU
    'db2_J2_32x32': dict(wave='db2', mode='symmetric', J=2, hw=32, per_cu=6, extra=lambda G: 3, dtype=F32, want_G=4, inverse=True),
    # eight workgroups per CU: three groups more than workgroups (those walk twice) and a last group of five planes
    'haar_J1_8x8': dict(wave='haar', mode='zero', J=1, hw=8, per_cu=8, extra=lambda G: 3 * G + 5, dtype=F32, want_G=16),
    # the run-time-tap instantiation (LT = 0, ten taps), float16: six groups per CU and a short last group
    'db5_J2_32x32_f16': dict(wave='db5', mode='symmetric', J=2, hw=32, per_cu=6, extra=lambda G: G - 1, dtype=F16),
}
DT_SMALL_CASES = {
    # (the launcher takes 16 planes and more: on a chip of fewer than four CUs the run of two starts there)
    'near_sym_a_32x32': dict(biort='near_sym_a', mode='symmetric', hw=32, planes_of=lambda cus: max(4 * cus, 16) + 1, want_G=2, last_run=1, dtype=F32),
    'near_sym_a_32x32_f16': dict(biort='near_sym_a', mode='symmetric', hw=32, planes_of=lambda cus: max(4 * cus, 16) + 1, want_G=2, last_run=1, dtype=F16),
    'legall_16x16': dict(biort='legall', mode='zero', hw=16, planes_of=lambda cus: 9 * 2 * cus + 5, want_G=9, last_run=5, dtype=F32),
}
