"""Shared checks of the transposed a-trous bank (wl_iswt2d_level / wl_corr1d_adj), SWTForward's gradient and SWTInverse, run by
the emulator (CPU) and the GPU test modules.

The checker is built from the pinned oracle alone: the dense matrices A_b of the analysis along one axis are what
``wo.afb1d_atrous`` makes of an identity; the expected gradient is their transpose, the expected inverse
1/4 sum_{r,b} A_b(g_col)^T Y_rb A_r(g_row) with the stored synthesis taps g.

Tolerances: those of tests/test_ext_emu.py::test_swt_level_kernel_vs_oracle - 1e-12 (float64), 2e-6 (float32), 3e-3 (float16)
times max(1, |ref|max); bfloat16 by the rule of tests/_bf16_cases.py (relative to |ref|max: 4e-3 for one level out of rounded
inputs, 3e-2 for chains)."""
import numpy as np
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters
from pytorch_wavelets_amd.dwt import lowlevel as dwl
from pytorch_wavelets_amd.dwt.transform2d import SWTForward

TOL = {torch.float64: 1e-12, torch.float32: 2e-6, torch.float16: 3e-3}
BF_ONE, BF_MULTI = 4e-3, 3e-2          # tests/_bf16_cases.py
MODES = ('periodic', 'zero', 'constant', 'symmetric', 'reflect', 'replicate')
FUSED_MODES = ('periodic', 'zero', 'constant')   # the rules wl_iswt2d_level takes itself; the others it hands to wl_corr1d_adj


def amat(h0, h1, n, mode, d):
    """(A_0, A_1): the K x n matrices of afb1d_atrous along an axis of n samples (columns = responses to unit samples)."""
    lo, hi = wo.afb1d_atrous(np.eye(n), h0, h1, 'zero' if mode == 'constant' else mode, 0, d)
    return lo, hi


def adj2d_ref(y, row, col, mode, d, hw):
    """The transpose of wo.afb2d_atrous: y (N,4C,Kh,Kw) float64 -> (N,C,H,W); row / col = (h0, h1) along W / H."""
    H, W = hw
    Ar, Ac = amat(row[0], row[1], W, mode, d), amat(col[0], col[1], H, mode, d)
    N, C4 = y.shape[:2]
    out = np.zeros((N, C4 // 4, H, W))
    for r in (0, 1):
        for b in (0, 1):
            out += Ac[b].T @ y[:, 2 * r + b::4] @ Ar[r]
    return out


def inv_ref(coeffs, g_row, g_col):
    """The inverse by its matrix formula: coeffs[j] (N,4C,H,W) float64, finest first; g = the stored synthesis taps."""
    J = len(coeffs)
    ll = coeffs[-1][:, 0::4]
    for j in range(J - 1, -1, -1):
        y = coeffs[j].copy()
        y[:, 0::4] = ll
        ll = 0.25 * adj2d_ref(y, g_row, g_col, 'periodic', 2 ** j, y.shape[-2:])
    return ll


def taps_t(hs, dev, dtype=torch.float64):
    return tuple(torch.tensor(np.ascontiguousarray(h), dtype=dtype, device=dev) for h in hs)


def filts4(row, col, dev):
    """(h0_col, h1_col, h0_row, h1_row) as prepared tensors (1,1,L,1) / (1,1,1,L)."""
    c0, c1 = taps_t(col, dev)
    r0, r1 = taps_t(row, dev)
    return c0.reshape(1, 1, -1, 1), c1.reshape(1, 1, -1, 1), r0.reshape(1, 1, 1, -1), r1.reshape(1, 1, 1, -1)


def npy(t):
    return t.detach().cpu().double().numpy()


def close(a, ref, dtype, what=''):
    err = float(np.abs(npy(a) - ref).max())
    bound = TOL[dtype] * max(1.0, float(np.abs(ref).max()))
    print('%s: max err %.3e, bound %.3e' % (what, err, bound))
    assert tuple(a.shape) == ref.shape and a.dtype == dtype, (a.shape, ref.shape, a.dtype)
    assert err <= bound, (what, err, bound)


def check_adjoint(dev, wave_row, wave_col, mode, d, shape, dtype, fused=True, seed=5):
    """The gradient of afb2d_atrous (autograd) and the two ll modes of the transposed level (ll = every 4th channel of
    another level's tensor, not copied) against the oracle's transpose; and which kernels ran."""
    rng = np.random.RandomState(seed)
    row, col = filters.dwt_analysis_taps(wave_row), filters.dwt_analysis_taps(wave_col)
    N, C, H, W = shape
    dy = torch.tensor(rng.randn(N, 4 * C, H, W)).to(dtype).to(dev)
    other = torch.tensor(rng.randn(N, 4 * C, H, W)).to(dtype).to(dev)
    dyn, lln = npy(dy), npy(other)[:, 0::4]
    ref = adj2d_ref(dyn, row, col, mode, d, (H, W))
    filts = filts4(row, col, dev)
    expect_fused = fused and mode in FUSED_MODES
    x = torch.zeros(shape, dtype=dtype, device=dev, requires_grad=True)
    y = dwl.afb2d_atrous(x, filts, mode, d)
    assert y.grad_fn is not None
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(y, x, dy)
    ks = pw.kernels_since(c0)
    if expect_fused:
        assert len(ks) == 1 and ks[0].startswith('WlSwtInvLevel'), ks
    else:
        assert len(ks) == 3 and all(k.startswith('WlCorr1dAdj') for k in ks), ks
    close(dx, ref, dtype, 'dx %s %s d=%d' % (wave_row, mode, d))
    # the ll plane from elsewhere: replaced / added, read through its plane stride
    t_row, t_col = (filts[2], filts[3]), (filts[0], filts[1])
    ext = dwl._ATROUS_EXT[mode]
    for ll_mode in (1, 2):
        yn = dyn.copy()
        yn[:, 0::4] = lln if ll_mode == 1 else yn[:, 0::4] + lln
        c0 = pw.launch_count()
        got = dwl._atrous_level_adj(dy, other[:, 0::4], ll_mode, t_row, t_col, ext, d, 0.25, (H, W))
        ks = pw.kernels_since(c0)
        assert ks[0].startswith('WlSwtInvLevel' if expect_fused else 'WlCorr1dAdj'), ks
        close(got, 0.25 * adj2d_ref(yn, row, col, mode, d, (H, W)), dtype, 'll_mode %d' % ll_mode)
    # no y at all: the three other bands are zeros
    yn = np.zeros_like(dyn)
    yn[:, 0::4] = lln
    got = dwl._atrous_level_adj(None, other[:, 0::4], 1, t_row, t_col, ext, d, 1.0, (H, W))
    close(got, adj2d_ref(yn, row, col, mode, d, (H, W)), dtype, 'll only')


def check_adjoint_1d(dev, wave, mode, d, shape, dim, dtype, seed=6):
    """afb1d_atrous's gradient (wl_corr1d_adj) against the transpose, along either axis."""
    rng = np.random.RandomState(seed)
    h0, h1 = filters.dwt_analysis_taps(wave)
    x = torch.tensor(rng.randn(*shape)).to(dtype).to(dev).requires_grad_(True)
    t0, t1 = taps_t((h0, h1), dev)
    y = dwl.afb1d_atrous(x, t0, t1, mode, dim, d)
    dy = torch.tensor(rng.randn(*y.shape)).to(dtype).to(dev)
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(y, x, dy)
    assert pw.kernels_since(c0)[-1].startswith('WlCorr1dAdj'), pw.kernels_since(c0)
    A0, A1 = amat(h0, h1, shape[dim], mode, d)
    dyn = np.moveaxis(npy(dy), dim, -1)
    ref = np.moveaxis(dyn[:, 0::2] @ A0 + dyn[:, 1::2] @ A1, -1, dim)
    close(dx, ref, dtype, 'dx1d %s %s d=%d' % (wave, mode, d))


def swt_modules(dev, wave_f, wave_i, J, mode='periodic', dtype=torch.float64):
    """(SWTForward, SWTInverse) holding their taps in `dtype` (float64 modules are built under a float64 default dtype: the
    buffers of a float32 module converted afterwards carry taps rounded to float32)."""
    from pytorch_wavelets_amd.dwt.transform2d import SWTInverse
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return SWTForward(J=J, wave=wave_f, mode=mode).to(dev), SWTInverse(wave=wave_i, mode='periodic').to(dev)
    finally:
        torch.set_default_dtype(prev)


def check_roundtrip(dev, wave, J, shape, dtype, seed=7, waves=None):
    """SWTInverse(SWTForward(x)) == x, one WlSwtInvLevel launch per level.  `waves` = (forward bank, inverse bank) when the
    row and the column filters differ."""
    rng = np.random.RandomState(seed)
    wf, wi = waves if waves is not None else (wave, wave)
    xfm, ifm = swt_modules(dev, wf, wi, J, dtype=torch.float64 if dtype == torch.float64 else torch.float32)
    x = torch.tensor(rng.randn(*shape)).to(dtype).to(dev)
    coeffs = xfm(x)
    c0 = pw.launch_count()
    rec = ifm(coeffs)
    ks = pw.kernels_since(c0)
    assert len(ks) == J and all(k.startswith('WlSwtInvLevel') for k in ks), ks
    err = float((rec.double() - x.double()).abs().max())
    bound = TOL[dtype] * max(1.0, float(x.abs().max()))
    print('round trip %s J=%d %s: max err %.3e, bound %.3e' % (wave, J, dtype, err, bound))
    assert rec.shape == x.shape and rec.dtype == dtype
    assert err <= bound, (err, bound)
    return coeffs, rec


def reversed_db2():
    """Two different 4-tap banks for the two axes: db2 along H, its time reverse (also orthogonal) along W - as the tuples
    SWTForward (dec filters) and SWTInverse (rec filters) take: (col lo, col hi, row lo, row hi)."""
    w = filters.Wavelet('db2')
    return (w.dec_lo, w.dec_hi, w.rec_lo, w.rec_hi), (w.rec_lo, w.rec_hi, w.dec_lo, w.dec_hi)


def check_bf16(dev, shape):
    """bfloat16 data takes the float16 kernels (fp32 taps and accumulators): the same launches, outputs within the bounds of
    tests/_bf16_cases.py of the matrix formulas on the rounded inputs (a float32 module: exact float32 taps)."""
    F16, BF16 = torch.float16, torch.bfloat16
    rng = np.random.RandomState(12)
    N, C, H, W = shape
    g, h = filters.dwt_synthesis_taps('db2'), filters.dwt_analysis_taps('db2')
    g32, h32 = ([np.asarray(v, dtype=np.float32).astype(np.float64) for v in t] for t in (g, h))
    xfm, ifm = swt_modules(dev, 'db2', 'db2', 2, dtype=torch.float32)
    names = {}
    for dt in (F16, BF16):
        coeffs = [torch.tensor(rng.randn(N, 4 * C, H, W)).to(dt).to(dev) for _ in range(2)]
        c0 = pw.launch_count()
        rec = ifm(coeffs)
        names[dt] = pw.kernels_since(c0)
        assert rec.dtype == dt
        ref = inv_ref([npy(c) for c in coeffs], g32, g32)
        rel = float(np.abs(npy(rec) - ref).max() / np.abs(ref).max())
        print('%s inverse rel %.3e' % (dt, rel))
        assert rel <= BF_MULTI
        x = torch.zeros(N, C, H, W, device=dev, dtype=dt, requires_grad=True)
        y = xfm(x)[0]
        dy = torch.tensor(rng.randn(*y.shape)).to(dt).to(dev)
        c0 = pw.launch_count()
        dx, = torch.autograd.grad(y, x, dy)
        names[dt] += pw.kernels_since(c0)
        assert dx.dtype == dt
        ref = adj2d_ref(npy(dy), h32, h32, 'periodic', 1, (H, W))
        rel = float(np.abs(npy(dx) - ref).max() / np.abs(ref).max())
        print('%s dx rel %.3e' % (dt, rel))
        assert rel <= BF_ONE
    assert names[BF16] == [k.replace('_Float16', '__bf16') for k in names[F16]], names
    assert all(k.startswith('WlSwtInvLevel<__bf16') for k in names[BF16]), names
