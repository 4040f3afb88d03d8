"""Shared checks of the 1-D stationary transform - SWT1DForward / SWT1DInverse, lowlevel.swt1d / iswt1d, their gradients and the
wave-tile kernels of csrc/wl_swt1d.h -, run by the emulator (CPU) and the GPU test modules.

Expected values come from the pinned oracle alone: level j is ``wo.afb1d_atrous`` with dilation 2**(j-1), chained in float64 on
the module's own (float32) taps.  The inverse and the gradients are the transposed matrices A_b^T that ``wo.afb1d_atrous`` makes
of an identity (tests/_swt_inv_cases.py).  A periodic bank is a circulant, whose transpose is itself between two index
reversals: rows too long for a dense identity use that form, and check_transpose_forms ties it to the matrices.

Tolerances (tests/_ext_cases.py::check_dwt1d_fused, tests/_bf16_cases.py): values relative to |ref|max - 1e-5 float32, 4e-3
float16, 3e-2 bfloat16 -; reconstructions absolute, times max(1, |x|max) - 2e-5 float32, 6e-3 float16."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import _lib, filters, ops

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
REL = {F64: 1e-12, F32: 1e-5, F16: 4e-3, BF16: 3e-2}
REC = {F64: 1e-12, F32: 2e-5, F16: 6e-3}
WAVES = ('haar', 'bior2.2', 'db4', 'db10')
LEVELS = (1, 2, 3, 5)
ROWS = ((1, 3), (2, 2))
OTHER_MODES = ('zero', 'constant', 'symmetric', 'reflect', 'replicate')
ODD_PAIR = ([0.1, 0.25, 0.3, 0.25, 0.1], [-0.1, -0.2, 0.6, -0.2, -0.1])      # (dec_lo, dec_hi): five taps


def ntaps(wave):
    return len(filters.dwt_analysis_taps(wave)[0])


def lens(wave, J):
    """The lengths at which a piece of the kernel can go wrong: rows shorter than the filter and the halo (several wraps inside
    a tile), rows that lose 16-byte alignment from the second row on, exactly one tile, one position into a second, three."""
    core = ops.swt1d_core(ntaps(wave), min(J, ops.SWT1D_MAXJ))
    return (1, 3, 5, 37, 64, core - 1, core, core + 1, 2 * core + 3)


def f32taps(pair):
    """The taps as a float32 module holds them, in float64."""
    return tuple(np.asarray(h, dtype=np.float32).astype(np.float64) for h in pair)


def ana_taps(wave):
    return f32taps(filters.dwt_analysis_taps(wave))


def syn_taps(wave):
    return f32taps(filters.dwt_synthesis_taps(wave))


def npy(t):
    return t.detach().cpu().double().numpy()


def analysis_ref(x, taps, J, mode='periodic', scale=1.0):
    """(lo_J, [hi_1 ..]): scale * wo.afb1d_atrous per level, chained."""
    lo, his = x, []
    for j in range(J):
        lo, hi = wo.afb1d_atrous(lo, taps[0], taps[1], 'zero' if mode == 'constant' else mode, -1, 2 ** j)
        lo, hi = scale * lo, scale * hi
        his.append(hi)
    return lo, his


@functools.lru_cache(maxsize=None)
def _amat(t0, t1, n, d):
    """(A_0, A_1): the n x n matrices of the periodic bank of dilation d - what the oracle makes of an identity."""
    return wo.afb1d_atrous(np.eye(n), np.array(t0), np.array(t1), 'periodic', 0, d)


def transposed(lo, hi, taps, d, dense=None):
    """A_0^T lo + A_1^T hi along the last axis, periodic: the matrices of an identity, or (long rows) the circulant form."""
    n = lo.shape[-1]
    if dense is None:
        dense = n <= 160
    if dense:
        A0, A1 = _amat(tuple(taps[0]), tuple(taps[1]), n, d)
        return lo @ A0 + hi @ A1
    r0 = wo.afb1d_atrous(lo[..., ::-1], taps[0], taps[1], 'periodic', -1, d)[0]
    r1 = wo.afb1d_atrous(hi[..., ::-1], taps[0], taps[1], 'periodic', -1, d)[1]
    return (r0 + r1)[..., ::-1]


def adjoint_ref(lo, his, taps, scale):
    """The transposed cascade, coarsest first: his finest first, None = zeros."""
    for j in range(len(his) - 1, -1, -1):
        hi = np.zeros_like(lo) if his[j] is None else his[j]
        lo = scale * transposed(lo, hi, taps, 2 ** j)
    return lo


def check_transpose_forms():
    """The circulant form of the transpose is the matrix form (what long rows are checked against)."""
    rng = np.random.RandomState(3)
    for wave in WAVES:
        for n, d in ((37, 1), (64, 2), (5, 4), (64, 4), (1, 2)):
            lo, hi = rng.randn(2, n), rng.randn(2, n)
            a, b = transposed(lo, hi, ana_taps(wave), d, True), transposed(lo, hi, ana_taps(wave), d, False)
            assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(a).max()), (wave, n, d)


def check_oracle_reconstructs():
    """The definition inverts: the oracle's chain followed by 1/2 (A_0(g)^T lo + A_1(g)^T hi) per level gives x back."""
    rng = np.random.RandomState(4)
    for wave in WAVES:
        for n in (1, 5, 37, 64):
            x = rng.randn(2, n)
            lo, his = analysis_ref(x, filters.dwt_analysis_taps(wave), 3)
            rec = adjoint_ref(lo, his, filters.dwt_synthesis_taps(wave), 0.5)
            assert np.abs(rec - x).max() <= 1e-13, (wave, n)


def cancel_floor(taps, *sources):
    """What float32 accumulation may leave of a band that cancels (the highpass of a constant row - every row of one sample - is
    0 in exact arithmetic, and a bound relative to |ref|max is then no bound): the a-priori error of an L-term float32 dot
    product, (L + 1) 2^-24 sum|h| |source|max, over the signals the levels read.  It is below the relative bound of any band
    that reaches a quarter of its source's size."""
    L = len(taps[0])
    return (L + 1) * 2.0 ** -24 * max(np.abs(taps[0]).sum(), np.abs(taps[1]).sum()) * max(float(np.abs(v).max()) for v in sources)


def close(a, ref, dtype, what, tol=None, floor=0.0):
    tol = REL[dtype] if tol is None else tol
    err = float(np.abs(npy(a) - ref).max())
    bound = max(tol * float(np.abs(ref).max()), floor)
    print('%s: max err %.3e, bound %.3e' % (what, err, bound))
    assert tuple(a.shape) == ref.shape and a.dtype == dtype, (what, a.shape, ref.shape, a.dtype)
    assert err <= bound, (what, err, bound)


def modules(dev, wave, J, mode='periodic'):
    return pw.SWT1DForward(J=J, wave=wave, mode=mode).to(dev), pw.SWT1DInverse(wave=wave).to(dev)


def names_since(c0):
    return [k.split('<')[0] for k in pw.kernels_since(c0)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, J, seed):
    """x, the coefficients of a random inverse / the cotangents of a forward (yl, yh), and a cotangent of the inverse: float64
    numpy, made once per shape and shared (never written to)."""
    rng = np.random.RandomState(seed)
    return rng.randn(*shape), rng.randn(*shape), [rng.randn(*shape) for _ in range(J)], rng.randn(*shape)


def dev_t(a, dtype, dev):
    return torch.tensor(a).to(dtype).to(dev)


def check_forward(dev, wave, J, shape, dtype=F32):
    """yl and every yh[j] against the oracle; one WlSwt1dFwd launch for J <= 3, one plus the composed levels beyond."""
    x = dev_t(_inputs(shape, J, 11)[0], dtype, dev)
    xfm = modules(dev, wave, J)[0]
    c0 = pw.launch_count()
    yl, yh = xfm(x)
    ks = names_since(c0)
    assert ks == ['WlSwt1dFwd'] + ['WlCorr1d'] * (J - min(J, 3)), (wave, J, shape, ks)
    rl, rh = analysis_ref(npy(x), ana_taps(wave), J)
    assert len(yh) == J
    floor = cancel_floor(ana_taps(wave), npy(x), *[analysis_ref(npy(x), ana_taps(wave), j)[0] for j in range(1, J)])
    close(yl, rl, dtype, 'yl %s J=%d %s' % (wave, J, shape))
    for j in range(J):
        close(yh[j], rh[j], dtype, 'yh[%d] %s J=%d %s' % (j, wave, J, shape), floor=floor)
        assert yh[j].is_contiguous()
    return x, yl, yh


def check_inverse(dev, wave, J, shape, dtype=F32, coeffs=None):
    """The round trip, and the inverse of random coefficients - every level, a None level, all None - against the matrix form."""
    xfm, ifm = modules(dev, wave, J)
    if coeffs is not None and dtype in REC:
        x, yl, yh = coeffs
        c0 = pw.launch_count()
        rec = ifm((yl, yh))
        ks = names_since(c0)
        assert ks == ['WlCorr1dAdj'] * (J - min(J, 3)) + ['WlSwt1dAdj'], (wave, J, shape, ks)
        err = float((rec.double() - x.double()).abs().max())
        bound = REC[dtype] * max(1.0, float(x.abs().max()))
        print('round trip %s J=%d %s %s: max err %.3e, bound %.3e' % (wave, J, shape, dtype, err, bound))
        assert rec.shape == x.shape and rec.dtype == dtype and err <= bound, (wave, J, shape, err, bound)
    _, cl, ch, _ = _inputs(shape, J, 12)
    g = syn_taps(wave)
    tl, th = dev_t(cl, dtype, dev), [dev_t(h, dtype, dev) for h in ch]
    drops = [(), (J - 1,), tuple(range(J))] if J > 1 else [(), (0,)]
    for drop in drops:
        hs = [None if j in drop else th[j] for j in range(J)]
        ref = adjoint_ref(npy(tl), [None if h is None else npy(h) for h in hs], g, 0.5)
        close(ifm((tl, hs)), ref, dtype, 'inverse %s J=%d %s without %s' % (wave, J, shape, drop))


def check_gradients(dev, wave, J, shape, dtype=F32):
    """dx of the forward from random (dyl, dyh), and (dyl, dyh) of the inverse from a random dx, against the transposed matrices;
    each backward is one launch of the other kernel for J <= 3."""
    xn, cl, ch, cx = _inputs(shape, J, 12)
    xfm, ifm = modules(dev, wave, J)
    x = dev_t(xn, dtype, dev).requires_grad_(True)
    yl, yh = xfm(x)
    dl, dh = dev_t(cl, dtype, dev), [dev_t(h, dtype, dev) for h in ch]
    c0 = pw.launch_count()
    dx, = torch.autograd.grad([yl] + list(yh), x, [dl] + dh)
    ks = names_since(c0)
    assert ks == ['WlCorr1dAdj'] * (J - min(J, 3)) + ['WlSwt1dAdj'], (wave, J, shape, ks)
    close(dx, adjoint_ref(npy(dl), [npy(h) for h in dh], ana_taps(wave), 1.0), dtype, 'dx %s J=%d %s' % (wave, J, shape))
    # the inverse, its middle level (J > 1) absent
    tl = dev_t(cl, dtype, dev).requires_grad_(True)
    th = [None if (J > 1 and j == J // 2) else dev_t(h, dtype, dev).requires_grad_(True) for j, h in enumerate(ch)]
    rec = ifm((tl, th))
    dy = dev_t(cx, dtype, dev)
    live = [tl] + [h for h in th if h is not None]
    c0 = pw.launch_count()
    grads = torch.autograd.grad(rec, live, dy)
    ks = names_since(c0)
    assert ks[0] == 'WlSwt1dFwd' and 'WlSwt1dAdj' not in ks and sum(k == 'WlCorr1d' for k in ks) == J - min(J, 3), (wave, J, ks)
    rl, rh = analysis_ref(npy(dy), syn_taps(wave), J, scale=0.5)
    floor = cancel_floor(syn_taps(wave), npy(dy))          # (every level halves: no later source is larger)
    close(grads[0], rl, dtype, 'd yl of the inverse %s J=%d %s' % (wave, J, shape))
    it = iter(grads[1:])
    for j, h in enumerate(th):
        if h is not None:
            close(next(it), rh[j], dtype, 'd yh[%d] of the inverse %s J=%d' % (j, wave, J), floor=floor)


def check_grid(dev, wave, J):
    """Every length and row count of the table, float32: values, round trip, inverse, gradients."""
    for n in lens(wave, J):
        for lead in ROWS:
            got = check_forward(dev, wave, J, lead + (n,))
            check_inverse(dev, wave, J, lead + (n,), coeffs=got)
            check_gradients(dev, wave, J, lead + (n,))


def check_two_byte(dev, wave, dtype):
    J = 3
    core = ops.swt1d_core(ntaps(wave), J)
    for n in (37, core + 1):
        got = check_forward(dev, wave, J, (2, 2, n), dtype)
        check_inverse(dev, wave, J, (2, 2, n), dtype, coeffs=got)
        check_gradients(dev, wave, J, (2, 2, n), dtype)


GRID_WAVES = tuple('db%d' % i for i in range(1, 11))        # L = 2, 4, .., 20: one case of the dispatchers' switch each
GRID_DTYPES = (F32, F16, BF16)
TNAME = {F32: 'float', F16: '_Float16', BF16: '__bf16'}


def check_instantiation(dev, wave, dtype):
    """WlSwt1dFwd<T, L> / WlSwt1dAdj<T, L> of one tap count and element type x nlev 1..3 through ops.swt1d_fwd / swt1d_adj: three
    rows of one tile plus one position, which crosses the seam.  The kernel names are built from (T, L)."""
    L = ntaps(wave)
    h = ana_taps(wave)
    for nlev in (1, 2, 3):
        n = ops.swt1d_core(L, nlev) + 1
        xn, cl, ch, _ = _inputs((3, n), nlev, 21)
        th = [dev_t(t, F32, dev) for t in h]
        x, tl, ths = dev_t(xn, dtype, dev), dev_t(cl, dtype, dev), [dev_t(v, dtype, dev) for v in ch]
        c0 = pw.launch_count()
        lo, his = ops.swt1d_fwd(x, th[0], th[1], nlev)
        y = ops.swt1d_adj(tl, ths, th[0], th[1], 0.5)
        ks = pw.kernels_since(c0)
        assert ks == ['WlSwt1d%s<%s, %d>' % (k, TNAME[dtype], L) for k in ('Fwd', 'Adj')], ks
        what = '%s nlev=%d %s' % (wave, nlev, dtype)
        rl, rh = analysis_ref(npy(x), h, nlev)
        floor = cancel_floor(h, npy(x), *[analysis_ref(npy(x), h, j)[0] for j in range(1, nlev)])
        close(lo, rl, dtype, 'lo ' + what)
        for j in range(nlev):
            close(his[j], rh[j], dtype, 'hi[%d] %s' % (j, what), floor=floor)
        close(y, adjoint_ref(npy(tl), [npy(v) for v in ths], h, 0.5), dtype, 'adjoint ' + what)


def fused_pair(dev, wave, J, shape, dtype, origin):
    """(lo, his, y): ops.swt1d_fwd of x and ops.swt1d_adj of random bands, the first tile moved left by `origin`."""
    xn, cl, ch, _ = _inputs(shape, J, 13)
    h = [dev_t(t, F32, dev) for t in ana_taps(wave)]
    lo, his = ops.swt1d_fwd(dev_t(xn, dtype, dev), h[0], h[1], J, origin=origin)
    y = ops.swt1d_adj(dev_t(cl, dtype, dev), [dev_t(v, dtype, dev) for v in ch], h[0], h[1], 0.5, origin=origin)
    return [lo] + his + [y]


def check_origin(dev, wave, J, dtype=F32):
    """The seams of a row fall elsewhere: not a bit changes, forward and adjoint."""
    core = ops.swt1d_core(ntaps(wave), J)
    for n in (core + 1, 2 * core + 3, 37):
        base = fused_pair(dev, wave, J, (2, 1, n), dtype, 0)
        for origin in (1, 5, core // 2):
            got = fused_pair(dev, wave, J, (2, 1, n), dtype, origin)
            assert all(torch.equal(a, b) for a, b in zip(got, base)), (wave, J, n, origin)


def schedule_case(dev):
    """One forward + inverse + gradient (db4, J = 3, (2, 1, core + 1)): everything that comes out, for a bitwise comparison."""
    n = ops.swt1d_core(8, 3) + 1
    xn, cl, ch, _ = _inputs((2, 1, n), 3, 14)
    xfm, ifm = modules(dev, 'db4', 3)
    x = dev_t(xn, F32, dev).requires_grad_(True)
    yl, yh = xfm(x)
    rec = ifm((yl, yh))
    dx, = torch.autograd.grad(rec, x, dev_t(cl, F32, dev))
    return [yl.detach()] + [h.detach() for h in yh] + [rec.detach(), dx]


def check_unfused_routes(dev):
    """The other five modes, an odd tap count and float64: the oracle's answers, and none of the wave-tile kernels."""
    xn = _inputs((2, 2, 45), 3, 15)[0]
    for mode in OTHER_MODES:
        for wave in ('db4', 'bior2.2'):
            xfm = pw.SWT1DForward(J=3, wave=wave, mode=mode).to(dev)
            c0 = pw.launch_count()
            yl, yh = xfm(dev_t(xn, F32, dev))
            assert names_since(c0) == ['WlCorr1d'] * 3, (mode, names_since(c0))
            rl, rh = analysis_ref(xn.astype(np.float32).astype(np.float64), ana_taps(wave), 3, mode)
            close(yl, rl, F32, 'yl %s %s' % (wave, mode))
            for j in range(3):
                close(yh[j], rh[j], F32, 'yh[%d] %s %s' % (j, wave, mode))
    for mode in ('periodic', 'symmetric'):
        xfm = pw.SWT1DForward(J=2, wave=ODD_PAIR, mode=mode).to(dev)
        c0 = pw.launch_count()
        x = dev_t(xn, F32, dev).requires_grad_(True)
        yl, yh = xfm(x)
        taps = f32taps([h[::-1] for h in ODD_PAIR])
        rl, rh = analysis_ref(npy(x), taps, 2, mode)
        close(yl, rl, F32, 'yl odd taps %s' % mode)
        for j in range(2):
            close(yh[j], rh[j], F32, 'yh[%d] odd taps %s' % (j, mode))
        torch.autograd.grad([yl] + list(yh), x, [torch.ones_like(yl)] + [torch.ones_like(h) for h in yh])
        assert not any(k.startswith('WlSwt1d') for k in names_since(c0)), names_since(c0)
    for wave in ('db4', 'db10'):
        for n in (5, 45):
            x = dev_t(_inputs((2, 2, n), 3, 15)[0], F64, dev)
            prev = torch.get_default_dtype()
            torch.set_default_dtype(F64)
            try:
                xfm, ifm = modules(dev, wave, 3)
            finally:
                torch.set_default_dtype(prev)
            c0 = pw.launch_count()
            yl, yh = xfm(x)
            rec = ifm((yl, yh))
            assert not any(k.startswith('WlSwt1d') for k in names_since(c0)), names_since(c0)
            rl, rh = analysis_ref(npy(x), filters.dwt_analysis_taps(wave), 3)
            close(yl, rl, F64, 'yl float64 %s' % wave)
            for j in range(3):
                close(yh[j], rh[j], F64, 'yh[%d] float64 %s' % (j, wave))
            assert float((rec - x).abs().max()) <= 1e-12


def check_switch(dev, dtype=F32):
    """ops.SWT1D_FUSED = False: level by level, the same answers within the tolerance."""
    for wave, n in (('db4', 37), ('db10', ops.swt1d_core(20, 3) + 1)):
        xn, cl, ch, _ = _inputs((2, 2, n), 3, 16)
        xfm, ifm = modules(dev, wave, 3)
        outs = {}
        for flag in (True, False):
            prev = ops.SWT1D_FUSED
            ops.SWT1D_FUSED = flag
            try:
                x = dev_t(xn, dtype, dev).requires_grad_(True)
                c0 = pw.launch_count()
                yl, yh = xfm(x)
                rec = ifm((yl, yh))
                dx, = torch.autograd.grad([yl] + list(yh), x, [dev_t(cl, dtype, dev)] + [dev_t(h, dtype, dev) for h in ch])
                ks = names_since(c0)
            finally:
                ops.SWT1D_FUSED = prev
            assert any(k.startswith('WlSwt1d') for k in ks) == flag, (flag, ks)
            outs[flag] = [yl] + list(yh) + [rec, dx]
        for i, (a, b) in enumerate(zip(outs[True], outs[False])):
            ref = npy(b)
            close(a, ref, dtype, 'fused against level by level %s output %d' % (wave, i))


def check_gradcheck(dev):
    """torch.autograd.gradcheck of both modules on the float64 (composed) path."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        xfm, ifm = modules(dev, 'db2', 2)
    finally:
        torch.set_default_dtype(prev)
    rng = np.random.RandomState(17)
    x = dev_t(rng.randn(1, 2, 12), F64, dev).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: tuple([xfm(v)[0]] + xfm(v)[1]), (x,), eps=1e-6, atol=1e-7)
    cs = [dev_t(rng.randn(1, 2, 12), F64, dev).requires_grad_(True) for _ in range(3)]
    assert torch.autograd.gradcheck(lambda a, b, c: ifm((a, [b, c])), tuple(cs), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, c: ifm((a, [None, c])), (cs[0], cs[2]), eps=1e-6, atol=1e-7)


def check_errors_and_edges(dev):
    x = dev_t(_inputs((2, 2, 20), 1, 18)[0], F32, dev)
    yl, yh = pw.SWT1DForward(J=0, wave='db2').to(dev)(x)
    assert yl is x and yh == []
    assert pw.SWT1DInverse(wave='db2').to(dev)((x, [])) is x
    with pytest.raises(ValueError, match='Unkown pad type'):
        pw.SWT1DForward(J=1, wave='db2', mode='periodization').to(dev)(x)
    with pytest.raises(ValueError, match="'periodic' only"):
        pw.SWT1DInverse(wave='db2', mode='symmetric').to(dev)((x, [x]))
    with pytest.raises(ValueError, match='even number of taps'):
        pw.SWT1DInverse(wave=ODD_PAIR).to(dev)((x, [x]))
    with pytest.raises(ValueError):
        pw.SWT1DForward(J=1, wave='db2').to(dev)(x[None])
    with pytest.raises(ValueError):
        pw.SWT1DInverse(wave='db2').to(dev)((x[None], [x[None]]))
    with pytest.raises(ValueError):
        pw.SWT1DInverse(wave='db2').to(dev)((x, [x[..., 1:]]))
    # the C entries outside their envelope decline: the wrappers return None
    h = [dev_t(t, F32, dev) for t in ana_taps('db2')]
    assert ops.swt1d_fwd(x.double(), h[0], h[1], 1) is None and ops.swt1d_fwd(x, h[0], h[1], 4) is None
    assert ops.swt1d_fwd(x, h[0][:3], h[1][:3], 1) is None and ops.swt1d_adj(x, [x] * 4, h[0], h[1], 0.5) is None
    be, unsupported = ops._backend(), _lib.WL_ERR_UNSUPPORTED
    ptrs = (ctypes.c_void_p * 3)(x.data_ptr(), x.data_ptr(), x.data_ptr())
    args = (x.data_ptr(), x.data_ptr(), ptrs, 0, 4, 20, 1, h[0].data_ptr(), h[1].data_ptr(), 4)
    assert be.wl_swt1d_analysis(*(args + (ops.EXT_SYM, 1.0, 0, None))) == unsupported          # not periodic
    assert be.wl_swt1d_analysis(*(args[:3] + (2,) + args[4:] + (ops.EXT_PERIODIC, 1.0, 0, None))) == unsupported   # float64
    assert be.wl_swt1d_analysis(*(args[:-1] + (22, ops.EXT_PERIODIC, 1.0, 0, None))) == unsupported      # 22 taps
    assert be.wl_swt1d_analysis(*(args + (ops.EXT_PERIODIC, 1.0, ops.swt1d_core(4, 1), None))) != 0        # origin past the core


def check_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.SWT1DForward(J=2, wave='db2')(torch.zeros(1, 1, 16))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.SWT1DInverse(wave='db2')((torch.zeros(1, 1, 16), [torch.zeros(1, 1, 16)]))


def check_views(dev):
    """x[..., 1:-1] and x[:, 1:] give the answers of their contiguous copies, bit for bit."""
    n = ops.swt1d_core(8, 3) + 3
    base = dev_t(_inputs((2, 3, n), 3, 19)[0], F32, dev)
    xfm, ifm = modules(dev, 'db4', 3)
    other = base.flip(-1)
    for cut in (lambda t: t[..., 1:-1], lambda t: t[:, 1:]):
        view, hv = cut(base), cut(other)
        assert not view.is_contiguous() and not hv.is_contiguous()
        a, b = xfm(view), xfm(view.contiguous())
        assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
        assert torch.equal(ifm((view, [hv, None, hv])), ifm((view.contiguous(), [hv.contiguous(), None, hv.contiguous()])))


def check_state_dict(dev):
    src = pw.DWT1DForward(J=2, wave='db3').to(dev)
    dst = pw.SWT1DForward(J=2, wave='db1').to(dev)
    with pytest.raises(RuntimeError):
        dst.load_state_dict(src.state_dict())              # (db1's buffers hold two taps)
    dst = pw.SWT1DForward(J=2, wave='db5').to(dev)
    res = dst.load_state_dict(pw.DWT1DForward(J=2, wave='sym5').to(dev).state_dict())
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.h0, pw.DWT1DForward(wave='sym5').h0.to(dev)) and sorted(dst.state_dict()) == ['h0', 'h1']
    inv = pw.SWT1DInverse(wave='db5').to(dev)
    res = inv.load_state_dict(pw.DWT1DInverse(wave='sym5').to(dev).state_dict())
    assert not res.missing_keys and not res.unexpected_keys and sorted(inv.state_dict()) == ['g0', 'g1']
