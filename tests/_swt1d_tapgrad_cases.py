"""Shared checks of the filter-tap gradients of the 1-D stationary transform - SWT1DForward / SWT1DInverse / SWT1DShrink with
learned taps, lowlevel.SWT1DMulti / ISWT1DMulti, ops.swt1d_tapgrad and the wave-tile kernel of csrc/wl_swt1d_tapgrad.h -, run by
the emulator (CPU) and the GPU test modules.

The oracle is the float64 chain of tests/_swt1d_cases.py (``wo.afb1d_atrous`` per level, its transposed matrices the other way)
plus the formula of the kernel's header, on the taps and the signals as stored:
    u_0 = s, u_j = sigma A0_j(k0) u_{j-1};   v_J = top, v_{j-1} = sigma (A0_j(k0)^T v_j + A1_j(k1)^T w_j);   d_j = 2^(j-1)
    c0[t] = sigma sum_j sum_p u_{j-1}[p + (t - (L/2 - 1)) d_j] v_j[p],       c1[t] = the same with w_j[p].
check_oracle ties it to central differences of the transform itself, in float64, once.

Tolerance: a tap gradient is a long cancelling sum, so |c - ref| <= REL * sum |terms| with sum |terms| from the oracle and REL
that of tests/_swt1d_cases.py - the rule the shrinkage tests hold the threshold gradient to.  The fused route keeps both chains in
float32 registers whatever the storage type, and its taps and partial sums are float32: REL[float32] for every storage type.
The composed route rounds every level of the chains to the storage type: REL[dtype].  float64: REL[float64]."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import _lib, ops
from pytorch_wavelets_amd.dwt import lowlevel
import _swt1d_cases as W

F64, F32, F16, BF16 = W.F64, W.F32, W.F16, W.BF16
REL = W.REL
WAVES, LEVELS, ROWS = W.WAVES, W.LEVELS, W.ROWS
GRID_WAVES, GRID_DTYPES, TNAME = W.GRID_WAVES, W.GRID_DTYPES, W.TNAME
SEAM_WAVES = ('haar', 'db4', 'db10')        # L = 2, 8, 20
npy, dev_t, ntaps, ana_taps, syn_taps, names_since = W.npy, W.dev_t, W.ntaps, W.ana_taps, W.syn_taps, W.names_since
KERNEL = 'WlSwt1dTapGrad'


def core_of(wave, J):
    return ops.swt1d_tapgrad_core(ntaps(wave), min(J, 3))


def lens(wave, J):
    """Rows shorter than the filter (many wraps per tile), small rows, and - three levels of 2, 8 and 20 taps - the seams."""
    out = (1, 3, 5, 8, 37)
    if J == 3 and wave in SEAM_WAVES:
        core = core_of(wave, J)
        out += (core - 1, core, core + 1, 2 * core + 1)
    return out


def rel_of(dtype, fused):
    return REL[F32] if fused and dtype != F64 else REL[dtype]


# ---------------------------------------------------------------------------------------------- the oracle
def tapgrad_ref(s, top, his, taps, scale):
    """(c (2, L), sum |terms| (2, L)) of s, top (.., n) and his = [finest ..] (None = zeros), float64."""
    J, L, n = len(his), len(taps[0]), s.shape[-1]
    us = [s]
    for j in range(J - 1):
        us.append(scale * wo.afb1d_atrous(us[-1], taps[0], taps[1], 'periodic', -1, 2 ** j)[0])
    c, mags = np.zeros((2, L)), np.zeros((2, L))
    v = top
    for j in range(J - 1, -1, -1):
        d = 2 ** j
        w = np.zeros_like(v) if his[j] is None else his[j]
        for t in range(L):
            u = np.roll(us[j], -(t - (L // 2 - 1)) * d, -1)
            for b, q in enumerate((v, w)):
                c[b, t] += (u * q).sum()
                mags[b, t] += np.abs(u * q).sum()
        v = scale * W.transposed(v, w, taps, d)
    return scale * c, scale * mags


def check_oracle():
    """The two identifications against central differences in float64: the formula with (x, dlo, dhi, h, 1) is the gradient of
    <dlo, lo> + sum <dhi_j, hi_j> in the analysis taps, and with (dx, lo, hi, g, 1/2) the gradient of <dx, inverse> in the
    synthesis taps - rows shorter than the filter included."""
    rng = np.random.RandomState(5)
    eps = 1e-6
    for L, n, J in ((2, 3, 1), (4, 7, 2), (6, 16, 3), (8, 33, 3), (20, 40, 3), (20, 7, 2), (8, 3, 3)):
        taps = [rng.randn(L), rng.randn(L)]
        x, top = rng.randn(2, n), rng.randn(2, n)
        his = [rng.randn(2, n) for _ in range(J)]
        if J > 1:
            his[J // 2] = None

        def f_ana(tp):
            lo, hs = W.analysis_ref(x, tp, J)
            return (lo * top).sum() + sum((h * d).sum() for h, d in zip(hs, his) if d is not None)

        def f_syn(tp):
            return (x * W.adjoint_ref(top, his, tp, 0.5)).sum()

        for f, scale in ((f_ana, 1.0), (f_syn, 0.5)):
            c, mags = tapgrad_ref(x, top, his, taps, scale)
            for b in range(2):
                for t in range(L):
                    hi_t, lo_t = [k.copy() for k in taps], [k.copy() for k in taps]
                    hi_t[b][t] += eps
                    lo_t[b][t] -= eps
                    fd = (f(hi_t) - f(lo_t)) / (2 * eps)
                    assert abs(fd - c[b, t]) <= 1e-7 * max(1.0, mags[b, t]), (L, n, J, scale, b, t, fd, c[b, t])


@functools.lru_cache(maxsize=None)
def _inputs(shape, J, seed):
    """s, top, his: float64 numpy, made once per shape and shared (never written to)."""
    rng = np.random.RandomState(seed)
    return rng.randn(*shape), rng.randn(*shape), [rng.randn(*shape) for _ in range(J)]


def stored(a, dtype):
    """`a` as `dtype` holds it, in float64."""
    return torch.tensor(a).to(dtype).double().numpy()


def close_taps(got, ref, mags, tol, what):
    """got = (c0, c1), any shape with L elements each."""
    for b in range(2):
        err = np.abs(npy(got[b]).ravel() - ref[b])
        bound = tol * mags[b]
        print('%s c%d: max err %.3e, least bound %.3e' % (what, b, float(err.max()), float(bound.min())))
        assert bool((err <= bound).all()), (what, b, err, bound)


# ---------------------------------------------------------------------------------------------- the launcher
def direct_case(dev, taps, J, shape, dtype, scale, drop=(), origin=0, seed=51):
    """ops.swt1d_tapgrad of random rows -> (c0, c1), the oracle's (c, mags)."""
    sn, tn, hn = _inputs(shape, J, seed)
    sn, tn = stored(sn, dtype), stored(tn, dtype)
    hn = [None if j in drop else stored(h, dtype) for j, h in enumerate(hn)]
    k = [dev_t(t, F32, dev) for t in taps]
    got = ops.swt1d_tapgrad(dev_t(sn, dtype, dev), dev_t(tn, dtype, dev), [None if h is None else dev_t(h, dtype, dev) for h in hn],
                            k[0], k[1], scale, origin=origin)
    return got, tapgrad_ref(sn, tn, hn, taps, scale)


def check_instantiation(dev, wave, dtype):
    """WlSwt1dTapGrad<T, L> of one tap count and element type at three levels: three rows of one core plus 40 positions, which
    crosses a seam; both scales, a missing level in one."""
    L = ntaps(wave)
    n = ops.swt1d_tapgrad_core(L, 3) + 40
    for taps, scale, drop in ((ana_taps(wave), 1.0, ()), (syn_taps(wave), 0.5, (1,))):
        c0 = pw.launch_count()
        got, (ref, mags) = direct_case(dev, taps, 3, (3, n), dtype, scale, drop)
        assert pw.kernels_since(c0) == ['%s<%s, %d>' % (KERNEL, TNAME[dtype], L)], pw.kernels_since(c0)
        assert got[0].dtype == F32 and tuple(got[0].shape) == (L,) and tuple(got[1].shape) == (L,)
        close_taps(got, ref, mags, REL[F32], '%s %s scale %s' % (wave, dtype, scale))


def check_levels(dev, wave):
    """nlev 1 and 2 of the launcher (the modules' grid reaches them too): the seam of each."""
    L = ntaps(wave)
    for nlev in (1, 2):
        n = ops.swt1d_tapgrad_core(L, nlev) + 1
        got, (ref, mags) = direct_case(dev, syn_taps(wave), nlev, (2, n), F32, 0.5)
        close_taps(got, ref, mags, REL[F32], '%s nlev=%d' % (wave, nlev))


def check_origin(dev, wave, J=3, dtype=F32):
    """The seams of a row fall elsewhere: the same sums within the tolerance (the partial sums regroup: not bit for bit)."""
    core = core_of(wave, J)
    for n in (core + 1, 37):
        for origin in (0, 1, core - 1):
            got, (ref, mags) = direct_case(dev, ana_taps(wave), J, (2, 1, n), dtype, 1.0, origin=origin)
            close_taps(got, ref, mags, REL[F32], '%s J=%d n=%d origin %d' % (wave, J, n, origin))


def schedule_case(dev):
    """One launch (db4, J = 3, two rows across a seam): what comes out, for a bitwise comparison."""
    return list(direct_case(dev, ana_taps('db4'), 3, (2, 1, core_of('db4', 3) + 1), F32, 1.0)[0])


# ---------------------------------------------------------------------------------------------- the modules
def learn_modules(dev, wave, J, dtype=F32, mode='periodic'):
    """(the taps are float32 parameters whatever the data, float64 for float64 rows)"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64 if dtype == F64 else F32)
    try:
        return pw.SWT1DForward(J=J, wave=wave, mode=mode, learn=True).to(dev), pw.SWT1DInverse(wave=wave, learn=True).to(dev)
    finally:
        torch.set_default_dtype(prev)


def taps_of(*ts):
    return [npy(t).ravel() for t in ts]


def check_forward_taps(dev, wave, J, shape, dtype=F32):
    """(dh0, dh1) of SWT1DForward(learn=True) from random (dlo, dhi): one WlSwt1dTapGrad launch behind the dx launch for J <= 3,
    the composition (no such launch) for J = 5 and float64."""
    xn, dl, dh = _inputs(shape, J, 52)
    xn, dl, dh = stored(xn, dtype), stored(dl, dtype), [stored(h, dtype) for h in dh]
    xfm = learn_modules(dev, wave, J, dtype)[0]
    fused = J <= 3 and dtype != F64
    x = dev_t(xn, dtype, dev).requires_grad_(True)
    yl, yh = xfm(x)
    c0 = pw.launch_count()
    grads = torch.autograd.grad([yl] + list(yh), (x, xfm.h0, xfm.h1), [dev_t(dl, dtype, dev)] + [dev_t(h, dtype, dev) for h in dh])
    ks = names_since(c0)
    assert (ks == ['WlSwt1dAdj', KERNEL]) if fused else (KERNEL not in ks and 'WlCorr1d' in ks), (wave, J, shape, dtype, ks)
    assert grads[1].shape == xfm.h0.shape and grads[1].dtype == xfm.h0.dtype and grads[2].shape == xfm.h1.shape
    ref, mags = tapgrad_ref(xn, dl, dh, taps_of(xfm.h0, xfm.h1), 1.0)
    close_taps(grads[1:], ref, mags, rel_of(dtype, fused), 'forward taps %s J=%d %s %s' % (wave, J, shape, dtype))
    W.close(grads[0], W.adjoint_ref(dl, dh, taps_of(xfm.h0, xfm.h1), 1.0), dtype, 'dx beside them')


def check_inverse_taps(dev, wave, J, shape, dtype=F32):
    """(dg0, dg1) of SWT1DInverse(learn=True) from a random dx, sigma = 1/2: every level present, the middle one None, all None."""
    dxn, ln, hn = _inputs(shape, J, 53)
    dxn, ln, hn = stored(dxn, dtype), stored(ln, dtype), [stored(h, dtype) for h in hn]
    ifm = learn_modules(dev, wave, J, dtype)[1]
    fused = J <= 3 and dtype != F64
    for drop in ((), (J // 2,), tuple(range(J))):
        hs = [None if j in drop else h for j, h in enumerate(hn)]
        rec = ifm((dev_t(ln, dtype, dev), [None if h is None else dev_t(h, dtype, dev) for h in hs]))
        c0 = pw.launch_count()
        grads = torch.autograd.grad(rec, (ifm.g0, ifm.g1), dev_t(dxn, dtype, dev))
        ks = names_since(c0)
        assert (ks == [KERNEL]) if fused else (KERNEL not in ks and ks), (wave, J, shape, dtype, drop, ks)
        ref, mags = tapgrad_ref(dxn, ln, hs, taps_of(ifm.g0, ifm.g1), 0.5)
        close_taps(grads, ref, mags, rel_of(dtype, fused), 'inverse taps %s J=%d %s %s without %s' % (wave, J, shape, dtype, drop))
        if len(drop) == J:
            assert not bool(grads[1].any())


def check_grid(dev, wave, J):
    """Every length of the table, float32, both directions: the short rows under both row counts, the seams under one."""
    for n in lens(wave, J):
        for lead in (ROWS if n <= 37 else ROWS[1:]):
            check_forward_taps(dev, wave, J, lead + (n,))
            check_inverse_taps(dev, wave, J, lead + (n,))


def check_two_byte(dev, wave, dtype):
    for n in (37, core_of(wave, 3) + 1):
        check_forward_taps(dev, wave, 3, (2, 2, n), dtype)
        check_inverse_taps(dev, wave, 3, (2, 2, n), dtype)
    check_forward_taps(dev, wave, 5, (2, 2, 37), dtype)          # (the composition, at the storage type's tolerance)
    check_inverse_taps(dev, wave, 5, (2, 2, 37), dtype)


def check_float64(dev):
    for wave in ('db4', 'db10'):
        check_forward_taps(dev, wave, 3, (2, 2, 45), F64)
        check_inverse_taps(dev, wave, 2, (2, 2, 5), F64)


def check_empty_yh(dev):
    """An empty yh returns yl: no node, so no tap gradient."""
    ifm = learn_modules(dev, 'db2', 1)[1]
    yl = dev_t(_inputs((1, 2, 9), 1, 54)[0], F32, dev).requires_grad_(True)
    out = ifm((yl, []))
    assert out is yl
    assert torch.autograd.grad(out.sum(), (ifm.g0, ifm.g1), allow_unused=True) == (None, None)


# ---------------------------------------------------------------------------------------------- routes
class switch(object):
    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        self.prev, ops.SWT1D_TAPGRAD_FUSED = ops.SWT1D_TAPGRAD_FUSED, self.flag

    def __exit__(self, *exc):
        ops.SWT1D_TAPGRAD_FUSED = self.prev
        return False


def _both_tap_grads(dev, wave, n, dtype):
    """[dh0, dh1, dg0, dg1] of one forward + inverse pass, and the launches of the backward."""
    xn, dl, dh = _inputs((2, 2, n), 3, 55)
    xfm, ifm = learn_modules(dev, wave, 3, dtype)
    x = dev_t(xn, dtype, dev)
    yl, yh = xfm(x)
    rec = ifm((yl, [yh[0], None, yh[2]]))
    c0 = pw.launch_count()
    grads = torch.autograd.grad(rec, (xfm.h0, xfm.h1, ifm.g0, ifm.g1), dev_t(dl, dtype, dev))
    return list(grads), names_since(c0)


def check_routes(dev, dtype=F32):
    """The switch off, and a launcher that declines: the composition's answer, no WlSwt1dTapGrad launch."""
    for wave, n in (('db4', 37), ('db10', core_of('db10', 3) + 1)):
        base, ks = _both_tap_grads(dev, wave, n, dtype)
        assert ks.count(KERNEL) == 2, ks
        with switch(False):
            off, ks = _both_tap_grads(dev, wave, n, dtype)
        assert KERNEL not in ks and 'WlCorr1d' in ks, ks
        saved = ops.swt1d_tapgrad
        ops.swt1d_tapgrad = lambda *a, **k: None
        try:
            declined, ks = _both_tap_grads(dev, wave, n, dtype)
        finally:
            ops.swt1d_tapgrad = saved
        assert KERNEL not in ks and 'WlCorr1d' in ks, ks
        # The oracle from x and the cotangent alone: its own coefficients for the synthesis taps, its own cotangents of the
        # inverse for the analysis taps.  The rule's bound as it stands, the fused route at float32's.
        xn, dl, _ = _inputs((2, 2, n), 3, 55)
        xn, dl = stored(xn, dtype), stored(dl, dtype)
        dlo, dhis = W.analysis_ref(dl, syn_taps(wave), 3, scale=0.5)
        dhis[1] = np.zeros_like(dhis[1])
        lo, his = W.analysis_ref(xn, ana_taps(wave), 3)
        refs = [tapgrad_ref(xn, dlo, dhis, ana_taps(wave), 1.0), tapgrad_ref(dl, lo, [his[0], None, his[2]], syn_taps(wave), 0.5)]
        for got, name in ((base, 'fused'), (off, 'switch off'), (declined, 'declined')):
            tol = rel_of(dtype, name == 'fused')
            close_taps(got[:2], refs[0][0], refs[0][1], tol, '%s analysis taps behind an inverse %s' % (name, wave))
            close_taps(got[2:], refs[1][0], refs[1][1], tol, '%s synthesis taps behind a forward %s' % (name, wave))


def check_a_memoised_decline(dev):
    """A launcher's WL_ERR_UNSUPPORTED is remembered under the call's key: the next call does not reach the C entry."""
    taps = [dev_t(t, F32, dev) for t in ana_taps('db2')]
    x = dev_t(_inputs((2, 9), 1, 56)[0], F32, dev)
    seen, call0 = [], ops._call

    def call(name, ref, *args):
        seen.append(name)
        return _lib.WL_ERR_UNSUPPORTED if name == 'wl_swt1d_tapgrad' else call0(name, ref, *args)

    ops._call = call
    try:
        assert ops.swt1d_tapgrad(x, x, [x], taps[0], taps[1], 1.0) is None
        assert ops.swt1d_tapgrad(x, x, [x], taps[0], taps[1], 1.0) is None
    finally:
        ops._call = call0
        ops._FUSED_DECLINED.discard(('swt1d_tapgrad', x.device, x.dtype, 2, 9, 4, 1))
    assert seen.count('wl_swt1d_tapgrad') == 1, seen
    assert ops.swt1d_tapgrad(x, x, [x], taps[0], taps[1], 1.0) is not None


def check_fixed_taps_launch_as_before(dev):
    """No tap requires a gradient: exactly the launches of the transform and its backward, nothing more saved."""
    xn, dl, dh = _inputs((2, 2, 37), 3, 57)
    xfm, ifm = W.modules(dev, 'db4', 3)
    x = dev_t(xn, F32, dev).requires_grad_(True)
    c0 = pw.launch_count()
    yl, yh = xfm(x)
    rec = ifm((yl, yh))
    assert len(yl.grad_fn.saved_tensors) == 2 and len(rec.grad_fn.saved_tensors) == 2
    rec.backward(dev_t(dl, F32, dev))
    assert names_since(c0) == ['WlSwt1dFwd', 'WlSwt1dAdj', 'WlSwt1dFwd', 'WlSwt1dAdj'], names_since(c0)
    assert xfm.h0.grad is None and ifm.g0.grad is None
    # learned: x (forward) and lo + the highs (inverse) are saved as well
    xfm, ifm = learn_modules(dev, 'db4', 3)
    yl, yh = xfm(x)
    rec = ifm((yl, [yh[0], None, yh[2]]))
    assert len(yl.grad_fn.saved_tensors) == 3 and len(rec.grad_fn.saved_tensors) == 5
    # only the taps ask: the inverse's backward is the tap launch alone
    lo = dev_t(dl, F32, dev)
    rec = ifm((lo, [lo, lo, lo]))
    c0 = pw.launch_count()
    rec.backward(lo)
    assert names_since(c0) == [KERNEL], names_since(c0)
    # under no_grad nothing is asked
    with torch.no_grad():
        c0 = pw.launch_count()
        xfm(x)
        assert names_since(c0) == ['WlSwt1dFwd']


# ---------------------------------------------------------------------------------------------- gradcheck
def check_gradcheck(dev):
    """torch.autograd.gradcheck in float64 (the composition) of swt1d, iswt1d and swt1d_shrink (soft) with all taps as inputs."""
    import _shrink1d_cases as S
    rng = np.random.RandomState(58)
    h = [dev_t(t, F64, dev).requires_grad_(True) for t in ana_taps('db2')]
    g = [dev_t(t, F64, dev).requires_grad_(True) for t in syn_taps('db2')]
    x = dev_t(rng.randn(1, 2, 12), F64, dev).requires_grad_(True)
    c0 = pw.launch_count()
    assert torch.autograd.gradcheck(lambda a, p, q: (lambda r: tuple([r[0]] + r[1]))(lowlevel.swt1d(a, p, q, 'periodic', 2)),
                                    (x, h[0], h[1]), eps=1e-6, atol=1e-7)
    cs = [dev_t(rng.randn(1, 2, 12), F64, dev).requires_grad_(True) for _ in range(3)]
    assert torch.autograd.gradcheck(lambda a, b, c, p, q: lowlevel.iswt1d(a, [b, c], p, q), tuple(cs) + tuple(g), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, c, p, q: lowlevel.iswt1d(a, [None, c], p, q), (cs[0], cs[2]) + tuple(g), eps=1e-6, atol=1e-7)
    # shrinkage on gap rows (a finite difference across a threshold is no derivative)
    xn, _, thr = S.gap_case('db2', 2, (1, 2, 12), F64)
    his = S.coeffs_ref(xn, 'db2', 2)[1]
    assert min(float(np.abs(np.abs(w) - thr[j][..., None]).min()) for j, w in enumerate(his)) > 1e-4
    xs = dev_t(xn, F64, dev).requires_grad_(True)
    t = dev_t(thr, F64, dev).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, p, q, r, s: lowlevel.swt1d_shrink(a, p, q, r, s, b, 2, 'soft'),
                                    (xs, t, h[0], h[1], g[0], g[1]), eps=1e-6, atol=1e-7)
    assert KERNEL not in names_since(c0) and not any(k.startswith('WlShrink1d') for k in names_since(c0))


# ---------------------------------------------------------------------------------------------- SWT1DShrink
def check_shrink_learns_everything(dev, dtype=F32):
    """One loss.backward() through SWT1DShrink(learn=True, learn_filters=True) fills .grad of the thresholds and of all four
    taps, against the oracle on gap rows (tests/_shrink1d_cases.py: no coefficient near its threshold)."""
    import _shrink1d_cases as S
    wave, J, shape = 'db4', 3, (2, 2, 37)
    xn, dyn, thr = S.gap_case(wave, J, shape, dtype)
    t32 = thr.astype(np.float32)
    table = np.broadcast_to(t32.astype(np.float64), (J, 2, 2))
    mod = pw.SWT1DShrink(J=J, wave=wave, thresh=torch.tensor(t32), learn=True, learn_filters=True).to(dev)
    assert sorted(k for k, _ in mod.named_parameters()) == ['g0', 'g1', 'h0', 'h1', 'thresh']
    c0 = pw.launch_count()
    y = mod(dev_t(xn, dtype, dev))
    y.backward(dev_t(dyn, dtype, dev))
    ks = names_since(c0)
    assert ks.count(KERNEL) == 2 and not any(k.startswith('WlShrink1d') for k in ks), ks
    for name in ('h0', 'h1', 'g0', 'g1', 'thresh'):
        p = getattr(mod, name)
        assert p.grad is not None and p.grad.shape == p.shape, name
    h, g = ana_taps(wave), syn_taps(wave)
    lo, his = S.coeffs_ref(xn, wave, J)
    shrunk = [S.shrink_np(w, table[j][..., None], 'soft') for j, w in enumerate(his)]
    S.close_values(y, W.adjoint_ref(lo, shrunk, g, 0.5), xn, dtype, 'y with learned filters')
    ref, mags = tapgrad_ref(dyn, lo, shrunk, g, 0.5)
    close_taps((mod.g0.grad, mod.g1.grad), ref, mags, REL[dtype], 'shrink synthesis taps')
    dlo, dhis = W.analysis_ref(dyn, g, J, scale=0.5)
    masked = [d * (np.abs(w) > table[j][..., None]) for j, (d, w) in enumerate(zip(dhis, his))]
    ref, mags = tapgrad_ref(xn, dlo, masked, h, 1.0)
    close_taps((mod.h0.grad, mod.h1.grad), ref, mags, REL[dtype], 'shrink analysis taps')
    _, rdt, tm = S.backward_ref(xn, dyn, table, wave, J, 'soft')
    S.close_dt(mod.thresh.grad, rdt.sum(1, keepdims=True), tm.sum(1, keepdims=True), dtype, 0.0, 'dt with learned filters')
    # fixed filters keep the one-launch kernels
    fixed = pw.SWT1DShrink(J=J, wave=wave, thresh=torch.tensor(t32), learn=True).to(dev)
    c0 = pw.launch_count()
    fixed(dev_t(xn, dtype, dev)).backward(dev_t(dyn, dtype, dev))
    assert names_since(c0) == ['WlShrink1dFwd', 'WlShrink1dBwd'] and fixed.h0.grad is None


# ---------------------------------------------------------------------------------------------- modules, errors, views
def check_modules(dev):
    for make, names in ((lambda **kw: pw.SWT1DForward(J=2, wave='db3', **kw), ['h0', 'h1']),
                        (lambda **kw: pw.SWT1DInverse(wave='db3', **kw), ['g0', 'g1']),
                        (lambda **kw: pw.SWT1DShrink(J=2, wave='db3', **({'learn_filters': kw['learn']} if kw else {})),
                         ['g0', 'g1', 'h0', 'h1'])):
        fixed, learned = make().to(dev), make(learn=True).to(dev)
        assert [k for k, _ in fixed.named_parameters()] == [] and sorted(k for k, _ in learned.named_parameters()) == names
        assert all(isinstance(getattr(learned, k), torch.nn.Parameter) and getattr(learned, k).requires_grad for k in names)
        keys = names + ['thresh'] if 'g0' in names and 'h0' in names else names
        assert sorted(fixed.state_dict()) == sorted(keys) and sorted(learned.state_dict()) == sorted(keys)
        assert all(torch.equal(fixed.state_dict()[k], learned.state_dict()[k]) for k in keys)
        assert 'taps=buffers' in repr(fixed) and 'taps=parameters' in repr(learned)
        # the two forms load each other's state
        with torch.no_grad():
            for k in names:
                getattr(learned, k).mul_(1.5)
        res = fixed.load_state_dict(learned.state_dict())
        assert not res.missing_keys and not res.unexpected_keys
        assert all(torch.equal(getattr(fixed, k), getattr(learned, k).detach()) for k in names)
        other = make(learn=True).to(dev)
        res = other.load_state_dict(fixed.state_dict())
        assert not res.missing_keys and not res.unexpected_keys
        assert all(torch.equal(getattr(other, k).detach(), getattr(fixed, k)) and isinstance(getattr(other, k), torch.nn.Parameter)
                   for k in names)


def check_errors_and_edges(dev):
    x = dev_t(_inputs((2, 2, 20), 1, 59)[0], F32, dev)
    with pytest.raises(ValueError, match="'periodic' only"):
        pw.SWT1DForward(J=1, wave='db2', mode='symmetric', learn=True).to(dev)(x)
    yl, yh = pw.SWT1DForward(J=1, wave='db2', mode='symmetric').to(dev)(x)           # fixed taps: as before
    ref = W.analysis_ref(npy(x), ana_taps('db2'), 1, 'symmetric')
    W.close(yl, ref[0], F32, 'symmetric with fixed taps')
    with torch.no_grad():                                                            # nothing asks for a gradient
        pw.SWT1DForward(J=1, wave='db2', mode='symmetric', learn=True).to(dev)(x)
    with pytest.raises(ValueError, match='even number of taps'):
        pw.SWT1DForward(J=1, wave=W.ODD_PAIR, learn=True).to(dev)(x)
    pw.SWT1DForward(J=1, wave=W.ODD_PAIR).to(dev)(x)
    with pytest.raises(ValueError, match="'periodic' only"):
        pw.SWT1DShrink(J=1, wave='db2', mode='symmetric', learn_filters=True).to(dev)(x)
    # the C entry outside its envelope, the codes in the order of wl_swt1d_adjoint
    h = [dev_t(t, F32, dev) for t in ana_taps('db2')]
    part = torch.empty(4, 1, 2, 4, device=dev)
    be, unsupported, shape_err, taps_err = ops._backend(), _lib.WL_ERR_UNSUPPORTED, -2, -5
    ptrs = (ctypes.c_void_p * 3)(x.data_ptr(), None, None)

    def entry(s=x.data_ptr(), his=ptrs, dtype=0, rows=4, n=20, J=1, k0=h[0].data_ptr(), L=4, ext=ops.EXT_PERIODIC, origin=0):
        return be.wl_swt1d_tapgrad(s, x.data_ptr(), his, part.data_ptr(), dtype, rows, n, J, k0, h[1].data_ptr(), L, ext, 1.0, origin, None)

    assert entry() == 0
    assert entry(dtype=2) == unsupported and entry(L=3) == unsupported and entry(L=22) == unsupported
    assert entry(J=4) == unsupported and entry(J=0) == shape_err and entry(ext=ops.EXT_SYM) == unsupported
    assert entry(n=0) == shape_err and entry(rows=-1) == shape_err
    assert entry(origin=-1) == shape_err and entry(origin=ops.swt1d_tapgrad_core(4, 1)) == shape_err
    assert entry(s=None) == shape_err and entry(his=None) == shape_err
    assert entry(k0=None) == taps_err
    assert entry(s=None, k0=None) == shape_err and entry(L=22, s=None) == unsupported
    c0 = pw.launch_count()
    assert entry(rows=0) == 0 and pw.launch_count() == c0
    # the wrapper outside the envelope declines
    assert ops.swt1d_tapgrad(x.double(), x.double(), [x.double()], h[0], h[1], 1.0) is None
    assert ops.swt1d_tapgrad(x, x, [x] * 4, h[0], h[1], 1.0) is None
    assert ops.swt1d_tapgrad(x, x, [x], h[0][:3], h[1][:3], 1.0) is None
    with pytest.raises(ValueError):
        ops.swt1d_tapgrad(x, x[..., 1:], [x], h[0], h[1], 1.0)
    assert ops.swt1d_tapgrad_core(20, 3) == 891 and ops.swt1d_tapgrad_core(2, 3) == 1011 and ops.swt1d_tapgrad_core(8, 1) == 1017
    for L in range(2, 21, 2):
        for J in (1, 2, 3):
            need = [max((L // 2 - 1) * (2 ** j - 1), (L // 2) * (2 ** J - 2 ** j)) for j in range(1, J + 1)]
            back = [max((L // 2) * (2 ** j - 1), (L // 2 - 1) * (2 ** J - 2 ** j)) for j in range(1, J + 1)]
            assert ops.swt1d_tapgrad_core(L, J) == 1024 - max(need) - max(back)


def check_cpu_tensor_raises():
    x = torch.zeros(1, 1, 16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.SWT1DForward(J=2, wave='db2', learn=True)(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.SWT1DInverse(wave='db2', learn=True)((x, [x]))
    h = torch.zeros(4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.swt1d_tapgrad(x, x, [x], h, h, 1.0)


def check_views(dev):
    """A non-contiguous cotangent, x[..., 1:-1] and a sliced batch: the tap gradients of their contiguous copies, bit for bit."""
    n = core_of('db4', 3) + 3
    base = dev_t(_inputs((3, 3, n), 3, 60)[0], F32, dev)
    other = base.flip(-1)
    xfm, ifm = learn_modules(dev, 'db4', 3)
    for cut in (lambda t: t[..., 1:-1], lambda t: t[:, 1:], lambda t: t[::2]):
        view, dy = cut(base), cut(other)
        assert not view.is_contiguous() and not dy.is_contiguous()
        outs = []
        for x, d in ((view, dy), (view.contiguous(), dy.contiguous())):
            yl, yh = xfm(x)
            rec = ifm((yl, yh))
            outs.append(torch.autograd.grad([rec, yh[1]], (xfm.h0, xfm.h1, ifm.g0, ifm.g1), [d, d]))
        assert all(torch.equal(a, b) for a, b in zip(*outs))


def check_guard(dev):
    """One fused launch inside the poisoned parents of tests/_guard_cases.py: `part` is written in full, nothing outside it."""
    import _guard_cases as G
    L, n = 8, core_of('db4', 3) + 40
    with G.guarded(dev) as g:
        got, (ref, mags) = direct_case(dev, syn_taps('db4'), 3, (3, n), F32, 0.5, drop=(0,))
        parts = [b for b in g.blocks if b.package and 'swt1d_tapgrad' in b.site]
        assert [b.shape for b in parts] == [(3, 2, 2, L)], [b.describe() for b in g.blocks]
    close_taps(got, ref, mags, REL[F32], 'guarded launch')
