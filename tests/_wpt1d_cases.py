"""Shared checks of the 1-D wavelet packet transform - WPT1DForward / WPT1DInverse, lowlevel.wpt1d_level / iwpt1d_level, their
gradients and the wave-tile kernels of csrc/wl_wpt1d.h -, run by the emulator (CPU) and the GPU test modules.

Expected values come from the pinned oracle alone, in float64 on the module's own (float32) taps: a level is ``wo.afb1d`` on the
stacked bands, child 2b + s of band b; the inverse is ``wo.sfb1d`` per level.  For rows of up to 296 samples the gradients come
from the dense matrix W of the J-level tree, which the oracle makes of an identity: W_h^T dy for the forward's backward, W_g^T y
for the inverse, W_g dx for the inverse's backward.  Longer rows (periodization only) use the oracle's banks with the taps
swapped - the synthesis bank is the transpose of the analysis bank with the same stored taps -, and check_transposes ties the
two forms together.  Outside periodization and zero padding the reference's gradient is no transpose: there the expected
value is the reference's rule itself, the synthesis with the analysis taps cropped to the level's input.

Tolerances: the REL / REC tables and close() of tests/_swt1d_cases.py - values relative to |ref|max, 1e-5 float32, 4e-3 float16,
3e-2 bfloat16, 1e-12 float64; reconstructions absolute, times max(1, |x|max)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import _lib, filters, ops
from pytorch_wavelets_amd.dwt import lowlevel
from _swt1d_cases import REL, REC, ODD_PAIR, close, dev_t, f32taps, names_since, npy, ntaps, ana_taps, syn_taps

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
WAVES = ('haar', 'bior2.2', 'db4', 'db10')
ORTHOGONAL = ('haar', 'db4', 'db10')
LEVELS = (1, 2, 3, 5)
ROWS = ((1, 3), (2, 2))
OTHER_MODES = ('zero', 'symmetric', 'reflect', 'periodic')
GRID_WAVES = tuple('db%d' % i for i in range(1, 11))        # L = 2, 4, .., 20: one case of the dispatchers' switch each
GRID_DTYPES = (F32, F16, BF16)
PER = 'periodization'
DENSE_MAX = 296


def chunks(J):
    return [3] * (J // 3) + ([J % 3] if J % 3 else [])


def lens(wave, J):
    """The envelope's edge (the last level's input is as long as the filter; the row wraps many times inside one tile), one
    tile with an odd band length (every band row off the 16-byte grid), two seams and a sliver tile."""
    L, q = ntaps(wave), 2 ** J
    return (-(-L * 2 ** (J - 1) // q) * q, q * 37, 2 * ops.wpt1d_core(L, min(J, 3)) + q)


def fused_launches(n, L, J, mode=PER):
    """Launches of a wave-tile kernel per direction of a J-level transform of n samples: the chunks inside the envelope."""
    k = 0
    for c in chunks(J):
        if mode in (PER, 'per') and L % 2 == 0 and L <= 20 and n % 2 ** c == 0 and n >> (c - 1) >= L:
            k += 1
        for _ in range(c):
            n = ops.coeff_len(n, L, lowlevel.mode_to_int(mode))
    return k


def level_lens(n, J, L, mode):
    out = [n]
    for _ in range(J):
        out.append(ops.coeff_len(out[-1], L, lowlevel.mode_to_int(mode)))
    return out


def tree_ref(x, taps, J, mode=PER):
    """x (..., n) -> (..., 2**J, n_J): wo.afb1d per level on the stacked bands, band 2b + s under band b."""
    y = x[..., None, :]
    for _ in range(J):
        lo, hi = wo.afb1d(y, taps[0], taps[1], mode, -1)
        y = np.stack([lo, hi], -2).reshape(lo.shape[:-2] + (2 * lo.shape[-2], lo.shape[-1]))
    return y


def tree_inv_ref(y, taps, mode=PER, crop=None):
    """y (..., 2**J, m) -> (..., n): wo.sfb1d per level; crop = [n_0 .. n_J] cuts level j's result to n_j."""
    J = y.shape[-2].bit_length() - 1
    for j in range(J, 0, -1):
        y = y.reshape(y.shape[:-2] + (2 ** (j - 1), 2, y.shape[-1]))
        y = wo.sfb1d(y[..., 0, :], y[..., 1, :], taps[0], taps[1], mode, -1)
        if crop is not None:
            y = y[..., :crop[j - 1]]
    return y[..., 0, :]


@functools.lru_cache(maxsize=None)
def _wmat(t0, t1, n, J, mode):
    """W (n, 2**J, n_J): the J-level tree of an identity."""
    return tree_ref(np.eye(n), (np.array(t0), np.array(t1)), J, mode)


def w_apply(x, taps, J, mode=PER):
    """W x."""
    return np.einsum('ibk,...i->...bk', _wmat(tuple(taps[0]), tuple(taps[1]), x.shape[-1], J, mode), x)


def w_transposed(y, taps, n, mode=PER):
    """W^T y."""
    J = y.shape[-2].bit_length() - 1
    return np.einsum('ibk,...bk->...i', _wmat(tuple(taps[0]), tuple(taps[1]), n, J, mode), y)


def transposed_ref(y, taps, n):
    """W^T y in periodization: the matrix for short rows, the oracle's synthesis bank with the same taps for long ones."""
    return w_transposed(y, taps, n) if n <= DENSE_MAX else tree_inv_ref(y, taps)


def per_analysis_closed(x, h0, h1):
    """lo[k], hi[k] = sum_t h0[t], h1[t] * in[(2k + t - (L/2 - 1)) mod m]: the form the kernels compute."""
    m, L = x.shape[-1], len(h0)
    idx = (2 * np.arange(m // 2)[:, None] + np.arange(L)[None, :] - (L // 2 - 1)) % m
    return (x[..., idx] * h0).sum(-1), (x[..., idx] * h1).sum(-1)


def per_synthesis_closed(lo, hi, g0, g1):
    """out[i] = sum over (k, t) with 2k + t - (L/2 - 1) = i (mod m) of g0[t] lo[k] + g1[t] hi[k]: the exact transpose."""
    K, L = lo.shape[-1], len(g0)
    out = np.zeros(lo.shape[:-1] + (2 * K,))
    for k in range(K):
        for t in range(L):
            out[..., (2 * k + t - (L // 2 - 1)) % (2 * K)] += g0[t] * lo[..., k] + g1[t] * hi[..., k]
    return out


def check_closed_forms():
    """The two closed forms of csrc/wl_wpt1d.h are the oracle's periodization banks for every band at least as long as the
    filter (no kernel runs here)."""
    rng = np.random.RandomState(1)
    for wave in WAVES + ('db2',):
        L = ntaps(wave)
        for n in (L, L + 2, 4 * L + 6):
            x = rng.randn(2, n)
            h, g = ana_taps(wave), syn_taps(wave)
            lo, hi = wo.afb1d(x, h[0], h[1], PER, -1)
            a, b = per_analysis_closed(x, h[0], h[1])
            assert max(np.abs(a - lo).max(), np.abs(b - hi).max()) <= 1e-13, (wave, n)
            rec = wo.sfb1d(lo, hi, g[0], g[1], PER, -1)
            assert np.abs(per_synthesis_closed(lo, hi, g[0], g[1]) - rec).max() <= 1e-13, (wave, n)


def check_transposes():
    """In periodization the oracle's synthesis bank is the transpose of its analysis bank with the same taps (what long rows
    are checked against), and the inverse is W_g^T."""
    rng = np.random.RandomState(2)
    for wave in WAVES:
        L = ntaps(wave)
        for J, n in ((1, L), (2, 2 * L + 4), (3, 8 * 37)):
            y = rng.randn(2, 2 ** J, n >> J)
            for taps in (ana_taps(wave), syn_taps(wave)):
                a, b = w_transposed(y, taps, n), tree_inv_ref(y, taps)
                assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max()), (wave, J, n)
            x = rng.randn(2, n)
            assert np.abs(w_apply(x, ana_taps(wave), J) - tree_ref(x, ana_taps(wave), J)).max() <= 1e-12
            rec = tree_inv_ref(tree_ref(x, filters.dwt_analysis_taps(wave), J), filters.dwt_synthesis_taps(wave))
            assert np.abs(rec - x).max() <= 1e-10, (wave, J, n)


@functools.lru_cache(maxsize=None)
def _inputs(shape, J, seed):
    """x, coefficients / cotangents y (..., 2**J, n >> J) and a cotangent of the inverse: float64 numpy, made once per shape and
    shared (never written to)."""
    rng = np.random.RandomState(seed)
    return rng.randn(*shape), rng.randn(*(shape[:-1] + (2 ** J, shape[-1] >> J))), rng.randn(*shape)


def modules(dev, wave, J, mode=PER, dtype=None):
    prev = torch.get_default_dtype()
    if dtype == F64:
        torch.set_default_dtype(F64)
    try:
        return pw.WPT1DForward(J=J, wave=wave, mode=mode).to(dev), pw.WPT1DInverse(wave=wave, mode=mode).to(dev)
    finally:
        torch.set_default_dtype(prev)


def check_case(dev, wave, J, shape, dtype=F32):
    """One shape inside the envelope: forward values, the inverse of given coefficients, the round trip with size=, both backward
    passes, and the launches - ceil(J / 3) of WlWpt1dAfb / WlWpt1dSfb per direction, nothing else."""
    n, L = shape[-1], ntaps(wave)
    k = fused_launches(n, L, J)
    assert k == -(-J // 3), (wave, J, n, k)
    xn, yn, cn = _inputs(shape, J, 21)
    h, g = ana_taps(wave), syn_taps(wave)
    xfm, ifm = modules(dev, wave, J)
    tag = '%s J=%d %s' % (wave, J, shape)
    # forward and its backward
    x = dev_t(xn, dtype, dev).requires_grad_(True)
    c0 = pw.launch_count()
    y = xfm(x)
    assert names_since(c0) == ['WlWpt1dAfb'] * k, (tag, names_since(c0))
    assert y.is_contiguous()
    close(y, tree_ref(npy(x), h, J), dtype, 'forward ' + tag)
    dy = dev_t(yn, dtype, dev)
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(y, x, dy)
    assert names_since(c0) == ['WlWpt1dSfb'] * k, (tag, names_since(c0))
    close(dx, transposed_ref(npy(dy), h, n), dtype, 'backward of the forward ' + tag)
    # the inverse of given coefficients and its backward
    c = dev_t(yn, dtype, dev).requires_grad_(True)
    c0 = pw.launch_count()
    rec = ifm(c)
    assert names_since(c0) == ['WlWpt1dSfb'] * k, (tag, names_since(c0))
    close(rec, tree_inv_ref(npy(c), g), dtype, 'inverse ' + tag)
    if n <= DENSE_MAX:
        close(rec, w_transposed(npy(c), g, n), dtype, 'inverse against W_g^T ' + tag)
    dr = dev_t(cn, dtype, dev)
    c0 = pw.launch_count()
    dc, = torch.autograd.grad(rec, c, dr)
    assert names_since(c0) == ['WlWpt1dAfb'] * k, (tag, names_since(c0))
    ref = w_apply(npy(dr), g, J) if n <= DENSE_MAX else tree_ref(npy(dr), g, J)
    close(dc, ref, dtype, 'backward of the inverse ' + tag)
    # round trip
    if wave in ORTHOGONAL and dtype in REC:
        back = ifm(y.detach(), size=n)
        err = float((back.double() - x.detach().double()).abs().max())
        bound = REC[dtype] * max(1.0, float(x.detach().abs().max()))
        print('round trip %s %s: max err %.3e, bound %.3e' % (tag, dtype, err, bound))
        assert back.shape == x.shape and back.dtype == dtype and err <= bound, (tag, err, bound)


def check_grid(dev, wave, J):
    """Every length and row count of the table, float32."""
    for n in lens(wave, J):
        for lead in ROWS:
            check_case(dev, wave, J, lead + (n,))


def check_two_byte(dev, wave, dtype):
    for J in (3, 5):
        for n in lens(wave, J)[1:]:
            check_case(dev, wave, J, (2, 2, n), dtype)


def check_identities(dev):
    """J = 1 is DWT1DForward's (yl, yh[0]) stacked, and band 0 of any tree is DWT1DForward's yl, in every mode - both sides on
    the device."""
    for mode in (PER,) + OTHER_MODES:
        for wave, n in (('db4', 296), ('bior2.2', 45)):
            x = dev_t(_inputs((2, 2, n), 1, 22)[0], F32, dev)
            yl, yh = pw.DWT1DForward(J=1, wave=wave, mode=mode).to(dev)(x)
            y = pw.WPT1DForward(J=1, wave=wave, mode=mode).to(dev)(x)
            ref = npy(torch.stack([yl, yh[0]], 2))
            close(y, ref, F32, 'J = 1 against DWT1DForward %s %s' % (wave, mode))
            for J in (2, 3):
                yl = pw.DWT1DForward(J=J, wave=wave, mode=mode).to(dev)(x)[0]
                y = pw.WPT1DForward(J=J, wave=wave, mode=mode).to(dev)(x)
                close(y[:, :, 0], npy(yl), F32, 'band 0 against DWT1DForward %s %s J=%d' % (wave, mode, J))


def _launch_taps(dev, taps):
    return [dev_t(t, F32, dev) for t in taps]


def check_instantiation(dev, wave, dtype):
    """One tap count x one dtype x nlev 1..3 through ops.wpt1d_afb / wpt1d_sfb, at a short length just past the envelope's edge."""
    L = ntaps(wave)
    h, g = ana_taps(wave), syn_taps(wave)
    for nlev in (1, 2, 3):
        q = 2 ** nlev
        n = -(-L * 2 ** (nlev - 1) // q) * q + q
        xn, yn, _ = _inputs((3, n), nlev, 23)
        th, tg = _launch_taps(dev, h), _launch_taps(dev, g)
        c0 = pw.launch_count()
        y = ops.wpt1d_afb(dev_t(xn, dtype, dev), th[0], th[1], 2, nlev)
        x = ops.wpt1d_sfb(dev_t(yn, dtype, dev), tg[0], tg[1], 2, nlev)
        ks = pw.kernels_since(c0)
        assert [k.split('<')[0] for k in ks] == ['WlWpt1dAfb', 'WlWpt1dSfb'] and all('%d>' % L in k for k in ks), ks
        close(y, tree_ref(npy(dev_t(xn, dtype, dev)), h, nlev), dtype, 'analysis %s nlev=%d %s' % (wave, nlev, dtype))
        close(x, tree_inv_ref(npy(dev_t(yn, dtype, dev)), g), dtype, 'synthesis %s nlev=%d %s' % (wave, nlev, dtype))


def fused_pair(dev, wave, J, shape, dtype, origin):
    xn, yn, _ = _inputs(shape, J, 24)
    h = _launch_taps(dev, ana_taps(wave))
    return [ops.wpt1d_afb(dev_t(xn, dtype, dev), h[0], h[1], 2, J, origin=origin),
            ops.wpt1d_sfb(dev_t(yn, dtype, dev), h[0], h[1], 2, J, origin=origin)]


def check_origin(dev, wave, J, dtype=F32):
    """The seams of a row fall elsewhere: not a bit changes, analysis and synthesis."""
    for n in lens(wave, J):
        base = fused_pair(dev, wave, J, (2, 1, n), dtype, 0)
        assert all(b is not None for b in base)
        for origin in (2 ** J, 5 * 2 ** J):
            got = fused_pair(dev, wave, J, (2, 1, n), dtype, origin)
            assert all(torch.equal(a, b) for a, b in zip(got, base)), (wave, J, n, origin)


def _no_wave_tile(ks):
    return not any(k.startswith('WlWpt1d') for k in ks)


def check_declined(dev, wave, J, n, mode=PER, dtype=F32, fused=0, oracle_wave=None):
    """A transform that leaves the envelope (wholly, or - fused > 0 - in its later chunks): the oracle's answers for the forward,
    the inverse with size= and the forward's backward by the reference's rule (the synthesis with the analysis taps, every
    level cropped to its input), and `fused` launches of the wave-tile kernels per direction."""
    if oracle_wave is None:
        h, g = (filters.dwt_analysis_taps(wave), filters.dwt_synthesis_taps(wave)) if dtype == F64 else (ana_taps(wave), syn_taps(wave))
    else:
        h, g = oracle_wave
    L = len(h[0])
    xn = _inputs((2, 2, n), 0, 25)[0]
    xfm, ifm = modules(dev, wave, J, mode, dtype)
    tag = '%s %s J=%d n=%d %s' % (wave if isinstance(wave, str) else 'pair', mode, J, n, dtype)
    x = dev_t(xn, dtype, dev).requires_grad_(True)
    c0 = pw.launch_count()
    y = xfm(x)
    ks = names_since(c0)
    assert ks.count('WlWpt1dAfb') == fused and 'WlWpt1dSfb' not in ks, (tag, ks)
    ref = tree_ref(npy(x), h, J, mode)
    close(y, ref, dtype, 'forward ' + tag)
    crop = level_lens(n, J, L, mode)
    rng = np.random.RandomState(26)
    dyn = rng.randn(*ref.shape)
    dy = dev_t(dyn, dtype, dev)
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(y, x, dy)
    ks = names_since(c0)
    assert ks.count('WlWpt1dSfb') == fused and 'WlWpt1dAfb' not in ks, (tag, ks)
    close(dx, tree_inv_ref(npy(dy), h, mode, crop), dtype, 'backward of the forward ' + tag)
    if len(g[0]) % 2 == 0:
        rec = ifm(dy, size=n)
        close(rec, tree_inv_ref(npy(dy), g, mode, crop), dtype, 'inverse ' + tag)


def check_declined_routes(dev):
    for mode in OTHER_MODES:
        for wave in ('db4', 'bior2.2'):
            check_declined(dev, wave, 3, 45, mode)
        check_declined(dev, 'db4', 3, 296, mode)
    check_declined(dev, 'db4', 2, 45)                       # n odd
    check_declined(dev, 'db4', 3, 100)                      # n % 2**J != 0
    check_declined(dev, 'db4', 3, 24)                       # below the envelope: level 3 reads 6 samples with 8 taps
    check_declined(dev, 'db4', 5, 96, fused=1)              # routes mix: three levels in one launch, rows of 12 level by level
    check_declined(dev, ODD_PAIR, 2, 48, oracle_wave=(f32taps([v[::-1] for v in ODD_PAIR]), f32taps(ODD_PAIR)))
    for wave, n in (('db4', 296), ('db10', 80), ('db4', 45)):
        check_declined(dev, wave, 3, n, dtype=F64)


def check_gradcheck(dev):
    """torch.autograd.gradcheck of both modules on the float64 (level-by-level) path, periodization and zero padding."""
    rng = np.random.RandomState(27)
    for mode, n in ((PER, 16), ('zero', 13)):
        xfm, ifm = modules(dev, 'db2', 2, mode, F64)
        x = dev_t(rng.randn(1, 2, n), F64, dev).requires_grad_(True)
        assert torch.autograd.gradcheck(xfm, (x,), eps=1e-6, atol=1e-7)
        y = xfm(x).detach().clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda v: ifm(v, size=n), (y,), eps=1e-6, atol=1e-7)


def check_switch(dev, dtype=F32):
    """ops.WPT1D_FUSED = False: level by level, the same answers within the tolerance."""
    for wave, J, n in (('db4', 3, 296), ('db10', 5, lens('db10', 5)[2])):
        xn, yn, _ = _inputs((2, 2, n), J, 28)
        xfm, ifm = modules(dev, wave, J)
        outs = {}
        for flag in (True, False):
            prev = ops.WPT1D_FUSED
            ops.WPT1D_FUSED = flag
            try:
                x = dev_t(xn, dtype, dev).requires_grad_(True)
                c0 = pw.launch_count()
                y = xfm(x)
                rec = ifm(dev_t(yn, dtype, dev), size=n)
                dx, = torch.autograd.grad(y, x, dev_t(yn, dtype, dev))
                ks = names_since(c0)
            finally:
                ops.WPT1D_FUSED = prev
            assert any(k.startswith('WlWpt1d') for k in ks) == flag, (flag, ks)
            outs[flag] = [y, rec, dx]
        for i, (a, b) in enumerate(zip(outs[True], outs[False])):
            close(a, npy(b), dtype, 'fused against level by level %s output %d' % (wave, i))


def check_errors_and_edges(dev):
    x = dev_t(_inputs((2, 2, 32), 1, 29)[0], F32, dev)
    y = pw.WPT1DForward(J=0, wave='db2', mode=PER).to(dev)(x)
    assert y.shape == (2, 2, 1, 32) and torch.equal(y[:, :, 0], x)
    assert torch.equal(pw.WPT1DInverse(wave='db2', mode=PER).to(dev)(y), x)
    xfm, ifm = modules(dev, 'db2', 2)
    with pytest.raises(ValueError, match='no power of 2'):
        ifm(torch.zeros(2, 2, 3, 8, device=dev))
    with pytest.raises(ValueError, match='coefficients per band'):
        ifm(xfm(x), size=34)
    assert ifm(xfm(x), size=32).shape == x.shape
    for bad in (x[0], x[None, None]):
        with pytest.raises(ValueError):
            xfm(bad)
    for bad in (x, xfm(x)[None]):
        with pytest.raises(ValueError):
            ifm(bad)
    e = xfm(x[:0])
    assert e.shape == (0, 2, 4, 8) and ifm(e, size=32).shape == (0, 2, 32)
    assert pw.WPT1D is pw.WPT1DForward and pw.IWPT1D is pw.WPT1DInverse
    assert all(k in pw.__all__ for k in ('WPT1DForward', 'WPT1DInverse', 'WPT1D', 'IWPT1D', 'wpt1d_freq_order'))
    # the function level: one level = the module's J = 1, taps as pywt orders them
    w = filters.Wavelet('db2')
    one = lowlevel.wpt1d_level(x, w.dec_lo, w.dec_hi, PER)
    assert torch.equal(one, pw.WPT1DForward(J=1, wave='db2', mode=PER).to(dev)(x))
    back = lowlevel.iwpt1d_level(one, w.rec_lo, w.rec_hi, PER, out_len=32)
    assert float((back - x).abs().max()) <= 2e-5 * max(1.0, float(x.abs().max()))
    with pytest.raises(ValueError):
        lowlevel.iwpt1d_level(one, w.rec_lo, w.rec_hi, PER, out_len=40)
    # the C entries outside their envelope decline: the wrappers return None
    h = _launch_taps(dev, ana_taps('db2'))
    assert ops.wpt1d_afb(x.double(), h[0], h[1], 2, 1) is None and ops.wpt1d_afb(x, h[0], h[1], 2, 4) is None
    assert ops.wpt1d_afb(x, h[0][:3], h[1][:3], 2, 1) is None and ops.wpt1d_afb(x, h[0], h[1], 0, 1) is None
    assert ops.wpt1d_afb(x[..., :30], h[0], h[1], 2, 2) is None and ops.wpt1d_afb(x[..., :4], h[0], h[1], 2, 2) is None
    assert ops.wpt1d_sfb(x.view(2, 2, 4, 8), h[0], h[1], 1, 2) is None
    be, unsupported = ops._backend(), _lib.WL_ERR_UNSUPPORTED
    out = torch.empty_like(x)
    args = (x.data_ptr(), out.data_ptr(), 0, 4, 32, 1, h[0].data_ptr(), h[1].data_ptr(), 4)
    for fn in (be.wl_wpt1d_analysis, be.wl_wpt1d_synthesis):
        assert fn(*(args + (0, 0, None))) == unsupported                                     # not periodization
        assert fn(*(args[:2] + (2,) + args[3:] + (2, 0, None))) == unsupported               # float64
        assert fn(*(args[:-1] + (22, 2, 0, None))) == unsupported                            # 22 taps
        assert fn(*(args[:4] + (30, 2) + args[6:] + (2, 0, None))) == unsupported            # 30 % 4
        assert fn(*(args[:4] + (4, 2) + args[6:] + (2, 0, None))) == unsupported             # level 2 reads 2 samples with 4 taps
        assert fn(*(args[:5] + (4,) + args[6:] + (2, 0, None))) == unsupported               # four levels
        assert fn(*(args + (2, 1, None))) not in (0, unsupported)                            # origin off the 2**nlev grid
        assert fn(*(args + (2, ops.wpt1d_core(4, 1), None))) not in (0, unsupported)         # origin past the core


def check_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.WPT1DForward(J=2, wave='db2', mode=PER)(torch.zeros(1, 1, 16))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.WPT1DInverse(wave='db2', mode=PER)(torch.zeros(1, 1, 4, 4))


def check_views(dev):
    """An offset base, a cropped last axis, a strided channel slice and cotangents that are views give the answers of their
    contiguous copies, bit for bit."""
    n, J = 296, 3
    xfm, ifm = modules(dev, 'db4', J)
    base = dev_t(_inputs((2, 4, n + 16), J, 30)[0], F32, dev)
    flat = dev_t(_inputs((1, 1, 2 * 3 * n + 1), 0, 30)[0], F32, dev).reshape(-1)
    cuts = (lambda t: t[..., 8:-8], lambda t: t[:, ::2, :n], lambda t: flat[1:].view(2, 3, n))
    for cut in cuts:
        view = cut(base)
        assert not view.is_contiguous() or view.data_ptr() % 16
        a, b = xfm(view), xfm(view.contiguous())
        assert torch.equal(a, b)
    cbase = dev_t(_inputs((2, 3, 16, n >> J), 0, 31)[0], F32, dev)
    for cut in (lambda t: t[:, :, ::2], lambda t: t[:, 1:, 8:], lambda t: t[:, :, :8].transpose(0, 1)[:, :2]):
        view = cut(cbase)
        assert not view.is_contiguous()
        assert torch.equal(ifm(view), ifm(view.contiguous()))
    x = base[..., :n].contiguous().requires_grad_(True)
    y = xfm(x)
    cot = dev_t(_inputs((2, 4, 16, n >> J), 0, 32)[0], F32, dev)[:, :, ::2]
    assert not cot.is_contiguous()
    ga, = torch.autograd.grad(y, x, cot, retain_graph=True)
    gb, = torch.autograd.grad(y, x, cot.contiguous())
    assert torch.equal(ga, gb)
    c = cbase[:, :, :8].contiguous().requires_grad_(True)
    rec = ifm(c)
    cot = base[:, :3, 4:n + 4]
    ga, = torch.autograd.grad(rec, c, cot, retain_graph=True)
    gb, = torch.autograd.grad(rec, c, cot.contiguous())
    assert torch.equal(ga, gb)


def check_state_dict(dev):
    dst = pw.WPT1DForward(J=2, wave='db1').to(dev)
    with pytest.raises(RuntimeError):
        dst.load_state_dict(pw.DWT1DForward(J=2, wave='db3').to(dev).state_dict())       # (db1's buffers hold two taps)
    dst = pw.WPT1DForward(J=2, wave='db5').to(dev)
    res = dst.load_state_dict(pw.DWT1DForward(J=2, wave='sym5').to(dev).state_dict())
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(dst.h0, pw.DWT1DForward(wave='sym5').h0.to(dev)) and sorted(dst.state_dict()) == ['h0', 'h1']
    inv = pw.WPT1DInverse(wave='db5').to(dev)
    res = inv.load_state_dict(pw.DWT1DInverse(wave='sym5').to(dev).state_dict())
    assert not res.missing_keys and not res.unexpected_keys and sorted(inv.state_dict()) == ['g0', 'g1']
    assert torch.equal(inv.g0, pw.DWT1DInverse(wave='sym5').g0.to(dev))


def check_freq_order():
    """wpt1d_freq_order(J) is a permutation, the 1-D case of wpt2d_freq_order; and (J <= 3, the oracle's tree, no kernel) a pure
    sinusoid in the middle of frequency slot f puts its energy into band idx[f]."""
    for J in range(0, 7):
        idx = pw.wpt1d_freq_order(J)
        assert sorted(idx) == list(range(2 ** J))
        # (the first row of the 2-D order - H lowest - carries the W path in the twos of its base-4 digits)
        assert [int(bin(b)[2:], 4) * 2 for b in idx] == pw.wpt2d_freq_order(J)[:2 ** J]
        for f, b in enumerate(idx):
            assert b == f ^ (f >> 1)
    n = 1024
    t = np.arange(n)
    for J in (1, 2, 3):
        idx = pw.wpt1d_freq_order(J)
        for f in range(2 ** J):
            cycles = round((f + 0.5) / 2 ** J * n / 2)                   # a whole number of periods in the (periodized) row
            y = tree_ref(np.cos(2 * np.pi * cycles * t / n)[None], filters.dwt_analysis_taps('db10'), J)[0]
            energy = (y ** 2).sum(-1)
            assert int(np.argmax(energy)) == idx[f] and energy[idx[f]] > 0.6 * energy.sum(), (J, f, energy)
