"""CPU tests (host emulation of the kernels): the transposed a-trous bank (wl_iswt2d_level, wl_corr1d_adj), the gradient of
SWTForward / afb2d_atrous / afb1d_atrous and SWTInverse, against matrices built from the pinned oracle (tests/_swt_inv_cases.py)."""
import numpy as np
import pytest
import torch

import _swt_inv_cases as S
import emu_backend
import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import filters
from pytorch_wavelets_amd.dwt import lowlevel as dwl
from pytorch_wavelets_amd.dwt.transform2d import SWTForward

F64, F32, F16 = torch.float64, torch.float32, torch.float16

# (taps along W, taps along H, mode, dilation, shape, dtype): every pad mode, dilations 1-4, ragged tiles, compile-time tap
# counts, run-time ones (db7 = 14 taps; db2 against db3 = two different banks for the two axes), the three storage types
ADJ_CASES = [('db2', 'db2', 'periodic', 1, (1, 2, 20, 24), F64), ('db2', 'db2', 'symmetric', 2, (2, 1, 37, 70), F32),
             ('db4', 'db4', 'reflect', 4, (1, 1, 45, 130), F32), ('haar', 'haar', 'zero', 1, (1, 3, 5, 7), F32),
             ('db3', 'db3', 'replicate', 2, (1, 2, 33, 65), F16), ('db7', 'db7', 'constant', 1, (1, 1, 40, 64), F32),
             ('db10', 'db10', 'symmetric', 2, (1, 1, 36, 30), F32), ('db4', 'db4', 'symmetric', 2, (1, 1, 36, 30), F64),
             ('db5', 'db5', 'periodic', 3, (1, 1, 16, 200), F32), ('db2', 'db3', 'zero', 2, (2, 1, 37, 70), F32),
             ('db3', 'db2', 'periodic', 4, (1, 2, 45, 130), F64), ('db4', 'db4', 'periodic', 2, (1, 2, 33, 65), F16),
             ('db2', 'db2', 'replicate', 3, (1, 1, 5, 7), F64), ('db3', 'db3', 'reflect', 1, (1, 2, 5, 7), F64),
             ('db2', 'db2', 'constant', 3, (1, 1, 37, 70), F16), ('db7', 'db7', 'periodic', 1, (1, 1, 40, 64), F64)]


@pytest.mark.parametrize('wrow,wcol,mode,dil,shape,dtype', ADJ_CASES)
def test_adjoint_level_vs_oracle_transpose(wrow, wcol, mode, dil, shape, dtype):
    """The gradient of afb2d_atrous and the replace / add / ll-only forms of the transposed level: one WlSwtInvLevel launch for
    the rules the fused kernel takes, three WlCorr1dAdj launches for the ones it hands over."""
    with emu_backend.emulated():
        S.check_adjoint('cpu', wrow, wcol, mode, dil, shape, dtype)


@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('wave,dil,shape,dtype', [('db2', 1, (1, 2, 20, 24), F64), ('db7', 3, (1, 1, 37, 70), F32),
                                                  ('db3', 2, (2, 1, 33, 65), F16), ('db4', 4, (1, 1, 5, 7), F64)])
def test_adjoint_on_the_single_axis_kernel_every_mode(monkeypatch, mode, wave, dil, shape, dtype):
    """The same transposes with the fused kernel switched off: wl_corr1d_adj carries every rule, with as many folds as the pad
    is long (db4 dilated by 4 on 5 x 7: the pad is several signals long), along H and along W."""
    monkeypatch.setattr(dwl, 'FUSED_LEVELS', False)
    with emu_backend.emulated():
        S.check_adjoint('cpu', wave, wave, mode, dil, shape, dtype, fused=False)
        S.check_adjoint_1d('cpu', wave, mode, dil, shape, 2, dtype)
        S.check_adjoint_1d('cpu', wave, mode, dil, shape, 3, dtype)


@pytest.mark.parametrize('mode', ['periodic', 'zero', 'symmetric', 'reflect', 'replicate'])
def test_pad_longer_than_the_signal_goes_to_the_single_axis_kernel(mode):
    """db10 dilated by 8 on 24 x 40: the dilated filter does not fit a tile in LDS (and its pad is longer than the signal) - the
    fused kernel declines, wl_corr1d_adj gives the transpose."""
    h0, h1 = filters.dwt_analysis_taps('db10')
    dy = np.random.RandomState(2).randn(1, 4, 24, 40)
    with emu_backend.emulated():
        x = torch.zeros(1, 1, 24, 40, dtype=F64, requires_grad=True)
        y = dwl.afb2d_atrous(x, S.filts4((h0, h1), (h0, h1), 'cpu'), mode, 8)
        c0 = pw.launch_count()
        dx, = torch.autograd.grad(y, x, torch.tensor(dy))
        ks = pw.kernels_since(c0)
    assert len(ks) == 3 and all(k.startswith('WlCorr1dAdj') for k in ks), ks
    ref = S.adj2d_ref(dy, (h0, h1), (h0, h1), mode, 8, (24, 40))
    S.close(dx, ref, F64, 'long pad ' + mode)


@pytest.mark.parametrize('mode', ['periodic', 'symmetric'])
def test_gradcheck_swt_forward(mode):
    xfm, _ = S.swt_modules('cpu', 'db2', 'db2', 2, mode=mode)
    x = torch.randn(1, 2, 6, 7, dtype=F64, requires_grad=True)
    with emu_backend.emulated():
        assert torch.autograd.gradcheck(lambda v: tuple(xfm(v)), (x,), eps=1e-6, atol=1e-8)


def test_gradcheck_swt_inverse_and_banks():
    _, ifm = S.swt_modules('cpu', 'bior2.2', 'bior2.2', 2)
    cs = [torch.randn(1, 8, 6, 7, dtype=F64, requires_grad=True) for _ in range(2)]
    g0, g1 = (torch.tensor(g) for g in filters.dwt_synthesis_taps('db2'))
    lo, hi = (torch.randn(1, 2, 5, 6, dtype=F64, requires_grad=True) for _ in range(2))
    with emu_backend.emulated():
        assert torch.autograd.gradcheck(lambda a, b: ifm([a, b]), tuple(cs), eps=1e-6, atol=1e-8)
        assert torch.autograd.gradcheck(lambda a, b: dwl.sfb1d_atrous(a, b, g0, g1, 'periodic', 2, 2), (lo, hi), eps=1e-6, atol=1e-8)
        assert torch.autograd.gradcheck(lambda a, b: dwl.sfb1d_atrous(a, b, g0, g1, 'periodic', 3, 1), (lo, hi), eps=1e-6, atol=1e-8)


@pytest.mark.parametrize('mode', S.MODES)
def test_inner_product_identity(mode):
    """<A x, y> == <x, A^T y> through SWTForward (J = 2) and its backward."""
    rng = np.random.RandomState(4)
    xfm, _ = S.swt_modules('cpu', 'db3', 'db3', 2, mode=mode)
    x = torch.tensor(rng.randn(2, 2, 19, 33), requires_grad=True)
    with emu_backend.emulated():
        ys = xfm(x)
        assert all(y.grad_fn is not None for y in ys)
        cots = [torch.tensor(rng.randn(*y.shape)) for y in ys]
        dx, = torch.autograd.grad(ys, x, cots)
    lhs = sum(float((y.detach() * c).sum()) for y, c in zip(ys, cots))
    rhs = float((x.detach() * dx).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)), (lhs, rhs)


@pytest.mark.parametrize('mode', ['periodic', 'symmetric'])
def test_backward_one_launch_per_level_and_unused_levels_are_zeros(mode):
    rng = np.random.RandomState(8)
    xfm, _ = S.swt_modules('cpu', 'db2', 'db2', 3, mode=mode)
    xv = rng.randn(1, 2, 20, 24)
    cots = [torch.tensor(rng.randn(1, 8, 20, 24)) for _ in range(3)]
    with emu_backend.emulated():
        def grad(used):
            x = torch.tensor(xv, requires_grad=True)
            ys = xfm(x)
            c0 = pw.launch_count()
            sum((ys[j] * cots[j]).sum() for j in used).backward()
            assert x.grad is not None
            return x.grad, pw.kernels_since(c0)
        full, ks = grad([0, 1, 2])
        if mode == 'periodic':
            assert len(ks) == 3 and all(k.startswith('WlSwtInvLevel') for k in ks), ks
        for used in ([0], [1], [2], [0, 2]):
            got, ks = grad(used)
            x = torch.tensor(xv, requires_grad=True)
            ys = xfm(x)
            want, = torch.autograd.grad(ys, x, [cots[j] if j in used else torch.zeros_like(cots[j]) for j in range(3)])
            assert float((got - want).abs().max()) <= 1e-12, used
            if mode == 'periodic':
                assert len(ks) == max(used) + 1 and all(k.startswith('WlSwtInvLevel') for k in ks), (used, ks)


# float64 round trips use wavelets whose tabulated filters satisfy perfect reconstruction to rounding: 1/2 (B_0^T A_0 + B_1^T A_1)
# - I, formed from the oracle's matrices alone, is below 3e-16 for haar, db*, coif2, bior1.3, bior2.2 and rbio3.5, but 8.5e-13
# for bior4.4 and 1.8e-13 for sym5 / bior6.8 (pywt tabulates those to fewer digits), which a two-level 2-D round trip
# compounds past the 1e-12 bound whatever computes it.  Those run in float32 here and, in float64, against the matrix formula
# below, which is exact for any filters.
RT_CASES = [('haar', 1, (1, 1, 16, 16), F64), ('db2', 2, (1, 2, 20, 24), F64), ('db4', 3, (2, 3, 37, 45), F64),
            ('bior2.2', 3, (1, 2, 21, 35), F64), ('bior1.3', 2, (1, 1, 33, 70), F64), ('rbio3.5', 2, (1, 1, 40, 64), F64),
            ('db7', 1, (1, 1, 40, 64), F64), ('coif2', 2, (1, 2, 13, 37), F64), ('db2', 3, (2, 3, 37, 45), F32),
            ('bior2.2', 2, (1, 2, 33, 70), F32), ('bior4.4', 2, (1, 1, 33, 70), F32), ('sym5', 2, (1, 1, 13, 37), F32)]


@pytest.mark.parametrize('wave,J,shape,dtype', RT_CASES)
def test_inverse_reconstructs(wave, J, shape, dtype):
    with emu_backend.emulated():
        S.check_roundtrip('cpu', wave, J, shape, dtype)


@pytest.mark.parametrize('dtype', [F64, F32])
def test_inverse_with_separate_row_and_column_banks(dtype):
    fwd, inv = S.reversed_db2()
    with emu_backend.emulated():
        S.check_roundtrip('cpu', 'db2 / reversed db2', 3, (2, 3, 21, 37), dtype, waves=(fwd, inv))


@pytest.mark.parametrize('wave,J,shape,dtype', [('bior2.2', 3, (1, 2, 20, 24), F64), ('db4', 2, (2, 1, 37, 70), F32), ('db7', 2, (1, 1, 33, 65), F64),
                                                ('db3', 2, (1, 2, 33, 65), F16), ('bior4.4', 2, (1, 1, 33, 70), F64), ('bior6.8', 2, (1, 1, 13, 37), F64)])
def test_inverse_equals_the_matrix_formula_on_random_coefficients(wave, J, shape, dtype):
    """Coefficients that are not in the range of the forward; and the ll channels of the finer levels do not matter."""
    rng = np.random.RandomState(9)
    N, C, H, W = shape
    g = filters.dwt_synthesis_taps(wave)
    _, ifm = S.swt_modules('cpu', wave, wave, J, dtype=F64 if dtype == F64 else F32)
    coeffs = [torch.tensor(rng.randn(N, 4 * C, H, W)).to(dtype) for _ in range(J)]
    ref = S.inv_ref([S.npy(c) for c in coeffs], g, g)
    with emu_backend.emulated():
        c0 = pw.launch_count()
        rec = ifm(coeffs)
        ks = pw.kernels_since(c0)
        assert len(ks) == J and all(k.startswith('WlSwtInvLevel') for k in ks), ks
        S.close(rec, ref, dtype, 'inverse ' + wave)
        edited = [c.clone() for c in coeffs]
        for c in edited[:-1]:
            c[:, 0::4] = 7.0
        assert torch.equal(ifm(edited), rec)


def test_bfloat16_takes_the_float16_kernels():
    with emu_backend.emulated():
        S.check_bf16('cpu', (1, 2, 20, 24))


def test_function_level_banks_invert_the_atrous_banks():
    """sfb1d_atrous / sfb2d_atrous with pywt-ordered arrays, as sfb1d / sfb2d take them."""
    rng = np.random.RandomState(10)
    w = filters.Wavelet('bior2.2')
    x = torch.tensor(rng.randn(1, 2, 13, 18))
    with emu_backend.emulated():
        for d in (1, 2, 3):
            for dim in (2, 3):
                y = dwl.afb1d_atrous(x, w.dec_lo, w.dec_hi, 'periodic', dim, d).double()
                rec = dwl.sfb1d_atrous(y[:, 0::2].contiguous(), y[:, 1::2], w.rec_lo, w.rec_hi, 'periodic', dim, d)
                assert float((rec - x).abs().max()) < 1e-6            # (array filters become float32 taps, like sfb1d's)
            y = dwl.afb2d_atrous(x, (w.dec_lo, w.dec_hi), 'periodic', d)
            rec = dwl.sfb2d_atrous(y[:, 0::4], y[:, 1::4], y[:, 2::4], y[:, 3::4], (w.rec_lo, w.rec_hi), 'periodic', d)
            assert rec.shape == x.shape and float((rec - x).abs().max()) < 1e-6
        g = tuple(torch.tensor(v) for v in filters.dwt_synthesis_taps('bior2.2'))
        h = tuple(torch.tensor(v) for v in filters.dwt_analysis_taps('bior2.2'))
        y = dwl.afb1d_atrous(x, h[0], h[1], 'periodic', 3, 2)
        rec = dwl.sfb1d_atrous(y[:, 0::2], y[:, 1::2], g[0], g[1], 'periodic', 3, 2)
        assert float((rec - x).abs().max()) < 1e-12


def test_training_step_through_forward_and_inverse():
    xfm, ifm = S.swt_modules('cpu', 'db2', 'db2', 2)
    x = torch.randn(2, 3, 16, 20, dtype=F64, requires_grad=True)
    with emu_backend.emulated():
        coeffs = xfm(x)
        rec = ifm([c * 0.5 for c in coeffs])
        loss = (rec - x.detach()).square().sum()
        loss.backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    # rec = x / 2 (the transform is linear and inverted exactly): d/dx sum (x/2 - x0)^2 at x0 = x is -x/2
    assert float((x.grad + 0.5 * x.detach()).abs().max()) < 1e-11


def test_errors_and_the_reference_import_path():
    from pytorch_wavelets_amd.dwt.swt_inverse import SWTInverse, sfb1d_atrous, sfb2d_atrous
    from pytorch_wavelets_amd.dwt import transform2d
    assert SWTInverse is transform2d.SWTInverse and sfb1d_atrous is dwl.sfb1d_atrous and sfb2d_atrous is dwl.sfb2d_atrous
    for mode in ('symmetric', 'zero', 'periodization', 'nonsense', None):
        with pytest.raises(ValueError):
            SWTInverse(wave='db2', mode=mode)
    with pytest.raises(ValueError):
        SWTInverse(wave=([1.0, 1.0, 1.0], [1.0, -2.0, 1.0]))                 # odd tap count
    ifm = SWTInverse(wave='db2')
    assert sorted(dict(ifm.named_buffers())) == ['g0_col', 'g0_row', 'g1_col', 'g1_row']
    x = torch.randn(1, 4, 8, 8)
    with emu_backend.emulated():
        with pytest.raises(ValueError):
            ifm([x, torch.randn(1, 4, 8, 10)])                                # mismatched levels
        with pytest.raises(ValueError):
            ifm([torch.randn(1, 3, 8, 8)])                                    # not four bands per channel
        with pytest.raises(ValueError):
            ifm([])
        with pytest.raises(ValueError):
            sfb1d_atrous(x, x, [1.0, 1.0], [1.0, -1.0], mode='symmetric')
        with pytest.raises(ValueError):
            sfb2d_atrous(x, x, x, x, ([1.0, 1.0], [1.0, -1.0]), mode='zero')
        with pytest.raises(ValueError, match='Unkown pad type'):
            SWTForward(J=1, wave='db2', mode='periodization')(x)
        # the module reads its buffers on every call
        ifm.g0_col.mul_(2.0)
        a = ifm([x])
        ifm.g0_col.mul_(0.5)
        assert not torch.equal(a, ifm([x]))
