"""-m gpu: the transposed a-trous bank (wl_iswt2d_level / wl_corr1d_adj), SWTForward's gradient and SWTInverse through the
C ABI on the MI355X, against matrices built from the pinned oracle (tests/_swt_inv_cases.py)."""
import numpy as np
import pytest
import torch

import _swt_inv_cases as S
import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import filters
from pytorch_wavelets_amd.dwt import lowlevel as dwl

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16


@pytest.mark.parametrize('wrow,wcol,mode,dil,shape,dtype', [
    ('db2', 'db2', 'periodic', 1, (1, 2, 20, 24), F64), ('db2', 'db3', 'zero', 2, (2, 1, 37, 70), F32),
    ('db4', 'db4', 'reflect', 4, (1, 1, 45, 130), F32), ('db3', 'db3', 'replicate', 2, (1, 2, 33, 65), F16),
    ('db7', 'db7', 'constant', 1, (1, 1, 40, 64), F32), ('db2', 'db2', 'symmetric', 3, (2, 1, 37, 70), F64),
    ('db5', 'db5', 'periodic', 3, (1, 1, 16, 200), F32), ('db4', 'db4', 'periodic', 2, (2, 2, 70, 130), F16),
    ('db10', 'db10', 'periodic', 8, (1, 1, 24, 40), F64),
    # tiles that fit no four rows in 64 KiB of LDS and take the 160 KiB budget (132 KiB and 150 KiB): still the fused kernel
    ('db10', 'db10', 'periodic', 3, (1, 2, 40, 70), F32), ('db4', 'db4', 'zero', 4, (1, 1, 45, 130), F64)])
def test_adjoint_level_vs_oracle_transpose(wrow, wcol, mode, dil, shape, dtype):
    S.check_adjoint(DEV, wrow, wcol, mode, dil, shape, dtype, fused=not (wrow == 'db10' and dil == 8))


@pytest.mark.parametrize('mode', S.MODES)
def test_adjoint_on_the_single_axis_kernel_every_mode(monkeypatch, mode):
    monkeypatch.setattr(dwl, 'FUSED_LEVELS', False)
    S.check_adjoint(DEV, 'db4', 'db4', mode, 4, (1, 2, 9, 13), F64, fused=False)
    S.check_adjoint_1d(DEV, 'db3', mode, 2, (2, 1, 33, 65), 2, F32)
    S.check_adjoint_1d(DEV, 'db3', mode, 2, (2, 1, 33, 65), 3, F32)


@pytest.mark.parametrize('wave,J,shape,dtype', [('db2', 2, (1, 2, 20, 24), F64), ('bior2.2', 3, (1, 2, 21, 35), F64),
                                                ('db4', 3, (2, 3, 37, 45), F64), ('db7', 2, (2, 1, 64, 96), F32)])
def test_inverse_reconstructs_and_equals_the_matrix_formula(wave, J, shape, dtype):
    S.check_roundtrip(DEV, wave, J, shape, dtype)
    rng = np.random.RandomState(9)
    N, C, H, W = shape
    g = filters.dwt_synthesis_taps(wave)
    _, ifm = S.swt_modules(DEV, wave, wave, J, dtype=F64 if dtype == F64 else F32)
    coeffs = [torch.tensor(rng.randn(N, 4 * C, H, W)).to(dtype).to(DEV) for _ in range(J)]
    S.close(ifm(coeffs), S.inv_ref([S.npy(c) for c in coeffs], g, g), dtype, 'inverse ' + wave)


def test_inverse_with_separate_row_and_column_banks():
    fwd, inv = S.reversed_db2()
    S.check_roundtrip(DEV, 'db2 / reversed db2', 3, (2, 3, 21, 37), F64, waves=(fwd, inv))


@pytest.mark.parametrize('dtype', [F32, F16])
def test_flagship_shape_round_trip_and_gradient(dtype):
    """16 x 3 x 512 x 512, db2, periodic, J = 2: the round trip, and dx of SWTForward against the oracle's transpose on a
    sample of planes (the planes are independent: the transposes of levels 2 and 1 applied to those planes' cotangents)."""
    torch.manual_seed(0)
    h = filters.dwt_analysis_taps('db2')
    xfm, ifm = S.swt_modules(DEV, 'db2', 'db2', 2, dtype=F32)
    x = torch.randn(16, 3, 512, 512, device=DEV).to(dtype).requires_grad_(True)
    c0 = pw.launch_count()
    coeffs = xfm(x)
    assert [k.split('<')[0] for k in pw.kernels_since(c0)] == ['WlSwtLevel', 'WlSwtLevel']
    c0 = pw.launch_count()
    rec = ifm([c.detach() for c in coeffs])
    assert [k.split('<')[0] for k in pw.kernels_since(c0)] == ['WlSwtInvLevel', 'WlSwtInvLevel']
    err = float((rec.double() - x.detach().double()).abs().max())
    # float16 coefficients: every stored value carries a rounding of 2^-11 relative, two levels each way
    bound = S.TOL[dtype] * max(1.0, float(x.detach().abs().max()))
    print('round trip %s: max err %.3e, bound %.3e' % (dtype, err, bound))
    assert err <= bound
    cots = [torch.randn(c.shape, device=DEV).to(dtype) for c in coeffs]
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(coeffs, x, cots)
    assert [k.split('<')[0] for k in pw.kernels_since(c0)] == ['WlSwtInvLevel', 'WlSwtInvLevel']
    for n, c in ((0, 0), (7, 1), (15, 2)):
        d1, d2 = (S.npy(t[n:n + 1, 4 * c:4 * c + 4]) for t in cots)
        carry = S.adj2d_ref(d2, h, h, 'periodic', 2, (512, 512))
        d1[:, 0::4] += carry
        ref = S.adj2d_ref(d1, h, h, 'periodic', 1, (512, 512))
        S.close(dx[n:n + 1, c:c + 1], ref, dtype, 'dx plane (%d, %d)' % (n, c))


def test_bfloat16_inverse_and_gradient():
    S.check_bf16(DEV, (2, 2, 64, 96))


def test_training_step_through_forward_and_inverse():
    torch.manual_seed(1)
    xfm, ifm = S.swt_modules(DEV, 'db2', 'db2', 2, dtype=F32)
    x = torch.randn(4, 3, 128, 128, device=DEV, requires_grad=True)
    w = torch.full((1,), 0.5, device=DEV, requires_grad=True)
    coeffs = xfm(x)
    rec = ifm([c * w for c in coeffs])
    loss = (rec - x.detach()).square().sum()
    loss.backward()
    torch.cuda.synchronize()
    assert x.grad is not None and w.grad is not None
    # every band the inverse reads is scaled by w once (it ignores the ll channels of the finer level), so rec = w x:
    # loss = (w - 1)^2 sum x0^2 at x = x0 -> d/dx = 2 (w x - x0) w = -x / 2, d/dw = 2 (w - 1) sum x^2 = -sum x^2
    xd = x.detach().double()
    assert float((x.grad.double() + 0.5 * xd).abs().max()) <= 1e-4 * float(xd.abs().max())
    assert abs(float(w.grad) + float(xd.square().sum())) <= 1e-4 * float(xd.square().sum())
