"""The shared synthesis ladder (dwt/lowlevel.py: _synthesis_ladder) on the real chip, on both of its device-side paths - several
levels in one launch with the crop as a view, and the lone wide level that the strip kernel crops itself: forward and inverse
against the oracle, x.grad against the per-level tile path, relative error at most 1e-5 of the reference's largest magnitude.

Two cases of tests/_route_cases.py.  The engine's policy asks the multi-level kernels only when the planes fill the chip
(ops.sfb2d_fused: 8 * planes >= 3 * CUs; twelve planes of 96 x 80 are too few for 256 CUs and too large for the small-plane
kernel) and leaves a strip launch that does not fill it to the launcher's judgement, so the streaming kernels are pinned the
way the other tests pin them (ops.FUSED_STRIPS / ops.STREAM_FORCE): without that the cases could take the per-level tile
kernels on the real chip and touch neither path."""
import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import ops
from pytorch_wavelets_amd.dwt import lowlevel

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = 'cuda:0'


def _run(x0, xfm, ifm):
    """(yl, yh, rec, x.grad, the inverse's launches) of a forward, an inverse and one backward pass through both."""
    x = x0.clone().requires_grad_(True)
    yl, yh = xfm(x)
    c0 = pw.launch_count()
    rec = ifm((yl, yh))
    ks = [k for k in pw.kernels_since(c0) if not k.endswith(')')]        # (without the auxiliary / armed launches of a hinted variant)
    (rec.square().sum() + yh[0].sum()).backward()
    return yl.detach(), [h.detach() for h in yh], rec.detach(), x.grad.detach(), ks


def _close(a, ref, what):
    a, ref = a.double().cpu().numpy(), np.asarray(ref, dtype=np.float64)
    err, bound = float(np.abs(a - ref).max()), TOL * float(np.abs(ref).max())
    print('%s: max err %.3e, bound %.3e' % (what, err, bound))
    assert a.shape == ref.shape and err <= bound, (what, err, bound)


@pytest.mark.parametrize('shape,J,pin', [((12, 96, 80), 3, 'FUSED_STRIPS'), ((2, 40, 704), 1, 'STREAM_FORCE')])
def test_synthesis_ladder_paths_vs_oracle(shape, J, pin, monkeypatch):
    wave, mode = 'db2', 'symmetric'
    planes, H, W = shape
    x0 = torch.tensor(np.random.RandomState(3).randn(planes, 1, H, W), dtype=torch.float32, device=DEV)
    xfm, ifm = pw.DWTForward(J=J, wave=wave, mode=mode).to(DEV), pw.DWTInverse(wave=wave, mode=mode).to(DEV)
    with monkeypatch.context() as m:
        m.setattr(ops, pin, 1 if pin == 'FUSED_STRIPS' else True)
        yl, yh, rec, gx, ks = _run(x0, xfm, ifm)
    print(shape, 'inverse:', ks)
    if pin == 'FUSED_STRIPS':       # all three levels in one launch (which of the two kernels is the chip's and the engine's affair)
        assert len(ks) == 1 and ks[0].startswith(('WlSfbRows<', 'WlSfbSmall<')), ks
    else:                           # the lone wide level on the strip kernel
        assert ks[-1].startswith('WlSfbStrip<'), ks
    f = [b.double().cpu().numpy().ravel() for b in (xfm.h0_col, xfm.h1_col, xfm.h0_row, xfm.h1_row)]
    g = [b.double().cpu().numpy().ravel() for b in (ifm.g0_col, ifm.g1_col, ifm.g0_row, ifm.g1_row)]
    oyl, oyh = wo.dwt_forward(x0.double().cpu().numpy(), J, f[0], f[1], f[2], f[3], mode)
    _close(yl, oyl, 'yl')
    for j in range(J):
        _close(yh[j], oyh[j], 'yh%d' % j)
    _close(rec, wo.dwt_inverse(yl.double().cpu().numpy(), [h.double().cpu().numpy() for h in yh], g[0], g[1], g[2], g[3], mode), 'rec')
    # the gradient's reference: one tile-kernel launch per level
    monkeypatch.setattr(lowlevel, 'FUSED_LEVELS', False)
    ops.set_option('no_stream', 1)
    try:
        ref = _run(x0, xfm, ifm)
    finally:
        ops.set_option('no_stream', 0)
    assert all('Tile' in k for k in ref[4]), ref[4]
    _close(gx, ref[3].double().cpu().numpy(), 'x.grad')
