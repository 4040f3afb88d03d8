"""The fused DWT kernels' HBM streams under their cache policy (csrc/wl_common.h: the non-temporal LDS-DMA forms and stream
stores; WL_ROWS_NT_* / WL_IROWS_NT_* pick the streams that take them).  A cache hint changes no arithmetic and no byte that is
written, so every case is the plain parity check - forward against the oracle, forward -> inverse against the input - on
shapes that reach each form of access the policy can sit on, forced onto WlAfbRows / WlSfbRows (strips = 1: whole planes,
strips = 2: every plane cut into a top and a bottom segment, what fewer planes than compute units get).

Tolerances are those of tests/test_dwt_gpu.py: 1e-5 relative (max-norm) in float32; 3e-3 against the oracle and 2e-2 for a
round trip in float16 (storage rounding only, half-ulp 2^-11).  bfloat16 has eight times float16's ulp (half-ulp 2^-8):
eight times float16's bounds, 2.4e-2 and 1.6e-1.

The 66-column case is a view of a buffer whose row pitch is a whole number of 16-byte pieces (68 floats / 72 halfs): the
analysis kernel loads rows as 16-byte pieces and declines a dense plane of such rows.  Its level-2 bands are 22 x 21: odd
rows of 84 bytes, which adjacent waves' store lines share, in planes of 1848 bytes, which end off a 16-byte boundary (the
synthesis loader's dword tail pieces)."""
import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters as F
from pytorch_wavelets_amd import ops
from pytorch_wavelets_amd.dwt import lowlevel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ORACLE_TOL = {torch.float32: 1e-5, torch.float16: 3e-3, torch.bfloat16: 8 * 3e-3}
TRIP_TOL = {torch.float32: 1e-5, torch.float16: 2e-2, torch.bfloat16: 8 * 2e-2}


def npy(v):
    return v.detach().cpu().double().numpy()


def rel(a, b):
    a = npy(a) if torch.is_tensor(a) else a
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def on_device(x, dtype):
    """x (CPU, float32) as `dtype` on the device; rows that are no whole 16-byte pieces: a view of a padded buffer."""
    es = torch.empty(0, dtype=dtype).element_size()
    W = x.shape[-1]
    q = 16 // es
    buf = torch.zeros(x.shape[:-1] + ((W + q - 1) // q * q,), dtype=dtype, device=DEV)
    view = buf[..., :W]
    view.copy_(x.to(dtype))
    return view


def taps(wave):
    h0, h1 = F.dwt_analysis_taps(wave)
    g0, g1 = F.dwt_synthesis_taps(wave)
    th = [torch.tensor(v, dtype=torch.float32, device=DEV) for v in (h0, h1, h0, h1)]
    tg = [torch.tensor(v, dtype=torch.float32, device=DEV) for v in (g0, g1, g0, g1)]
    return (h0, h1, g0, g1), th, tg


def fused_forward(x, th, mode, J, strips):
    c0 = pw.launch_count()
    res = ops.afb2d_fused(x, *th, lowlevel.mode_to_int(mode), J, strips=strips)
    ks = pw.kernels_since(c0)
    assert res is not None and any('WlAfbRows' in k for k in ks), ks
    return res


def fused_inverse(yl, yh, tg, mode, strips):
    c0 = pw.launch_count()
    rec = ops.sfb2d_fused(yl, list(yh), *tg, lowlevel.mode_to_int(mode), strips=strips)
    ks = pw.kernels_since(c0)
    assert rec is not None and any('WlSfbRows' in k for k in ks), ks
    return rec


CASES = [
    ('db4', 'symmetric', 3, (2, 3, 70, 66), torch.float32),
    ('db4', 'symmetric', 3, (2, 3, 70, 66), torch.float16),
    ('db4', 'symmetric', 3, (2, 3, 70, 66), torch.bfloat16),
    ('db4', 'symmetric', 3, (2, 3, 70, 70), torch.float16),        # band widths 38, 22, 14: all three levels both ways in 2-byte data
    ('db4', 'symmetric', 3, (2, 3, 70, 70), torch.bfloat16),
    ('db2', 'symmetric', 2, (8, 4, 40, 40), torch.float32),        # several planes per workgroup
    ('db4', 'periodization', 3, (2, 3, 64, 64), torch.float32),    # loader_per / emit_per, the pair the roll splits
]


@pytest.mark.parametrize('wave,mode,J,shape,dtype', CASES, ids=['%s-%s-J%d-%s-%s' % (c[0], c[1], c[2], 'x'.join(map(str, c[3])), str(c[4]).split('.')[-1])
                                                                  for c in CASES])
def test_fused_kernels_parity_under_the_stream_policy(wave, mode, J, shape, dtype):
    (h0, h1, g0, g1), th, tg = taps(wave)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(17))
    xd = on_device(x, dtype)
    xr = npy(xd)                                                   # the input as the kernels see it (rounded to dtype)
    oyl, oyh = wo.dwt_forward(xr, J, h0, h1, h0, h1, mode)
    otol, ttol = ORACLE_TOL[dtype], TRIP_TOL[dtype]
    # 2-byte data: the synthesis kernel copies its coefficients in 4-byte units and takes band rows of whole units only
    # (ops.sfb2d_fused).  66 columns give 21 at level 2: there the round trip is the finest level's alone (38 x 36 bands).
    whole_pyramid = dtype == torch.float32 or all(v.shape[-1] % 2 == 0 for v in oyh)
    for strips in (1, 2):
        yl, yh = fused_forward(xd, th, mode, J, strips)
        assert yl.dtype == dtype
        errs = [rel(yl, oyl)] + [rel(a, b) for a, b in zip(yh, oyh)]
        print('forward', strips, errs)
        assert max(errs) < otol, (strips, errs)
        if not whole_pyramid:
            yl, yh = fused_forward(xd, th, mode, 1, strips)
        rec = fused_inverse(yl, yh, tg, mode, strips)
        assert rec.dtype == dtype
        want = wo.dwt_inverse(npy(yl), [npy(v) for v in yh], g0, g1, g0, g1, mode)   # the inverse of the coefficients as stored
        e_inv, e_trip = rel(rec, want), rel(rec[..., :shape[2], :shape[3]], xr)
        print('inverse', strips, e_inv, e_trip)
        assert e_inv < otol and e_trip < ttol, (strips, e_inv, e_trip)


def test_forward_outputs_are_visible_to_their_consumers_at_once():
    """What the forward stores is read straight away by a reduction on the same stream and by a copy to the host: both see
    the same, complete, coefficients (no synchronize between the launch and its consumers)."""
    (h0, h1, _, _), th, _ = taps('db4')
    x = torch.randn(2, 3, 70, 66, generator=torch.Generator().manual_seed(18))
    xd = on_device(x, torch.float32)
    oyl, oyh = wo.dwt_forward(npy(xd), 3, h0, h1, h0, h1, 'symmetric')
    for strips in (1, 2):
        yl, yh = fused_forward(xd, th, 'symmetric', 3, strips)
        outs = [yl] + list(yh)
        sums = [v.double().sum() for v in outs]                    # device reductions, queued behind the kernel
        host = [v.cpu() for v in outs]                             # device -> host copies of the same buffers
        torch.cuda.synchronize()
        for v, s, h, o in zip(outs, sums, host, [oyl] + list(oyh)):
            # float64 sums of <= 1e4 float32 values in two orders: they differ by rounding alone, 1e-12 of sum|v| at the most;
            # one coefficient missing from either reader's view is O(1)
            assert abs(float(s) - float(h.double().sum())) <= 1e-12 * float(h.double().abs().sum())
            assert torch.equal(v.cpu(), h)                         # a copy made after the device has drained: the same bytes
            assert rel(h, o) < 1e-5
