"""Goldens of the 1-D DTCWT (tests/golden/dtcwt1d_*.npz) from the REFERENCE's own CPU column primitives in float64:

    PYTHONPATH=tools/ref_shim:<reference checkout> python tools/make_dtcwt1d_golden.py

Per file: the input x (1, 3, n), yl, yh0 .., the reconstruction `rec` of (yl, yh), seeded cotangents c0 (of yl), c1 .. (of yh) and
dx = torch.autograd.grad through the reference's primitives.  The composition is the 2-D transform's level structure carried to
one axis (dtcwt/transform2d.py:117-133, :235-236 of the reference).  No test imports the reference."""
import os

import numpy as np
import torch
from pytorch_wavelets.dtcwt import lowlevel as rl
from pytorch_wavelets.dtcwt.coeffs import biort as _biort, qshift as _qshift

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')
CASES = [('near_sym_a', 'qshift_a', 22, 3), ('near_sym_b', 'qshift_b', 37, 4), ('legall', 'qshift_06', 20, 3),
         ('antonini', 'qshift_c', 36, 3), ('near_sym_b', 'qshift_d', 100, 4)]


def prep(h):
    return rl.prep_filt(h, 1).double()


def col(fn, x, *a):
    return fn(x.unsqueeze(-1), *a).squeeze(-1)


def forward(x, J, f):
    h0o, h1o, h0a, h0b, h1a, h1b = f
    if x.shape[-1] % 2:
        x = torch.cat((x, x[..., -1:]), dim=-1)
    lo, hi = col(rl.colfilter, x, h0o), col(rl.colfilter, x, h1o)
    yh = [hi.reshape(hi.shape[:-1] + (-1, 2))]
    for _ in range(1, J):
        if lo.shape[-1] % 4:
            lo = torch.cat((lo[..., :1], lo, lo[..., -1:]), dim=-1)
        hi = col(rl.coldfilt, lo, h1b, h1a, True)
        lo = col(rl.coldfilt, lo, h0b, h0a, False)
        yh.append(hi.reshape(hi.shape[:-1] + (-1, 2)))
    return lo, yh


def inverse(lo, yh, g):
    g0o, g1o, g0a, g0b, g1a, g1b = g
    for j in range(len(yh) - 1, -1, -1):
        h = yh[j].reshape(yh[j].shape[:-2] + (-1,))
        if lo.shape[-1] != h.shape[-1]:
            lo = lo[..., 1:-1]
        if j == 0:
            lo = col(rl.colfilter, lo, g0o) + col(rl.colfilter, h, g1o)
        else:
            lo = col(rl.colifilt, lo, g0b, g0a, False) + col(rl.colifilt, h, g1b, g1a, True)
    return lo


def main():
    torch.set_default_dtype(torch.float64)
    for i, (b, q, n, J) in enumerate(CASES):
        h0o, g0o, h1o, g1o = _biort(b)
        h0a, h0b, g0a, g0b, h1a, h1b, g1a, g1b = _qshift(q)
        f = [prep(v) for v in (h0o, h1o, h0a, h0b, h1a, h1b)]
        g = [prep(v) for v in (g0o, g1o, g0a, g0b, g1a, g1b)]
        rs = np.random.RandomState(100 + i)
        x = torch.tensor(rs.randn(1, 3, n), requires_grad=True)
        yl, yh = forward(x, J, f)
        cots = [torch.tensor(rs.randn(*t.shape)) for t in [yl] + yh]
        dx, = torch.autograd.grad([yl] + yh, x, cots)
        rec = inverse(yl.detach(), [h.detach() for h in yh], g)
        d = dict(biort=b, qshift=q, J=J, x=x.detach().numpy(), yl=yl.detach().numpy(), rec=rec.numpy(), dx=dx.numpy())
        for j in range(J):
            d['yh%d' % j] = yh[j].detach().numpy()
        for k, c in enumerate(cots):
            d['c%d' % k] = c.numpy()
        np.savez(os.path.join(OUT, 'dtcwt1d_%02d.npz' % i), **d)
        print('dtcwt1d_%02d' % i, b, q, n, J, 'round trip', float((rec[..., :n] - x.detach()).abs().max()))


if __name__ == '__main__':
    main()
