"""Every instantiation the dispatchers of the fused 1-D DWT kernels compile - WlDwt1dFused<T, L> (csrc/wl_dwt1d_fused.h) and
WlIdwt1dFused<T, L> (csrc/wl_idwt1d_fused.h), L = 2 .. 20 x float32, float16, bfloat16 -, one tap count and element type per
call, run by the emulator (CPU) and the GPU test modules.

Expected values come from the pinned oracle in float64 on the rounded input: ``wo.dwt1d_forward`` for yl and every yh[j],
``wo.dwt1d_inverse`` of the engine's own coefficients for the reconstruction, and for dx the reference's definition of the
backward (which the dwt1d goldens pin): the oracle's synthesis chain run with the ANALYSIS taps, every level cropped to its
input length.

Shapes: three rows of N = 4203 (odd) samples, J = 4, symmetric - two analysis chunks (a seam inside every level) and three
synthesis chunks at every tap count, asserted through the launches' grids; three rows of 4204 samples, J = 2, periodization -
the whole wrapped row in one chunk, and the inverse and the backward level by level (the fused synthesis declines the mode).

Tolerances: the REL / REC tables of tests/_swt1d_cases.py - values and gradients relative to |ref|max, 1e-5 float32, 4e-3
float16, 3e-2 bfloat16; reconstructions absolute, times max(1, |ref|max), 2e-5 float32, 6e-3 float16 and for bfloat16 (no
entry there) the value bound 3e-2: its only error is the rounding of the output, 2^-9 of an element."""
import numpy as np
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters
from _swt1d_cases import REL, REC, close, dev_t, npy, ntaps
from _wpt2d_cases import TNAME, last_grid

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GRID_WAVES = tuple('db%d' % i for i in range(1, 11))        # L = 2, 4, .., 20: one case of the dispatchers' switch each
GRID_DTYPES = (F32, F16, BF16)
REC_ALL = dict(REC)
REC_ALL[BF16] = REL[BF16]
ROWS = 3
CASES = (('symmetric', 4, 4203, 2, 3), ('periodization', 2, 4204, 1, 0))   # mode, J, N, analysis chunks, synthesis chunks (0: declined)


def grad_ref(dlo, dhis, lens, h0, h1, mode):
    """The reference's backward of the level chain: the synthesis with the analysis taps, each level cropped to its input."""
    d = dlo
    for dh, n in zip(dhis[::-1], lens[::-1]):
        d = wo.sfb1d(d, dh, h0, h1, mode, axis=-1)[..., :n]
    return d


def rec_close(a, ref, dtype, what):
    err, bound = float(np.abs(npy(a) - ref).max()), REC_ALL[dtype] * max(1.0, float(np.abs(ref).max()))
    print('%s: max err %.3e, bound %.3e' % (what, err, bound))
    assert tuple(a.shape) == ref.shape and a.dtype == dtype and err <= bound, (what, err, bound)


def check_instantiation(dev, wave, dtype):
    L = ntaps(wave)
    h0, h1 = filters.dwt_analysis_taps(wave)
    g0, g1 = filters.dwt_synthesis_taps(wave)
    A, S = ('Wl%s1dFused<%s, %d>' % (k, TNAME[dtype], L) for k in ('Dwt', 'Idwt'))
    for mode, J, N, na, ns in CASES:
        rng = np.random.RandomState(31 + J)
        what = '%s %s J=%d %s' % (wave, mode, J, TNAME[dtype])
        x = dev_t(rng.randn(1, ROWS, N), dtype, dev).requires_grad_(True)
        xfm = pw.DWT1DForward(J=J, wave=wave, mode=mode).to(dev).to(dtype)
        ifm = pw.DWT1DInverse(wave=wave, mode=mode).to(dev).to(dtype)
        c0 = pw.launch_count()
        yl, yh = xfm(x)
        ks, g = pw.kernels_since(c0), last_grid()
        assert ks == [A] and g == ROWS * na, (what, ks, g)
        oyl, oyh = wo.dwt1d_forward(npy(x), J, h0, h1, mode)
        close(yl, oyl, dtype, 'yl ' + what)
        for j in range(J):
            close(yh[j], oyh[j], dtype, 'yh[%d] %s' % (j, what))
            assert yh[j].is_contiguous()
        # ---- the reconstruction from the engine's own coefficients
        c0 = pw.launch_count()
        rec = ifm((yl.detach(), [h.detach() for h in yh]))
        ks, g = pw.kernels_since(c0), last_grid()
        if ns:
            assert ks == [S] and g == ROWS * ns, (what, ks, g)
        else:
            assert len(ks) == J and not any('Idwt1dFused' in k for k in ks), (what, ks)
        rec_close(rec, wo.dwt1d_inverse(npy(yl), [npy(h) for h in yh], g0, g1, mode), dtype, 'rec ' + what)
        # ---- dx: the synthesis chain with the analysis taps, cropped
        cots = [dev_t(rng.randn(*t.shape), dtype, dev) for t in [yl] + list(yh)]
        c0 = pw.launch_count()
        dx, = torch.autograd.grad([yl] + list(yh), x, cots)
        ks, g = pw.kernels_since(c0), last_grid()
        if ns:
            assert ks == [S] and g == ROWS * ns, (what, ks, g)
        else:
            assert len(ks) == J and not any('Idwt1dFused' in k for k in ks), (what, ks)
        lens = [N] + [h.shape[-1] for h in oyh[:-1]]
        close(dx, grad_ref(npy(cots[0]), [npy(c) for c in cots[1:]], lens, h0, h1, mode), dtype, 'dx ' + what)
