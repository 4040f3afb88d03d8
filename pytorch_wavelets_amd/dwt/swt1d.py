"""SWT1DForward / SWT1DInverse: the 1-D stationary (undecimated, a-trous) wavelet transform of (N, C, L) signals and its
inverse - the ``swt / iswt`` of the wavelet libraries, with DWT1DForward's constructor signature, buffer names and (yl, yh)
layout.  Level j is ``lowlevel.afb1d_atrous`` with dilation 2**(j-1) on the previous lowpass; in 'periodic' mode the first three
levels run in one launch of the wave-tile kernels (csrc/wl_swt1d.h), in either direction and in both backward passes."""
import torch.nn as nn

from . import lowlevel
from .transform1d import _resolve_pair


class SWT1DForward(nn.Module):
    """``SWT1DForward(J=1, wave='db1', mode='periodic')(x:(N,C,L)) -> (yl, [yh_1 .. yh_J])``, finest scale first, every tensor
    (N, C, L).  `mode` is one of afb1d_atrous's six pad modes; only 'periodic' has an inverse."""

    def __init__(self, J=1, wave='db1', mode='periodic'):
        super().__init__()
        h0, h1 = _resolve_pair(wave, 'dec_lo', 'dec_hi')
        filts = lowlevel.prep_filt_afb1d(h0, h1)
        self.register_buffer('h0', filts[0])
        self.register_buffer('h1', filts[1])
        self.J = J
        self.mode = mode

    def forward(self, x):
        return lowlevel.swt1d(x, self.h0, self.h1, self.mode, self.J)


class SWT1DInverse(nn.Module):
    """``SWT1DInverse(wave='db1', mode='periodic')((yl, yh)) -> x``: per level, coarsest first,
    lo_{j-1} = 1/2 (A_0(g)^T lo_j + A_1(g)^T hi_j) with the synthesis taps g; ``None`` entries of ``yh`` are zeros, an empty
    ``yh`` returns ``yl``.  'periodic' and even tap counts only (ValueError otherwise)."""

    def __init__(self, wave='db1', mode='periodic'):
        super().__init__()
        g0, g1 = _resolve_pair(wave, 'rec_lo', 'rec_hi')
        filts = lowlevel.prep_filt_sfb1d(g0, g1)
        self.register_buffer('g0', filts[0])
        self.register_buffer('g1', filts[1])
        self.mode = mode

    def forward(self, coeffs):
        yl, yh = coeffs
        return lowlevel.iswt1d(yl, yh, self.g0, self.g1, self.mode)
