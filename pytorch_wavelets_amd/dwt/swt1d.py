"""SWT1DForward / SWT1DInverse: the 1-D stationary (undecimated, a-trous) wavelet transform of (N, C, L) signals and its
inverse - the ``swt / iswt`` of the wavelet libraries, with DWT1DForward's constructor signature, buffer names and (yl, yh)
layout.  Level j is ``lowlevel.afb1d_atrous`` with dilation 2**(j-1) on the previous lowpass; in 'periodic' mode the first three
levels run in one launch of the wave-tile kernels (csrc/wl_swt1d.h), in either direction and in both backward passes.  With
``learn=True`` the filter taps are parameters: their gradient is one more launch (csrc/wl_swt1d_tapgrad.h)."""
import torch.nn as nn

from . import lowlevel
from .transform1d import _resolve_pair


def _register_taps(module, names, taps, learn):
    """The taps as parameters (`learn`) or buffers: the same names and ``state_dict`` keys either way, so the two forms load each
    other's state."""
    for name, t in zip(names, taps):
        if learn:
            setattr(module, name, nn.Parameter(t.clone()))
        else:
            module.register_buffer(name, t)


def _taps_form(t):
    return 'parameters' if isinstance(t, nn.Parameter) else 'buffers'


class SWT1DForward(nn.Module):
    """``SWT1DForward(J=1, wave='db1', mode='periodic')(x:(N,C,L)) -> (yl, [yh_1 .. yh_J])``, finest scale first, every tensor
    (N, C, L).  `mode` is one of afb1d_atrous's six pad modes; only 'periodic' has an inverse.  With `learn` the taps h0 / h1 are
    ``nn.Parameter``s under the buffers' names ('periodic' and even tap counts only: ValueError otherwise), buffers without."""

    def __init__(self, J=1, wave='db1', mode='periodic', learn=False):
        super().__init__()
        h0, h1 = _resolve_pair(wave, 'dec_lo', 'dec_hi')
        filts = lowlevel.prep_filt_afb1d(h0, h1)
        _register_taps(self, ('h0', 'h1'), filts, learn)
        self.J = J
        self.mode = mode

    def forward(self, x):
        return lowlevel.swt1d(x, self.h0, self.h1, self.mode, self.J)

    def extra_repr(self):
        return "J={}, mode='{}', taps={}".format(self.J, self.mode, _taps_form(self.h0))


class SWT1DInverse(nn.Module):
    """``SWT1DInverse(wave='db1', mode='periodic')((yl, yh)) -> x``: per level, coarsest first,
    lo_{j-1} = 1/2 (A_0(g)^T lo_j + A_1(g)^T hi_j) with the synthesis taps g; ``None`` entries of ``yh`` are zeros, an empty
    ``yh`` returns ``yl``.  'periodic' and even tap counts only (ValueError otherwise).  With `learn` the taps g0 / g1 are
    ``nn.Parameter``s under the buffers' names, buffers without."""

    def __init__(self, wave='db1', mode='periodic', learn=False):
        super().__init__()
        g0, g1 = _resolve_pair(wave, 'rec_lo', 'rec_hi')
        filts = lowlevel.prep_filt_sfb1d(g0, g1)
        _register_taps(self, ('g0', 'g1'), filts, learn)
        self.mode = mode

    def forward(self, coeffs):
        yl, yh = coeffs
        return lowlevel.iswt1d(yl, yh, self.g0, self.g1, self.mode)

    def extra_repr(self):
        return "mode='{}', taps={}".format(self.mode, _taps_form(self.g0))
