"""SWT1DShrink: translation-invariant wavelet shrinkage of (N, C, L) signals - SWT1DForward, a threshold on every highpass,
SWT1DInverse - with thresholds that can be learned, and swt1d_universal_thresh, the classical estimate of them.  Up to three
levels run in one launch per direction of the wave-tile kernels (csrc/wl_shrink1d.h): the coefficients never leave registers
and nothing but x and the thresholds is kept for the backward."""
import math

import torch
import torch.nn as nn

from . import lowlevel
from .. import filters
from .swt1d import SWT1DForward, _register_taps, _taps_form


def _resolve_bank(wave):
    """(dec_lo, dec_hi, rec_lo, rec_hi) of a name, a wavelet object, four arrays, or two: the analysis pair of an orthonormal
    bank, whose synthesis pair is its reversal."""
    if isinstance(wave, str):
        wave = filters.Wavelet(wave)
    if filters.is_wavelet_like(wave):
        return wave.dec_lo, wave.dec_hi, wave.rec_lo, wave.rec_hi
    assert len(wave) in (2, 4)
    if len(wave) == 2:
        return wave[0], wave[1], list(wave[0])[::-1], list(wave[1])[::-1]
    return tuple(wave)


class SWT1DShrink(nn.Module):
    """``SWT1DShrink(J=1, wave='db1', thresh=0.0, kind='soft', learn=False)(x:(N,C,L), thresh=None) -> y:(N,C,L)``:
    ``SWT1DInverse(wave)((yl, [shrink(yh_j, t_j)]))`` of ``SWT1DForward(J, wave, 'periodic')(x)`` with soft
    ``sign(w) max(|w| - t, 0)`` or hard ``w [|w| > t]`` shrinkage.  `thresh` is 0-d, (J,) or 3-d with every dimension 1 or that
    of (J, N, C); it is an ``nn.Parameter`` with `learn`, a buffer otherwise, and an argument of the call overrides it.  It is used
    as given: nothing clamps a learned threshold that turns negative.  The gradient reaches x and the thresholds (hard: zeros).
    'periodic' and even tap counts only (ValueError otherwise, as SWT1DInverse); J = 0 returns x.  With `learn_filters` the four
    taps are ``nn.Parameter``s under the buffers' names and the gradient reaches them too: the call then runs SWT1DForward,
    element-wise shrinkage and SWT1DInverse, whose nodes have the tap gradients (the one-launch kernels have none)."""

    def __init__(self, J=1, wave='db1', thresh=0.0, kind='soft', learn=False, mode='periodic', learn_filters=False):
        super().__init__()
        if kind not in ('soft', 'hard'):
            raise ValueError("kind must be 'soft' or 'hard', not {!r}".format(kind))
        h0, h1, g0, g1 = _resolve_bank(wave)
        ana, syn = lowlevel.prep_filt_afb1d(h0, h1), lowlevel.prep_filt_sfb1d(g0, g1)
        _register_taps(self, ('h0', 'h1', 'g0', 'g1'), tuple(ana[:2]) + tuple(syn[:2]), learn_filters)
        t = torch.as_tensor(thresh, dtype=torch.float32).clone()
        if learn:
            self.thresh = nn.Parameter(t)
        else:
            self.register_buffer('thresh', t)
        self.J = J
        self.kind = kind
        self.mode = mode

    def forward(self, x, thresh=None):
        return lowlevel.swt1d_shrink(x, self.h0, self.h1, self.g0, self.g1, self.thresh if thresh is None else thresh, self.J,
                                     self.kind, self.mode)

    def extra_repr(self):
        return "J={}, kind='{}', learn={}, taps={}".format(self.J, self.kind, isinstance(self.thresh, nn.Parameter), _taps_form(self.h0))


def swt1d_universal_thresh(x, wave='db1', J=1):
    """The universal threshold of x (N, C, L) for SWT1DShrink, (J, N, C): ``sigma sqrt(2 ln L)`` with the noise level estimated
    from the finest band of one ``SWT1DForward(J=1)``, ``sigma = median(|yh_1|, -1) / 0.6745``.  The same value serves every
    level: the stationary transform's levels use the taps at scale 1 - they are not renormalised as the bands widen -, and
    an orthonormal bank at scale 1 keeps the variance of white noise at every undecimated level (each level's filter has
    unit energy).  For a biorthogonal bank this holds only approximately."""
    xfm = SWT1DForward(J=1, wave=wave, mode='periodic').to(x.device)
    with torch.no_grad():
        hi = xfm(x)[1][0]
        sigma = hi.abs().float().median(-1).values / 0.6745
        t = sigma * math.sqrt(2.0 * math.log(x.shape[-1]))
    return t.unsqueeze(0).expand(J, -1, -1).contiguous()
