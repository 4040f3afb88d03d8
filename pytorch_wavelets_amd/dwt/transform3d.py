"""DWT3DForward / DWT3DInverse: the separable 3-D DWT of (N, C, D, H, W) volumes (CT / MRI, video clips) on the gfx950 engine.
The reference has no 3-D transform; the conventions are those of its 2-D modules (constructor, buffers, (yl, yh), modes,
quirks) carried to a third axis.  Every level is the 2-D engine on the N*C*D planes - the reshape is free - followed by ONE
launch of the streaming depth kernel (csrc/wl_dwt3d.h), which writes the final layout."""
import torch.nn as nn

from .. import filters
from .. import ops
from . import lowlevel
from .transform2d import _qmf_banks, _same_banks


def _resolve_bank3(wave, lo_attr, hi_attr):
    """str | Wavelet-like | (f0, f1) | (f0_dep, f1_dep, f0_col, f1_col, f0_row, f1_row) -> six tap vectors."""
    if isinstance(wave, str):
        wave = filters.Wavelet(wave)
    if filters.is_wavelet_like(wave):
        wave = (getattr(wave, lo_attr), getattr(wave, hi_attr))
    if len(wave) == 2:
        return (wave[0], wave[1]) * 3
    if len(wave) == 6:
        return tuple(wave)
    raise ValueError("wave must be a name, a Wavelet, or a tuple of 2 or 6 filters")


class DWT3DForward(nn.Module):
    """3-D multi-level DWT.  ``DWT3DForward(J=1, wave='db1', mode='zero')(x) -> (yl, yh)`` for x (N, C, D, H, W):
    yl (N, C, D_J, H_J, W_J) and yh[j] (N, C, 7, D_j, H_j, W_j), finest scale first; per axis the lengths of the 2-D transform
    (``ops.coeff_len``).  The modes are DWTForward's: zero, symmetric, reflect, periodization, periodic.

    Sub-band s = 4 b_D + 2 b_W + b_H (b = 1: highpass along that axis): s = 0 is yl, band s sits at ``yh[j][:, :, s - 1]`` - so
    bands 1..3 are DWTForward's (lh, hl, hh) of the depth-lowpass, bands 4..7 (ll, lh, hl, hh) of the depth-highpass.  As pywt's
    ``dwtn`` keys over the axes (D, H, W):

        s     1    2    3    4    5    6    7
        key  ada  aad  add  daa  dda  dad  ddd

    ``wave``: a name, a Wavelet-like object, (lo, hi) or (h0_dep, h1_dep, h0_col, h1_col, h0_row, h1_row).  Buffers: h0_dep,
    h1_dep (1, 1, L, 1, 1), stored reversed like the others; h0_col .. h1_row exactly as DWTForward stores them and hands them on
    (its quirk Q1 included: the module's *col* pair filters along W).  The backward of a level is the synthesis with the
    stored analysis taps, cropped - the reference's rule for its 2-D transform, on all three axes."""

    def __init__(self, J=1, wave='db1', mode='zero'):
        super().__init__()
        h0_dep, h1_dep, h0_col, h1_col, h0_row, h1_row = _resolve_bank3(wave, 'dec_lo', 'dec_hi')
        filts = lowlevel.prep_filt_afb3d(h0_dep, h1_dep, h0_col, h1_col, h0_row, h1_row)
        for name, f in zip(('h0_dep', 'h1_dep', 'h0_col', 'h1_col', 'h0_row', 'h1_row'), filts):
            self.register_buffer(name, f)
        self.J = J
        self.mode = mode
        self._qmf = ops.TapVerdict(_qmf_banks)      # the 2-D stage's kernel-variant hints, as DWTForward keeps them
        self._same = ops.TapVerdict(_same_banks)

    def forward(self, x):
        mode = lowlevel.mode_to_int(self.mode)
        if x.dim() != 5:
            raise ValueError('DWT3DForward takes (N, C, D, H, W) tensors, not %d-D ones' % x.dim())
        if self.J < 1:
            return x, []
        banks = (self.h0_col, self.h1_col, self.h0_row, self.h1_row)    # (DWTForward's argument order: quirk Q1)
        yh, ll = [], x
        with ops.qmf_hint(self._qmf(*banks)), ops.same_banks_hint(self._same(*banks)):
            for _ in range(self.J):
                ll, high = lowlevel._afb3d_level(ll, (self.h0_dep, self.h1_dep), banks, mode)
                yh.append(high)
        return ll, yh


class DWT3DInverse(nn.Module):
    """3-D multi-level inverse DWT.  ``DWT3DInverse(wave='db1', mode='zero')((yl, yh)) -> x`` takes what DWT3DForward returns;
    ``None`` entries of ``yh`` are zeros.  Coarsest level first; a low-pass one sample longer than the next highs along an axis
    loses that sample, and the output is even-sized per axis (an odd input axis comes back one sample longer), as in
    DWTInverse.  Buffers: g0_dep, g1_dep (1, 1, L, 1, 1) and the four of DWTInverse."""

    def __init__(self, wave='db1', mode='zero'):
        super().__init__()
        g0_dep, g1_dep, g0_col, g1_col, g0_row, g1_row = _resolve_bank3(wave, 'rec_lo', 'rec_hi')
        filts = lowlevel.prep_filt_sfb3d(g0_dep, g1_dep, g0_col, g1_col, g0_row, g1_row)
        for name, f in zip(('g0_dep', 'g1_dep', 'g0_col', 'g1_col', 'g0_row', 'g1_row'), filts):
            self.register_buffer(name, f)
        self.mode = mode
        self._qmf = ops.TapVerdict(_qmf_banks)
        self._same = ops.TapVerdict(_same_banks)

    def forward(self, coeffs):
        yl, yh = coeffs
        mode = lowlevel.mode_to_int(self.mode)
        if yl.dim() != 5:
            raise ValueError('DWT3DInverse takes (N, C, D, H, W) tensors, not %d-D ones' % yl.dim())
        banks = (self.g0_col, self.g1_col, self.g0_row, self.g1_row)
        ll = yl
        with ops.qmf_hint(self._qmf(*banks)), ops.same_banks_hint(self._same(*banks)):
            for h in yh[::-1]:
                ll = lowlevel._sfb3d_level(ll, h, (self.g0_dep, self.g1_dep), banks, mode)
        return ll
