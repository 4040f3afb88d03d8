"""WPT1DForward / WPT1DInverse: the 1-D wavelet packet transform - the full tree, in which every sub-band is split again, not
only the low-pass - of (N, C, n) signals on the gfx950 engine.  The reference has no packet transform; constructor, buffers,
modes and the gradient rule are those of its 1-D DWT modules.  In periodization mode up to three levels are ONE launch of a
barrier-free wave-tile kernel (csrc/wl_wpt1d.h) that writes the bands of every row side by side, so the next launch reads them
as 2**3 times as many rows without a copy."""
import torch.nn as nn

from .. import ops
from . import lowlevel
from .transform1d import _resolve_pair


def wpt1d_freq_order(J):
    """The band indices of a J-level packet tree in frequency order: a list ``idx`` of length 2**J such that ``y[:, :, idx[f]]``
    is the band at frequency slot f, 0 = lowest.  (Downsampling a highpass band mirrors its spectrum, so along a path the natural
    index of slot f is its Gray code f ^ (f >> 1), bit by bit: the 1-D case of wpt2d_freq_order.)"""
    return [f ^ (f >> 1) for f in range(1 << J)]


def _chunks(J):
    """The levels of a J-level tree in launches of up to ops.WPT1D_MAXJ, finest first."""
    return [ops.WPT1D_MAXJ] * (J // ops.WPT1D_MAXJ) + ([J % ops.WPT1D_MAXJ] if J % ops.WPT1D_MAXJ else [])


def _level_lens(n, J, L, mode):
    """[n_0, ..., n_J]: the band lengths of a forward transform of n samples."""
    lens = [int(n)]
    for _ in range(J):
        lens.append(ops.coeff_len(lens[-1], L, mode))
    return lens


class WPT1DForward(nn.Module):
    """1-D wavelet packet transform.  ``WPT1DForward(J=1, wave='db1', mode='zero')(x) -> y`` takes x (N, C, n) to the dense
    y (N, C, 2**J, n_J) of x's dtype, n_j = ops.coeff_len(n_{j-1}, L, mode); J = 0 returns ``x.unsqueeze(2)``.  ``wave`` and
    ``mode`` as in DWT1DForward.

    Band index (natural / Paley order): b = sum_j s_j 2**(J-j), s_j = 1 where level j took the highpass - level 1 is the most
    significant bit, so ``y.view(N, C, 2, 2**(J-1), n_J)[:, :, s]`` is the whole subtree under band s, for J = 1
    ``y == torch.stack([yl, yh[0]], 2)`` of DWT1DForward, and ``y[:, :, 0]`` is its ``yl`` for every J.
    ``wpt1d_freq_order(J)`` sorts the bands by frequency.

    Buffers h0, h1 exactly as DWT1DForward stores them.  The backward of a level is the packet synthesis with the stored
    analysis taps, cropped to the level's input."""

    def __init__(self, J=1, wave='db1', mode='zero'):
        super().__init__()
        h0, h1 = _resolve_pair(wave, 'dec_lo', 'dec_hi')
        filts = lowlevel.prep_filt_afb1d(h0, h1)
        self.register_buffer('h0', filts[0])
        self.register_buffer('h1', filts[1])
        self.J = J
        self.mode = mode

    def forward(self, x):
        mode = lowlevel.mode_to_int(self.mode)
        if x.dim() != 3:
            raise ValueError('WPT1DForward takes (N, C, n) tensors, not %d-D ones' % x.dim())
        N, C = x.shape[:2]
        if self.J < 1:
            return x.unsqueeze(2)
        y, done = x, 0
        for n in _chunks(self.J):
            # up to three levels per node (one launch where ops.WPT1D_FUSED and the kernels' envelope allow)
            y = lowlevel.AFBWPT1D.apply(y, self.h0, self.h1, mode, n)
            done += n
            y = y.view(N, C << done, y.shape[-1])
        return y.view(N, C, 1 << self.J, y.shape[-1])


class WPT1DInverse(nn.Module):
    """Inverse 1-D wavelet packet transform.  ``WPT1DInverse(wave='db1', mode='zero')(y, size=None) -> x`` takes what
    WPT1DForward returns; J is read from ``y.shape[2]`` (a power of 2, else ValueError).  With ``size=n`` every level is cropped
    to the length the forward transform of n samples had there (ValueError if that chain does not end at y's band length), so
    ``WPT1DInverse(..)(WPT1DForward(..)(x), size=x.shape[-1])`` has x's shape; without it every level returns its natural
    length, 2K - L + 2 (periodization: 2K).  Buffers g0, g1 as in DWT1DInverse.  The backward of a level is the packet analysis
    with the stored synthesis taps."""

    def __init__(self, wave='db1', mode='zero'):
        super().__init__()
        g0, g1 = _resolve_pair(wave, 'rec_lo', 'rec_hi')
        filts = lowlevel.prep_filt_sfb1d(g0, g1)
        self.register_buffer('g0', filts[0])
        self.register_buffer('g1', filts[1])
        self.mode = mode

    def forward(self, y, size=None):
        mode = lowlevel.mode_to_int(self.mode)
        if y.dim() != 4:
            raise ValueError('WPT1DInverse takes (N, C, 2**J, n) tensors, not %d-D ones' % y.dim())
        N, C, B = y.shape[:3]
        J = B.bit_length() - 1
        if B < 1 or 1 << J != B:
            raise ValueError('%d bands are no power of 2' % B)
        lens = None
        if size is not None:
            lens = _level_lens(size, J, self.g0.numel(), mode)
            if lens[-1] != y.shape[-1]:
                raise ValueError('a %d-level transform of %d samples has %d coefficients per band, not %d'
                                 % (J, lens[0], lens[-1], y.shape[-1]))
        j = J
        for n in _chunks(J)[::-1]:                      # the forward's nodes in reverse: the short one first
            y = y.reshape(N, C << (j - n), 1 << n, y.shape[-1])
            y = lowlevel.SFBWPT1D.apply(y, self.g0, self.g1, mode, None if lens is None else lens[j - n], n)
            j -= n
        return y.reshape(N, C, y.shape[-1])
