"""WPT2DForward / WPT2DInverse: the 2-D wavelet packet transform - the full tree, in which every sub-band is split again, not
only the low-pass - on the gfx950 engine.  The reference has no packet transform; constructor, buffers, modes and the gradient
rule are those of its 2-D DWT modules.  A level is ONE launch of a packed-band kernel (csrc/wl_wpt2d.h) that writes the four
bands of every plane side by side, so the next level reads them as four times as many planes without a copy."""
import torch.nn as nn

from .. import ops
from . import lowlevel
from .transform2d import _resolve_bank


def wpt2d_freq_order(J):
    """The band indices of a J-level packet tree in frequency order: a list ``idx`` of length 4**J such that
    ``y[:, :, idx].view(N, C, 2**J, 2**J, H_J, W_J)[:, :, fh, fw]`` is the band at frequency slot (fh, fw), 0 = lowest.
    (Downsampling a highpass band mirrors its spectrum, so along a path the natural index of slot f is its Gray code
    f ^ (f >> 1), per axis and bit by bit.)"""
    n = 1 << J
    idx = []
    for fh in range(n):
        gh = fh ^ (fh >> 1)
        for fw in range(n):
            gw = fw ^ (fw >> 1)
            b = 0
            for j in range(J - 1, -1, -1):          # level 1 = the most significant bit of the Gray code and digit of b
                b = 4 * b + 2 * ((gw >> j) & 1) + ((gh >> j) & 1)
            idx.append(b)
    return idx


def _level_sizes(size, J, Lh, Lw, mode):
    """[(H_0, W_0), ..., (H_J, W_J)]: the plane sizes of a forward transform of a (H_0, W_0) image."""
    sizes = [(int(size[0]), int(size[1]))]
    for _ in range(J):
        h, w = sizes[-1]
        sizes.append((ops.coeff_len(h, Lh, mode), ops.coeff_len(w, Lw, mode)))
    return sizes


class WPT2DForward(nn.Module):
    """2-D wavelet packet transform.  ``WPT2DForward(J=1, wave='db1', mode='zero')(x) -> y`` takes x (N, C, H, W) to the dense
    y (N, C, 4**J, H_J, W_J) of x's dtype, H_j = ops.coeff_len(H_{j-1}, L, mode); J = 0 returns ``x.unsqueeze(2)``.  ``wave`` and
    ``mode`` as in DWTForward.

    Band index (natural / Paley order): b = sum_j s_j 4**(J-j), s_j = 2 b_W + b_H the sub-band taken at level j (0 = ll,
    1 = W-lo/H-hi, 2 = W-hi/H-lo, 3 = hh: DWTForward's order) - level 1 is the most significant digit, so
    ``y.view(N, C, 4, 4**(J-1), H_J, W_J)[:, :, s]`` is the whole subtree under band s, and for J = 1
    ``y == torch.cat([yl[:, :, None], yh[0]], 2)`` of DWTForward.  ``wpt2d_freq_order(J)`` sorts the bands by frequency.

    Buffers h0_col, h1_col, h0_row, h1_row exactly as DWTForward stores them and hands them on (its quirk Q1 included).  The
    backward of a level is the packet synthesis with the stored analysis taps, cropped to the level's input."""

    def __init__(self, J=1, wave='db1', mode='zero'):
        super().__init__()
        h0_col, h1_col, h0_row, h1_row = _resolve_bank(wave, 'dec_lo', 'dec_hi')
        filts = lowlevel.prep_filt_afb2d(h0_col, h1_col, h0_row, h1_row)
        for name, f in zip(('h0_col', 'h1_col', 'h0_row', 'h1_row'), filts):
            self.register_buffer(name, f)
        self.J = J
        self.mode = mode

    def forward(self, x):
        mode = lowlevel.mode_to_int(self.mode)
        if x.dim() != 4:
            raise ValueError('WPT2DForward takes (N, C, H, W) tensors, not %d-D ones' % x.dim())
        N, C = x.shape[:2]
        if self.J < 1:
            return x.unsqueeze(2)
        y, left = x, self.J
        while left:
            # two levels per node while two are left (one launch where ops.WPT_FUSED and the kernels' envelope allow), then one
            # (DWTForward's argument order: the module's *col* pair lands in the row slots, quirk Q1)
            n = 2 if left >= 2 else 1
            y = lowlevel.AFBWPT2D.apply(y, self.h0_col, self.h1_col, self.h0_row, self.h1_row, mode, n)
            y = y.view(N, -1, y.shape[-2], y.shape[-1])
            left -= n
        return y.view(N, C, -1, y.shape[-2], y.shape[-1])


class WPT2DInverse(nn.Module):
    """Inverse 2-D wavelet packet transform.  ``WPT2DInverse(wave='db1', mode='zero')(y, size=None) -> x`` takes what
    WPT2DForward returns; J is read from ``y.shape[2]`` (a power of 4, else ValueError).  With ``size=(H, W)`` every level is
    cropped to the size the forward transform of an (H, W) image had there (ValueError if that chain does not end at y's plane
    size), so ``WPT2DInverse(..)(WPT2DForward(..)(x), size=x.shape[-2:])`` has x's shape; without it every level returns its
    natural size, 2K - L + 2 (periodization: 2K).  Buffers g0_col .. g1_row as in DWTInverse.  The backward of a level is the
    packet analysis with the stored synthesis taps."""

    def __init__(self, wave='db1', mode='zero'):
        super().__init__()
        g0_col, g1_col, g0_row, g1_row = _resolve_bank(wave, 'rec_lo', 'rec_hi')
        filts = lowlevel.prep_filt_sfb2d(g0_col, g1_col, g0_row, g1_row)
        for name, f in zip(('g0_col', 'g1_col', 'g0_row', 'g1_row'), filts):
            self.register_buffer(name, f)
        self.mode = mode

    def forward(self, y, size=None):
        mode = lowlevel.mode_to_int(self.mode)
        if y.dim() != 5:
            raise ValueError('WPT2DInverse takes (N, C, 4**J, H, W) tensors, not %d-D ones' % y.dim())
        N, C, B = y.shape[:3]
        J = (B.bit_length() - 1) // 2
        if B < 1 or 4 ** J != B:
            raise ValueError('%d bands are no power of 4' % B)
        sizes = None
        if size is not None:
            # (the module's *col* pair filters along W: quirk Q1)
            sizes = _level_sizes(size, J, self.g0_row.numel(), self.g0_col.numel(), mode)
            if sizes[-1] != tuple(y.shape[-2:]):
                raise ValueError('a %d-level transform of a %d x %d image has %d x %d coefficients per band, not %d x %d'
                                 % ((J,) + sizes[0] + sizes[-1] + tuple(y.shape[-2:])))
        j = J
        while j:                                        # the forward's nodes in reverse: the single level first when J is odd
            n = 1 if j % 2 else 2
            y = y.reshape(N, -1, 4 ** n, y.shape[-2], y.shape[-1])
            y = lowlevel.SFBWPT2D.apply(y, self.g0_col, self.g1_col, self.g0_row, self.g1_row, mode,
                                        None if sizes is None else sizes[j - n], n)
            j -= n
        return y.reshape(N, C, y.shape[-2], y.shape[-1])
