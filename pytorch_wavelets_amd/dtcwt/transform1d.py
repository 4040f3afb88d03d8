"""DTCWT1DForward / DTCWT1DInverse: the dual-tree complex wavelet transform of signals (N, C, L) along their last axis, with
the constructor signature, buffer names and filter-tuple forms of the 2-D modules (dtcwt/transform2d.py) and the same level
structure carried to one axis: level 1 the two odd-length filters at full rate, every further level the q-shift pair of both
trees; ``yh[j]`` (N, C, L_j, 2) holds (real, imaginary) last, finest level first, ``yl`` the 2x oversampled lowpass.  Up to four
levels run as one launch of the fused kernels of csrc/wl_dtcwt1d.h (one autograd node), deeper transforms in groups of four."""
import torch
import torch.nn as nn
from numpy import ndarray

from ..filters import biort as _biort, qshift as _qshift
from .lowlevel import prep_filt
from .transform_funcs import DTCWT1DAnalysis, DTCWT1DSynthesis


def _is_empty(t):
    return t is None or t.shape == torch.Size([])


def _check_mode(mode):
    if mode != 'symmetric':
        raise ValueError("The 1-D DTCWT implements mode 'symmetric' only, got {!r}".format(mode))


class DTCWT1DForward(nn.Module):
    """1-D DTCWT.  ``DTCWT1DForward(biort='near_sym_a', qshift='qshift_a', J=3, skip_hps=False, include_scale=False, ri_dim=-1,
    mode='symmetric')(x: (N, C, L)) -> (yl, yh)``: ``yh[j]`` (N, C, L_j, 2) for the default ri_dim
    (``torch.view_as_complex(yh[j])`` is the analytic band of level j + 1), ``yl`` (N, C, ~L / 2^(J-1)).  An odd L gets a copy of
    its last sample; a level whose length is no multiple of 4 one replicated sample either side.  With include_scale the first
    return value is the list of the levels' lowpass signals."""

    def __init__(self, biort='near_sym_a', qshift='qshift_a', J=3, skip_hps=False, include_scale=False, ri_dim=-1,
                 mode='symmetric'):
        super().__init__()
        _check_mode(mode)
        self.biort, self.qshift, self.J = biort, qshift, J
        self.ri_dim, self.mode = ri_dim, mode
        if isinstance(biort, str):
            h0o, _, h1o, _ = _biort(biort)[:4]
        else:
            h0o, h1o = biort[0], biort[1]
        self.register_buffer('h0o', prep_filt(h0o, 1))
        self.register_buffer('h1o', prep_filt(h1o, 1))
        if isinstance(qshift, str):
            h0a, h0b, _, _, h1a, h1b, _, _ = _qshift(qshift)[:8]
        else:
            h0a, h0b, h1a, h1b = qshift[0], qshift[1], qshift[2], qshift[3]
        self.register_buffer('h0a', prep_filt(h0a, 1))
        self.register_buffer('h0b', prep_filt(h0b, 1))
        self.register_buffer('h1a', prep_filt(h1a, 1))
        self.register_buffer('h1b', prep_filt(h1b, 1))
        self.skip_hps = skip_hps if isinstance(skip_hps, (list, tuple, ndarray)) else [skip_hps, ] * self.J
        self.include_scale = (include_scale if isinstance(include_scale, (list, tuple, ndarray))
                              else [include_scale, ] * self.J)

    def forward(self, x):
        if self.J == 0:
            return x, None
        assert x.ndim == 3, "Can only handle 3d inputs (N, C, L)"
        want_scales = True in self.include_scale
        highs, scales, low = [], [], x
        for first in range(0, self.J, 4):
            skip = tuple(bool(v) for v in self.skip_hps[first:first + 4])
            scale = tuple(bool(v) for v in self.include_scale[first:first + 4])
            n = len(skip)
            outs = DTCWT1DAnalysis.apply(low, self.h0o, self.h1o, self.h0a, self.h0b, self.h1a, self.h1b, first > 0, skip, scale)
            low = outs[0]
            for l in range(n):
                h = outs[1 + l]
                if h is None:
                    h = x.new_zeros([])
                else:
                    h = h.reshape(tuple(h.shape[:-1]) + (h.shape[-1] // 2, 2))
                    if self.ri_dim % 4 != 3:
                        h = h.movedim(-1, self.ri_dim)
                highs.append(h)
                s = low if l == n - 1 else outs[1 + n + l]
                scales.append(s if scale[l] else x.new_zeros([]))
        if want_scales:
            return scales, highs
        return low, highs


class DTCWT1DInverse(nn.Module):
    """1-D inverse DTCWT.  ``DTCWT1DInverse(biort, qshift, ri_dim=-1, mode='symmetric')((yl, yh)) -> x`` of the even length
    2 L_0 (a caller whose input was odd drops the last sample); entries of ``yh`` may be None / 0-dim tensors (zeros)."""

    def __init__(self, biort='near_sym_a', qshift='qshift_a', ri_dim=-1, mode='symmetric'):
        super().__init__()
        _check_mode(mode)
        self.biort, self.qshift = biort, qshift
        self.ri_dim, self.mode = ri_dim, mode
        if isinstance(biort, str):
            _, g0o, _, g1o = _biort(biort)[:4]
        else:
            g0o, g1o = biort[0], biort[1]
        self.register_buffer('g0o', prep_filt(g0o, 1))
        self.register_buffer('g1o', prep_filt(g1o, 1))
        if isinstance(qshift, str):
            _, _, g0a, g0b, _, _, g1a, g1b = _qshift(qshift)[:8]
        else:
            g0a, g0b, g1a, g1b = qshift[0], qshift[1], qshift[2], qshift[3]
        self.register_buffer('g0a', prep_filt(g0a, 1))
        self.register_buffer('g0b', prep_filt(g0b, 1))
        self.register_buffer('g1a', prep_filt(g1a, 1))
        self.register_buffer('g1b', prep_filt(g1b, 1))

    def forward(self, coeffs):
        low, highs = coeffs
        assert low.ndim == 3, "Can only handle 3d inputs (N, C, L)"
        J = len(highs)
        flat = []
        for s in highs:
            if _is_empty(s):
                flat.append(None)
                continue
            assert len(s.shape) == 4, "Bandpass inputs must have 4 dimensions"
            assert s.shape[self.ri_dim] == 2, \
                "Inputs must be complex with real and imaginary parts in the ri dimension"
            s = s if self.ri_dim % 4 == 3 else s.movedim(self.ri_dim, -1)
            s = s.contiguous()
            flat.append(s.reshape(tuple(s.shape[:-2]) + (2 * s.shape[-2],)))
        # samples of every level's inputs: a band's own length, or what the next coarser level makes (the lowpass for the coarsest)
        ns = [None] * J
        for j in range(J - 1, -1, -1):
            ns[j] = flat[j].shape[-1] if flat[j] is not None else (low.shape[-1] if j == J - 1 else 2 * ns[j + 1])
        last = ((J - 1) // 4) * 4
        for first in range(last, -1, -4):
            grp = flat[first:first + 4]
            low = DTCWT1DSynthesis.apply(low, self.g0o, self.g1o, self.g0a, self.g0b, self.g1a, self.g1b, first > 0,
                                         tuple(ns[first:first + 4]), *grp)
        return low
