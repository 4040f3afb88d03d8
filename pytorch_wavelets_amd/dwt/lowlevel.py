"""Per-scale DWT operators (layer L2 of SURVEY.md): the autograd Functions the reference exposes in
``pytorch_wavelets/dwt/lowlevel.py``, with the same names, argument order, mode codes and error
text - but each forward/backward is ONE fused gfx950 kernel launch through the C ABI instead of
a chain of ATen gathers / grouped convs / copies.
"""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops

_MODE_TO_INT = {'zero': 0, 'symmetric': 1, 'per': 2, 'periodization': 2, 'constant': 3, 'reflect': 4,
                'replicate': 5, 'periodic': 6}
_INT_TO_MODE = {0: 'zero', 1: 'symmetric', 2: 'periodization', 3: 'constant', 4: 'reflect',
                5: 'replicate', 6: 'periodic'}
FUSED_LEVELS = True   # set False to force one launch per level (A/B measurements)
WIDE_ONE_LEVEL = 640  # coefficient-row pairs: a synthesis level left on its own whose output is at least this wide goes to the one-level strip kernel (_synthesis_ladder)
_FILTERBANK_MODES = (0, 1, 2, 4, 6)   # the ones afb1d/sfb1d accept upstream (dwt/lowlevel.py:134-170)


def mode_to_int(mode):
    """Reference dwt/lowlevel.py:274-290."""
    try:
        return _MODE_TO_INT[mode]
    except (KeyError, TypeError):
        raise ValueError("Unkown pad type: {}".format(mode))


def int_to_mode(mode):
    """Reference dwt/lowlevel.py:293-309."""
    try:
        return _INT_TO_MODE[mode]
    except (KeyError, TypeError):
        raise ValueError("Unkown pad type: {}".format(mode))


def _check_bank_mode(mode):
    if mode not in _FILTERBANK_MODES:
        raise ValueError("Unkown pad type: {}".format(int_to_mode(mode)))


class AFB2D(Function):
    """One level of 2-D analysis.  ``AFB2D.apply(x, h0_row, h1_row, h0_col, h1_col, mode_int)
    -> (low (N,C,H',W'), highs (N,C,3,H',W'))``; the *row* pair filters along W, the *col* pair
    along H (reference dwt/lowlevel.py:336-347).  Backward = synthesis with the same stored taps,
    cropped to the input size (reference :350-365, quirk Q9 reproduced)."""

    @staticmethod
    def forward(ctx, x, h0_row, h1_row, h0_col, h1_col, mode):
        _check_bank_mode(mode)
        ctx.save_for_backward(h0_row, h1_row, h0_col, h1_col)
        ctx.shape = x.shape[-2:]
        ctx.mode = mode
        return ops.afb2d_best(x, h0_row, h1_row, h0_col, h1_col, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, low, highs):
        dx = None
        if ctx.needs_input_grad[0]:
            h0_row, h1_row, h0_col, h1_col = ctx.saved_tensors
            dx = ops.sfb2d_best(low, highs, h0_row, h1_row, h0_col, h1_col, ctx.mode,
                           out_hw=tuple(ctx.shape))
        return dx, None, None, None, None, None


class SFB2D(Function):
    """One level of 2-D synthesis.  ``SFB2D.apply(low, highs, g0_row, g1_row, g0_col, g1_col,
    mode_int) -> y`` (reference dwt/lowlevel.py:671-680).  Backward = analysis with the stored
    synthesis taps (reference :683-694)."""

    @staticmethod
    def forward(ctx, low, highs, g0_row, g1_row, g0_col, g1_col, mode):
        _check_bank_mode(mode)
        ctx.mode = mode
        ctx.save_for_backward(g0_row, g1_row, g0_col, g1_col)
        ctx.has_highs = highs is not None
        return ops.sfb2d_best(low, highs, g0_row, g1_row, g0_col, g1_col, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dlow, dhigh = None, None
        if ctx.needs_input_grad[0] or (ctx.has_highs and ctx.needs_input_grad[1]):
            g0_row, g1_row, g0_col, g1_col = ctx.saved_tensors
            dlow, dhigh = ops.afb2d_best(dy, g0_row, g1_row, g0_col, g1_col, ctx.mode)
            if not ctx.has_highs:
                dhigh = None
        return dlow, dhigh, None, None, None, None, None


def _synthesis_ladder(ll, highs, banks, mode, out_hws=None):
    """All synthesis levels in as few launches as the engine takes: ll = the coarsest low-pass, highs finest first (``None`` =
    zeros), banks = (g0_row, g1_row, g0_col, g1_col) as the ops calls take them -> (x, ll_shapes), ll_shapes[j] = the size of
    the low-pass handed to level j before its 'unpad'.  The inverse transform (SFB2DMulti.forward) and the backward of the
    analysis (AFB2DMulti._backward, with the analysis taps) both run it: there out_hws[j] is the input size of level j, to which
    its output is cropped - by the kernel on the one-level paths, as a view after a multi-level launch -, while the inverse
    leaves a surplus row / column to the next level's 'unpad'."""
    J, L = len(highs), banks[0].numel()
    ll_shapes = [None] * J
    j = J - 1
    while j >= 0:
        n = 0                       # levels j, j-1, .. that one launch can take together: a missing level ends the group
        while n < 4 and j - n >= 0 and highs[j - n] is not None:
            n += 1
        # small planes (CNN feature maps): several planes per workgroup, up to four levels in LDS
        res = ops.sfb2d_small(ll, list(highs[j - n + 1:j + 1]), *banks, mode) if FUSED_LEVELS and n else None
        if res is None and n:
            # More levels than one streaming launch takes (three): the COARSEST (j mod 3) + 1 go first, so that the finest -
            # nearly all of the bytes - go three to a launch (J = 4 as 3 + 1 from the coarse end ran its finest level
            # alone: 0.288 ms against 0.188 for J = 3 at 128 x 3 x 512 x 512); the coarse remainder are small planes.
            m = min(n, 3, (j % 3) + 1 if j + 1 > 3 else 3)
            if FUSED_LEVELS and m < n:
                res = ops.sfb2d_small(ll, list(highs[j - m + 1:j + 1]), *banks, mode)
            n = m
        while FUSED_LEVELS and n >= 1 and res is None:
            if n == 1 and 2 * highs[j].shape[-1] >= WIDE_ONE_LEVEL:
                # a single WIDE level: the one-level strip kernel is ahead of the fused kernel's one-level form (same-box, float32,
                # tools/gpu_r5u.py: 64x3x1024^2 0.333 -> 0.309 ms, 128x3x768^2 0.362 -> 0.342, 128x3x640^2 0.244 -> 0.228);
                # when it declines (few planes, a width that is no multiple of four) the fused kernel is asked as before
                # (the reference's 'unpad' drops exactly ONE surplus row / column, dwt/transform2d.py:141-146: a low-pass that is
                # larger than that is malformed and takes the per-level path below, which raises like every other path)
                h = highs[j]
                dh, dw = ll.shape[-2] - h.shape[-2], ll.shape[-1] - h.shape[-1]
                if 0 <= dh <= 1 and 0 <= dw <= 1:
                    res = ops.sfb2d_stream(ll[..., :h.shape[-2], :h.shape[-1]], h, *banks, mode,
                                           out_hw=None if out_hws is None else out_hws[j], force=ops.STREAM_FORCE)
            if res is None:
                res = ops.sfb2d_fused(ll, list(highs[j - n + 1:j + 1]), *banks, mode)
            if res is None:
                n -= 1
        if res is not None:
            sh = tuple(ll.shape[-2:])
            for i in range(j, j - n, -1):
                ll_shapes[i] = sh
                sh = tuple(ops.synth_len(k, L, mode) for k in highs[i].shape[-2:])
            j -= n
            ll = res if out_hws is None else res[..., :out_hws[j + 1][0], :out_hws[j + 1][1]]
            continue
        h = highs[j]
        ll_shapes[j] = tuple(ll.shape[-2:])
        if h is not None:
            if ll.shape[-2] > h.shape[-2]:
                ll = ll[..., :-1, :]
            if ll.shape[-1] > h.shape[-1]:
                ll = ll[..., :-1]
        ll = ops.sfb2d_best(ll, h, *banks, mode, out_hw=None if out_hws is None else out_hws[j])
        j -= 1
    return ll, ll_shapes


class SFB2DMulti(Function):
    """All synthesis levels as ONE autograd node: ``SFB2DMulti.apply(yl, g0_row, g1_row, g0_col, g1_col, mode_int,
    *yh) -> x`` with yh finest first, ``None`` entries = zeros (the level loop of DWTInverse.forward, reference
    dwt/transform2d.py:131-148, incl. the 'unpad' of a low-pass one row / column larger than the next high-pass).

    Forward: up to three levels at a time in ONE launch of the streaming kernel (wl_dwt2d_synthesis_fused: the
    intermediate low-passes stay in LDS) whenever the engine takes the configuration, otherwise one tile-kernel launch
    per level.  Backward = the chain of SFB2D.backward steps of the reference (analysis with the stored synthesis
    taps, dwt/lowlevel.py:683-694), finest level first; a dropped row / column gets a zero gradient."""

    @staticmethod
    def forward(ctx, yl, g0_row, g1_row, g0_col, g1_col, mode, *yh):
        _check_bank_mode(mode)
        ctx.save_for_backward(g0_row, g1_row, g0_col, g1_col)
        ctx.mode = mode
        ctx.hints = ops.current_hints()     # (the module's kernel-variant hints, re-installed around the backward pass: autograd's thread)
        ctx.has_highs = [h is not None for h in yh]
        x, ctx.ll_shapes = _synthesis_ladder(yl, yh, (g0_row, g1_row, g0_col, g1_col), mode)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        with ops.hints(*ctx.hints):
            return SFB2DMulti._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        J = len(ctx.has_highs)
        grads = [None] * J
        d = None
        if any(ctx.needs_input_grad[:1]) or any(ctx.needs_input_grad[6 + j] for j in range(J)):
            g0_row, g1_row, g0_col, g1_col = ctx.saved_tensors
            d, j, L = dy, 0, g0_row.numel()
            while j < J:
                # Levels whose low-pass the forward handed on WHOLE (no 'unpad' between them: always so in periodization) are a plain
                # multi-level analysis with the synthesis taps: up to three of them in ONE launch of the fused kernel (round 6);
                # a level after which a dropped row / column gets its zero gradient back ends the group.
                n, res = 0, None
                h, w = d.shape[-2:]
                while FUSED_LEVELS and n < 3 and j + n < J and g0_col.numel() == L:
                    h, w = ops.coeff_len(h, L, ctx.mode), ops.coeff_len(w, L, ctx.mode)
                    n += 1
                    if (h, w) != tuple(ctx.ll_shapes[j + n - 1]):
                        break
                while n >= 2 and res is None:
                    res = ops.afb2d_fused(d, g0_row, g1_row, g0_col, g1_col, ctx.mode, n, whole=False)
                    if res is None:
                        n -= 1
                if res is None:
                    n = 1
                    d, dhigh = ops.afb2d_best(d, g0_row, g1_row, g0_col, g1_col, ctx.mode)
                    dhighs = [dhigh]
                else:
                    d, dhighs = res
                for i, dhigh in enumerate(dhighs):
                    if ctx.has_highs[j + i] and ctx.needs_input_grad[6 + j + i]:
                        grads[j + i] = dhigh
                j += n
                full = ctx.ll_shapes[j - 1]
                if tuple(d.shape[-2:]) != full:      # the forward dropped a row / column of this low-pass
                    d = torch.nn.functional.pad(d, (0, full[1] - d.shape[-1], 0, full[0] - d.shape[-2]))
            if not ctx.needs_input_grad[0]:
                d = None
        return (d, None, None, None, None, None) + tuple(grads)


_PAD_LL = False   # inner-level LL_j at a cache-line-aligned row pitch for the per-level path (measured neutral: off)


class AFB2DMulti(Function):
    """J analysis levels as ONE autograd node: ``AFB2DMulti.apply(x, h0_row, h1_row, h0_col, h1_col,
    mode_int, J) -> (yl, yh_0, ..., yh_{J-1})``.

    Forward: up to three levels at a time in ONE launch of the streaming kernel (wl_dwt2d_analysis_fused: LL_j stay
    in LDS) whenever the engine takes the configuration - enough planes to fill the chip, even tap count <= 12,
    16-byte rows - otherwise one specialised tile-kernel launch per level (generic kernel for unusual tap counts /
    float64).  Backward = the chain of J AFB2D.backward steps of the reference (synthesis with the stored analysis
    taps + crop, dwt/lowlevel.py:350-365), coarsest level first - which is an inverse transform with the analysis taps,
    so it runs on the streaming synthesis kernel too (the crops are its 'unpad')."""

    @staticmethod
    def forward(ctx, x, h0_row, h1_row, h0_col, h1_col, mode, J):
        _check_bank_mode(mode)
        ctx.save_for_backward(h0_row, h1_row, h0_col, h1_col)
        ctx.mode = mode
        ctx.hints = ops.current_hints()     # (see SFB2DMulti: the backward pass is an inverse transform with these taps - same hints)
        shapes, yh, ll, done = [], [], x, 0
        while done < J:
            n = min(4, J - done)
            # small planes (CNN feature maps, CIFAR-sized images): several planes per workgroup, up to four levels in LDS
            res = ops.afb2d_small(ll, h0_row, h1_row, h0_col, h1_col, mode, n) if FUSED_LEVELS else None
            if res is None:
                n = min(3, J - done)
            while FUSED_LEVELS and n >= 1 and res is None:   # e.g. periodization: one level per streaming launch
                res = ops.afb2d_fused(ll, h0_row, h1_row, h0_col, h1_col, mode, n, whole=J == 1)
                if res is None:
                    n -= 1
            if res is None:
                n = 1
                shapes.append(tuple(ll.shape[-2:]))
                ll, high = ops.afb2d_best(ll, h0_row, h1_row, h0_col, h1_col, mode, pad_ll=_PAD_LL and done + 1 < J, more_levels=done + 1 < J)
                yh.append(high)
            else:
                shapes.append(tuple(ll.shape[-2:]))
                ll, highs = res
                shapes.extend(tuple(h.shape[-2:]) for h in highs[:-1])
                yh.extend(highs)
            done += n
        ctx.shapes = shapes
        return (ll,) + tuple(yh)

    @staticmethod
    @once_differentiable
    def backward(ctx, dyl, *dyh):
        with ops.hints(*ctx.hints):
            return AFB2DMulti._backward(ctx, dyl, *dyh)

    @staticmethod
    def _backward(ctx, dyl, *dyh):
        dx = None
        if ctx.needs_input_grad[0]:
            # an inverse transform with the analysis taps: the crop of each level to its input size is the inverse's 'unpad'
            dx, _ = _synthesis_ladder(dyl, dyh, ctx.saved_tensors, ctx.mode, out_hws=ctx.shapes)
            dx = dx.contiguous()             # (the crop after a multi-level launch is a view)
        return dx, None, None, None, None, None, None


class AFB1D(Function):
    """One level of 1-D analysis.  ``AFB1D.apply(x:(N,C,L), h0, h1, mode_int) -> (x0, x1)`` each (N,C,L')
    (reference dwt/lowlevel.py:368-424).  Backward = synthesis with the same stored taps, cropped to the input length."""

    @staticmethod
    def forward(ctx, x, h0, h1, mode):
        _check_bank_mode(mode)
        ctx.save_for_backward(h0, h1)
        ctx.shape = x.shape[2]
        ctx.mode = mode
        return ops.afb1d(x, h0, h1, mode, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dx0, dx1):
        dx = None
        if ctx.needs_input_grad[0]:
            h0, h1 = ctx.saved_tensors
            dx = ops.sfb1d(dx0, dx1, h0, h1, ctx.mode, 2, out_len=ctx.shape)
        return dx, None, None, None


class AFB1DMulti(Function):
    """All J levels of DWT1DForward as ONE autograd node: ``AFB1DMulti.apply(x, h0, h1, mode_int, J) -> (yl, yh_1 .. yh_J)`` =
    J x AFB1D chained (reference dwt/transform1d.py:44-59).  One launch of the fused 1-D kernel where the engine takes it
    (ops.afb1d_fused), the per-level launches otherwise; the backward is the chain of the per-level backward passes
    (synthesis with the same stored taps, cropped: reference dwt/lowlevel.py:409-424)."""

    @staticmethod
    def forward(ctx, x, h0, h1, mode, J):
        _check_bank_mode(mode)
        ctx.save_for_backward(h0, h1)
        ctx.mode = mode
        res = ops.afb1d_fused(x, h0, h1, mode, J) if FUSED_LEVELS else None
        if res is None:
            lo, his = x, []
            for _ in range(J):
                lo, hi = ops.afb1d(lo, h0, h1, mode, 2)
                his.append(hi)
        else:
            lo, his = res
        ctx.lens = [x.shape[2]] + [h.shape[2] for h in his[:-1]]
        return (lo,) + tuple(his)

    @staticmethod
    @once_differentiable
    def backward(ctx, dlo, *dhis):
        dx = None
        if ctx.needs_input_grad[0]:
            h0, h1 = ctx.saved_tensors
            dx = None
            if FUSED_LEVELS and len(dhis) <= 4 and all(d is not None for d in dhis):
                # one launch (csrc/wl_idwt1d_fused.h): the crops to the levels' input lengths are its 'unpad' / output length
                dx = ops.sfb1d_fused(dlo, list(dhis), h0, h1, ctx.mode, out_len=ctx.lens[0])
            if dx is None:
                dx = dlo
                for dh, n in zip(dhis[::-1], ctx.lens[::-1]):
                    dx = ops.sfb1d(dx, dh, h0, h1, ctx.mode, 2, out_len=n)
        return dx, None, None, None, None


class SFB1DMulti(Function):
    """All levels of DWT1DInverse as ONE autograd node: ``SFB1DMulti.apply(x0, g0, g1, mode_int, *highs) -> x`` with highs finest
    first, ``None`` entries = zeros (the level loop of DWT1DInverse.forward, reference dwt/transform1d.py:97-115, incl. the 'unpad'
    of a lowpass one sample longer than the next highpass).  One launch of the fused 1-D synthesis kernel where the engine takes
    it (ops.sfb1d_fused), the per-level launches otherwise; backward = the chain of SFB1D.backward steps (analysis with the stored
    synthesis taps, dwt/lowlevel.py:729-743), finest level first; a dropped sample gets a zero gradient."""

    @staticmethod
    def forward(ctx, x0, g0, g1, mode, *highs):
        _check_bank_mode(mode)
        ctx.save_for_backward(g0, g1)
        ctx.mode = mode
        ctx.has_highs = [h is not None for h in highs]
        J = len(highs)
        lo_lens = [None] * J            # length of the lowpass handed to level j, before the 'unpad'
        res = None
        if FUSED_LEVELS and 1 <= J <= 4 and all(ctx.has_highs):
            res = ops.sfb1d_fused(x0, list(highs), g0, g1, mode)
            if res is not None:
                n = x0.shape[-1]
                for j in range(J - 1, -1, -1):
                    lo_lens[j] = n
                    n = ops.synth_len(highs[j].shape[-1], g0.numel(), mode)
        if res is None:
            res = x0
            for j in range(J - 1, -1, -1):
                x1 = highs[j]
                lo_lens[j] = res.shape[-1]
                if x1 is None:
                    x1 = torch.zeros_like(res)
                if res.shape[-1] > x1.shape[-1]:
                    res = res[..., :-1]
                res = ops.sfb1d(res, x1, g0, g1, mode, 2)
        ctx.lo_lens = lo_lens
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        J = len(ctx.has_highs)
        grads = [None] * J
        d = None
        if ctx.needs_input_grad[0] or any(ctx.needs_input_grad[4 + j] for j in range(J)):
            g0, g1 = ctx.saved_tensors
            d = dy
            for j in range(J):
                d, dh = ops.afb1d(d, g0, g1, ctx.mode, 2)
                if ctx.has_highs[j] and ctx.needs_input_grad[4 + j]:
                    grads[j] = dh
                if d.shape[-1] < ctx.lo_lens[j]:         # the forward dropped the last sample of this lowpass
                    d = torch.nn.functional.pad(d, (0, ctx.lo_lens[j] - d.shape[-1]))
            if not ctx.needs_input_grad[0]:
                d = None
        return (d, None, None, None) + tuple(grads)


class SFB1D(Function):
    """One level of 1-D synthesis.  ``SFB1D.apply(low, high, g0, g1, mode_int) -> y`` (reference dwt/lowlevel.py:697-743).
    Backward = analysis with the stored synthesis taps."""

    @staticmethod
    def forward(ctx, low, high, g0, g1, mode):
        _check_bank_mode(mode)
        ctx.mode = mode
        ctx.save_for_backward(g0, g1)
        return ops.sfb1d(low, high, g0, g1, mode, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dlow, dhigh = None, None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g0, g1 = ctx.saved_tensors
            dlow, dhigh = ops.afb1d(dy, g0, g1, ctx.mode, 2)
        return dlow, dhigh, None, None, None


def _as_taps(h, x):
    """Array-likes are the pywt-ordered filters (reversed into cross-correlation taps, as the reference does when it is
    handed arrays); tensors are taken as already prepared."""
    if isinstance(h, torch.Tensor):
        return h
    return torch.tensor(np.copy(np.array(h, dtype=np.float64).ravel()[::-1]), dtype=torch.float, device=x.device)


def afb1d(x, h0, h1, mode='zero', dim=-1):
    """Function-level 1-D analysis along one axis of a 4-D tensor (reference dwt/lowlevel.py:91-172): returns the
    lowpass and highpass sub-bands interleaved along the channel axis, (N, 2C, H', W') with channel 2c = low."""
    d = dim % 4
    lo, hi = ops.afb1d(x, _as_taps(h0, x), _as_taps(h1, x), mode_to_int(mode), d)
    n, c = lo.shape[:2]
    return torch.stack([lo, hi], dim=2).reshape(n, 2 * c, lo.shape[2], lo.shape[3])


def sfb1d(lo, hi, g0, g1, mode='zero', dim=-1):
    """Function-level 1-D synthesis along one axis of 4-D tensors (reference dwt/lowlevel.py:226-271); array-like
    filters are used as given (no reversal), like upstream."""
    d = dim % 4

    def prep(g):
        return g if isinstance(g, torch.Tensor) else torch.tensor(np.copy(np.array(g, dtype=np.float64).ravel()),
                                                                  dtype=torch.float, device=lo.device)
    return ops.sfb1d(lo, hi, prep(g0), prep(g1), mode_to_int(mode), d)


_ATROUS_EXT = {'zero': ops.EXT_ZERO, 'constant': ops.EXT_ZERO, 'symmetric': ops.EXT_SYM, 'reflect': ops.EXT_REFL,
               'periodic': ops.EXT_PERIODIC, 'replicate': ops.EXT_REPLICATE}


def _atrous_geom(n, L, dilation):
    """(K, start) of the a-trous bank along an axis of n samples: the output length and the extended position its first
    output's first tap reads (reference dwt/lowlevel.py:175-223)."""
    L2 = (L * dilation) // 2
    return n + 2 * L2 - dilation - dilation * (L - 1), -(L2 - dilation)


class AFB1DAtrous(Function):
    """The a-trous bank along one axis as an autograd node: ``AFB1DAtrous.apply(x, h0, h1, ext, dim, dilation) -> (lo, hi)``.
    Backward = the transpose of the dilated correlation under the extension rule (ops.corr1d_adj) - upstream gets it from
    autograd through mypad + conv2d."""

    @staticmethod
    def forward(ctx, x, h0, h1, ext, dim, dilation):
        ctx.save_for_backward(h0, h1)
        ctx.geom = (ext, dim, dilation, x.shape[dim])
        K, start = _atrous_geom(x.shape[dim], h0.numel(), dilation)
        return ops.corr1d(x, dim, h0, h1, K, start, 1, dilation, ext)

    @staticmethod
    @once_differentiable
    def backward(ctx, dlo, dhi):
        dx = None
        if ctx.needs_input_grad[0]:
            h0, h1 = ctx.saved_tensors
            ext, dim, dilation, n = ctx.geom
            dx = ops.corr1d_adj(dlo, dhi, dim, h0, h1, n, _atrous_geom(n, h0.numel(), dilation)[1], dilation, ext)
        return dx, None, None, None, None, None


def afb1d_atrous(x, h0, h1, mode='periodic', dim=-1, dilation=1):
    """Undecimated (a-trous) 1-D analysis along one axis (reference dwt/lowlevel.py:175-223): the taps are dilated, the
    signal is padded by (L*dilation)//2 - dilation before and (L*dilation)//2 after with `mode`, the output keeps the
    input size.  Returns (N, 2C, H, W) with channel 2c = low; differentiable in x.  NB like upstream the padding is done by
    ``mypad``, which knows 'symmetric', 'periodic', 'constant', 'reflect', 'replicate' and 'zero' - 'periodization' raises."""
    if mode not in _ATROUS_EXT:
        raise ValueError("Unkown pad type: {}".format(mode))
    lo, hi = AFB1DAtrous.apply(x, _as_taps(h0, x), _as_taps(h1, x), _ATROUS_EXT[mode], dim % 4, dilation)
    nb, c = lo.shape[:2]
    return torch.stack([lo, hi], dim=2).reshape(nb, 2 * c, lo.shape[2], lo.shape[3])


def _atrous_level(x, t_row, t_col, ext, dilation):
    """One undecimated 2-D level, no autograd: the fused kernel (csrc/wl_swt2d.h: x read once, the four sub-bands written once
    in the returned layout), or the two single-axis passes for what it declines."""
    if FUSED_LEVELS and x.dim() == 4:
        y = ops.swt2d_level(x, t_row[0], t_row[1], t_col[0], t_col[1], dilation, ext)
        if y is not None:
            return y

    def bank(v, taps, dim):
        K, start = _atrous_geom(v.shape[dim], taps[0].numel(), dilation)
        lo, hi = ops.corr1d(v, dim, taps[0], taps[1], K, start, 1, dilation, ext)
        nb, c = lo.shape[:2]
        return torch.stack([lo, hi], dim=2).reshape(nb, 2 * c, lo.shape[2], lo.shape[3])
    return bank(bank(x, t_row, 3), t_col, 2)


def _atrous_level_adj(y, ll, ll_mode, t_row, t_col, ext, dilation, scale, hw):
    """scale * the transpose of _atrous_level: y (N,4C,Kh,Kw) or None -> (N,C,H,W), hw = (H, W); `ll` replaces (ll_mode 1) or is
    added to (2) the channels 4c + 0.  One launch (csrc/wl_iswt2d.h), or three of the single-axis transpose for what the fused
    kernel declines (mirror / replicate rules, dilated filters too long for its tile, odd L * dilation)."""
    if FUSED_LEVELS:
        x = ops.iswt2d_level(y, t_row[0], t_row[1], t_col[0], t_col[1], dilation, ext, scale, ll, ll_mode)
        if x is not None:
            return x
    H, W = hw
    sh = _atrous_geom(H, t_col[0].numel(), dilation)[1]
    sw = _atrous_geom(W, t_row[0].numel(), dilation)[1]
    u = []
    for r in (0, 1):                         # along H: the two bands b of each band r along W
        if y is None:
            y0, y1 = (ll if r == 0 else None), None
        else:
            y0, y1 = y[:, 2 * r::4], y[:, 2 * r + 1::4]
            if r == 0 and ll_mode == 1:
                y0 = ll
            elif r == 0 and ll_mode == 2:
                y0 = y0 + ll
        if y0 is None:
            u.append(None)
        else:
            u.append(ops.corr1d_adj(y0, y1, 2, t_col[0], None if y1 is None else t_col[1], H, sh, dilation, ext))
    if u[1] is None:
        return ops.corr1d_adj(u[0], None, 3, t_row[0], None, W, sw, dilation, ext, scale)
    return ops.corr1d_adj(u[0], u[1], 3, t_row[0], t_row[1], W, sw, dilation, ext, scale)


class AFB2DAtrousMulti(Function):
    """J undecimated 2-D levels as ONE autograd node: ``AFB2DAtrousMulti.apply(x, h0_row, h1_row, h0_col, h1_col, ext,
    dilation, J) -> (y_1 .. y_J)``, level j on the ll channels of level j-1 (a strided view, no copy) with the taps dilated by
    dilation * 2**(j-1).  Backward: one launch of the transposed level per level, coarsest first; the gradient that arrives
    from level j+1 joins the user's gradient on the ll channels inside the kernel (no clone, no zeros_like), and a level whose
    output nobody used contributes nothing but what comes through its ll channels."""

    @staticmethod
    def forward(ctx, x, h0_row, h1_row, h0_col, h1_col, ext, dilation, J):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h0_row, h1_row, h0_col, h1_col)
        outs, hws, ll = [], [], x
        for j in range(J):
            hws.append(tuple(ll.shape[-2:]))
            y = _atrous_level(ll, (h0_row, h1_row), (h0_col, h1_col), ext, dilation * 2 ** j)
            outs.append(y)
            ll = y[:, 0::4]
        ctx.geom = (ext, dilation, hws)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dys):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        h0_row, h1_row, h0_col, h1_col = ctx.saved_tensors
        ext, dilation, hws = ctx.geom
        carry = None
        for j in range(len(dys) - 1, -1, -1):
            dy = dys[j]
            if dy is None and carry is None:
                continue
            ll_mode = 0 if carry is None else (1 if dy is None else 2)
            carry = _atrous_level_adj(dy, carry, ll_mode, (h0_row, h1_row), (h0_col, h1_col), ext, dilation * 2 ** j, 1.0, hws[j])
        return (carry,) + (None,) * 7


def _atrous_filts(filts, ref, prep):
    """The reference's 2- / 4-tuple of filters (arrays or prepared tensors) -> (col lo, col hi, row lo, row hi)."""
    tensorize = [not isinstance(f, torch.Tensor) for f in filts]
    if len(filts) == 2:
        f0, f1 = filts
        if True in tensorize:
            return prep(f0, f1, device=ref.device)
        return f0, f1, f0.transpose(2, 3), f1.transpose(2, 3)
    if len(filts) == 4:
        if True in tensorize:
            return prep(*filts, device=ref.device)
        return tuple(filts)
    raise ValueError("Unknown form for input filts")


def afb2d_atrous_multi(x, filts, mode, dilation, J):
    """J undecimated levels (SWTForward.forward's loop): a list of (N, 4C, H, W), level j+1 on the ll channels of level j with
    the taps dilated twice as far; differentiable in x."""
    h0_col, h1_col, h0_row, h1_row = _atrous_filts(filts, x, prep_filt_afb2d)
    if mode not in _ATROUS_EXT:
        raise ValueError("Unkown pad type: {}".format(mode))
    if J < 1:
        return []
    return list(AFB2DAtrousMulti.apply(x, _as_taps(h0_row, x), _as_taps(h1_row, x), _as_taps(h0_col, x), _as_taps(h1_col, x),
                                       _ATROUS_EXT[mode], dilation, J))


def afb2d_atrous(x, filts, mode='periodization', dilation=1):
    """One undecimated 2-D level (reference dwt/lowlevel.py:475-521): rows then columns; returns (N, 4C, H, W) with
    channel 4c + 2r + b (r: band along W, b: band along H), i.e. (ll, lh, hl, hh) per input channel.  Differentiable in x (one
    launch of the transposed level, csrc/wl_iswt2d.h)."""
    return afb2d_atrous_multi(x, filts, mode, dilation, 1)[0]


# ---- the way back: the transposed a-trous bank with the synthesis taps ------------------------------------------------------
# Upstream's dwt/swt_inverse.py is dead code (no imports; its forward calls the decimated sfb2d; its sfb1d_atrous divides by
# 2 * dilation), so the inverse is defined here by its mathematics.  With A_b(g, periodic, d) the n x n matrix of afb1d_atrous for
# the stored synthesis taps g_b (pywt's rec_lo / rec_hi, as prep_filt_sfb2d stores them) and B_b the same for the analysis taps,
#     1/2 (A_0(g)^T B_0 + A_1(g)^T B_1) = I        for every pywt wavelet, even tap count and dilation,
# i.e. per axis x = 1/2 (A_0(g)^T lo + A_1(g)^T hi), per 2-D level 1/4 of the four-band sum.  In the other pad modes the forward
# keeps n samples and loses what the border needs: 'periodic' only.
def _check_atrous_inverse(mode, *taps):
    if mode != 'periodic':
        raise ValueError("the inverse stationary transform is defined for mode 'periodic' only, not {!r}".format(mode))
    for t in taps:
        if t.numel() % 2:
            raise ValueError("the inverse stationary transform needs an even number of taps, not {}".format(t.numel()))


def _as_syn_taps(g, ref):
    """Array-likes are used as given (no reversal), like sfb1d / sfb2d; tensors are taken as already prepared."""
    if isinstance(g, torch.Tensor):
        return g
    return torch.tensor(np.copy(np.array(g, dtype=np.float64).ravel()), dtype=torch.float, device=ref.device)


class SFB1DAtrous(Function):
    """``SFB1DAtrous.apply(lo, hi, g0, g1, dim, dilation) -> x = 1/2 (A_0(g)^T lo + A_1(g)^T hi)``, periodic; backward = 1/2 of
    the a-trous analysis with the synthesis taps."""

    @staticmethod
    def forward(ctx, lo, hi, g0, g1, dim, dilation):
        ctx.save_for_backward(g0, g1)
        ctx.geom = (dim, dilation)
        n = lo.shape[dim]
        return ops.corr1d_adj(lo, hi, dim, g0, g1, n, _atrous_geom(n, g0.numel(), dilation)[1], dilation, ops.EXT_PERIODIC, 0.5)

    @staticmethod
    @once_differentiable
    def backward(ctx, dx):
        g0, g1 = ctx.saved_tensors
        dim, dilation = ctx.geom
        K, start = _atrous_geom(dx.shape[dim], g0.numel(), dilation)
        dlo, dhi = ops.corr1d(dx, dim, g0, g1, K, start, 1, dilation, ops.EXT_PERIODIC)
        return dlo.mul_(0.5), dhi.mul_(0.5), None, None, None, None


def sfb1d_atrous(lo, hi, g0, g1, mode='periodic', dim=-1, dilation=1):
    """The inverse of afb1d_atrous along one axis of 4-D tensors: x = 1/2 (A_0(g)^T lo + A_1(g)^T hi), A_b(g) the a-trous
    analysis matrix of the synthesis taps (arrays are used as given, like sfb1d).  Upstream's sketch of this function
    (dwt/swt_inverse.py) pads, runs conv_transpose2d and divides by 2*dilation, and was never run; this one inverts
    afb1d_atrous exactly in 'periodic' mode and raises ValueError in every other."""
    t0, t1 = _as_syn_taps(g0, lo), _as_syn_taps(g1, lo)
    _check_atrous_inverse(mode, t0, t1)
    if lo.shape != hi.shape:
        raise ValueError("lo is {} and hi is {}".format(tuple(lo.shape), tuple(hi.shape)))
    return SFB1DAtrous.apply(lo, hi, t0, t1, dim % lo.dim(), dilation)


# ---- the 1-D stationary transform along the last axis ----------------------------------------------------------------------------
# Level j = afb1d_atrous with dilation 2**(j-1) on the previous lowpass.  Periodic, even L <= 20, not float64: the first (up to)
# three levels are ONE launch of the wave-tile kernels (csrc/wl_swt1d.h: x read once, the intermediate lowpasses stay fp32 in
# registers); deeper levels and everything else go level by level on corr1d / corr1d_adj, with the same answer.
def _swt1d_fused_levels(t, L, ext, J):
    if not ops.SWT1D_FUSED or ext != ops.EXT_PERIODIC or not ops.wave1d_covered(t.dtype, L):
        return 0
    return min(J, ops.SWT1D_MAXJ)


def _swt1d_analysis(x, h0, h1, ext, J, scale=1.0):
    """J levels of scale * the a-trous bank along the last axis, no autograd -> (lo, [hi_1 ..], [n_0 ..]): n_j = the length of
    the input of level j + 1 (odd tap counts lose a sample per level)."""
    L = h0.numel()
    lo, his, ns, j = x, [], [], 0
    nf = _swt1d_fused_levels(x, L, ext, J)
    if nf:
        res = ops.swt1d_fwd(x, h0, h1, nf, scale=scale)
        if res is not None:
            lo, his = res[0], list(res[1])
            ns, j = [x.shape[-1]] * nf, nf
    while j < J:
        n = lo.shape[-1]
        K, start = _atrous_geom(n, L, 2 ** j)
        if K < 1:
            raise ValueError("level {} of the stationary transform is left without samples".format(j + 1))
        lo, hi = ops.corr1d(lo, -1, h0, h1, K, start, 1, 2 ** j, ext)
        if scale != 1.0:
            lo.mul_(scale), hi.mul_(scale)
        his.append(hi)
        ns.append(n)
        j += 1
    return lo, his, ns


def _swt1d_adjoint(lo, his, g0, g1, ext, ns, scale=1.0):
    """The transpose of _swt1d_analysis times scale per level: his finest first, None = zeros; ns[j] = the length of the output
    of level j + 1's transpose."""
    J, L = len(his), g0.numel()
    nf = _swt1d_fused_levels(lo, L, ext, J)
    j = J
    while j > 0:
        if j == nf:
            y = ops.swt1d_adj(lo, his[:nf], g0, g1, scale)
            if y is not None:
                return y
        hi = his[j - 1]
        start = _atrous_geom(ns[j - 1], L, 2 ** (j - 1))[1]
        lo = ops.corr1d_adj(lo, hi, -1, g0, None if hi is None else g1, ns[j - 1], start, 2 ** (j - 1), ext, scale)
        j -= 1
    return lo


# ---- the gradients of the filter taps --------------------------------------------------------------------------------------------
# Periodic, even L.  With d_j = 2^(j-1), a signal s, a top v_J, highs w_j (None = zeros), taps k and the per-level scale sigma:
#     u_0 = s, u_j = sigma A0_j(k0) u_{j-1};        v_{j-1} = sigma (A0_j(k0)^T v_j + A1_j(k1)^T w_j)
#     c0[t] = sigma sum_j sum_p u_{j-1}[p + (t - (L/2 - 1)) d_j] v_j[p],        c1[t] = the same with w_j[p]
# (x, dlo, dhi, h, 1) gives (dh0, dh1) of SWT1DMulti, (dx, lo, hi, g, 1/2) gives (dg0, dg1) of ISWT1DMulti.  Up to three levels of
# float32 / float16 / bfloat16 data are ONE launch (csrc/wl_swt1d_tapgrad.h); everything else is the composition below, which is
# also the definition.
def _check_tap_grad_envelope(ext, *taps):
    if ext != ops.EXT_PERIODIC:
        raise ValueError("the filter taps of the stationary transform have a gradient in mode 'periodic' only")
    for t in taps:
        if t.numel() % 2:
            raise ValueError("the gradient of the filter taps needs an even number of taps, not {}".format(t.numel()))
    if taps[0].numel() != taps[1].numel():
        raise ValueError("the gradient of the filter taps needs two filters of one length, not {} and {}".format(
            taps[0].numel(), taps[1].numel()))


def _swt1d_tapgrad_composed(s, top, his, k0, k1, scale):
    """The definition: both chains one level at a time on corr1d / corr1d_adj, and per level and tap a rolled product summed in
    float64 on the device -> (c0, c1), float64 (L,)."""
    J, L, n = len(his), k0.numel(), s.shape[-1]
    ext = ops.EXT_PERIODIC
    us = [s]
    for j in range(J - 1):
        K, start = _atrous_geom(n, L, 2 ** j)
        lo, _ = ops.corr1d(us[-1], -1, k0, k1, K, start, 1, 2 ** j, ext)
        us.append(lo.mul_(scale) if scale != 1.0 else lo)
    c0 = torch.zeros(L, dtype=torch.float64, device=s.device)
    c1 = torch.zeros(L, dtype=torch.float64, device=s.device)
    v = top
    for j in range(J - 1, -1, -1):
        d, w = 2 ** j, his[j]
        v64 = v.double()
        w64 = None if w is None else w.double()
        for t in range(L):
            u64 = torch.roll(us[j], -(t - (L // 2 - 1)) * d, -1).double()
            c0[t] += (u64 * v64).sum()
            if w64 is not None:
                c1[t] += (u64 * w64).sum()
        if j:
            v = ops.corr1d_adj(v, w, -1, k0, None if w is None else k1, n, _atrous_geom(n, L, d)[1], d, ext, scale)
    return c0 * scale, c1 * scale


def _swt1d_tapgrad(s, top, his, k0, k1, scale):
    """(c0, c1) shaped and typed like k0 / k1: one launch where the kernel covers the call, the composition otherwise."""
    res = None
    if len(his) <= ops.SWT1D_MAXJ:
        res = ops.swt1d_tapgrad(s, top, his, k0, k1, scale)
    if res is None:
        res = _swt1d_tapgrad_composed(s, top, his, k0, k1, scale)
    return res[0].to(k0.dtype).reshape(k0.shape), res[1].to(k1.dtype).reshape(k1.shape)


class SWT1DMulti(Function):
    """``SWT1DMulti.apply(x, h0, h1, ext, J) -> (lo, hi_1 .. hi_J)``: all levels of the 1-D stationary analysis as ONE autograd
    node.  Backward = the transposed cascade with the same taps; a tap tensor that asks for a gradient ('periodic', even L) gets
    it from _swt1d_tapgrad, for which x is saved as well."""

    @staticmethod
    def forward(ctx, x, h0, h1, ext, J):
        ctx.taps_learn = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if ctx.taps_learn:
            ctx.save_for_backward(h0, h1, x)
        else:
            ctx.save_for_backward(h0, h1)
        lo, his, ns = _swt1d_analysis(x, h0, h1, ext, J)
        ctx.geom = (ext, ns)
        return (lo,) + tuple(his)

    @staticmethod
    @once_differentiable
    def backward(ctx, dlo, *dhis):
        dx = dh0 = dh1 = None
        ext, ns = ctx.geom
        if ctx.needs_input_grad[0]:
            h0, h1 = ctx.saved_tensors[:2]
            dx = _swt1d_adjoint(dlo, list(dhis), h0, h1, ext, ns)
        if ctx.taps_learn:
            h0, h1, x = ctx.saved_tensors
            dh0, dh1 = _swt1d_tapgrad(x, dlo, list(dhis), h0, h1, 1.0)
            dh0 = dh0 if ctx.needs_input_grad[1] else None
            dh1 = dh1 if ctx.needs_input_grad[2] else None
        return dx, dh0, dh1, None, None


class ISWT1DMulti(Function):
    """``ISWT1DMulti.apply(lo, g0, g1, *his) -> x``: all levels of the inverse 1-D stationary transform, coarsest first
    lo_{j-1} = 1/2 (A_0(g)^T lo_j + A_1(g)^T hi_j), as ONE autograd node; his finest first, None = zeros.  Backward = 1/2 per
    level of the analysis cascade with the synthesis taps; a tap tensor that asks for a gradient gets it from _swt1d_tapgrad, for
    which lo and the highs that are present are saved as well."""

    @staticmethod
    def forward(ctx, lo, g0, g1, *his):
        ctx.taps_learn = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ctx.present = [h is not None for h in his]
        if ctx.taps_learn:
            ctx.save_for_backward(g0, g1, lo, *[h for h in his if h is not None])
        else:
            ctx.save_for_backward(g0, g1)
        n = lo.shape[-1]
        return _swt1d_adjoint(lo, list(his), g0, g1, ops.EXT_PERIODIC, [n] * len(his), 0.5)

    @staticmethod
    @once_differentiable
    def backward(ctx, dx):
        g0, g1 = ctx.saved_tensors[:2]
        grads = (None,) * len(ctx.present)
        dlo = dg0 = dg1 = None
        if any(ctx.needs_input_grad[:1] + ctx.needs_input_grad[3:]) or not ctx.taps_learn:
            dlo, dhis, _ = _swt1d_analysis(dx, g0, g1, ops.EXT_PERIODIC, len(ctx.present), 0.5)
            # (level j's bands carry the factors of the levels above it as well: they were applied on the way down)
            grads = tuple(d if p else None for d, p in zip(dhis, ctx.present))
        if ctx.taps_learn:
            kept = iter(ctx.saved_tensors[3:])
            his = [next(kept) if p else None for p in ctx.present]
            dg0, dg1 = _swt1d_tapgrad(dx, ctx.saved_tensors[2], his, g0, g1, 0.5)
            dg0 = dg0 if ctx.needs_input_grad[1] else None
            dg1 = dg1 if ctx.needs_input_grad[2] else None
        return (dlo, dg0, dg1) + grads


def _check_swt1d_input(t, name):
    if t.dim() != 3:
        raise ValueError("{} must be (N, C, L), not {}".format(name, tuple(t.shape)))


def swt1d(x, h0, h1, mode='periodic', J=1):
    """J levels of the 1-D stationary (undecimated) transform of x (N, C, L) along L: (yl, [yh_1 .. yh_J]) finest first, every
    tensor (N, C, L).  Level j is afb1d_atrous with dilation 2**(j-1) on the previous lowpass (stored taps, the six pad modes of
    afb1d_atrous; any other mode raises its ValueError).  Differentiable in x, and in tap tensors that require a gradient
    ('periodic', two filters of one even length: ValueError otherwise)."""
    if mode not in _ATROUS_EXT:
        raise ValueError("Unkown pad type: {}".format(mode))
    _check_swt1d_input(x, 'x')
    if J < 1:
        return x, []
    h0, h1 = _as_taps(h0, x), _as_taps(h1, x)
    if torch.is_grad_enabled() and (h0.requires_grad or h1.requires_grad):
        _check_tap_grad_envelope(_ATROUS_EXT[mode], h0, h1)
    outs = SWT1DMulti.apply(x, h0, h1, _ATROUS_EXT[mode], J)
    return outs[0], list(outs[1:])


def iswt1d(yl, yh, g0, g1, mode='periodic'):
    """The inverse of swt1d: yl (N, C, L) and yh = [finest .. coarsest] (None = zeros) -> x (N, C, L), per level, coarsest first,
    lo_{j-1} = 1/2 (A_0(g)^T lo_j + A_1(g)^T hi_j) - the 1-D case of sfb1d_atrous.  'periodic' and even tap counts only.
    Differentiable in yl, yh and in tap tensors that require a gradient (two filters of one length)."""
    t0, t1 = _as_syn_taps(g0, yl), _as_syn_taps(g1, yl)
    _check_atrous_inverse(mode, t0, t1)
    _check_swt1d_input(yl, 'yl')
    yh = list(yh)
    for h in yh:
        if h is not None and h.shape != yl.shape:
            raise ValueError("yl is {} and a level of yh is {}".format(tuple(yl.shape), tuple(h.shape)))
    if not yh:
        return yl
    if torch.is_grad_enabled() and (t0.requires_grad or t1.requires_grad):
        _check_tap_grad_envelope(ops.EXT_PERIODIC, t0, t1)
    return ISWT1DMulti.apply(yl, t0, t1, *yh)


# ---- shrinkage of the 1-D stationary transform -----------------------------------------------------------------------------------
# y = iswt1d(lo_J, shrink(hi_j, t_j)) of swt1d(x).  Periodic, four even filters of one length <= 20, J <= 3, not float64: ONE launch
# per direction of the wave-tile kernels (csrc/wl_shrink1d.h: the coefficients never leave registers, the backward recomputes
# them); everything else is the composition below with ordinary autograd, which is also the definition.
class _ShrinkDeclined(Exception):
    """The launcher declined a call ops.shrink1d_covered let through (a memoised decline, an engine option): swt1d_shrink
    composes instead."""


class SWT1DShrinkF(Function):
    """``SWT1DShrinkF.apply(x, table, h0, h1, g0, g1, J, kind) -> y``: table = the float32 (J, N, C) thresholds.  One autograd
    node that saves x and the table; the backward is one launch, which writes the tiles' shares of d table only when the table
    asks for a gradient.  A forward the launcher declines raises _ShrinkDeclined; a backward it declines differentiates the
    composition on the saved x and table."""

    @staticmethod
    def forward(ctx, x, table, h0, h1, g0, g1, J, kind):
        y = ops.shrink1d_fwd(x, table, h0, h1, g0, g1, J, kind)
        if y is None:
            raise _ShrinkDeclined()
        ctx.save_for_backward(x, table, h0, h1, g0, g1)
        ctx.geom = (J, kind)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 8
        x, table, h0, h1, g0, g1 = ctx.saved_tensors
        J, kind = ctx.geom
        res = ops.shrink1d_bwd(x, dy, table, h0, h1, g0, g1, J, kind, need_dthr=ctx.needs_input_grad[1])
        if res is None:
            with torch.enable_grad():
                xr, tr = x.detach().requires_grad_(True), table.detach().requires_grad_(True)
                dx, dtable = torch.autograd.grad(_shrink_composed(xr, tr, h0, h1, g0, g1, J, kind), (xr, tr), dy)
            return (dx if ctx.needs_input_grad[0] else None, dtable if ctx.needs_input_grad[1] else None) + (None,) * 6
        dx, part = res
        dtable = None
        if part is not None:
            dtable = part.sum(1).t().reshape(table.shape)          # (rows, tiles, J) -> (J, N, C)
        return (dx if ctx.needs_input_grad[0] else None, dtable) + (None,) * 6


def _shrink_table(thresh, J, N, C, ref):
    """The thresholds as a (J, N, C) view: 0-d, (J,), or 3-d with every dimension 1 or the size of (J, N, C)."""
    if not isinstance(thresh, torch.Tensor):
        thresh = torch.as_tensor(thresh, dtype=torch.float32, device=ref.device)
    if not thresh.is_floating_point():
        thresh = thresh.float()
    ops._same_device(ref, thresh)
    if thresh.dim() == 1 and thresh.shape[0] == J:
        thresh = thresh.reshape(J, 1, 1)
    elif thresh.dim() == 0:
        thresh = thresh.reshape(1, 1, 1)
    elif thresh.dim() != 3 or any(s not in (1, full) for s, full in zip(thresh.shape, (J, N, C))):
        raise ValueError("thresh must be 0-d, ({},) or 3-d with every dimension 1 or that of ({}, {}, {}), not {}".format(
            J, J, N, C, tuple(thresh.shape)))
    return thresh.expand(J, N, C)


def shrink(w, t, kind='soft'):
    """Element-wise shrinkage with ordinary autograd: soft sign(w) max(|w| - t, 0), hard w [|w| > t]; hard gives t a zero
    gradient.  The result has w's dtype."""
    if kind == 'soft':
        out = torch.sign(w) * torch.clamp(w.abs() - t, min=0)
    else:
        out = w * (w.abs() > t)
        if isinstance(t, torch.Tensor) and t.requires_grad:
            out = out + 0 * t
    return out.to(w.dtype)


def _shrink_composed(x, table, h0, h1, g0, g1, J, kind):
    """The definition: swt1d, element-wise shrinkage under table (J, N, C), iswt1d, with ordinary autograd."""
    lo, his = swt1d(x, h0, h1, 'periodic', J)
    return iswt1d(lo, [shrink(hi, table[j].unsqueeze(-1), kind) for j, hi in enumerate(his)], g0, g1, 'periodic')


def swt1d_shrink(x, h0, h1, g0, g1, thresh, J, kind='soft', mode='periodic'):
    """Translation-invariant wavelet shrinkage of x (N, C, L) along L: ``iswt1d(lo_J, [shrink(hi_j, t_j)])`` of
    ``swt1d(x, h0, h1, 'periodic', J)``, soft ``sign(w) max(|w| - t, 0)`` or hard ``w [|w| > t]``, with t_j the threshold of
    level j for the row's (n, c): `thresh` is 0-d, (J,) or 3-d with every dimension 1 or that of (J, N, C), and is used as given
    (no clamp).  Differentiable in x and thresh (hard: zeros for thresh).  One launch per direction where the kernels cover
    the call (ops.shrink1d_covered); otherwise - float64, J > 3, odd, long or unequal filters, ops.SHRINK1D_FUSED off, a tap
    tensor that requires a gradient - the composition.  'periodic' and even tap counts only, as the inverse."""
    h0, h1 = _as_taps(h0, x), _as_taps(h1, x)
    g0, g1 = _as_syn_taps(g0, x), _as_syn_taps(g1, x)
    _check_atrous_inverse(mode, h0, h1, g0, g1)
    if kind not in ops.SHRINK1D_KINDS:
        raise ValueError("kind must be 'soft' or 'hard', not {!r}".format(kind))
    _check_swt1d_input(x, 'x')
    ops._check_tensor(x, 'x')
    if J < 1:
        return x
    N, C = x.shape[:2]
    table = _shrink_table(thresh, J, N, C, x)
    if x.numel() == 0:
        return x.clone()
    # (filters that are learned: the composition, whose two transform nodes have the tap gradients - the fused kernels have none)
    taps_learn = torch.is_grad_enabled() and any(t.requires_grad for t in (h0, h1, g0, g1))
    if not taps_learn and ops.shrink1d_covered(x, h0, h1, g0, g1, J):
        try:
            return SWT1DShrinkF.apply(x, table.to(torch.float32).contiguous(), h0, h1, g0, g1, J, kind)
        except _ShrinkDeclined:
            pass
    return _shrink_composed(x, table, h0, h1, g0, g1, J, kind)


class SWTInvMulti(Function):
    """All levels of the inverse stationary transform as ONE autograd node: ``SWTInvMulti.apply(g0_row, g1_row, g0_col, g1_col,
    dilation, *coeffs) -> x`` with coeffs[j] (N,4C,H,W), finest first, level j dilated by dilation * 2**j.  It starts from the ll
    channels of the last entry; the ll channels of the finer entries are redundant and ignored (the reconstructed ll of the
    coarser level takes their place inside the kernel).  Backward = 1/4 of the a-trous analysis (csrc/wl_swt2d.h) with the
    synthesis taps, level by level."""

    @staticmethod
    def forward(ctx, g0_row, g1_row, g0_col, g1_col, dilation, *coeffs):
        ctx.save_for_backward(g0_row, g1_row, g0_col, g1_col)
        ctx.geom = (dilation, len(coeffs))
        ctx.needs = [ctx.needs_input_grad[5 + j] for j in range(len(coeffs))]
        ll = None
        for j in range(len(coeffs) - 1, -1, -1):
            ll = _atrous_level_adj(coeffs[j], ll, 0 if ll is None else 1, (g0_row, g1_row), (g0_col, g1_col), ops.EXT_PERIODIC,
                                   dilation * 2 ** j, 0.25, tuple(coeffs[j].shape[-2:]))
        return ll

    @staticmethod
    @once_differentiable
    def backward(ctx, dx):
        g0_row, g1_row, g0_col, g1_col = ctx.saved_tensors
        dilation, J = ctx.geom
        grads, cur = [], dx
        for j in range(J):
            if not any(ctx.needs[j:]):
                break
            g = _atrous_level(cur, (g0_row, g1_row), (g0_col, g1_col), ops.EXT_PERIODIC, dilation * 2 ** j).mul_(0.25)
            grads.append(g)
            cur = g[:, 0::4]
        for g in grads[:J - 1]:
            g[:, 0::4].zero_()                  # the ll channels of the finer levels were not read
        grads = [g if ctx.needs[j] else None for j, g in enumerate(grads)] + [None] * (J - len(grads))
        return (None,) * 5 + tuple(grads)


def _swt_inverse(coeffs, taps, dilation=1):
    coeffs = list(coeffs)
    if len(coeffs) == 0:
        raise ValueError("no coefficients: SWTInverse takes the list SWTForward returns")
    shape = tuple(coeffs[0].shape)
    if len(shape) != 4 or shape[1] % 4:
        raise ValueError("a level is (N, 4C, H, W), not {}".format(shape))
    for c in coeffs[1:]:
        if tuple(c.shape) != shape or c.dtype != coeffs[0].dtype:
            raise ValueError("the levels differ: {} {} and {} {}".format(shape, coeffs[0].dtype, tuple(c.shape), c.dtype))
    g0_col, g1_col, g0_row, g1_row = taps
    return SWTInvMulti.apply(g0_row, g1_row, g0_col, g1_col, dilation, *coeffs)


def sfb2d_atrous(ll, lh, hl, hh, filts, mode='periodic', dilation=1):
    """The inverse of afb2d_atrous: the four sub-bands (N, C, H, W) of one level -> x (N, C, H, W), 1/4 of the transposed a-trous
    bank of the synthesis filters (``filts`` as for sfb2d: (g0_col, g1_col[, g0_row, g1_row]), arrays as given).  'periodic'
    only: ValueError for any other mode."""
    g0_col, g1_col, g0_row, g1_row = _atrous_filts(filts, ll, prep_filt_sfb2d)
    taps = tuple(_as_syn_taps(g, ll) for g in (g0_col, g1_col, g0_row, g1_row))
    _check_atrous_inverse(mode, *taps)
    n, c = ll.shape[:2]
    y = torch.stack([ll, lh, hl, hh], dim=2).reshape(n, 4 * c, ll.shape[2], ll.shape[3])
    return _swt_inverse([y], taps, dilation)


def prep_filt_afb2d_nonsep(h0_col, h1_col, h0_row=None, h1_row=None, device=None):
    """The four 2-D point-spread functions (ll, lh, hl, hh) of an analysis bank as a (4, 1, Ly, Lx) tensor, mirrored for
    cross-correlation (reference dwt/lowlevel.py:801-833)."""
    h0_col = np.array(h0_col).ravel()
    h1_col = np.array(h1_col).ravel()
    h0_row = h0_col if h0_row is None else np.array(h0_row).ravel()
    h1_row = h1_col if h1_row is None else np.array(h1_row).ravel()
    psf = [np.outer(c, r)[::-1, ::-1] for c, r in ((h0_col, h0_row), (h1_col, h0_row), (h0_col, h1_row), (h1_col, h1_row))]
    return torch.tensor(np.stack(psf)[:, None].copy(), dtype=torch.get_default_dtype(), device=device)


def prep_filt_sfb2d_nonsep(g0_col, g1_col, g0_row=None, g1_row=None, device=None):
    """The four 2-D point-spread functions of a synthesis bank as a (4, 1, Ly, Lx) tensor, not mirrored (reference
    dwt/lowlevel.py:836-867)."""
    g0_col = np.array(g0_col).ravel()
    g1_col = np.array(g1_col).ravel()
    g0_row = g0_col if g0_row is None else np.array(g0_row).ravel()
    g1_row = g1_col if g1_row is None else np.array(g1_row).ravel()
    psf = [np.outer(c, r) for c, r in ((g0_col, g0_row), (g1_col, g0_row), (g0_col, g1_row), (g1_col, g1_row))]
    return torch.tensor(np.stack(psf)[:, None], dtype=torch.get_default_dtype(), device=device)


class _AFB2DNonsep(Function):
    """afb2d_nonsep as an autograd node.  Backward = the true adjoint of the boundary gather + strided correlation in
    every mode - what autograd gives upstream, where the function is a plain ATen chain (dwt/lowlevel.py:524-597):
    mirrored / wrapped / repeated samples fold their gradient back onto their source (one kernel launch)."""

    @staticmethod
    def forward(ctx, x, filts, mode):
        ctx.save_for_backward(filts)
        ctx.mode, ctx.shape = mode, tuple(x.shape)
        return ops.afb2d_nonsep(x, filts, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dx = None
        if ctx.needs_input_grad[0]:
            filts, = ctx.saved_tensors
            dx = ops.afb2d_nonsep_bwd(dy, filts, ctx.mode, ctx.shape[-2:])
        return dx, None, None


class _SFB2DNonsep(Function):
    """sfb2d_nonsep as an autograd node.  Backward = an analysis of the gradient with the same point-spread functions
    (zero extension; periodic for periodization) - the exact adjoint in every mode, one kernel launch."""

    @staticmethod
    def forward(ctx, coeffs, filts, mode):
        ctx.save_for_backward(filts)
        ctx.mode, ctx.shape = mode, tuple(coeffs.shape)
        return ops.sfb2d_nonsep(coeffs, filts, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dc = None
        if ctx.needs_input_grad[0]:
            filts, = ctx.saved_tensors
            dc = ops.sfb2d_nonsep_bwd(dy, filts, ctx.mode, ctx.shape)
        return dc, None, None


def afb2d_nonsep(x, filts, mode='zero'):
    """One analysis level WITHOUT separate row and column filtering (reference dwt/lowlevel.py:524-597): ``filts`` =
    the (4,1,Ly,Lx) tensor of prep_filt_afb2d_nonsep, or a 2- / 4-tuple of 1-D banks.  Returns (N, 4C, H', W').
    'zero', 'symmetric', 'reflect', 'periodization' ('periodic' raises, as upstream)."""
    if isinstance(filts, (tuple, list)):
        filts = prep_filt_afb2d_nonsep(*filts, device=x.device)
    if mode not in ('zero', 'symmetric', 'reflect', 'periodization', 'per'):
        raise ValueError("Unkown pad type: {}".format(mode))
    return _AFB2DNonsep.apply(x, filts, mode_to_int(mode))


def sfb2d_nonsep(coeffs, filts, mode='zero'):
    """One synthesis level without separable filtering (reference dwt/lowlevel.py:746-798): coeffs (N,C,4,H,W) ->
    (N,C,2H-Ly+2,2W-Lx+2) (periodization: (N,C,2H,2W)); ``filts`` = the tensor of prep_filt_sfb2d_nonsep or a 2- /
    4-tuple of 1-D banks."""
    if isinstance(filts, (tuple, list)):
        if len(filts) not in (2, 4):
            raise ValueError("Unkown form for input filts")
        filts = prep_filt_sfb2d_nonsep(*filts, device=coeffs.device)
    if mode not in ('zero', 'symmetric', 'reflect', 'periodic', 'periodization', 'per'):
        raise ValueError("Unkown pad type: {}".format(mode))
    return _SFB2DNonsep.apply(coeffs, filts, mode_to_int(mode))


def afb2d(x, filts, mode='zero'):
    """Function-level analysis (reference dwt/lowlevel.py:427-472): ``filts`` is a 2- or 4-tuple
    of arrays / tensors (h0_col, h1_col[, h0_row, h1_row]); here the *col* pair really filters
    along H (the Module path swaps them, quirk Q1).  Returns (N, 4C, H', W')."""
    tensorize = [not isinstance(f, torch.Tensor) for f in filts]
    if len(filts) == 2:
        h0, h1 = filts
        if True in tensorize:
            h0_col, h1_col, h0_row, h1_row = prep_filt_afb2d(h0, h1, device=x.device)
        else:
            h0_col, h0_row, h1_col, h1_row = h0, h0.transpose(2, 3), h1, h1.transpose(2, 3)
    elif len(filts) == 4:
        if True in tensorize:
            h0_col, h1_col, h0_row, h1_row = prep_filt_afb2d(*filts, device=x.device)
        else:
            h0_col, h1_col, h0_row, h1_row = filts
    else:
        raise ValueError("Unknown form for input filts")
    low, highs = AFB2D.apply(x, h0_row, h1_row, h0_col, h1_col, mode_to_int(mode))
    n, c = low.shape[:2]
    return torch.cat([low[:, :, None], highs], dim=2).reshape(n, 4 * c, low.shape[-2], low.shape[-1])


def sfb2d(ll, lh, hl, hh, filts, mode='zero'):
    """Function-level synthesis (reference dwt/lowlevel.py:600-644)."""
    tensorize = [not isinstance(f, torch.Tensor) for f in filts]
    if len(filts) == 2:
        g0, g1 = filts
        if True in tensorize:
            g0_col, g1_col, g0_row, g1_row = prep_filt_sfb2d(g0, g1, device=ll.device)
        else:
            g0_col, g0_row, g1_col, g1_row = g0, g0.transpose(2, 3), g1, g1.transpose(2, 3)
    elif len(filts) == 4:
        if True in tensorize:
            g0_col, g1_col, g0_row, g1_row = prep_filt_sfb2d(*filts, device=ll.device)
        else:
            g0_col, g1_col, g0_row, g1_row = filts
    else:
        raise ValueError("Unknown form for input filts")
    highs = torch.stack([lh, hl, hh], dim=2)
    return SFB2D.apply(ll, highs, g0_row, g1_row, g0_col, g1_col, mode_to_int(mode))


# ---- the 2-D wavelet packet transform: every sub-band is split again (csrc/wl_wpt2d.h) ---------------------------------
# A level takes (N, C, H, W) to the packed block (N, C, 4, Kh, Kw), band s = 2 b_W + b_H = AFB2D's (low, highs) side by side; the
# next level reads it as (N, 4C, Kh, Kw) - a view - so the band index of a J-level tree is the base-4 number of its path, level 1
# first.
def _wpt_analysis(x, banks, mode, nlev=1):
    """`nlev` (1 or 2) packet analysis levels, banks = (h0_row, h1_row, h0_col, h1_col) as AFB2D takes them.  One level: one launch
    of the packed-band kernel, or - where it declines - ops.afb2d with the four bands copied into the packed tensor.  Two levels:
    one launch of the two-level kernel where ops.WPT_FUSED allows and the launcher takes it, else level by level."""
    if nlev == 2:
        y = ops.wpt2d_afb(x, banks[0], banks[1], banks[2], banks[3], mode, nlev=2) if ops.WPT_FUSED else None
        if y is None:
            N, C = x.shape[:2]
            y = _wpt_analysis(x, banks, mode)
            y = _wpt_analysis(y.view(N, 4 * C, y.shape[-2], y.shape[-1]), banks, mode)
            y = y.view(N, C, 16, y.shape[-2], y.shape[-1])
        return y
    y = ops.wpt2d_afb(x, banks[0], banks[1], banks[2], banks[3], mode)
    if y is None:
        ll, highs = ops.afb2d(x, banks[0], banks[1], banks[2], banks[3], mode)
        y = torch.empty(tuple(ll.shape[:2]) + (4,) + tuple(ll.shape[2:]), dtype=ll.dtype, device=ll.device)
        y[:, :, 0].copy_(ll)
        y[:, :, 1:].copy_(highs)
    return y


def _wpt_synthesis(y, banks, mode, out_hw=None, nlev=1):
    """`nlev` (1 or 2) packet synthesis levels of y (N, C, 4**nlev, Kh, Kw), the result cropped to out_hw if given (two levels: the
    level in between to the size whose analysis out_hw has): the mirror image of _wpt_analysis, ops.sfb2d on the bands sliced
    out of the packed tensor where a one-level launch declines."""
    if y.dim() != 5 or y.shape[2] != 4 ** nlev:
        raise ValueError('%d packet level(s) take (N, C, %d, H, W) coefficients, not %s' % (nlev, 4 ** nlev, tuple(y.shape)))
    if nlev == 2:
        x = ops.wpt2d_sfb(y, banks[0], banks[1], banks[2], banks[3], mode, out_hw=out_hw, nlev=2) if ops.WPT_FUSED else None
        if x is None:
            N, C = y.shape[:2]
            mid = None
            if out_hw is not None:
                mid = (ops.coeff_len(out_hw[0], banks[2].numel(), mode), ops.coeff_len(out_hw[1], banks[0].numel(), mode))
            x = _wpt_synthesis(y.reshape(N, 4 * C, 4, y.shape[-2], y.shape[-1]), banks, mode, out_hw=mid)
            x = _wpt_synthesis(x.view(N, C, 4, x.shape[-2], x.shape[-1]), banks, mode, out_hw=out_hw)
        return x
    x = ops.wpt2d_sfb(y, banks[0], banks[1], banks[2], banks[3], mode, out_hw=out_hw)
    if x is None:
        x = ops.sfb2d(y[:, :, 0], y[:, :, 1:], banks[0], banks[1], banks[2], banks[3], mode, out_hw=out_hw)
    return x


class AFBWPT2D(Function):
    """One or two levels of 2-D packet analysis.  ``AFBWPT2D.apply(x, h0_row, h1_row, h0_col, h1_col, mode_int, nlev) ->
    y (N,C,4**nlev,H',W')``; one level = AFB2D's (low, highs) as one packed block.  Backward = the packet synthesis with the same
    stored taps, every level cropped to its input size (the reference's rule for AFB2D.backward, dwt/lowlevel.py:350-365, quirk Q9)."""

    @staticmethod
    def forward(ctx, x, h0_row, h1_row, h0_col, h1_col, mode, nlev=1):
        _check_bank_mode(mode)
        ctx.save_for_backward(h0_row, h1_row, h0_col, h1_col)
        ctx.shape = tuple(x.shape[-2:])
        ctx.mode = mode
        ctx.nlev = nlev
        return _wpt_analysis(x, (h0_row, h1_row, h0_col, h1_col), mode, nlev)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _wpt_synthesis(dy, ctx.saved_tensors, ctx.mode, out_hw=ctx.shape, nlev=ctx.nlev)
        return dx, None, None, None, None, None, None


class SFBWPT2D(Function):
    """One or two levels of 2-D packet synthesis.  ``SFBWPT2D.apply(y (N,C,4**nlev,H',W'), g0_row, g1_row, g0_col, g1_col, mode_int,
    out_hw, nlev) -> x``, out_hw = (H, W) to crop to or None.  Backward = the packet analysis with the stored synthesis taps of dy
    at the size it has (the reference's SFB2D.backward, dwt/lowlevel.py:683-694)."""

    @staticmethod
    def forward(ctx, y, g0_row, g1_row, g0_col, g1_col, mode, out_hw, nlev=1):
        _check_bank_mode(mode)
        ctx.save_for_backward(g0_row, g1_row, g0_col, g1_col)
        ctx.mode = mode
        ctx.nlev = nlev
        return _wpt_synthesis(y, (g0_row, g1_row, g0_col, g1_col), mode, out_hw=out_hw, nlev=nlev)

    @staticmethod
    @once_differentiable
    def backward(ctx, dx):
        dy = None
        if ctx.needs_input_grad[0]:
            dy = _wpt_analysis(dx, ctx.saved_tensors, ctx.mode, ctx.nlev)
        return dy, None, None, None, None, None, None, None


def _filts2d(filts, prep, device):
    """(f0_col, f1_col, f0_row, f1_row) of a 2- or 4-tuple of arrays (prepared here) or prepared tensors, as afb2d / sfb2d read it."""
    if len(filts) not in (2, 4):
        raise ValueError("Unknown form for input filts")
    if any(not isinstance(f, torch.Tensor) for f in filts):
        return prep(*filts, device=device)
    if len(filts) == 2:
        f0, f1 = filts
        return f0, f1, f0.transpose(2, 3), f1.transpose(2, 3)
    return tuple(filts)


def wpt2d_level(x, filts, mode='zero'):
    """Function-level packet analysis of x (N, C, H, W): ``filts`` as afb2d takes them (the *col* pair filters along H).
    Returns (N, C, 4, H', W'), band s = 2 b_W + b_H."""
    if x.dim() != 4:
        raise ValueError('a packet level takes (N, C, H, W) tensors, not %d-D ones' % x.dim())
    h0_col, h1_col, h0_row, h1_row = _filts2d(filts, prep_filt_afb2d, x.device)
    return AFBWPT2D.apply(x, h0_row, h1_row, h0_col, h1_col, mode_to_int(mode))


def iwpt2d_level(y, filts, mode='zero', out_hw=None):
    """Function-level packet synthesis, the inverse of wpt2d_level: y (N, C, 4, H', W') -> (N, C, H, W), the natural size of a
    synthesis level or out_hw = (H, W) - a size whose analysis has H' x W' coefficients."""
    g0_col, g1_col, g0_row, g1_row = _filts2d(filts, prep_filt_sfb2d, y.device)
    m = mode_to_int(mode)
    if out_hw is not None:
        out_hw = (int(out_hw[0]), int(out_hw[1]))
        Ls = (g0_col.numel(), g0_row.numel())
        if y.dim() == 5 and tuple(ops.coeff_len(n, L, m) for n, L in zip(out_hw, Ls)) != tuple(y.shape[-2:]):
            raise ValueError('out_hw %s has no %d x %d coefficients' % (out_hw, y.shape[-2], y.shape[-1]))
    return SFBWPT2D.apply(y, g0_row, g1_row, g0_col, g1_col, m, out_hw)


# ---- the 1-D wavelet packet transform along the last axis (csrc/wl_wpt1d.h) ---------------------------------------------
# `nlev` levels take (N, C, n) to the packed block (N, C, 2**nlev, n_nlev), band b = sum_j s_j 2**(nlev-j) (s_j = 1: the highpass
# of level j); the next chunk of levels reads it as (N, 2**nlev C, n_nlev) - a view - so the band index of a J-level tree is the
# binary number of its path, level 1 first.  Periodization with every level even and at least as long as the filter, even
# L <= 20, not float64: one launch of the wave-tile kernels per (up to) three levels; everything else level by level on
# ops.afb1d / ops.sfb1d with the band axis folded into the channels, with the same answer.
def _wpt1d_analysis(x, h0, h1, mode, nlev):
    """`nlev` (1..3) packet analysis levels of x (N, C, n), no autograd -> (N, C, 2**nlev, n_nlev)."""
    y = ops.wpt1d_afb(x, h0, h1, mode, nlev) if ops.WPT1D_FUSED else None
    if y is not None:
        return y
    N, C = x.shape[:2]
    y = x
    for j in range(nlev):
        lo, hi = ops.afb1d(y, h0, h1, mode, 2)
        y = torch.stack([lo, hi], 2).view(N, C << (j + 1), lo.shape[-1])         # channel c 2^j + b -> c 2^(j+1) + 2b + s
    return y.view(N, C, 1 << nlev, y.shape[-1])


def _wpt1d_synthesis(y, g0, g1, mode, nlev, out_len=None):
    """`nlev` (1..3) packet synthesis levels of y (N, C, 2**nlev, m) -> (N, C, n): every level its natural length (2K,
    or 2K - L + 2 outside periodization), or - out_len given - the lengths the analysis of out_len samples has on its way down."""
    if y.dim() != 4 or y.shape[2] != 1 << nlev:
        raise ValueError('%d packet level(s) take (N, C, %d, n) coefficients, not %s' % (nlev, 1 << nlev, tuple(y.shape)))
    N, C, _, m = y.shape
    x = None
    if ops.WPT1D_FUSED and out_len in (None, m << nlev):
        x = ops.wpt1d_sfb(y, g0, g1, mode, nlev)
    if x is not None:
        return x
    lens = [None] * nlev
    if out_len is not None:
        lens[0] = out_len
        for j in range(1, nlev):
            lens[j] = ops.coeff_len(lens[j - 1], g0.numel(), mode)
    for j in range(nlev, 0, -1):
        y = y.reshape(N, C << (j - 1), 2, y.shape[-1])
        y = ops.sfb1d(y[:, :, 0], y[:, :, 1], g0, g1, mode, 2, out_len=lens[j - 1])
    return y


class AFBWPT1D(Function):
    """One to three levels of 1-D packet analysis.  ``AFBWPT1D.apply(x, h0, h1, mode_int, nlev) -> y (N,C,2**nlev,n')``; one level
    = AFB1D's (x0, x1) as one packed block.  Backward = the packet synthesis with the same stored taps, every level cropped to
    its input length (the reference's rule for AFB1D.backward, dwt/lowlevel.py:409-424)."""

    @staticmethod
    def forward(ctx, x, h0, h1, mode, nlev=1):
        _check_bank_mode(mode)
        ctx.save_for_backward(h0, h1)
        ctx.geom = (x.shape[-1], mode, nlev)
        return _wpt1d_analysis(x, h0, h1, mode, nlev)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dx = None
        if ctx.needs_input_grad[0]:
            h0, h1 = ctx.saved_tensors
            n, mode, nlev = ctx.geom
            dx = _wpt1d_synthesis(dy, h0, h1, mode, nlev, out_len=n)
        return dx, None, None, None, None


class SFBWPT1D(Function):
    """One to three levels of 1-D packet synthesis.  ``SFBWPT1D.apply(y (N,C,2**nlev,n'), g0, g1, mode_int, out_len, nlev) -> x``,
    out_len = the length to crop to or None.  Backward = the packet analysis with the stored synthesis taps of dx at the length
    it has (the reference's SFB1D.backward, dwt/lowlevel.py:729-743)."""

    @staticmethod
    def forward(ctx, y, g0, g1, mode, out_len, nlev=1):
        _check_bank_mode(mode)
        ctx.save_for_backward(g0, g1)
        ctx.geom = (mode, nlev)
        return _wpt1d_synthesis(y, g0, g1, mode, nlev, out_len=out_len)

    @staticmethod
    @once_differentiable
    def backward(ctx, dx):
        dy = None
        if ctx.needs_input_grad[0]:
            g0, g1 = ctx.saved_tensors
            dy = _wpt1d_analysis(dx, g0, g1, ctx.geom[0], ctx.geom[1])
        return dy, None, None, None, None, None


def wpt1d_level(x, h0, h1, mode='zero'):
    """Function-level packet analysis of x (N, C, n) along n: (N, C, 2, n'), band 0 = lowpass.  Array-like filters are the
    pywt-ordered ones (reversed here, as afb1d does); tensors are taken as prepared."""
    if x.dim() != 3:
        raise ValueError('a 1-D packet level takes (N, C, n) tensors, not %d-D ones' % x.dim())
    return AFBWPT1D.apply(x, _as_taps(h0, x), _as_taps(h1, x), mode_to_int(mode))


def iwpt1d_level(y, g0, g1, mode='zero', out_len=None):
    """Function-level packet synthesis, the inverse of wpt1d_level: y (N, C, 2, n') -> (N, C, n), the natural length of a
    synthesis level or out_len - a length whose analysis has n' coefficients.  Array-like filters are used as given (sfb1d)."""
    def prep(g):
        return g if isinstance(g, torch.Tensor) else torch.tensor(np.copy(np.array(g, dtype=np.float64).ravel()),
                                                                  dtype=torch.float, device=y.device)
    g0, g1 = prep(g0), prep(g1)
    m = mode_to_int(mode)
    if out_len is not None:
        out_len = int(out_len)
        if y.dim() == 4 and ops.coeff_len(out_len, g0.numel(), m) != y.shape[-1]:
            raise ValueError('out_len %d has no %d coefficients' % (out_len, y.shape[-1]))
    return SFBWPT1D.apply(y, g0, g1, m, out_len)


# ---- the 3-D DWT: the 2-D engine on the N*C*D planes, then one depth level (csrc/wl_dwt3d.h) -------------------------
# Sub-band s = 4 b_D + 2 b_W + b_H (b = 1: highpass) of a level: s = 0 is the low-pass, band s sits at yh[:, :, s - 1].  The 2-D
# level's (ll, lh, hl, hh) = b_D-lowpass bands 0..3, so its dense outputs are the depth kernel's four sources as they are.
def _depth_analysis(ll, highs, C, h0, h1, mode, chunks=0):
    """ll (N, C*D, H', W') and highs (N, C*D, 3, H', W') of a 2-D level on the planes of a volume -> yl (N, C, D', H', W'),
    yh (N, C, 7, D', H', W'): one launch of the depth analysis kernel that writes the final layout, or - where it declines -
    ops.afb1d along the depth axis per band."""
    N, CD, Kh, Kw = ll.shape
    D = CD // C
    Kd = ops.coeff_len(D, h0.numel(), mode)
    ll = ll.contiguous()                  # (dense already, as the 2-D level leaves them; a cotangent may be any view)
    highs = highs.contiguous().view(N, C, D, 3, Kh, Kw)
    srcs = [ll.view(N, C, D, Kh, Kw)] + [highs[:, :, :, b] for b in range(3)]
    yl = torch.empty((N, C, Kd, Kh, Kw), dtype=ll.dtype, device=ll.device)
    yh = torch.empty((N, C, 7, Kd, Kh, Kw), dtype=ll.dtype, device=ll.device)
    los = [yl] + [yh[:, :, b] for b in range(3)]
    his = [yh[:, :, 3 + b] for b in range(4)]
    if ops.afb_depth(srcs, h0, h1, mode, chunks=chunks, dim=2, out=(los, his)) is None:
        for src, lo, hi in zip(srcs, los, his):
            a, b = ops.afb1d(src, h0, h1, mode, 2)
            lo.copy_(a)
            hi.copy_(b)
    return yl, yh


def _depth_synthesis(yl, yh, g0, g1, mode, out_len=None, chunks=0):
    """yl (N, C, K, H', W') and yh (N, C, 7, K, H', W') or None (zeros) -> the dense ll (N, C*D, H', W') and highs
    (N, C*D, 3, H', W') (None without yh) that the 2-D synthesis takes, D = ops.synth_len(K) or out_len: one launch of the depth
    synthesis kernel, or - where it declines - ops.sfb1d along the depth axis per band pair."""
    N, C, K, Kh, Kw = yl.shape
    D = ops.synth_len(K, g0.numel(), mode, out_len)
    ll = torch.empty((N, C * D, Kh, Kw), dtype=yl.dtype, device=yl.device)
    ys = [ll.view(N, C, D, Kh, Kw)]
    los, his, highs = [yl], [None], None
    if yh is not None:
        if yh.dtype != yl.dtype:
            yh = yh.to(yl.dtype)
        if tuple(yh.shape) != (N, C, 7, K, Kh, Kw):
            raise ValueError('yh %s does not match yl %s' % (tuple(yh.shape), tuple(yl.shape)))
        highs = torch.empty((N, C * D, 3, Kh, Kw), dtype=yl.dtype, device=yl.device)
        hv = highs.view(N, C, D, 3, Kh, Kw)
        ys += [hv[:, :, :, b] for b in range(3)]
        los += [yh[:, :, b] for b in range(3)]
        his = [yh[:, :, 3 + b] for b in range(4)]
    if ops.sfb_depth(los, his, g0, g1, mode, out_len=out_len, chunks=chunks, dim=2, out=ys) is None:
        for lo, hi, y in zip(los, his, ys):
            y.copy_(ops.sfb1d(lo, hi, g0, g1, mode, 2, out_len=out_len))
    return ll, highs


class AFBDepth(Function):
    """The depth level of a 3-D analysis: ``AFBDepth.apply(ll, highs, h0_dep, h1_dep, mode_int, C) -> (yl, yh)`` takes the 2-D
    level of the N*C*D planes (ll (N, C*D, H', W'), highs (N, C*D, 3, H', W')) to yl (N, C, D', H', W') and yh
    (N, C, 7, D', H', W').  Backward = the depth synthesis with the same stored taps, cropped to the input depth: the reference's
    convention for AFB2D.backward (dwt/lowlevel.py:350-365, quirk Q9) applied to the third axis, so that the three axes agree -
    the exact adjoint in 'zero' mode."""

    @staticmethod
    def forward(ctx, ll, highs, h0, h1, mode, C):
        _check_bank_mode(mode)
        ctx.save_for_backward(h0, h1)
        ctx.mode = mode
        ctx.depth = ll.shape[1] // C
        return _depth_analysis(ll, highs, C, h0, h1, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, dyl, dyh):
        dll = dhighs = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            h0, h1 = ctx.saved_tensors
            dll, dhighs = _depth_synthesis(dyl, dyh, h0, h1, ctx.mode, out_len=ctx.depth)
        return dll, dhighs, None, None, None, None


class SFBDepth(Function):
    """The depth level of a 3-D synthesis: ``SFBDepth.apply(yl, yh, g0_dep, g1_dep, mode_int) -> (ll, highs)``, yh None = zeros
    (highs is then None too).  Backward = the depth analysis with the stored synthesis taps (the reference's SFB2D.backward,
    dwt/lowlevel.py:683-694, on the third axis)."""

    @staticmethod
    def forward(ctx, yl, yh, g0, g1, mode):
        _check_bank_mode(mode)
        ctx.save_for_backward(g0, g1)
        ctx.mode = mode
        ctx.has_highs = yh is not None
        ctx.C = yl.shape[1]
        ll, highs = _depth_synthesis(yl, yh, g0, g1, mode)
        if highs is None:
            return ll
        return ll, highs

    @staticmethod
    @once_differentiable
    def backward(ctx, dll, dhighs=None):
        dyl = dyh = None
        if ctx.needs_input_grad[0] or (ctx.has_highs and ctx.needs_input_grad[1]):
            g0, g1 = ctx.saved_tensors
            if ctx.has_highs:
                dyl, dyh = _depth_analysis(dll, dhighs, ctx.C, g0, g1, ctx.mode)
            else:
                N, CD, Kh, Kw = dll.shape
                dyl = ops.afb1d(dll.reshape(N, ctx.C, CD // ctx.C, Kh, Kw), g0, g1, ctx.mode, 2)[0]
        return dyl, dyh, None, None, None


def _afb3d_level(x, dep, banks, mode):
    """One 3-D analysis level: x (N, C, D, H, W) -> yl, yh; dep = (h0_dep, h1_dep), banks = the four 2-D banks in AFB2DMulti's
    argument order (the first pair filters along W)."""
    if x.dim() != 5:
        raise ValueError('the 3-D transform takes (N, C, D, H, W) tensors, not %d-D ones' % x.dim())
    N, C, D, H, W = x.shape
    outs = AFB2DMulti.apply(x.reshape(N, C * D, H, W), banks[0], banks[1], banks[2], banks[3], mode, 1)
    return AFBDepth.apply(outs[0], outs[1], dep[0], dep[1], mode, C)


def _sfb3d_level(yl, yh, dep, banks, mode):
    """One 3-D synthesis level (yh None = zeros): the 'unpad' of a low-pass one sample longer than the highs along any axis, the
    depth synthesis, the 2-D synthesis of the planes."""
    if yl.dim() != 5:
        raise ValueError('the 3-D transform takes (N, C, D, H, W) tensors, not %d-D ones' % yl.dim())
    if yh is not None:
        for ax in (-3, -2, -1):
            if yl.shape[ax] > yh.shape[ax]:
                yl = yl.narrow(ax, 0, yl.shape[ax] - 1)
    N, C = yl.shape[:2]
    res = SFBDepth.apply(yl, yh, dep[0], dep[1], mode)
    ll, highs = res if yh is not None else (res, None)
    y = SFB2DMulti.apply(ll, banks[0], banks[1], banks[2], banks[3], mode, highs)
    return y.reshape(N, C, ll.shape[1] // C, y.shape[-2], y.shape[-1])


def prep_filt_afb3d(h0_dep, h1_dep, h0_col=None, h1_col=None, h0_row=None, h1_row=None, device=None):
    """(h0_dep, h1_dep, h0_col, h1_col, h0_row, h1_row): the depth pair stored reversed with shape (1,1,L,1,1), the other four as
    prep_filt_afb2d makes them (one pair given: the same wavelet on the three axes)."""
    d0, d1 = prep_filt_afb1d(h0_dep, h1_dep, device)
    if h0_col is None:
        h0_col, h1_col = h0_dep, h1_dep
    return (d0.reshape(1, 1, -1, 1, 1), d1.reshape(1, 1, -1, 1, 1)) + prep_filt_afb2d(h0_col, h1_col, h0_row, h1_row, device)


def prep_filt_sfb3d(g0_dep, g1_dep, g0_col=None, g1_col=None, g0_row=None, g1_row=None, device=None):
    """(g0_dep, g1_dep, g0_col, g1_col, g0_row, g1_row): synthesis taps as given, shapes as prep_filt_afb3d."""
    d0, d1 = prep_filt_sfb1d(g0_dep, g1_dep, device)
    if g0_col is None:
        g0_col, g1_col = g0_dep, g1_dep
    return (d0.reshape(1, 1, -1, 1, 1), d1.reshape(1, 1, -1, 1, 1)) + prep_filt_sfb2d(g0_col, g1_col, g0_row, g1_row, device)


def _filts3d(filts, prep, device):
    if len(filts) not in (2, 6):
        raise ValueError("Unknown form for input filts")
    if any(not isinstance(f, torch.Tensor) for f in filts):
        return prep(*filts, device=device)
    if len(filts) == 2:
        f0, f1 = (f.reshape(-1) for f in filts)
        return (f0.reshape(1, 1, -1, 1, 1), f1.reshape(1, 1, -1, 1, 1)) + _to_2d(f0, f1, f0, f1)
    return tuple(filts)


def afb3d(x, filts, mode='zero'):
    """Function-level 3-D analysis of x (N, C, D, H, W): ``filts`` = (h0, h1) for the three axes or (h0_dep, h1_dep, h0_col,
    h1_col, h0_row, h1_row) - arrays in pywt order (reversed here) or prepared tensors; as in afb2d the *col* pair filters
    along H, the *row* pair along W.  Returns (yl (N, C, D', H', W'), yh (N, C, 7, D', H', W')), band s = 4 b_D + 2 b_W + b_H at
    yh[:, :, s - 1]."""
    h0_dep, h1_dep, h0_col, h1_col, h0_row, h1_row = _filts3d(filts, prep_filt_afb3d, x.device)
    return _afb3d_level(x, (h0_dep, h1_dep), (h0_row, h1_row, h0_col, h1_col), mode_to_int(mode))


def sfb3d(ll, highs, filts, mode='zero'):
    """Function-level 3-D synthesis, the inverse of afb3d: ll (N, C, K, H', W'), highs (N, C, 7, K, H', W') or None."""
    g0_dep, g1_dep, g0_col, g1_col, g0_row, g1_row = _filts3d(filts, prep_filt_sfb3d, ll.device)
    return _sfb3d_level(ll, highs, (g0_dep, g1_dep), (g0_row, g1_row, g0_col, g1_col), mode_to_int(mode))


# ---- filter preparation (buffer shapes/orders are part of the state_dict contract) -----------------
def _vec(h, reverse, device):
    h = np.array(h, dtype=np.float64).ravel()
    if reverse:
        h = h[::-1].copy()
    return torch.tensor(h, device=device, dtype=torch.get_default_dtype())


def prep_filt_afb1d(h0, h1, device=None):
    """Analysis taps are stored reversed, shape (1,1,L) (reference dwt/lowlevel.py:956-975)."""
    return _vec(h0, True, device).reshape(1, 1, -1), _vec(h1, True, device).reshape(1, 1, -1)


def prep_filt_sfb1d(g0, g1, device=None):
    """Synthesis taps are stored as given (reference dwt/lowlevel.py:902-922)."""
    return _vec(g0, False, device).reshape(1, 1, -1), _vec(g1, False, device).reshape(1, 1, -1)


def _to_2d(col0, col1, row0, row1):
    return (col0.reshape(1, 1, -1, 1), col1.reshape(1, 1, -1, 1),
            row0.reshape(1, 1, 1, -1), row1.reshape(1, 1, 1, -1))


def prep_filt_afb2d(h0_col, h1_col, h0_row=None, h1_row=None, device=None):
    """(h0_col, h1_col, h0_row, h1_row) with shapes (1,1,L,1) / (1,1,1,L)
    (reference dwt/lowlevel.py:925-953)."""
    c0, c1 = prep_filt_afb1d(h0_col, h1_col, device)
    r0, r1 = (c0, c1) if h0_row is None else prep_filt_afb1d(h0_row, h1_row, device)
    return _to_2d(c0, c1, r0, r1)


def prep_filt_sfb2d(g0_col, g1_col, g0_row=None, g1_row=None, device=None):
    """(g0_col, g1_col, g0_row, g1_row) (reference dwt/lowlevel.py:870-899)."""
    c0, c1 = prep_filt_sfb1d(g0_col, g1_col, device)
    r0, r1 = (c0, c1) if g0_row is None else prep_filt_sfb1d(g0_row, g1_row, device)
    return _to_2d(c0, c1, r0, r1)
