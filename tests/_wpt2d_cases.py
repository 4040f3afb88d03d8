"""Shared checks of the 2-D wavelet packet transform (WPT2DForward / WPT2DInverse, dwt.lowlevel.wpt2d_level / iwpt2d_level,
ops.wpt2d_afb / ops.wpt2d_sfb and the packed-band kernels of csrc/wl_wpt2d.h), run by the emulator (CPU) and the GPU test modules.

The expected answer is a numpy composition of the pinned per-axis oracle: per level ``wo.afb1d`` along W, then along H, the four
bands stacked as s = 2 b_W + b_H and reshaped to planes; ``wo.sfb1d`` along H, then W for the inverse.  Gradients follow the
reference's rule for AFB2D / SFB2D (quirk Q9, oracle/wavelet_oracle.py) level by level: the backward of an analysis level is the
packet synthesis with the ANALYSIS taps cropped to the level's input, the backward of a synthesis level the packet analysis with
the SYNTHESIS taps of the cotangent at the size it has.

Tolerances (tests/_dwt3d_cases.close): float32 1e-5 |ref|max; float16 3e-3 max(1, |ref|max); float64 1e-12 max(1, |ref|max);
bfloat16 3e-2 |ref|max (a packet chain rounds once per level) - the 2-byte types against the oracle on the rounded inputs with the
float32 taps the modules hold."""
import contextlib

import numpy as np
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters, ops
from pytorch_wavelets_amd.dwt import lowlevel as dwl

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
MODES = ('zero', 'symmetric', 'reflect', 'periodization', 'periodic')
TNAME = {F32: 'float', F16: '_Float16', BF16: '__bf16'}


def npy(t):
    return t.detach().cpu().double().numpy()


def taps(wave, syn=False, f32=False):
    """(lo, hi) as the oracle takes them: the stored analysis taps (reversed) or the synthesis taps; f32: rounded to float32."""
    t = filters.dwt_synthesis_taps(wave) if syn else filters.dwt_analysis_taps(wave)
    t = tuple(np.asarray(v, dtype=np.float64) for v in t)
    return tuple(v.astype(np.float32).astype(np.float64) for v in t) if f32 else t


def level_ref(x, h, mode):
    """One packet analysis level in numpy: x (N,C,H,W) -> (N,C,4,H',W'), band s = 2 b_W + b_H."""
    out = [None] * 4
    for bw, xw in enumerate(wo.afb1d(x, h[0], h[1], mode, axis=3)):
        for bh, xh in enumerate(wo.afb1d(xw, h[0], h[1], mode, axis=2)):
            out[2 * bw + bh] = xh
    return np.stack(out, axis=2)


def unlevel_ref(y, g, mode, crop=None):
    """One packet synthesis level in numpy: y (N,C,4,K,K') -> (N,C,H,W); crop = (H, W) or None."""
    lo = wo.sfb1d(y[:, :, 0], y[:, :, 1], g[0], g[1], mode, axis=2)
    hi = wo.sfb1d(y[:, :, 2], y[:, :, 3], g[0], g[1], mode, axis=2)
    x = wo.sfb1d(lo, hi, g[0], g[1], mode, axis=3)
    return x if crop is None else x[:, :, :crop[0], :crop[1]]


def fwd_ref(x, J, h, mode):
    x = np.asarray(x)
    N, C = x.shape[:2]
    y = x
    for _ in range(J):
        b = level_ref(y, h, mode)
        y = b.reshape(N, -1, b.shape[-2], b.shape[-1])
    return y.reshape(N, C, 4 ** J, y.shape[-2], y.shape[-1])


def inv_ref(y, g, mode, sizes=None):
    """sizes = [(H_0, W_0), .., (H_J, W_J)] of the forward (every level cropped) or None (natural sizes)."""
    y = np.asarray(y)
    N, C, B = y.shape[:3]
    J = int(round(np.log(B) / np.log(4)))
    for j in range(J, 0, -1):
        y = y.reshape(N, -1, 4, y.shape[-2], y.shape[-1])
        y = unlevel_ref(y, g, mode, None if sizes is None else sizes[j - 1])
    return y.reshape(N, C, y.shape[-2], y.shape[-1])


def level_sizes(hw, J, L, mode):
    m = dwl.mode_to_int(mode)
    sizes = [tuple(hw)]
    for _ in range(J):
        sizes.append(tuple(ops.coeff_len(n, L, m) for n in sizes[-1]))
    return sizes


def close(a, ref, dtype, what=''):
    a = npy(a) if isinstance(a, torch.Tensor) else a
    assert tuple(a.shape) == tuple(ref.shape), (what, a.shape, ref.shape)
    err, top = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    bound = {F64: 1e-12 * max(1.0, top), F32: 1e-5 * top, F16: 3e-3 * max(1.0, top), BF16: 3e-2 * top}[dtype]
    print('%s %s: max err %.3e, bound %.3e' % (what, dtype, err, bound))
    assert err <= bound, (what, err, bound)


def modules(dev, wave, J, mode, dtype=F32):
    """(WPT2DForward, WPT2DInverse) whose buffers are float64 for float64 data, float32 otherwise."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64 if dtype == F64 else F32)
    try:
        return pw.WPT2DForward(J=J, wave=wave, mode=mode).to(dev), pw.WPT2DInverse(wave=wave, mode=mode).to(dev)
    finally:
        torch.set_default_dtype(prev)


def rand(shape, dtype, dev, seed):
    return torch.tensor(np.random.RandomState(seed).randn(*shape)).to(dtype).to(dev)


@contextlib.contextmanager
def fused(flag):
    """ops.WPT_FUSED = flag inside the block: two packet levels per launch where the kernels take them, or never."""
    prev = ops.WPT_FUSED
    ops.WPT_FUSED = flag
    try:
        yield
    finally:
        ops.WPT_FUSED = prev


def names(ks):
    return [k for k in ks if not k.endswith(')')]          # (without armed fallbacks and helper launches)


def ntaps(wave):
    return len(taps(wave)[0])


# ---- 1: values and layout ----------------------------------------------------------------------------------------------
def check_forward(dev, shape, wave, J, mode, dtype=F32, seed=1):
    x = rand(shape, dtype, dev, seed)
    xfm, _ = modules(dev, wave, J, mode, dtype)
    c0 = pw.launch_count()
    y = xfm(x)
    ks = names(pw.kernels_since(c0))
    sizes = level_sizes(shape[2:], J, ntaps(wave), mode)
    assert tuple(y.shape) == tuple(shape[:2]) + (4 ** J,) + sizes[-1] and y.dtype == dtype and y.is_contiguous()
    ref = fwd_ref(npy(x), J, taps(wave, f32=dtype != F64), mode)
    close(y, ref, dtype, 'J=%d %s %s %s' % (J, wave, mode, tuple(shape)))              # (every band: the whole packed tensor)
    return x, y, ks


# ---- 2: band table -------------------------------------------------------------------------------------------------------
def check_band_table(dev, shape, wave, mode):
    x = rand(shape, F32, dev, 2)
    y1 = modules(dev, wave, 1, mode)[0](x)
    yl, yh = pw.DWTForward(J=1, wave=wave, mode=mode).to(dev)(x)
    close(y1, npy(torch.cat([yl[:, :, None], yh[0]], 2)), F32, 'J=1 against DWTForward')
    y2 = modules(dev, wave, 2, mode)[0](x)
    N, C = shape[:2]
    sub = y2.view(N, C, 4, 4, y2.shape[-2], y2.shape[-1])
    for s in range(4):
        close(sub[:, :, s], npy(modules(dev, wave, 1, mode)[0](y1[:, :, s])), F32, 'subtree under band %d' % s)


def check_freq_order(dev, J=2, n=64, wave='db4'):
    """A separable cosine at the centre of frequency slot (fh, fw) puts its energy maximum into exactly that band."""
    idx = pw.wpt2d_freq_order(J)
    assert sorted(idx) == list(range(4 ** J))
    xfm, _ = modules(dev, wave, J, 'periodization')
    t = np.arange(n)
    slots = [(fh, fw) for fh in range(2 ** J) for fw in range(2 ** J)]
    imgs = np.stack([np.outer(np.cos((fh + 0.5) * np.pi / 2 ** J * t), np.cos((fw + 0.5) * np.pi / 2 ** J * t)) for fh, fw in slots])
    y = xfm(torch.tensor(imgs[:, None], dtype=F32).to(dev))                     # (slots, 1, 4**J, n', n')
    energy = npy(y)[:, 0][:, idx].reshape(len(slots), 2 ** J, 2 ** J, -1)
    energy = (energy ** 2).sum(-1)
    for i, (fh, fw) in enumerate(slots):
        assert np.unravel_index(np.argmax(energy[i]), energy[i].shape) == (fh, fw), (fh, fw, energy[i])


# ---- 3: the new kernels really ran -----------------------------------------------------------------------------------------
def check_kernels_ran(dev, mode='symmetric', shape=(1, 2, 37, 61), J=3):
    """One launch of the packed-band kernel per level - forward, inverse and both backwards - and nothing else (outside the
    two-level envelope: check_two_level_sequence has the sequences inside it)."""
    xfm, ifm = modules(dev, 'db4', J, mode)
    x = rand(shape, F32, dev, 3).requires_grad_(True)
    c0 = pw.launch_count()
    y = xfm(x)
    assert names(pw.kernels_since(c0)) == ['WlWptAfb<float, 8, 1>'] * J, pw.kernels_since(c0)
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(y, x, torch.ones_like(y))
    assert names(pw.kernels_since(c0)) == ['WlWptSfb<float, 8, 1>'] * J, pw.kernels_since(c0)
    for size in (shape[2:], None):
        yc = y.detach().clone().requires_grad_(True)
        c0 = pw.launch_count()
        rec = ifm(yc, size=size)
        assert names(pw.kernels_since(c0)) == ['WlWptSfb<float, 8, 1>'] * J, pw.kernels_since(c0)
        c0 = pw.launch_count()
        torch.autograd.grad(rec, yc, torch.ones_like(rec))
        assert names(pw.kernels_since(c0)) == ['WlWptAfb<float, 8, 1>'] * J, pw.kernels_since(c0)


def check_float64_generic(dev):
    """float64: ops.afb2d / ops.sfb2d per level on the generic kernels, and still the oracle's numbers."""
    x, y, ks = check_forward(dev, (1, 2, 13, 17), 'db4', 2, 'symmetric', F64)
    assert len(ks) >= 2 and not any('Wpt' in k for k in ks) and any('<double>' in k for k in ks), ks
    _, ifm = modules(dev, 'db4', 2, 'symmetric', F64)
    c0 = pw.launch_count()
    rec = ifm(y, size=(13, 17))
    ks = names(pw.kernels_since(c0))
    assert not any('Wpt' in k for k in ks) and any('<double>' in k for k in ks), ks
    close(rec, inv_ref(npy(y), taps('db4', syn=True), 'symmetric', level_sizes((13, 17), 2, 8, 'symmetric')), F64, 'float64 inverse')


def check_generic_only(dev):
    """generic_only: the launchers decline, the level-by-level fallback gives the same numbers within the bound."""
    x, y, ks = check_forward(dev, (1, 2, 20, 28), 'db2', 2, 'symmetric')
    assert ks == ['WlWptAfb<float, 4, 1>'] * 2, ks
    ops.set_option('generic_only', 1)
    try:
        _, y2, ks2 = check_forward(dev, (1, 2, 20, 28), 'db2', 2, 'symmetric')
        rec = modules(dev, 'db2', 2, 'symmetric')[1](y2, size=(20, 28))
    finally:
        ops.set_option('generic_only', 0)
    assert not any('Wpt' in k for k in ks2), ks2
    close(y2, npy(y), F32, 'generic_only against the packet kernels')
    close(rec, npy(x), F32, 'generic_only round trip')


def check_declines(dev):
    """Outside the kernels' envelope - 22 taps, periodization of a plane shorter than the filter - ops returns None and the
    modules still match the oracle."""
    h = [torch.tensor(np.ascontiguousarray(v), dtype=F32, device=dev) for v in taps('db11', f32=True)]
    assert ops.wpt2d_afb(rand((1, 1, 30, 30), F32, dev, 1), h[0], h[1], h[0], h[1], 1) is None
    assert ops.wpt2d_sfb(rand((1, 1, 4, 30, 30), F32, dev, 1), h[0], h[1], h[0], h[1], 1) is None
    h = [torch.tensor(np.ascontiguousarray(v), dtype=F32, device=dev) for v in taps('db4', f32=True)]
    assert ops.wpt2d_afb(rand((1, 1, 5, 16), F32, dev, 1), h[0], h[1], h[0], h[1], 2) is None
    assert ops.wpt2d_sfb(rand((1, 1, 4, 2, 16), F32, dev, 1), h[0], h[1], h[0], h[1], 2) is None
    assert ops.wpt2d_afb(rand((1, 1, 16, 16), F32, dev, 1), h[0], h[1], h[0], h[1], 1, nlev=2) is None    # two levels: the wrap mode only
    assert ops.wpt2d_afb(rand((1, 1, 16, 16), F32, dev, 1), h[0], h[1], h[0], h[1], 2, nlev=2) is not None
    check_forward(dev, (1, 1, 30, 34), 'db11', 1, 'symmetric')
    check_inverse(dev, (1, 1, 30, 34), 'db11', 'symmetric', J=1)


def check_two_level_sequence(dev, shape=(1, 2, 72, 200), J=3):
    """Periodization, sizes multiples of 4, ops.WPT_FUSED on: J // 2 two-level launches and a single-level one when J is odd -
    forward, inverse and both backwards, the inverse's in mirrored order - with the oracle's numbers; ops.WPT_FUSED off: J
    single-level launches and the same numbers within the bound."""
    A1, A2, S1, S2 = ('WlWpt%s<float, 8, %d>' % (k, n) for k in ('Afb', 'Sfb') for n in (1, 2))
    mode = 'periodization'
    xfm, ifm = modules(dev, 'db4', J, mode)
    sizes = level_sizes(shape[2:], J, 8, mode)
    h, g = taps('db4', f32=True), taps('db4', syn=True, f32=True)
    outs = {}
    for flag, fwd, inv in ((True, [A2, A1], [S1, S2]), (False, [A1] * J, [S1] * J)):
        with fused(flag):
            x = rand(shape, F32, dev, 3).requires_grad_(True)
            c0 = pw.launch_count()
            y = xfm(x)
            assert names(pw.kernels_since(c0)) == fwd, (flag, pw.kernels_since(c0))
            close(y, fwd_ref(npy(x), J, h, mode), F32, 'forward fused=%s' % flag)
            cot = rand(tuple(y.shape), F32, dev, 4)
            c0 = pw.launch_count()
            dx, = torch.autograd.grad(y, x, cot)
            assert names(pw.kernels_since(c0)) == inv, (flag, pw.kernels_since(c0))
            close(dx, fwd_grad_ref(npy(cot), sizes, h, mode), F32, 'dx fused=%s' % flag)
            res = [y.detach(), dx]
            for size in (shape[2:], None):
                yc = y.detach().clone().requires_grad_(True)
                c0 = pw.launch_count()
                rec = ifm(yc, size=size)
                assert names(pw.kernels_since(c0)) == inv, (flag, pw.kernels_since(c0))
                close(rec, inv_ref(npy(yc), g, mode, sizes), F32, 'inverse fused=%s size=%s' % (flag, size))
                dy = rand(tuple(rec.shape), F32, dev, 5)
                c0 = pw.launch_count()
                dc, = torch.autograd.grad(rec, yc, dy)
                assert names(pw.kernels_since(c0)) == fwd, (flag, pw.kernels_since(c0))
                close(dc, inv_grad_ref(npy(dy), J, g, mode), F32, 'd(coeffs) fused=%s size=%s' % (flag, size))
                res += [rec.detach(), dc]
            outs[flag] = res
    for a, b in zip(outs[True], outs[False]):
        close(a, npy(b), F32, 'two levels per launch against level by level')


def check_two_level_low_precision(dev, dtype, shape=(2, 3, 20, 28), wave='db2'):
    L = ntaps(wave)
    with fused(True):
        x, y, ks = check_forward(dev, shape, wave, 2, 'periodization', dtype)
        assert ks == ['WlWptAfb<%s, %d, 2>' % (TNAME[dtype], L)], ks
        _, ifm = modules(dev, wave, 2, 'periodization', dtype)
        c0 = pw.launch_count()
        rec = ifm(y, size=shape[2:])
        assert names(pw.kernels_since(c0)) == ['WlWptSfb<%s, %d, 2>' % (TNAME[dtype], L)]
        close(rec, inv_ref(npy(y), taps(wave, syn=True, f32=True), 'periodization', level_sizes(shape[2:], 2, L, 'periodization')),
              dtype, 'two-level inverse')


# ---- 4: the seams of the two-level kernels -----------------------------------------------------------------------------------
def check_wrap_shapes(dev, wave, shape, mode='periodization', two_level=True):
    """J = 2 with ops.WPT_FUSED on, against the oracle and against the level-by-level route.  two_level: the kernels' envelope
    (periodization, sizes multiples of 4, at most 12 taps, level 2 no shorter than the filter) holds - one launch per
    direction; else the launcher declines and single-level launches (or, for planes shorter than the filter, the fallback) run.
    (72, 200): level-2 bands of 18 x 50 = 3 x 4 tiles of 8 x 16 with partial last tiles, 3 x 4 tiles of 32 x 64 of the image;
    (8, 12): one wrapped tile smaller than the footprint."""
    L = ntaps(wave)
    sizes = level_sizes(shape[2:], 2, L, mode)
    _, ifm = modules(dev, wave, 2, mode)
    with fused(True):
        x, y, ks = check_forward(dev, shape, wave, 2, mode)
        c0 = pw.launch_count()
        rec = ifm(y, size=shape[2:])
        ki = names(pw.kernels_since(c0))
    if two_level:
        assert ks == ['WlWptAfb<float, %d, 2>' % L] and ki == ['WlWptSfb<float, %d, 2>' % L], (ks, ki)
    else:
        assert len(ks) == 2 and len(ki) == 2 and not any(', 2>' in k for k in ks + ki), (ks, ki)
    close(rec, inv_ref(npy(y), taps(wave, syn=True, f32=True), mode, sizes), F32, 'inverse %s %s' % (wave, tuple(shape)))
    with fused(False):
        _, y1, ks1 = check_forward(dev, shape, wave, 2, mode)
        rec1 = ifm(y1, size=shape[2:])
    assert len(ks1) == 2 and not any(', 2>' in k for k in ks1), ks1
    close(y, npy(y1), F32, 'forward against level by level')
    close(rec, npy(rec1), F32, 'inverse against level by level')
    if min(n + (n & 1) for hw in sizes[:2] for n in hw) >= L - 1:     # (no level shorter than the filter: the DWT reconstructs)
        close(rec, npy(x), F32, 'round trip %s %s' % (wave, tuple(shape)))


# ---- 5: inverse ----------------------------------------------------------------------------------------------------------
def check_inverse(dev, shape, wave, mode, J=2, dtype=F32, with_size=True):
    """WPT2DInverse of random coefficients shaped like a forward's against the numpy synthesis."""
    sizes = level_sizes(shape[2:], J, ntaps(wave), mode)
    _, ifm = modules(dev, wave, J, mode, dtype)
    y = rand(tuple(shape[:2]) + (4 ** J,) + sizes[-1], dtype, dev, 12)
    rec = ifm(y, size=shape[2:] if with_size else None)
    ref = inv_ref(npy(y), taps(wave, syn=True, f32=dtype != F64), mode, sizes if with_size else None)
    if with_size:
        assert tuple(rec.shape) == tuple(shape)
    close(rec, ref, dtype, 'inverse %s %s J=%d size=%s' % (wave, mode, J, with_size))


def check_roundtrip(dev, shape, wave, mode, J=2):
    xfm, ifm = modules(dev, wave, J, mode)
    x = rand(shape, F32, dev, 20)
    close(ifm(xfm(x), size=shape[2:]), npy(x), F32, 'round trip %s %s %s' % (wave, mode, tuple(shape)))


def check_inverse_errors(dev):
    _, ifm = modules(dev, 'db2', 2, 'symmetric')
    y = rand((1, 2, 16, 7, 9), F32, dev, 21)
    for bad, size in ((y, (24, 28)), (y[:, :, :8], None), (y[:, :, :2], None)):
        try:
            ifm(bad, size=size)
        except ValueError:
            pass
        else:
            raise AssertionError('%s with size %s did not raise' % (tuple(bad.shape), size))
    assert tuple(ifm(y, size=(20, 28)).shape) == (1, 2, 20, 28)


# ---- 6: gradients --------------------------------------------------------------------------------------------------------
def fwd_grad_ref(dy, sizes, h, mode):
    return inv_ref(dy, h, mode, sizes)                      # the packet synthesis with the ANALYSIS taps, cropped level by level


def inv_grad_ref(dx, J, g, mode):
    return fwd_ref(dx, J, g, mode)                          # the packet analysis with the SYNTHESIS taps


def check_gradients(dev, shape, wave, mode, J=2, dtype=F32):
    xfm, ifm = modules(dev, wave, J, mode, dtype)
    f32 = dtype != F64
    sizes = level_sizes(shape[2:], J, ntaps(wave), mode)
    x = rand(shape, dtype, dev, 30).requires_grad_(True)
    y = xfm(x)
    cot = rand(tuple(y.shape), dtype, dev, 31)
    dx, = torch.autograd.grad(y, x, cot)
    close(dx, fwd_grad_ref(npy(cot), sizes, taps(wave, f32=f32), mode), dtype, 'dx %s %s' % (wave, mode))
    for size in (shape[2:], None):
        c = y.detach().clone().requires_grad_(True)
        rec = ifm(c, size=size)
        dy = rand(tuple(rec.shape), dtype, dev, 40)
        dc, = torch.autograd.grad(rec, c, dy)
        close(dc, inv_grad_ref(npy(dy), J, taps(wave, syn=True, f32=f32), mode), dtype, 'd(coeffs) %s %s size=%s' % (wave, mode, size))


def check_dot_product(dev, shape, wave, J=2):
    """<A x, y> = <x, A^T y> through the real modules, 'zero' mode (where the Q9 backward is the exact adjoint), float64."""
    xfm, _ = modules(dev, wave, J, 'zero', F64)
    x = rand(shape, F64, dev, 50).requires_grad_(True)
    out = xfm(x)
    y = rand(tuple(out.shape), F64, dev, 51)
    dx, = torch.autograd.grad(out, x, y)
    lhs, rhs = float((out.detach() * y).sum()), float((x.detach() * dx).sum())
    print('dot product: %.15e against %.15e' % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)


# ---- 7: float16 and bfloat16 -----------------------------------------------------------------------------------------------
def check_low_precision(dev, dtype, mode, shape=(2, 3, 20, 28), wave='db2', J=2):
    with fused(False):                                     # (the one-level kernels; check_two_level_low_precision: the two-level ones)
        _check_low_precision(dev, dtype, mode, shape, wave, J)


def _check_low_precision(dev, dtype, mode, shape, wave, J):
    x, y, ks = check_forward(dev, shape, wave, J, mode, dtype)
    assert ks == ['WlWptAfb<%s, %d, 1>' % (TNAME[dtype], ntaps(wave))] * J, ks
    xfm, ifm = modules(dev, wave, J, mode, dtype)
    sizes = level_sizes(shape[2:], J, ntaps(wave), mode)
    c0 = pw.launch_count()
    rec = ifm(y, size=shape[2:])
    assert names(pw.kernels_since(c0)) == ['WlWptSfb<%s, %d, 1>' % (TNAME[dtype], ntaps(wave))] * J
    assert rec.dtype == dtype
    close(rec, inv_ref(npy(y), taps(wave, syn=True, f32=True), mode, sizes), dtype, 'inverse %s' % mode)
    xg = x.clone().requires_grad_(True)
    out = xfm(xg)
    cot = rand(tuple(out.shape), dtype, dev, 60)
    dx, = torch.autograd.grad(out, xg, cot)
    assert dx.dtype == dtype
    close(dx, fwd_grad_ref(npy(cot), sizes, taps(wave, f32=True), mode), dtype, 'dx %s' % mode)


# ---- 7a: every compiled instantiation ------------------------------------------------------------------------------------------
GRID_WAVES = tuple('db%d' % i for i in range(1, 11))        # L = 2, 4, .., 20: one case of the dispatchers' switch each
GRID_WAVES2 = GRID_WAVES[:6]                                # the two-level kernels stop at 12 taps
GRID_DTYPES = (F32, F16, BF16)


def last_grid():
    """Workgroups of the engine's last launch."""
    return int(ops._backend().wl_last_grid())


def check_wide_instantiation(dev, wave, dtype, shape=(1, 2, 37, 61)):
    """WlWptAfb<T, L, 1> / WlWptSfb<T, L, 1> of one tap count and element type on a plane with partial last tiles in both axes
    (level 1: one plane per workgroup, the wide walk), J = 2, a mirror mode and the wrap mode; float32 also the gradients.  The
    kernel names are built from (T, L)."""
    L = ntaps(wave)
    A, Sy = ('WlWpt%s<%s, %d, 1>' % (k, TNAME[dtype], L) for k in ('Afb', 'Sfb'))
    with fused(False):
        for mode in ('symmetric', 'periodization'):
            _, _, ks = check_forward(dev, shape, wave, 2, mode, dtype)
            assert ks == [A] * 2, (mode, ks)
            c0 = pw.launch_count()
            check_inverse(dev, shape, wave, mode, J=2, dtype=dtype)
            assert names(pw.kernels_since(c0)) == [Sy] * 2, (mode, pw.kernels_since(c0))
            if dtype == F32:
                check_gradients(dev, shape, wave, mode, J=2)


def check_plane_run_instantiation(dev, wave, dtype, shape):
    """The same instantiations on a run of 8 x 8 planes, several planes per workgroup (the plane-run walk): one level, 'zero' and
    'symmetric' for every tap count, 'periodization' where the launchers take an 8 x 8 plane - the analysis up to 9 taps
    (8 >= L - 1), the synthesis of the 4 x 4 bands up to 10 (2 * 4 >= L - 2) - and their decline asserted where they do not.  A
    launch of fewer workgroups than planes (times tiles: one here) proves that planes shared a workgroup."""
    L = ntaps(wave)
    A, Sy = ('WlWpt%s<%s, %d, 1>' % (k, TNAME[dtype], L) for k in ('Afb', 'Sfb'))
    assert tuple(shape[2:]) == (8, 8)
    planes = shape[0] * shape[1]
    with fused(False):
        for mode in ('zero', 'symmetric', 'periodization'):
            m = dwl.mode_to_int(mode)
            if mode != 'periodization' or 8 >= L - 1:
                _, _, ks = check_forward(dev, shape, wave, 1, mode, dtype)
                assert ks == [A] and last_grid() < planes, (mode, ks, last_grid(), planes)
            else:
                h = [torch.tensor(np.ascontiguousarray(v), dtype=F32, device=dev) for v in taps(wave, f32=True)]
                assert ops.wpt2d_afb(rand(shape, dtype, dev, 1), h[0], h[1], h[0], h[1], m) is None
            if mode != 'periodization' or 8 >= L - 2:
                c0 = pw.launch_count()
                check_inverse(dev, shape, wave, mode, J=1, dtype=dtype)
                assert names(pw.kernels_since(c0)) == [Sy] and last_grid() < planes, (mode, pw.kernels_since(c0), last_grid(), planes)
            else:
                g = [torch.tensor(np.ascontiguousarray(v), dtype=F32, device=dev) for v in taps(wave, syn=True, f32=True)]
                assert ops.wpt2d_sfb(rand(tuple(shape[:2]) + (4, 4, 4), dtype, dev, 1), g[0], g[1], g[0], g[1], m) is None


def check_two_level_instantiation(dev, wave, dtype, shape=(2, 3, 40, 72)):
    """WlWptAfb<T, L, 2> / WlWptSfb<T, L, 2> of one tap count (up to 12) and element type: J = 2, periodization, level-2 bands of
    10 x 18 = 2 x 2 tiles of 8 x 16 with partial last tiles in both axes, a 32 x 64 synthesis tile that overhangs both axes;
    H / 2 = 20 >= L - 1 up to 12 taps.  Forward and inverse against the oracle, exactly one launch each; float32 also against the
    level-by-level route (check_wrap_shapes)."""
    if dtype == F32:
        check_wrap_shapes(dev, wave, shape)
    else:
        check_two_level_low_precision(dev, dtype, shape, wave)


# ---- 8: views --------------------------------------------------------------------------------------------------------------
def check_views(dev):
    """A non-contiguous input equals its .contiguous() twin exactly; so do a cotangent and coefficients that are views."""
    xfm, ifm = modules(dev, 'db2', 2, 'reflect')
    big = rand((2, 3, 12, 18), F32, dev, 70)
    for v in (big[..., 1:-1], big[:, 1:], big[:, :, ::2]):
        assert not v.is_contiguous()
        assert torch.equal(xfm(v), xfm(v.contiguous()))
    x = big[..., 1:-1].contiguous().requires_grad_(True)
    y = xfm(x)
    cot = rand(tuple(y.shape[:-1]) + (y.shape[-1] + 2,), F32, dev, 71)[..., 1:-1]
    cot2 = rand(tuple(y.shape[:2]) + (18,) + tuple(y.shape[3:]), F32, dev, 72)[:, :, 1:17]
    for c in (cot, cot2):
        assert not c.is_contiguous()
        d1, = torch.autograd.grad(y, x, c, retain_graph=True)
        d2, = torch.autograd.grad(y, x, c.contiguous(), retain_graph=True)
        assert torch.equal(d1, d2)
        assert torch.equal(ifm(c, size=(12, 16)), ifm(c.contiguous(), size=(12, 16)))


# ---- 9: API ----------------------------------------------------------------------------------------------------------------
def check_api(dev):
    xfm, ifm = modules(dev, 'db4', 2, 'symmetric')
    sd = xfm.state_dict()
    assert list(sd) == ['h0_col', 'h1_col', 'h0_row', 'h1_row']
    assert [tuple(v.shape) for v in sd.values()] == [(1, 1, 8, 1)] * 2 + [(1, 1, 1, 8)] * 2
    ref2d = pw.DWTForward(J=1, wave='db4', mode='symmetric').state_dict()
    other = pw.WPT2DForward(J=2, wave='db4', mode='symmetric')
    for v in other.state_dict().values():
        v.zero_()
    other.load_state_dict(ref2d)
    for k in ref2d:
        assert torch.equal(other.state_dict()[k], ref2d[k]) and torch.equal(sd[k].cpu(), ref2d[k])
    sd = ifm.state_dict()
    assert list(sd) == ['g0_col', 'g1_col', 'g0_row', 'g1_row']
    ref2d = pw.DWTInverse(wave='db4', mode='symmetric').state_dict()
    for k in ref2d:
        assert torch.equal(sd[k].cpu(), ref2d[k])
    assert pw.WPT2D is pw.WPT2DForward and pw.IWPT2D is pw.WPT2DInverse
    assert all(n in pw.__all__ for n in ('WPT2DForward', 'WPT2DInverse', 'WPT2D', 'IWPT2D'))
    x = rand((1, 2, 9, 10), F32, dev, 80)
    for bad in (x[0], x[None]):
        try:
            xfm(bad)
        except ValueError:
            pass
        else:
            raise AssertionError('a %d-D input did not raise' % bad.dim())
    y0 = modules(dev, 'db4', 0, 'symmetric')[0](x)
    assert tuple(y0.shape) == (1, 2, 1, 9, 10) and torch.equal(y0[:, :, 0], x)
    assert torch.equal(ifm(y0), x)
    # the function-level pair, and a (lo, hi) tuple of taps as the wavelet
    w = filters.Wavelet('db2')
    h, g = taps('db2', f32=True), taps('db2', syn=True, f32=True)
    for mode in ('periodization', 'symmetric'):
        y = dwl.wpt2d_level(x, (w.dec_lo, w.dec_hi), mode)
        close(y, level_ref(npy(x), h, mode), F32, 'wpt2d_level %s' % mode)
        close(dwl.iwpt2d_level(y, (w.rec_lo, w.rec_hi), mode), unlevel_ref(npy(y), g, mode), F32, 'iwpt2d_level %s' % mode)
        close(dwl.iwpt2d_level(y, (w.rec_lo, w.rec_hi), mode, out_hw=(9, 10)), unlevel_ref(npy(y), g, mode, (9, 10)), F32,
              'iwpt2d_level out_hw %s' % mode)
    close(pw.WPT2DForward(J=2, wave=(w.dec_lo, w.dec_hi), mode='zero').to(dev)(x), fwd_ref(npy(x), 2, h, 'zero'), F32, 'tuple wave')


def check_cpu_tensor_raises():
    """Without the emulator installed a CPU tensor meets the engine's usual error."""
    try:
        pw.WPT2DForward(J=1, wave='db2')(torch.zeros(1, 1, 8, 8))
    except RuntimeError as e:
        assert 'no CPU fallback' in str(e), e
    else:
        raise AssertionError('a CPU tensor did not raise')
