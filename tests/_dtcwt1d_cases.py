"""Shared checks of the 1-D DTCWT (DTCWT1DForward / DTCWT1DInverse, ops.dtcwt1d_fwd / ops.dtcwt1d_inv and the fused kernels of
csrc/wl_dtcwt1d.h), run by the emulator (CPU) and the GPU test modules.

The expected answer is a numpy composition of the pinned column primitives of the oracle (``wo.colfilter / wo.coldfilt /
wo.colifilt`` with ``axis=``): level 1 the two odd-length filters at full rate (an odd length first gets a copy of its last
sample), every further level ``coldfilt`` of the lowpass - padded by one replicated sample either side where its length is no
multiple of 4 -, ``yh[j][..., k, :] = (hi[2k], hi[2k+1])``; the inverse is ``colifilt`` / ``colfilter`` of the lowpass (cropped by one
sample either side where it is longer than the band) plus that of the interleaved band.  Gradients follow the reference's rule
(transform_funcs.py:361-413, 434-488 on one axis): the backward of the analysis is the synthesis structure with the analysis
taps, a / b trees swapped at the q-shift levels, pad samples folded back by addition; the backward of the synthesis the analysis
structure with the synthesis taps, swapped likewise, zero padding where the forward cropped.  Goldens (tests/golden/dtcwt1d_*.npz,
tools/make_dtcwt1d_golden.py): the reference's own CPU primitives in float64, dx from torch.autograd through them.

Tolerances (tests/_dwt3d_cases.py): float32 1e-5 |ref|max; float16 3e-3 max(1, |ref|max); float64 1e-12 max(1, |ref|max); bfloat16
relative to |ref|max 4e-3 where one launch made the value, 3e-2 across launches - the 2-byte types against the oracle on the
rounded inputs with float32 taps."""
import glob
import os

import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters, ops

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
BF_ONE, BF_MULTI = 4e-3, 3e-2
FUSED_PAIRS = (('near_sym_a', 'qshift_a'), ('near_sym_b', 'qshift_b'), ('legall', 'qshift_06'))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def npy(t):
    return t.detach().cpu().double().numpy()


def taps(biort, qshift, syn=False, f32=False):
    t = filters.dtcwt_inverse_taps(biort, qshift) if syn else filters.dtcwt_forward_taps(biort, qshift)
    t = tuple(np.asarray(v, dtype=np.float64) for v in t)
    return tuple(v.astype(np.float32).astype(np.float64) for v in t) if f32 else t


def swap(t):
    return t[0], t[1], t[3], t[2], t[5], t[4]


# ---------------------------------------------------------------------------------------------- numpy references
def fwd_ref(x, J, t, scales=False):
    """(yl, [yh_j (.., L_j, 2)]) - and the lowpass of every level with scales."""
    h0o, h1o, h0a, h0b, h1a, h1b = t
    x = np.asarray(x)
    if x.shape[-1] % 2:
        x = np.concatenate((x, x[..., -1:]), axis=-1)
    lo, hi = wo.colfilter(x, h0o, axis=x.ndim - 1), wo.colfilter(x, h1o, axis=x.ndim - 1)
    yh, los = [hi.reshape(hi.shape[:-1] + (-1, 2))], [lo]
    for _ in range(1, J):
        if lo.shape[-1] % 4:
            lo = np.concatenate((lo[..., :1], lo, lo[..., -1:]), axis=-1)
        hi = wo.coldfilt(lo, h1b, h1a, True, axis=lo.ndim - 1)
        lo = wo.coldfilt(lo, h0b, h0a, False, axis=lo.ndim - 1)
        yh.append(hi.reshape(hi.shape[:-1] + (-1, 2)))
        los.append(lo)
    return (lo, yh, los) if scales else (lo, yh)


def inv_ref(yl, yh, t, fold=None, odd=False):
    """The inverse; with fold (a list over the levels: the analysis padded that level's input) the ends are folded back by
    addition instead of cropped, with odd the last sample onto the one before: the backward rule of the analysis."""
    g0o, g1o, g0a, g0b, g1a, g1b = t
    lo = np.asarray(yl)
    ax = lo.ndim - 1
    for j in range(len(yh) - 1, -1, -1):
        h = yh[j]
        if h is not None:
            h = np.asarray(h).reshape(h.shape[:-2] + (-1,))
            if lo.shape[-1] != h.shape[-1]:
                assert lo.shape[-1] == h.shape[-1] + 2
                lo = lo[..., 1:-1]
        if j == 0:
            y = wo.colfilter(lo, g0o, axis=ax) + (0 if h is None else wo.colfilter(h, g1o, axis=ax))
            if odd:
                y = np.concatenate((y[..., :-2], y[..., -2:-1] + y[..., -1:]), axis=-1)
        else:
            y = wo.colifilt(lo, g0b, g0a, False, axis=ax) + (0 if h is None else wo.colifilt(h, g1b, g1a, True, axis=ax))
            if fold is not None and fold[j]:
                y = np.concatenate((y[..., 1:2] + y[..., 0:1], y[..., 2:-2], y[..., -2:-1] + y[..., -1:]), axis=-1)
        lo = y
    return lo


def fwd_grad_ref(dyl, dyh, n, t):
    """dx of the analysis of an n-sample signal by the reference's rule; t = the ANALYSIS taps."""
    J, m, fold = len(dyh), n + (n & 1), []
    for j in range(J):
        fold.append(j > 0 and m % 4 != 0)
        m = m if j == 0 else (m + (2 if fold[j] else 0)) // 2
    return inv_ref(dyl, dyh, swap(t), fold=fold, odd=n % 2 == 1)


def inv_grad_ref(dy, lo_len, band_lens, t):
    """(dyl, [dyh_j]) of the synthesis; band_lens[j] = samples of level j's interleaved band (the lowpass it is handed is cropped to
    it), lo_len = samples of yl; t = the SYNTHESIS taps."""
    g0o, g1o, g0a, g0b, g1a, g1b = swap(t)
    d = np.asarray(dy)
    ax = d.ndim - 1
    hi, lo = wo.colfilter(d, g1o, axis=ax), wo.colfilter(d, g0o, axis=ax)
    grads = [hi.reshape(hi.shape[:-1] + (-1, 2))]
    for j in range(1, len(band_lens)):
        if lo.shape[-1] != 2 * band_lens[j]:
            lo = np.pad(lo, [(0, 0)] * ax + [(1, 1)])
        hi = wo.coldfilt(lo, g1b, g1a, True, axis=ax)
        lo = wo.coldfilt(lo, g0b, g0a, False, axis=ax)
        grads.append(hi.reshape(hi.shape[:-1] + (-1, 2)))
    if lo.shape[-1] != lo_len:
        lo = np.pad(lo, [(0, 0)] * ax + [(1, 1)])
    return lo, grads


def close(a, ref, dtype, what='', chain=False):
    a = npy(a) if isinstance(a, torch.Tensor) else a
    assert tuple(a.shape) == tuple(ref.shape), (what, a.shape, ref.shape)
    err, top = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    bound = {F64: 1e-12 * max(1.0, top), F32: 1e-5 * top, F16: 3e-3 * max(1.0, top),
             BF16: (BF_MULTI if chain else BF_ONE) * top}[dtype]
    print('%s %s: max err %.3e, bound %.3e' % (what, dtype, err, bound))
    assert err <= bound, (what, err, bound)


def modules(dev, biort, qshift, J, dtype=F32, **kw):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64 if dtype == F64 else F32)
    try:
        return (pw.DTCWT1DForward(biort=biort, qshift=qshift, J=J, **kw).to(dev),
                pw.DTCWT1DInverse(biort=biort, qshift=qshift, ri_dim=kw.get('ri_dim', -1)).to(dev))
    finally:
        torch.set_default_dtype(prev)


def rand(shape, dtype, dev, seed):
    return torch.tensor(np.random.RandomState(seed).randn(*shape)).to(dtype).to(dev)


def names(ks):
    return [k.split('<')[0] for k in ks if not k.endswith(')')]


class forced_chunk(object):
    def __init__(self, chunk):
        self.chunk = chunk

    def __enter__(self):
        self.prev, ops.DT1D_CHUNK = ops.DT1D_CHUNK, self.chunk

    def __exit__(self, *exc):
        ops.DT1D_CHUNK = self.prev
        return False


# ---------------------------------------------------------------------------------------------- checks
QLEN = {'qshift_06': 10, 'qshift_a': 10, 'qshift_b': 14, 'qshift_c': 16, 'qshift_d': 18}


def expect_fused(n, J, qshift):
    """(analysis, synthesis) take the fused kernels: float data, 10 / 14 / 18 q-shift taps, and every q-shift level long enough to
    mirror its ends with ONE fold - the analysis pair k = 0 reads m - 2 samples in front of its (padded) input, the synthesis
    group q = 0 reads m / 2 - 1 in front of its band."""
    m = QLEN[qshift]
    if J > 1 and m not in (10, 14, 18):
        return False, False
    fwd = inv = True
    ln = n + (n & 1)
    for _ in range(1, J):
        ln += 2 if ln % 4 else 0
        fwd = fwd and ln >= m - 2
        ln //= 2
        inv = inv and ln >= m // 2 - 1
    return fwd, inv

def check_values(dev, n, J, biort, qshift, dtype=F32, fused=None, shape=None, seed=0):
    """Forward, layout, kernel names, inverse against the oracle and the round trip."""
    shape = shape or (1, 3, n)
    xfm, ifm = modules(dev, biort, qshift, J, dtype)
    x = rand(shape, dtype, dev, seed + n + 10 * J)
    f32 = dtype != F64
    c0 = pw.launch_count()
    yl, yh = xfm(x)
    kf = names(pw.kernels_since(c0))
    rl, rh = fwd_ref(npy(x), J, taps(biort, qshift, f32=f32))
    close(yl, rl, dtype, 'yl n=%d J=%d %s' % (n, J, biort))
    for j in range(J):
        assert yh[j].shape[-1] == 2 and yh[j].is_contiguous()
        close(yh[j], rh[j], dtype, 'yh[%d]' % j)
        z = torch.view_as_complex(yh[j]) if dtype in (F32, F64) else None
        assert z is None or z.shape == yh[j].shape[:-1]
    c0 = pw.launch_count()
    rec = ifm((yl, yh))
    ki = names(pw.kernels_since(c0))
    chain = dtype == BF16
    close(rec, inv_ref(npy(yl), [npy(h) for h in yh], taps(biort, qshift, syn=True, f32=f32)), dtype, 'rec', chain=False)
    xe = npy(x)
    xe = np.concatenate((xe, xe[..., -1:]), axis=-1) if n % 2 else xe
    close(rec, xe, dtype, 'round trip', chain=chain)
    ef, ei = (False, False) if dtype == F64 else expect_fused(n, J, qshift)
    assert fused is None or (ef, ei) == (fused, fused), (n, J, qshift, ef, ei)
    assert kf == ['WlDt1dFwd'] if ef else ('WlDt1dFwd' not in kf and len(kf) > 1), kf
    assert ki == ['WlDt1dInv'] if ei else ('WlDt1dInv' not in ki and len(ki) > 1), ki
    return kf, ki


def check_options(dev):
    """skip_hps / include_scale as lists, ri_dim = 2, J = 0, two groups."""
    biort, qshift, n, J = 'near_sym_a', 'qshift_a', 20, 3
    t = taps(biort, qshift, f32=True)
    x = rand((2, 2, n), F32, dev, 5)
    rl, rh, rlos = fwd_ref(npy(x), J, t, scales=True)
    xfm, _ = modules(dev, biort, qshift, J, skip_hps=[False, True, False], include_scale=[True, False, True])
    c0 = pw.launch_count()
    scales, yh = xfm(x)
    assert names(pw.kernels_since(c0)) == ['WlDt1dFwd']
    assert yh[1].shape == torch.Size([]) and scales[1].shape == torch.Size([])
    close(yh[0], rh[0], F32, 'yh[0] with skip'); close(yh[2], rh[2], F32, 'yh[2] with skip')
    close(scales[0], rlos[0], F32, 'scale 0'); close(scales[2], rlos[2], F32, 'scale 2')
    xfm, ifm = modules(dev, biort, qshift, J, ri_dim=2)
    yl, yh = xfm(x)
    for j in range(J):
        assert yh[j].shape[2] == 2
        close(yh[j].movedim(2, -1), rh[j], F32, 'ri_dim=2 yh[%d]' % j)
    close(ifm((yl, yh)), npy(x), F32, 'ri_dim=2 round trip')
    x0 = pw.DTCWT1DForward(J=0).to(dev)(x)
    assert x0[0] is x and x0[1] is None
    # two groups of levels
    x = rand((1, 2, 512), F32, dev, 6)
    xfm, ifm = modules(dev, biort, qshift, 6)
    c0 = pw.launch_count()
    yl, yh = xfm(x)
    assert names(pw.kernels_since(c0)) == ['WlDt1dFwd'] * 2
    rl, rh = fwd_ref(npy(x), 6, t)
    close(yl, rl, F32, 'J=6 yl')
    for j in range(6):
        close(yh[j], rh[j], F32, 'J=6 yh[%d]' % j)
    c0 = pw.launch_count()
    rec = ifm((yl, yh))
    assert names(pw.kernels_since(c0)) == ['WlDt1dInv'] * 2
    close(rec, npy(x), F32, 'J=6 round trip')


def check_float64_takes_the_generic_kernels(dev):
    kf, ki = check_values(dev, 22, 3, 'near_sym_a', 'qshift_a', F64, fused=False)
    assert set(kf) == {'WlCorr1d'} and set(ki) == {'WlCorr1d'}, (kf, ki)


def run_both(dev, n, J, biort, qshift, dtype, chunks, shape=None, seed=3):
    """(yl, yh, rec, dx) with forced chunk lengths (analysis pairs, synthesis samples)."""
    shape = shape or (2, 1, n)
    xfm, ifm = modules(dev, biort, qshift, J, dtype)
    x = rand(shape, dtype, dev, seed).requires_grad_(True)
    with forced_chunk(chunks[0]):
        yl, yh = xfm(x)
    with forced_chunk(chunks[1]):
        rec = ifm((yl.detach(), [h.detach() for h in yh]))
        cots = [rand(tuple(t.shape), dtype, dev, seed + 1 + i) for i, t in enumerate([yl] + yh)]
        dx, = torch.autograd.grad([yl] + yh, x, cots)
    return x, yl, yh, rec, dx, cots


def check_seams(dev, n, dtype=F32):
    """Forced chunks (at least three per row) against one chunk per row: bit for bit, both kernels, and the oracle."""
    biort, qshift, J = 'near_sym_a', 'qshift_a', 3
    one = run_both(dev, n, J, biort, qshift, dtype, (1 << 20, 1 << 20))
    for chunks in ((8, 64), (5, 44), (13, 100)):
        cut = run_both(dev, n, J, biort, qshift, dtype, chunks)
        for a, b in zip([one[1]] + one[2] + [one[3], one[4]], [cut[1]] + cut[2] + [cut[3], cut[4]]):
            assert torch.equal(a, b), chunks
    t = taps(biort, qshift, f32=True)
    rl, rh = fwd_ref(npy(one[0]), J, t)
    close(one[1], rl, dtype, 'seams yl')
    close(one[4], fwd_grad_ref(npy(one[5][0]), [npy(c) for c in one[5][1:]], n, t), dtype, 'seams dx')


def check_natural_chunks(dev):
    n, J = 9000, 3
    x, yl, yh, rec, dx, cots = run_both(dev, n, J, 'near_sym_a', 'qshift_a', F32, (0, 0), shape=(2, 1, n))
    t = taps('near_sym_a', 'qshift_a', f32=True)
    rl, rh = fwd_ref(npy(x), J, t)
    close(yl, rl, F32, '9000 yl')
    for j in range(J):
        close(yh[j], rh[j], F32, '9000 yh[%d]' % j)
    close(rec, npy(x), F32, '9000 round trip')
    close(dx, fwd_grad_ref(npy(cots[0]), [npy(c) for c in cots[1:]], n, t), F32, '9000 dx')


def check_none_highs(dev, drop):
    biort, qshift, n, J = 'near_sym_b', 'qshift_b', 22, 3
    xfm, ifm = modules(dev, biort, qshift, J)
    yl, yh = xfm(rand((1, 3, n), F32, dev, 7))
    yh = list(yh)
    yh[drop] = None
    c0 = pw.launch_count()
    rec = ifm((yl, yh))
    assert names(pw.kernels_since(c0)) == ['WlDt1dInv']
    close(rec, inv_ref(npy(yl), [None if h is None else npy(h) for h in yh], taps(biort, qshift, syn=True, f32=True)), F32,
          'inverse without yh[%d]' % drop)


def check_gradients(dev, n, J, biort, qshift, dtype, only=None):
    """dx of the forward and (dyl, dyh) of the inverse against the oracle rule; only = the one output that gets a cotangent."""
    f32 = dtype != F64
    xfm, ifm = modules(dev, biort, qshift, J, dtype)
    x = rand((1, 3, n), dtype, dev, 11).requires_grad_(True)
    yl, yh = xfm(x)
    outs = [yl] + list(yh)
    cots = [rand(tuple(t.shape), dtype, dev, 12 + i) for i, t in enumerate(outs)]
    pick = range(len(outs)) if only is None else [only]
    dx, = torch.autograd.grad([outs[i] for i in pick], x, [cots[i] for i in pick])
    zc = [npy(c) if i in pick else np.zeros(tuple(c.shape)) for i, c in enumerate(cots)]
    close(dx, fwd_grad_ref(zc[0], zc[1:], n, taps(biort, qshift, f32=f32)), dtype, 'dx only=%s' % (only,), chain=False)
    if only is not None:
        return
    wl = yl.detach().clone().requires_grad_(True)
    wh = [h.detach().clone().requires_grad_(True) for h in yh]
    rec = ifm((wl, wh))
    dy = rand(tuple(rec.shape), dtype, dev, 20)
    grads = torch.autograd.grad(rec, [wl] + wh, dy)
    gl, gh = inv_grad_ref(npy(dy), wl.shape[-1], [2 * h.shape[-2] for h in wh], taps(biort, qshift, syn=True, f32=f32))
    close(grads[0], gl, dtype, 'dyl')
    for j in range(J):
        close(grads[1 + j], gh[j], dtype, 'dyh[%d]' % j)


def check_gradcheck(dev):
    xfm, ifm = modules(dev, 'near_sym_a', 'qshift_a', 3, F64)
    x = rand((1, 2, 22), F64, dev, 30).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: tuple([xfm(v)[0]] + list(xfm(v)[1])), (x,), eps=1e-6, atol=1e-7)
    yl, yh = xfm(x.detach())
    ins = [yl.clone().requires_grad_(True)] + [h.clone().requires_grad_(True) for h in yh]
    assert torch.autograd.gradcheck(lambda l, *h: ifm((l, list(h))), tuple(ins), eps=1e-6, atol=1e-7)


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, 'dtcwt1d_*.npz')))


def check_golden(dev, path, dtype):
    g = np.load(path)
    biort, qshift, J = str(g['biort']), str(g['qshift']), int(g['J'])
    xfm, ifm = modules(dev, biort, qshift, J, dtype)
    x = torch.tensor(g['x']).to(dtype).to(dev).requires_grad_(True)
    yl, yh = xfm(x)
    exact = dtype in (F32, F64)
    if exact:                                                   # (the 2-byte types: against the oracle on the rounded inputs)
        close(yl, g['yl'], dtype, 'golden yl')
        for j in range(J):
            close(yh[j], g['yh%d' % j], dtype, 'golden yh[%d]' % j)
    else:
        # (a configuration the fused kernels decline is a chain of launches, each rounding to the 2-byte type)
        ef, ei = expect_fused(int(g['x'].shape[-1]), J, qshift)
        rl, rh = fwd_ref(npy(x), J, taps(biort, qshift, f32=True))
        close(yl, rl, dtype, 'yl', chain=not ef)
        for j in range(J):
            close(yh[j], rh[j], dtype, 'yh[%d]' % j, chain=not ef)
    cots = [torch.tensor(g['c%d' % i]).to(dtype).to(dev) for i in range(J + 1)]
    dx, = torch.autograd.grad([yl] + list(yh), x, cots)
    if exact:
        close(dx, g['dx'], dtype, 'golden dx')
        close(ifm((torch.tensor(g['yl']).to(dtype).to(dev), [torch.tensor(g['yh%d' % j]).to(dtype).to(dev) for j in range(J)])),
              g['rec'], dtype, 'golden rec')
    else:
        close(dx, fwd_grad_ref(npy(cots[0]), [npy(c) for c in cots[1:]], x.shape[-1], taps(biort, qshift, f32=True)), dtype, 'dx',
              chain=not ei)


def check_views(dev):
    biort, qshift, J = 'near_sym_a', 'qshift_a', 3
    xfm, ifm = modules(dev, biort, qshift, J)
    big = rand((3, 2, 42), F32, dev, 40)
    for v in (big[1:], big[..., 1:-1], big[:, :, ::2]):
        yl, yh = xfm(v)
        wl, wh = xfm(v.contiguous())
        assert torch.equal(yl, wl) and all(torch.equal(a, b) for a, b in zip(yh, wh))
    yl, yh = xfm(big)
    wide = [torch.cat((h, h), dim=-1)[..., :2] for h in yh]                  # views with a pitch of 4
    wide[1] = torch.stack((yh[1], yh[1]), dim=0)[1]                          # an offset base
    assert not wide[0].is_contiguous()
    assert torch.equal(ifm((yl, wide)), ifm((yl, yh)))
    pad = torch.nn.functional.pad(yl, (3, 3))[..., 3:-3]
    assert torch.equal(ifm((pad, yh)), ifm((yl, yh)))


def check_errors(dev):
    with pytest.raises(ValueError):
        pw.DTCWT1DForward(mode='zero')
    with pytest.raises(ValueError):
        pw.DTCWT1DInverse(mode='periodization')
    xfm, ifm = modules(dev, 'near_sym_a', 'qshift_a', 2)
    yl, yh = xfm(rand((1, 1, 16), F32, dev, 50))
    with pytest.raises(AssertionError, match='real and imaginary'):
        ifm((yl, [yh[0], torch.cat((yh[1], yh[1][..., :1]), dim=-1)]))


def check_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.DTCWT1DForward(J=2)(torch.zeros(1, 1, 16))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.DTCWT1DInverse()((torch.zeros(1, 1, 16), [torch.zeros(1, 1, 8, 2)]))
