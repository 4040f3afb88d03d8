"""Shared checks of the 1-D scattering layer - ScatLayer1D, ops.scat1d_fwd / scat1d_bwd and the wave-tile kernels of
csrc/wl_scat1d.h -, run by the emulator (CPU) and the GPU test modules.

Expected values are a numpy restatement of the definition on the pinned oracle's ``wo.colfilter(axis=2)``: xe = x with a copy of
its last sample where n is odd, lo / hi = colfilter(xe, h0o / h1o), Z = [(lo[2k] + lo[2k+1]) / 2, sqrt(hi[2k]^2 + hi[2k+1]^2 +
b^2) - b]; the gradient is the reference's rule (ScatLayerj1_f.backward on one axis): dlo[2k] = dlo[2k+1] = dZ_low[k] / 2,
dhi[2k + i] = dZ_mag[k] hi[2k + i] / r, dxe = colfilter(dlo, h0o) + colfilter(dhi, h1o), an odd n adds dxe[n] onto dx[n-1].
For 2-byte types the reference is computed in float64 on the rounded inputs with the module's float32 taps.

Tolerances are those of tests/_dtcwt1d_cases.py (its ``close``), relative to |ref|max: float32 1e-5, float16 3e-3 max(1, .),
bfloat16 4e-3 forward and 3e-2 for the backward, which goes through the rounded directions, float64 1e-12."""
import functools

import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import _lib, ops
from _dtcwt1d_cases import close

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
BIORTS = {'near_sym_a': (5, 7), 'legall': (5, 3), 'near_sym_b': (13, 19), 'antonini': (9, 7)}
LEAD = (2, 3)          # (N, C): 6 rows - the (b, c) split of the output rows, and with three tiles 18 waves: no multiple of 4
BIAS = 1e-2
CUSTOM = ([0.02, -0.05, 0.28, 0.5, 0.28, -0.05, 0.02], [-0.1, -0.2, 0.6, -0.2, -0.1])      # (h0o, h1o): 7 / 5 taps, no kernel
WL_ERR_SHAPE = -2


def core_of(biort):
    return ops.scat1d_core(*BIORTS[biort])


def lens(biort):
    """Rows shorter than either filter (the fold wraps many times in one tile), odd rows, rows off the 16-byte grid from the
    second row on, one position either side of a full tile, two tiles and an odd sample into a third."""
    core = core_of(biort)
    return (2, 3, 7, 16, core - 1, core, core + 1, core + 2, 2 * core + 1)


def npy(t):
    return t.detach().cpu().double().numpy()


def layer(dev, biort='near_sym_a', dtype=F32, **kw):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64 if dtype == F64 else F32)
    try:
        return pw.ScatLayer1D(biort=biort, magbias=kw.pop('magbias', BIAS), **kw).to(dev)
    finally:
        torch.set_default_dtype(prev)


def taps_of(mod):
    return npy(mod.h0o).ravel(), npy(mod.h1o).ravel()


def names_since(c0):
    return [k.split('<')[0] for k in pw.kernels_since(c0)]


def dev_t(a, dtype, dev):
    return torch.tensor(a).to(dtype).to(dev)


# ---------------------------------------------------------------------------------------------- numpy references
def fwd_ref(x, taps, bias):
    """(Z (N, 2C, ne/2), dir (N, C, ne)) of x (N, C, n), float64."""
    x = np.asarray(x)
    if x.shape[-1] % 2:
        x = np.concatenate((x, x[..., -1:]), axis=-1)
    lo, hi = wo.colfilter(x, taps[0], axis=2), wo.colfilter(x, taps[1], axis=2)
    r = np.sqrt(hi[..., 0::2] ** 2 + hi[..., 1::2] ** 2 + bias * bias)
    Z = np.concatenate((0.5 * (lo[..., 0::2] + lo[..., 1::2]), r - bias), axis=1)
    return Z, hi / np.repeat(r, 2, axis=-1)


def bwd_ref(dz, d, taps, n):
    """dx (N, C, n) from dz (N, 2C, ne/2) and the directions d (N, C, ne)."""
    C = d.shape[1]
    dlo, dhi = 0.5 * np.repeat(dz[:, :C], 2, axis=-1), np.repeat(dz[:, C:], 2, axis=-1) * d
    dxe = wo.colfilter(dlo, taps[0], axis=2) + wo.colfilter(dhi, taps[1], axis=2)
    if n % 2:
        dxe = np.concatenate((dxe[..., :n - 1], dxe[..., n - 1:n] + dxe[..., n:]), axis=-1)
    return dxe


@functools.lru_cache(maxsize=None)
def _inputs(shape, seed):
    """(x, dZ): float64 numpy, made once per shape and shared (never written to)."""
    rng = np.random.RandomState(seed)
    N, C, n = shape
    return rng.randn(N, C, n), rng.randn(N, 2 * C, (n + 1) // 2)


def check_adjoint_of_the_rule():
    """The reference's rule is the exact adjoint of the linear part for the library's symmetric filters: <A x, g> = <x, A^T g>."""
    rng = np.random.RandomState(2)
    for biort in BIORTS:
        taps = taps_of(layer('cpu', biort, F64))
        for n in (2, 4, 6, 16, 40):
            x, g = rng.randn(1, 1, n), rng.randn(1, 1, n)
            for h in taps:
                a, b = float((wo.colfilter(x, h, axis=2) * g).sum()), float((x * wo.colfilter(g, h, axis=2)).sum())
                assert abs(a - b) <= 1e-13 * max(1.0, abs(a)), (biort, n, a, b)


# ---------------------------------------------------------------------------------------------- values
def check_values(dev, biort, n, dtype=F32):
    """Z and dx of the module against the definition; one launch of either kernel."""
    xn, gn = _inputs(LEAD + (n,), 31)
    mod = layer(dev, biort)
    taps = taps_of(mod)
    x = dev_t(xn, dtype, dev).requires_grad_(True)
    c0 = pw.launch_count()
    Z = mod(x)
    assert names_since(c0) == ['WlScat1dFwd'], (biort, n, names_since(c0))
    g = dev_t(gn, dtype, dev)
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(Z, x, g)
    assert names_since(c0) == ['WlScat1dBwd'], (biort, n, names_since(c0))
    rz, rd = fwd_ref(npy(x), taps, BIAS)
    what = '%s n=%d' % (biort, n)
    assert Z.dtype == dtype and Z.is_contiguous() and dx.dtype == dtype and dx.shape == x.shape
    C = LEAD[1]
    close(Z[:, :C], rz[:, :C], dtype, 'Z low ' + what)
    close(Z[:, C:], rz[:, C:], dtype, 'Z mag ' + what)
    close(dx, bwd_ref(npy(g), rd, taps, n), dtype, 'dx ' + what, chain=True)


def check_grid(dev, biort):
    for n in lens(biort):
        check_values(dev, biort, n)


def check_two_byte(dev, biort, dtype):
    for n in (3, core_of(biort) + 1):
        check_values(dev, biort, n, dtype)


# ---------------------------------------------------------------------------------------------- seams
def fused_pair(dev, biort, shape, dtype, origin):
    """(Z, dir, dx): ops.scat1d_fwd of x and ops.scat1d_bwd of a random dZ, the first tile moved left by `origin`."""
    xn, gn = _inputs(shape, 32)
    mod = layer(dev, biort)
    Z, d = ops.scat1d_fwd(dev_t(xn, dtype, dev), mod.h0o, mod.h1o, BIAS, True, origin=origin)
    dx = ops.scat1d_bwd(dev_t(gn, dtype, dev), d, mod.h0o, mod.h1o, shape[-1], origin=origin)
    return [Z, d, dx]


def check_origin(dev, biort, dtype=F32):
    """The seams of a row fall elsewhere: not a bit changes, forward, directions and backward; an odd origin and one past the
    core are refused."""
    core = core_of(biort)
    for n in (core + 1, 2 * core + 1, 7):
        base = fused_pair(dev, biort, (2, 1, n), dtype, 0)
        for origin in (2, core - 2):
            got = fused_pair(dev, biort, (2, 1, n), dtype, origin)
            assert all(torch.equal(a, b) for a, b in zip(got, base)), (biort, n, origin)
    mod = layer(dev, biort)
    x = dev_t(_inputs((2, 1, 40), 32)[0], F32, dev)
    h = [ops._taps(t, x) for t in (mod.h0o, mod.h1o)]
    z, d = torch.empty(2, 2, 20, device=dev), torch.empty(2, 1, 40, device=dev)
    be = ops._backend()
    L0, L1 = BIORTS[biort]
    for origin in (1, core - 1, core, core + 2):
        args = (0, 2, 1, 40, h[0].data_ptr(), L0, h[1].data_ptr(), L1, BIAS, origin, None)
        assert be.wl_scat1d_forward(x.data_ptr(), z.data_ptr(), d.data_ptr(), *args) == WL_ERR_SHAPE, origin
        assert be.wl_scat1d_backward(z.data_ptr(), d.data_ptr(), x.data_ptr(), *args) == WL_ERR_SHAPE, origin


def schedule_case(dev):
    """One forward + backward (near_sym_b, (2, 2, core + 1)): everything that comes out, for a bitwise comparison."""
    return fused_pair(dev, 'near_sym_b', (2, 2, core_of('near_sym_b') + 1), F32, 0)


# ---------------------------------------------------------------------------------------------- the existing transform
def hand_written(dev, biort, x, b, dtype=F32):
    """What a user writes today: level 1 of DTCWT1DForward and element-wise torch."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64 if dtype == F64 else F32)
    try:
        xfm = pw.DTCWT1DForward(biort=biort, J=1).to(dev)
    finally:
        torch.set_default_dtype(prev)
    yl, yh = xfm(x)
    mag = torch.sqrt(yh[0][..., 0] ** 2 + yh[0][..., 1] ** 2 + b * b) - b
    low = 0.5 * (yl[..., 0::2] + yl[..., 1::2])
    return torch.cat((low, mag), 1)


def check_identity(dev, biort, dtype=F32):
    """Z is the hand-written composition from DTCWT1DForward(J=1); two layers in a row give (N, 4C, .)."""
    mod = layer(dev, biort)
    for n in (7, 16, core_of(biort) + 1):
        x = dev_t(_inputs(LEAD + (n,), 33)[0], dtype, dev)
        c0 = pw.launch_count()
        Z = mod(x)
        assert names_since(c0) == ['WlScat1dFwd']
        close(Z, npy(hand_written(dev, biort, x, BIAS, dtype)), dtype, 'against DTCWT1DForward %s n=%d' % (biort, n))
        c0 = pw.launch_count()
        Z2 = mod(Z)
        assert names_since(c0) == ['WlScat1dFwd']
        n1 = (n + 1) // 2
        assert tuple(Z2.shape) == (LEAD[0], 4 * LEAD[1], (n1 + 1) // 2) and bool(torch.isfinite(Z2).all())
        close(Z2, fwd_ref(npy(Z), taps_of(mod), BIAS)[0], dtype, 'second order %s n=%d' % (biort, n))


# ---------------------------------------------------------------------------------------------- routes
class switch(object):
    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        self.prev, ops.SCAT1D_FUSED = ops.SCAT1D_FUSED, self.flag

    def __exit__(self, *exc):
        ops.SCAT1D_FUSED = self.prev
        return False


def run_once(mod, x, g):
    """(Z, dx, kernel names)."""
    x = x.clone().requires_grad_(True)
    c0 = pw.launch_count()
    Z = mod(x)
    dx, = torch.autograd.grad(Z, x, g)
    return Z.detach(), dx, names_since(c0)


def check_routes(dev):
    """float64, a 7 / 5 tap pair and the switch take the composition - no WlScat1d kernel -, with the definition's answers; the
    fused and the composed route agree."""
    for n in (7, 40):
        xn, gn = _inputs(LEAD + (n,), 34)
        # float64
        mod = layer(dev, 'near_sym_b', F64)
        Z, dx, ks = run_once(mod, dev_t(xn, F64, dev), dev_t(gn, F64, dev))
        assert not any(k.startswith('WlScat1d') for k in ks), ks
        rz, rd = fwd_ref(xn, taps_of(mod), BIAS)
        close(Z, rz, F64, 'Z float64 n=%d' % n)
        close(dx, bwd_ref(gn, rd, taps_of(mod), n), F64, 'dx float64 n=%d' % n)
        # taps no kernel is instantiated for
        mod = layer(dev, CUSTOM)
        x, g = dev_t(xn, F32, dev), dev_t(gn, F32, dev)
        Z, dx, ks = run_once(mod, x, g)
        assert ks and not any(k.startswith('WlScat1d') for k in ks), ks
        rz, rd = fwd_ref(npy(x), taps_of(mod), BIAS)
        close(Z, rz, F32, 'Z 7/5 taps n=%d' % n)
        close(dx, bwd_ref(npy(g), rd, taps_of(mod), n), F32, 'dx 7/5 taps n=%d' % n)
    # the switch
    for biort, dtype in (('near_sym_a', F32), ('near_sym_b', F32), ('near_sym_a', F16)):
        for n in (7, core_of(biort) + 1):
            xn, gn = _inputs(LEAD + (n,), 34)
            mod = layer(dev, biort)
            x, g = dev_t(xn, dtype, dev), dev_t(gn, dtype, dev)
            outs = {}
            for flag in (True, False):
                with switch(flag):
                    Z, dx, ks = run_once(mod, x, g)
                assert (ks == ['WlScat1dFwd', 'WlScat1dBwd']) if flag else not any(k.startswith('WlScat1d') for k in ks), (flag, ks)
                outs[flag] = (Z, dx)
            close(outs[True][0], npy(outs[False][0]), dtype, 'fused against composed Z %s n=%d' % (biort, n))
            close(outs[True][1], npy(outs[False][1]), dtype, 'fused against composed dx %s n=%d' % (biort, n), chain=True)


def check_inference_stores_no_directions(dev):
    """Under torch.no_grad(), and for an input that asks for no gradient, the launch gets a null `dir`; the C entry accepts it
    and writes the same Z."""
    mod = layer(dev, 'near_sym_a')
    n = core_of('near_sym_a') + 1
    x = dev_t(_inputs(LEAD + (n,), 35)[0], F32, dev)
    seen, call0 = [], ops._call

    def call(name, ref, *args):
        if name == 'wl_scat1d_forward':
            seen.append(args[2])
        return call0(name, ref, *args)

    ops._call = call
    try:
        c0 = pw.launch_count()
        Za = mod(x)
        with torch.no_grad():
            Zb = mod(x.clone().requires_grad_(True))
        Zc = mod(x.clone().requires_grad_(True))
        assert names_since(c0) == ['WlScat1dFwd'] * 3
    finally:
        ops._call = call0
    assert seen[0] is None and seen[1] is None and seen[2] is not None, seen
    assert not Zb.requires_grad and Zc.requires_grad and torch.equal(Za, Zb) and torch.equal(Za, Zc)
    h = [ops._taps(t, x) for t in (mod.h0o, mod.h1o)]
    z = torch.full_like(Za, float('nan'))
    rc = ops._backend().wl_scat1d_forward(x.data_ptr(), z.data_ptr(), None, 0, LEAD[0], LEAD[1], n, h[0].data_ptr(), 5,
                                          h[1].data_ptr(), 7, BIAS, 0, ops._stream(x))
    if x.is_cuda:
        torch.cuda.synchronize()
    assert rc == 0 and torch.equal(z, Za)


# ---------------------------------------------------------------------------------------------- gradients
def check_gradcheck(dev):
    """torch.autograd.gradcheck on the float64 (composed) route: even, odd and shorter than the filters."""
    rng = np.random.RandomState(36)
    for biort in ('near_sym_a', 'near_sym_b'):
        mod = layer(dev, biort, F64, magbias=0.1)
        for n in (3, 8, 11):
            x = dev_t(rng.randn(1, 2, n), F64, dev).requires_grad_(True)
            assert torch.autograd.gradcheck(mod, (x,), eps=1e-6, atol=1e-6), (biort, n)


# ---------------------------------------------------------------------------------------------- edges
def check_errors_and_edges(dev):
    mod = layer(dev, 'near_sym_a')
    # zero rows
    for shape in ((0, 3, 16), (2, 0, 16)):
        x = torch.zeros(shape, device=dev, requires_grad=True)
        Z = mod(x)
        assert tuple(Z.shape) == (shape[0], 2 * shape[1], 8)
        Z.sum().backward()
        assert x.grad is not None and x.grad.shape == x.shape
    x = dev_t(_inputs((2, 2, 20), 37)[0], F32, dev)
    h = [ops._taps(t, x) for t in (mod.h0o, mod.h1o)]
    be, unsupported = ops._backend(), _lib.WL_ERR_UNSUPPORTED
    z, d = torch.empty(2, 4, 10, device=dev), torch.empty(2, 2, 20, device=dev)
    p = (x.data_ptr(), z.data_ptr(), d.data_ptr())
    tail = (h[0].data_ptr(), 5, h[1].data_ptr(), 7, BIAS, 0, None)
    assert be.wl_scat1d_forward(*(p + (0, 0, 2, 20) + tail)) == 0 and be.wl_scat1d_backward(*(p + (0, 0, 2, 20) + tail)) == 0
    assert be.wl_scat1d_forward(*(p + (2, 2, 2, 20) + tail)) == unsupported                                     # float64
    assert be.wl_scat1d_forward(*(p + (0, 2, 2, 20, h[1].data_ptr(), 7, h[0].data_ptr(), 5, BIAS, 0, None))) == unsupported
    assert be.wl_scat1d_forward(*(p + (0, 2, 2, 0) + tail)) == WL_ERR_SHAPE
    assert be.wl_scat1d_forward(*((None,) + p[1:] + (0, 2, 2, 20) + tail)) == WL_ERR_SHAPE
    # the wrappers outside the envelope decline
    assert ops.scat1d_fwd(x.double(), mod.h0o, mod.h1o, BIAS, False) is None
    assert ops.scat1d_fwd(x, mod.h1o, mod.h0o, BIAS, False) is None
    with pytest.raises(ValueError, match="'symmetric' only"):
        pw.ScatLayer1D(mode='zero')
    with pytest.raises(AssertionError):
        mod(x[None])
    assert repr(mod) == "ScatLayer1D(biort='near_sym_a', mode='symmetric', magbias=0.01)"
    assert sorted(mod.state_dict()) == ['h0o', 'h1o']
    assert not any(q.requires_grad for q in mod.parameters())
    src = pw.DTCWT1DForward(biort='near_sym_a', J=1).to(dev)
    assert torch.equal(mod.h0o, src.h0o) and torch.equal(mod.h1o, src.h1o)
    res = layer(dev, 'near_sym_a').load_state_dict(mod.state_dict())
    assert not res.missing_keys and not res.unexpected_keys


def check_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.ScatLayer1D()(torch.zeros(1, 1, 16))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.ScatLayer1D(biort=CUSTOM)(torch.zeros(1, 1, 16))


def check_views(dev):
    """x[1:], x[..., 1:-1], x[:, 1:] and a non-contiguous grad_output give the answers of their contiguous copies, bit for bit."""
    n = core_of('near_sym_a') + 3
    base = dev_t(_inputs((3, 3, n), 38)[0], F32, dev)
    mod = layer(dev, 'near_sym_a')
    for cut in (lambda t: t[1:], lambda t: t[..., 1:-1], lambda t: t[:, 1:]):
        view = cut(base).detach().requires_grad_(True)             # (a leaf with the view's offset and strides)
        copy = view.detach().contiguous().requires_grad_(True)
        assert view.data_ptr() != base.data_ptr() or not view.is_contiguous()
        Za, Zb = mod(view), mod(copy)
        assert torch.equal(Za, Zb)
        g = dev_t(np.random.RandomState(39).randn(*(tuple(Zb.shape[:-1]) + (2 * Zb.shape[-1],))), F32, dev)[..., ::2]
        assert not g.is_contiguous()
        da, = torch.autograd.grad(Za, view, g)
        db, = torch.autograd.grad(Zb, copy, g.contiguous())
        assert torch.equal(da, db)
