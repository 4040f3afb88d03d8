"""Every kernel family on tensors past 4 GiB / 2**31 elements - the harness shared by tests/test_large_emu.py (the same code at a
scaled-down plane count, on the host emulation) and tests/test_large_gpu.py (the real sizes, on the chip).

The kernels' address arithmetic is only right where its 64-bit part sits in the right place; an overflow mostly wraps inside the
same allocation: wrong coefficients, no fault.  Two constructions make a check of EVERY output element cheap:

Part A, many planes.  Every transform treats the leading planes (rows, volumes) independently.  Flat plane i of every input is
``base[i % P]`` of P random planes, P a small prime that does not divide the plane count; the float64 oracle runs on the P planes
alone and every plane i of every output is compared with ``ref[i % P]`` on the device (`compare_planes`).  No threshold - 2**31
bytes, 2**32 bytes, 2**31 elements - is a whole multiple of P * plane bytes (`plan` asserts it for every tensor), so an address
wrapped by one of them never lands on an equal plane.

Part B, one plane / row at the top of a launcher's envelope.  The plane is periodic along H (a row: along its samples) with a
period T that is a multiple of 2**J.  The full output is then the oracle's output of a SHORT plane of a few periods, stretched:
its first rows from the short output's top, its last rows from its bottom, the rows between its middle period repeated
(`stretch_index`, `compare_stretched`); in periodization that is plain tiling.  It is exact - tests/test_large_emu.py holds it to
1e-12 against the oracle on the full plane - once the short plane has `min_short_len` rows: the borders must not reach the
middle period.

Tolerances are the families' own: `_view_cases.bound_of` (= REL of tests/_swt1d_cases.py) relative to the largest magnitude of
the reference, and for the 3-D / packet / 1-D dual-tree families the bound of their `close` (float32 1e-5 |ref|max, float16 3e-3
max(1, |ref|max)).  References are the oracles of the families' existing checks; the gradients of the transforms of
tests/_view_cases.py (2-D DWT, DTCWT, ScatLayer, SWT) have none and are compared, as there, with the engine's per-level tile
kernels on the small piece - that checks the addressing of the planes, not the kernels' arithmetic."""
import time

import numpy as np
import torch

import _dtcwt1d_cases as D1
import _dwt3d_cases as D3
import _mutation_cases
import _scat1d_cases as C1
import _swt1d_cases as S1
import _view_cases as V
import _wpt1d_cases as W1
import _wpt2d_cases as P2
import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters as F
from pytorch_wavelets_amd import ops
from pytorch_wavelets_amd.dtcwt import lowlevel as dtl
from pytorch_wavelets_amd.dwt import lowlevel as dwl

F32, F16, F64 = torch.float32, torch.float16, torch.float64
B31, B32, E31 = 2 ** 31, 2 ** 32, 2 ** 31
MAX_NEED = 48 * 2 ** 30            # bytes: no case may need more
HEADROOM = 1.25                    # a case skips only if less than this times its need is free
CHUNK_ELEMS = 1 << 24              # elements of one comparison chunk (three float64 temporaries of it)
SLACK = 3                          # planes by which the largest input and output exceed the threshold


def esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def thresholds(dtype, b32=B32):
    """[(name, byte offset)] that a tensor of `dtype` is checked around; `b32`: the 2**32-byte threshold scaled down to a test's
    size (the others scale with it)."""
    return [('2^31 bytes', b32 // 2), ('2^32 bytes', b32), ('2^31 elements', b32 // 2 * esize(dtype))]


# ---- builders ----------------------------------------------------------------------------------------------------------------
def periodic_planes(base, count):
    """(count, ...) whose plane i is base[i % P], on base's device."""
    idx = torch.arange(count, device=base.device) % base.shape[0]
    return base.index_select(0, idx)


def tiled(base, reps, axes):
    """`base` repeated reps[k] times along axes[k]."""
    r = [1] * base.dim()
    for n, a in zip(reps, axes):
        r[a] = n
    return base.repeat(*r)


# ---- the checker -------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    """The first bad flat plane / row of a tensor, the element and byte offset of its first bad element in that tensor, and the
    side of every threshold that element lies on."""

    def __init__(self, what, plane, elem, byte, sides, err, bound):
        self.what, self.plane, self.elem, self.byte, self.sides, self.err, self.bound = what, plane, elem, byte, sides, err, bound
        where = ', '.join('%s %s' % (s, n) for n, s in sides.items())
        AssertionError.__init__(self, '%s: first bad plane / row %d, first bad element %d (byte offset %d: %s), error %.3e, bound %.3e'
                                % (what, plane, elem, byte, where, err, bound))


def _sides(byte, ths):
    return {n: ('at or above' if byte >= t else 'below') for n, t in ths}


def _bad(d, bound):
    return ~(d <= bound)          # (a NaN is bad)


def compare_planes(out, ref, P, bound, what='', ths=None):
    """Every plane i of `out` (count, ...) against ref[i % P] (float64, (P, ...)), reduced on the device in chunks; returns the
    largest error, raises Mismatch at the first plane above `bound`."""
    count = out.shape[0]
    assert ref.shape[0] == P and tuple(out.shape[1:]) == tuple(ref.shape[1:]), (what, tuple(out.shape), tuple(ref.shape))
    pe = int(np.prod(out.shape[1:]))
    o2, r2 = out.reshape(count, pe), ref.reshape(P, pe).double()
    step = max(1, CHUNK_ELEMS // pe)
    worst = torch.empty(count, dtype=F64, device=out.device)
    for a in range(0, count, step):
        b = min(count, a + step)
        idx = torch.arange(a, b, device=out.device) % P
        worst[a:b] = (o2[a:b].double() - r2.index_select(0, idx)).abs().amax(1)
    bad = _bad(worst, bound).nonzero()
    if bad.numel():
        i = int(bad[0])
        d = (o2[i].double() - r2[i % P]).abs()
        e = i * pe + int(_bad(d, bound).nonzero()[0])
        es = out.element_size()
        raise Mismatch(what, i, e, e * es, _sides(e * es, ths or thresholds(out.dtype)), float(worst[i]), bound)
    return float(worst.max())


def min_short_len(L, J, T):
    """Rows a short plane needs for the stretched form to be exact: the borders of J levels of an L-tap bank reach (L - 1)(2**J - 1)
    rows in from either end, and a whole period must lie clear of both."""
    return 2 * (L - 1) * (2 ** J - 1) + 2 * T


def stretch_index(n_out, n_short, p, device='cpu'):
    """For every index r along a stretched axis of the full output, the index of the short output that holds the same value:
    the short output's top, then its middle period of p samples repeated, then its bottom."""
    assert p > 0 and n_short >= p and (n_out - n_short) % p == 0 and n_out >= n_short, (n_out, n_short, p)
    head = (n_short - p) // 2
    tail = n_short - p - head
    r = torch.arange(n_out, device=device)
    mid = head + (r - head) % p
    return torch.where(r < head, r, torch.where(r >= n_out - tail, r - (n_out - n_short), mid))


def compare_stretched(out, short, periods, bound, what='', ths=None):
    """`out` against `short` (float64) stretched along the axes of `periods` ({axis: period of that output along it}), in chunks
    along the first of them; returns the largest error, raises Mismatch at the first bad index along that axis."""
    assert out.dim() == short.dim() and out.is_contiguous(), (what, tuple(out.shape), tuple(short.shape))
    axes = sorted(a % out.dim() for a in periods)
    per = {a % out.dim(): p for a, p in periods.items()}
    assert all(out.shape[a] == short.shape[a] or a in axes for a in range(out.dim())), (what, tuple(out.shape), tuple(short.shape))
    idx = {a: stretch_index(out.shape[a], short.shape[a], per[a], out.device) for a in axes}
    exp = short.double()
    for a in axes[1:]:
        exp = exp.index_select(a, idx[a])
    a0 = axes[0]
    n = out.shape[a0]
    step = max(1, CHUNK_ELEMS // max(1, out.numel() // n))
    worst = torch.empty(n, dtype=F64, device=out.device)
    other = [a for a in range(out.dim()) if a != a0]
    for a in range(0, n, step):
        b = min(n, a + step)
        d = (out.narrow(a0, a, b - a).double() - exp.index_select(a0, idx[a0][a:b])).abs()
        worst[a:b] = d.amax(other) if other else d
    bad = _bad(worst, bound).nonzero()
    if bad.numel():
        i = int(bad[0])
        d = (out.narrow(a0, i, 1).double() - exp.index_select(a0, idx[a0][i:i + 1])).abs()
        at = [int(v) for v in _bad(d, bound).nonzero()[0]]
        at[a0] = i
        e = int(sum(k * s for k, s in zip(at, out.stride())))
        es = out.element_size()
        raise Mismatch(what, i, e, e * es, _sides(e * es, ths or thresholds(out.dtype)), float(worst[i]), bound)
    return float(worst.max())


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def rel_bound(tf, dtype, top):
    return V.bound_of(dtype, tf.one_level) * top


def close_bound(tf, dtype, top):
    """the bound of `close` in tests/_dwt3d_cases.py, _wpt2d_cases.py, _dtcwt1d_cases.py (and, through it, _scat1d_cases.py)"""
    return {F64: 1e-12 * max(1.0, top), F32: 1e-5 * top, F16: 3e-3 * max(1.0, top)}[dtype]


# ---- transforms beyond those of tests/_view_cases.py (same interface; `grad_ref(inputs, cotangents)` where the family has an
#      oracle of its gradient, `bound` where its checks use another bound than _view_cases.bound_of) -------------------------------
def _tf(name, shapes, build, one_level=False, bound=None):
    t = V.Tf(name, shapes, build, one_level)
    t.bound = bound
    return t


def swt1d_fwd(J, wave):
    h = S1.ana_taps(wave)

    def build(dev, dtype):
        m = S1.modules(dev, wave, J)[0]

        def run(x):
            yl, yh = m(x)
            return [yl] + list(yh)

        def oracle(x):
            rl, rh = S1.analysis_ref(x, h, J)
            return [rl] + list(rh)
        return run, oracle
    t = _tf('SWT1DForward(J=%d, %s)' % (J, wave), lambda s: [s], build, J == 1)
    t.grad_ref = lambda xs, cs: [S1.adjoint_ref(cs[0], list(cs[1:]), h, 1.0)]
    return t


def swt1d_inv(J, wave):
    g = S1.syn_taps(wave)

    def build(dev, dtype):
        m = S1.modules(dev, wave, J)[1]
        return (lambda yl, *yh: [m((yl, list(yh)))]), (lambda yl, *yh: [S1.adjoint_ref(yl, list(yh), g, 0.5)])
    return _tf('SWT1DInverse(J=%d, %s)' % (J, wave), lambda s: [s] * (J + 1), build)


def wpt1d_fwd(J, wave):
    h = W1.ana_taps(wave)

    def build(dev, dtype):
        m = W1.modules(dev, wave, J)[0]
        return (lambda x: [m(x)]), (lambda x: [W1.tree_ref(x, h, J)])
    t = _tf('WPT1DForward(J=%d, %s, periodization)' % (J, wave), lambda s: [s], build, J == 1)
    t.grad_ref = lambda xs, cs: [W1.transposed_ref(cs[0], h, xs[0].shape[-1])]
    return t


def wpt1d_inv(J, wave):
    g = W1.syn_taps(wave)

    def build(dev, dtype):
        m = W1.modules(dev, wave, J)[1]
        return (lambda y: [m(y)]), (lambda y: [W1.tree_inv_ref(y, g)])
    return _tf('WPT1DInverse(J=%d, %s, periodization)' % (J, wave), lambda s: [tuple(s[:-1]) + (2 ** J, s[-1] >> J)], build)


def _dt1d_shapes(J, s):
    yl, yh = D1.fwd_ref(np.zeros((1, 1, s[-1])), J, D1.taps('near_sym_a', 'qshift_a'))
    return [tuple(s[:-1]) + yl.shape[2:]] + [tuple(s[:-1]) + h.shape[2:] for h in yh]


def dt1d_fwd(J, biort='near_sym_a', qshift='qshift_a'):
    t = D1.taps(biort, qshift, f32=True)

    def build(dev, dtype):
        m = D1.modules(dev, biort, qshift, J)[0]

        def run(x):
            yl, yh = m(x)
            return [yl] + list(yh)

        def oracle(x):
            yl, yh = D1.fwd_ref(x, J, t)
            return [yl] + list(yh)
        return run, oracle
    tf = _tf('DTCWT1DForward(J=%d, %s, %s)' % (J, biort, qshift), lambda s: [s], build, bound=close_bound)
    tf.grad_ref = lambda xs, cs: [D1.fwd_grad_ref(cs[0], list(cs[1:]), xs[0].shape[-1], t)]
    return tf


def dt1d_inv(J, biort='near_sym_a', qshift='qshift_a'):
    t = D1.taps(biort, qshift, syn=True, f32=True)

    def build(dev, dtype):
        m = D1.modules(dev, biort, qshift, J)[1]
        return (lambda yl, *yh: [m((yl, list(yh)))]), (lambda yl, *yh: [D1.inv_ref(yl, list(yh), t)])
    return _tf('DTCWT1DInverse(J=%d, %s, %s)' % (J, biort, qshift), lambda s: _dt1d_shapes(J, s), build, bound=close_bound)


def scat1d(biort='near_sym_a'):
    def build(dev, dtype):
        m = C1.layer(dev, biort)
        taps = C1.taps_of(m)
        build.taps = taps
        return (lambda x: [m(x)]), (lambda x: [C1.fwd_ref(x, taps, C1.BIAS)[0]])
    tf = _tf('ScatLayer1D(%s)' % biort, lambda s: [s], build, bound=close_bound)
    tf.grad_ref = lambda xs, cs: [C1.bwd_ref(cs[0], C1.fwd_ref(xs[0], build.taps, C1.BIAS)[1], build.taps, xs[0].shape[-1])]
    return tf


def dwt3d_fwd(J, wave, mode):
    def build(dev, dtype):
        m = D3.modules(dev, wave, J, mode, dtype)[0]
        bk = D3.banks(wave, f32=dtype != F64)

        def run(x):
            yl, yh = m(x)
            return [yl] + list(yh)

        def oracle(x):
            yl, yh = D3.fwd_ref(x, J, bk, mode)
            return [yl] + list(yh)
        return run, oracle
    return _tf('DWT3DForward(J=%d, %s, %s)' % (J, wave, mode), lambda s: [s], build, bound=close_bound)


def dwt3d_inv(J, wave, mode):
    def shapes(s):
        yl, yh = D3.fwd_ref(np.zeros((1, 1) + tuple(s[2:])), J, D3.banks(wave), mode)
        return [tuple(s[:2]) + yl.shape[2:]] + [tuple(s[:2]) + h.shape[2:] for h in yh]

    def build(dev, dtype):
        m = D3.modules(dev, wave, J, mode, dtype)[1]
        bk = D3.banks(wave, syn=True, f32=dtype != F64)
        return (lambda yl, *yh: [m((yl, list(yh)))]), (lambda yl, *yh: [D3.inv_ref(yl, list(yh), bk, mode)])
    return _tf('DWT3DInverse(J=%d, %s, %s)' % (J, wave, mode), shapes, build, bound=close_bound)


def depth_level(wave, mode):
    """The depth level of the 3-D analysis on its own (lowlevel._depth_analysis): ll (N, D, H', W') and highs (N, D, 3, H', W') of
    a 2-D level on the D planes of one volume -> yl (N, 1, D', H', W'), yh (N, 1, 7, D', H', W').  `inner` of the depth launcher is
    H' W': through DWT3DForward it could only be approached with planes of 2**31 elements."""
    hn = D3.taps(wave, f32=True)

    def build(dev, dtype):
        h = D3.tap_tensors(wave, dev)
        m = dwl.mode_to_int(mode)

        def oracle(ll, highs):
            srcs = [ll[:, None]] + [highs[:, None, :, b] for b in range(3)]
            bands = [wo.afb1d(v, hn[0], hn[1], mode, axis=2) for v in srcs]
            return [bands[0][0], np.stack([b[0] for b in bands[1:]] + [b[1] for b in bands], axis=2)]
        return (lambda ll, highs: list(dwl._depth_analysis(ll, highs, 1, h[0], h[1], m))), oracle
    return _tf('depth level(%s, %s)' % (wave, mode), lambda s: [tuple(s), (s[0], s[1], 3, s[2], s[3])], build, True, bound=close_bound)


def wpt2d_fwd(J, wave, mode):
    def build(dev, dtype):
        m = P2.modules(dev, wave, J, mode, dtype)[0]
        h = P2.taps(wave, f32=dtype != F64)
        return (lambda x: [m(x)]), (lambda x: [P2.fwd_ref(x, J, h, mode)])
    tf = _tf('WPT2DForward(J=%d, %s, %s)' % (J, wave, mode), lambda s: [s], build, bound=close_bound)
    tf.grad_ref = lambda xs, cs: [P2.fwd_grad_ref(cs[0], P2.level_sizes(xs[0].shape[2:], J, P2.ntaps(wave), mode), P2.taps(wave, f32=True), mode)]
    return tf


def wpt2d_inv(J, wave, mode):
    def shapes(s):
        hw = P2.level_sizes(s[2:], J, P2.ntaps(wave), mode)[-1]
        return [tuple(s[:2]) + (4 ** J,) + tuple(hw)]

    def build(dev, dtype):
        m = P2.modules(dev, wave, J, mode, dtype)[1]
        g = P2.taps(wave, syn=True, f32=dtype != F64)
        return (lambda y: [m(y)]), (lambda y: [P2.inv_ref(y, g, mode)])
    return _tf('WPT2DInverse(J=%d, %s, %s)' % (J, wave, mode), shapes, build, bound=close_bound)


def afb1d_prim(wave, mode, dim):
    """lowlevel.afb1d along `dim` of a 4-D tensor: (N, 2C, ..) with the lowpass and the highpass of a channel side by side"""
    w = F.Wavelet(wave)
    h = F.dwt_analysis_taps(wave)

    def build(dev, dtype):
        return (lambda x: [dwl.afb1d(x, w.dec_lo, w.dec_hi, mode=mode, dim=dim)]), \
               (lambda x: [np.concatenate(wo.afb1d(x, h[0], h[1], mode, axis=dim), axis=1)])
    return _tf('afb1d(%s, %s, dim=%d)' % (wave, mode, dim), lambda s: [s], build, True)


def sfb1d_prim(wave, mode, dim):
    w = F.Wavelet(wave)
    g = F.dwt_synthesis_taps(wave)
    L = len(g[0])

    def shapes(s):
        k = list(s)
        k[dim] = V._klen(s[dim], L, mode)
        return [tuple(k)] * 2

    def build(dev, dtype):
        return (lambda lo, hi: [dwl.sfb1d(lo, hi, w.rec_lo, w.rec_hi, mode=mode, dim=dim)]), \
               (lambda lo, hi: [wo.sfb1d(lo, hi, g[0], g[1], mode, axis=dim)])
    return _tf('sfb1d(%s, %s, dim=%d)' % (wave, mode, dim), shapes, build)


def filt_prim(dim):
    """dtcwt.lowlevel.colfilter (dim 2) / rowfilter (dim 3): one band as large as the input - the only single-axis call whose
    WlCorr1d launch has 2**31 outputs below 2**32 elements (afb1d's launch makes both bands in one thread)"""
    h32 = np.asarray(F.dtcwt_forward_taps('near_sym_a', 'qshift_a')[0], dtype=np.float32).ravel()

    def build(dev, dtype):
        hp = dtl.prep_filt(h32, 1).to(dev)
        fn = dtl.colfilter if dim == 2 else dtl.rowfilter
        return (lambda x: [fn(x, hp)]), (lambda x: [wo.colfilter(x, h32.astype(np.float64), axis=dim)])
    return _tf('%s(near_sym_a h0o)' % ('colfilter' if dim == 2 else 'rowfilter'), lambda s: [s], build, True)


# ---- part A: the table -----------------------------------------------------------------------------------------------------------
class Row(object):
    """One kernel route on `count` planes of `plane` (the shape behind (N, C = 1)).  `expect`: name prefixes, each of which must
    start a launch of the forward call, in this order ('prefix...suffix' also fixes the end of the name); `expect_bwd` likewise for the launches of torch.autograd.grad (rows with
    `grad`).  `emu_plane`: a smaller plane for the emulator where the chip's plane would take it minutes.  `raw`: the armed
    fallbacks and auxiliary launches count as launches too."""

    def __init__(self, name, family, tf, plane, dtype, expect, pin=None, grad=False, expect_bwd=(), emu_plane=None, P=5, raw=False):
        self.name, self.family, self.tf, self.plane, self.dtype, self.pin, self.grad, self.P = name, family, tf, tuple(plane), dtype, pin, grad, P
        self.expect = [expect] if isinstance(expect, str) else list(expect)
        self.expect_bwd = [expect_bwd] if isinstance(expect_bwd, str) else list(expect_bwd)
        self.emu_plane, self.raw = (tuple(emu_plane) if emu_plane else None), raw

    def __repr__(self):
        return self.name

    def plane_on(self, backend):
        return self.emu_plane if backend == 'emu' and self.emu_plane else self.plane


def _table():
    T = []

    def add(name, *a, **kw):
        assert all(r.name != name for r in T), name
        T.append(Row(name, *a, **kw))

    ST, SR, GEN = V.STRIPS, V.STREAM, V.GENERIC
    SR1 = {'STREAM_FORCE': True, 'FUSED_LEVELS': False}      # (one level, many planes: the fused kernels would be asked first)
    NS = {'FUSED_LEVELS': False, 'no_stream': 1}            # (one launch per level, and planes that fill the chip stay off the strip kernels)
    tn = V._T
    # -- 2-D DWT -------------------------------------------------------------------------------------------------------------
    for dt in (F32, F16):
        add('small-fwd-' + V._n(dt), 'dwt2d', V.dwt_fwd(2, 'db2', 'symmetric'), (66, 70), dt, 'WlAfbSmall<', grad=True, expect_bwd='WlSfbSmall<')
        add('small-inv-' + V._n(dt), 'dwt2d', V.dwt_inv(2, 'db2', 'symmetric'), (66, 70), dt, 'WlSfbSmall<', grad=True, expect_bwd='WlAfbSmall<')
    add('rows-fwd-db4-sym-f32', 'dwt2d', V.dwt_fwd(3, 'db4', 'symmetric'), (250, 262), F32, 'WlAfbRows<float', pin=ST, grad=True)
    add('rows-inv-db4-sym-f32', 'dwt2d', V.dwt_inv(3, 'db4', 'symmetric'), (250, 262), F32, 'WlSfbRows<float', pin=ST, grad=True)
    add('rows-fwd-db4-per-f16', 'dwt2d', V.dwt_fwd(3, 'db4', 'periodization'), (248, 264), F16, 'WlAfbRows<_Float16', pin=ST)
    add('rows-inv-db4-per-f16', 'dwt2d', V.dwt_inv(3, 'db4', 'periodization'), (248, 264), F16, 'WlSfbRows<_Float16', pin=ST)
    # (the lattice variants: the examination of the banks in front, the armed two-bank fallback behind)
    add('rows-fwd-db8-lattice-f32', 'dwt2d', V.dwt_fwd(3, 'db8', 'symmetric'), (250, 262), F32, ['WlTapPrep', 'WlAfbRows<float, 16', 'WlAfbRows<float...(armed fallback)'], pin=ST, raw=True)
    add('rows-inv-db8-lattice-f32', 'dwt2d', V.dwt_inv(3, 'db8', 'symmetric'), (250, 262), F32, ['WlTapPrep', 'WlSfbRows<float, 16', 'WlSfbRows<float...(armed fallback)'], pin=ST, raw=True)
    add('strip-fwd-db8-per-f16', 'dwt2d', V.dwt_fwd(1, 'db8', 'periodization'), (2040, 2056), F16, 'WlAfbStrip<', pin=SR, emu_plane=(40, 704))
    add('strip-inv-db8-per-f16', 'dwt2d', V.dwt_inv(1, 'db8', 'periodization'), (2040, 2056), F16, 'WlSfbStrip<', pin=SR, emu_plane=(40, 704))
    add('strip-fwd-db4-sym-f32', 'dwt2d', V.dwt_fwd(1, 'db4', 'symmetric'), (250, 518), F32, 'WlAfbStrip<', pin=SR1, emu_plane=(40, 518))
    add('strip-inv-db4-sym-f32', 'dwt2d', V.dwt_inv(1, 'db4', 'symmetric'), (250, 518), F32, 'WlSfbStrip<', pin=SR1, emu_plane=(40, 518))
    add('tile-fwd-f32', 'dwt2d', V.dwt_fwd(1, 'db2', 'symmetric'), (70, 132), F32, 'WlAfbTile<', pin=NS)
    add('tile-inv-f32', 'dwt2d', V.dwt_inv(1, 'db2', 'symmetric'), (70, 132), F32, 'WlSfbTile<', pin=NS)
    add('generic-fwd-f64', 'dwt2d', V.dwt_fwd(1, 'db2', 'symmetric'), (70, 132), F64, 'WlAfb2dTile<double>', pin=GEN)
    add('generic-inv-f64', 'dwt2d', V.dwt_inv(1, 'db5', 'zero'), (70, 132), F64, 'WlSfb2dTile<double>', pin=GEN)
    # -- DTCWT and scattering --------------------------------------------------------------------------------------------------
    add('dt-fwd-strip-a-f32', 'dtcwt', V.dt_fwd(3), (72, 264), F32, 'WlDtFwd12Strip<float, 5, 7, 10', pin=SR, grad=True)
    add('dt-inv-strip-a-f32', 'dtcwt', V.dt_inv(3), (72, 264), F32, 'WlDtInv21Strip<float', pin=SR, grad=True)
    add('dt-fwd-strip-a-f16', 'dtcwt', V.dt_fwd(3), (72, 264), F16, 'WlDtFwd12Strip<_Float16, 5, 7, 10', pin=SR)
    add('dt-inv-strip-a-f16', 'dtcwt', V.dt_inv(3), (72, 264), F16, 'WlDtInv21Strip<_Float16', pin=SR)
    add('dt-fwd-strip-b-f32', 'dtcwt', V.dt_fwd(2, 'near_sym_b', 'qshift_b'), (72, 264), F32, 'WlDtFwd12Strip<float, 13, 19', pin=SR)
    add('dt-inv-strip-b-f32', 'dtcwt', V.dt_inv(2, 'near_sym_b', 'qshift_b'), (72, 264), F32, ['WlDtInv2Strip<float, 14', 'WlDtInv1Strip<float, 19, 13'], pin=SR)
    add('dt-fwd1-small-f32', 'dtcwt', V.dt_fwd(1), (32, 32), F32, 'WlDtFwd1Small<float')
    add('dt-fwd-tile-f32', 'dtcwt', V.dt_fwd(2), (36, 44), F32, ['WlDtFwd1Tile<', 'WlDtFwd2Tile<'], pin={'no_stream': 1})
    add('dt-inv-tile-f32', 'dtcwt', V.dt_inv(2), (36, 44), F32, ['WlDtInv2Tile<', 'WlDtInv1Tile<'], pin={'no_stream': 1})
    lean = 'WlDtFwd12Strip<%s, 5, 7, 10, 1, 4, 2>'
    # (the lean level-1 kernel takes planes of up to 256 columns)
    add('scat-infer-f32', 'dtcwt', V.scat(), (72, 248), F32, lean % 'float')
    add('scat-train-f32', 'dtcwt', V.scat(), (72, 248), F32, 'WlDtFwd12Strip<float, 5, 7, 10', grad=True, expect_bwd='WlDtInv1Strip<float')
    add('scatj2-infer-f16', 'dtcwt', V.scatj2(), (72, 264), F16, 'WlDtFwd12Strip<_Float16')
    # -- 2-D stationary and non-separable ---------------------------------------------------------------------------------------
    # (two levels: 8 bytes out per byte in - with cotangents and the gradient that is past 48 GiB, so the backward pass runs on one)
    add('swt-fwd-f32', 'swt2d', V.swt_fwd(2, 'db2'), (21, 35), F32, ['WlSwtLevel<'] * 2)
    add('swt-fwd-j1-grad-f32', 'swt2d', V.swt_fwd(1, 'db2'), (21, 35), F32, 'WlSwtLevel<', grad=True, expect_bwd='WlSwtInvLevel<')
    add('swt-inv-f32', 'swt2d', V.swt_inv(2, 'db2'), (21, 35), F32, 'WlSwtInvLevel<')
    add('nonsep-afb-f32', 'swt2d', V.nonsep_afb('db2', 'symmetric'), (20, 24), F32, 'WlAfbNonsep<float>')
    add('nonsep-sfb-f32', 'swt2d', V.nonsep_sfb('db2', 'symmetric'), (20, 24), F32, 'WlSfbNonsep<float>')
    # -- single-axis primitives, float16, along H (inner > 1) and along W: every output passes 2**31 elements.  WlSynth1d (one thread
    #    per output) and the one-band WlCorr1d of colfilter / rowfilter then take their 64-bit index branch (wl_filt1d.h); afb1d's
    #    WlCorr1d makes both bands in a thread and stays on 32 bits until the pair has 2**32 elements
    for dim, tag in ((2, 'h'), (3, 'w')):
        add('afb1d-%s-f16' % tag, 'prim', afb1d_prim('db3', 'symmetric', dim), (66, 70), F16, 'WlCorr1d<')
        add('sfb1d-%s-f16' % tag, 'prim', sfb1d_prim('db3', 'symmetric', dim), (66, 70), F16, 'WlSynth1d<')
        add('filt-%s-f16' % tag, 'prim', filt_prim(dim), (66, 70), F16, 'WlCorr1d<')
    # -- 1-D ---------------------------------------------------------------------------------------------------------------------
    for dt in (F32, F16):
        n = V._n(dt)
        add('dwt1d-fwd-' + n, 'dwt1d', V.dwt1d_fwd(3, 'db4', 'symmetric'), (1001,), dt, 'WlDwt1dFused<' + tn[dt])
        add('dwt1d-inv-' + n, 'dwt1d', V.dwt1d_inv(3, 'db4', 'symmetric'), (1001,), dt, 'WlIdwt1dFused<' + tn[dt])
        add('swt1d-fwd-' + n, 'swt1d', swt1d_fwd(3, 'db4'), (1001,), dt, 'WlSwt1dFwd<', grad=dt == F32, expect_bwd='WlSwt1dAdj<')
        add('swt1d-inv-' + n, 'swt1d', swt1d_inv(3, 'db4'), (1001,), dt, 'WlSwt1dAdj<')
        add('wpt1d-fwd-j3-' + n, 'wpt1d', wpt1d_fwd(3, 'db4'), (1000,), dt, 'WlWpt1dAfb<', grad=dt == F32, expect_bwd='WlWpt1dSfb<')
        add('wpt1d-inv-j3-' + n, 'wpt1d', wpt1d_inv(3, 'db4'), (1000,), dt, 'WlWpt1dSfb<')
        add('dt1d-fwd-' + n, 'dt1d', dt1d_fwd(3), (2008,), dt, 'WlDt1dFwd<', grad=dt == F32, expect_bwd='WlDt1dInv<')
        add('dt1d-inv-' + n, 'dt1d', dt1d_inv(3), (2008,), dt, 'WlDt1dInv<')
        add('scat1d-infer-' + n, 'scat1d', scat1d(), (1501,), dt, 'WlScat1dFwd<')
    # (six levels: the second launch runs over eight times the rows)
    add('wpt1d-fwd-j6-f32', 'wpt1d', wpt1d_fwd(6, 'db4'), (4032,), F32, ['WlWpt1dAfb<', 'WlWpt1dAfb<'], grad=True, expect_bwd='WlWpt1dSfb<')
    add('wpt1d-inv-j6-f32', 'wpt1d', wpt1d_inv(6, 'db4'), (4032,), F32, ['WlWpt1dSfb<', 'WlWpt1dSfb<'])
    add('scat1d-train-f32', 'scat1d', scat1d(), (1501,), F32, 'WlScat1dFwd<', grad=True, expect_bwd='WlScat1dBwd<')
    # -- 3-D and packets ---------------------------------------------------------------------------------------------------------
    # (the depth kernels see inner = H' W' elements per depth plane: a whole number of 16-byte pieces, and not)
    add('dwt3d-fwd-vec-f32', 'dwt3d', dwt3d_fwd(1, 'db4', 'symmetric'), (12, 20, 24), F32, 'WlAfbDepth<')
    add('dwt3d-inv-vec-f32', 'dwt3d', dwt3d_inv(1, 'db4', 'symmetric'), (12, 20, 24), F32, 'WlSfbDepth<')
    add('dwt3d-fwd-scalar-f32', 'dwt3d', dwt3d_fwd(1, 'db4', 'symmetric'), (11, 9, 13), F32, 'WlAfbDepth<')
    add('dwt3d-inv-scalar-f32', 'dwt3d', dwt3d_inv(1, 'db4', 'symmetric'), (11, 9, 13), F32, 'WlSfbDepth<')
    add('wpt2d-fwd-per-f32', 'wpt2d', wpt2d_fwd(3, 'db4', 'periodization'), (72, 200), F32, 'WlWptAfb', grad=True, expect_bwd='WlWptSfb')
    add('wpt2d-inv-per-f32', 'wpt2d', wpt2d_inv(3, 'db4', 'periodization'), (72, 200), F32, 'WlWptSfb')
    add('wpt2d-fwd-sym-f32', 'wpt2d', wpt2d_fwd(3, 'db4', 'symmetric'), (37, 61), F32, ['WlWptAfb'] * 3, grad=True, expect_bwd='WlWptSfb')
    add('wpt2d-inv-sym-f32', 'wpt2d', wpt2d_inv(3, 'db4', 'symmetric'), (37, 61), F32, ['WlWptSfb'] * 3)
    return T


ROWS = _table()
BY_NAME = {r.name: r for r in ROWS}
FAMILIES = sorted(set(r.family for r in ROWS))


# ---- the arithmetic of a row ------------------------------------------------------------------------------------------------------
class Plan(object):
    """in_planes / out_planes: elements of one plane of every input / output; count: the planes; need: bytes of inputs, outputs,
    cotangents and gradients (rows with `grad`) and one comparison chunk."""


def _shape_of(row, backend, count):
    return (count, 1) + row.plane_on(backend)


_OUT_PLANES = {}


def out_plane_shapes(row, backend='gpu'):
    """The shape of one plane of every output: what the row's oracle makes of one plane of zeros."""
    key = (row.name, backend)
    if key not in _OUT_PLANES:
        _, oracle = row.tf.build('cpu', row.dtype)
        refs = oracle(*[np.zeros(s) for s in row.tf.shapes(_shape_of(row, backend, 1))])
        _OUT_PLANES[key] = [r.shape[1:] for r in refs]
    return _OUT_PLANES[key]


def prime_ok(plane_bytes, P, dtype, b32=B32):
    """no threshold is a whole multiple of P * plane bytes: a wrapped address cannot land on an equal plane"""
    return all(t % (P * plane_bytes) != 0 for _, t in thresholds(dtype, b32))


def plan(row, backend='gpu', count=None):
    es, P = esize(row.dtype), row.P
    p = Plan()
    p.in_planes = [int(np.prod(s[1:])) for s in row.tf.shapes(_shape_of(row, backend, 1))]
    p.out_planes = [int(np.prod(s)) for s in out_plane_shapes(row, backend)]
    if count is None:
        small = min(max(p.in_planes), max(p.out_planes)) * es
        count = -(-B32 // small) + SLACK
        while count % P == 0:
            count += 1
    p.count = count
    p.in_bytes, p.out_bytes = [count * n * es for n in p.in_planes], [count * n * es for n in p.out_planes]
    p.need = (sum(p.in_bytes) + sum(p.out_bytes)) * (2 if row.grad else 1) + 3 * 8 * CHUNK_ELEMS
    return p


def check_plan(row, p, b32=B32):
    """The largest input and the largest output lie `SLACK` planes past the threshold (2**32 bytes; for a 2-byte type that is
    2**31 elements), P does not divide the plane count, and the prime condition holds for every tensor."""
    es = esize(row.dtype)
    for planes, total in ((p.in_planes, p.in_bytes), (p.out_planes, p.out_bytes)):
        k = int(np.argmax(planes))
        assert total[k] >= b32 + SLACK * planes[k] * es, (row.name, total[k], b32)
    assert p.count % row.P != 0, (row.name, p.count, row.P)
    for n in p.in_planes + p.out_planes:
        assert prime_ok(n * es, row.P, row.dtype, b32), (row.name, n, row.P)
    assert p.need <= MAX_NEED, (row.name, p.need)


# ---- running a row ------------------------------------------------------------------------------------------------------------
def _bound(tf, dtype, ref):
    top = float(np.abs(ref).max())
    fn = getattr(tf, 'bound', None) or rel_bound
    return fn(tf, dtype, top)


def _sync(dev):
    if str(dev) != 'cpu':
        torch.cuda.synchronize()


def _match(k, e):
    """a launch name against 'prefix' or 'prefix...suffix'"""
    pre, _, suf = e.partition('...')
    return k.startswith(pre) and k.endswith(suf)


def _has(ks, expect, what):
    """the expected names, in their order, each matching a launch behind the one its predecessor matched"""
    at = 0
    for e in expect:
        while at < len(ks) and not _match(ks[at], e):
            at += 1
        assert at < len(ks), (what, ks, expect)
        at += 1


def _launches(c0, raw):
    ks = pw.kernels_since(c0)
    return list(ks) if raw else _mutation_cases.primary(ks)


def _enough(need, dev):
    if str(dev) == 'cpu':
        return True
    free, _ = torch.cuda.mem_get_info()
    return free >= HEADROOM * need


def _prealloc(sizes, dev):
    """Blocks of these many bytes pass through the caching allocator once, so that the timed call finds them there: every case
    returns its memory to the device, and the first allocation of a multi-GiB block takes longer than the kernels."""
    if str(dev) != 'cpu':
        blocks = [torch.empty(int(n), dtype=torch.uint8, device=dev) for n in sizes]
        del blocks


def _judge(secs, moved, full):
    """the note for a case slower than ten times what its bytes take at 1 TB/s (cases under 1 GB are launch-bound: not judged)"""
    return ' - FINDING: more than ten times its bytes at 1 TB/s' if full and moved >= 1e9 and secs > 10 * moved / 1e12 else ''


def _device_grad_ref(row, dev, bases, cots):
    """The gradients of the P base planes (part B: of the short object) on the per-level tile path, as _view_cases.check_grad takes
    them - the engine's own kernels at a small size, which the families' suites hold against their oracles; no float64 oracle.  float64 numpy."""
    prev = dwl.FUSED_LEVELS
    dwl.FUSED_LEVELS = False
    ops.set_option('no_stream', 1)
    try:
        run, _ = row.tf.build(dev, row.dtype)
        xs = [b.clone().requires_grad_(True) for b in bases]
        c0 = pw.launch_count()
        ref = torch.autograd.grad(run(*xs), xs, grad_outputs=cots)
        k_ref = pw.kernels_since(c0)
    finally:
        ops.set_option('no_stream', 0)
        dwl.FUSED_LEVELS = prev
    assert not any('Strip' in k or 'Rows' in k for k in k_ref), k_ref
    return [V._npy(g) for g in ref]


def run_row(row, dev, count=None, seed=5):
    """One row: build the inputs from P base planes, run, synchronise, compare every plane of every output (and, rows with
    `grad`, of every gradient) with the oracle of the base planes, assert the kernels.  `count`: a scaled-down plane count (the
    emulator); the thresholds of the reports scale with it.  Returns a dict of what it printed."""
    backend = V._backend_of(dev)
    full = count is None
    p = plan(row, backend, count)
    es, P = esize(row.dtype), row.P
    big = max(p.in_bytes + p.out_bytes)
    b32 = B32 if full else (P * big // p.count + big // p.count // 2) // 16 * 16
    if full:
        check_plan(row, p)
    if not _enough(p.need, dev):
        import pytest
        pytest.skip('%s needs %.1f GiB free' % (row.name, HEADROOM * p.need / 2 ** 30))
    ths = thresholds(row.dtype, b32)
    rng = np.random.RandomState(seed)
    shapes = row.tf.shapes(_shape_of(row, backend, P))
    host = [torch.tensor(rng.randn(*s)).to(row.dtype) for s in shapes]
    res = {'row': row.name, 'count': p.count, 'in_bytes': p.in_bytes, 'out_bytes': p.out_bytes, 'need': p.need, 'errs': []}
    print('%s %s: %d planes of %s %s, inputs %s bytes, outputs %s bytes, need %.2f GiB'
          % (row.name, row.tf.name, p.count, row.plane_on(backend), row.dtype, p.in_bytes, p.out_bytes, p.need / 2 ** 30))
    ops._FUSED_DECLINED.clear()
    xs = outs = cots = grads = refs_d = bases = None
    try:
        with V.pinned(row.pin):
            run, oracle = row.tf.build(dev, row.dtype)
            refs = oracle(*[V._npy(t) for t in host])
            bases = [t.to(dev) for t in host]
            xs = [periodic_planes(b, p.count) for b in bases]
            if row.grad:
                xs = [x.requires_grad_(True) for x in xs]
            cbase = [torch.tensor(rng.randn(*r.shape)).to(row.dtype).to(dev) for r in refs]
            # (before the clock starts: the code objects are loaded, autograd has run once, the outputs' blocks are in the allocator)
            if row.grad:
                wb = [b.clone().requires_grad_(True) for b in bases]
                torch.autograd.grad(run(*wb), wb, grad_outputs=cbase)
            else:
                run(*bases)
            _prealloc(p.out_bytes, dev)
            _sync(dev)
            t0 = time.time()
            c0 = pw.launch_count()
            outs = run(*xs)
            _sync(dev)                       # a launch that went out of bounds surfaces here, in the case that caused it
            secs = time.time() - t0
            ks = _launches(c0, row.raw)
            print('    launches %s, %.3f s' % (ks, secs))
            assert len(outs) == len(refs), (len(outs), len(refs))
            for i, (o, ref) in enumerate(zip(outs, refs)):
                assert o.dtype == row.dtype and tuple(o.shape) == (p.count,) + ref.shape[1:], (i, o.dtype, tuple(o.shape), ref.shape)
                assert o.numel() * es == p.out_bytes[i]
                bound = _bound(row.tf, row.dtype, ref)
                err = compare_planes(o.detach(), torch.tensor(ref).to(dev), P, bound, '%s output %d' % (row.name, i), ths)
                print('    out %d %s, %d elements, %d bytes: max err %.3e, bound %.3e' % (i, tuple(o.shape), o.numel(), o.numel() * es, err, bound))
                res['errs'].append((err, bound))
            kb = []
            if row.grad:
                gref_fn = getattr(row.tf, 'grad_ref', None)
                if gref_fn is not None:
                    grefs = gref_fn([V._npy(t) for t in host], [V._npy(c) for c in cbase])
                else:
                    grefs = _device_grad_ref(row, dev, bases, cbase)
                cots = [periodic_planes(c, p.count) for c in cbase]
                _prealloc(p.in_bytes, dev)
                _sync(dev)
                t0 = time.time()
                c0 = pw.launch_count()
                grads = torch.autograd.grad(outs, xs, grad_outputs=cots)
                _sync(dev)
                bsecs = time.time() - t0
                kb = _launches(c0, row.raw)
                print('    backward launches %s, %.3f s' % (kb, bsecs))
                secs += bsecs
                for i, (g, ref) in enumerate(zip(grads, grefs)):
                    assert g.dtype == row.dtype and tuple(g.shape) == tuple(xs[i].shape), (i, g.dtype, tuple(g.shape))
                    bound = _bound(row.tf, row.dtype, ref)
                    err = compare_planes(g, torch.tensor(ref).to(dev), P, bound, '%s gradient %d' % (row.name, i), ths)
                    print('    grad %d %s: max err %.3e, bound %.3e' % (i, tuple(g.shape), err, bound))
                    res['errs'].append((err, bound))
        moved = (sum(p.in_bytes) + sum(p.out_bytes)) * (2 if row.grad else 1)
        res.update(kernels=ks, kernels_bwd=kb, seconds=secs)
        print('    %.3f s for %.2f GB%s' % (secs, moved / 1e9, _judge(secs, moved, full)))
        if backend == 'gpu':
            _has(ks, row.expect, row.name)
            if row.grad:
                _has(kb, row.expect_bwd, row.name + ' backward')
        return res
    finally:
        del xs, outs, cots, grads, bases
        if str(dev) != 'cpu':
            torch.cuda.empty_cache()


# ---- part B: one plane / row at the top of an envelope ------------------------------------------------------------------------------
class Edge(object):
    """One object within 1 % below a launcher's limit, or (`over`) about 1 % above it.  `shape`: the shape handed to `tf.shapes`,
    every input periodic along its axis of `in_axes` (default: `axis`) with the period T scaled to its level; `short`: the samples
    of the short object along `axis`; `L`, `J`: taps and levels (`min_short_len`); `periods(T)`: for every output, {axis: its
    period along it}; `measure(shape)`: the sides whose product the guard bounds by `limit_elems`; `out_ratio`: bytes of the outputs
    per byte of the inputs (the memory need).  Below the limit `expect` names what runs.  Above it `over` says what must happen:
    'other' - other kernels, the same values - or the exception class the package documents for it.  `cols`: the transform gets the
    first `cols` columns of the plane as a view - `shape` is then the parent, whose row pitch the guard bounds.  `grad`: one
    torch.autograd.grad with periodic cotangents, against the gradient of the short object on the per-level tile kernels."""

    def __init__(self, name, family, tf, shape, dtype, axis, T, short, L, J, periods, expect, in_axes=None, pin=None, over=None,
                 limit_elems=2 ** 30, measure=None, out_ratio=1.0, guard='', cols=None, grad=False, expect_bwd=()):
        self.name, self.family, self.tf, self.shape, self.dtype, self.axis, self.T, self.short = name, family, tf, tuple(shape), dtype, axis, T, short
        self.L, self.J, self.periods, self.pin, self.over, self.limit_elems, self.guard, self.out_ratio = L, J, periods, pin, over, limit_elems, guard, out_ratio
        self.expect = [expect] if isinstance(expect, str) else list(expect)
        self.in_axes = list(in_axes) if in_axes else [axis]
        self.cols, self.grad = cols, grad
        self.expect_bwd = [expect_bwd] if isinstance(expect_bwd, str) else list(expect_bwd)
        self.measure = measure or (lambda s: tuple(s[2:]))

    def __repr__(self):
        return self.name


def edge_shapes(edge, n, cut=True):
    """(the shapes of the inputs, the shape handed to tf.shapes) with n samples along the edge's axis; `cut`: the other axes
    behind (N, C) at most 72 samples (the emulator, the host oracles)."""
    s = list(edge.shape)
    s[edge.axis] = n
    if cut:
        s = s[:2] + [k if a + 2 == edge.axis else min(k, edge.cols + 16 if edge.cols else 72) for a, k in enumerate(s[2:])]
    return [tuple(v) for v in edge.tf.shapes(tuple(s))], tuple(s)


def edge_period_shapes(edge, shapes, n, T):
    """the shape of one period of every input: T scaled by the input's length along its axis over n"""
    out = []
    for s, a in zip(shapes, edge.in_axes):
        assert s[a] * T % n == 0, (edge.name, s, a, n, T)
        out.append(tuple(s[:a]) + (s[a] * T // n,) + tuple(s[a + 1:]))
    return out


def edge_need(edge, shape):
    ins = sum(int(np.prod(s)) for s in edge.tf.shapes(tuple(shape))) * esize(edge.dtype)
    return int(ins * (1 + edge.out_ratio)) + 3 * 8 * CHUNK_ELEMS


def _edges():
    E = []

    def add(name, *a, **kw):
        assert all(e.name != name for e in E), name
        E.append(Edge(name, *a, **kw))

    def both(name, family, tf, shape, over_shape, *a, **kw):
        """the object below the limit and its twin about 1 % above it"""
        over = kw.pop('over')
        over_expect = kw.pop('over_expect', ())
        over_bwd = kw.pop('over_expect_bwd', ())
        add(name, family, tf, shape, *a, **kw)
        kw['expect'] = over_expect
        if kw.get('grad'):
            kw['expect_bwd'] = over_bwd
        add(name + '-over', family, tf, over_shape, *a, over=over, **kw)

    T, SH = 208, 624
    A30, A30o = (1, 1, 208 * 625, 8248), (1, 1, 208 * 631, 8248)          # H W: 0.14 % below 2**30, 0.8 % above
    A29, A29o = (1, 1, 208 * 313, 8240), (1, 1, 208 * 316, 8240)          # likewise 2**29
    lv = lambda axis, *js: (lambda t: [{axis: t >> j} for j in js])   # noqa: E731
    # -- 2-D DWT (wl_api.inc:140, :253, wl_rows_api.inc:105: H W < 2**30) ------------------------------------------------------
    per3 = lambda t: [{2: t >> 3}, {3: t >> 1}, {3: t >> 2}, {3: t >> 3}]   # noqa: E731
    fw3, iv3 = V.dwt_fwd(3, 'db4', 'periodization'), V.dwt_inv(3, 'db4', 'periodization')
    both('dwt2d-fwd-per-j3-f32', 'dwt2d', fw3, A30, A30o, F32, 2, T, SH, 8, 3, per3, expect=['WlAfbTile<float', 'WlAfbStrip<float', 'WlAfbTile<float'],
         over='other', over_expect=['WlAfb2dTile<float>', 'WlAfbStrip<float', 'WlAfbTile<float'],
         guard='wl_api.inc wl_afb2d_multi: H W < 2^30')
    both('dwt2d-fwd-per-j3-f16', 'dwt2d', fw3, A30, A30o, F16, 2, T, SH, 8, 3, per3, expect=['WlAfbTile<_Float16', 'WlAfbStrip<_Float16', 'WlAfbTile<_Float16'],
         over='other', over_expect='WlAfb2dTile<_Float16>', guard='wl_api.inc wl_afb2d_multi: H W < 2^30')
    both('dwt2d-inv-per-j3-f32', 'dwt2d', iv3, A30, A30o, F32, 2, T, SH, 8, 3, lv(2, 0), in_axes=[2, 3, 3, 3], expect=['WlSfbTile<float'] * 3, over='other',
         over_expect=['WlSfbTile<float', 'WlSfbTile<float', 'WlSfb2dTile<float>'], guard='wl_api.inc wl_sfb2d_multi: OH OW < 2^30')
    both('dwt2d-inv-per-j3-f16', 'dwt2d', iv3, A30, A30o, F16, 2, T, SH, 8, 3, lv(2, 0), in_axes=[2, 3, 3, 3], expect=['WlSfbTile<_Float16'] * 3, over='other',
         over_expect='WlSfb2dTile<_Float16>', guard='wl_api.inc wl_sfb2d_multi: OH OW < 2^30')
    # (the fused multi-level analysis - wl_rows_api.inc:105: H * row pitch < 2**30 - takes narrow planes of up to ~3000 rows, its schedule
    #  table's size: the first 256 columns, as a view, of 2912 rows whose pitch puts the product at the limit)
    both('dwt2d-fwd-rows-pitch-f32', 'dwt2d', fw3, (1, 1, 2912, 368200), (1, 1, 2912, 372000), F32, 2, T, SH, 8, 3, per3, expect='WlAfbRows<float',
         over='other', over_expect=['WlAfb2dTile<float>', 'WlAfbRows<float'], pin=V.STRIPS, cols=256, guard='wl_rows_api.inc wl_afb_rows_launch: H x_rs < 2^30')
    both('dwt2d-fwd-sym-j1-f32', 'dwt2d', V.dwt_fwd(1, 'db4', 'symmetric'), A30, A30o, F32, 2, T, SH, 8, 1, lambda t: [{2: t >> 1}, {3: t >> 1}],
         expect='WlAfbTile<float, 8>', over='other', over_expect='WlAfb2dTile<float>', guard='wl_api.inc wl_afb2d_multi: H W < 2^30')
    # -- DTCWT and ScatLayer (wl_api.inc:671, :745: H W < 2**30; the streaming kernels end at 2**28) -------------------------------------
    both('dt2d-fwd-j2-f32', 'dtcwt', V.dt_fwd(2), A30, A30o, F32, 2, T, SH, 10, 2, lambda t: [{2: t >> 1}, {3: t >> 1}, {3: t >> 2}],
         expect=['WlDtFwd1Tile<float', 'WlDtFwd2Tile<float'], over='other', over_expect=['WlDtFwd1<float>', 'WlDtFwd2<float>'], out_ratio=4.1, guard='wl_api.inc wl_dtcwt_fwd1 / fwd2: H W < 2^30')
    both('dt2d-inv-j2-f32', 'dtcwt', V.dt_inv(2), A30, A30o, F32, 2, T, SH, 10, 2, lv(2, 0), in_axes=[2, 3, 3], expect=['WlDtInv2Tile<float', 'WlDtInv1Tile<float'], over='other',
         over_expect=['WlDtInv2<float>', 'WlDtInv1<float>'], out_ratio=0.25, guard='wl_api.inc wl_dtcwt_inv1 / inv2: H W < 2^30')
    both('scat2d-f32', 'dtcwt', V.scat(), A30, A30o, F32, 2, T, SH, 7, 1, lv(2, 1), expect='WlDtFwd1Tile<float, 5, 7>', over='other', over_expect='WlDtFwd1<float>',
         out_ratio=1.75, guard='wl_api.inc wl_scat_fwd_level1: H W < 2^30')
    # (the training step: the forward that keeps what the backward needs, and one backward pass - wl_api.inc wl_scat_bwd_launch)
    both('scat2d-train-f32', 'dtcwt', V.scat(), A30, A30o, F32, 2, T, SH, 7, 1, lv(2, 1), expect='WlDtFwd1Tile<float, 5, 7>', over='other', over_expect='WlDtFwd1<float>',
         grad=True, expect_bwd='WlDtInv1Tile<float, 5, 7, 1>', over_expect_bwd='WlDtInv1<float>', out_ratio=4.6, guard='wl_api.inc wl_scat_bwd_launch: H W < 2^30')
    # -- 2-D stationary (wl_api.inc:1073, :1140) and packets (wl_wpt2d_api.inc:91, :106, :146: H W < 2**29) ---------------------------
    both('swt2d-fwd-j1-f32', 'swt2d', V.swt_fwd(1, 'db4'), A30, A30o, F32, 2, T, SH, 8, 1, lv(2, 0), expect='WlSwtLevel<', over='other',
         over_expect=['WlCorr1d<float>'] * 2, out_ratio=4.0, guard='wl_api.inc wl_swt2d_level: H W < 2^30')
    both('swt2d-inv-j1-f32', 'swt2d', V.swt_inv(1, 'db4'), A30, A30o, F32, 2, T, SH, 8, 1, lv(2, 0), expect='WlSwtInvLevel<float', over='other',
         over_expect='WlCorr1dAdj<float>', out_ratio=0.25, guard='wl_api.inc wl_iswt2d_level: H W < 2^30')
    both('wpt2d-fwd-per-j3-f32', 'wpt2d', wpt2d_fwd(3, 'db4', 'periodization'), A29, A29o, F32, 2, T, SH, 8, 3, lv(3, 3), expect=['WlWptAfb<float, 8, 2>', 'WlWptAfb<float, 8, 1>'],
         over='other', over_expect=['WlAfbTile<float', 'WlWptAfb<float, 8, 1>', 'WlWptAfb<float, 8, 1>'], limit_elems=2 ** 29, guard='wl_wpt2d_api.inc: H W < 2^29')
    both('wpt2d-inv-per-j3-f32', 'wpt2d', wpt2d_inv(3, 'db4', 'periodization'), A29, A29o, F32, 2, T, SH, 8, 3, lv(2, 0), in_axes=[3],
         expect='WlWptSfb<float, 8, 2>', over='other', over_expect=['WlWptSfb<float, 8, 1>'] * 3, limit_elems=2 ** 29, guard='wl_wpt2d_api.inc: OH OW < 2^30, Kh Kw < 2^29')
    # -- one long row (wl_wave1d_api.inc:17, ops.py wave1d envelope, wl_dtcwt1d_api.inc:53: len < 2**30; the 1-D scattering layer: 2**29) --
    T1, S1n = 1064, 4 * 1064
    R30, R30o, R29, R29o = (1, 1, T1 * 1008000), (1, 1, T1 * 1020000), (1, 1, T1 * 504000), (1, 1, T1 * 510000)
    row = dict(measure=lambda s: (s[2],))
    both('dwt1d-fwd-per-j3-f32', 'dwt1d', V.dwt1d_fwd(3, 'db4', 'periodization'), R30, R30o, F32, 2, T1, S1n, 8, 3, lv(2, 3, 1, 2, 3), expect=['WlCorr1d<float>'] * 3,
         over='other', over_expect=['WlCorr1d<float>'] * 3, guard='wl_api.inc wl_corr1d: no limit of its own at these lengths', **row)
    # (the fused 1-D analysis folds with wl_ext, whose period 2N must be an int; the single-axis kernel behind it folds in 64 bits)
    both('dwt1d-fwd-sym-j3-f32', 'dwt1d', V.dwt1d_fwd(3, 'db4', 'symmetric'), R30, R30o, F32, 2, T1, S1n, 8, 3, lv(2, 3, 1, 2, 3), expect='WlDwt1dFused<float',
         over='other', over_expect=['WlCorr1d<float>'] * 3, guard='wl_dwt1d_api.inc wl_dwt1d_analysis_fused: N < 2^30', **row)
    both('swt1d-fwd-j3-f32', 'swt1d', swt1d_fwd(3, 'db4'), R30, R30o, F32, 2, T1, S1n, 8, 3, lv(2, 0, 0, 0, 0), expect='WlSwt1dFwd<', over='other',
         over_expect='WlCorr1d', out_ratio=4.0, guard='ops.py wave1d envelope / wl_wave1d_api.inc: len < 2^30', **row)
    both('wpt1d-fwd-j3-f32', 'wpt1d', wpt1d_fwd(3, 'db4'), R30, R30o, F32, 2, T1, S1n, 8, 3, lv(3, 3), expect='WlWpt1dAfb<', over='other',
         over_expect='WlCorr1d', guard='ops.py wave1d envelope / wl_wave1d_api.inc: len < 2^30', **row)
    both('dt1d-fwd-j3-f32', 'dt1d', dt1d_fwd(3), R30, R30o, F32, 2, T1, S1n, 10, 3, lambda t: [{2: t >> 2}, {2: t >> 1}, {2: t >> 2}, {2: t >> 3}],
         expect='WlDt1dFwd<', over='other', over_expect='WlCorr1d', out_ratio=2.0, guard='wl_dtcwt1d_api.inc: N < 2^30', **row)
    both('scat1d-f32', 'scat1d', scat1d(), R29, R29o, F32, 2, T1, S1n, 7, 1, lv(2, 1), expect='WlScat1dFwd<', over='other', over_expect='WlDt1dFwd<',
         limit_elems=2 ** 29, guard='ops.py scat1d envelope / wl_wave1d_api.inc:142: n < 2^29', **row)
    # -- the depth level of the 3-D DWT (wl_dwt3d_api.inc wl_depth_check: inner = H' W' < 2**29), float16: four planes of a 2-D level ------
    both('dwt3d-depth-f16', 'dwt3d', depth_level('db2', 'periodization'), (1, 4) + A29[2:], (1, 4) + A29o[2:], F16, 2, T, SH, 4, 1,
         lambda t: [{3: t}, {4: t}], in_axes=[2, 3], expect='WlAfbDepth<_Float16', over='other', over_expect=['WlCorr1d<_Float16>'] * 4,
         limit_elems=2 ** 29, guard='wl_dwt3d_api.inc wl_depth_check: inner < 2^29')
    return E


EDGES = _edges()
EDGE_BY_NAME = {e.name: e for e in EDGES}
_FAULT_WORDS = ('illegal memory', 'HIP error', 'hipError', 'out of memory')


def run_edge(edge, dev, reps=None, seed=6):
    """One object of part B: the oracle on the short object, stretched, against the engine on the full one.  `reps`: a
    scaled-down number of periods (the emulator; the other axes are cut as well)."""
    backend = V._backend_of(dev)
    full = reps is None
    T = edge.T
    n = edge.shape[edge.axis] if full else reps * T
    assert n % T == 0 and edge.short % T == 0 and n > edge.short and edge.short >= min_short_len(edge.L, edge.J, T)
    shapes, shape = edge_shapes(edge, n, cut=not full)
    es = esize(edge.dtype)
    need = edge_need(edge, shape)
    assert need <= MAX_NEED, (edge.name, need)
    if not _enough(need, dev):
        import pytest
        pytest.skip('%s needs %.1f GiB free' % (edge.name, HEADROOM * need / 2 ** 30))
    rng = np.random.RandomState(seed)
    pshapes = edge_period_shapes(edge, shapes, n, T)
    if full:
        # no threshold is a whole number of periods of any input: an address wrapped by one never lands on an equal sample
        for s, q in zip(shapes, pshapes):
            pbytes = int(np.prod(q[edge.in_axes[shapes.index(s)]:])) * es
            assert all(t % pbytes for _, t in thresholds(edge.dtype)), (edge.name, q, pbytes)
    periods = [torch.tensor(rng.randn(*s)).to(edge.dtype) for s in pshapes]
    print('%s %s: inputs %s %s (%s; %d elements against %d), period %d along axis %d, short %d, need %.2f GiB'
          % (edge.name, edge.tf.name, shapes, edge.dtype, edge.guard, int(np.prod(edge.measure(shape))), edge.limit_elems, T, edge.axis, edge.short,
             need / 2 ** 30))
    xs = outs = None
    try:
        with V.pinned(edge.pin):
            run, oracle = edge.tf.build(dev, edge.dtype)
            cols = slice(None, edge.cols)
            refs = oracle(*[V._npy(tiled(q[..., cols], [edge.short // T], [a])) for q, a in zip(periods, edge.in_axes)])
            xs = [tiled(q.to(dev), [s[a] // q.shape[a]], [a]) for q, s, a in zip(periods, shapes, edge.in_axes)]
            assert [tuple(x.shape) for x in xs] == shapes
            xs = [x[..., cols] for x in xs]
            if edge.grad:
                xs = [x.requires_grad_(True) for x in xs]
            run(*[tiled(q.to(dev), [edge.short // T], [a])[..., cols].contiguous() for q, a in zip(periods, edge.in_axes)])      # (loads the code objects)
            _prealloc([sum(x.numel() for x in xs) * es * edge.out_ratio], dev)
            _sync(dev)
            t0 = time.time()
            c0 = pw.launch_count()
            raised = None
            try:
                outs = run(*xs)
                _sync(dev)                       # a launch that went out of bounds surfaces here, in the case that caused it
            except (RuntimeError, ValueError, NotImplementedError) as e:
                if edge.over is None or not full or any(w in str(e) for w in _FAULT_WORDS):
                    raise
                raised = e
            secs = time.time() - t0
            ks = _launches(c0, False)
            if raised is not None:
                print('    raised %s: %s' % (type(raised).__name__, str(raised)[:300]))
                assert edge.over != 'other' and isinstance(raised, edge.over), (edge.name, 'raised', type(raised).__name__, str(raised)[:300])
                return {'edge': edge.name, 'raised': type(raised).__name__, 'errs': []}
            assert edge.over in (None, 'other') or not full, (edge.name, 'ran where it must raise', ks)
            print('    launches %s, %.3f s' % (ks, secs))
            errs = []
            assert len(outs) == len(refs)
            for i, (o, ref, per) in enumerate(zip(outs, refs, edge.periods(T))):
                assert o.dtype == edge.dtype
                bound = _bound(edge.tf, edge.dtype, ref)
                err = compare_stretched(o.detach().contiguous(), torch.tensor(ref).to(dev), per, bound, '%s output %d' % (edge.name, i))
                print('    out %d %s, %d bytes: max err %.3e, bound %.3e' % (i, tuple(o.shape), o.numel() * es, err, bound))
                errs.append((err, bound))
            kb = []
            if edge.grad:
                # periodic cotangents; the reference: the gradient of the short object on the per-level tile kernels, stretched
                pers = [dict((a % o.dim(), v) for a, v in per.items()) for o, per in zip(outs, edge.periods(T))]
                cper = []
                for ref, per in zip(refs, pers):
                    (a, v), = per.items()
                    assert ref.shape[a] % v == 0
                    cper.append(torch.tensor(rng.randn(*(ref.shape[:a] + (v,) + ref.shape[a + 1:]))).to(edge.dtype).to(dev))
                short_in = [tiled(q.to(dev), [edge.short // T], [a]) for q, a in zip(periods, edge.in_axes)]
                short_cot = [tiled(c, [ref.shape[a] // c.shape[a]], [a]) for c, ref, per in zip(cper, refs, pers) for a in per]
                grefs = _device_grad_ref(edge, dev, short_in, short_cot)
                cots = [tiled(c, [o.shape[a] // c.shape[a]], [a]) for c, o, per in zip(cper, outs, pers) for a in per]
                _prealloc([x.numel() * es for x in xs], dev)
                _sync(dev)
                t0 = time.time()
                c0 = pw.launch_count()
                grads = torch.autograd.grad(outs, xs, grad_outputs=cots)
                _sync(dev)
                bsecs = time.time() - t0
                kb = _launches(c0, False)
                print('    backward launches %s, %.3f s' % (kb, bsecs))
                secs += bsecs
                for i, (g, ref, q, a) in enumerate(zip(grads, grefs, pshapes, edge.in_axes)):
                    bound = _bound(edge.tf, edge.dtype, ref)
                    err = compare_stretched(g.contiguous(), torch.tensor(ref).to(dev), {a: q[a]}, bound, '%s gradient %d' % (edge.name, i))
                    print('    grad %d %s: max err %.3e, bound %.3e' % (i, tuple(g.shape), err, bound))
                    errs.append((err, bound))
                del grads, cots
        moved = (sum(x.numel() for x in xs) * es + sum(o.numel() for o in outs) * es) * (2 if edge.grad else 1)
        assert moved + 3 * 8 * CHUNK_ELEMS <= 1.05 * need, (edge.name, moved, need)
        print('    %.3f s for %.2f GB%s' % (secs, moved / 1e9, _judge(secs, moved, full)))
        if backend == 'gpu':
            _has(ks, edge.expect, edge.name)
            _has(kb, edge.expect_bwd, edge.name + ' backward')
        return {'edge': edge.name, 'kernels': ks, 'errs': errs, 'seconds': secs}
    finally:
        del xs, outs
        if str(dev) != 'cpu':
            torch.cuda.empty_cache()
