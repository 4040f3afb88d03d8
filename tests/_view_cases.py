"""Every transform on tensor VIEWS - offset bases, crops, odd pitches, slices - shared by the emulator (CPU) and the GPU
test modules (tests/test_views_emu.py, tests/test_views_gpu.py).

The launchers hold predicates on pointer alignment (`(uintptr_t)x % 16`, `vec_ok`, `pair_ok`, `q4`, ...): each selects a
scalar branch inside a kernel or makes the launcher decline to another kernel.  A fresh allocation is aligned to 256 bytes,
so only a view reaches the other side of them.  A case hands a transform its inputs as views inside NaN-filled parents whose
first element lies on a 256-byte boundary, and `check` asserts
  (a) the outputs against the float64 oracle run on the view's own values (for 16-bit data: the rounded values);
  (b) no NaN in any output (a read outside the view meets the padding);
  (c) every parent bitwise what it was before the call, view and padding;
  (d) the launches (without armed fallbacks / auxiliary launches) start with the kernel family the case names;
  (e) the dense, aligned call launches the same kernels before and after the view call (no decline caused by a pointer is
      remembered for aligned tensors).
`check_grad` runs a case through torch.autograd.grad with a crop view as the input and offset(1) views as the gradient
outputs, against the gradient of dense aligned clones on the per-level tile path.

Bounds, each relative to the largest magnitude of the reference: float32 1e-5 (tests/test_dwt_routes_gpu.py), float16 4e-3
(tests/test_dwt_emu.py::test_half_precision_tile_kernels), bfloat16 as tests/_bf16_cases.py (4e-3 for a one-level forward,
3e-2 otherwise), float64 1e-12 (emulator only)."""
import contextlib

import numpy as np
import torch

import _bf16_cases
import _mutation_cases
import _swt_inv_cases
import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters as F
from pytorch_wavelets_amd import ops
from pytorch_wavelets_amd.dwt import lowlevel as dwl
from pytorch_wavelets_amd.dwt.transform2d import SWTForward, SWTInverse

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
TOL = {F32: 1e-5, F16: 4e-3, F64: 1e-12}
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def bound_of(dtype, one_level):
    if dtype == BF16:
        return _bf16_cases.ONE if one_level else _bf16_cases.MULTI
    return TOL[dtype]


# ---- view makers: maker(t, dev) -> (view holding t's values, the NaN-filled parent it lies in) ---------------------------
def _parent(numel, dtype, dev):
    """`numel` NaNs, the first of them on a 256-byte boundary."""
    es = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((numel + 256 // es,), float('nan'), dtype=dtype, device=dev)
    skip = (-buf.data_ptr()) % 256 // es
    p = buf[skip:skip + numel]
    assert p.data_ptr() % 256 == 0 and p.numel() == numel
    return p


class Maker(object):
    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __call__(self, t, dev):
        v, p = self.fn(t, dev)
        assert v.shape == t.shape and v.dtype == t.dtype
        v.copy_(t)
        return v, p

    def __repr__(self):
        return self.name


def offset(k):
    """contiguous, the base k elements past the boundary (k = 0: the dense aligned tensor)"""
    def fn(t, dev):
        p = _parent(k + t.numel() + 8, t.dtype, dev)
        return p[k:k + t.numel()].view(t.shape), p
    return Maker('offset(%d)' % k, fn)


def crop(top, left, right, bottom=1, pitch16=False):
    """parent[..., top:top+H, left:left+W]: pitch W+left+right (`pitch16`: `right` grows until the pitch is a whole number
    of 16-byte pieces), base offset top*pitch+left"""
    def fn(t, dev):
        H, W = t.shape[-2:]
        r = right
        if pitch16:
            q = 16 // t.element_size()
            r += (-(W + left + r)) % q
        shape = tuple(t.shape[:-2]) + (top + H + bottom, W + left + r)
        p = _parent(int(np.prod(shape)), t.dtype, dev)
        return p.view(shape)[..., top:top + H, left:left + W], p
    return Maker('crop(%d,%d,%d,%d%s)' % (top, left, right, bottom, ',pitch16' if pitch16 else ''), fn)


def padded16():
    """a crop with left = 0 whose pitch is the next whole number of 16-byte pieces above W: the fused analysis accepts it"""
    def fn(t, dev):
        q = 16 // t.element_size()
        return crop(0, 0, (t.shape[-1] // q + 1) * q - t.shape[-1], 0).fn(t, dev)
    return Maker('padded16()', fn)


def last_slice(left, right):
    """parent[..., left:left+n] of a longer last axis (any rank)"""
    def fn(t, dev):
        shape = tuple(t.shape[:-1]) + (left + t.shape[-1] + right,)
        p = _parent(int(np.prod(shape)), t.dtype, dev)
        return p.view(shape)[..., left:left + t.shape[-1]], p
    return Maker('last_slice(%d,%d)' % (left, right), fn)


def channel_slice():
    """parent[:, 1:1+C] of C+2 channels: uniform plane stride, batch stride != C * plane stride - copied"""
    def fn(t, dev):
        shape = (t.shape[0], t.shape[1] + 2) + tuple(t.shape[2:])
        p = _parent(int(np.prod(shape)), t.dtype, dev)
        return p.view(shape)[:, 1:1 + t.shape[1]], p
    return Maker('channel_slice()', fn)


def batch_step():
    """parent[::2] of single-channel images: plane stride 2 H W, read in place"""
    def fn(t, dev):
        assert t.shape[1] == 1
        shape = (2 * t.shape[0],) + tuple(t.shape[1:])
        p = _parent(int(np.prod(shape)), t.dtype, dev)
        return p.view(shape)[::2], p
    return Maker('batch_step()', fn)


def transposed():
    """column stride != 1 - copied (no padding: the parent is the transposed storage itself)"""
    def fn(t, dev):
        p = torch.empty(tuple(t.shape[:-2]) + (t.shape[-1], t.shape[-2]), dtype=t.dtype, device=dev)
        return p.transpose(-1, -2), p.view(-1)
    return Maker('transposed()', fn)


def band_slice():
    """highpass tensors (N,C,3,Kh,Kw): y5[:, :, 1:] of an (N,C,4,Kh,Kw) buffer, the base Kh*Kw elements into it"""
    def fn(t, dev):
        assert t.dim() == 5 and t.shape[2] == 3
        shape = tuple(t.shape[:2]) + (4,) + tuple(t.shape[3:])
        p = _parent(int(np.prod(shape)), t.dtype, dev)
        return p.view(shape)[:, :, 1:], p
    return Maker('band_slice()', fn)


DENSE = offset(0)


# ---- transforms: shapes(input shape) -> the shapes of all inputs; build(dev, dtype) -> (run, oracle) ----------------------
class Tf(object):
    def __init__(self, name, shapes, build, one_level=False):
        self.name, self.shapes, self.build, self.one_level = name, shapes, build, one_level


def _mod(m, dev, dtype):
    m = m.to(dev)
    return m.double() if dtype == F64 else m


def _bufs(m, names):
    return [getattr(m, n).detach().double().cpu().numpy().ravel() for n in names]


def _klen(n, L, mode):
    return (n + 1) // 2 if mode == 'periodization' else (n + L - 1) // 2


def _some(vs):
    return [v for v in vs if v is not None and v.ndim > 1]      # (a skipped level: None, or a 0-dim placeholder)


def dwt_fwd(J, wave, mode):
    def build(dev, dtype):
        m = _mod(pw.DWTForward(J=J, wave=wave, mode=mode), dev, dtype)
        f = _bufs(m, ('h0_col', 'h1_col', 'h0_row', 'h1_row'))

        def run(x):
            yl, yh = m(x)
            return [yl] + list(yh)

        def oracle(x):
            yl, yh = wo.dwt_forward(x, J, f[0], f[1], f[2], f[3], mode)
            return [yl] + list(yh)
        return run, oracle
    return Tf('DWTForward(J=%d, %s, %s)' % (J, wave, mode), lambda s: [s], build, J == 1)


def dwt_inv(J, wave, mode, yl_plus=0):
    """inputs: yl, yh[0] (finest) .. yh[J-1]; `yl_plus`: the lowpass one row and column larger than the coarsest level"""
    L = len(F.dwt_analysis_taps(wave)[0])

    def shapes(s):
        N, C, H, W = s
        out = []
        for _ in range(J):
            H, W = _klen(H, L, mode), _klen(W, L, mode)
            out.append((N, C, 3, H, W))
        return [(N, C, H + yl_plus, W + yl_plus)] + out

    def build(dev, dtype):
        m = _mod(pw.DWTInverse(wave=wave, mode=mode), dev, dtype)
        g = _bufs(m, ('g0_col', 'g1_col', 'g0_row', 'g1_row'))

        def run(yl, *yh):
            return [m((yl, list(yh)))]

        def oracle(yl, *yh):
            return [wo.dwt_inverse(yl, list(yh), g[0], g[1], g[2], g[3], mode)]
        return run, oracle
    return Tf('DWTInverse(J=%d, %s, %s%s)' % (J, wave, mode, ', yl+1' if yl_plus else ''), shapes, build)


def dt_fwd(J, biort='near_sym_a', qshift='qshift_a', skip_hps=False):
    def build(dev, dtype):
        m = _mod(pw.DTCWTForward(J=J, biort=biort, qshift=qshift, skip_hps=skip_hps), dev, dtype)
        taps = F.dtcwt_forward_taps(biort, qshift)

        def run(x):
            yl, yh = m(x)
            return [yl] + _some(yh)

        def oracle(x):
            yl, yh = wo.dtcwt_forward(x, J, *taps, skip_hps=skip_hps)
            return [yl] + _some(yh)
        return run, oracle
    return Tf('DTCWTForward(J=%d, %s, %s%s)' % (J, biort, qshift, ', skip_hps' if skip_hps else ''), lambda s: [s], build)


def dt_inv(J, biort='near_sym_a', qshift='qshift_a'):
    """inputs: yl, yh[0] (finest) .. yh[J-1] of an (N,C,H,W) image, H and W multiples of 2**J"""
    def shapes(s):
        N, C, H, W = s
        return [(N, C, H >> (J - 1), W >> (J - 1))] + [(N, C, 6, H >> (j + 1), W >> (j + 1), 2) for j in range(J)]

    def build(dev, dtype):
        m = _mod(pw.DTCWTInverse(biort=biort, qshift=qshift), dev, dtype)
        taps = F.dtcwt_inverse_taps(biort, qshift)

        def run(yl, *yh):
            return [m((yl, list(yh)))]

        def oracle(yl, *yh):
            return [wo.dtcwt_inverse(yl, list(yh), *taps)]
        return run, oracle
    return Tf('DTCWTInverse(J=%d, %s, %s)' % (J, biort, qshift), shapes, build)


def scat(biort='near_sym_a', magbias=1e-2):
    def build(dev, dtype):
        m = _mod(pw.ScatLayer(biort=biort, magbias=magbias), dev, dtype)
        h0o, h1o = F.dtcwt_forward_taps(biort, 'qshift_a')[:2]
        return (lambda x: [m(x)]), (lambda x: [wo.scat_layer_forward(x, h0o, h1o, magbias=magbias)])
    return Tf('ScatLayer(%s, magbias=%g)' % (biort, magbias), lambda s: [s], build)


def scatj2():
    def build(dev, dtype):
        m = _mod(pw.ScatLayerj2(), dev, dtype)
        taps = F.dtcwt_forward_taps('near_sym_a', 'qshift_a')
        return (lambda x: [m(x)]), (lambda x: [wo.scat_layer_j2_forward(x, *taps)])
    return Tf('ScatLayerj2()', lambda s: [s], build)


def dwt1d_fwd(J, wave, mode):
    def build(dev, dtype):
        m = _mod(pw.DWT1DForward(J=J, wave=wave, mode=mode), dev, dtype)
        h0, h1 = F.dwt_analysis_taps(wave)

        def run(x):
            yl, yh = m(x)
            return [yl] + list(yh)

        def oracle(x):
            yl, yh = wo.dwt1d_forward(x, J, h0, h1, mode)
            return [yl] + list(yh)
        return run, oracle
    return Tf('DWT1DForward(J=%d, %s, %s)' % (J, wave, mode), lambda s: [s], build, J == 1)


def dwt1d_inv(J, wave, mode):
    L = len(F.dwt_analysis_taps(wave)[0])

    def shapes(s):
        n, out = s[-1], []
        for _ in range(J):
            n = _klen(n, L, mode)
            out.append(tuple(s[:-1]) + (n,))
        return [out[-1]] + out

    def build(dev, dtype):
        m = _mod(pw.DWT1DInverse(wave=wave, mode=mode), dev, dtype)
        g0, g1 = F.dwt_synthesis_taps(wave)
        return (lambda yl, *yh: [m((yl, list(yh)))]), (lambda yl, *yh: [wo.dwt1d_inverse(yl, list(yh), g0, g1, mode)])
    return Tf('DWT1DInverse(J=%d, %s, %s)' % (J, wave, mode), shapes, build)


def swt_fwd(J, wave, mode='periodic'):
    def build(dev, dtype):
        m = _mod(SWTForward(J=J, wave=wave, mode=mode), dev, dtype)
        h0, h1 = F.dwt_analysis_taps(wave)

        def oracle(x):
            out, ll = [], x
            for j in range(J):
                out.append(wo.afb2d_atrous(ll, h0, h1, h0, h1, mode, 2 ** j))
                ll = out[-1][:, 0::4]
            return out
        return (lambda x: list(m(x))), oracle
    return Tf('SWTForward(J=%d, %s, %s)' % (J, wave, mode), lambda s: [s], build, J == 1)


def swt_inv(J, wave):
    """inputs: the J tensors (N,4C,H,W) SWTForward returns, finest first"""
    def build(dev, dtype):
        m = _mod(SWTInverse(wave=wave, mode='periodic'), dev, dtype)
        g = F.dwt_synthesis_taps(wave)
        return (lambda *cs: [m(list(cs))]), (lambda *cs: [_swt_inv_cases.inv_ref(list(cs), g, g)])
    return Tf('SWTInverse(J=%d, %s)' % (J, wave), lambda s: [(s[0], 4 * s[1], s[2], s[3])] * J, build)


def _nonsep_filts(wave, dev, dtype):
    w = F.Wavelet(wave)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        fa, fs = dwl.prep_filt_afb2d_nonsep(w.dec_lo, w.dec_hi), dwl.prep_filt_sfb2d_nonsep(w.rec_lo, w.rec_hi)
    finally:
        torch.set_default_dtype(prev)
    acc = F64 if dtype == F64 else F32
    return fa.to(acc).to(dev), fs.to(acc).to(dev), fa.to(acc).double().numpy(), fs.to(acc).double().numpy()


def nonsep_afb(wave, mode):
    def build(dev, dtype):
        fa, _, fan, _ = _nonsep_filts(wave, dev, dtype)
        return (lambda x: [dwl.afb2d_nonsep(x, fa, mode)]), (lambda x: [wo.afb2d_nonsep(x, fan, mode)])
    return Tf('afb2d_nonsep(%s, %s)' % (wave, mode), lambda s: [s], build, True)


def nonsep_sfb(wave, mode):
    """input: coefficients (N,C,4,Kh,Kw) of an (N,C,H,W) image"""
    L = len(F.dwt_analysis_taps(wave)[0])

    def build(dev, dtype):
        _, fs, _, fsn = _nonsep_filts(wave, dev, dtype)
        return (lambda c: [dwl.sfb2d_nonsep(c, fs, mode)]), (lambda c: [wo.sfb2d_nonsep(c, fsn, mode)])
    return Tf('sfb2d_nonsep(%s, %s)' % (wave, mode), lambda s: [(s[0], s[1], 4, _klen(s[2], L, mode), _klen(s[3], L, mode))], build)


# ---- route pins ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def pinned(pin):
    """`pin`: module flags of ops (FUSED_STRIPS=1, STREAM_FORCE=True) or dwt/lowlevel.py (FUSED_LEVELS=False) and / or engine
    options ('generic_only', 'no_stream', 'scat_stream'), restored afterwards."""
    pin = dict(pin or {})
    opts = [k for k in pin if k in ('generic_only', 'no_stream', 'scat_stream')]
    flags = {k: ops if hasattr(ops, k) else dwl for k in pin if k not in opts}
    prev = {k: getattr(m, k) for k, m in flags.items()}
    try:
        for k, m in flags.items():
            setattr(m, k, pin[k])
        for k in opts:
            ops.set_option(k, pin[k])
        yield
    finally:
        for k, m in flags.items():
            setattr(m, k, prev[k])
        for k in opts:
            ops.set_option(k, 0)


STRIPS, STREAM = {'FUSED_STRIPS': 1}, {'STREAM_FORCE': True}
PER_LEVEL = {'FUSED_LEVELS': False}          # one launch per level: neither the small-plane nor the multi-level kernels
GENERIC = {'generic_only': 1, 'FUSED_LEVELS': False}


class Case(object):
    """One row of the table.  `makers`: one maker for every input, or a list (one per input; a short list repeats its last
    entry).  `expect_emu` / `expect_gpu`: for the first launches of the view call, the allowed name prefixes of each (a string
    or a tuple of strings per launch).  `gpu_planes`: N on the real chip where the launcher's policy asks for more planes
    than the 2-CU emulator.  `only`: 'emu' for float64 rows."""

    def __init__(self, name, tf, shape, dtype, makers, expect_emu, expect_gpu=None, pin=None, gpu_planes=None, only=None, cus=2):
        self.name, self.tf, self.shape, self.dtype, self.pin, self.only, self.cus = name, tf, tuple(shape), dtype, pin, only, cus
        self.makers = list(makers) if isinstance(makers, (list, tuple)) else [makers]
        self.expect = {'emu': expect_emu, 'gpu': expect_gpu if expect_gpu is not None else expect_emu}
        self.gpu_planes = gpu_planes

    def __repr__(self):
        return self.name

    def shape_on(self, backend):
        if backend == 'gpu' and self.gpu_planes:
            return (self.gpu_planes,) + self.shape[1:]
        return self.shape

    def maker(self, i):
        return self.makers[min(i, len(self.makers) - 1)]


def _backend_of(dev):
    return 'emu' if str(dev) == 'cpu' else 'gpu'


def _sync(dev):
    if str(dev) != 'cpu':
        torch.cuda.synchronize()


def _inputs(case, dev, seed):
    """the dense values of every input, in the case's dtype (for 16-bit data: rounded), on the host"""
    rng = np.random.RandomState(seed)
    return [torch.tensor(rng.randn(*s)).to(case.dtype) for s in case.tf.shapes(case.shape_on(_backend_of(dev)))]


def _launches(c0):
    return _mutation_cases.primary(pw.kernels_since(c0))


def _expect(ks, expect, what):
    expect = [expect] if isinstance(expect, str) else list(expect)
    expect = [(e,) if isinstance(e, str) else tuple(e) for e in expect]
    assert len(ks) >= len(expect) and all(k.startswith(e) for k, e in zip(ks, expect)), (what, ks, expect)


def _bits(p):
    return p.view(_INT[p.element_size()]).clone()


def _npy(t):
    return t.detach().cpu().double().numpy()


def check(case, dev, seed=11, outs_to=None):
    """Checks (a) - (e) of the module docstring; returns [(output index, max error, bound)].  `outs_to`: a list that receives
    the output tensors of the view call (tests/_guard_cases.py looks at where they lie)."""
    backend = _backend_of(dev)
    host = _inputs(case, dev, seed)
    ops._FUSED_DECLINED.clear()
    with pinned(case.pin):
        run, oracle = case.tf.build(dev, case.dtype)
        dense = [DENSE(t, dev)[0] for t in host]
        assert all(d.data_ptr() % 256 == 0 and d.is_contiguous() for d in dense)
        c0 = pw.launch_count()
        run(*dense)
        k_dense = _launches(c0)
        views, parents = zip(*[case.maker(i)(t, dev) for i, t in enumerate(host)])
        before = [_bits(p) for p in parents]
        c0 = pw.launch_count()
        outs = run(*views)
        k_view = _launches(c0)
        c0 = pw.launch_count()
        run(*dense)
        k_again = _launches(c0)
        _sync(dev)
    print('%s %s %s %s: view %s, dense %s' % (case.name, case.tf.name, case.shape_on(backend), [case.maker(i) for i in range(len(host))],
                                             k_view, k_dense))
    # (c) the inputs, padding included
    assert all(torch.equal(_bits(p), b) for p, b in zip(parents, before)), 'an input or its padding was written'
    # (a), (b)
    refs = oracle(*[_npy(t) for t in host])
    assert len(refs) == len(outs), (len(refs), len(outs))
    if outs_to is not None:
        outs_to.extend(outs)
    errs = []
    for i, (o, ref) in enumerate(zip(outs, refs)):
        assert o.dtype == case.dtype and tuple(o.shape) == ref.shape, (i, o.dtype, tuple(o.shape), ref.shape)
        a = _npy(o)
        assert not np.isnan(a).any(), 'NaN in output %d' % i
        err, bound = float(np.abs(a - ref).max()), bound_of(case.dtype, case.tf.one_level) * float(np.abs(ref).max())
        print('    out %d: max err %.3e, bound %.3e' % (i, err, bound))
        errs.append((i, err, bound))
    assert all(e <= b for _, e, b in errs), errs
    # (d) the kernel the row is about
    _expect(k_view, case.expect[backend], case.name)
    # (e) what the view call left behind does not reroute the dense call
    assert k_again == k_dense, ('the dense route changed after the view call', k_dense, k_again)
    return errs


def check_grad(case, dev, seed=12, outs_to=None):
    """torch.autograd.grad through the case's transform: every input a crop view (the case's own makers where it has several
    inputs), every gradient output an offset(1) view; against the gradients of dense aligned clones on the per-level tile
    path, which must be full tensors without NaN.  `outs_to`: a list that receives the gradients of the view call."""
    host = _inputs(case, dev, seed)
    rng = np.random.RandomState(seed + 1)
    ops._FUSED_DECLINED.clear()
    with pinned(case.pin):
        run, _ = case.tf.build(dev, case.dtype)
        mk = [crop(1, 1, 2) if len(host) == 1 and host[0].dim() == 4 else case.maker(i) for i in range(len(host))]
        xs = [m(t, dev)[0].requires_grad_(True) for m, t in zip(mk, host)]
        outs = run(*xs)
        cots = [torch.tensor(rng.randn(*o.shape)).to(case.dtype) for o in outs]
        c0 = pw.launch_count()
        grads = torch.autograd.grad(outs, xs, grad_outputs=[offset(1)(c, dev)[0] for c in cots])
        k_view = _launches(c0)
    prev = dwl.FUSED_LEVELS
    dwl.FUSED_LEVELS = False
    ops.set_option('no_stream', 1)
    try:
        run, _ = case.tf.build(dev, case.dtype)
        xd = [DENSE(t, dev)[0].requires_grad_(True) for t in host]
        c0 = pw.launch_count()
        ref = torch.autograd.grad(run(*xd), xd, grad_outputs=[DENSE(c, dev)[0] for c in cots])
        k_ref = _launches(c0)
    finally:
        ops.set_option('no_stream', 0)
        dwl.FUSED_LEVELS = prev
    _sync(dev)
    print('%s %s backward: view %s, reference %s' % (case.name, case.tf.name, k_view, k_ref))
    assert not any('Strip' in k or 'Rows' in k for k in k_ref), k_ref
    if outs_to is not None:
        outs_to.extend(grads)
    errs = []
    for i, (g, r, x) in enumerate(zip(grads, ref, xs)):
        assert g.shape == x.shape and g.dtype == case.dtype
        a, b = _npy(g), _npy(r)
        assert not np.isnan(a).any(), 'NaN in gradient %d' % i
        err, bound = float(np.abs(a - b).max()), bound_of(case.dtype, case.tf.one_level) * float(np.abs(b).max())
        print('    grad %d: max err %.3e, bound %.3e' % (i, err, bound))
        errs.append((i, err, bound))
    assert all(e <= b for _, e, b in errs), errs
    return errs


# ---- the table ---------------------------------------------------------------------------------------------------------
def _offs(dtype):
    return (1, 2) if dtype in (F32, F64) else (1, 2, 4)


_T = {F32: 'float', F16: '_Float16', BF16: '__bf16', F64: 'double'}


def _n(dtype):
    return {F32: 'f32', F16: 'f16', BF16: 'bf16', F64: 'f64'}[dtype]


def _table():
    T = []

    def add(name, *a, **kw):
        assert all(c.name != name for c in T), name
        T.append(Case(name, *a, **kw))

    CR = crop(1, 1, 2)
    # -- 2-D DWT, several small planes per workgroup (vec_ok of wl_api.inc: the 16-byte loads of a group of planes) --------
    for dt in (F32, F16):
        for shape, mks in (((3, 2, 35, 35), [offset(1), CR]), ((4, 1, 36, 36), [offset(k) for k in _offs(dt)])):
            for mk in mks:
                tag = '%dx%d-%s-%s' % (shape[2], shape[3], _n(dt), mk)
                add('small-fwd-' + tag, dwt_fwd(2, 'db2', 'symmetric'), shape, dt, mk, 'WlAfbSmall<')
                add('small-inv-' + tag, dwt_inv(2, 'db2', 'symmetric'), shape, dt, mk, 'WlSfbSmall<')
    # -- the tile kernels (vec_ok / q4 of wl_api.inc, the pair loads of wl_dwt_tile_syn.h), one launch per level: on the
    #    2-CU emulator two planes already fill the chip and the dense 132-column planes would take the fused kernels
    NS = PER_LEVEL
    sym, per, zero = ('db2', 'symmetric'), ('db4', 'periodization'), ('db5', 'zero')
    tile = [(F32, sym, offset(1)), (F32, sym, offset(2)), (F32, sym, CR), (F32, sym, padded16()), (F32, sym, batch_step()),
            (F32, sym, transposed()), (F16, sym, offset(1)), (F16, sym, offset(2)), (F16, sym, offset(4)), (F16, sym, CR),
            (F16, sym, batch_step()), (F32, per, CR), (F32, per, offset(2)), (F16, per, offset(1)), (F16, per, offset(4)),
            (F32, zero, offset(1)), (F32, zero, batch_step()), (F16, zero, CR), (F16, zero, offset(2)),
            # (bfloat16 takes the float16 kernels: both sides of their pair and quad predicates)
            (BF16, sym, offset(1)), (BF16, sym, offset(2)), (BF16, sym, offset(4))]
    for dt, (wave, mode), mk in tile:
        tag = '%s-%s-%s-%s' % (wave, mode[:3], _n(dt), mk)
        add('tile-fwd-' + tag, dwt_fwd(1, wave, mode), (2, 1, 70, 132), dt, mk, 'WlAfbTile<', pin=NS)
        add('tile-inv-' + tag, dwt_inv(1, wave, mode), (2, 1, 70, 132), dt, mk, 'WlSfbTile<', pin=NS)
    for dt in (F32, F16):
        # (two channels: the slice has no uniform plane stride and is copied)
        add('tile-fwd-chan-' + _n(dt), dwt_fwd(1, 'db2', 'symmetric'), (2, 2, 70, 132), dt, channel_slice(), 'WlAfbTile<', pin=NS)
        add('tile-inv-band-' + _n(dt), dwt_inv(1, 'db2', 'symmetric'), (2, 1, 70, 132), dt, [offset(1), band_slice()], 'WlSfbTile<', pin=NS)
    add('tile-inv-band-dense-yl', dwt_inv(1, 'db4', 'periodization'), (2, 1, 70, 132), F32, [DENSE, band_slice()], 'WlSfbTile<', pin=NS)
    add('tile-fwd-f64', dwt_fwd(1, 'db2', 'symmetric'), (2, 1, 70, 132), F64, CR, 'WlAfb2dTile<double>', pin=NS, only='emu')
    add('tile-inv-f64', dwt_inv(1, 'db5', 'zero'), (2, 1, 70, 132), F64, offset(1), 'WlSfb2dTile<double>', pin=NS, only='emu')
    # (the runtime-tap kernels)
    add('generic-fwd-f32', dwt_fwd(1, 'db2', 'symmetric'), (2, 1, 70, 132), F32, offset(1), 'WlAfb2dTile<float>', pin=GENERIC)
    add('generic-fwd-f16', dwt_fwd(1, 'db2', 'symmetric'), (2, 1, 70, 132), F16, offset(2), 'WlAfb2dTile<_Float16>', pin=GENERIC)
    add('generic-inv-f32', dwt_inv(1, 'db2', 'symmetric'), (2, 1, 70, 132), F32, offset(1), 'WlSfb2dTile<float>', pin=GENERIC)
    # -- the one-level strip kernels, forced (element-aligned stagers; pair_ok of wl_strip_api.inc) ------------------------
    strip = [((1, 2, 40, 259), 'db2', 'symmetric', F32, CR), ((1, 2, 40, 259), 'db2', 'symmetric', F16, CR),
             ((1, 2, 40, 259), 'db8', 'symmetric', F32, offset(1)), ((2, 1, 40, 704), 'db8', 'periodization', F32, offset(1)),
             ((2, 1, 40, 704), 'db8', 'periodization', F16, offset(1)), ((2, 1, 40, 704), 'db8', 'periodization', F16, offset(2)),
             ((2, 1, 40, 704), 'db2', 'symmetric', F32, offset(2)), ((2, 1, 40, 704), 'db2', 'symmetric', F16, CR),
             ((2, 1, 40, 704), 'db2', 'periodization', F32, crop(1, 1, 3))]
    for shape, wave, mode, dt, mk in strip:
        tag = '%d-%s-%s-%s-%s' % (shape[3], wave, mode[:3], _n(dt), mk)
        # (an emulated chip of 8 CUs: on 2 CUs two planes fill the chip and the fused kernels would be asked first)
        add('strip-fwd-' + tag, dwt_fwd(1, wave, mode), shape, dt, mk, 'WlAfbStrip<', pin=STREAM, cus=8)
        add('strip-inv-' + tag, dwt_inv(1, wave, mode), shape, dt, mk, 'WlSfbStrip<', pin=STREAM, cus=8)
    # -- the fused multi-level kernels, forced: the analysis declines every base and pitch that is no whole 16-byte piece
    #    (ops.afb2d_fused / wl_rows_api.inc); the synthesis copies planes as 16-byte pieces + a dword tail from 4-byte
    #    aligned addresses (ops.sfb2d_fused / wl_rows_api.inc)
    rows = (12, 1, 96, 80)
    fw3, iv3 = dwt_fwd(3, 'db2', 'symmetric'), dwt_inv(3, 'db2', 'symmetric')
    add('rows-fwd-f32-padded16', fw3, rows, F32, padded16(), 'WlAfbRows<float', pin=STRIPS)
    add('rows-fwd-f16-padded16', fw3, rows, F16, padded16(), 'WlAfbRows<_Float16', pin=STRIPS)
    add('rows-fwd-f32-offset1', fw3, rows, F32, offset(1), ['WlAfbTile<'] * 3, pin=STRIPS)
    add('rows-fwd-f32-pitch16-base4', fw3, rows, F32, crop(0, 1, 0, 0, pitch16=True), ['WlAfbTile<'] * 3, pin=STRIPS)
    # (4-byte aligned planes, not 16: the LDS-DMA source at its loosest alignment)
    add('rows-inv-f32-offset1', iv3, rows, F32, offset(1), 'WlSfbRows<float', pin=STRIPS)
    add('rows-inv-f32-offset2', iv3, rows, F32, offset(2), 'WlSfbRows<float', pin=STRIPS)
    # (float16: the finest level's 41-column rows are no whole dwords - it is a tile launch behind the two fused levels;
    #  a 2-byte base leaves the fused kernel altogether)
    add('rows-inv-f16-offset1', iv3, rows, F16, offset(1), ['WlSfbTile<_Float16'] * 3, pin=STRIPS)
    add('rows-inv-f16-offset2', iv3, rows, F16, offset(2), ['WlSfbRows<_Float16', 'WlSfbTile<_Float16'], pin=STRIPS)
    add('rows-inv-f32-yl-larger', dwt_inv(3, 'db2', 'symmetric', yl_plus=1), rows, F32, [DENSE, offset(1)], 'WlSfbRows<float', pin=STRIPS)
    add('rows-inv-f32-yl-crop', iv3, rows, F32, [CR, offset(1)], 'WlSfbRows<float', pin=STRIPS)
    add('rows-inv-per-f32-offset1', dwt_inv(2, 'db4', 'periodization'), (12, 1, 64, 96), F32, offset(1), 'WlSfbRows<float, 8', pin=STRIPS)
    # -- DTCWT ---------------------------------------------------------------------------------------------------------
    df2, di2 = dt_fwd(2), dt_inv(2)
    DTF, DTI = ['WlDtFwd1Tile<', 'WlDtFwd2Tile<'], ['WlDtInv2Tile<', 'WlDtInv1Tile<']
    PYR = [CR, offset(1)]          # yl a crop, every highpass tensor one element past its boundary
    add('dt-fwd-tile-f32-offset1', df2, (3, 2, 36, 44), F32, offset(1), DTF)
    add('dt-fwd-tile-f32-crop', df2, (3, 2, 36, 44), F32, CR, DTF)
    add('dt-fwd-tile-f16-offset1', df2, (3, 2, 36, 44), F16, offset(1), DTF)
    add('dt-fwd-tile-f16-offset2', df2, (3, 2, 36, 44), F16, offset(2), DTF)
    add('dt-fwd-tile-b-f32-offset1', dt_fwd(2, 'near_sym_b', 'qshift_b'), (3, 2, 36, 44), F32, offset(1), ['WlDtFwd1Tile<float, 13, 19>', 'WlDtFwd2Tile<float, 14>'])
    add('dt-fwd-tile-skip-f32-offset1', dt_fwd(2, skip_hps=(True, False)), (3, 2, 36, 44), F32, offset(1), DTF)
    for shape in ((2, 1, 64, 256), (2, 1, 40, 72)):
        for dt, k in ((F32, 1), (F16, 1), (F16, 2), (BF16, 1)):
            add('dt-fwd-strip-%d-%s-offset%d' % (shape[3], _n(dt), k), df2, shape, dt, offset(k), 'WlDtFwd12Strip<' + _T[dt] + ', 5, 7, 10>', pin=STREAM)
    add('dt-inv-tile-f32', di2, (3, 2, 36, 44), F32, PYR, DTI)
    add('dt-inv-tile-f16', di2, (3, 2, 36, 44), F16, PYR, DTI)
    add('dt-inv-tile-b-f32', dt_inv(2, 'near_sym_b', 'qshift_b'), (3, 2, 36, 44), F32, PYR, ['WlDtInv2Tile<float, 14>', 'WlDtInv1Tile<float, 19, 13>'])
    # (the engine's own policy, nothing forced: what a misaligned pyramid leaves behind must not reroute the aligned one -
    #  check (e); 256 CUs ask for 256 planes of 256 columns)
    add('dt-inv-policy-256-f32-offset1', di2, (2, 1, 64, 256), F32, offset(1), DTI, gpu_planes=256)
    add('dt-inv-policy-256-f16-offset1', di2, (2, 1, 64, 256), F16, offset(1), DTI, gpu_planes=256)
    add('dt-inv-policy-256-f32-pyr', di2, (2, 1, 64, 256), F32, PYR, DTI, gpu_planes=256)
    # (pairs of elements are loaded at once: bases on 2 * sizeof(T) stay on the streaming kernels, the others - and the
    #  crop's odd row pitch - decline to the tile kernels, whatever is forced)
    add('dt-inv-forced-256-f32-pyr', di2, (2, 1, 64, 256), F32, PYR, DTI, pin=STREAM)
    add('dt-inv-forced-256-f32-offset2', di2, (2, 1, 64, 256), F32, offset(2), 'WlDtInv21Strip<float', pin=STREAM)
    add('dt-inv-forced-256-f16-offset2', di2, (2, 1, 64, 256), F16, offset(2), 'WlDtInv21Strip<_Float16', pin=STREAM)
    add('dt-inv-forced-72-f32-pyr', di2, (2, 1, 40, 72), F32, PYR, DTI, pin=STREAM)
    add('dt-inv-forced-72-f16-offset1', di2, (2, 1, 40, 72), F16, offset(1), DTI, pin=STREAM)
    # (no launch for levels 2 + 1 of the 13 / 19-tap pair: the level >= 2 and the level-1 streaming kernels, by the engine's
    #  own policy - on the real chip they ask for a plane per CU)
    dib = dt_inv(2, 'near_sym_b', 'qshift_b')
    add('dt-inv-b-256-f32-offset2', dib, (2, 1, 64, 256), F32, offset(2), ['WlDtInv2Strip<float, 14', 'WlDtInv1Strip<float, 19, 13'], gpu_planes=256)
    add('dt-inv-b-256-f32-offset1', dib, (2, 1, 64, 256), F32, offset(1), ['WlDtInv2Tile<float, 14', 'WlDtInv1Tile<float, 19, 13'], gpu_planes=256)
    add('dt-inv1-256-f16-offset2', dt_inv(1), (2, 1, 64, 256), F16, offset(2), 'WlDtInv1Strip<_Float16, 7, 5', gpu_planes=256)
    add('dt-inv1-256-f16-offset1', dt_inv(1), (2, 1, 64, 256), F16, offset(1), 'WlDtInv1Tile<_Float16, 7, 5', gpu_planes=256)
    add('dt-fwd1-small-f32', dt_fwd(1), (6, 3, 32, 32), F32, offset(1), 'WlDtFwd1Small<float')
    add('dt-fwd1-small-f16', dt_fwd(1), (6, 3, 32, 32), F16, offset(1), 'WlDtFwd1Small<_Float16')
    LEAN = 'WlDtFwd12Strip<%s, 5, 7, 10, 1, 4, 2>'
    # -- ScatLayer -------------------------------------------------------------------------------------------------------
    add('scat-44-f32-offset1', scat(), (3, 2, 36, 44), F32, offset(1), 'WlDtFwd1Tile<float, 5, 7>')
    add('scat-44-f16-offset1', scat(), (3, 2, 36, 44), F16, offset(1), 'WlDtFwd1Tile<_Float16, 5, 7>')
    add('scat-44-b-f32-crop', scat('near_sym_b'), (3, 2, 36, 44), F32, CR, 'WlDtFwd1Tile<float, 13, 19>')
    # (the lean level-1 kernel - an instantiation of WlDtFwd12Strip - takes planes of up to 256 columns when they fill the chip)
    add('scat-256-f32-offset1', scat(), (2, 3, 64, 256), F32, offset(1), LEAN % 'float', gpu_planes=86)
    add('scat-256-f16-crop', scat(), (2, 3, 64, 256), F16, CR, LEAN % '_Float16', gpu_planes=86)
    add('scat-256-stream-f32-offset1', scat(), (2, 3, 64, 256), F32, offset(1), LEAN % 'float', pin={'scat_stream': 1}, gpu_planes=86)
    add('scat-256-magbias-f32-offset2', scat(magbias=0.1), (2, 3, 64, 256), F32, offset(2), LEAN % 'float', gpu_planes=86)
    add('scatj2-44-f32-offset1', scatj2(), (3, 2, 36, 44), F32, offset(1), ['WlDtFwd1Tile<float', 'WlDtFwd2Tile<float', 'WlDtFwd1Small<float'])
    add('scatj2-256-f16-offset1', scatj2(), (2, 3, 64, 256), F16, offset(1), ['WlDtFwd12Strip<_Float16'] * 3, gpu_planes=86)
    # -- single axis, stationary, non-separable ---------------------------------------------------------------------------
    f1, i1 = dwt1d_fwd(3, 'db4', 'symmetric'), dwt1d_inv(3, 'db4', 'symmetric')
    for dt, mk in ((F32, offset(1)), (F32, last_slice(1, 2)), (F16, offset(1))):
        add('dwt1d-fwd-%s-%s' % (_n(dt), mk), f1, (5, 3, 1001), dt, mk, 'WlDwt1dFused<' + _T[dt])
        add('dwt1d-inv-%s-%s' % (_n(dt), mk), i1, (5, 3, 1001), dt, mk, 'WlIdwt1dFused<' + _T[dt])
    add('swt-fwd-f32-crop', swt_fwd(2, 'db2'), (1, 2, 21, 35), F32, CR, ['WlSwtLevel<'] * 2)
    add('swt-fwd-f16-crop', swt_fwd(2, 'db2'), (1, 2, 21, 35), F16, CR, ['WlSwtLevel<'] * 2)
    add('swt-fwd-f32-batch-step', swt_fwd(2, 'db2'), (2, 1, 21, 35), F32, batch_step(), ['WlSwtLevel<'] * 2)
    # (batch_step() is for single-channel images: the inverse's (N, 4C, H, W) tensors have four channels at least, and the engine
    #  reads them dense - its plane-strided `ll` is its own `[:, 0::4]` slice of the coarsest tensor, whatever view that is)
    add('swt-inv-f32-crop', swt_inv(2, 'db2'), (1, 2, 21, 35), F32, CR, ['WlSwtInvLevel<'] * 2)
    add('swt-inv-f32-offset1', swt_inv(2, 'db2'), (1, 2, 21, 35), F32, offset(1), ['WlSwtInvLevel<'] * 2)
    add('nonsep-afb-f32-offset1', nonsep_afb('db2', 'symmetric'), (2, 2, 20, 24), F32, offset(1), 'WlAfbNonsep<float>')
    add('nonsep-afb-f16-offset1', nonsep_afb('db2', 'symmetric'), (2, 2, 20, 24), F16, offset(1), 'WlAfbNonsep<_Float16>')
    add('nonsep-afb-f32-chan', nonsep_afb('db2', 'symmetric'), (2, 2, 20, 24), F32, channel_slice(), 'WlAfbNonsep<float>')
    add('nonsep-sfb-f32-offset1', nonsep_sfb('db2', 'symmetric'), (2, 2, 20, 24), F32, offset(1), 'WlSfbNonsep<float>')
    add('nonsep-sfb-f32-chan', nonsep_sfb('db2', 'symmetric'), (2, 2, 20, 24), F32, channel_slice(), 'WlSfbNonsep<float>')
    return T


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
# one backward pass per family
GRAD_CASES = ['small-fwd-35x35-f32-offset(1)', 'small-inv-35x35-f32-crop(1,1,2,1)', 'tile-fwd-db2-sym-f16-offset(1)',
              'strip-fwd-704-db2-sym-f32-offset(2)', 'strip-inv-704-db8-per-f32-offset(1)', 'rows-fwd-f32-padded16',
              'rows-inv-f32-yl-crop', 'dt-fwd-strip-256-f32-offset1', 'dt-inv-forced-256-f32-pyr', 'dt-inv-tile-f32',
              'scat-44-f32-offset1', 'scat-256-f32-offset1', 'dwt1d-fwd-f32-last_slice(1,2)', 'dwt1d-inv-f32-offset(1)',
              'swt-fwd-f32-crop', 'swt-inv-f32-crop', 'nonsep-afb-f32-offset1', 'nonsep-sfb-f32-chan']
