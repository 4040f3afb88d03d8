"""Shared bfloat16 checks, run by the emulator (CPU) and the GPU test modules.

bfloat16 data takes exactly the kernels float16 data takes (fp32 taps, fp32 accumulation, one round-to-nearest-even per
store).  Every case runs twice - float16 and bfloat16 data - and checks
  * the kernels: the bfloat16 launches are the float16 ones with `_Float16` replaced by `__bf16`, forward and backward;
  * the outputs against the float64 oracle (oracle/wavelet_oracle.py) on the bfloat16-rounded input and on the taps the
    module actually holds (rounded to bfloat16 for a `.to(torch.bfloat16)` module, float32 otherwise), batch item 0;
  * the gradients against the engine's float64 path (pinned to the reference's goldens by the float64 suite) on the same
    rounded input, taps and cotangents;
  * output and gradient dtypes.
rel = max|a - ref| / max|ref|: 4e-3 for one-level forwards (2^-8, a single rounding to bfloat16), 3e-2 for everything else."""
import contextlib

import numpy as np
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters as F
from pytorch_wavelets_amd import ops
from pytorch_wavelets_amd.dtcwt import lowlevel as dtl
from pytorch_wavelets_amd.dwt import lowlevel as dwl
from pytorch_wavelets_amd.dwt.transform2d import SWTForward

BF, HF = torch.bfloat16, torch.float16
ONE, MULTI = 4e-3, 3e-2


def rnd(a, dt=BF):
    """a (array-like) rounded to dt, as float64 numpy (numpy has no bfloat16: the rounding goes through torch)."""
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dt).double().numpy()


def npy(t):
    return t.detach().cpu().double().numpy()


def rel(a, ref):
    a = npy(a) if torch.is_tensor(a) else a
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def flat(v):
    if v is None:
        return []
    if torch.is_tensor(v):
        return [] if v.dim() == 0 else [v]
    return [t for u in v for t in flat(u)]


class Taps(object):
    """How a run holds its filters: `dt` the data dtype under test, `rounded` whether the module / taps were converted to it
    (case (a)) or stay float32 (case (b), the autocast case); `f64` for the float64 reference run on the same taps."""

    def __init__(self, dev, dt, rounded, f64=False):
        self.dev, self.dt, self.rounded, self.f64 = dev, dt, rounded, f64

    def mod(self, m):
        m = m.to(self.dev)
        if self.rounded:
            m = m.to(self.dt)
        return m.double() if self.f64 else m

    def tap(self, h):
        t = torch.tensor(np.ascontiguousarray(np.asarray(h, dtype=np.float64)))
        if self.rounded:
            t = t.to(self.dt)
        return (t.double() if self.f64 else t.float()).to(self.dev)

    def np(self, h):
        """the oracle's copy of taps h: rounded like the module's"""
        return rnd(h, self.dt) if self.rounded else np.asarray(h, dtype=np.float32).astype(np.float64)


@contextlib.contextmanager
def _setattrs(obj, **kv):
    prev = {k: getattr(obj, k) for k in kv}
    for k, v in kv.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in prev.items():
            setattr(obj, k, v)


def stream_force():
    return _setattrs(ops, STREAM_FORCE=True)


def strips_force():
    return _setattrs(ops, STREAM_FORCE=True, FUSED_STRIPS=1)


def lattice_force():
    # (tests/_lattice_cases.py: one level of db8 periodization on the strip kernels, the lattice variant with its armed fallback)
    @contextlib.contextmanager
    def ctx():
        with _setattrs(ops, STREAM_FORCE=True), _setattrs(dwl, FUSED_LEVELS=False):
            yield
    return ctx()


def no_small():
    return _setattrs(ops, SMALL_PLANES=False)


@contextlib.contextmanager
def option(name, value=1):
    """wl_set_option on whichever backend ops calls (the emulator in the CPU tests), restored to 0 afterwards."""
    be = ops._backend()
    be.wl_set_option(name, value)
    try:
        yield
    finally:
        be.wl_set_option(name, 0)


class Case(object):
    """`make(taps)` -> callable on the inputs; `oracle(xs, taps)` -> [(array, tol)] for the flattened outputs of batch item 0
    (xs: the bfloat16-rounded inputs of that item as float64); `family`: a substring some launch of the bfloat16 forward must
    carry; `ctx`: forcing options around every run."""

    def __init__(self, name, shapes, make, oracle, family, ctx=None, grad=True):
        self.name, self.shapes, self.make, self.oracle, self.family = name, shapes, make, oracle, family
        self.ctx, self.grad = ctx or contextlib.nullcontext, grad

    def __repr__(self):
        return self.name


def _inputs(case, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in case.shapes]


def _run(case, dev, dt, rounded, seed, f64=False):
    taps = Taps(dev, dt, rounded, f64)
    xs = [x.to(dt) for x in _inputs(case, seed)]
    xs = [(x.double() if f64 else x).to(dev).requires_grad_(case.grad) for x in xs]
    fn = case.make(taps)
    with case.ctx():
        c0 = pw.launch_count()
        outs = flat(fn(*xs))
        kf = pw.kernels_since(c0)
        grads, kb = None, None
        if case.grad:
            g = torch.Generator().manual_seed(seed + 1)
            cots = [torch.randn(o.shape, generator=g).to(dt) for o in outs]    # representable in dt: the same for every run
            cots = [(c.double() if f64 else c).to(dev) for c in cots]
            c0 = pw.launch_count()
            grads = torch.autograd.grad(sum((o * c).float().sum() for o, c in zip(outs, cots)), xs)
            kb = pw.kernels_since(c0)
    if dev != 'cpu':
        torch.cuda.synchronize()
    return xs, outs, grads, kf, kb


def check(case, dev, rounded=True, seed=0):
    """The float16 and the bfloat16 run of `case` (module / taps in the data dtype when `rounded`, float32 otherwise)."""
    _, o16, _, kf16, kb16 = _run(case, dev, HF, rounded, seed)
    xs, outs, grads, kf, kb = _run(case, dev, BF, rounded, seed)
    # the same kernels as float16
    assert kf == [k.replace('_Float16', '__bf16') for k in kf16], (kf, kf16)
    assert any(case.family in k for k in kf), (case.family, kf)
    assert any('__bf16' in k for k in kf), kf
    assert kb == (None if kb16 is None else [k.replace('_Float16', '__bf16') for k in kb16]), (kb, kb16)
    # dtypes
    assert len(outs) == len(o16) and all(o.dtype == BF for o in outs), [o.dtype for o in outs]
    # outputs against the oracle (batch item 0)
    want = case.oracle([npy(x[:1]) for x in xs], Taps(dev, BF, rounded))
    assert len(want) == len(outs)
    errs = [(rel(o[:1], w), t) for o, (w, t) in zip(outs, want)]
    assert all(e <= t for e, t in errs), errs
    if not case.grad:
        return errs
    assert all(g.dtype == BF for g in grads)
    _, _, g64, _, _ = _run(case, dev, BF, rounded, seed, f64=True)
    gerrs = [rel(a, npy(b)) for a, b in zip(grads, g64)]
    assert all(e <= MULTI for e in gerrs), gerrs
    return errs, gerrs


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _dwt_rt(J, wave, mode):
    def make(tp):
        xfm = tp.mod(pw.DWTForward(J=J, wave=wave, mode=mode))
        ifm = tp.mod(pw.DWTInverse(wave=wave, mode=mode))

        def run(x):
            yl, yh = xfm(x)
            return [yl] + list(yh) + [ifm((yl, yh))]
        return run

    def oracle(xs, tp):
        h0, h1 = (tp.np(h) for h in F.dwt_analysis_taps(wave))
        g0, g1 = (tp.np(g) for g in F.dwt_synthesis_taps(wave))
        yl, yh = wo.dwt_forward(xs[0], J, h0, h1, h0, h1, mode)
        rec = wo.dwt_inverse(yl, yh, g0, g1, g0, g1, mode)
        t = ONE if J == 1 else MULTI
        return [(yl, t)] + [(h, t) for h in yh] + [(rec, MULTI)]
    return make, oracle


def dwt(name, shape, J, wave, mode, family, ctx=None):
    make, oracle = _dwt_rt(J, wave, mode)
    return Case(name, [shape], make, oracle, family, ctx)


def dwt1d(name, shape, J, wave, mode, family):
    def make(tp):
        xfm = tp.mod(pw.DWT1DForward(J=J, wave=wave, mode=mode))
        ifm = tp.mod(pw.DWT1DInverse(wave=wave, mode=mode))

        def run(x):
            yl, yh = xfm(x)
            return [yl] + list(yh) + [ifm((yl, yh))]
        return run

    def oracle(xs, tp):
        h0, h1 = (tp.np(h) for h in F.dwt_analysis_taps(wave))
        g0, g1 = (tp.np(g) for g in F.dwt_synthesis_taps(wave))
        yl, yh = wo.dwt1d_forward(xs[0], J, h0, h1, mode)
        return [(yl, MULTI)] + [(h, MULTI) for h in yh] + [(wo.dwt1d_inverse(yl, yh, g0, g1, mode), MULTI)]
    return Case(name, [shape], make, oracle, family)


def swt(name, shape, J, wave, mode, family):
    def make(tp):
        return tp.mod(SWTForward(J=J, wave=wave, mode=mode))

    def oracle(xs, tp):
        h0, h1 = (tp.np(h) for h in F.dwt_analysis_taps(wave))
        out, ll = [], xs[0]
        for j in range(J):
            y = wo.afb2d_atrous(ll, h0, h1, h0, h1, mode, 2 ** j)
            out.append((y, ONE if j == 0 else MULTI))
            ll = y[:, 0::4]
        return out
    return Case(name, [shape], make, oracle, family, grad=False)   # (SWTForward has no autograd Function)


def nonsep(name, shape, wave, mode, family):
    def make(tp):
        w = F.Wavelet(wave)
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            fa = dwl.prep_filt_afb2d_nonsep(w.dec_lo, w.dec_hi)
            fs = dwl.prep_filt_sfb2d_nonsep(w.rec_lo, w.rec_hi)
        finally:
            torch.set_default_dtype(prev)
        fa, fs = tp.tap(fa.numpy()), tp.tap(fs.numpy())

        def run(x):
            y = dwl.afb2d_nonsep(x, fa, mode)
            return [y, dwl.sfb2d_nonsep(y.reshape(y.shape[0], -1, 4, y.shape[-2], y.shape[-1]), fs, mode)]
        return run

    def oracle(xs, tp):
        w = F.Wavelet(wave)
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            fa = tp.np(dwl.prep_filt_afb2d_nonsep(w.dec_lo, w.dec_hi).numpy())
            fs = tp.np(dwl.prep_filt_sfb2d_nonsep(w.rec_lo, w.rec_hi).numpy())
        finally:
            torch.set_default_dtype(prev)
        y = wo.afb2d_nonsep(xs[0], fa, mode)
        return [(y, ONE), (wo.sfb2d_nonsep(y.reshape(y.shape[0], -1, 4, y.shape[-2], y.shape[-1]), fs, mode), MULTI)]
    return Case(name, [shape], make, oracle, family)


def dtcwt(name, shape, J, biort, qshift, family, ctx=None):
    def make(tp):
        xfm = tp.mod(pw.DTCWTForward(J=J, biort=biort, qshift=qshift))
        ifm = tp.mod(pw.DTCWTInverse(biort=biort, qshift=qshift))

        def run(x):
            yl, yh = xfm(x)
            return [yl] + list(yh) + [ifm((yl, yh))]
        return run

    def oracle(xs, tp):
        fw = [tp.np(h) for h in F.dtcwt_forward_taps(biort, qshift)]
        iv = [tp.np(h) for h in F.dtcwt_inverse_taps(biort, qshift)]
        yl, yh = wo.dtcwt_forward(xs[0], J, *fw)
        return [(yl, MULTI)] + [(h, MULTI) for h in yh] + [(wo.dtcwt_inverse(yl, yh, *iv), MULTI)]
    return Case(name, [shape], make, oracle, family, ctx)


def scat(name, shape, biort, family, grad=True, ctx=None):
    def make(tp):
        return tp.mod(pw.ScatLayer(biort=biort))

    def oracle(xs, tp):
        if biort.endswith('_bp'):
            # the band-pass layer: its own float64 path (the suite pins it to the reference's goldens ext_rot_*)
            m = Taps(tp.dev, BF, tp.rounded, f64=True).mod(pw.ScatLayer(biort=biort))
            with torch.no_grad():
                return [(npy(m(torch.tensor(xs[0], device=tp.dev))), MULTI)]
        h0o, h1o = (tp.np(h) for h in F.dtcwt_forward_taps(biort, 'qshift_a')[:2])
        return [(wo.scat_layer_forward(xs[0], h0o, h1o), MULTI)]
    return Case(name, [shape], make, oracle, family, ctx, grad=grad)


def scatj2(name, shape, family):
    def make(tp):
        return tp.mod(pw.ScatLayerj2())

    def oracle(xs, tp):
        return [(wo.scat_layer_j2_forward(xs[0], *[tp.np(h) for h in F.dtcwt_forward_taps('near_sym_a', 'qshift_a')]), MULTI)]
    return Case(name, [shape], make, oracle, family)


def primitives(name, shape, family):
    """The function-level primitives of dwt/lowlevel.py and dtcwt/lowlevel.py, chained on one input."""
    h0, h1 = F.dwt_analysis_taps('db3')
    g0, g1 = F.dwt_synthesis_taps('db3')
    h0o, h1o, h0a, h0b, h1a, h1b = F.dtcwt_forward_taps('near_sym_a', 'qshift_a')

    def make(tp):
        t = [tp.tap(v) for v in (h0, h1, g0, g1, h0o, h1o, h0a, h0b)]

        def run(x):
            lohi = dwl.afb1d(x, t[0], t[1], 'symmetric', 3)
            n, c2 = lohi.shape[:2]
            lo, hi = lohi[:, 0::2], lohi[:, 1::2]
            rec = dwl.sfb1d(lo, hi, t[2], t[3], 'symmetric', 3)
            cf, rf = dtl.colfilter(x, t[4]), dtl.rowfilter(x, t[5])
            cd, rd = dtl.coldfilt(x, t[6], t[7]), dtl.rowdfilt(x, t[6], t[7], highpass=True)
            ci, ri = dtl.colifilt(x, t[6], t[7]), dtl.rowifilt(x, t[6], t[7], highpass=True)
            (z1r, z1i), (z2r, z2i) = dtl.q2c(x)
            return [lo, hi, rec, cf, rf, cd, rd, ci, ri, z1r, z1i, z2r, z2i, dtl.c2q((z1r, z1i), (z2r, z2i))]
        return run

    def oracle(xs, tp):
        x = xs[0]
        a, b, c, d, e, f, ga, gb = (tp.np(v) for v in (h0, h1, g0, g1, h0o, h1o, h0a, h0b))
        lo, hi = wo.afb1d(x, a, b, 'symmetric', axis=-1)
        (z1r, z1i), (z2r, z2i) = wo.q2c(x)
        outs = [lo, hi, wo.sfb1d(lo, hi, c, d, 'symmetric', axis=-1), wo.colfilter(x, e), wo.rowfilter(x, f),
                wo.coldfilt(x, ga, gb), wo.rowdfilt(x, ga, gb, highpass=True), wo.colifilt(x, ga, gb), wo.rowifilt(x, ga, gb, highpass=True),
                z1r, z1i, z2r, z2i, wo.c2q((z1r, z1i), (z2r, z2i))]
        # (q2c / c2q are tensor-library arithmetic in the data dtype, as upstream: a scaling and a sum, two roundings)
        return [(o, MULTI if i == 2 or i >= 9 else ONE) for i, o in enumerate(outs)]
    return Case(name, [shape], make, oracle, family)


def rounding_check(dev):
    """A float32 DWTForward(J=1, db2, zero) on bfloat16 data: the stores round to nearest even - at least 99.9 % of the
    outputs bit-equal to RNE(float32(oracle)), the rest exactly 1 ulp away (a truncating conversion fails)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 128, generator=g).to(BF)
    m = pw.DWTForward(J=1, wave='db2', mode='zero').to(dev)
    yl, yh = m(x.to(dev))
    h0, h1 = (np.asarray(h, dtype=np.float32).astype(np.float64) for h in F.dwt_analysis_taps('db2'))
    oyl, oyh = wo.dwt_forward(x.double().numpy(), 1, h0, h1, h0, h1, 'zero')
    got = torch.cat([yl.detach().cpu().reshape(-1), yh[0].detach().cpu().reshape(-1)])
    want = torch.cat([torch.tensor(oyl).reshape(-1), torch.tensor(oyh[0]).reshape(-1)]).float().to(BF)
    assert got.dtype == BF
    gi, wi = got.view(torch.int16).int(), want.view(torch.int16).int()
    d = (gi - wi).abs()
    same = float((d == 0).double().mean())
    assert same >= 0.999 and int(d.max()) <= 1, (same, int(d.max()))
    return same
