"""Shared checks of SWT1DShrink - lowlevel.swt1d_shrink, ops.shrink1d_fwd / shrink1d_bwd, swt1d_universal_thresh and the wave-tile
kernels of csrc/wl_shrink1d.h -, run by the emulator (CPU) and the GPU test modules.

The oracle is the float64 chain of tests/_swt1d_cases.py - ``analysis_ref`` with the analysis taps, numpy shrinkage,
``adjoint_ref`` with the synthesis taps and 1/2 per level - on the module's float32 taps and on x as stored.  The gradients are
the definition's: (dlo, dhi) = analysis_ref(dy, g, 1/2), dhi *= [|hi| > t], dx = adjoint_ref(dlo, dhi, h, 1),
dt = - sum sign(hi) [|hi| > t] dhi (soft; zeros for hard).

Tolerances are those of tests/_swt1d_cases.py: values absolute, times max(1, |x|max) - REC float32 2e-5, float16 6e-3,
REL[bfloat16] 3e-2 -; gradients relative to |ref|max with REL; dt, a cancelling sum, REL * sum |terms| from the oracle.  Only
on rows shorter than the filter (n = 1, 3, 5), whose highpasses cancel inside every dot product, that bound is not taken below
one ``_swt1d_cases.cancel_floor`` (``dt_floor``).

A threshold is a discontinuity.  Soft VALUES are 1-Lipschitz in w and t and are checked on random rows.  Masks, hard values and
every gradient are checked on GAP rows: piecewise-constant rows whose jumps all have one amplitude +-A, plus noise of 1e-3 A,
so that each level's magnitudes take few distinct values; t_j[c] is the midpoint of the widest gap between consecutive sorted
magnitudes (0 included) of level j over the rows of channel c.  Before the engine runs, the oracle alone must show that every
||w| - t| is at least 4 REL[dtype] |w|max of its level and, for rows of 37 samples and more, that each level keeps between
10 % and 90 % of its coefficients.  Jumps spaced wider than the filters' reach cannot meet the second condition (the finest
level then keeps a handful of coefficients out of hundreds) and for long filters not the first (an isolated step's response
samples a smooth curve densely: its widest gap is 0.14 |w|max at db10's level 3, bfloat16 asks for 0.24), so the spacing is
what is tuned: the jumps follow a PERIODIC pattern of a short period P - a level then takes at most P magnitudes, each many
times - chosen per (wave, J, shape, dtype) by a search on the CPU (``find_gap_pattern``), whose results for the long rows are
kept in tests/golden/shrink1d_gap_patterns.json."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import _lib, ops
import _swt1d_cases as W

F64, F32, F16, BF16 = W.F64, W.F32, W.F16, W.BF16
REL = W.REL
VAL = {F64: 1e-12, F32: W.REC[F32], F16: W.REC[F16], BF16: W.REL[BF16]}
WAVES, LEVELS, ROWS = W.WAVES, W.LEVELS, W.ROWS
KINDS = ('soft', 'hard')
npy, dev_t, ntaps, ana_taps, syn_taps = W.npy, W.dev_t, W.ntaps, W.ana_taps, W.syn_taps
A = 1.0                 # the jumps' amplitude


def core_of(wave, J):
    return ops.shrink1d_core(ntaps(wave), min(J, 3))


def lens(wave, J):
    core = core_of(wave, J)
    return (1, 3, 5, 37, 64, core - 1, core, core + 1, 2 * core + 3)


def names_since(c0):
    return [k.split('<')[0] for k in pw.kernels_since(c0)]


def module(dev, wave, J, kind='soft', dtype=F32, **kw):
    """(the buffers are float32 whatever the data: the oracle runs on those taps for float64 rows too)"""
    return pw.SWT1DShrink(J=J, wave=wave, kind=kind, **kw).to(dev)


# ---------------------------------------------------------------------------------------------- the oracle
def shrink_np(w, t, kind):
    if kind == 'soft':
        return np.sign(w) * np.maximum(np.abs(w) - t, 0.0)
    return w * (np.abs(w) > t)


def coeffs_ref(x, wave, J):
    """(lo_J, [hi_1 ..]) of x (N, C, n), float64."""
    return W.analysis_ref(x, ana_taps(wave), J)


def forward_ref(x, thr, wave, J, kind):
    """y of x (N, C, n) under thr (J, N, C)."""
    lo, his = coeffs_ref(x, wave, J)
    return W.adjoint_ref(lo, [shrink_np(h, thr[j][..., None], kind) for j, h in enumerate(his)], syn_taps(wave), 0.5)


def backward_ref(x, dy, thr, wave, J, kind):
    """(dx, dt (J, N, C), sum |terms| of dt (J, N, C)); dt is zeros for hard."""
    _, his = coeffs_ref(x, wave, J)
    dlo, dhis = W.analysis_ref(dy, syn_taps(wave), J, scale=0.5)
    masks = [np.abs(h) > thr[j][..., None] for j, h in enumerate(his)]
    dx = W.adjoint_ref(dlo, [d * m for d, m in zip(dhis, masks)], ana_taps(wave), 1.0)
    terms = [-np.sign(h) * m * d for h, m, d in zip(his, masks, dhis)]
    dt = np.stack([t.sum(-1) for t in terms]) * (kind == 'soft')
    return dx, dt, np.stack([np.abs(t).sum(-1) for t in terms])


def dt_floor(wave, dy, n, dtype):
    """The bound of dt is the issue's, REL * sum |terms|, on every row at least as long as the filter.  A row SHORTER than the
    filter (n = 1, 3, 5 of the grid, by the bank) wraps inside every dot product: the folded taps of a highpass cancel, a
    one-sample row's to exactly 0, and dhi - so every term - is small against the dy it is summed from (sum |terms| is 0 at
    n = 1 and 1e-3 of |dy| at n = 3 under 20 taps), while a float32 dot product is accurate relative to its sources.  There,
    and only there, the bound is not below ONE ``_swt1d_cases.cancel_floor`` - what an L-term float32 dot product may leave of
    a band that cancels, the floor the stationary transform's own highpass checks have -, not scaled by the rows, the levels
    or the length (measured on such rows: at most 1.1e-7, under floors of 8e-7 to 2.9e-6).  float64 has no floor."""
    return W.cancel_floor(syn_taps(wave), dy) if n < ntaps(wave) and dtype != F64 else 0.0


def close_values(y, ref, x, dtype, what):
    err = float(np.abs(npy(y) - ref).max())
    bound = VAL[dtype] * max(1.0, float(np.abs(x).max()))
    print('%s: max err %.3e, bound %.3e' % (what, err, bound))
    assert tuple(y.shape) == ref.shape and y.dtype == dtype, (what, y.shape, y.dtype)
    assert err <= bound, (what, err, bound)


def close_dt(dt, ref, mags, dtype, floor, what):
    err = np.abs(npy(dt) - ref)
    bound = np.maximum(REL[dtype] * mags, floor)
    print('%s: max err %.3e, least bound %.3e' % (what, float(err.max()), float(bound.min())))
    assert tuple(dt.shape) == ref.shape, (what, dt.shape)
    assert bool((err <= bound).all()), (what, err, bound)


# ---------------------------------------------------------------------------------------------- random rows: soft values
@functools.lru_cache(maxsize=None)
def _random(shape, seed):
    """(x, dy): float64 numpy, made once per shape and shared (never written to)."""
    rng = np.random.RandomState(seed)
    return rng.randn(*shape), rng.randn(*shape)


def quantile_thresholds(his, form):
    """Thresholds of one of the three accepted forms from the oracle's magnitudes, as (what the module is handed, its (J, N, C)
    expansion)."""
    J, (N, C) = len(his), his[0].shape[:2]
    if form == 'scalar':
        t = np.float64(np.quantile(np.abs(np.stack(his)), 0.5))
        return t, np.full((J, N, C), t)
    if form == 'levels':
        t = np.array([np.quantile(np.abs(h), 0.6) for h in his])
        return t, np.broadcast_to(t[:, None, None], (J, N, C)).copy()
    t = np.stack([np.quantile(np.abs(h), 0.4, axis=-1) for h in his])
    return t, t


def check_soft_values(dev, wave, J, shape, dtype=F32, forms=('scalar', 'levels', 'table')):
    """y of random rows under quantile thresholds of the three forms; one WlShrink1dFwd launch for J <= 3 (none for J = 5 and
    for float64, which take the composition)."""
    x = dev_t(_random(shape, 41)[0], dtype, dev)
    mod = module(dev, wave, J, 'soft', dtype)
    his = coeffs_ref(npy(x), wave, J)[1]
    for form in forms:
        given, table = quantile_thresholds(his, form)
        # (the table the kernel reads is float32: the oracle uses what it holds)
        t32 = np.asarray(given, dtype=np.float64 if dtype == F64 else np.float32)
        table = np.broadcast_to(t32.astype(np.float64).reshape((-1, 1, 1) if t32.ndim == 1 else t32.shape), table.shape)
        c0 = pw.launch_count()
        y = mod(x, torch.tensor(t32).to(dev))
        ks = names_since(c0)
        if J <= 3 and dtype != F64:
            assert ks == ['WlShrink1dFwd'], (wave, J, shape, form, ks)
        else:
            assert ks and not any(k.startswith('WlShrink1d') for k in ks), (wave, J, shape, form, ks)
        close_values(y, forward_ref(npy(x), table, wave, J, 'soft'), npy(x), dtype, 'soft y %s J=%d %s %s %s' % (wave, J, shape, form, dtype))
        assert y.is_contiguous()


# ---------------------------------------------------------------------------------------------- gap rows
# tests/golden/shrink1d_gap_patterns.json: rows [wave, J, shape, dtype name, P, seed] - the pattern ``gap_pattern`` makes, as
# ``find_gap_pattern`` found it on the CPU, for the rows of 37 samples and more.  It is a cache of that search and nothing else:
# a key that is absent (shorter rows; the 2-byte rows of check_instantiation, whose float32 margin the first few periods meet;
# any shape a later change of the grid brings) takes the first pattern the search finds at test time, and gap_case asserts the
# conditions on whatever it was handed.  A seed that is a list holds the residues mod P themselves.
def _load_gap_patterns():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shrink1d_gap_patterns.json')
    with open(path) as f:
        return {(w, J, tuple(shape), dt): (P, tuple(seed) if isinstance(seed, list) else seed) for w, J, shape, dt, P, seed in json.load(f)}


GAP_PATTERNS = _load_gap_patterns()


def gap_pattern(n, P, seed):
    """A row of n samples, values on the lattice A * k: jumps of +-A at the positions p with pattern[p mod P] set, their signs
    alternating (an odd count drops the last), so that the row closes on itself."""
    if isinstance(seed, tuple):             # the residues themselves (the bfloat16 cells a seeded draw did not reach)
        pat = np.zeros(P, dtype=bool)
        pat[list(seed)] = True
    else:
        rng = np.random.RandomState(1000 * P + seed)
        pat = rng.rand(P) < rng.choice([0.2, 0.35, 0.5])
        if not pat.any():
            pat[rng.randint(P)] = True
    pos = np.nonzero(pat[np.arange(n) % P])[0]
    if len(pos) % 2:
        pos = pos[:-1]                  # (P divides n and the count is even: no irregular stretch anywhere on the circle)
    if n < 37:
        # rows shorter than the filters: a draw may leave no jump at all, and what a level makes of a constant is the rounding
        # of that constant, in any float32 engine - such a row has one jump up and one down, and no mean
        if len(pos) < 2 and n > 1:
            pos = np.array([0, (n + 1) // 2])
    jumps = np.zeros(n)
    jumps[pos[0::2]] = A
    jumps[pos[1::2]] = -A
    x = np.cumsum(jumps) - 0.5 * A
    return x - x.mean() if 1 < n < 37 else x


def gap_rows(shape, P, seed, dtype):
    """x (N, C, n) as stored in `dtype`, float64: every row the pattern, shifted by a different amount, with its own noise of
    1e-3 A."""
    N, C, n = shape
    rng = np.random.RandomState(77 + (len(seed) if isinstance(seed, tuple) else seed))
    base = gap_pattern(n, P, seed)
    x = np.stack([np.roll(base, (3 * i) % n) for i in range(N * C)]).reshape(N, C, n) + 1e-3 * A * rng.randn(N, C, n)
    return torch.tensor(x).to(dtype).double().numpy()


def gap_thresholds(his):
    """t (J, 1, C): per level and channel the midpoint of the widest gap between consecutive sorted magnitudes, 0 included."""
    out = []
    for h in his:
        row = []
        for c in range(h.shape[1]):
            m = np.sort(np.concatenate(([0.0], np.abs(h[:, c]).ravel())))
            k = int(np.argmax(np.diff(m)))
            row.append(0.5 * (m[k] + m[k + 1]))
        out.append(row)
    return np.array(out)[:, None, :]


def gap_conditions(his, thr, dtype, n):
    """The two conditions on the oracle alone, as a list of what fails."""
    bad = []
    for j, h in enumerate(his):
        a = np.abs(h)
        t = thr[j][..., None]
        margin, need = float(np.abs(a - t).min()), 4 * REL[dtype] * float(a.max())
        if margin < need:
            bad.append('level %d: a coefficient %.3e from its threshold, %.3e asked' % (j + 1, margin, need))
        kept = (a > t).mean(axis=(0, 2))
        if n >= 37 and not bool(((kept >= 0.1) & (kept <= 0.9)).all()):
            bad.append('level %d keeps %s of its coefficients' % (j + 1, kept))
    return bad


def find_gap_pattern(wave, J, shape, dtype, periods=range(2, 129), seeds=range(12), margin=None):
    """The first (P, seed) whose rows meet both conditions: periods that divide n first (no irregular stretch at the wrap)."""
    n = shape[-1]
    order = sorted(periods, key=lambda P: (n % P != 0, P))
    for P in order:
        for seed in seeds:
            x = gap_rows(shape, P, seed, dtype)
            his = coeffs_ref(x, wave, J)[1]
            if not gap_conditions(his, gap_thresholds(his), margin or dtype, n):
                return P, seed
    return None


DTNAME = {F32: 'float32', F16: 'float16', BF16: 'bfloat16', F64: 'float64'}


@functools.lru_cache(maxsize=None)
def gap_case(wave, J, shape, dtype, margin=None):
    """(x, dy, thr (J, 1, C)) of a gap case, float64 numpy, the conditions asserted; made once and shared (never written to).
    `margin`: the type whose REL the first condition uses, where it is not the storage type (check_instantiation)."""
    n = shape[-1]
    found = GAP_PATTERNS.get((wave, J, shape, DTNAME[dtype])) if margin is None else None
    if found is None:
        found = find_gap_pattern(wave, J, shape, dtype, margin=margin)
    assert found is not None, 'no gap rows for %s J=%d %s %s' % (wave, J, shape, dtype)
    x = gap_rows(shape, found[0], found[1], dtype)
    his = coeffs_ref(x, wave, J)[1]
    thr = gap_thresholds(his)
    bad = gap_conditions(his, thr, margin or dtype, n)
    assert not bad, (wave, J, shape, dtype, found, bad)
    dy = torch.tensor(np.random.RandomState(43).randn(*shape)).to(dtype).double().numpy()
    return x, dy, thr


def check_gap(dev, wave, J, shape, dtype=F32, kinds=KINDS):
    """Hard and soft values, dx and dt on gap rows; the backward is one WlShrink1dBwd launch."""
    xn, dyn, thr = gap_case(wave, J, shape, dtype)
    N, C, n = shape
    # float32 holds the thresholds: the margin of the conditions covers their rounding (2^-24 relative)
    t32 = np.asarray(thr, dtype=np.float64 if dtype == F64 else np.float32)
    table = np.broadcast_to(t32.astype(np.float64), (J, N, C))
    fused = J <= 3 and dtype != F64
    for kind in kinds:
        mod = module(dev, wave, J, kind, dtype)
        x = dev_t(xn, dtype, dev).requires_grad_(True)
        t = torch.tensor(t32).to(dev).requires_grad_(True)
        c0 = pw.launch_count()
        y = mod(x, t)
        ks = names_since(c0)
        assert (ks == ['WlShrink1dFwd']) if fused else not any(k.startswith('WlShrink1d') for k in ks), (wave, J, shape, kind, ks)
        what = '%s %s J=%d %s %s' % (kind, wave, J, shape, dtype)
        close_values(y, forward_ref(xn, table, wave, J, kind), xn, dtype, 'y ' + what)
        c0 = pw.launch_count()
        dx, dt = torch.autograd.grad(y, (x, t), dev_t(dyn, dtype, dev))
        ks = names_since(c0)
        assert (ks == ['WlShrink1dBwd']) if fused else not any(k.startswith('WlShrink1d') for k in ks), (wave, J, shape, kind, ks)
        rdx, rdt, mags = backward_ref(xn, dyn, table, wave, J, kind)
        W.close(dx, rdx, dtype, 'dx ' + what, floor=W.cancel_floor(ana_taps(wave), dyn))
        assert dt.shape == t.shape and dt.dtype == t.dtype
        # (t is (J, 1, C): its gradient is the sum over the rows of a channel, and so is its bound)
        close_dt(dt, rdt.sum(1, keepdims=True), mags.sum(1, keepdims=True), dtype, dt_floor(wave, dyn, n, dtype), 'dt ' + what)
        if kind == 'hard':
            assert not bool(dt.any())


def check_grid(dev, wave, J):
    """Every length and row count of the table, float32: soft values on random rows, everything on gap rows."""
    for n in lens(wave, J):
        for lead in ROWS:
            check_soft_values(dev, wave, J, lead + (n,))
            check_gap(dev, wave, J, lead + (n,))


def check_two_byte(dev, wave, dtype):
    J = 3
    for n in (37, core_of(wave, J) + 1):
        check_soft_values(dev, wave, J, (2, 2, n), dtype)
        check_gap(dev, wave, J, (2, 2, n), dtype)


def check_float64(dev):
    """float64 takes the composition: the oracle's answers at its own precision, no WlShrink1d launch."""
    for wave in ('db4', 'db10'):
        check_soft_values(dev, wave, 3, (2, 2, 45), F64)
        check_gap(dev, wave, 2, (2, 2, 37), F64)


# ---------------------------------------------------------------------------------------------- instantiations
GRID_WAVES, GRID_DTYPES, TNAME = W.GRID_WAVES, W.GRID_DTYPES, W.TNAME


def check_instantiation(dev, wave, dtype):
    """WlShrink1dFwd<T, L> / WlShrink1dBwd<T, L> of one tap count and element type x nlev 1..3 through ops.shrink1d_fwd /
    shrink1d_bwd: three rows of one tile plus one position, which crosses the seam.  Soft values, dx and the dt partials on gap
    rows whose margin is float32's for every T: these kernels compute the coefficients from the stored x in float32 and never
    round them to T, so a coefficient's error - what the margin guards the mask against - is float32's whatever the storage
    (bfloat16's own margin, 0.24 |w|max between two magnitudes, has no such row at 14 to 18 taps and three levels; the
    2-byte margins are asked of check_two_byte)."""
    L = ntaps(wave)
    h, g = [dev_t(t, F32, dev) for t in ana_taps(wave)], [dev_t(t, F32, dev) for t in syn_taps(wave)]
    for nlev in (1, 2, 3):
        n = ops.shrink1d_core(L, nlev) + 1
        xn, dyn, thr = gap_case(wave, nlev, (1, 3, n), dtype, None if dtype == F32 else F32)
        table = np.broadcast_to(np.asarray(thr, dtype=np.float32).astype(np.float64), (nlev, 1, 3))
        x, dy = dev_t(xn, dtype, dev).reshape(3, n), dev_t(dyn, dtype, dev).reshape(3, n)
        t = torch.tensor(table.astype(np.float32)).reshape(nlev, 3).to(dev)
        c0 = pw.launch_count()
        y = ops.shrink1d_fwd(x, t, h[0], h[1], g[0], g[1], nlev, 'soft')
        dx, part = ops.shrink1d_bwd(x, dy, t, h[0], h[1], g[0], g[1], nlev, 'soft')
        ks = pw.kernels_since(c0)
        assert ks == ['WlShrink1d%s<%s, %d>' % (k, TNAME[dtype], L) for k in ('Fwd', 'Bwd')], ks
        what = '%s nlev=%d %s' % (wave, nlev, dtype)
        close_values(y.reshape(1, 3, n), forward_ref(xn, table, wave, nlev, 'soft'), xn, dtype, 'y ' + what)
        rdx, rdt, mags = backward_ref(xn, dyn, table, wave, nlev, 'soft')
        W.close(dx.reshape(1, 3, n), rdx, dtype, 'dx ' + what)
        assert tuple(part.shape) == (3, 2, nlev) and part.dtype == F32
        close_dt(part.sum(1).t().reshape(nlev, 1, 3), rdt, mags, dtype, dt_floor(wave, dyn, n, dtype), 'dt ' + what)


# ---------------------------------------------------------------------------------------------- seams and schedules
def fused_triple(dev, wave, J, shape, dtype, origin, kind='soft'):
    """(y, dx, dt (rows, J)): ops.shrink1d_fwd and ops.shrink1d_bwd of a gap case, the first tile moved left by `origin`."""
    xn, dyn, thr = gap_case(wave, J, shape, dtype)
    N, C, n = shape
    h, g = [dev_t(t, F32, dev) for t in ana_taps(wave)], [dev_t(t, F32, dev) for t in syn_taps(wave)]
    t = torch.tensor(np.broadcast_to(thr, (J, N, C)).astype(np.float32)).reshape(J, N * C).to(dev)
    x, dy = dev_t(xn, dtype, dev), dev_t(dyn, dtype, dev)
    y = ops.shrink1d_fwd(x, t, h[0], h[1], g[0], g[1], J, kind, origin=origin)
    dx, part = ops.shrink1d_bwd(x, dy, t, h[0], h[1], g[0], g[1], J, kind, origin=origin)
    assert part.shape[1] == -(-(n + origin) // ops.shrink1d_core(ntaps(wave), J))
    return y, dx, part.sum(1)


def check_origin(dev, wave, J, dtype=F32):
    """The seams of a row fall elsewhere: y and dx do not change by a bit.  The dt partials are sums over other sets of
    positions - the tiles are cut elsewhere -, so their total is compared within the dt bound."""
    core = core_of(wave, J)
    for n in (core + 1, 2 * core + 3, 37):
        shape = (2, 1, n)
        base = fused_triple(dev, wave, J, shape, dtype, 0)
        xn, dyn, thr = gap_case(wave, J, shape, dtype)
        table = np.broadcast_to(np.asarray(thr, dtype=np.float32).astype(np.float64), (J, 2, 1))
        _, rdt, mags = backward_ref(xn, dyn, table, wave, J, 'soft')
        for origin in (1, 5, core // 2):
            got = fused_triple(dev, wave, J, shape, dtype, origin)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (wave, J, n, origin)
            close_dt(got[2].t().reshape(J, 2, 1), rdt, mags, dtype, dt_floor(wave, dyn, n, dtype), 'dt %s J=%d n=%d origin %d' % (wave, J, n, origin))


def schedule_case(dev):
    """One forward + backward (db4, J = 3, (2, 1, core + 1)): everything that comes out, for a bitwise comparison."""
    return list(fused_triple(dev, 'db4', 3, (2, 1, core_of('db4', 3) + 1), F32, 0))


# ---------------------------------------------------------------------------------------------- identities and routes
class switch(object):
    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        self.prev, ops.SHRINK1D_FUSED = ops.SHRINK1D_FUSED, self.flag

    def __exit__(self, *exc):
        ops.SHRINK1D_FUSED = self.prev
        return False


def check_identities(dev, dtype=F32):
    """thresh = 0 gives x back within the round-trip bound; a threshold above every magnitude gives the inverse of (lo_J, zeros)."""
    for wave, n in (('db4', 37), ('bior2.2', 64), ('db10', core_of('db10', 3) + 1)):
        for kind in KINDS:
            x = dev_t(_random((2, 2, n), 44)[0], dtype, dev)
            y = module(dev, wave, 3, kind)(x)
            close_values(y, npy(x), npy(x), dtype, 'thresh 0 %s %s n=%d' % (kind, wave, n))
            lo, his = coeffs_ref(npy(x), wave, 3)
            top = 2.0 * max(float(np.abs(h).max()) for h in his)
            y = module(dev, wave, 3, kind, thresh=top)(x)
            close_values(y, W.adjoint_ref(lo, [None] * 3, syn_taps(wave), 0.5), npy(x), dtype, 'thresh above all %s %s n=%d' % (kind, wave, n))


def check_switch(dev, dtype=F32):
    """ops.SHRINK1D_FUSED = False: the composition, the same answers within the tolerances, no WlShrink1d launch."""
    for wave, n in (('db4', 37), ('db10', core_of('db10', 3) + 1)):
        shape = (2, 2, n)
        xn, dyn, thr = gap_case(wave, 3, shape, dtype)
        for kind in KINDS:
            mod = module(dev, wave, 3, kind)
            outs = {}
            for flag in (True, False):
                with switch(flag):
                    x = dev_t(xn, dtype, dev).requires_grad_(True)
                    t = torch.tensor(thr.astype(np.float32)).to(dev).requires_grad_(True)
                    c0 = pw.launch_count()
                    y = mod(x, t)
                    dx, dt = torch.autograd.grad(y, (x, t), dev_t(dyn, dtype, dev))
                    ks = names_since(c0)
                assert (ks == ['WlShrink1dFwd', 'WlShrink1dBwd']) if flag else not any(k.startswith('WlShrink1d') for k in ks), (flag, ks)
                outs[flag] = (y.detach(), dx, dt)
            what = '%s %s n=%d' % (kind, wave, n)
            close_values(outs[True][0], npy(outs[False][0]), xn, dtype, 'fused against composed y ' + what)
            W.close(outs[True][1], npy(outs[False][1]), dtype, 'fused against composed dx ' + what)
            table = np.broadcast_to(thr.astype(np.float32).astype(np.float64), (3, 2, 2))
            mags = backward_ref(xn, dyn, table, wave, 3, kind)[2].sum(1, keepdims=True)
            close_dt(outs[True][2], npy(outs[False][2]), 2 * mags, dtype, dt_floor(wave, dyn, n, dtype), 'fused against composed dt ' + what)


def check_a_declined_launch_composes(dev):
    """A launcher that declines a call the Python envelope let through (a memoised decline, an engine option): the forward takes
    the composition, and a backward that is declined behind a fused forward differentiates the composition."""
    n = core_of('db4', 3) + 1
    xn, dyn, thr = gap_case('db4', 3, (2, 2, n), F32)
    mod = module(dev, 'db4', 3, 'soft')
    outs = {}
    for declined in ((), ('shrink1d_fwd',), ('shrink1d_bwd',)):
        saved = {name: getattr(ops, name) for name in declined}
        for name in declined:
            setattr(ops, name, lambda *a, **k: None)
        try:
            x = dev_t(xn, F32, dev).requires_grad_(True)
            t = torch.tensor(thr.astype(np.float32)).to(dev).requires_grad_(True)
            c0 = pw.launch_count()
            y = mod(x, t)
            kf = names_since(c0)
            c0 = pw.launch_count()
            dx, dt = torch.autograd.grad(y, (x, t), dev_t(dyn, F32, dev))
            kb = names_since(c0)
        finally:
            for name, fn in saved.items():
                setattr(ops, name, fn)
        assert (kf == ['WlShrink1dFwd']) == ('shrink1d_fwd' not in declined), (declined, kf)
        assert (kb == ['WlShrink1dBwd']) == (not declined), (declined, kb)
        assert kb and not (declined and any(k.startswith('WlShrink1d') for k in kb)), (declined, kb)
        outs[declined] = (y.detach(), dx, dt)
    table = np.broadcast_to(thr.astype(np.float32).astype(np.float64), (3, 2, 2))
    mags = backward_ref(xn, dyn, table, 'db4', 3, 'soft')[2].sum(1, keepdims=True)
    for declined in (('shrink1d_fwd',), ('shrink1d_bwd',)):
        close_values(outs[declined][0], npy(outs[()][0]), xn, F32, 'y with %s declined' % declined)
        W.close(outs[declined][1], npy(outs[()][1]), F32, 'dx with %s declined' % declined)
        close_dt(outs[declined][2], npy(outs[()][2]), 2 * mags, F32, 0.0, 'dt with %s declined' % declined)


def check_no_partials_without_a_learned_threshold(dev):
    """learn=False and a threshold that asks for no gradient: the backward launch gets a null dthr_part and allocates none; a
    learned threshold gets the buffer.  The C entry accepts the null pointer and writes the same dx."""
    n = core_of('db4', 3) + 1
    xn, dyn, thr = gap_case('db4', 3, (2, 2, n), F32)
    seen, call0 = [], ops._call

    def call(name, ref, *args):
        if name == 'wl_shrink1d_backward':
            seen.append(args[4])
        return call0(name, ref, *args)

    ops._call = call
    try:
        outs = []
        for learn in (False, True):
            mod = module(dev, 'db4', 3, 'soft', thresh=torch.tensor(thr.astype(np.float32)), learn=learn)
            x = dev_t(xn, F32, dev).requires_grad_(True)
            c0 = pw.launch_count()
            mod(x).backward(dev_t(dyn, F32, dev))
            assert names_since(c0) == ['WlShrink1dFwd', 'WlShrink1dBwd']
            outs.append(x.grad)
            assert (mod.thresh.grad is not None) == learn and isinstance(mod.thresh, torch.nn.Parameter) == learn
    finally:
        ops._call = call0
    assert seen[0] is None and seen[1] is not None, seen
    assert torch.equal(outs[0], outs[1]) and tuple(mod.thresh.grad.shape) == (3, 1, 2)


# ---------------------------------------------------------------------------------------------- gradcheck
def check_gradcheck(dev):
    """torch.autograd.gradcheck of the float64 composition with respect to x and thresh: db2, J = 2, 12 samples, soft,
    gap-chosen thresholds (a finite difference across a threshold is no derivative)."""
    xn, _, thr = gap_case('db2', 2, (1, 2, 12), F64)
    mod = module(dev, 'db2', 2, 'soft', F64)
    x = dev_t(xn, F64, dev).requires_grad_(True)
    t = dev_t(thr, F64, dev).requires_grad_(True)
    his = coeffs_ref(xn, 'db2', 2)[1]
    assert min(float(np.abs(np.abs(h) - thr[j][..., None]).min()) for j, h in enumerate(his)) > 1e-4      # (eps = 1e-6 stays inside)
    c0 = pw.launch_count()
    assert torch.autograd.gradcheck(lambda a, b: mod(a, b), (x, t), eps=1e-6, atol=1e-7)
    assert not any(k.startswith('WlShrink1d') for k in names_since(c0))


# ---------------------------------------------------------------------------------------------- errors and edges
def check_errors_and_edges(dev):
    x = dev_t(_random((2, 2, 20), 45)[0], F32, dev)
    assert module(dev, 'db2', 0)(x) is x
    with pytest.raises(ValueError, match="'periodic' only"):
        module(dev, 'db2', 1, mode='symmetric')(x)
    with pytest.raises(ValueError, match='even number of taps'):
        module(dev, W.ODD_PAIR, 1)(x)
    with pytest.raises(ValueError, match="'soft' or 'hard'"):
        pw.SWT1DShrink(kind='garrote')
    with pytest.raises(ValueError):
        module(dev, 'db2', 1)(x[None])
    mod = module(dev, 'db2', 2)
    for bad in ((3,), (2, 2), (2, 3, 2), (2, 2, 2, 1), (1, 2, 3)):
        with pytest.raises(ValueError, match='thresh must be'):
            mod(x, torch.zeros(bad, device=dev))
    for good in ((), (2,), (1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (2, 2, 2)):
        assert mod(x, torch.full(good, 0.1, device=dev)).shape == x.shape
    assert torch.equal(mod(x, 0.1), mod(x, torch.full((2, 2, 2), 0.1, device=dev)))
    # the C entries outside their envelope
    h = [dev_t(t, F32, dev) for t in ana_taps('db2') + syn_taps('db2')]
    thr = torch.full((1, 4), 0.1, device=dev)
    y, part = torch.empty_like(x), torch.empty(4, 1, 1, device=dev)
    be, unsupported, shape_err = ops._backend(), _lib.WL_ERR_UNSUPPORTED, -2
    taps = tuple(t.data_ptr() for t in h)

    def fwd(dtype=0, rows=4, n=20, J=1, L=4, kind=0, origin=0):
        return be.wl_shrink1d_forward(x.data_ptr(), y.data_ptr(), thr.data_ptr(), dtype, rows, n, J, *(taps + (L, kind, origin, None)))

    def bwd(dtype=0, rows=4, n=20, J=1, L=4, kind=0, origin=0):
        return be.wl_shrink1d_backward(x.data_ptr(), x.data_ptr(), y.data_ptr(), thr.data_ptr(), part.data_ptr(), dtype, rows, n, J,
                                       *(taps + (L, kind, origin, None)))

    for entry in (fwd, bwd):
        assert entry(dtype=2) == unsupported                       # float64
        assert entry(L=3) == unsupported and entry(L=22) == unsupported
        assert entry(J=4) == unsupported and entry(J=0) == shape_err
        assert entry(kind=2) == unsupported
        assert entry(n=0) == shape_err and entry(rows=-1) == shape_err
        assert entry(origin=-1) == shape_err and entry(origin=ops.shrink1d_core(4, 1)) == shape_err
        assert entry(rows=0) == 0
    c0 = pw.launch_count()
    assert fwd(rows=0) == 0 and bwd(rows=0) == 0 and pw.launch_count() == c0
    assert be.wl_shrink1d_forward(None, y.data_ptr(), thr.data_ptr(), 0, 4, 20, 1, *(taps + (4, 0, 0, None))) == shape_err
    # the wrappers outside the envelope decline
    assert ops.shrink1d_fwd(x.double(), thr, h[0], h[1], h[2], h[3], 1) is None
    assert ops.shrink1d_fwd(x, thr, h[0][:3], h[1][:3], h[2], h[3], 1) is None
    assert ops.shrink1d_fwd(x, torch.zeros(4, 4, device=dev), h[0], h[1], h[2], h[3], 4) is None
    assert ops.shrink1d_bwd(x.double(), x.double(), thr, h[0], h[1], h[2], h[3], 1) is None
    assert ops.shrink1d_core(20, 3) == 758 and ops.shrink1d_core(2, 3) == 1010
    # the module: buffers, the parameter, DWT1DForward's state
    mod = module(dev, 'db5', 2, learn=True, thresh=[0.1, 0.2])
    assert sorted(mod.state_dict()) == ['g0', 'g1', 'h0', 'h1', 'thresh']
    assert [k for k, _ in mod.named_parameters()] == ['thresh'] and mod.thresh.requires_grad
    assert [k for k, _ in module(dev, 'db5', 2).named_parameters()] == []
    res = mod.load_state_dict(pw.DWT1DForward(J=2, wave='sym5').to(dev).state_dict(), strict=False)
    assert sorted(res.missing_keys) == ['g0', 'g1', 'thresh'] and not res.unexpected_keys
    assert torch.equal(mod.h0, pw.DWT1DForward(wave='sym5').h0.to(dev)) and torch.equal(mod.h1, pw.DWT1DForward(wave='sym5').h1.to(dev))
    assert torch.equal(mod.h0, pw.SWT1DForward(wave='sym5').h0.to(dev))
    assert 'SWT1DShrink' in pw.__all__ and 'swt1d_universal_thresh' in pw.__all__


def check_cpu_tensor_raises():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.SWT1DShrink(J=2, wave='db2')(torch.zeros(1, 1, 16))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pw.SWT1DShrink(J=5, wave='db2')(torch.zeros(1, 1, 16))


def check_views(dev):
    """x[..., 1:-1] and x[:, 1:] give the bits of their contiguous copies, forward and backward."""
    n = core_of('db4', 3) + 3
    base = dev_t(_random((2, 3, n), 46)[0], F32, dev)
    mod = module(dev, 'db4', 3, thresh=0.5)
    for cut in (lambda t: t[..., 1:-1], lambda t: t[:, 1:]):
        view = cut(base).detach().requires_grad_(True)
        copy = view.detach().contiguous().requires_grad_(True)
        assert not view.is_contiguous()
        ya, yb = mod(view), mod(copy)
        assert torch.equal(ya, yb)
        g = cut(base.flip(-1))
        assert not g.is_contiguous()
        da, = torch.autograd.grad(ya, view, g)
        db, = torch.autograd.grad(yb, copy, g.contiguous())
        assert torch.equal(da, db)


def check_universal_thresh(dev, dtype=F32):
    """swt1d_universal_thresh against its numpy restatement."""
    for wave, n in (('db4', 37), ('haar', 64), ('db10', 1500)):
        x = dev_t(_random((2, 3, n), 47)[0], dtype, dev)
        t = pw.swt1d_universal_thresh(x, wave, 3)
        hi = coeffs_ref(npy(x), wave, 1)[1][0]
        # torch.median of an even count is the lower of the two middle values
        sigma = np.sort(np.abs(hi), axis=-1)[..., (n - 1) // 2] / 0.6745
        ref = np.broadcast_to(sigma * np.sqrt(2.0 * np.log(n)), (3, 2, 3))
        assert tuple(t.shape) == (3, 2, 3) and t.dtype == F32 and not t.requires_grad
        err = float(np.abs(npy(t) - ref).max())
        assert err <= REL[dtype] * float(np.abs(ref).max()), (wave, n, err)
        y = pw.SWT1DShrink(J=3, wave=wave).to(dev)(x, t)
        assert y.shape == x.shape and bool(torch.isfinite(y).all())
