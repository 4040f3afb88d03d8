"""CPU tests of the large-tensor harness (tests/_large_cases.py): its checker catches planted address wraps and names the right
plane and side of the threshold, its stretching oracle is the oracle of the full plane, the arithmetic of every table row holds
(thresholds crossed by three planes, the prime condition, at most 48 GiB), and every row and envelope object runs through the
host emulation of the kernels at a scaled-down count with the builders and the checker that run on the chip."""
import numpy as np
import pytest
import torch

import _large_cases as L
import emu_backend
from pytorch_wavelets_amd import _lib, ops

F32, F16, F64 = L.F32, L.F16, L.F64
P, PLANE = 5, (6, 7)
COUNT = 3 * P + 1


def _planted(dtype):
    """A correct output of COUNT planes, its reference, the scaled thresholds and the bound."""
    rng = np.random.RandomState(1)
    ref = torch.tensor(rng.randn(P, 1, *PLANE)).to(dtype)
    out = L.periodic_planes(ref, COUNT)
    pb = int(np.prod(PLANE)) * L.esize(dtype)
    b32 = (P * pb + pb // 2) // 16 * 16          # (every scaled threshold on an element boundary)
    ths = L.thresholds(dtype, b32)
    assert all(t < out.numel() * L.esize(dtype) for _, t in ths) and L.prime_ok(pb, P, dtype, b32)
    return out, ref.double(), ths, 1e-6


@pytest.mark.parametrize('dtype', [F32, F16])
def test_the_untouched_output_passes(dtype):
    out, ref, ths, bound = _planted(dtype)
    assert L.compare_planes(out, ref, P, bound, 'untouched', ths) == 0.0


@pytest.mark.parametrize('dtype', [F32, F16])
@pytest.mark.parametrize('which', [0, 1, 2])
def test_a_wrapped_address_is_reported_at_its_threshold(dtype, which):
    """everything past threshold `which` replaced by what lies that far below it"""
    out, ref, ths, bound = _planted(dtype)
    name, t = ths[which]
    w = t // L.esize(dtype)
    flat = out.reshape(-1).clone()
    flat[w:] = out.reshape(-1)[:flat.numel() - w]
    with pytest.raises(L.Mismatch) as ei:
        L.compare_planes(flat.view(out.shape), ref, P, bound, 'wrapped', ths)
    e, pe = ei.value, int(np.prod(PLANE))
    assert e.plane == w // pe and w <= e.elem < w + 3 and e.byte == e.elem * L.esize(dtype), (e.plane, e.elem, w)
    assert e.sides == {n: ('at or above' if t2 <= t else 'below') for n, t2 in ths}, e.sides
    assert 'at or above ' + name in str(e) and 'plane / row %d' % (w // pe) in str(e)


@pytest.mark.parametrize('dtype', [F32, F16])
def test_an_unwritten_upper_part_is_reported(dtype):
    out, ref, ths, bound = _planted(dtype)
    w = ths[1][1] // L.esize(dtype)
    for sentinel in (float('nan'), 12345.0):
        flat = out.reshape(-1).clone()
        flat[w:] = sentinel
        with pytest.raises(L.Mismatch) as ei:
            L.compare_planes(flat.view(out.shape), ref, P, bound, 'sentinel', ths)
        assert ei.value.plane == w // int(np.prod(PLANE)) and ei.value.elem == w and ei.value.sides['2^32 bytes'] == 'at or above'


def test_one_wrong_element_in_the_last_plane_is_reported():
    out, ref, ths, bound = _planted(F32)
    flat = out.reshape(-1).clone()
    flat[-3] += 1e-3
    with pytest.raises(L.Mismatch) as ei:
        L.compare_planes(flat.view(out.shape), ref, P, bound, 'last', ths)
    assert ei.value.plane == COUNT - 1 and ei.value.elem == flat.numel() - 3
    assert all(s == 'at or above' for s in ei.value.sides.values())


def test_the_stretched_checker_reports_the_row():
    rng = np.random.RandomState(2)
    short = torch.tensor(rng.randn(1, 1, 20, 6))
    idx = L.stretch_index(44, 20, 8)
    out = short.index_select(2, idx).float().contiguous()
    assert L.compare_stretched(out, short, {2: 8}, 1e-6) < 1e-6
    out[0, 0, 37, 4] += 1e-3
    ths = L.thresholds(F32, 4 * (30 * 6))
    with pytest.raises(L.Mismatch) as ei:
        L.compare_stretched(out, short, {2: 8}, 1e-6, 'row', ths)
    assert ei.value.plane == 37 and ei.value.elem == 37 * 6 + 4 and ei.value.sides['2^32 bytes'] == 'at or above'
    assert ei.value.sides['2^31 elements'] == 'below'


def test_stretch_index():
    idx = L.stretch_index(28, 12, 4).tolist()
    assert idx[:4] == [0, 1, 2, 3] and idx[-4:] == [8, 9, 10, 11] and idx[4:24] == [4, 5, 6, 7] * 5
    assert L.stretch_index(12, 4, 4).tolist() == [0, 1, 2, 3] * 3          # (plain tiling)


# ---- the fold of an axis whose doubled length is no int -----------------------------------------------------------------------------
def _fold(i, n, rule):
    """half-sample symmetric (rule 1) / whole-sample reflect (rule 2) extension in Python integers"""
    p = 2 * n if rule == 1 else 2 * n - 2
    j = i % p
    return j if j < n else p - (1 if rule == 1 else 0) - j


@pytest.mark.parametrize('n', [37, 2 ** 30 - 1, 2 ** 30, 1064 * 1020000, 2 ** 31 - 1])
def test_the_single_axis_fold_beyond_2_to_the_30(n):
    """Above 2**30 samples the period of the fold - 2n, 2n - 2 - does not fit an int: the level-by-level route of a 1-D transform
    (the 1-D dual-tree above its fused kernel's limit) returned wrong samples at both ends of the row."""
    ext = emu_backend.ext_any_fn()
    for rule in (ops.EXT_SYM, ops.EXT_REFL):
        for i in (-19, -2, -1, 0, 5, n - 1, n, n + 1, n + 18):
            if i < 2 ** 31:          # (wl_corr1d refuses a call whose positions leave the int range)
                assert ext(i, n, rule) == _fold(i, n, rule), (i, n, rule)


def test_the_single_axis_entries_refuse_what_their_ints_cannot_hold():
    """wl_corr1d_adj walks extended positions up to 2n + the pad in an int: it ends at 2**30 samples (NotImplementedError in
    Python).  wl_corr1d forms start + step k + tap_step t in an int: a row within a filter length of 2**31 is refused.  Both return
    before anything is launched - the buffers here are a few bytes."""
    lib = emu_backend.handle()
    t = torch.zeros(16)
    p, f32, unsupported = t.data_ptr(), ops._DTYPES[F32], _lib.WL_ERR_UNSUPPORTED
    for ext in (ops.EXT_ZERO, ops.EXT_SYM, ops.EXT_REFL, ops.EXT_PERIODIC, ops.EXT_REPLICATE):
        assert lib.wl_corr1d_adj(p, 0, None, 0, p, f32, 1, 2 ** 30, 1, 2 ** 30, p, None, 4, -1, 1, ext, 1.0, None) == unsupported
    n = 2 ** 31 - 1
    assert lib.wl_corr1d(p, p, None, f32, 1, n, 1, n, n, p, None, 0, 1, 8, -3, 1, 1, ops.EXT_SYM, 0, 1, None) == unsupported
    with pytest.raises(NotImplementedError):
        _lib.check(unsupported, 'wl_corr1d_adj')


# ---- the tiling and stretching oracles --------------------------------------------------------------------------------------------
def _stretch_error(edge, short_reps, full_reps, T=None):
    """max |oracle(full) - stretched oracle(short)| over the outputs, float64, the other axes cut to a few samples"""
    T = T or edge.T
    shapes, _ = L.edge_shapes(edge, full_reps * T, cut=True)
    _, oracle = edge.tf.build('cpu', F64)
    rng = np.random.RandomState(3)
    periods = [rng.randn(*s) for s in L.edge_period_shapes(edge, shapes, full_reps * T, T)]
    ax = edge.in_axes
    full = oracle(*[np.concatenate([p] * full_reps, axis=a) for p, a in zip(periods, ax)])
    short = oracle(*[np.concatenate([p] * short_reps, axis=a) for p, a in zip(periods, ax)])
    err = 0.0
    for f, s, per in zip(full, short, edge.periods(T)):
        exp = torch.tensor(s)
        for a, p in per.items():
            exp = exp.index_select(a % exp.dim(), L.stretch_index(f.shape[a], s.shape[a], p))
        err = max(err, float(np.abs(exp.numpy() - f).max()))
    return err


@pytest.mark.parametrize('name', [e.name for e in L.EDGES if e.over is None])
def test_the_stretched_short_output_is_the_oracle_of_the_full_object(name):
    edge = L.EDGE_BY_NAME[name]
    short_reps = edge.short // edge.T
    assert edge.short >= L.min_short_len(edge.L, edge.J, edge.T)
    assert _stretch_error(edge, short_reps, short_reps + 5) <= 1e-12


@pytest.mark.parametrize('name', ['dwt2d-fwd-sym-j1-f32', 'dt2d-fwd-j2-f32', 'dt1d-fwd-j3-f32'])
def test_a_short_object_below_the_minimum_fails(name):
    """borders that reach the middle period: a period of 2**J samples, two of them"""
    edge = L.EDGE_BY_NAME[name]
    T = 2 ** edge.J
    assert 2 * T < L.min_short_len(edge.L, edge.J, T)
    assert _stretch_error(edge, 2, 9, T) > 1e-3


# ---- the table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [r.name for r in L.ROWS])
def test_a_row_crosses_its_thresholds_within_48_gib(name):
    row = L.BY_NAME[name]
    p = L.plan(row)
    L.check_plan(row, p)
    es = L.esize(row.dtype)
    assert max(p.in_bytes) > L.B32 and max(p.out_bytes) > L.B32
    if es == 2:
        assert max(p.in_bytes) // es > L.E31 and max(p.out_bytes) // es > L.E31


def test_the_float16_primitives_pass_2_to_the_31_elements():
    for name in ('afb1d-h-f16', 'afb1d-w-f16', 'sfb1d-h-f16', 'sfb1d-w-f16', 'filt-h-f16', 'filt-w-f16'):
        p = L.plan(L.BY_NAME[name])
        assert L.E31 <= p.count * p.out_planes[0] < 2 ** 32, name


@pytest.mark.parametrize('name', [e.name for e in L.EDGES])
def test_an_envelope_object_sits_at_its_limit(name):
    edge = L.EDGE_BY_NAME[name]
    n = int(np.prod(edge.measure(edge.shape)))
    assert (edge.limit_elems <= n <= 1.011 * edge.limit_elems) if edge.over is not None else (0.99 * edge.limit_elems <= n < edge.limit_elems), (n, edge.limit_elems)
    assert all(s & (s - 1) for s in edge.measure(edge.shape))           # no side a power of two
    assert edge.shape[edge.axis] % edge.T == 0 and edge.T % 2 ** edge.J == 0 and L.edge_need(edge, edge.shape) <= L.MAX_NEED


@pytest.mark.parametrize('name', [r.name for r in L.ROWS])
def test_a_row_scaled_down(name):
    row = L.BY_NAME[name]
    with emu_backend.emulated(), emu_backend.chip_of(8):
        res = L.run_row(row, 'cpu', count=3 * row.P + 1)
    assert res['count'] == 3 * row.P + 1 and all(e <= b for e, b in res['errs'])


@pytest.mark.parametrize('name', [e.name for e in L.EDGES])
def test_an_envelope_object_scaled_down(name):
    edge = L.EDGE_BY_NAME[name]
    with emu_backend.emulated(), emu_backend.chip_of(8):
        res = L.run_edge(edge, 'cpu', reps=edge.short // edge.T + 3)
    assert all(e <= b for e, b in res['errs'])
