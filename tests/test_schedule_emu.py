"""Every kernel family with LDS rings, LDS-DMA loaders or barrier-paced producer / consumer waves, on the host emulator under
every schedule it can take (tests/emu/wl_backend_emu.h, emu_backend.schedule): the fibres of a barrier phase alternating,
forward, backward, shuffled by waves, and LDS-DMA copies landing at the latest legal moment (late) or the earliest (eager).
A race between waves then shows as a difference: every case must give BITWISE the same results under every schedule (no
kernel here reduces with atomics) and pass the oracle checks of its shared helper.  Each case asserts by name the kernel
it is there for, so a later dispatch change fails it instead of leaving it vacuous.  test_every_barrier_kernel_has_a_case reads
the kernel headers and fails when a functor whose body has a barrier is named by no case."""
import contextlib
import glob
import os
import re

import numpy as np
import pytest
import torch

import emu_backend
import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import ops

import _bf16_cases as B
import _dtcwt1d_cases as D1
import _dtcwt_cases as D
import _ext_cases as E
import _lattice_cases as LC
import _nearsymb_cases as NB
import _packed_cases as PK
import _per_cases as PC
import _swt_inv_cases as SI
import _wpt2d_cases as WP
from pytorch_wavelets_amd.dwt import lowlevel as dwl

SCHEDULES = [('alternate', 'late', 0), ('forward', 'late', 0), ('reverse', 'late', 0), ('forward', 'eager', 0),
             ('reverse', 'eager', 0), ('shuffled', 'eager', 1), ('shuffled', 'eager', 2)]


@contextlib.contextmanager
def _recording(arrays, kernels):
    """Everything the case turns into numpy (the kernel outputs it compares with the oracle, gradients included) and every
    kernel launched, as (functor name, grid of the launch - None for an auxiliary or armed launch)."""
    numpy0, call0 = torch.Tensor.numpy, ops._call

    def numpy(t, *a, **k):
        r = numpy0(t, *a, **k)
        arrays.append(r.copy())
        return r

    def call(name, ref, *args):
        be = ops._backend()
        n0 = int(be.wl_launch_count())
        rc = call0(name, ref, *args)
        n = min(int(be.wl_launch_count()) - n0, 32)
        last, grid = be.wl_last_kernel().decode(), int(be.wl_last_grid())
        for back in range(n - 1, -1, -1):
            raw = be.wl_kernel_history(back).decode()
            kernels.append((raw.split('K = ')[-1].rstrip(']'), grid if back == 0 and raw == last else None))
        return rc

    torch.Tensor.numpy, ops._call = numpy, call
    try:
        yield
    finally:
        torch.Tensor.numpy, ops._call = numpy0, call0


def _record(*ts):
    """Hand tensors the case computed itself to the cross-schedule comparison."""
    for t in ts:
        t.detach().numpy()


def _args(name, kernel):
    """The template arguments of the first `kernel<...>` in a kernel name."""
    i = name.index(kernel + '<') + len(kernel) + 1
    depth, j = 1, i
    while depth:
        depth += {'<': 1, '>': -1}.get(name[j], 0)
        j += 1
    return [a.strip() for a in name[i:j - 1].split(',')]


def _rows_np2(k):
    a = _args(k, 'WlAfbRows')
    return len(a) == 8 and a[7] == '1'


def _rows_odd(k):
    a = _args(k, 'WlAfbRows')
    return len(a) >= 7 and a[6] == '1'


def _rows_lat(k):
    a = _args(k, 'WlAfbRows')
    return len(a) >= 6 and a[4] == '1' and a[5] == '1'


def _pw2(k):
    a = _args(k, 'WlAfbRows')
    return len(a) < 8 or a[7] == '0'


def _strip_lat(k):
    a = _args(k, 'WlAfbStrip')
    return len(a) >= 4 and a[3] == '1'


def _t(kernel, pred=None, dtype=None, grid=None):
    """A kernel the case must launch: `kernel<...>`, whose arguments satisfy `pred`, with element type `dtype`, launched on a
    grid that satisfies `grid` (a runtime property of the plan, e.g. several planes per workgroup)."""
    def ok(rec):
        k, g = rec
        if not k.startswith(kernel + '<'):
            return False
        a = _args(k, kernel)
        if dtype is not None and a[0] != dtype:
            return False
        if grid is not None and (g is None or not grid(g)):
            return False
        return pred is None or pred(k)
    ok.kernel = kernel
    ok.what = kernel + (' (%s)' % pred.__name__ if pred else '') + (' ' + dtype if dtype else '') + (' (%s)' % grid.__name__ if grid else '')
    return ok


def _below(n):
    def grid(g):
        return g < n
    grid.__name__ = 'grid < %d' % n
    return grid


def _exactly(n):
    def grid(g):
        return g == n
    grid.__name__ = 'grid == %d' % n
    return grid


def _tail(kernel, tail):
    """`kernel<..., tail>`: the trailing template arguments."""
    def pred(k):
        return k.rstrip().endswith(tail) and k.startswith(kernel + '<')
    pred.__name__ = '...' + tail
    return _t(kernel, pred)


def _with(kernel, i, v):
    def pred(k):
        return _args(k, kernel)[i] == v
    pred.__name__ = 'arg%d=%s' % (i, v)
    return _t(kernel, pred)


def _above(n):
    def grid(g):
        return g > n
    grid.__name__ = 'grid > %d' % n
    return grid


def _dwt_fwd_inv(wave, mode, shape, J, cus=2):
    """DWTForward + DWTInverse against the oracle (float32)."""
    from oracle import wavelet_oracle as wo
    rng = np.random.RandomState(sum(shape) + J)
    x = rng.randn(*shape)
    xfm, ifm = pw.DWTForward(J=J, wave=wave, mode=mode), pw.DWTInverse(wave=wave, mode=mode)
    f = [b.double().numpy().ravel() for b in (xfm.h0_col, xfm.h1_col, xfm.h0_row, xfm.h1_row)]
    g = [b.double().numpy().ravel() for b in (ifm.g0_col, ifm.g1_col, ifm.g0_row, ifm.g1_row)]
    oyl, oyh = wo.dwt_forward(x, J, f[0], f[1], f[2], f[3], mode)
    with emu_backend.chip_of(cus):
        yl, yh = xfm(torch.tensor(x, dtype=torch.float32))
        rec = ifm((yl, yh))
    orec = wo.dwt_inverse(yl.double().numpy(), [t.double().numpy() for t in yh], g[0], g[1], g[2], g[3], mode)
    pairs = [(yl, oyl)] + list(zip(yh, oyh)) + [(rec, orec)]
    e = max(float(np.abs(a.double().numpy() - b).max() / max(np.abs(b).max(), 1e-30)) for a, b in pairs)
    assert e < 1e-5, (wave, mode, shape, J, e)


def _dtcwt_fwd_inv(shape, biort, qshift, J, stream=True, grad=False):
    """DTCWTForward + DTCWTInverse (on the oracle's coefficients) against the oracle, float32; the streaming kernels forced;
    with `grad`, the forward's gradient (the fused inverse run with the forward taps) against the per-level tile kernels' backward."""
    from oracle import wavelet_oracle as wo
    from pytorch_wavelets_amd import filters as F
    rng = np.random.RandomState(sum(shape) + J)
    x = rng.randn(*shape)
    hb, gb = F.dtcwt_forward_taps(biort, qshift), F.dtcwt_inverse_taps(biort, qshift)
    oyl, oyh = wo.dtcwt_forward(x, J, *hb)
    want = wo.dtcwt_inverse(oyl, oyh, *gb)
    prev = ops.STREAM_FORCE
    ops.STREAM_FORCE = stream
    try:
        xfm = pw.DTCWTForward(biort=biort, qshift=qshift, J=J)
        ifm = pw.DTCWTInverse(biort=biort, qshift=qshift)
        xt = torch.tensor(x, dtype=torch.float32, requires_grad=grad)
        yl, yh = xfm(xt)
        rec = ifm((torch.tensor(oyl, dtype=torch.float32), [torch.tensor(v, dtype=torch.float32) for v in oyh]))
        if grad:
            dx, = torch.autograd.grad(yl.sum() + sum(h.sum() for h in yh), xt)
            h = emu_backend.handle()
            h.wl_set_option(b'no_stream', 1)   # the per-level tile kernels' backward (pinned to the reference's dx by the goldens)
            try:
                xb = torch.tensor(x, dtype=torch.float32, requires_grad=True)
                ylb, yhb = xfm(xb)
                dxb, = torch.autograd.grad(ylb.sum() + sum(h.sum() for h in yhb), xb)
            finally:
                h.wl_set_option(b'no_stream', 0)
    finally:
        ops.STREAM_FORCE = prev
    for a, b in [(yl, oyl)] + list(zip(yh, oyh)) + [(rec, want)]:
        assert a.shape == b.shape and float(np.abs(a.detach().double().numpy() - b).max()) <= 1e-5 * float(np.abs(b).max()), (shape, J)
    if grad:   # (d/dx of the sum of all coefficients)
        assert dx.shape == xt.shape and _rel(dx, dxb.double().numpy()) <= 3e-6


def _dt_level2(qshift, shape=(2, 1, 64, 256)):
    """The streaming level-2 forward (WlDtFwd12Strip, MODE 4) and inverse (WlDtInv2Strip) on their own, against the oracle's
    fwd_j2plus / inv_j2plus in float64."""
    from oracle import wavelet_oracle as wo
    from pytorch_wavelets_amd import filters as F
    rng = np.random.RandomState(13)
    x = rng.randn(*shape)
    h0o, h1o, h0a, h0b, h1a, h1b = F.dtcwt_forward_taps('near_sym_a', qshift)
    g0o, g1o, g0a, g0b, g1a, g1b = F.dtcwt_inverse_taps('near_sym_a', qshift)
    xfm, ifm = pw.DTCWTForward(J=2, qshift=qshift), pw.DTCWTInverse(qshift=qshift)
    oll, ohi = wo.fwd_j2plus(x, h0a, h1a, h0b, h1b)
    ll, hi = ops.dtcwt_fwd2(torch.tensor(x, dtype=torch.float32), xfm.h0a, xfm.h0b, xfm.h1a, xfm.h1b)
    for got, want in ((ll, oll), (hi, ohi)):
        assert got.shape == want.shape and _rel(got, want) <= 1e-5, (qshift, got.shape, want.shape)
    yl, yh = rng.randn(*oll.shape), rng.randn(*ohi.shape)
    rec = ops.dtcwt_inv2(torch.tensor(yl, dtype=torch.float32), torch.tensor(yh, dtype=torch.float32), ifm.g0a, ifm.g0b, ifm.g1a, ifm.g1b)
    want = wo.inv_j2plus(yl, yh, g0a, g1a, g0b, g1b)
    assert rec.shape == want.shape and _rel(rec, want) <= 1e-5, qshift


def _rel(t, want):
    """max |t - want| / max |want|; records t for the cross-schedule comparison."""
    return float(np.abs(t.detach().numpy().astype(np.float64) - want).max() / max(float(np.abs(want).max()), 1e-30))


def _scatj2(shape=(2, 2, 64, 256)):
    """ScatLayerj2() inference: the in-place launches (wl_scat_fwd_level1_into; the ScatLayerj2 epilogue = WlDtFwd12Strip MODE 5,
    wl_scat_fwd_level2_into; four 128-column planes per workgroup in the second-order layer) against the oracle's ScatLayerj2."""
    from oracle import wavelet_oracle as wo
    from pytorch_wavelets_amd import filters as F
    rng = np.random.RandomState(19)
    x = rng.randn(*shape)
    with torch.no_grad():
        z = pw.ScatLayerj2()(torch.tensor(x, dtype=torch.float32))
    want = wo.scat_layer_j2_forward(x, *F.dtcwt_forward_taps('near_sym_a', 'qshift_a'))
    assert z.shape == want.shape and _rel(z, want) <= 1e-5


def _scatj2_rot(shape=(2, 1, 64, 80)):
    """ScatLayerj2(near_sym_b_bp, qshift_b_bp) training step: the helper's checks against the chain and the oracle, and the
    layer's output and input gradient recorded for the cross-schedule comparison."""
    ks = NB.check_scatj2_rot('cpu', shape, torch.float32)
    rng = np.random.RandomState(23)
    m = pw.ScatLayerj2(biort='near_sym_b_bp', qshift='qshift_b_bp')
    x = torch.tensor(rng.randn(*shape), dtype=torch.float32, requires_grad=True)
    z = m(x)
    dx, = torch.autograd.grad(z, x, torch.tensor(rng.randn(*z.shape), dtype=torch.float32))
    _record(z, dx)
    return ks


def _nlev(n):
    def pred(k):
        return k.rstrip().endswith(', %d>' % n)
    pred.__name__ = 'NLEV=%d' % n
    return pred


def _wpt(wave, mode, shape, J, two):
    """WPT2DForward / WPT2DInverse and both backwards (each runs the other direction's kernel) against the oracle; two: two
    levels per launch where the kernels take them."""
    with WP.fused(two):
        WP.check_forward('cpu', shape, wave, J, mode)
        WP.check_inverse('cpu', shape, wave, mode, J=J)
        WP.check_gradients('cpu', shape, wave, mode, J=J)


def _wpt_f16():
    with WP.fused(False):
        WP.check_low_precision('cpu', F16, 'symmetric')


def _dt1d(n, J, biort, qshift, chunks, shape):
    """DTCWT1DForward, DTCWT1DInverse and dx with cotangents on every output (tests/_dtcwt1d_cases.run_both), chunk lengths
    forced (analysis pairs, synthesis samples; 0: the engine's), against the oracle."""
    x, yl, yh, rec, dx, cots = D1.run_both('cpu', n, J, biort, qshift, F32, chunks, shape=shape)
    t = D1.taps(biort, qshift, f32=True)
    rl, rh = D1.fwd_ref(D1.npy(x), J, t)
    D1.close(yl, rl, F32, 'yl')
    for j in range(J):
        D1.close(yh[j], rh[j], F32, 'yh[%d]' % j)
    D1.close(rec, D1.inv_ref(D1.npy(yl), [D1.npy(h) for h in yh], D1.taps(biort, qshift, syn=True, f32=True)), F32, 'rec')
    D1.close(dx, D1.fwd_grad_ref(D1.npy(cots[0]), [D1.npy(c) for c in cots[1:]], n, t), F32, 'dx')


def _swt_inverse(shape=(1, 2, 20, 24)):
    """SWTInverse (one WlSwtInvLevel launch per level), the transposed level against the oracle's transpose, and the backward of
    SWTForward (J = 2) - at the smallest periodic shape of tests/test_swt_inverse_emu.py."""
    _, rec = SI.check_roundtrip('cpu', 'db2', 2, shape, torch.float64)
    SI.check_adjoint('cpu', 'db2', 'db2', 'periodic', 1, shape, torch.float64)
    rng = np.random.RandomState(8)
    xfm, _ = SI.swt_modules('cpu', 'db2', 'db2', 2)
    x = torch.tensor(rng.randn(*shape), requires_grad=True)
    ys = xfm(x)
    cots = [torch.tensor(rng.randn(*y.shape)) for y in ys]
    c0 = pw.launch_count()
    dx, = torch.autograd.grad(ys, x, cots)
    ks = pw.kernels_since(c0)
    assert len(ks) == 2 and all(k.startswith('WlSwtInvLevel') for k in ks), ks
    lhs, rhs = sum(float((y.detach() * c).sum()) for y, c in zip(ys, cots)), float((x.detach() * dx).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(1.0, abs(lhs)), (lhs, rhs)                # <A x, y> = <x, A^T y>
    _record(rec, dx)


def _dwt_per_level(wave, mode, shape, J, generic=False):
    """DWTForward + DWTInverse one launch per level, planes kept off the several-planes-per-workgroup kernels: the tile kernels
    WlAfbTile / WlSfbTile, or - generic - the runtime-tap ones."""
    import _opts
    with B._setattrs(dwl, FUSED_LEVELS=False), B.no_small():
        _opts.set_generic(int(generic))
        try:
            _dwt_fwd_inv(wave, mode, shape, J)
        finally:
            _opts.set_generic(0)


def _dtcwt_generic(shape):
    import _opts
    _opts.set_generic(1)
    try:
        _dtcwt_fwd_inv(shape, 'near_sym_a', 'qshift_a', 2, stream=False)
    finally:
        _opts.set_generic(0)


F32 = torch.float32
F16 = torch.float16
CASES = [
    # ---- WlAfbRows: the fused multi-level analysis
    ('rows_pow2_reflect_J3', lambda: PK.check_padded_fused('cpu', 'db3', 'reflect', 44, 261, 3), [_t('WlAfbRows', _pw2)]),
    ('rows_odd_per', lambda: PC.check_fused_periodization('cpu', 'db2', 96, 128, 3, F32, 2), [_t('WlAfbRows', _rows_odd)]),
    ('rows_np2_sym', lambda: LC.check_rows_exact_rings('cpu', 'db8', 'symmetric'), [_t('WlAfbRows', _rows_np2)]),
    ('rows_np2_per_db9', lambda: LC.check_rows_exact_rings('cpu', 'db9', 'periodization', shape=(1, 1, 256, 512)), [_t('WlAfbRows', _rows_np2)]),
    ('rows_np2_per_coif3', lambda: LC.check_rows_exact_rings('cpu', 'coif3', 'periodization', shape=(1, 1, 200, 512)), [_t('WlAfbRows', _rows_np2)]),
    ('rows_np2_cut', lambda: LC.check_rows_exact_rings('cpu', 'db7', 'reflect', shape=(1, 1, 264, 512), planes_cut=True), [_t('WlAfbRows', _rows_np2)]),
    ('rows_lattice_J2', lambda: LC.check_rows_lattice_vs_oracle('cpu', 'sym8', 'zero', 2, shape=(1, 2, 64, 256)), [_t('WlAfbRows', _rows_lat)]),
    ('rows_lattice_J1', lambda: LC.check_rows_lattice_vs_oracle('cpu', 'db6', 'zero', 1, shape=(1, 2, 64, 256)), [_t('WlAfbRows', _rows_lat)]),
    # 6 planes on fewer workgroups than planes: several planes per workgroup (grid = units + cut halves, units = planes / pp)
    ('rows_planes_per_wg', lambda: PK.check_padded_fused('cpu', 'haar', 'zero', 36, 130, 2), [_t('WlAfbRows', grid=_below(6))]),
    ('rows_per_planes_cut', lambda: PC.check_fused_periodization('cpu', 'db4', 128, 256, 3, F32, 2, planes=(1, 1)), [_t('WlAfbRows')]),
    # the round-6 triage case (random pyramid seed 28): bior2.2, zero mode, 11 planes of 64 x 172, J = 3, 8-CU chip
    ('rows_pyramid_bior22', lambda: _dwt_fwd_inv('bior2.2', 'zero', (11, 1, 64, 172), 3, cus=8), [_with('WlAfbRows', 1, '6'), _with('WlSfbRows', 1, '6')]),
    # ---- WlSfbRows: the fused multi-level synthesis
    ('irows_per', lambda: PC.check_fused_periodization_inverse('cpu', 'db4', 128, 256, 3, F32, 1), [_t('WlSfbRows')]),
    ('irows_lattice', lambda: LC.check_irows_lattice_vs_oracle('cpu', 'db8', 'symmetric', 2, shape=(1, 2, 64, 256)), [_t('WlSfbRows', LC._is_lattice_irows)]),
    ('dwt_dx_per', lambda: PC.check_periodization_gradient('cpu'), [_t('WlAfbRows'), _t('WlSfbRows')]),
    # ---- WlAfbStrip / WlSfbStrip
    ('strip_plain', lambda: PK.check_packed('cpu', 'db4', 'symmetric', F32, 32, 1100, 2, packed=False), [_t('WlAfbStrip'), _t('WlSfbStrip')]),
    ('strip_packed_f16', lambda: PK.check_packed('cpu', 'sym7', 'symmetric', F16, 30, 200, 7), [_t('WlAfbStrip', dtype='_Float16')]),
    ('strip_lattice', lambda: LC.check_lattice_vs_oracle('cpu', 'db8', 'periodization', shape=(1, 2, 40, 288)), [_t('WlAfbStrip', _strip_lat)]),
    ('strip_lattice_inverse', lambda: LC.check_lattice_inverse_vs_oracle('cpu', 'db6', 'symmetric', shape=(1, 2, 40, 288)), [_t('WlSfbStrip', LC._is_lattice_syn)]),
    # ---- WlDtFwd12Strip and the DTCWT inverses
    ('dt_fused_J2', lambda: _dtcwt_fwd_inv((2, 1, 64, 256), 'near_sym_a', 'qshift_a', 2, grad=True), [_t('WlDtFwd12Strip'), _t('WlDtInv21Strip')]),
    ('dt_level2_q18', lambda: _dt_level2('qshift_d'), [_with('WlDtInv2Strip', 1, '18')]),
    ('dt_level2_q14', lambda: _dt_level2('qshift_b'), [_with('WlDtFwd12Strip', 3, '14'), _with('WlDtInv2Strip', 1, '14')]),
    ('dt_level2_q10', lambda: _dt_level2('qshift_a'), [_with('WlDtFwd12Strip', 3, '10'), _with('WlDtInv2Strip', 1, '10')]),
    ('dt_near_sym_b_J1', lambda: NB.check_dtcwt_near_sym_b('cpu', (1, 2, 40, 256), F32, J=1), [_t('WlDtFwd12Strip'), _t('WlDtInv1Strip')]),
    ('scat_backward', lambda: D.check_scat_backward_streaming('cpu', [((1, 2, 64, 256), F32)]), [_t('WlDtFwd12Strip'), _t('WlDtInv1Strip')]),
    ('scat_near_sym_b', lambda: NB.check_scat_near_sym_b('cpu', (1, 2, 44, 256), F32), [_t('WlDtFwd12Strip'), _t('WlDtInv1Strip')]),
    ('scat_rot_lean', lambda: NB.check_scat_rot_lean('cpu', (1, 2, 44, 256), F32), [_t('WlDtFwd12Strip')]),
    ('scat_rot_training', lambda: NB.check_scat_rot_training('cpu', (1, 2, 44, 256), F32), [_t('WlDtFwd12Strip'), _t('WlDtInv1Strip')]),
    # the band-pass second scale: MODE 1 (plain pair) and MODE 3 (training, saved quotients) of the 13 / 19-tap kernel, its backward
    ('scatj2_rot', _scatj2_rot, [_tail('WlDtFwd12Strip', '13, 19, 10, 1, 4, 2>'), _tail('WlDtFwd12Strip', '13, 19, 10, 3, 4, 2>'),
                                 _tail('WlDtInv1Strip', '13, 19, 1, 2>')]),
    ('scatj2_epilogue', _scatj2, [_tail('WlDtFwd12Strip', '10, 5, 2>'), _tail('WlDtFwd12Strip', '10, 1, 4, 4>')]),
    # ---- the other kernels
    ('dwt1d_fused', lambda: E.check_dwt1d_fused('cpu', cases=[('db4', 'symmetric', 3, (2, 2, 3000), F32), ('db2', 'periodization', 2, (1, 2, 1000), F32)]),
     [_t('WlDwt1dFused'), _t('WlIdwt1dFused')]),
    ('small_planes', lambda: _dwt_fwd_inv('db2', 'symmetric', (3, 2, 20, 24), 2), [_t('WlAfbSmall'), _t('WlSfbSmall')]),
    # the LDS reuse between a workgroup's consecutive units: 14 rows of three chunks on the 2-CU chip = two consecutive chunks per
    # workgroup (28 workgroups for 42 chunks: the commit of chunk c + 1 into buffer 0 follows the levels of chunk c); 36 planes =
    # nine groups of four on the eight resident workgroups (workgroup 0 walks over groups 0 and 8)
    ('dwt1d_chunk_walk', lambda: E.check_dwt1d_fused('cpu', cases=[('db4', 'symmetric', 1, (14, 1, 8400), F32)]),
     [_t('WlDwt1dFused', grid=_exactly(28)), _t('WlIdwt1dFused')]),
    ('small_planes_group_walk', lambda: _dwt_fwd_inv('db2', 'symmetric', (9, 4, 32, 32), 2), [_t('WlAfbSmall', grid=_exactly(8)), _t('WlSfbSmall')]),
    ('dt_small', lambda: _dtcwt_fwd_inv((6, 3, 32, 32), 'near_sym_a', 'qshift_a', 1, stream=False), [_t('WlDtFwd1Small')]),
    ('rot_level1', lambda: [E.check_rot(n, 'cpu', F32, 1e-5) for n in E.ROT_CASES[:1]], [_t('WlDtFwd1Rot')]),
    ('swt', lambda: [E.check_swt(n, 'cpu', F32, 1e-5) for n in E.SWT_CASES[:1]], [_t('WlSwtLevel')]),
    ('swt_inverse', _swt_inverse, [_t('WlSwtInvLevel')]),
    # ---- WlWptAfb / WlWptSfb: two levels per launch (five barrier phases, the staging words reused for the level-2 rows; 12 taps:
    # the largest aliased region), one level per launch on the wide walk and on the plane-run walk (8 planes on 2 workgroups)
    ('wpt_two_level_db4', lambda: _wpt('db4', 'periodization', (1, 2, 40, 72), 2, True), [_t('WlWptAfb', _nlev(2)), _t('WlWptSfb', _nlev(2))]),
    ('wpt_two_level_db6', lambda: _wpt('db6', 'periodization', (1, 2, 40, 72), 2, True), [_t('WlWptAfb', _nlev(2)), _t('WlWptSfb', _nlev(2))]),
    ('wpt_wide', lambda: _wpt('db4', 'symmetric', (1, 2, 37, 61), 2, False), [_t('WlWptAfb', _nlev(1)), _t('WlWptSfb', _nlev(1))]),
    ('wpt_plane_run', lambda: _wpt('db2', 'symmetric', (2, 4, 8, 8), 1, False),
     [_t('WlWptAfb', _nlev(1), grid=_below(8)), _t('WlWptSfb', _nlev(1), grid=_below(8))]),
    ('wpt_f16', _wpt_f16, [_t('WlWptAfb', _nlev(1), dtype='_Float16'), _t('WlWptSfb', _nlev(1), dtype='_Float16')]),
    # ---- WlDt1dFwd / WlDt1dInv: a geometry block written by lane 0, up to four level buffers, `put` into up to three cells
    ('dt1d_chunks_J3', lambda: _dt1d(301, 3, 'near_sym_a', 'qshift_a', (5, 44), (2, 1, 301)), [_with('WlDt1dFwd', 1, '10'), _with('WlDt1dInv', 1, '10')]),
    ('dt1d_J4_q14', lambda: _dt1d(301, 4, 'near_sym_b', 'qshift_b', (5, 44), (2, 1, 301)), [_with('WlDt1dFwd', 1, '14'), _with('WlDt1dInv', 1, '14')]),
    ('dt1d_two_groups_J6', lambda: _dt1d(512, 6, 'near_sym_a', 'qshift_a', (0, 0), (1, 2, 512)), [_t('WlDt1dFwd'), _t('WlDt1dInv')]),
    ('dt1d_none_high', lambda: D1.check_none_highs('cpu', 1), [_t('WlDt1dFwd'), _t('WlDt1dInv')]),
    # ---- the per-level kernels: the tile kernels and the runtime-tap (generic) ones, on the smallest planes that reach them
    ('dwt_tile', lambda: _dwt_per_level('db4', 'symmetric', (1, 2, 20, 36), 2), [_t('WlAfbTile'), _t('WlSfbTile')]),
    ('dwt_generic', lambda: _dwt_per_level('db3', 'reflect', (1, 2, 20, 36), 2, generic=True), [_t('WlAfb2dTile'), _t('WlSfb2dTile')]),
    ('dt_tile', lambda: _dtcwt_fwd_inv((1, 2, 40, 56), 'near_sym_a', 'qshift_a', 2, stream=False),
     [_t('WlDtFwd1Tile'), _t('WlDtFwd2Tile'), _t('WlDtInv1Tile'), _t('WlDtInv2Tile')]),
    ('dt_generic', lambda: _dtcwt_generic((1, 2, 24, 40)), [_t('WlDtFwd1'), _t('WlDtFwd2'), _t('WlDtInv1'), _t('WlDtInv2')]),
    ('dt_level1_strip', lambda: _dtcwt_fwd_inv((1, 2, 24, 256), 'near_sym_a', 'qshift_a', 1), [_t('WlDtFwd1Strip'), _t('WlDtInv1Strip')]),
]


def _run(fn, sched):
    arrays, kernels = [], []
    order, dma, seed = sched
    with emu_backend.emulated(), emu_backend.schedule(order, dma, seed), _recording(arrays, kernels):
        torch.manual_seed(0)
        fn()
    return arrays, kernels


@pytest.mark.parametrize('name,fn,want', CASES, ids=[c[0] for c in CASES])
def test_kernel_family_under_every_schedule(name, fn, want):
    ref = None
    for sched in SCHEDULES:
        arrays, kernels = _run(fn, sched)
        for w in want:
            assert any(w(k) for k in kernels), (name, sched, w.what, kernels)
        assert arrays, (name, 'no output was recorded: nothing to compare across the schedules')
        if ref is None:
            ref = arrays
            continue
        assert len(arrays) == len(ref), (name, sched)
        for i, (a, b) in enumerate(zip(arrays, ref)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, sched, i, float(np.nanmax(np.abs(a.astype(np.float64) - b))))


def test_ring_slot_is_a_floor_mod():
    """The slot of a row in an exactly-sized (NP2) LL ring: r mod rows (a floor mod) for every row number the plan can produce -
    negative ones (the unfolded rows of periodized levels) included, and far enough up that the multiply-high's 'one less'
    quotient occurs."""
    slot = emu_backend.ring_slot_fn()
    assert slot(-1, 3) == 2 and slot(0, 3) == 0
    rs = range(-64, 70001)
    for rows in range(2, 65):
        bad = [r for r in rs if slot(r, rows) != r % rows]
        assert not bad, (rows, bad[:5], [slot(r, rows) for r in bad[:5]])


# Barrier functors that need no case here, each with the reason.
EXEMPT = {}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pytorch_wavelets_amd', 'csrc')


def barrier_functors(csrc=CSRC):
    """Every kernel functor of the engine whose body has a barrier - a plain text scan of the kernel sources.  A file is cut into
    regions at every `struct Wl...` and every `wl_..._body(` function defined at the start of a line; a body function whose region
    calls ctx.sync() is a barrier body; a struct is a barrier functor when its region calls ctx.sync() or a barrier body - the
    WL_FUNCTOR(name, args, body) lines of wl_api.inc included.  -> {functor: file}"""
    head = re.compile(r'^(?:struct (Wl\w+)[^;\n]*$|(?:WL_DEV|WL_HD|static|inline)[^;\n]*?\b(wl_\w+_body)\()', re.M)
    regions = []
    for path in sorted(glob.glob(os.path.join(csrc, '*.h')) + glob.glob(os.path.join(csrc, '*.inc'))):
        text = open(path).read()
        marks = list(head.finditer(text))
        for m, nxt in zip(marks, marks[1:] + [None]):
            regions.append((m.group(1), m.group(2), text[m.end():nxt.start() if nxt else len(text)], os.path.basename(path)))
        for m in re.finditer(r'^WL_FUNCTOR\((Wl\w+), \w+, (wl_\w+)\)', text, re.M):
            regions.append((m.group(1), None, m.group(2) + '(', os.path.basename(path)))
    bodies = set(fn for _, fn, body, _ in regions if fn and 'ctx.sync()' in body)
    return dict((st, f) for st, _, body, f in regions
                if st and not st.endswith('Args') and ('ctx.sync()' in body or any(b + '<' in body or b + '(' in body for b in bodies)))


def test_every_barrier_kernel_has_a_case():
    """The next kernel with a barrier cannot slip past this suite: every functor of csrc/ whose body calls ctx.sync() is named
    by the wanted-kernel list of some case above, or stands in EXEMPT with a reason."""
    found = barrier_functors()
    # the scan itself: one known functor per way a barrier reaches a functor (its own body, a specialisation, a body function
    # behind a plain struct, one behind WL_FUNCTOR), and nothing that is no kernel
    for name in ('WlAfbRows', 'WlWptAfb', 'WlWptSfb', 'WlDt1dFwd', 'WlDt1dInv', 'WlSwtInvLevel', 'WlAfb2dTile', 'WlDtInv2', 'WlDtFwd1Tile'):
        assert name in found, (name, sorted(found))
    assert len(found) >= 33 and not any(n in found for n in ('WlAfbDepth', 'WlSfbDepth', 'WlCorr1d', 'WlCtx')), sorted(found)
    named = set(w.kernel for _, _, want in CASES for w in want)
    missing = sorted(k for k in found if k not in named and k not in EXEMPT)
    assert not missing, 'barrier kernels without a schedule case: %s' % ', '.join('%s (%s)' % (k, found[k]) for k in missing)
    stale = sorted(k for k in EXEMPT if k not in found or k in named)
    assert not stale, ('exempt, but covered or gone', stale)
