"""CPU tests: guard bands around every output (tests/_guard_cases.py).  First the harness itself, on plain torch tensors - no
kernel runs, and what these tests write stays inside the parent allocation.  Then the existing shared checks of every kernel
family on the host emulation of the kernels, run inside ``guarded('cpu')``: they still compare with their float64 oracles and
still assert which kernels ran, and on exit no store may have landed outside an output and no output element may be left unwritten."""
import ctypes
import os

import pytest
import torch

import _bf16_cases as B
import _dtcwt1d_cases as D1
import _dtroute_cases as DRC
import _dwt3d_cases as V3
import _guard_cases as G
import _route_cases as RC
import _scat1d_cases as SC
import _swt1d_cases as S1
import _view_cases as V
import _wpt1d_cases as P1
import _wpt2d_cases as P2
import emu_backend
import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import ops

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
IDS = dict(ids=lambda v: v if isinstance(v, str) else str(v).replace('torch.', ''))


# ---- the harness itself ------------------------------------------------------------------------------------------------------
def _package_like(src):
    """A function compiled as if its file lay under pytorch_wavelets_amd/ (no file is written): what the guard takes for package
    code."""
    scope = {'torch': torch}
    exec(compile(src, os.path.join(os.path.dirname(os.path.abspath(pw.__file__)), '_guard_probe.py'), 'exec'), scope)
    return scope['alloc']


ALLOC = _package_like('def alloc(*a, **kw):\n    return torch.empty(*a, **kw)\n')
ALLOC_LIKE = _package_like('def alloc(*a, **kw):\n    return torch.empty_like(*a, **kw)\n')


@pytest.mark.parametrize('dtype', [F16, BF16, F32, F64], **IDS)
@pytest.mark.parametrize('where', ['behind', 'in front', 'last guard word', 'first guard word'])
def test_a_write_outside_the_body_is_reported(where, dtype):
    with pytest.raises(AssertionError) as e:
        with G.guarded('cpu') as g:
            t = torch.empty(3, 5, dtype=dtype)
            t.zero_()
            blk = g.blocks[-1]
            p = blk.parent()
            assert p.numel() == 2 * blk.g + 15 and blk.g * t.element_size() == 4096
            at = {'behind': blk.g + 15, 'in front': blk.g - 1, 'last guard word': p.numel() - 1, 'first guard word': 0}[where]
            p[at] = 1.0
    side, dist = {'behind': ('BACK', 1), 'in front': ('FRONT', 1), 'last guard word': ('BACK', blk.g), 'first guard word': ('FRONT', blk.g)}[where]
    msg = str(e.value)
    assert side + ' guard of (3, 5) ' + str(dtype).replace('torch.', '') in msg and '[%d] element(s)' % dist in msg, msg
    assert 'launches since entry' in msg


def test_an_untouched_body_from_package_code_is_reported_a_written_one_is_not():
    with G.guarded('cpu'):
        ALLOC(4, 7).fill_(0.5)
        ALLOC_LIKE(torch.zeros(2, 3, dtype=F16)).fill_(2.0)
        torch.empty(4, 7)                                   # (a test's own scratch may stay unwritten)
    for skip in (0, 13, 27):
        with pytest.raises(AssertionError, match=r'1 element\(s\) of \(4, 7\) float32 .* never written, flat indices \[%d\]' % skip):
            with G.guarded('cpu'):
                t = ALLOC(4, 7)
                t.view(-1)[:skip] = 1.0
                t.view(-1)[skip + 1:] = 1.0
    with pytest.raises(AssertionError, match=r'6 element\(s\) of \(2, 3\) float16'):
        with G.guarded('cpu'):
            ALLOC_LIKE(torch.zeros(2, 3, dtype=F16))


def test_the_allow_list_is_keyed_by_the_allocating_function():
    assert all(len(e) == 2 and all(isinstance(v, str) and v for v in e) for e in G.UNWRITTEN_OK)
    with G.guarded('cpu') as g:
        ops._new_tap_scratch(torch.device('cpu'))
        assert g.blocks[-1].package and g.blocks[-1].allowed


def test_outputs_of_a_declined_launch_may_stay_wholly_unwritten(monkeypatch):
    """ops._declined: the wrapper drops the outputs it allocated for a launch the launcher refused.  The blocks whose addresses
    the call carried - plain or in a pointer array - may stay untouched; a partly written one, or one of a launch that ran, may not."""
    real = ops._declined
    monkeypatch.setattr(ops, '_declined', lambda key, name, ref, *a: True)
    with G.guarded('cpu') as g:
        t, u, v = ALLOC(4, 7), ALLOC(2, 3), ALLOC(5).fill_(1.0)
        assert ops._declined(None, 'wl_x', t, t.data_ptr(), 3, (ctypes.c_void_p * 2)(u.data_ptr(), None), None)
        assert [b.declined for b in g.blocks] == [True, True, False]
    assert ops._declined is not real
    with pytest.raises(AssertionError, match=r'27 element\(s\) of \(4, 7\)'):
        with G.guarded('cpu'):
            t = ALLOC(4, 7)
            t.view(-1)[0] = 1.0
            ops._declined(None, 'wl_x', t, t.data_ptr())
    monkeypatch.setattr(ops, '_declined', lambda key, name, ref, *a: False)
    with pytest.raises(AssertionError, match=r'28 element\(s\) of \(4, 7\)'):
        with G.guarded('cpu'):
            t = ALLOC(4, 7)
            assert not ops._declined(None, 'wl_x', t, t.data_ptr())
    monkeypatch.undo()
    assert ops._declined is real


@pytest.mark.parametrize('dtype', [F16, BF16, F32, F64], **IDS)
def test_returned_tensors_are_what_was_asked_for(dtype):
    with G.guarded('cpu') as g:
        for shape in ((5,), (3, 5, 7), (1, 1, 1)):
            t = torch.empty(shape, dtype=dtype, device='cpu')
            u = torch.empty(*shape, dtype=dtype)
            w = torch.empty_like(t)
            for v in (t, u, w):
                assert v.is_contiguous() and v.data_ptr() % 256 == 0 and tuple(v.shape) == shape and v.dtype == dtype
                assert v.device.type == 'cpu' and not v.requires_grad and v._base is None
                v.fill_(1.0)
            g.assert_guarded(t, [u, (w, None)], t[1:], t.view(-1)[::2])
        assert torch.empty(3, dtype=dtype, requires_grad=True).requires_grad
        assert len(g.blocks) == 10


def test_requests_the_guard_passes_through():
    with G.guarded('cpu') as g:
        assert torch.empty(4, dtype=torch.int32).dtype == torch.int32 and torch.empty(4, dtype=torch.bool).dtype == torch.bool
        out = torch.zeros(6)
        assert torch.empty(6, out=out) is out
        cl = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last) and not cl.is_contiguous()
        src = torch.zeros(4, 6)[:, ::2]
        assert tuple(torch.empty_like(src).shape) == (4, 3)
        assert torch.empty(0, 3).numel() == 0 and torch.empty_like(torch.zeros(2, dtype=torch.int64)).dtype == torch.int64
        assert not g.blocks


def test_assert_guarded_sees_an_output_that_went_round_the_guard():
    outside = torch.zeros(3)
    with G.guarded('cpu') as g:
        inside = torch.empty(3).zero_()
        x = torch.zeros(2, 4)
        G.assert_guarded(inside, x[1], torch.zeros(0), inputs=[x])          # an alias of an input and a zero-size tensor are exempt
        for t in (outside, torch.zeros(3), x[1]):
            with pytest.raises(AssertionError, match='went round the guard'):
                g.assert_guarded(inside, t)
    with pytest.raises(AssertionError, match='outside guarded'):
        G.assert_guarded(outside)


def test_the_allocators_are_restored():
    e0, l0, d0 = torch.empty, torch.empty_like, ops._declined
    with G.guarded('cpu'):
        assert torch.empty is not e0 and torch.empty_like is not l0 and ops._declined is not d0
    assert torch.empty is e0 and torch.empty_like is l0 and ops._declined is d0
    with pytest.raises(KeyError):
        with G.guarded('cpu'):
            raise KeyError('x')
    assert torch.empty is e0 and torch.empty_like is l0 and ops._declined is d0
    with pytest.raises(AssertionError, match='BACK guard'):            # a failed guard check restores them too
        with G.guarded('cpu') as g:
            torch.empty(2)
            g.blocks[-1].parent()[-1] = 0.0
    assert torch.empty is e0 and torch.empty_like is l0
    with pytest.raises(AssertionError, match=r'FRONT guard[\s\S]*the guarded code itself raised KeyError'):   # the leak is reported first
        with G.guarded('cpu') as g:
            torch.empty(2)
            g.blocks[-1].parent()[0] = 0.0
            raise KeyError('x')
    assert torch.empty is e0 and torch.empty_like is l0 and ops._declined is d0


# ---- every kernel family under the guard ---------------------------------------------------------------------------------------
def _guarded(fn, *a, **kw):
    with emu_backend.emulated(), G.guarded('cpu'):
        return fn('cpu', *a, **kw)


@pytest.mark.parametrize('family', sorted(G.DIRECT))
def test_module_outputs_lie_in_guarded_blocks(family):
    """Forward, inverse and one autograd.grad of each newer family's modules: everything returned is a block of the guard."""
    _guarded(G.DIRECT[family])


# ScatLayer1D
@pytest.mark.parametrize('biort', sorted(SC.BIORTS))
def test_scat1d_grid(biort):
    _guarded(SC.check_grid, biort)


@pytest.mark.parametrize('dtype', [F16, BF16], **IDS)
@pytest.mark.parametrize('biort', ['near_sym_a', 'near_sym_b'])
def test_scat1d_two_byte(biort, dtype):
    _guarded(SC.check_two_byte, biort, dtype)


def test_scat1d_views():
    _guarded(SC.check_views)


# SWT1D
@pytest.mark.parametrize('J', S1.LEVELS)
@pytest.mark.parametrize('wave', S1.WAVES)
def test_swt1d_grid(wave, J):
    _guarded(S1.check_grid, wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16], **IDS)
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_swt1d_two_byte(wave, dtype):
    _guarded(S1.check_two_byte, wave, dtype)


@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', S1.WAVES)
def test_swt1d_origin(wave, J):
    _guarded(S1.check_origin, wave, J)
    if wave == 'db4' and J == 3:
        _guarded(S1.check_origin, wave, J, F16)


# WPT1D
@pytest.mark.parametrize('J', P1.LEVELS)
@pytest.mark.parametrize('wave', P1.WAVES)
def test_wpt1d_grid(wave, J):
    _guarded(P1.check_grid, wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16], **IDS)
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_wpt1d_two_byte(wave, dtype):
    _guarded(P1.check_two_byte, wave, dtype)


@pytest.mark.parametrize('dtype', [F32, F16], **IDS)
@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', P1.WAVES)
def test_wpt1d_origin(wave, J, dtype):
    _guarded(P1.check_origin, wave, J, dtype)


# DTCWT1D
@pytest.mark.parametrize('pair', D1.FUSED_PAIRS, ids='-'.join)
@pytest.mark.parametrize('n', [16, 20, 22, 37])
def test_dtcwt1d_values(n, pair):
    for J in (1, 2, 3, 4):
        _guarded(D1.check_values, n, J, pair[0], pair[1])


@pytest.mark.parametrize('pair', D1.FUSED_PAIRS, ids='-'.join)
def test_dtcwt1d_gradients(pair):
    for n, J in ((22, 3), (37, 4), (20, 2), (16, 1)):
        _guarded(D1.check_gradients, n, J, pair[0], pair[1], F32)
    _guarded(D1.check_gradients, 22, 3, pair[0], pair[1], F64)


@pytest.mark.parametrize('dtype', [F16, BF16], **IDS)
def test_dtcwt1d_two_byte(dtype):
    for b, q in D1.FUSED_PAIRS + (('antonini', 'qshift_d'),):
        _guarded(D1.check_values, 37, 3, b, q, dtype, fused=True)
    _guarded(D1.check_gradients, 22, 3, 'near_sym_a', 'qshift_a', dtype)


@pytest.mark.parametrize('n', [300, 301])
def test_dtcwt1d_seams(n):
    _guarded(D1.check_seams, n)


@pytest.mark.parametrize('drop', [0, 1])
def test_dtcwt1d_none_highs(drop):
    _guarded(D1.check_none_highs, drop)


# DWT3D
@pytest.mark.parametrize('mode', V3.MODES)
def test_dwt3d_forward_inverse_gradients(mode):
    with emu_backend.emulated(), G.guarded('cpu') as g:
        for shape, wave, J in (((2, 3, 10, 12, 16), 'db2', 1), ((2, 1, 7, 9, 11), 'db4', 2)):
            x, yl, yh, _ = V3.check_forward('cpu', shape, wave, J, mode)
            g.assert_guarded(yl, yh, inputs=[x])
        V3.check_inverse('cpu', (2, 1, 7, 9, 11), 'db4', mode, J=2)
        V3.check_inverse('cpu', (1, 2, 7, 9, 11), 'db2', mode, J=2, drop=1)
        V3.check_gradients('cpu', (2, 1, 7, 9, 11), 'db2', mode, J=2)


@pytest.mark.parametrize('dtype', [F32, F16, BF16], **IDS)
def test_dwt3d_vector_and_scalar_bodies(dtype):
    _guarded(V3.check_vec_bodies, dtype)


@pytest.mark.parametrize('dtype', V3.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', V3.GRID_WAVES)
def test_dwt3d_depth_kernels_inner_sizes_64_68_5(wave, dtype):
    _guarded(V3.check_depth_instantiation, wave, dtype)


# WPT2D
@pytest.mark.parametrize('mode', P2.MODES)
@pytest.mark.parametrize('J', [1, 2, 3])
def test_wpt2d_forward(J, mode):
    for shape, wave in (((2, 3, 20, 28), 'db2'), ((1, 2, 37, 141), 'db4'), ((1, 1, 5, 7), 'db4'), ((1, 2, 38, 150), 'db10')):
        _guarded(P2.check_forward, shape, wave, J, mode)


@pytest.mark.parametrize('mode', P2.MODES)
def test_wpt2d_inverse_and_gradients(mode):
    _guarded(P2.check_inverse, (1, 2, 37, 141), 'db4', mode, J=2)
    _guarded(P2.check_inverse, (1, 2, 37, 141), 'db4', mode, J=2, with_size=False)
    _guarded(P2.check_gradients, (2, 1, 9, 13), 'db2', mode, J=2)
    _guarded(P2.check_gradients, (1, 2, 13, 9), 'db4', mode, J=2, dtype=F64)


@pytest.mark.parametrize('wave', ['db1', 'db2', 'db4', 'db6'])
def test_wpt2d_two_level_kernel_seams(wave):
    _guarded(P2.check_wrap_shapes, wave, (1, 2, 72, 200))
    _guarded(P2.check_wrap_shapes, wave, (2, 1, 8, 12), two_level=wave in ('db1', 'db2'))


@pytest.mark.parametrize('dtype', [F16, BF16], **IDS)
def test_wpt2d_two_levels_per_launch_two_byte(dtype):
    _guarded(P2.check_two_level_low_precision, dtype)


@pytest.mark.parametrize('dtype', P2.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', P2.GRID_WAVES)
def test_wpt2d_wide_walk_every_tap_count(wave, dtype):
    _guarded(P2.check_wide_instantiation, wave, dtype)


# 2-D DWT, DTCWT, ScatLayer / ScatLayerj2, SWT 2-D, DWT1D, non-separable: the table of tests/_view_cases.py
@pytest.mark.parametrize('name', [c.name for c in V.CASES])
def test_view_table(name):
    case, outs = V.BY_NAME[name], []
    with emu_backend.emulated(), emu_backend.chip_of(case.cus), G.guarded('cpu') as g:
        V.check(case, 'cpu', outs_to=outs)
        g.assert_guarded(outs)


# (off by default - dwt/lowlevel.py: _PAD_LL -: the per-level path with its inner ll at a cache-line row pitch, the `_ll_pitch` buffers
#  of ops.afb2d whose pad columns nobody writes)
PAD_LL = V.Case('tile-fwd-pad-ll', V.dwt_fwd(2, 'db2', 'symmetric'), (2, 1, 70, 132), F32, V.offset(1), ['WlAfbTile<', ('WlAfbSmall<', 'WlAfbTile<')],
                pin={'_PAD_LL': True, 'FUSED_LEVELS': False})


def test_view_table_padded_ll_pitch():
    outs = []
    with emu_backend.emulated(), G.guarded('cpu') as g:
        V.check(PAD_LL, 'cpu', outs_to=outs)
        g.assert_guarded(outs)
        assert any(b.allowed and b.site.endswith(' afb2d()') for b in g.blocks), [b.site for b in g.blocks]


@pytest.mark.parametrize('name', V.GRAD_CASES)
def test_view_table_backward(name):
    case, grads = V.BY_NAME[name], []
    with emu_backend.emulated(), emu_backend.chip_of(case.cus), G.guarded('cpu') as g:
        V.check_grad(case, 'cpu', outs_to=grads)
        if name not in G.CROPPED_DX:
            g.assert_guarded(grads)


# the routes of the 2-D DWT and of the DTCWT / ScatLayer family: every recorded case, the routes still the recorded ones
def _torch_made(case):
    """The steps of a DTCWT-family case whose tensors torch operations assemble from the kernels' outputs (which are guarded all the
    same): nothing for assert_guarded to find.  Established by running the cases under the harness."""
    steps = set()
    if case['shape'][-2] % 2 or case['shape'][-1] % 2:
        # the modules replicate the last row / column of an odd image with torch.cat (scatternet/layers.py, dtcwt/transform2d.py);
        # x.grad is that concatenation's backward (scatternet/lowlevel.py: "gradient of the edge replication")
        steps.add('backward')
    if case['kind'] == 'scatj2' and case['backward']:
        # the training route of ScatLayerj2 concatenates its orders with torch.cat and sums the gradients of its branches
        steps.update(('forward', 'backward'))
    if case['kind'] == 'scat' and case['biort'].endswith('_bp') and case['backward']:
        # no fused backward kernel for the band-pass taps: ScatLayerj1_f.backward falls back to the level-1 inverse, whose
        # band-pass branch ends in tensor arithmetic
        steps.add('backward')
    return steps


def _routes(mod, block, blocks, torch_made=lambda case: ()):
    golden = mod.load()
    for case, want in list(zip(mod.CASES, golden))[block::blocks]:
        with G.guarded('cpu') as g:
            got, tensors = mod.run_case(case)
            assert got == want, (case, got, want)
            skip = torch_made(case)
            if isinstance(got.get('backward'), list) and 'backward' in skip:
                tensors = tensors[:-1]                      # (x.grad is the last one)
            if 'forward' in skip:
                tensors = tensors[1:]                       # (ScatLayerj2: Z is the first and only output)
            # (the 0-dim placeholder of a skipped level is no kernel's output)
            tensors = [t for t in tensors if t.dim() > 0]
            if tensors:
                g.assert_guarded(tensors)


@pytest.mark.parametrize('block', range(16))
def test_dwt_routes(block):
    _routes(RC, block, 16)


@pytest.mark.parametrize('block', range(8))
def test_dtcwt_routes(block):
    _routes(DRC, block, 8, _torch_made)


# bfloat16: one case of every family tests/_bf16_cases.py covers
BF16_CASES = [
    B.dwt('dwt_rows', (2, 3, 64, 128), 3, 'db4', 'symmetric', 'WlAfbRows'),
    B.dwt1d('dwt1d', (2, 2, 1024), 3, 'db4', 'symmetric', 'WlDwt1dFused'),
    B.swt('swt', (1, 2, 20, 24), 2, 'db2', 'periodic', 'WlSwtLevel'),
    B.nonsep('nonsep', (1, 2, 32, 32), 'db2', 'zero', 'WlAfbNonsep'),
    B.dtcwt('dtcwt_a', (1, 2, 64, 128), 2, 'near_sym_a', 'qshift_a', 'WlDt'),
    B.scat('scat_train', (2, 3, 64, 64), 'near_sym_a', 'WlDt'),
    B.scatj2('scatj2', (1, 3, 64, 64), 'WlDt'),
    B.primitives('primitives', (1, 2, 32, 32), 'WlCorr1d'),
]


@pytest.mark.parametrize('case', BF16_CASES, ids=[c.name for c in BF16_CASES])
def test_bf16(case):
    with emu_backend.emulated(), G.guarded('cpu'):
        B.check(case, 'cpu', True)
