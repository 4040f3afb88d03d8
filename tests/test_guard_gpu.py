"""-m gpu: guard bands around every output on the MI355X (tests/_guard_cases.py).  The existing shared checks of every kernel
family run inside ``guarded('cuda:0')``: they still compare with their float64 oracles and still assert which kernels ran, and on
exit no store may have landed in front of or behind an output - on the chip that is the caching allocator's neighbouring block,
somebody else's tensor - and no output element may be left unwritten.  The harness itself is tested in tests/test_guard_emu.py."""
import pytest
import torch

import _bf16_cases as B
import _dtcwt1d_cases as D1
import _dwt3d_cases as V3
import _guard_cases as G
import _scat1d_cases as SC
import _swt1d_cases as S1
import _view_cases as V
import _wpt1d_cases as P1
import _wpt2d_cases as P2
import test_dwt_routes_gpu as RG
from pytorch_wavelets_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
IDS = dict(ids=lambda v: v if isinstance(v, str) else str(v).replace('torch.', ''))


def _guarded(fn, *a, **kw):
    with G.guarded(DEV):
        return fn(DEV, *a, **kw)


def test_the_guard_hands_out_device_blocks():
    with G.guarded(DEV) as g:
        t = torch.empty(3, 5, device=DEV)
        assert t.is_cuda and t.is_contiguous() and t.data_ptr() % 256 == 0 and len(g.blocks) == 1
        t.zero_()
        g.assert_guarded(t)


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
def test_dtcwt1d_values(pair):
    for n in (16, 20, 22, 37):
        with G.guarded(DEV):
            for J in (1, 2, 3, 4):
                D1.check_values(DEV, n, J, pair[0], pair[1])


@pytest.mark.parametrize('pair', D1.FUSED_PAIRS, ids='-'.join)
def test_dtcwt1d_gradients(pair):
    with G.guarded(DEV):
        for n, J in ((22, 3), (37, 4), (20, 2), (16, 1)):
            D1.check_gradients(DEV, n, J, pair[0], pair[1], F32)
        D1.check_gradients(DEV, 22, 3, pair[0], pair[1], F64)


@pytest.mark.parametrize('dtype', [F16, BF16], **IDS)
def test_dtcwt1d_two_byte(dtype):
    with G.guarded(DEV):
        for b, q in D1.FUSED_PAIRS + (('antonini', 'qshift_d'),):
            D1.check_values(DEV, 37, 3, b, q, dtype, fused=True)
        D1.check_gradients(DEV, 22, 3, 'near_sym_a', 'qshift_a', dtype)


@pytest.mark.parametrize('n', [300, 301])
def test_dtcwt1d_seams(n):
    _guarded(D1.check_seams, n)


@pytest.mark.parametrize('drop', [0, 1])
def test_dtcwt1d_none_highs(drop):
    _guarded(D1.check_none_highs, drop)


# DWT3D
@pytest.mark.parametrize('mode', V3.MODES)
def test_dwt3d_forward_inverse_gradients(mode):
    with G.guarded(DEV) as g:
        for shape, wave, J in (((2, 3, 10, 12, 16), 'db2', 1), ((2, 1, 7, 9, 11), 'db4', 2)):
            x, yl, yh, _ = V3.check_forward(DEV, shape, wave, J, mode)
            g.assert_guarded(yl, yh, inputs=[x])
        V3.check_inverse(DEV, (2, 1, 7, 9, 11), 'db4', mode, J=2)
        V3.check_inverse(DEV, (1, 2, 7, 9, 11), 'db2', mode, J=2, drop=1)
        V3.check_gradients(DEV, (2, 1, 7, 9, 11), 'db2', mode, J=2)


@pytest.mark.parametrize('dtype', [F32, F16, BF16], **IDS)
def test_dwt3d_vector_and_scalar_bodies(dtype):
    _guarded(V3.check_vec_bodies, dtype)


@pytest.mark.parametrize('dtype', V3.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', V3.GRID_WAVES)
def test_dwt3d_depth_kernels_inner_sizes_64_68_5(wave, dtype):
    _guarded(V3.check_depth_instantiation, wave, dtype)


# WPT2D
@pytest.mark.parametrize('mode', P2.MODES)
def test_wpt2d_forward(mode):
    with G.guarded(DEV):
        for J in (1, 2, 3):
            for shape, wave in (((2, 3, 20, 28), 'db2'), ((1, 2, 37, 141), 'db4'), ((1, 1, 5, 7), 'db4'), ((1, 2, 38, 150), 'db10')):
                P2.check_forward(DEV, shape, wave, J, mode)


@pytest.mark.parametrize('mode', P2.MODES)
def test_wpt2d_inverse_and_gradients(mode):
    with G.guarded(DEV):
        P2.check_inverse(DEV, (1, 2, 37, 141), 'db4', mode, J=2)
        P2.check_inverse(DEV, (1, 2, 37, 141), 'db4', mode, J=2, with_size=False)
        P2.check_gradients(DEV, (2, 1, 9, 13), 'db2', mode, J=2)
        P2.check_gradients(DEV, (1, 2, 13, 9), 'db4', mode, J=2, dtype=F64)


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
@pytest.mark.parametrize('name', [c.name for c in V.CASES if c.only != 'emu'])
def test_view_table(name):
    outs = []
    with G.guarded(DEV) as g:
        V.check(V.BY_NAME[name], DEV, outs_to=outs)
        g.assert_guarded(outs)


# (off by default - dwt/lowlevel.py: _PAD_LL -: the per-level path with its inner ll at a cache-line row pitch, the `_ll_pitch` buffers
#  of ops.afb2d whose pad columns nobody writes)
PAD_LL = V.Case('tile-fwd-pad-ll', V.dwt_fwd(2, 'db2', 'symmetric'), (2, 1, 70, 132), F32, V.offset(1), ['WlAfbTile<', ('WlAfbSmall<', 'WlAfbTile<')],
                pin={'_PAD_LL': True, 'FUSED_LEVELS': False})


def test_view_table_padded_ll_pitch():
    outs = []
    with G.guarded(DEV) as g:
        V.check(PAD_LL, DEV, outs_to=outs)
        g.assert_guarded(outs)
        assert any(b.allowed and b.site.endswith(' afb2d()') for b in g.blocks), [b.site for b in g.blocks]


@pytest.mark.parametrize('name', V.GRAD_CASES)
def test_view_table_backward(name):
    grads = []
    with G.guarded(DEV) as g:
        V.check_grad(V.BY_NAME[name], DEV, outs_to=grads)
        if name not in G.CROPPED_DX:
            g.assert_guarded(grads)


# the two cases of tests/_route_cases.py that reach the streaming synthesis paths on the real chip
@pytest.mark.parametrize('shape,J,pin', [((12, 96, 80), 3, 'FUSED_STRIPS'), ((2, 40, 704), 1, 'STREAM_FORCE')])
def test_dwt_synthesis_ladder_paths(shape, J, pin, monkeypatch):
    with G.guarded(DEV):
        RG.test_synthesis_ladder_paths_vs_oracle(shape, J, pin, monkeypatch)


# bfloat16: one case of every family tests/_bf16_cases.py covers, at the emulator's sizes (the streaming kernels forced)
BF16_CASES = [
    B.dwt('dwt_rows', (2, 3, 64, 128), 3, 'db4', 'symmetric', 'WlAfbRows', ctx=lambda: B._setattrs(ops, FUSED_STRIPS=1)),
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
    with G.guarded(DEV):
        B.check(case, DEV, True)
