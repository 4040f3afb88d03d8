"""CPU tests (host emulation of the kernels): the 3-D DWT - DWT3DForward / DWT3DInverse, their gradients, ops.afb_depth /
ops.sfb_depth and the streaming depth kernels of csrc/wl_dwt3d.h - against the per-axis oracle (tests/_dwt3d_cases.py)."""
import pytest
import torch

import _dwt3d_cases as S
import emu_backend
import pytorch_wavelets_amd as pw

F64, F32, F16, BF16 = S.F64, S.F32, S.F16, S.BF16


@pytest.mark.parametrize('mode', S.MODES)
def test_forward_values_and_layout(mode):
    with emu_backend.emulated():
        S.check_forward('cpu', (2, 3, 10, 12, 16), 'db2', 1, mode)
        S.check_forward('cpu', (2, 1, 7, 9, 11), 'db4', 2, mode)          # everything odd, two levels


@pytest.mark.parametrize('mode', ['symmetric', 'reflect'])
def test_depth_shorter_than_the_filter_folds_several_times(mode):
    with emu_backend.emulated():
        S.check_forward('cpu', (1, 1, 3, 20, 24), 'bior2.2', 1, mode)


@pytest.mark.parametrize('mode', ['symmetric', 'periodization'])
def test_band_table_and_dwtforward_slices(mode):
    with emu_backend.emulated():
        S.check_band_table('cpu', (2, 3, 10, 12, 16), 'db2', mode)


def test_the_depth_kernels_ran_and_float64_takes_the_generic_ones():
    with emu_backend.emulated():
        S.check_kernels_ran('cpu')


@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('wave', ['db4', 'db10'])
@pytest.mark.parametrize('n', [22, 23])
def test_chunk_seams_do_not_change_a_bit(n, wave, mode):
    with emu_backend.emulated():
        S.check_chunks('cpu', n, wave, mode)


@pytest.mark.parametrize('mode', ['symmetric', 'periodization'])
def test_chunk_policy_on_two_chip_sizes(mode):
    """chunks = 0 on a chip of 1 and of 64 compute units: the policy cuts the depth axis on the larger one only, and the numbers
    stay those of one chunk."""
    with emu_backend.emulated():
        base, _, _ = S.depth_pair('cpu', (3, 22, 64), 'db4', mode, 1)
        grids = []
        for cus in (1, 64):
            with emu_backend.chip_of(cus):
                outs, _, _ = S.depth_pair('cpu', (3, 22, 64), 'db4', mode, 0)
                grids.append(int(emu_backend.handle().wl_last_grid()))
            for a, b in zip(outs, base):
                assert torch.equal(a, b)
        assert grids[1] > grids[0], grids


@pytest.mark.parametrize('dtype', [F32, F16, BF16])
def test_vector_and_scalar_bodies(dtype):
    with emu_backend.emulated():
        S.check_vec_bodies('cpu', dtype)


def test_declines_fall_back_to_the_generic_path():
    """Periodization of a depth shorter than the filter (the reference's single fold), 22 taps and float64: afb_depth / sfb_depth
    return None, the modules still give the oracle's numbers."""
    from pytorch_wavelets_amd import ops
    with emu_backend.emulated():
        h = S.tap_tensors('db4', 'cpu')
        x = S.rand((2, 5, 16), F32, 'cpu', 1)
        assert ops.afb_depth([x], h[0], h[1], 2) is None
        assert ops.afb_depth([x.double()], h[0], h[1], 1) is None
        h11 = S.tap_tensors('db11', 'cpu')
        assert ops.afb_depth([S.rand((2, 30, 16), F32, 'cpu', 2)], h11[0], h11[1], 1) is None
        assert ops.sfb_depth([S.rand((2, 2, 16), F32, 'cpu', 3)], [None], h[0], h[1], 2) is None
        x, yl, yh, ks = S.check_forward('cpu', (1, 2, 5, 12, 16), 'db4', 1, 'periodization')
        assert not any('Depth' in k for k in ks), ks
        S.check_inverse('cpu', (1, 2, 3, 12, 16), 'db4', 'periodization', J=1)
        S.check_forward('cpu', (1, 1, 30, 24, 24), 'db11', 1, 'symmetric')


@pytest.mark.parametrize('mode', S.MODES)
def test_inverse_vs_numpy_synthesis(mode):
    with emu_backend.emulated():
        S.check_inverse('cpu', (2, 1, 7, 9, 11), 'db4', mode, J=2)         # odd sizes: the 'unpad' along every axis
        S.check_inverse('cpu', (1, 2, 7, 9, 11), 'db2', mode, J=2, drop=0)
        S.check_inverse('cpu', (1, 2, 7, 9, 11), 'db2', mode, J=2, drop=1)


@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('wave', ['db2', 'db4', 'bior2.2'])
def test_perfect_reconstruction(wave, mode):
    with emu_backend.emulated():
        S.check_roundtrip('cpu', (1, 2, 8, 12, 16), wave, mode)
        S.check_roundtrip('cpu', (1, 1, 9, 11, 13), wave, mode)


@pytest.mark.parametrize('mode', S.MODES)
def test_gradients_follow_the_q9_rule(mode):
    with emu_backend.emulated():
        S.check_gradients('cpu', (2, 1, 7, 9, 11), 'db2', mode, J=2)
        S.check_gradients('cpu', (1, 2, 9, 7, 13), 'db4', mode, J=2, dtype=F64)


def test_zero_mode_dot_product_identity():
    with emu_backend.emulated():
        S.check_dot_product('cpu', (1, 2, 7, 9, 11), 'db4')
        S.check_dot_product('cpu', (2, 1, 10, 12, 16), 'db2')


@pytest.mark.parametrize('dtype', [F16, BF16])
def test_float16_and_bfloat16(dtype):
    with emu_backend.emulated():
        S.check_low_precision('cpu', dtype)


def test_views_equal_their_contiguous_twins():
    with emu_backend.emulated():
        S.check_views('cpu')


def test_api():
    with emu_backend.emulated():
        S.check_api('cpu')
    S.check_cpu_tensor_raises()
