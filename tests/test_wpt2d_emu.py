"""CPU tests (host emulation of the kernels): the 2-D wavelet packet transform - WPT2DForward / WPT2DInverse, their gradients,
the function-level pair and the packed-band kernels of csrc/wl_wpt2d.h - against the per-axis oracle (tests/_wpt2d_cases.py)."""
import pytest
import torch

import _wpt2d_cases as S
import emu_backend

F64, F32, F16, BF16 = S.F64, S.F32, S.F16, S.BF16


@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('J', [1, 2, 3])
def test_forward_values_and_layout(J, mode):
    with emu_backend.emulated():
        S.check_forward('cpu', (2, 3, 20, 28), 'db2', J, mode)
        S.check_forward('cpu', (1, 2, 37, 141), 'db4', J, mode)           # odd sizes, several tiles per axis, partial last tiles
        S.check_forward('cpu', (1, 1, 5, 7), 'db4', J, mode)              # planes shorter than the filter: several folds
        S.check_forward('cpu', (1, 2, 38, 150), 'db10', J, mode)


@pytest.mark.parametrize('mode', ['symmetric', 'periodization'])
def test_band_table_and_subtrees(mode):
    with emu_backend.emulated():
        S.check_band_table('cpu', (2, 3, 20, 28), 'db2', mode)


def test_freq_order_puts_every_cosine_into_its_slot():
    with emu_backend.emulated():
        S.check_freq_order('cpu')


def test_the_packet_kernels_ran_one_launch_per_level():
    with emu_backend.emulated():
        S.check_kernels_ran('cpu', 'symmetric')


def test_float64_generic_only_and_declines_take_the_fallback():
    with emu_backend.emulated():
        S.check_float64_generic('cpu')
        S.check_generic_only('cpu')
        S.check_declines('cpu')


def test_two_levels_per_launch_sequences_and_the_level_by_level_route():
    with emu_backend.emulated():
        S.check_two_level_sequence('cpu')


@pytest.mark.parametrize('dtype', [F16, BF16])
def test_two_levels_per_launch_float16_and_bfloat16(dtype):
    with emu_backend.emulated():
        S.check_two_level_low_precision('cpu', dtype)


@pytest.mark.parametrize('wave', ['db1', 'db2', 'db4', 'db6'])
def test_two_level_kernel_seams(wave):
    with emu_backend.emulated():
        S.check_wrap_shapes('cpu', wave, (1, 2, 72, 200))
        S.check_wrap_shapes('cpu', wave, (2, 1, 8, 12), two_level=wave in ('db1', 'db2'))   # db4 / db6: level 2 shorter than the filter


def test_outside_the_two_level_envelope_single_level_launches_run():
    with emu_backend.emulated():
        S.check_wrap_shapes('cpu', 'db4', (1, 2, 70, 200), two_level=False)                 # H % 4 != 0
        S.check_wrap_shapes('cpu', 'db7', (1, 2, 72, 200), two_level=False)                 # 14 taps
        S.check_wrap_shapes('cpu', 'db4', (1, 2, 72, 200), mode='symmetric', two_level=False)


@pytest.mark.parametrize('mode', S.MODES)
def test_inverse_vs_numpy_synthesis(mode):
    with emu_backend.emulated():
        S.check_inverse('cpu', (1, 2, 37, 141), 'db4', mode, J=2)
        S.check_inverse('cpu', (1, 2, 37, 141), 'db4', mode, J=2, with_size=False)


@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('wave', ['db2', 'db4', 'bior2.2'])
def test_perfect_reconstruction(wave, mode):
    with emu_backend.emulated():
        S.check_roundtrip('cpu', (1, 2, 16, 24), wave, mode)
        S.check_roundtrip('cpu', (1, 1, 19, 23), wave, mode)


def test_inverse_rejects_a_wrong_size_and_band_count():
    with emu_backend.emulated():
        S.check_inverse_errors('cpu')


@pytest.mark.parametrize('mode', S.MODES)
def test_gradients_follow_the_q9_rule(mode):
    with emu_backend.emulated():
        S.check_gradients('cpu', (2, 1, 9, 13), 'db2', mode, J=2)
        S.check_gradients('cpu', (1, 2, 13, 9), 'db4', mode, J=2, dtype=F64)


def test_zero_mode_dot_product_identity():
    with emu_backend.emulated():
        S.check_dot_product('cpu', (1, 2, 13, 9), 'db4')
        S.check_dot_product('cpu', (2, 1, 20, 28), 'db2')


@pytest.mark.parametrize('mode', ['symmetric', 'periodization'])
@pytest.mark.parametrize('dtype', [F16, BF16])
def test_float16_and_bfloat16(dtype, mode):
    with emu_backend.emulated():
        S.check_low_precision('cpu', dtype, mode)


def test_views_equal_their_contiguous_twins():
    with emu_backend.emulated():
        S.check_views('cpu')


def test_api():
    with emu_backend.emulated():
        S.check_api('cpu')
    S.check_cpu_tensor_raises()


SCHEDULES = [('forward', 'late', 0), ('reverse', 'eager', 0), ('shuffled', 'late', 1), ('shuffled', 'eager', 2)]


@pytest.mark.parametrize('order,dma,seed', SCHEDULES)
def test_lds_phases_do_not_depend_on_the_schedule(order, dma, seed):
    """The barrier phases of all four kernel forms: any visiting order of the lanes gives the bits of the default order.  The
    one-level pair on a multi-tile shape (the wide walk) and on a run of small planes (the plane-run walk) in symmetric mode, all
    four forms in a J = 3 periodization transform with two levels per launch on a multi-tile shape."""
    with emu_backend.emulated():
        cases = [((1, 2, 37, 141), 1, 'symmetric'), ((3, 20, 8, 8), 1, 'symmetric'), ((1, 2, 72, 200), 3, 'periodization')]
        with S.fused(True):
            for shape, J, mode in cases:
                xfm, ifm = S.modules('cpu', 'db4', J, mode)
                x = S.rand(shape, F32, 'cpu', 90)
                y = xfm(x)
                rec = ifm(y, size=shape[2:])
                with emu_backend.schedule(order, dma, seed):
                    assert torch.equal(xfm(x), y)
                    assert torch.equal(ifm(y, size=shape[2:]), rec)
