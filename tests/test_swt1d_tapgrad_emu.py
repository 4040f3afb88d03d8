"""CPU tests (host emulation of the kernels): the filter-tap gradients of the 1-D stationary transform - SWT1DForward /
SWT1DInverse / SWT1DShrink with learned taps and the wave-tile kernel of csrc/wl_swt1d_tapgrad.h - against the float64 chain of
the pinned oracle and the formula of the kernel's header (tests/_swt1d_tapgrad_cases.py)."""
import pytest
import torch

import _swt1d_tapgrad_cases as T
import emu_backend

F32, F16, BF16 = T.F32, T.F16, T.BF16
# (order, seed): the barrier-free kernels have shuffles, no LDS-DMA - the visiting orders of tests/test_swt1d_emu.py
SCHEDULES = [('forward', 0), ('reverse', 0), ('alternate', 0), ('shuffled', 1), ('shuffled', 2)]


def test_the_oracle_is_the_gradient():
    T.check_oracle()


@pytest.mark.parametrize('J', T.LEVELS)
@pytest.mark.parametrize('wave', T.WAVES)
def test_both_directions(wave, J):
    with emu_backend.emulated():
        T.check_grid('cpu', wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    with emu_backend.emulated():
        T.check_two_byte('cpu', wave, dtype)


def test_float64_takes_the_composition():
    with emu_backend.emulated():
        T.check_float64('cpu')


@pytest.mark.parametrize('dtype', T.GRID_DTYPES)
@pytest.mark.parametrize('wave', T.GRID_WAVES)
def test_every_instantiation(wave, dtype):
    with emu_backend.emulated():
        T.check_instantiation('cpu', wave, dtype)
        if dtype == F32:
            T.check_levels('cpu', wave)


@pytest.mark.parametrize('wave', T.SEAM_WAVES)
def test_tile_seams_do_not_change_the_sums(wave):
    with emu_backend.emulated():
        T.check_origin('cpu', wave)
        if wave == 'db10':
            T.check_origin('cpu', wave, 3, F16)


def test_every_schedule_gives_the_same_bits():
    outs = []
    with emu_backend.emulated():
        for order, seed in SCHEDULES:
            with emu_backend.schedule(order, 'late', seed):
                outs.append(T.schedule_case('cpu'))
    for o in outs[1:]:
        assert len(o) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(o, outs[0]))


def test_the_switch_and_a_declined_launch_compose():
    with emu_backend.emulated():
        T.check_routes('cpu')
        T.check_a_memoised_decline('cpu')


def test_fixed_taps_launch_as_before():
    with emu_backend.emulated():
        T.check_fixed_taps_launch_as_before('cpu')


def test_gradcheck_float64():
    with emu_backend.emulated():
        T.check_gradcheck('cpu')


def test_shrink_learns_thresholds_and_filters():
    with emu_backend.emulated():
        T.check_shrink_learns_everything('cpu')


def test_modules():
    with emu_backend.emulated():
        T.check_modules('cpu')
        T.check_empty_yh('cpu')


def test_errors_and_edges():
    with emu_backend.emulated():
        T.check_errors_and_edges('cpu')
    T.check_cpu_tensor_raises()


def test_views():
    with emu_backend.emulated():
        T.check_views('cpu')


def test_guarded_launch():
    with emu_backend.emulated():
        T.check_guard('cpu')
