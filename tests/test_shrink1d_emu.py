"""CPU tests (host emulation of the kernels): SWT1DShrink - one-launch wavelet shrinkage of the 1-D stationary transform, its
gradients in x and in the thresholds, and the wave-tile kernels of csrc/wl_shrink1d.h - against the float64 chain of the pinned
oracle with numpy shrinkage in between (tests/_shrink1d_cases.py)."""
import pytest
import torch

import _shrink1d_cases as S
import emu_backend

F32, F16, BF16 = S.F32, S.F16, S.BF16
# (order, seed): the barrier-free kernels have shuffles, no LDS-DMA - the visiting orders of tests/test_swt1d_emu.py
SCHEDULES = [('forward', 0), ('reverse', 0), ('alternate', 0), ('shuffled', 1), ('shuffled', 2)]


@pytest.mark.parametrize('J', S.LEVELS)
@pytest.mark.parametrize('wave', S.WAVES)
def test_values_and_gradients(wave, J):
    with emu_backend.emulated():
        S.check_grid('cpu', wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    with emu_backend.emulated():
        S.check_two_byte('cpu', wave, dtype)


def test_float64_takes_the_composition():
    with emu_backend.emulated():
        S.check_float64('cpu')


@pytest.mark.parametrize('dtype', S.GRID_DTYPES)
@pytest.mark.parametrize('wave', S.GRID_WAVES)
def test_every_instantiation(wave, dtype):
    with emu_backend.emulated():
        S.check_instantiation('cpu', wave, dtype)


@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', S.WAVES)
def test_tile_seams_do_not_change_a_bit(wave, J):
    with emu_backend.emulated():
        S.check_origin('cpu', wave, J)
        if wave == 'db10' and J == 3:
            S.check_origin('cpu', wave, J, F16)


def test_every_schedule_gives_the_same_bits():
    outs = []
    with emu_backend.emulated():
        for order, seed in SCHEDULES:
            with emu_backend.schedule(order, 'late', seed):
                outs.append(S.schedule_case('cpu'))
    for o in outs[1:]:
        assert len(o) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(o, outs[0]))


def test_identities():
    with emu_backend.emulated():
        S.check_identities('cpu')


def test_the_switch_takes_the_composition():
    with emu_backend.emulated():
        S.check_switch('cpu')


def test_a_declined_launch_composes():
    with emu_backend.emulated():
        S.check_a_declined_launch_composes('cpu')


def test_no_partials_without_a_learned_threshold():
    with emu_backend.emulated():
        S.check_no_partials_without_a_learned_threshold('cpu')


def test_gradcheck_float64():
    with emu_backend.emulated():
        S.check_gradcheck('cpu')


def test_errors_and_edges():
    with emu_backend.emulated():
        S.check_errors_and_edges('cpu')
    S.check_cpu_tensor_raises()


def test_views():
    with emu_backend.emulated():
        S.check_views('cpu')


def test_universal_thresh():
    with emu_backend.emulated():
        S.check_universal_thresh('cpu')
