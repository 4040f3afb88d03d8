"""CPU tests (host emulation of the kernels): the 1-D stationary transform - SWT1DForward / SWT1DInverse, their gradients and the
wave-tile kernels of csrc/wl_swt1d.h - against the oracle's a-trous bank and its transposed matrices (tests/_swt1d_cases.py)."""
import pytest
import torch

import _swt1d_cases as S
import emu_backend

F32, F16, BF16 = S.F32, S.F16, S.BF16
# (order, seed): the barrier-free kernels have shuffles, no LDS-DMA - the visiting orders of tests/test_schedule_emu.py
SCHEDULES = [('forward', 0), ('reverse', 0), ('alternate', 0), ('shuffled', 1), ('shuffled', 2)]


def test_the_references_agree_with_each_other():
    S.check_transpose_forms()
    S.check_oracle_reconstructs()


@pytest.mark.parametrize('J', S.LEVELS)
@pytest.mark.parametrize('wave', S.WAVES)
def test_values_round_trip_inverse_and_gradients(wave, J):
    with emu_backend.emulated():
        S.check_grid('cpu', wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    with emu_backend.emulated():
        S.check_two_byte('cpu', wave, dtype)


@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', S.WAVES)
def test_tile_seams_do_not_change_a_bit(wave, J):
    with emu_backend.emulated():
        S.check_origin('cpu', wave, J)
        if wave == 'db4' and J == 3:
            S.check_origin('cpu', wave, J, F16)


def test_every_schedule_gives_the_same_bits():
    outs = []
    with emu_backend.emulated():
        for order, seed in SCHEDULES:
            with emu_backend.schedule(order, 'late', seed):
                outs.append(S.schedule_case('cpu'))
    for o in outs[1:]:
        assert len(o) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(o, outs[0]))


def test_other_modes_odd_taps_and_float64_go_level_by_level():
    with emu_backend.emulated():
        S.check_unfused_routes('cpu')


@pytest.mark.parametrize('dtype', [F32, F16])
def test_the_switch_takes_the_composition(dtype):
    with emu_backend.emulated():
        S.check_switch('cpu', dtype)


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


def test_state_dicts_of_the_decimated_modules_load():
    S.check_state_dict('cpu')
