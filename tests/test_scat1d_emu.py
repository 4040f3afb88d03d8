"""CPU tests (host emulation of the kernels): the 1-D scattering layer - ScatLayer1D, its gradient and the wave-tile kernels of
csrc/wl_scat1d.h - against a numpy restatement of its definition on the oracle's colfilter (tests/_scat1d_cases.py)."""
import pytest
import torch

import _scat1d_cases as S
import emu_backend

F32, F16, BF16 = S.F32, S.F16, S.BF16
# (order, seed): the barrier-free kernels have shuffles, no LDS-DMA - the visiting orders of tests/test_swt1d_emu.py
SCHEDULES = [('forward', 0), ('reverse', 0), ('alternate', 0), ('shuffled', 1), ('shuffled', 2)]


def test_the_gradient_rule_is_the_adjoint():
    S.check_adjoint_of_the_rule()


@pytest.mark.parametrize('biort', sorted(S.BIORTS))
def test_values_and_gradients(biort):
    with emu_backend.emulated():
        S.check_grid('cpu', biort)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('biort', ['near_sym_a', 'near_sym_b'])
def test_float16_and_bfloat16(biort, dtype):
    with emu_backend.emulated():
        S.check_two_byte('cpu', biort, dtype)


@pytest.mark.parametrize('biort', sorted(S.BIORTS))
def test_tile_seams_do_not_change_a_bit(biort):
    with emu_backend.emulated():
        S.check_origin('cpu', biort)
        if biort == 'near_sym_b':
            S.check_origin('cpu', biort, F16)


def test_every_schedule_gives_the_same_bits():
    outs = []
    with emu_backend.emulated():
        for order, seed in SCHEDULES:
            with emu_backend.schedule(order, 'late', seed):
                outs.append(S.schedule_case('cpu'))
    for o in outs[1:]:
        assert len(o) == len(outs[0]) and all(torch.equal(a, b) for a, b in zip(o, outs[0]))


@pytest.mark.parametrize('biort', ['near_sym_a', 'near_sym_b'])
def test_the_layer_is_level_one_of_the_dtcwt(biort):
    with emu_backend.emulated():
        S.check_identity('cpu', biort)


def test_float64_custom_taps_and_the_switch_take_the_composition():
    with emu_backend.emulated():
        S.check_routes('cpu')


def test_inference_stores_no_directions():
    with emu_backend.emulated():
        S.check_inference_stores_no_directions('cpu')


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
