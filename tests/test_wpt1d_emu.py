"""CPU tests (host emulation of the kernels): the 1-D wavelet packet transform - WPT1DForward / WPT1DInverse, their gradients and
the wave-tile kernels of csrc/wl_wpt1d.h - against the oracle's filter banks and the dense matrices it makes of an identity
(tests/_wpt1d_cases.py)."""
import pytest

import _wpt1d_cases as P
import emu_backend

F32, F16, BF16 = P.F32, P.F16, P.BF16


def test_the_closed_forms_are_the_oracles_periodization_banks():
    P.check_closed_forms()


def test_the_references_agree_with_each_other():
    P.check_transposes()


@pytest.mark.parametrize('J', P.LEVELS)
@pytest.mark.parametrize('wave', P.WAVES)
def test_values_inverse_round_trip_gradients_and_launches(wave, J):
    with emu_backend.emulated():
        P.check_grid('cpu', wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    with emu_backend.emulated():
        P.check_two_byte('cpu', wave, dtype)


def test_one_level_and_band_zero_are_the_decimated_transform():
    with emu_backend.emulated():
        P.check_identities('cpu')


@pytest.mark.parametrize('dtype', P.GRID_DTYPES)
@pytest.mark.parametrize('wave', P.GRID_WAVES)
def test_every_instantiation(wave, dtype):
    with emu_backend.emulated():
        P.check_instantiation('cpu', wave, dtype)


@pytest.mark.parametrize('dtype', [F32, F16])
@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', P.WAVES)
def test_tile_seams_do_not_change_a_bit(wave, J, dtype):
    with emu_backend.emulated():
        P.check_origin('cpu', wave, J, dtype)


def test_declined_routes_give_the_oracles_answer():
    with emu_backend.emulated():
        P.check_declined_routes('cpu')


def test_gradcheck_float64():
    with emu_backend.emulated():
        P.check_gradcheck('cpu')


@pytest.mark.parametrize('dtype', [F32, F16])
def test_the_switch_takes_the_composition(dtype):
    with emu_backend.emulated():
        P.check_switch('cpu', dtype)


def test_errors_and_edges():
    with emu_backend.emulated():
        P.check_errors_and_edges('cpu')
    P.check_cpu_tensor_raises()


def test_views():
    with emu_backend.emulated():
        P.check_views('cpu')


def test_state_dicts_of_the_decimated_modules_load():
    P.check_state_dict('cpu')


def test_frequency_order():
    P.check_freq_order()
