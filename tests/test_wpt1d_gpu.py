"""-m gpu: the 1-D wavelet packet transform on the MI355X - WPT1DForward / WPT1DInverse, their gradients and the wave-tile kernels
of csrc/wl_wpt1d.h - against the oracle's filter banks and the dense matrices it makes of an identity (tests/_wpt1d_cases.py)."""
import pytest

import _wpt1d_cases as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F16, BF16 = P.F32, P.F16, P.BF16


@pytest.mark.parametrize('J', P.LEVELS)
@pytest.mark.parametrize('wave', P.WAVES)
def test_values_inverse_round_trip_gradients_and_launches(wave, J):
    P.check_grid(DEV, wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    P.check_two_byte(DEV, wave, dtype)


def test_one_level_and_band_zero_are_the_decimated_transform():
    P.check_identities(DEV)


@pytest.mark.parametrize('dtype', P.GRID_DTYPES)
@pytest.mark.parametrize('wave', P.GRID_WAVES)
def test_every_instantiation(wave, dtype):
    P.check_instantiation(DEV, wave, dtype)


@pytest.mark.parametrize('dtype', [F32, F16])
@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', P.WAVES)
def test_tile_seams_do_not_change_a_bit(wave, J, dtype):
    P.check_origin(DEV, wave, J, dtype)


def test_declined_routes_give_the_oracles_answer():
    P.check_declined_routes(DEV)


def test_gradcheck_float64():
    P.check_gradcheck(DEV)


@pytest.mark.parametrize('dtype', [F32, F16])
def test_the_switch_takes_the_composition(dtype):
    P.check_switch(DEV, dtype)


def test_errors_and_edges():
    P.check_errors_and_edges(DEV)
    P.check_cpu_tensor_raises()


def test_views():
    P.check_views(DEV)


def test_state_dicts_of_the_decimated_modules_load():
    P.check_state_dict(DEV)
