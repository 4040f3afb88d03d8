"""-m gpu: the 1-D stationary transform on the MI355X - SWT1DForward / SWT1DInverse, their gradients and the wave-tile kernels of
csrc/wl_swt1d.h - against the oracle's a-trous bank and its transposed matrices (tests/_swt1d_cases.py)."""
import pytest

import _swt1d_cases as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F16, BF16 = S.F32, S.F16, S.BF16


@pytest.mark.parametrize('J', S.LEVELS)
@pytest.mark.parametrize('wave', S.WAVES)
def test_values_round_trip_inverse_and_gradients(wave, J):
    S.check_grid(DEV, wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    S.check_two_byte(DEV, wave, dtype)


@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', S.WAVES)
def test_tile_seams_do_not_change_a_bit(wave, J):
    S.check_origin(DEV, wave, J)
    if wave == 'db4' and J == 3:
        S.check_origin(DEV, wave, J, F16)


def test_other_modes_odd_taps_and_float64_go_level_by_level():
    S.check_unfused_routes(DEV)


@pytest.mark.parametrize('dtype', [F32, F16])
def test_the_switch_takes_the_composition(dtype):
    S.check_switch(DEV, dtype)


def test_gradcheck_float64():
    S.check_gradcheck(DEV)


def test_errors_and_edges():
    S.check_errors_and_edges(DEV)
    S.check_cpu_tensor_raises()


def test_views():
    S.check_views(DEV)


def test_state_dicts_of_the_decimated_modules_load():
    S.check_state_dict(DEV)
