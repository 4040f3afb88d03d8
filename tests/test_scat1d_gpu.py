"""-m gpu: the 1-D scattering layer on the MI355X - ScatLayer1D, its gradient and the wave-tile kernels of csrc/wl_scat1d.h -
against a numpy restatement of its definition on the oracle's colfilter (tests/_scat1d_cases.py)."""
import pytest

import _scat1d_cases as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F16, BF16 = S.F32, S.F16, S.BF16


@pytest.mark.parametrize('biort', sorted(S.BIORTS))
def test_values_and_gradients(biort):
    S.check_grid(DEV, biort)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('biort', ['near_sym_a', 'near_sym_b'])
def test_float16_and_bfloat16(biort, dtype):
    S.check_two_byte(DEV, biort, dtype)


@pytest.mark.parametrize('biort', sorted(S.BIORTS))
def test_tile_seams_do_not_change_a_bit(biort):
    S.check_origin(DEV, biort)
    if biort == 'near_sym_b':
        S.check_origin(DEV, biort, F16)


@pytest.mark.parametrize('biort', ['near_sym_a', 'near_sym_b'])
def test_the_layer_is_level_one_of_the_dtcwt(biort):
    S.check_identity(DEV, biort)


def test_float64_custom_taps_and_the_switch_take_the_composition():
    S.check_routes(DEV)


def test_inference_stores_no_directions():
    S.check_inference_stores_no_directions(DEV)


def test_gradcheck_float64():
    S.check_gradcheck(DEV)


def test_errors_and_edges():
    S.check_errors_and_edges(DEV)
    S.check_cpu_tensor_raises()


def test_views():
    S.check_views(DEV)
