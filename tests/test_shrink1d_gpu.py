"""-m gpu: SWT1DShrink on the MI355X - one-launch wavelet shrinkage of the 1-D stationary transform, its gradients in x and in
the thresholds, and the wave-tile kernels of csrc/wl_shrink1d.h - against the float64 chain of the pinned oracle with numpy
shrinkage in between (tests/_shrink1d_cases.py)."""
import pytest

import _shrink1d_cases as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F16, BF16 = S.F32, S.F16, S.BF16


@pytest.mark.parametrize('J', S.LEVELS)
@pytest.mark.parametrize('wave', S.WAVES)
def test_values_and_gradients(wave, J):
    S.check_grid(DEV, wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    S.check_two_byte(DEV, wave, dtype)


def test_float64_takes_the_composition():
    S.check_float64(DEV)


@pytest.mark.parametrize('dtype', S.GRID_DTYPES)
@pytest.mark.parametrize('wave', S.GRID_WAVES)
def test_every_instantiation(wave, dtype):
    S.check_instantiation(DEV, wave, dtype)


@pytest.mark.parametrize('J', [1, 2, 3])
@pytest.mark.parametrize('wave', S.WAVES)
def test_tile_seams_do_not_change_a_bit(wave, J):
    S.check_origin(DEV, wave, J)
    if wave == 'db10' and J == 3:
        S.check_origin(DEV, wave, J, F16)


def test_identities():
    S.check_identities(DEV)


def test_the_switch_takes_the_composition():
    S.check_switch(DEV)


def test_a_declined_launch_composes():
    S.check_a_declined_launch_composes(DEV)


def test_no_partials_without_a_learned_threshold():
    S.check_no_partials_without_a_learned_threshold(DEV)


def test_gradcheck_float64():
    S.check_gradcheck(DEV)


def test_errors_and_edges():
    S.check_errors_and_edges(DEV)
    S.check_cpu_tensor_raises()


def test_views():
    S.check_views(DEV)


def test_universal_thresh():
    S.check_universal_thresh(DEV)
