"""-m gpu: the filter-tap gradients of the 1-D stationary transform on the MI355X - SWT1DForward / SWT1DInverse / SWT1DShrink
with learned taps and the wave-tile kernel of csrc/wl_swt1d_tapgrad.h - against the float64 chain of the pinned oracle and the
formula of the kernel's header (tests/_swt1d_tapgrad_cases.py)."""
import pytest

import _swt1d_tapgrad_cases as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F16, BF16 = T.F32, T.F16, T.BF16


@pytest.mark.parametrize('J', T.LEVELS)
@pytest.mark.parametrize('wave', T.WAVES)
def test_both_directions(wave, J):
    T.check_grid(DEV, wave, J)


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('wave', ['db4', 'db10'])
def test_float16_and_bfloat16(wave, dtype):
    T.check_two_byte(DEV, wave, dtype)


def test_float64_takes_the_composition():
    T.check_float64(DEV)


@pytest.mark.parametrize('dtype', T.GRID_DTYPES)
@pytest.mark.parametrize('wave', T.GRID_WAVES)
def test_every_instantiation(wave, dtype):
    T.check_instantiation(DEV, wave, dtype)
    if dtype == F32:
        T.check_levels(DEV, wave)


@pytest.mark.parametrize('wave', T.SEAM_WAVES)
def test_tile_seams_do_not_change_the_sums(wave):
    T.check_origin(DEV, wave)
    if wave == 'db10':
        T.check_origin(DEV, wave, 3, F16)


def test_the_switch_and_a_declined_launch_compose():
    T.check_routes(DEV)
    T.check_a_memoised_decline(DEV)


def test_fixed_taps_launch_as_before():
    T.check_fixed_taps_launch_as_before(DEV)


def test_gradcheck_float64():
    T.check_gradcheck(DEV)


def test_shrink_learns_thresholds_and_filters():
    T.check_shrink_learns_everything(DEV)


def test_modules():
    T.check_modules(DEV)
    T.check_empty_yh(DEV)


def test_errors_and_edges():
    T.check_errors_and_edges(DEV)
    T.check_cpu_tensor_raises()


def test_views():
    T.check_views(DEV)


def test_guarded_launch():
    T.check_guard(DEV)
