"""-m gpu: the 1-D DTCWT on the MI355X - DTCWT1DForward / DTCWT1DInverse, their gradients and the fused kernels of
csrc/wl_dtcwt1d.h - against the oracle's column primitives and the goldens (tests/_dtcwt1d_cases.py)."""
import pytest

import _dtcwt1d_cases as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32, F16, BF16 = S.F64, S.F32, S.F16, S.BF16


@pytest.mark.parametrize('pair', S.FUSED_PAIRS)
def test_values_layout_inverse_and_round_trip(pair):
    for n in (16, 20, 22, 37):
        for J in (1, 2, 3, 4):
            S.check_values(DEV, n, J, pair[0], pair[1])


@pytest.mark.parametrize('pair', [('antonini', 'qshift_c'), ('near_sym_b', 'qshift_d')])
def test_levels_far_shorter_than_the_filter(pair):
    S.check_values(DEV, 16, 4, pair[0], pair[1])
    S.check_values(DEV, 100, 3, pair[0], pair[1])


@pytest.mark.parametrize('dtype', [F16, BF16])
def test_float16_and_bfloat16(dtype):
    for b, q in S.FUSED_PAIRS + (('antonini', 'qshift_d'),):
        S.check_values(DEV, 37, 3, b, q, dtype, fused=True)
    S.check_gradients(DEV, 22, 3, 'near_sym_a', 'qshift_a', dtype)


def test_options_ri_dim_and_two_groups():
    S.check_options(DEV)


def test_float64_takes_the_generic_kernels():
    S.check_float64_takes_the_generic_kernels(DEV)


@pytest.mark.parametrize('n', [300, 301])
def test_chunk_seams_do_not_change_a_bit(n):
    S.check_seams(DEV, n)


def test_a_natural_multi_chunk_shape():
    S.check_natural_chunks(DEV)


@pytest.mark.parametrize('drop', [0, 1])
def test_inverse_with_none_highs(drop):
    S.check_none_highs(DEV, drop)


@pytest.mark.parametrize('pair', S.FUSED_PAIRS)
def test_gradients_follow_the_reference_rule(pair):
    for n, J in ((22, 3), (37, 4), (20, 2), (16, 1)):
        S.check_gradients(DEV, n, J, pair[0], pair[1], F32)
    S.check_gradients(DEV, 22, 3, pair[0], pair[1], F64)


@pytest.mark.parametrize('only', [0, 1, 3])
def test_gradient_of_a_single_output(only):
    S.check_gradients(DEV, 22, 3, 'near_sym_a', 'qshift_a', F32, only=only)


def test_gradcheck_float64():
    S.check_gradcheck(DEV)


@pytest.mark.parametrize('dtype', [F64, F32, F16, BF16])
def test_goldens(dtype):
    files = S.golden_files()
    assert files
    for f in files:
        S.check_golden(DEV, f, dtype)


def test_views():
    S.check_views(DEV)


def test_errors():
    S.check_errors(DEV)
    S.check_cpu_tensor_raises()
