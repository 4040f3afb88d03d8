"""CPU tests (host emulation of the kernels): the 1-D DTCWT - DTCWT1DForward / DTCWT1DInverse, their gradients and the fused
kernels of csrc/wl_dtcwt1d.h - against the oracle's column primitives and the goldens (tests/_dtcwt1d_cases.py)."""
import pytest
import torch

import _dtcwt1d_cases as S
import emu_backend

F64, F32, F16, BF16 = S.F64, S.F32, S.F16, S.BF16
# (order, dma, seed): the seven schedules of tests/test_schedule_emu.py
SCHEDULES = [('alternate', 'late', 0), ('forward', 'late', 0), ('reverse', 'late', 0), ('shuffled', 'late', 1),
             ('shuffled', 'late', 2), ('forward', 'eager', 0), ('shuffled', 'eager', 3)]


@pytest.mark.parametrize('pair', S.FUSED_PAIRS)
@pytest.mark.parametrize('n', [16, 20, 22, 37])
def test_values_layout_inverse_and_round_trip(n, pair):
    with emu_backend.emulated():
        for J in (1, 2, 3, 4):
            S.check_values('cpu', n, J, pair[0], pair[1])


def test_the_table_sizes_take_the_fused_kernels():
    """n = 16 .. 37 up to J = 3 with 10-tap q-shift filters, and what the one-fold rule says beyond."""
    for n in (16, 20, 22, 37):
        assert S.expect_fused(n, 3, 'qshift_a') == (True, True) and S.expect_fused(n, 3, 'qshift_06') == (True, True)
    assert S.expect_fused(16, 4, 'qshift_a') == (False, False) and S.expect_fused(512, 4, 'qshift_d') == (True, True)


@pytest.mark.parametrize('pair', [('antonini', 'qshift_c'), ('near_sym_b', 'qshift_d')])
def test_levels_far_shorter_than_the_filter(pair):
    with emu_backend.emulated():
        S.check_values('cpu', 16, 4, pair[0], pair[1])
        S.check_values('cpu', 100, 3, pair[0], pair[1])


@pytest.mark.parametrize('dtype', [F16, BF16])
def test_float16_and_bfloat16(dtype):
    with emu_backend.emulated():
        for b, q in S.FUSED_PAIRS + (('antonini', 'qshift_d'),):
            S.check_values('cpu', 37, 3, b, q, dtype, fused=True)
        S.check_gradients('cpu', 22, 3, 'near_sym_a', 'qshift_a', dtype)


def test_options_ri_dim_and_two_groups():
    with emu_backend.emulated():
        S.check_options('cpu')


def test_float64_takes_the_generic_kernels():
    with emu_backend.emulated():
        S.check_float64_takes_the_generic_kernels('cpu')


@pytest.mark.parametrize('n', [300, 301])
def test_chunk_seams_do_not_change_a_bit(n):
    with emu_backend.emulated():
        S.check_seams('cpu', n)


def test_a_natural_multi_chunk_shape():
    with emu_backend.emulated():
        S.check_natural_chunks('cpu')


@pytest.mark.parametrize('drop', [0, 1])
def test_inverse_with_none_highs(drop):
    with emu_backend.emulated():
        S.check_none_highs('cpu', drop)


@pytest.mark.parametrize('pair', S.FUSED_PAIRS)
def test_gradients_follow_the_reference_rule(pair):
    with emu_backend.emulated():
        for n, J in ((22, 3), (37, 4), (20, 2), (16, 1)):
            S.check_gradients('cpu', n, J, pair[0], pair[1], F32)
        S.check_gradients('cpu', 22, 3, pair[0], pair[1], F64)


@pytest.mark.parametrize('only', [0, 1, 3])
def test_gradient_of_a_single_output(only):
    with emu_backend.emulated():
        S.check_gradients('cpu', 22, 3, 'near_sym_a', 'qshift_a', F32, only=only)


def test_gradcheck_float64():
    with emu_backend.emulated():
        S.check_gradcheck('cpu')


@pytest.mark.parametrize('dtype', [F64, F32, F16, BF16])
def test_goldens(dtype):
    files = S.golden_files()
    assert files
    with emu_backend.emulated():
        for f in files:
            S.check_golden('cpu', f, dtype)


def test_views():
    with emu_backend.emulated():
        S.check_views('cpu')


def test_errors():
    with emu_backend.emulated():
        S.check_errors('cpu')
    S.check_cpu_tensor_raises()


def test_every_schedule_gives_the_same_bits():
    outs = []
    with emu_backend.emulated():
        for order, dma, seed in SCHEDULES:
            with emu_backend.schedule(order, dma, seed):
                r = S.run_both('cpu', 301, 3, 'near_sym_a', 'qshift_a', F32, (8, 64))
                outs.append([r[1]] + r[2] + [r[3], r[4]])
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
        S.check_seams('cpu', 301)


def test_chunk_policy_on_two_chip_sizes():
    """chunk = 0 on chips of 1 and of 64 compute units: the numbers are those of the default chip (and of the oracle:
    test_a_natural_multi_chunk_shape); a row of 9000 samples does not fit one chunk, so there is no one-chunk twin here."""
    with emu_backend.emulated():
        base = S.run_both('cpu', 9000, 3, 'near_sym_a', 'qshift_a', F32, (0, 0))
        for cus in (1, 64):
            with emu_backend.chip_of(cus):
                r = S.run_both('cpu', 9000, 3, 'near_sym_a', 'qshift_a', F32, (0, 0))
            for a, b in zip([r[1]] + r[2] + [r[3], r[4]], [base[1]] + base[2] + [base[3], base[4]]):
                assert torch.equal(a, b)
