"""-m gpu: the 2-D wavelet packet transform on the MI355X - WPT2DForward / WPT2DInverse, their gradients, the function-level pair
and the packed-band kernels of csrc/wl_wpt2d.h through the C ABI, against the per-axis oracle (tests/_wpt2d_cases.py)."""
import numpy as np
import pytest
import torch

import _wpt2d_cases as S
import pytorch_wavelets_amd as pw

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32, F16, BF16 = S.F64, S.F32, S.F16, S.BF16


@pytest.mark.parametrize('mode', S.MODES)
def test_forward_values_and_layout(mode):
    for J in (1, 2, 3):
        S.check_forward(DEV, (2, 3, 20, 28), 'db2', J, mode)
        S.check_forward(DEV, (1, 2, 37, 141), 'db4', J, mode)
        S.check_forward(DEV, (1, 1, 5, 7), 'db4', J, mode)
        S.check_forward(DEV, (1, 2, 38, 150), 'db10', J, mode)


def test_band_table_subtrees_and_freq_order():
    for mode in ('symmetric', 'periodization'):
        S.check_band_table(DEV, (2, 3, 20, 28), 'db2', mode)
    S.check_freq_order(DEV)


def test_the_packet_kernels_ran_one_launch_per_level():
    S.check_kernels_ran(DEV, 'symmetric')


def test_float64_generic_only_and_declines_take_the_fallback():
    S.check_float64_generic(DEV)
    S.check_generic_only(DEV)
    S.check_declines(DEV)


def test_two_levels_per_launch_sequences_and_the_level_by_level_route():
    S.check_two_level_sequence(DEV)


@pytest.mark.parametrize('dtype', [F16, BF16])
def test_two_levels_per_launch_float16_and_bfloat16(dtype):
    S.check_two_level_low_precision(DEV, dtype)


@pytest.mark.parametrize('wave', ['db1', 'db2', 'db4', 'db6'])
def test_two_level_kernel_seams(wave):
    S.check_wrap_shapes(DEV, wave, (1, 2, 72, 200))
    S.check_wrap_shapes(DEV, wave, (2, 1, 8, 12), two_level=wave in ('db1', 'db2'))   # db4 / db6: level 2 shorter than the filter


def test_outside_the_two_level_envelope_single_level_launches_run():
    S.check_wrap_shapes(DEV, 'db4', (1, 2, 70, 200), two_level=False)                 # H % 4 != 0
    S.check_wrap_shapes(DEV, 'db7', (1, 2, 72, 200), two_level=False)                 # 14 taps
    S.check_wrap_shapes(DEV, 'db4', (1, 2, 72, 200), mode='symmetric', two_level=False)


@pytest.mark.parametrize('mode', S.MODES)
def test_inverse_and_reconstruction(mode):
    S.check_inverse(DEV, (1, 2, 37, 141), 'db4', mode, J=2)
    S.check_inverse(DEV, (1, 2, 37, 141), 'db4', mode, J=2, with_size=False)
    for wave in ('db2', 'db4', 'bior2.2'):
        S.check_roundtrip(DEV, (1, 2, 16, 24), wave, mode)
        S.check_roundtrip(DEV, (1, 1, 19, 23), wave, mode)


def test_inverse_rejects_a_wrong_size_and_band_count():
    S.check_inverse_errors(DEV)


@pytest.mark.parametrize('mode', S.MODES)
def test_gradients_follow_the_q9_rule(mode):
    S.check_gradients(DEV, (2, 1, 9, 13), 'db2', mode, J=2)
    S.check_gradients(DEV, (1, 2, 13, 9), 'db4', mode, J=2, dtype=F64)


def test_zero_mode_dot_product_identity():
    S.check_dot_product(DEV, (1, 2, 13, 9), 'db4')
    S.check_dot_product(DEV, (2, 1, 20, 28), 'db2')


@pytest.mark.parametrize('mode', ['symmetric', 'periodization'])
@pytest.mark.parametrize('dtype', [F16, BF16])
def test_float16_and_bfloat16(dtype, mode):
    S.check_low_precision(DEV, dtype, mode)


def test_views_equal_their_contiguous_twins():
    S.check_views(DEV)


def test_api():
    S.check_api(DEV)
    S.check_cpu_tensor_raises()


@pytest.mark.parametrize('mode', ['symmetric', 'periodization'])
def test_a_shape_that_fills_the_chip_and_crosses_both_walks(mode):
    """(8,4,96,96) float32 db4 J=3: level 1 has several tiles per plane (the wide walk).  In periodization level 3 works on 512
    planes of 24 x 24 -> 12 x 12 coefficients, two planes per workgroup (the plane-run walk); in symmetric mode its 18 x 18
    coefficients stay on the wide walk.  Forward, inverse and dx against the oracle on four (n, c) pairs.  Then 1024 planes of
    8 x 8, which take the plane-run walk from the first level on (symmetric; in periodization they are the two-level kernels'): forward,
    inverse and the gradients."""
    shape, wave, J = (8, 4, 96, 96), 'db4', 3
    xfm, ifm = S.modules(DEV, wave, J, mode)
    x = S.rand(shape, F32, DEV, 90).requires_grad_(True)
    c0 = pw.launch_count()
    y = xfm(x)
    two = mode == 'periodization'                          # (two levels per launch, then the third on its own)
    assert S.names(pw.kernels_since(c0)) == (['WlWptAfb<float, 8, 2>', 'WlWptAfb<float, 8, 1>'] if two else ['WlWptAfb<float, 8, 1>'] * J)
    c0 = pw.launch_count()
    rec = ifm(y, size=shape[2:])
    assert S.names(pw.kernels_since(c0)) == (['WlWptSfb<float, 8, 1>', 'WlWptSfb<float, 8, 2>'] if two else ['WlWptSfb<float, 8, 1>'] * J)
    cot = S.rand(tuple(y.shape), F32, DEV, 91)
    dx, = torch.autograd.grad(y, x, cot)
    h, g = S.taps(wave, f32=True), S.taps(wave, syn=True, f32=True)
    sizes = S.level_sizes(shape[2:], J, 8, mode)
    for n, c in ((0, 0), (3, 1), (7, 3), (5, 2)):
        sl = (slice(n, n + 1), slice(c, c + 1))
        ref = S.fwd_ref(S.npy(x[sl]), J, h, mode)
        S.close(y[sl], ref, F32, 'y (%d, %d)' % (n, c))
        S.close(rec[sl], S.inv_ref(ref, g, mode, sizes), F32, 'rec (%d, %d)' % (n, c))
        S.close(dx[sl], S.fwd_grad_ref(S.npy(cot[sl]), sizes, h, mode), F32, 'dx (%d, %d)' % (n, c))
    assert float(np.abs(S.npy(rec) - S.npy(x)).max()) <= 1e-5 * float(x.detach().abs().max())
    S.check_forward(DEV, (16, 64, 8, 8), 'db2', 2, mode)
    S.check_inverse(DEV, (16, 64, 8, 8), 'db2', mode, J=2)
    S.check_gradients(DEV, (16, 64, 8, 8), 'db2', mode, J=2)
