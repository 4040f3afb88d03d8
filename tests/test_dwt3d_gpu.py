"""-m gpu: the 3-D DWT on the MI355X - DWT3DForward / DWT3DInverse, their gradients, ops.afb_depth / ops.sfb_depth and the
streaming depth kernels of csrc/wl_dwt3d.h through the C ABI, against the per-axis oracle (tests/_dwt3d_cases.py)."""
import numpy as np
import pytest
import torch

import _dwt3d_cases as S
import pytorch_wavelets_amd as pw

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32, F16, BF16 = S.F64, S.F32, S.F16, S.BF16


@pytest.mark.parametrize('mode', S.MODES)
def test_forward_values_and_layout(mode):
    S.check_forward(DEV, (2, 3, 10, 12, 16), 'db2', 1, mode)
    S.check_forward(DEV, (2, 1, 7, 9, 11), 'db4', 2, mode)
    if mode in ('symmetric', 'reflect'):
        S.check_forward(DEV, (1, 1, 3, 20, 24), 'bior2.2', 1, mode)
    S.check_band_table(DEV, (2, 3, 10, 12, 16), 'db2', mode)


def test_the_depth_kernels_ran_and_float64_takes_the_generic_ones():
    S.check_kernels_ran(DEV)


@pytest.mark.parametrize('mode', S.MODES)
def test_chunk_seams_do_not_change_a_bit(mode):
    for wave in ('db4', 'db10'):
        for n in (22, 23):
            S.check_chunks(DEV, n, wave, mode)


@pytest.mark.parametrize('dtype', [F32, F16, BF16])
def test_vector_and_scalar_bodies(dtype):
    S.check_vec_bodies(DEV, dtype)


@pytest.mark.parametrize('mode', S.MODES)
def test_inverse_and_reconstruction(mode):
    S.check_inverse(DEV, (2, 1, 7, 9, 11), 'db4', mode, J=2)
    S.check_inverse(DEV, (1, 2, 7, 9, 11), 'db2', mode, J=2, drop=0)
    S.check_inverse(DEV, (1, 2, 7, 9, 11), 'db2', mode, J=2, drop=1)
    for wave in ('db2', 'db4', 'bior2.2'):
        S.check_roundtrip(DEV, (1, 2, 8, 12, 16), wave, mode)
        S.check_roundtrip(DEV, (1, 1, 9, 11, 13), wave, mode)


@pytest.mark.parametrize('mode', S.MODES)
def test_gradients_follow_the_q9_rule(mode):
    S.check_gradients(DEV, (2, 1, 7, 9, 11), 'db2', mode, J=2)
    S.check_gradients(DEV, (1, 2, 9, 7, 13), 'db4', mode, J=2, dtype=F64)


def test_zero_mode_dot_product_identity():
    S.check_dot_product(DEV, (1, 2, 7, 9, 11), 'db4')
    S.check_dot_product(DEV, (2, 1, 10, 12, 16), 'db2')


@pytest.mark.parametrize('dtype', [F16, BF16])
def test_float16_and_bfloat16(dtype):
    S.check_low_precision(DEV, dtype)


def test_views_equal_their_contiguous_twins():
    S.check_views(DEV)


def test_api():
    S.check_api(DEV)
    S.check_cpu_tensor_raises()


def test_a_shape_that_fills_the_chip_and_crosses_the_chunk_policy():
    """(4,2,32,96,96) float32 db4 symmetric J=2: level 1 has enough workgroups without a cut, level 2 (8 planes of 22 x 54 x 54)
    is cut along the depth by the policy; forward, inverse and dx against the oracle on a handful of (n, c) pairs."""
    shape, wave, mode, J = (4, 2, 32, 96, 96), 'db4', 'symmetric', 2
    xfm, ifm = S.modules(DEV, wave, J, mode)
    x = S.rand(shape, F32, DEV, 90).requires_grad_(True)
    c0 = pw.launch_count()
    yl, yh = xfm(x)
    ks = S.names(pw.kernels_since(c0))
    assert S.depth(ks) == ['WlAfbDepth'] * 2, ks
    c0 = pw.launch_count()
    rec = ifm((yl, yh))
    assert S.depth(S.names(pw.kernels_since(c0))) == ['WlSfbDepth'] * 2
    cots = [S.rand(tuple(t.shape), F32, DEV, 91 + i) for i, t in enumerate([yl] + yh)]
    dx, = torch.autograd.grad([yl] + yh, x, cots)
    hb, gb = S.banks(wave, f32=True), S.banks(wave, syn=True, f32=True)
    in_shapes = [shape[2:], tuple(yh[0].shape[3:])]
    for n, c in ((0, 0), (1, 1), (3, 0), (2, 1)):
        sl = (slice(n, n + 1), slice(c, c + 1))
        rl, rh = S.fwd_ref(S.npy(x[sl]), J, hb, mode)
        S.close(yl[sl], rl, F32, 'yl (%d, %d)' % (n, c))
        for j in range(J):
            S.close(yh[j][sl], rh[j], F32, 'yh[%d] (%d, %d)' % (j, n, c))
        S.close(rec[sl], S.inv_ref(rl, rh, gb, mode), F32, 'rec (%d, %d)' % (n, c))
        ref = S.fwd_grad_ref(S.npy(cots[0][sl]), [S.npy(t[sl]) for t in cots[1:]], in_shapes, hb, mode)
        S.close(dx[sl], ref, F32, 'dx (%d, %d)' % (n, c))
    assert float(np.abs(S.npy(rec) - S.npy(x)).max()) <= 1e-5 * float(x.detach().abs().max())
