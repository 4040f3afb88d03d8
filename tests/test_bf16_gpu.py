"""bfloat16 data through every transform on the MI355X (tests/_bf16_cases.py) at sizes that reach the streaming kernels:
the float16 kernels, forward and backward, against the float64 oracle; both ways of holding the taps; the rounding."""
import pytest
import torch

import _bf16_cases as B
from pytorch_wavelets_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CASES = [
    B.dwt('dwt_rows_128x3x512', (128, 3, 512, 512), 3, 'db4', 'symmetric', 'WlAfbRows'),
    B.dwt('dwt_per_2x16x2048', (2, 16, 2048, 2048), 4, 'db8', 'periodization', 'WlAfb'),
    B.dwt('dwt_small_64x64x32', (64, 64, 32, 32), 3, 'db4', 'symmetric', 'WlAfbSmall'),
    B.dwt1d('dwt1d_2x2x8192', (2, 2, 8192), 3, 'db4', 'symmetric', 'WlDwt1dFused'),
    B.swt('swt_db2_periodic', (4, 3, 256, 256), 2, 'db2', 'periodic', 'WlSwtLevel'),
    B.nonsep('nonsep', (4, 3, 128, 128), 'db2', 'zero', 'WlAfbNonsep'),
    B.dtcwt('dtcwt_a_64x3x512', (64, 3, 512, 512), 3, 'near_sym_a', 'qshift_a', 'WlDt'),
    B.dtcwt('dtcwt_b_64x3x512', (64, 3, 512, 512), 3, 'near_sym_b', 'qshift_b', 'WlDt'),
    B.dtcwt('dtcwt_bp', (16, 3, 256, 256), 2, 'near_sym_b_bp', 'qshift_b_bp', 'WlDt'),
    B.scat('scat_train_256x3x256', (256, 3, 256, 256), 'near_sym_a', 'WlDt'),
    B.scat('scat_infer_256x3x256', (256, 3, 256, 256), 'near_sym_a', 'WlDt', grad=False),
    B.scat('scat_bp_64x3x256', (64, 3, 256, 256), 'near_sym_b_bp', 'WlDt'),
    B.scatj2('scatj2_64x3x256', (64, 3, 256, 256), 'WlDt'),
    B.primitives('primitives', (4, 3, 128, 128), 'WlCorr1d'),
]


@pytest.mark.parametrize('rounded', [True, False], ids=['bf16_module', 'f32_module'])
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_bf16_takes_the_float16_kernels_gpu(case, rounded):
    B.check(case, DEV, rounded)


def test_bf16_stores_round_to_nearest_even_gpu():
    B.rounding_check(DEV)


def test_bf16_unsupported_dtypes_still_raise_gpu():
    import pytorch_wavelets_amd as pw
    m = pw.DWTForward(J=1).to(DEV)
    assert m(torch.randn(1, 1, 16, 16, device=DEV).to(torch.bfloat16))[0].dtype == torch.bfloat16
    for dt in (torch.int32, torch.complex64):
        with pytest.raises(TypeError, match='bfloat16'):
            m(torch.zeros(1, 1, 16, 16, dtype=dt, device=DEV))
    assert ops._backend().wl_version() == 220
