"""bfloat16 data through every transform on the HOST EMULATION of the kernels (tests/_bf16_cases.py): the float16 kernels,
forward and backward, against the float64 oracle; both ways of holding the taps; the rounding of the stores."""
import numpy as np
import pytest
import torch

import _bf16_cases as B
import _opts
import emu_backend
import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import ops


def _generic():
    import contextlib

    @contextlib.contextmanager
    def ctx():
        _opts.set_generic(1)
        try:
            yield
        finally:
            _opts.set_generic(0)
    return ctx()


def _no_stream():
    return B.option(b'no_stream')


CASES = [
    B.dwt('dwt_rows', (2, 3, 64, 128), 3, 'db4', 'symmetric', 'WlAfbRows'),
    B.dwt('dwt_rows_per', (2, 3, 64, 128), 3, 'db4', 'periodization', 'WlAfbRows', ctx=lambda: B._setattrs(ops, FUSED_STRIPS=1)),
    B.dwt('dwt_strip', (2, 2, 48, 1024), 3, 'db4', 'symmetric', 'WlAfbStrip', ctx=B.strips_force),
    B.dwt('dwt_small', (4, 6, 32, 32), 2, 'db2', 'symmetric', 'WlAfbSmall'),
    B.dwt('dwt_tile', (2, 3, 64, 96), 2, 'db4', 'symmetric', 'WlSfbTile', ctx=_no_stream),
    B.dwt('dwt_generic', (1, 2, 72, 136), 2, 'db3', 'reflect', 'WlSfb2dTile', ctx=_generic),
    B.dwt('dwt_lattice', (1, 1, 48, 2048), 1, 'db8', 'periodization', 'WlAfbStrip', ctx=B.lattice_force),
    B.dwt1d('dwt1d', (2, 2, 1024), 3, 'db4', 'symmetric', 'WlDwt1dFused'),
    B.swt('swt', (1, 2, 20, 24), 2, 'db2', 'periodic', 'WlSwtLevel'),
    B.nonsep('nonsep', (1, 2, 32, 32), 'db2', 'zero', 'WlAfbNonsep'),
    B.dtcwt('dtcwt_a', (1, 2, 64, 128), 2, 'near_sym_a', 'qshift_a', 'WlDt'),
    B.dtcwt('dtcwt_a_stream', (1, 2, 64, 128), 2, 'near_sym_a', 'qshift_a', 'WlDtFwd12Strip', ctx=B.stream_force),
    B.dtcwt('dtcwt_b', (1, 2, 64, 128), 2, 'near_sym_b', 'qshift_b', 'WlDt', ctx=B.stream_force),
    B.dtcwt('dtcwt_d', (1, 2, 64, 128), 2, 'near_sym_a', 'qshift_d', 'WlDt'),
    B.dtcwt('dtcwt_bp', (1, 2, 64, 128), 2, 'near_sym_b_bp', 'qshift_b_bp', 'WlDt'),
    B.scat('scat_train', (2, 3, 64, 64), 'near_sym_a', 'WlDt'),
    B.scat('scat_infer', (2, 3, 64, 64), 'near_sym_a', 'WlDt', grad=False),
    B.scat('scat_bp', (2, 3, 64, 64), 'near_sym_b_bp', 'WlDt'),
    B.scatj2('scatj2', (1, 3, 64, 64), 'WlDt'),
    B.primitives('primitives', (1, 2, 32, 32), 'WlCorr1d'),
]


@pytest.mark.parametrize('rounded', [True, False], ids=['bf16_module', 'f32_module'])
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_bf16_takes_the_float16_kernels(case, rounded):
    with emu_backend.emulated():
        B.check(case, 'cpu', rounded)


def test_bf16_stores_round_to_nearest_even():
    with emu_backend.emulated():
        B.rounding_check('cpu')


def test_bf16_dtype_code_and_other_dtypes_still_raise():
    h = emu_backend.handle()
    assert ops._DTYPES[torch.bfloat16] == 3
    with emu_backend.emulated():
        assert pw.DWTForward(J=1)(torch.randn(1, 1, 16, 16).to(torch.bfloat16))[0].dtype == torch.bfloat16
        for dt in (torch.int32, torch.complex64):
            with pytest.raises(TypeError, match='bfloat16'):
                pw.DWTForward(J=1)(torch.zeros(1, 1, 16, 16, dtype=dt))
    # the C ABI: a dtype code it does not know is refused
    x = torch.zeros(1, 1, 8, 8)
    y = torch.zeros(1, 1, 4, 4)
    t = torch.tensor([0.5, 0.5])
    hs = torch.zeros(1, 1, 3, 4, 4)
    rc = h.wl_dwt2d_analysis(x.data_ptr(), y.data_ptr(), hs.data_ptr(), 4, 1, 8, 8, t.data_ptr(), t.data_ptr(), 2,
                             t.data_ptr(), t.data_ptr(), 2, 0, None)
    assert rc == -4
    assert h.wl_version() == 220
    np.testing.assert_equal(B.rnd([1.0 + 2 ** -9]), [1.0])   # (ties to even)
