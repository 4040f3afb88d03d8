"""Every transform on tensor views (offset bases, crops, odd pitches, slices) on the host emulation of the kernel sources:
the table and the checks of tests/_view_cases.py - outputs against the float64 oracle, no NaN from the padding, the parents
untouched, the kernel each row is about, and the dense route unchanged by the view call - on CPU tensors, float64 rows
included.  The emulator proves the index arithmetic of the alignment branches; tests/test_views_gpu.py proves the accesses."""
import pytest

import _view_cases as V
import emu_backend


def _run(fn, case):
    with emu_backend.emulated(), emu_backend.chip_of(case.cus):
        fn(case, 'cpu')


@pytest.mark.parametrize('name', [c.name for c in V.CASES])
def test_view(name):
    _run(V.check, V.BY_NAME[name])


@pytest.mark.parametrize('name', V.GRAD_CASES)
def test_view_backward(name):
    _run(V.check_grad, V.BY_NAME[name])
