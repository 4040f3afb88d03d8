"""Every transform on tensor views (offset bases, crops, odd pitches, slices) on the real chip: the table and the checks of
tests/_view_cases.py on cuda:0 (no float64 rows).  Each case prints its launches, its largest error and its bound: run with
-s, the log is the evidence that every row took the kernel it is about."""
import pytest

import _view_cases as V

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', [c.name for c in V.CASES if c.only != 'emu'])
def test_view(name):
    V.check(V.BY_NAME[name], DEV)


@pytest.mark.parametrize('name', V.GRAD_CASES)
def test_view_backward(name):
    V.check_grad(V.BY_NAME[name], DEV)
