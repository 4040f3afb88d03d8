"""Every kernel family on tensors past 4 GiB / 2**31 elements, on the real chip: the rows (part A: many planes) and the objects at
the top of the launchers' envelopes (part B) of tests/_large_cases.py at their real sizes.  Every case synchronises directly after
the engine call, compares every element of every output with the float64 oracle on the device, asserts the kernels it is about and
prints its shapes, bytes, launches, errors against bounds and seconds: run with -s, the log is the evidence.

On a shared machine run one family per invocation (-k <family>-), with -x -s, each under its own time limit, chained with &&."""
import pytest

import _large_cases as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('name', ['%s-%s' % (r.family, r.name) for r in L.ROWS])
def test_many_planes(name):
    L.run_row(L.BY_NAME[name.split('-', 1)[1]], DEV)


@pytest.mark.parametrize('name', ['%s-%s' % (e.family, e.name) for e in L.EDGES])
def test_envelope(name):
    L.run_edge(L.EDGE_BY_NAME[name.split('-', 1)[1]], DEV)
