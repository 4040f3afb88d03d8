"""The kernels every 2-D DWT case takes on the host emulation - forward, inverse, one backward pass through both - against
tests/golden/dwt_routes.json, entry for entry (tools/record_dwt_routes.py wrote it): a change of the Python layer that is
meant to keep every route shows here when it does not."""
import pytest

import _route_cases as RC

BLOCKS = 16


def test_fixture_lists_the_cases():
    assert [e['case'] for e in RC.load()] == RC.CASES


@pytest.mark.parametrize('block', range(BLOCKS))
def test_dwt_routes_match_the_recorded_ones(block):
    golden = RC.load()
    for case, want in list(zip(RC.CASES, golden))[block::BLOCKS]:
        got, _ = RC.run_case(case)
        assert got == want, (case, got, want)
