"""The kernels every DTCWT / ScatLayer / ScatLayerj2 case takes on the host emulation - forward, inverse, backward - against
tests/golden/dtcwt_routes.json, entry for entry (tools/record_dtcwt_routes.py wrote it): a change of the launchers that is
meant to keep every route shows here when it does not."""
import pytest

import _dtroute_cases as RC

BLOCKS = 8


def test_fixture_lists_the_cases():
    assert [e['case'] for e in RC.load()] == RC.CASES


@pytest.mark.parametrize('block', range(BLOCKS))
def test_dtcwt_routes_match_the_recorded_ones(block):
    golden = RC.load()
    for case, want in list(zip(RC.CASES, golden))[block::BLOCKS]:
        got, _ = RC.run_case(case)
        assert got == want, (case, got, want)
