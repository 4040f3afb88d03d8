"""What the 2-D DWT's dispatcher asks the engine for - every launcher of every ladder, with its sizes, pitches and policy
words, on chips of 2, 8 and 256 CUs and at the benchmark's own shapes - against tests/golden/dwt_asks.json, entry for entry
(tools/record_dwt_asks.py wrote it): a change of the Python layer that is meant to keep the policy shows here when it does
not.  No kernel runs and no tensor is read (tests/_ask_cases.py): neither a GPU nor the emulator library is needed."""
import pytest

import _ask_cases as AC

BLOCKS = 8


def test_fixture_lists_the_cases():
    assert [e['case'] for e in AC.load()] == AC.CASES


@pytest.mark.parametrize('block', range(BLOCKS))
def test_dwt_asks_match_the_recorded_ones(block):
    golden = AC.load()
    for case, want in list(zip(AC.CASES, golden))[block::BLOCKS]:
        got = AC.run_case(case)
        assert got == want, (case, got, want)
