"""-m gpu: the work-sharing walks the launchers take once a launch fills the chip (tests/_chipfill_cases.py), on the MI355X -
the row and plane counts derived from the device's CU count, the launch's grid asserted as the witness of the walk.
Log: profiles/chipfill_gpu_tests.txt."""
import pytest
import torch

import _chipfill_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


@pytest.mark.parametrize('case', sorted(C.DWT1D_CASES))
def test_dwt1d_fused_consecutive_chunks_per_workgroup(case):
    C.check_dwt1d_walk(DEV, cus(), **C.DWT1D_CASES[case])


@pytest.mark.parametrize('case', sorted(C.AFB_SMALL_CASES))
def test_small_plane_analysis_walks_over_groups(case):
    C.check_afb_small_walk(DEV, cus(), **C.AFB_SMALL_CASES[case])


@pytest.mark.parametrize('case', sorted(C.DT_SMALL_CASES))
def test_small_plane_dtcwt_runs_of_planes(case):
    C.check_dt_small_runs(DEV, cus(), **C.DT_SMALL_CASES[case])
