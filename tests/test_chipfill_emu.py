"""CPU tests (host emulation of the kernels): the work-sharing walks the launchers take once a launch fills the chip
(tests/_chipfill_cases.py) - several consecutive chunks per workgroup of WlDwt1dFused, several groups per workgroup of
WlAfbSmall, runs of planes per workgroup of WlDtFwd1Small - on emulated chips of 2, 8 and 256 compute units."""
import pytest

import _chipfill_cases as C
import emu_backend

CUS = (2, 8, 256)


@pytest.mark.parametrize('cus', CUS)
@pytest.mark.parametrize('case', sorted(C.DWT1D_CASES))
def test_dwt1d_fused_consecutive_chunks_per_workgroup(case, cus):
    with emu_backend.emulated(), emu_backend.chip_of(cus):
        C.check_dwt1d_walk('cpu', cus, **C.DWT1D_CASES[case])


@pytest.mark.parametrize('cus', CUS)
@pytest.mark.parametrize('case', sorted(C.AFB_SMALL_CASES))
def test_small_plane_analysis_walks_over_groups(case, cus):
    with emu_backend.emulated(), emu_backend.chip_of(cus):
        C.check_afb_small_walk('cpu', cus, **C.AFB_SMALL_CASES[case])


@pytest.mark.parametrize('cus', CUS)
@pytest.mark.parametrize('case', sorted(C.DT_SMALL_CASES))
def test_small_plane_dtcwt_runs_of_planes(case, cus):
    with emu_backend.emulated(), emu_backend.chip_of(cus):
        C.check_dt_small_runs('cpu', cus, **C.DT_SMALL_CASES[case])
