"""CPU tests (host emulation of the kernels): every instantiation the dispatchers of the depth kernels (csrc/wl_dwt3d.h) and of
the packet kernels (csrc/wl_wpt2d.h) compile - tap counts 2 .. 20 (the two-level packet kernels: 2 .. 12) x float32, float16,
bfloat16, the depth kernels also per body width - against the per-axis oracle, with the kernel names built from (T, L, VEC /
NLEV) (tests/_dwt3d_cases.py, tests/_wpt2d_cases.py); and the same grid
of the 1-D kernels: the fused DWT pair (csrc/wl_dwt1d_fused.h, wl_idwt1d_fused.h; tests/_dwt1d_grid_cases.py) and the stationary
wave-tile pair (csrc/wl_swt1d.h; tests/_swt1d_cases.py), names built from (T, L).  One pytest item per (tap count, element type)."""
import pytest

import _dwt1d_grid_cases as W1
import _dwt3d_cases as V
import _swt1d_cases as S1
import _wpt2d_cases as P
import emu_backend

IDS = dict(ids=lambda v: v if isinstance(v, str) else str(v).replace('torch.', ''))


@pytest.mark.parametrize('dtype', V.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', V.GRID_WAVES)
def test_depth_kernels_every_tap_count_type_and_body(wave, dtype):
    with emu_backend.emulated():
        V.check_depth_instantiation('cpu', wave, dtype)


@pytest.mark.parametrize('dtype', V.GRID_DTYPES[1:], **IDS)
@pytest.mark.parametrize('wave', V.GRID_WAVES)
def test_depth_kernels_in_the_modules_float16_and_bfloat16(wave, dtype):
    with emu_backend.emulated():
        V.check_module_instantiation('cpu', wave, dtype)


@pytest.mark.parametrize('dtype', P.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', P.GRID_WAVES)
def test_one_level_packet_kernels_wide_walk(wave, dtype):
    with emu_backend.emulated():
        P.check_wide_instantiation('cpu', wave, dtype)


@pytest.mark.parametrize('dtype', P.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', P.GRID_WAVES)
def test_one_level_packet_kernels_plane_run_walk(wave, dtype):
    """(2, 4, 8, 8): the fewest planes for which the launcher keeps several planes per workgroup on the emulator's two compute units."""
    with emu_backend.emulated():
        P.check_plane_run_instantiation('cpu', wave, dtype, (2, 4, 8, 8))


@pytest.mark.parametrize('dtype', P.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', P.GRID_WAVES2)
def test_two_level_packet_kernels(wave, dtype):
    with emu_backend.emulated():
        P.check_two_level_instantiation('cpu', wave, dtype)


@pytest.mark.parametrize('dtype', W1.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', W1.GRID_WAVES)
def test_fused_dwt1d_kernels_every_tap_count_and_type(wave, dtype):
    """WlDwt1dFused / WlIdwt1dFused: two analysis and three synthesis chunks (J = 4, symmetric, odd length), one wrapped chunk
    (J = 2, periodization); forward, reconstruction and dx against the oracle."""
    with emu_backend.emulated():
        W1.check_instantiation('cpu', wave, dtype)


@pytest.mark.parametrize('dtype', S1.GRID_DTYPES, **IDS)
@pytest.mark.parametrize('wave', S1.GRID_WAVES)
def test_swt1d_wave_tile_kernels_every_tap_count_and_type(wave, dtype):
    """WlSwt1dFwd / WlSwt1dAdj: one to three levels per launch, one tile plus one position."""
    with emu_backend.emulated():
        S1.check_instantiation('cpu', wave, dtype)
