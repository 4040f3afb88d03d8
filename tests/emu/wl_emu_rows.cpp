// libwl_emu.so, unit 'rows': the same kernel bodies and C ABI as the matching unit of libwavelets_hip.so, executed on the host.
#define WL_ROWS_UNIT_ANALYSIS 1   // (the synthesis half: wl_emu_irows.cpp)
#include "wl_backend_emu.h"
#include "../../pytorch_wavelets_amd/csrc/wl_rows_api.inc"

// test hook (emulator only): the LL ring slot of row r in a ring of `rows` rows, with the multiplier the launcher computes
extern "C" int wl_emu_ring_slot(int r, int rows) { return wl_ring_slot(r, rows, (unsigned)(0x100000000ull / (unsigned)rows)); }
