// libwl_emu.so, unit 'api': the same kernel bodies and C ABI as the matching unit of libwavelets_hip.so, executed on the host.
#include "wl_backend_emu.h"
#include "../../pytorch_wavelets_amd/csrc/wl_api.inc"

// test hook (emulator only, not part of the C ABI): the size of the emulated chip, for launcher policies that depend on it
extern "C" void wl_emu_set_cus(int n) { wl_emu_cus_v = n > 0 ? n : 2; }
// test hook (emulator only): the scheduling choices of wl_backend_emu.h - order 0 alternate (default), 1 forward, 2 reverse,
// 3 shuffled (seeded); dma 0 late (default), 1 eager
extern "C" void wl_emu_set_schedule(int order, int dma, unsigned seed) {
    wl_emu_order_v = order >= 0 && order <= 3 ? order : 0;
    wl_emu_dma_v = dma == 1 ? 1 : 0;
    wl_emu_seed_v = seed;
}
// test hook (emulator only): the extension rule of the single-axis kernels (wl_filt1d.h), for lengths no test can allocate on the host
extern "C" int wl_emu_ext_any(int i, int n, int ext) { return wl_ext_any(i, n, ext); }
