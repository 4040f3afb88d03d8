"""Test-only: load the HOST EMULATION build of the kernel sources (tests/emu/libwl_emu.so) and
install it as the ops backend, so the Python layer and the kernels' index arithmetic can be
exercised in the GPU-less container.  Never used by the product or by the -m gpu tests."""
import contextlib
import ctypes
import os
import subprocess

from pytorch_wavelets_amd import _capi, ops

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emu')
_SO = os.path.join(_DIR, 'libwl_emu.so')
_H = None


def handle():
    global _H
    if _H is None:
        srcs = [os.path.join(_DIR, f) for f in os.listdir(_DIR) if f.endswith(('.cpp', '.h', '.sh'))]
        csrc = os.path.join(os.path.dirname(_DIR), '..', 'pytorch_wavelets_amd', 'csrc')
        srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.h', '.inc'))]
        if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
            subprocess.check_call([os.path.join(_DIR, 'build.sh')])
        _H = _capi.bind(ctypes.CDLL(_SO))
        assert _H.wl_backend() == b'emu'
    return _H


@contextlib.contextmanager
def emulated():
    prev = ops._TEST_BACKEND
    ops._TEST_BACKEND = handle()
    try:
        yield
    finally:
        ops._TEST_BACKEND = prev


@contextlib.contextmanager
def chip_of(cus):
    """The emulated chip with `cus` compute units (default 2) - for launcher policies that depend on the chip's size."""
    handle()
    lib = ctypes.CDLL(_SO)
    lib.wl_emu_set_cus(int(cus))
    try:
        yield
    finally:
        lib.wl_emu_set_cus(2)


ORDERS = {'alternate': 0, 'forward': 1, 'reverse': 2, 'shuffled': 3}
DMA_MODES = {'late': 0, 'eager': 1}


@contextlib.contextmanager
def schedule(order, dma='late', seed=0):
    """The emulator's scheduling choices (tests/emu/wl_backend_emu.h): the visiting order of the fibres in a barrier phase
    ('alternate' - the default -, 'forward', 'reverse', 'shuffled' by `seed`) and when an LDS-DMA copy lands ('late' - the
    default: at the wl_wait_vm that releases it -, 'eager': as soon as its wave has issued it).  Restores the defaults."""
    handle()
    lib = ctypes.CDLL(_SO)
    lib.wl_emu_set_schedule(ORDERS[order], DMA_MODES[dma], ctypes.c_uint(seed & 0xffffffff))
    try:
        yield
    finally:
        lib.wl_emu_set_schedule(0, 0, ctypes.c_uint(0))


def ring_slot_fn():
    """slot(r, rows): the LL ring slot of row r in a ring of `rows` rows, as the exactly-sized (NP2) rings of WlAfbRows compute it."""
    handle()
    f = ctypes.CDLL(_SO).wl_emu_ring_slot
    f.argtypes, f.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_int
    return f


def ext_any_fn():
    """ext(i, n, rule): the source position of extended position i of an n-sample axis, as the single-axis kernels compute it."""
    handle()
    f = ctypes.CDLL(_SO).wl_emu_ext_any
    f.argtypes, f.restype = [ctypes.c_int, ctypes.c_int, ctypes.c_int], ctypes.c_int
    return f
