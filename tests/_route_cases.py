"""Which kernels a 2-D DWT takes on the host emulation: the cases of tests/golden/dwt_routes.json, shared by the tool that
records the file (tools/record_dwt_routes.py) and the test that replays it (tests/test_dwt_routes_emu.py).

A case is DWTForward, DWTInverse and one ``.backward()`` through both; each step is recorded as the list
``pw.kernels_since(count)`` of its launches, or as the type and message of the exception it raised.  The grid is wavelets x
modes x J x shapes on emulated chips of 2 and 8 CUs; every seventh point of it is a case, in a quarter of the cases one level
of the pyramid is replaced by ``None`` before the inverse."""
import itertools
import json
import os

import numpy as np
import torch

import emu_backend
import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dwt_routes.json')
WAVES = ('haar', 'db2', 'db4', 'db5', 'db7', 'bior2.2')
MODES = ('zero', 'symmetric', 'periodization', 'periodic')
LEVELS = (1, 2, 3, 4, 5)
SHAPES = ((3, 20, 24), (9, 70, 66), (5, 96, 132), (7, 100, 200), (2, 40, 704), (2, 38, 1028), (12, 96, 80))   # (planes, H, W)
CHIPS = (2, 8)
STRIDE = 7
FAMILIES = ('WlAfbSmall', 'WlSfbSmall', 'WlAfbRows', 'WlSfbRows', 'WlAfbStrip', 'WlSfbStrip', 'WlAfbTile', 'WlSfbTile',
            'WlAfbDirect', 'WlSfbDirect', 'WlTapPrep')
HISTORY = 32        # launches the engine remembers (pw.kernels_since)


def _cases():
    out = []
    # (seven shapes, the slowest index: a stride of seven visits every shape, mode, wavelet and level count)
    grid = list(itertools.product(SHAPES, MODES, WAVES, LEVELS))[::STRIDE]
    for cus in CHIPS:
        for k, ((planes, H, W), mode, wave, J) in enumerate(grid):
            if mode == 'periodization':
                H, W = H + H % 2, W + (-W) % 4
            none_level = (k // 4) % 3 % J if k % 4 == 3 else None
            out.append(dict(wave=wave, mode=mode, J=J, shape=[planes, H, W], cus=cus, dtype='float32', none_level=none_level))
    # float16 data: the fused synthesis takes up to ops.IROWS_F16_MAXL taps
    for wave in ('db2', 'db5'):
        out.append(dict(wave=wave, mode='symmetric', J=3, shape=[5, 96, 132], cus=2, dtype='float16', none_level=None))
    return out


CASES = _cases()


def run_case(case):
    """(entry, tensors): the routes of one case as they go into the file, and what it computed (yl, yh.., rec, x.grad)."""
    planes, H, W = case['shape']
    dtype = getattr(torch, case['dtype'])
    rng = np.random.RandomState(1000 + CASES.index(case))
    x = torch.tensor(rng.randn(planes, 1, H, W), dtype=torch.float32).to(dtype).requires_grad_(True)
    xfm = pw.DWTForward(J=case['J'], wave=case['wave'], mode=case['mode'])
    ifm = pw.DWTInverse(wave=case['wave'], mode=case['mode'])
    entry, tensors, state = dict(case=case), [], {}

    def forward():
        state['yl'], state['yh'] = xfm(x)
        tensors.extend([state['yl']] + state['yh'])

    def inverse():
        yh = list(state['yh'])
        if case['none_level'] is not None:
            yh[case['none_level']] = None
        state['rec'] = ifm((state['yl'], yh))
        tensors.append(state['rec'])

    def backward():
        (state['rec'].float().square().sum() + state['yh'][0].float().sum()).backward()
        tensors.append(x.grad)

    ops._FUSED_DECLINED.clear()
    with emu_backend.emulated(), emu_backend.chip_of(case['cus']):
        for name, step in (('forward', forward), ('inverse', inverse), ('backward', backward)):
            c0 = pw.launch_count()
            try:
                step()
            except Exception as e:      # noqa: BLE001 (the route of a malformed pyramid IS its exception)
                entry[name] = {'error': [type(e).__name__, str(e)]}
                break
            assert pw.launch_count() - c0 < HISTORY, (case, name)
            entry[name] = pw.kernels_since(c0)
    return entry, [t.detach() for t in tensors]


def load():
    with open(GOLDEN) as f:
        return json.load(f)
