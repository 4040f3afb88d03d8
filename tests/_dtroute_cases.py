"""Which kernels the DTCWT and the scattering layers take on the host emulation: the cases of tests/golden/dtcwt_routes.json,
shared by the tool that records the file (tools/record_dtcwt_routes.py) and the test that replays it
(tests/test_dtcwt_routes_emu.py).  The counterpart of tests/_route_cases.py for the other half of the C ABI.

A case is a module ('dtcwt': DTCWTForward + DTCWTInverse, 'scat': ScatLayer, 'scatj2': ScatLayerj2), a shape (N, C, H, W), a
dtype, an emulated chip (2 or 8 CUs) and optionally one engine option ('no_stream', 'generic_only', 'stream_force' =
ops.STREAM_FORCE).  It runs forward, inverse (the DTCWT) and - where the case asks for one - a backward pass; each step is
recorded as the list ``pw.kernels_since(count)`` of its launches, or as the type and message of the exception it raised."""
import json
import os

import numpy as np
import torch

import emu_backend
import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dtcwt_routes.json')
HISTORY = 32        # launches the engine remembers (pw.kernels_since)
STEPS = ('forward', 'inverse', 'backward')
# (planes, H, W) as (N, C, H, W): the sizes at which the emulator tests reach each kernel
ODD, SMALL, MID, NARROW, WIDE = [3, 1, 21, 27], [8, 2, 32, 32], [2, 2, 64, 96], [2, 1, 64, 160], [1, 2, 40, 512]
ODD_RGB = [1, 3, 21, 27]   # the same three planes as one colour image (combine_colour)
# the kernels the fixture has to go through to be worth replaying (WlDtFwd12Strip: <T, L0, L1, LQ, MODE, ...>)
FAMILIES = ('WlDtFwd1<', 'WlDtFwd1Tile<', 'WlDtFwd1Small<', 'WlDtFwd1Strip<', 'WlDtFwd12Strip<', 'WlDtFwd1Rot<', 'WlDtFwd2<',
            'WlDtFwd2Tile<', 'WlDtInv1<', 'WlDtInv1Tile<', 'WlDtInv1Strip<', 'WlDtInv2<', 'WlDtInv2Tile<', 'WlDtInv2Strip<',
            'WlDtInv21Strip<')
FUSED_MODES = (0, 1, 2, 3, 4, 5, 6)   # (2 = levels 1 + 2 in one launch, the default template argument)


def fused_mode(kernel):
    """MODE of a WlDtFwd12Strip<...> name, None for any other kernel."""
    if not kernel.startswith('WlDtFwd12Strip<'):
        return None
    args = kernel[kernel.index('<') + 1:kernel.rindex('>')].split(', ')
    return int(args[4]) if len(args) > 4 else 2


def _dt(shape, J, biort='near_sym_a', qshift='qshift_a', dtype='float32', cus=2, opt=None, **more):
    return dict(kind='dtcwt', shape=shape, dtype=dtype, cus=cus, opt=opt, J=J, biort=biort, qshift=qshift, mode='symmetric',
                skip_hps=False, no_lowpass=False, backward=True, **more)


def _scat(shape, biort='near_sym_a', dtype='float32', cus=2, opt=None, combine=False, backward=False, kind='scat'):
    return dict(kind=kind, shape=shape, dtype=dtype, cus=cus, opt=opt, biort=biort, combine=combine, backward=backward)


def _cases():
    dt = [
        _dt(ODD, 1), _dt(ODD, 3, 'near_sym_b', 'qshift_b', cus=8), _dt(ODD, 2, 'antonini', 'qshift_d', opt='generic_only'),
        _dt(ODD, 2, 'legall', dtype='float64'),
        _dt(SMALL, 1), _dt(SMALL, 2, 'near_sym_b', cus=8), _dt(SMALL, 2, opt='no_stream'),
        _dt(MID, 1), _dt(MID, 2, 'legall'), _dt(MID, 3, qshift='qshift_d', dtype='float16'), _dt(MID, 2, opt='stream_force'),
        _dt(NARROW, 1, 'near_sym_b'), _dt(NARROW, 2, 'antonini', 'qshift_b'), _dt(NARROW, 2, opt='stream_force'),
        _dt(NARROW, 3, dtype='bfloat16'),
        _dt(WIDE, 1), _dt(WIDE, 2), _dt(WIDE, 3, qshift='qshift_b'), _dt(WIDE, 2, 'antonini'), _dt(WIDE, 2, cus=8),
        _dt(WIDE, 2, opt='no_stream'), _dt(WIDE, 2, dtype='float16'), _dt(WIDE, 1, opt='generic_only'),
        _dt(WIDE, 2, 'legall', 'qshift_d'),
    ]
    dt[15]['mode'] = 'zero'                             # (the lean kernel mirrors: the column-strip kernel of level 1)
    dt.append(dict(_dt(NARROW, 3), skip_hps=[True, False, False]))
    dt.append(dict(_dt(WIDE, 2), no_lowpass=True))
    scat = [
        _scat(ODD), _scat(ODD_RGB, combine=True, backward=True), _scat(SMALL, backward=True),
        _scat(MID, 'near_sym_b', backward=True), _scat(MID, dtype='float16', backward=True), _scat(NARROW),
        _scat(WIDE, backward=True), _scat(WIDE, 'near_sym_b'), _scat(WIDE, 'near_sym_b_bp'),
        _scat(NARROW, 'near_sym_b_bp', backward=True), _scat(ODD_RGB, 'near_sym_b_bp', combine=True), _scat(WIDE, cus=8),
        _scat(WIDE, opt='generic_only', backward=True), _scat(WIDE, 'near_sym_b_bp', opt='no_stream'),
        _scat(SMALL, 'near_sym_b_bp'), _scat(ODD, 'near_sym_b_bp', dtype='float64'),
    ]
    j2 = [_scat(WIDE, kind='scatj2'), _scat(NARROW, kind='scatj2', backward=True), _scat(ODD, kind='scatj2', backward=True),
          _scat(WIDE, kind='scatj2', opt='no_stream')]
    return dt + scat + j2


CASES = _cases()


def _module_steps(case, x, tensors):
    """The steps of one case as (name, function) pairs; what they compute is appended to `tensors`."""
    dtype, state = x.dtype, {}
    if case['kind'] == 'dtcwt':
        xfm = pw.DTCWTForward(J=case['J'], biort=case['biort'], qshift=case['qshift'], skip_hps=case['skip_hps'],
                              mode=case['mode']).to(dtype)
        ifm = pw.DTCWTInverse(biort=case['biort'], qshift=case['qshift'], mode=case['mode']).to(dtype)

        def forward():
            state['yl'], state['yh'] = xfm(x)
            tensors.extend([state['yl']] + list(state['yh']))

        def inverse():
            state['rec'] = ifm((None if case['no_lowpass'] else state['yl'], state['yh']))
            tensors.append(state['rec'])

        def backward():
            loss = state['rec'].float().square().sum() + state['yl'].float().sum()
            for h in state['yh']:
                if h.numel():
                    loss = loss + h.float().sum()
            loss.backward()
            tensors.append(x.grad)
        return (('forward', forward), ('inverse', inverse), ('backward', backward))
    if case['kind'] == 'scat':
        layer = pw.ScatLayer(biort=case['biort'], combine_colour=case['combine']).to(dtype)
    else:
        layer = pw.ScatLayerj2(biort=case['biort'], combine_colour=case['combine']).to(dtype)

    def forward():
        with torch.set_grad_enabled(case['backward']):
            state['z'] = layer(x)
        tensors.append(state['z'])

    def backward():
        state['z'].float().square().sum().backward()
        tensors.append(x.grad)
    return (('forward', forward), ('backward', backward)) if case['backward'] else (('forward', forward),)


def run_case(case):
    """(entry, tensors): the routes of one case as they go into the file, and what it computed."""
    dtype = getattr(torch, case['dtype'])
    rng = np.random.RandomState(2000 + CASES.index(case))
    x = torch.tensor(rng.randn(*case['shape']), dtype=torch.float32).to(dtype).requires_grad_(case['backward'])
    entry, tensors = dict(case=case), []
    opt, force = case['opt'], ops.STREAM_FORCE
    ops._FUSED_DECLINED.clear()
    with emu_backend.emulated(), emu_backend.chip_of(case['cus']):
        try:
            if opt == 'stream_force':
                ops.STREAM_FORCE = True
            elif opt:
                ops.set_option(opt, 1)
            for name, step in _module_steps(case, x, tensors):
                c0 = pw.launch_count()
                try:
                    step()
                except Exception as e:      # noqa: BLE001 (the route of a case the engine refuses IS its exception)
                    entry[name] = {'error': [type(e).__name__, str(e)]}
                    break
                assert pw.launch_count() - c0 < HISTORY, (case, name)
                entry[name] = pw.kernels_since(c0)
        finally:
            ops.STREAM_FORCE = force
            if opt and opt != 'stream_force':
                ops.set_option(opt, 0)
    return entry, [t.detach() for t in tensors]


def load():
    with open(GOLDEN) as f:
        return json.load(f)
