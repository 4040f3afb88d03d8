"""What the Python dispatcher of the 2-D DWT ASKS the engine for, at the sizes the product runs: the cases of
tests/golden/dwt_asks.json, shared by the tool that records the file (tools/record_dwt_asks.py) and the test that replays it
(tests/test_dwt_asks.py).  tests/_route_cases.py pins which kernels RUN on the host emulation, which reaches chips of 2 and 8
CUs and planes of a few thousand pixels; the thresholds the benchmark's routes hang on (a 256-CU chip, 40 M elements, rows of
2 KiB) flip far above that.  Here no kernel runs: a recording stub stands in for the engine (``ops._TEST_BACKEND``), the chip's
size is a patched ``ops._num_cus``, and the tensors are ``torch.empty`` on the CPU, which nobody reads - a 400 MB transform
costs milliseconds.

An ask is ``[name, arguments...]`` of one ``wl_*`` call with the sizes, strides, pitches, tap counts, mode and the `strips` /
`policy` bit words (every ``c_int``, ``c_int64`` and ``double`` of ``_capi.PROTOTYPES``); pointers are dropped, except that a
NULL one is kept as ``null`` - the lattice scratch of the *_ex launchers and the high-pass of a ``None`` level are policy too.

A launcher may decline, and the dispatcher then asks the next one: to list such a ladder whole, every step of a case runs with
"decline the first k asks, accept the rest" for k = 0, 1, 2, ... until the sequence of asks stops growing or the run raises
(the last rung cannot decline).  The record of a step is the list of these sequences; the first is the route on an engine
that takes everything."""
import contextlib
import ctypes
import json
import os

import torch

import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import _capi, _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dwt_asks.json')
STEPS = ('forward', 'inverse', 'backward')
MAX_DECLINES = 64       # (no ladder is this long: a guard against a dispatcher that asks forever)
_SCALARS = (_capi.I, _capi.L, ctypes.c_double)
WRAPPERS = ('wl_dwt2d_analysis_small', 'wl_dwt2d_synthesis_small', 'wl_dwt2d_analysis_fused_ex', 'wl_dwt2d_synthesis_fused_ex',
            'wl_dwt2d_analysis_stream_ex', 'wl_dwt2d_synthesis_stream_ex', 'wl_dwt2d_analysis_strided', 'wl_dwt2d_synthesis')


class Recorder(object):
    """The stub backend: records every ``wl_*`` call, declines the first `declines` of them, accepts the rest."""

    def __init__(self, declines=0):
        self.declines = declines
        self.asks = []

    def wl_get_option(self, name):
        return 0

    def __getattr__(self, name):
        if name not in _capi.PROTOTYPES:
            raise AttributeError(name)
        kinds = _capi.PROTOTYPES[name][1]

        def call(*args):
            assert len(args) == len(kinds), (name, len(args), len(kinds))
            ask = [name]
            for kind, a in zip(kinds, args):
                if kind in _SCALARS:
                    ask.append(a)
                elif a is None:
                    ask.append(None)
            self.asks.append(ask)
            return _lib.WL_ERR_UNSUPPORTED if len(self.asks) <= self.declines else 0
        return call


@contextlib.contextmanager
def _installed(backend, case):
    prev = ops._TEST_BACKEND, ops._num_cus, ops.STREAM_FORCE
    threads = torch.get_num_threads()
    ops._TEST_BACKEND, ops._num_cus, ops.STREAM_FORCE = backend, (lambda device: case['cus']), bool(case.get('stream_force'))
    torch.set_num_threads(1)    # (the one large operation left is autograd's sum of the two gradients of yh[0]: no thread pool for it)
    try:
        yield
    finally:
        ops._TEST_BACKEND, ops._num_cus, ops.STREAM_FORCE = prev
        torch.set_num_threads(threads)


def _case(wave, mode, J, shape, cus=2, dtype='float32', steps=STEPS, **opts):
    """wave / mode / J of DWTForward + DWTInverse, shape = (N, C, H, W), cus = the chip.  opts: none_level (that level of the
    pyramid is ``None`` at the inverse), half_module (``.half()`` modules, as the float16 workload of bench.py has them),
    stream_force (``ops.STREAM_FORCE``, which tests set to reach the strip kernels at any width)."""
    assert not set(opts) - {'none_level', 'half_module', 'stream_force'}, opts
    return dict(wave=wave, mode=mode, J=J, shape=list(shape), cus=cus, dtype=dtype, steps=list(steps), **opts)


def _cases():
    out = []
    add = lambda *a, **k: out.append(_case(*a, **k))   # noqa: E731
    FWD, INV, FI = ('forward',), ('inverse',), ('forward', 'inverse')

    # ---- the workloads: bench.py's three DWT configurations and its two feature-map shapes
    for cus in (256, 8, 2):
        add('db4', 'symmetric', 3, (128, 3, 512, 512), cus, steps=STEPS if cus == 256 else FI)
    add('db4', 'symmetric', 3, (48, 3, 512, 512), 256)                        # 37.7 M elements: below LATTICE_MIN_ELEMS
    add('db8', 'periodization', 4, (16, 6, 2048, 2048), 256, 'float16', FWD, half_module=True)   # 8 * 96 planes = 3 * 256 CUs
    add('db2', 'symmetric', 2, (512, 16, 32, 32), 256)
    add('haar', 'zero', 1, (64, 64, 112, 112), 256)

    # ---- afb2d_fused
    # the planes against the chip: 8 * N * C against 3 * cus
    for cus, planes in ((256, 95), (256, 96), (8, 2), (8, 3)):
        add('db4', 'symmetric', 1, (planes, 1, 96, 96), cus, steps=FI)
    # 8 / 12 / 14 taps with the hints (orthogonal) and without (biorthogonal): L > 12 wants the lattice, the lattice wants the hints
    for wave in ('db4', 'db6', 'db7', 'bior3.3', 'bior3.5', 'bior2.6'):
        add(wave, 'symmetric', 2, (3, 1, 96, 96), steps=FI)
    # numel against LATTICE_MIN_ELEMS at 8 and 12 taps (160 x 500 x 500 = 40 M exactly), 10 taps for the analysis' own lower bound
    for wave in ('db4', 'db5', 'db6'):
        for planes in (159, 160):
            add(wave, 'symmetric', 1, (planes, 1, 500, 500), 256, steps=FWD)
    # periodization with 12 taps takes the lattice whatever the size; 10 taps do not
    for wave in ('db5', 'db6'):
        add(wave, 'periodization', 1, (3, 1, 96, 96), steps=FI)
    # float16 periodization at 8 / 12 / 16 taps: the odd-cell tap counts of the long filters stay with the strip kernels
    for wave in ('db4', 'db6', 'db8'):
        add(wave, 'periodization', 2, (3, 1, 96, 96), dtype='float16', steps=FI)
    # rows of 2044 / 2048 / 3072 / 3076 bytes (and 2032: the widest whole 16-byte pieces under 2 KiB), one level and two, as the
    # whole transform (J = 1, 2) and inside a longer one (the n = 2, 1 rungs of J = 2; J = 4)
    for W in (508, 511, 512, 768, 769):
        for J in (1, 2):
            add('db2', 'symmetric', J, (1, 1, 24, W), steps=STEPS if (W, J) == (512, 2) else FWD)
    for W in (512, 768):
        add('db2', 'symmetric', 4, (1, 1, 24, W), steps=FWD)
    add('db2', 'symmetric', 2, (2, 1, 16, 1024), dtype='float16', steps=FWD)      # 2 KiB rows of float16
    # rows that are no whole 16-byte pieces; 132 columns leave a 67-column ll, which the strip kernel writes at a padded pitch
    add('db2', 'symmetric', 2, (1, 1, 48, 130), steps=FWD)
    add('db2', 'symmetric', 2, (1, 1, 48, 132), steps=FWD)
    # 20 taps: the banks of a .half() module are no orthogonal pair to the lattice's tolerance
    add('db10', 'symmetric', 2, (3, 1, 96, 96), dtype='float16', steps=FI, half_module=True)
    add('db10', 'symmetric', 2, (3, 1, 96, 96), dtype='float16', steps=FI)
    add('db10', 'symmetric', 2, (3, 1, 96, 96), steps=FI)

    # ---- sfb2d_fused
    # the lattice at 8 (and 12) taps, one level, around LATTICE_MIN_ELEMS: 4 * 250 * 250 coefficients a plane, 160 planes = 40 M
    for wave, n in (('db4', 494), ('db6', 489)):
        for planes in (159, 160):
            add(wave, 'symmetric', 1, (planes, 1, n, n), 256, steps=INV)
    # ... two levels, around LATTICE_MIN_ELEMS_ML (64 planes = 16 M; 8 CUs, so that 64 planes fill the chip), and three
    for planes in (63, 64):
        add('db4', 'symmetric', 2, (planes, 1, 494, 494), 8, steps=INV)
    add('db4', 'symmetric', 3, (64, 1, 494, 494), 8, steps=INV)
    # float16 at 8 and 10 taps (IROWS_F16_MAXL); 52 coefficients a row both times: whole 4-byte pieces
    for wave, n in (('db4', 97), ('db5', 95)):
        add(wave, 'symmetric', 1, (3, 1, n, n), dtype='float16', steps=INV)
    # periodization: N * C around cus ...
    for planes in (255, 256):
        add('db4', 'periodization', 2, (planes, 1, 64, 320), 256, steps=INV)
    # ... float32 rows of 316 / 320 columns ...
    for W in (316, 320):
        add('db4', 'periodization', 2, (8, 1, 64, W), 8, steps=INV)
    # ... float16 rows of 380 / 384 / 512 / 516 columns at 4 and 6 taps ...
    for wave in ('db2', 'db3'):
        for W in (380, 384, 512, 516):
            add(wave, 'periodization', 2, (8, 1, 64, W), 8, 'float16', steps=INV)
    # ... 12 / 14 taps
    for wave in ('db6', 'db7'):
        add(wave, 'periodization', 2, (8, 1, 64, 320), 8, steps=INV)

    # ---- small planes: 5184 pixels against 5185, four levels against five
    add('db2', 'symmetric', 2, (4, 1, 72, 72))
    add('db2', 'symmetric', 2, (4, 1, 61, 85))
    add('db2', 'symmetric', 4, (4, 1, 64, 64))
    add('db2', 'symmetric', 5, (4, 1, 64, 64))

    # ---- the one-level strip kernels: 124 / 128 columns, an output width that is no multiple of four, W against 2 L (which only
    # a forced launch reaches), periodization on a width that is no multiple of four
    for W in (124, 128, 130, 132):
        add('db2', 'zero', 1, (2, 1, 40, W))
    for W in (15, 16):
        add('db4', 'zero', 1, (2, 1, 40, W), steps=FI, stream_force=True)
    for W in (130, 132):
        add('db2', 'periodization', 1, (2, 1, 40, W), steps=FI)

    # ---- the ladders of dwt/lowlevel.py: J = 4, 5, 7 (the coarsest (j mod 3) + 1 levels go first), a None level, a lone level of
    # 636 / 640 columns (WIDE_ONE_LEVEL) - the whole transform, and the finest level under a None -, odd sizes ('unpad' crops)
    for J in (4, 5, 7):
        add('haar', 'zero', J, (3, 1, 256, 256))
    add('db4', 'symmetric', 4, (3, 1, 160, 160))
    for none_level in (0, 1):
        add('db2', 'symmetric', 3, (3, 1, 96, 96), steps=('inverse', 'backward'), none_level=none_level)
    for W in (636, 640):
        add('haar', 'zero', 1, (2, 1, 24, W), steps=INV)
    add('haar', 'zero', 2, (2, 1, 24, 640), steps=INV, none_level=1)
    add('db4', 'symmetric', 3, (3, 1, 75, 131))
    add('db4', 'symmetric', 3, (9, 1, 70, 66), 8)
    # a biorthogonal wavelet (no quadrature-mirror hint) and float64 (no streaming kernel takes it) through whole transforms
    for mode in ('symmetric', 'periodization'):
        add('bior2.2', mode, 3, (3, 1, 96, 96))
    add('db2', 'symmetric', 2, (3, 1, 96, 96), dtype='float64')
    return out


CASES = _cases()


class _Run(object):
    """One case's modules and input; step(name) runs one step on what the steps before it left."""

    def __init__(self, case):
        dtype = getattr(torch, case['dtype'])
        self.case = case
        self.x = torch.empty(case['shape'], dtype=dtype).requires_grad_('backward' in case['steps'])
        self.xfm = pw.DWTForward(J=case['J'], wave=case['wave'], mode=case['mode'])
        self.ifm = pw.DWTInverse(wave=case['wave'], mode=case['mode'])
        if case.get('half_module'):
            self.xfm, self.ifm = self.xfm.half(), self.ifm.half()

    def step(self, name):
        if name == 'forward':
            self.yl, self.yh = self.xfm(self.x)
        elif name == 'inverse':
            yh = list(self.yh)
            if self.case.get('none_level') is not None:
                yh[self.case['none_level']] = None
            self.rec = self.ifm((self.yl, yh))
        else:
            # cotangents nobody has written: no large tensor is read on the way (but where autograd adds the two gradients of yh[0])
            torch.autograd.backward([self.rec, self.yh[0]], [torch.empty_like(self.rec), torch.empty_like(self.yh[0])])


def _asks_of(case, name, k):
    """The asks of step `name` with the first k declined (the steps before it run on an engine that takes everything), or
    None when the run raised."""
    run = _Run(case)
    ops._FUSED_DECLINED.clear()
    with _installed(Recorder(), case):
        for before in STEPS[:STEPS.index(name)]:
            run.step(before)
    ops._FUSED_DECLINED.clear()
    rec = Recorder(k)
    try:
        with _installed(rec, case):
            run.step(name)
    except NotImplementedError:         # (_lib.check: the last rung was declined)
        return None
    finally:
        ops._FUSED_DECLINED.clear()
    return rec.asks


def run_case(case):
    """The entry of one case as it goes into the file: per recorded step, the list of ask sequences."""
    entry = dict(case=case)
    for name in case['steps']:
        ladders = []
        for k in range(MAX_DECLINES):
            asks = _asks_of(case, name, k)
            if asks is None or (ladders and len(asks) <= len(ladders[-1])):
                break
            ladders.append(asks)
        else:
            raise AssertionError('the ladder of %r %s does not end' % (case, name))
        assert ladders, (case, name)
        entry[name] = ladders
    return entry


def load():
    with open(GOLDEN) as f:
        return json.load(f)
