"""Guard bands around every output the package allocates - shared by tests/test_guard_emu.py and tests/test_guard_gpu.py.

The transforms allocate their outputs with torch.empty / torch.empty_like (pytorch_wavelets_amd/ops.py and the lowlevel modules)
and hand raw pointers to kernels that store 16-byte pieces clipped by hand-written window tests.  The value checks of the suite
look inside the outputs only.  ``guarded(dev)`` replaces the two allocators for the whole process (autograd runs backward passes
on threads of its own) and hands out, for every dense floating-point request, a tensor that lies inside a parent

    [ front guard, 4 KiB | body, on a 256-byte boundary like a fresh allocation | back guard, 4 KiB ]

filled - body included - with a NaN whose payload no kernel produces, compared as integers.  4 KiB is four times the widest store
one wave can issue (64 lanes x 16 bytes).  On exit (after a device synchronisation)
  1. every guard word of every block must still be the sentinel: a store in front of or behind an output lands there, not in a
     neighbour's tensor;
  2. no body that package code allocated may still hold a sentinel word: an element no lane stores is seen although a recycled
     block would have held the previous, correct answer - except the internal buffers of UNWRITTEN_OK, and the outputs a wrapper
     allocated for a launch that the launcher then declined (ops._declined is watched: the blocks whose addresses such a call
     carried may stay WHOLLY untouched - the wrapper drops them and goes to another kernel; a partly written one is reported).
``assert_guarded`` is the coverage condition: an output whose storage lies in no block handed out here went round the harness,
and the test that calls it fails instead of passing silently."""
import contextlib
import ctypes
import linecache
import os
import sys

import torch

import pytorch_wavelets_amd as pw
from pytorch_wavelets_amd import ops

GUARD_BYTES = 4096
ALIGN = 256
# NaNs with a payload, per element size; the 2-byte pattern is a NaN as float16 (0 11111 1110100101) and as bfloat16
# (0 11111111 0100101)
SENTINEL = {2: 0x7FA5, 4: 0x7FC5A5A5, 8: 0x7FF85A5A5A5A5A5A}
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_PKG = os.path.dirname(os.path.abspath(pw.__file__)) + os.sep

# Package buffers that are legitimately not written in full: (allocating function, text the allocating statement contains).
# Established by running the unmodified code under the harness; none is keyed by a shape.
UNWRITTEN_OK = (
    # ops._hinted_taps: 16 floats of which the one-thread examination kernel of csrc/wl_lattice.h writes [0] verdict, [1] gain and
    # [2, 2 + K) one coefficient per tap pair - and only in launches that take the lattice variant: a hinted level of 8 / 10 taps on
    # the strip kernels allocates the scratch and never examines it (the library trusts it after its own examination alone, tap_state)
    ('_new_tap_scratch', 'TAP_SCRATCH_FLOATS'),
    # ops.afb2d(pad_ll=True): rows of Kw coefficients at a cache-line pitch - the kernels store the Kw columns, the caller sees
    # the [..., :Kw] view, nobody reads the pad columns
    ('afb2d', '_ll_pitch('),
    # ops.afb2d_stream(pad_ll=True): the same at a 16-byte pitch (Kp columns allocated, Kw written and returned)
    ('afb2d_stream', 'Kp)'),
)

_REAL_EMPTY, _REAL_EMPTY_LIKE = torch.empty, torch.empty_like
_ACTIVE = []


class Block(object):
    def __init__(self, buf, skip, numel, shape, dtype, site, package, allowed):
        self.buf, self.skip, self.numel, self.shape, self.dtype = buf, skip, numel, tuple(shape), dtype
        self.site, self.package, self.allowed = site, package, allowed
        self.declined = False          # an output of a launch the launcher declined (Guard.declined): dropped unwritten
        self.es = _REAL_EMPTY((), dtype=dtype).element_size()
        self.g = GUARD_BYTES // self.es

    def words(self):
        """the whole parent as integers: g guard words, numel body words, g guard words"""
        nbytes = 2 * GUARD_BYTES + self.numel * self.es
        return self.buf[self.skip:self.skip + nbytes].view(_INT[self.es])

    def parent(self):
        """the whole parent in the block's own dtype (the harness tests write through it)"""
        return self.words().view(self.dtype)

    def body_ptr(self):
        return self.buf.data_ptr() + self.skip + GUARD_BYTES

    def verdicts(self):
        """0-dim bools: front guard intact, back guard intact, body free of sentinel words, body nothing but sentinel words"""
        w, s = self.words(), SENTINEL[self.es]
        body = w[self.g:self.g + self.numel] == s
        return [(w[:self.g] == s).all(), (w[self.g + self.numel:] == s).all(), ~body.any(), body.all()]

    def describe(self):
        return '%s %s allocated at %s' % (self.shape, str(self.dtype).replace('torch.', ''), self.site)


class Guard(object):
    def __init__(self, dev):
        self.dev = torch.device(dev)
        self.blocks = []
        self.c0 = pw.launch_count()
        self.real_declined = ops._declined

    # ---- allocation ------------------------------------------------------------------------------------------------------
    def _wrap(self, t, frame):
        """`t`: what the real allocator returned for the request; the guarded tensor of its shape, dtype and device."""
        es = t.element_size()
        nbytes = 2 * GUARD_BYTES + t.numel() * es
        buf = _REAL_EMPTY(nbytes + ALIGN, dtype=torch.uint8, device=t.device)
        skip = (-buf.data_ptr()) % ALIGN
        code = frame.f_code
        line = linecache.getline(code.co_filename, frame.f_lineno)
        package = os.path.abspath(code.co_filename).startswith(_PKG)
        allowed = any(code.co_name == fn and text in line for fn, text in UNWRITTEN_OK)
        site = '%s:%d %s()' % (os.path.relpath(code.co_filename, os.path.dirname(_PKG.rstrip(os.sep))), frame.f_lineno, code.co_name)
        blk = Block(buf, skip, t.numel(), t.shape, t.dtype, site, package, allowed)
        blk.words().fill_(SENTINEL[es])
        out = _REAL_EMPTY(0, dtype=t.dtype, device=t.device).set_(buf.untyped_storage(), (buf.storage_offset() + skip + GUARD_BYTES) // es,
                                                                  t.shape)
        assert out.data_ptr() == blk.body_ptr() and out.data_ptr() % ALIGN == 0 and out.is_contiguous()
        if t.requires_grad:
            out.requires_grad_(True)
        self.blocks.append(blk)          # (list.append is atomic: autograd's threads allocate too)
        return out

    @staticmethod
    def _guardable(t, kw):
        return (t.is_floating_point() and t.element_size() in SENTINEL and t.layout == torch.strided and t.numel() > 0
                and t.device.type in ('cpu', 'cuda') and kw.get('out') is None and not kw.get('pin_memory')
                and kw.get('memory_format', torch.contiguous_format) in (torch.contiguous_format, torch.preserve_format)
                and t.is_contiguous())

    def empty(self, *a, **kw):
        t = _REAL_EMPTY(*a, **kw)
        return self._wrap(t, sys._getframe(1)) if self._guardable(t, kw) else t

    def empty_like(self, src, *a, **kw):
        t = _REAL_EMPTY_LIKE(src, *a, **kw)
        return self._wrap(t, sys._getframe(1)) if src.is_contiguous() and self._guardable(t, kw) else t

    def declined(self, key, name, ref, *args, **kw):
        """ops._declined: a launcher that declines (WL_ERR_UNSUPPORTED) has launched nothing, and the wrapper drops the outputs it
        had allocated for it.  The blocks whose addresses the call carried are marked: they may stay WHOLLY unwritten - a partly
        written one is reported like any other."""
        res = self.real_declined(key, name, ref, *args, **kw)
        if res:
            ptrs = set()
            for a in args:
                if isinstance(a, int):
                    ptrs.add(a)
                elif isinstance(a, ctypes.Array) and getattr(a, '_type_', None) is ctypes.c_void_p:
                    ptrs.update(v for v in a if v)
            for b in list(self.blocks):
                if b.body_ptr() in ptrs:
                    b.declined = True
        return res

    # ---- coverage ----------------------------------------------------------------------------------------------------------
    def assert_guarded(self, *tensors, **kw):
        """Every tensor (lists and tuples are walked, None is passed over) lies inside the body of a block handed out here.
        Exempt: tensors of zero size and tensors that share their storage with one of `inputs`."""
        inputs = [t.untyped_storage().data_ptr() for t in _flat(kw.pop('inputs', ())) if t.numel()]
        assert not kw, kw
        flat = _flat(tensors)
        assert flat, 'nothing to look at'
        for i, t in enumerate(flat):
            if t.numel() == 0 or t.untyped_storage().data_ptr() in inputs:
                continue
            lo = t.data_ptr()
            hi = lo + (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()
            assert any(b.buf.device == t.device and b.body_ptr() <= lo and hi <= b.body_ptr() + b.numel * b.es for b in self.blocks), \
                'tensor %d %s %s went round the guard: its storage is no block of this context' % (i, tuple(t.shape), t.dtype)

    # ---- the verdict -------------------------------------------------------------------------------------------------------
    def problems(self):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize(self.dev)
        blocks = list(self.blocks)
        if not blocks:
            return []
        by_dev = {}
        for i, b in enumerate(blocks):
            by_dev.setdefault(b.buf.device, []).append(i)
        ok = {}
        for idx in by_dev.values():                 # one transfer per device
            flags = torch.stack([v for i in idx for v in blocks[i].verdicts()]).cpu().tolist()
            for k, i in enumerate(idx):
                ok[i] = flags[4 * k:4 * k + 4]
        out = []
        for i, b in enumerate(blocks):
            front, back, body, untouched = ok[i]
            w, s = b.words(), SENTINEL[b.es]
            if not front:
                at = (w[:b.g] != s).nonzero().flatten().cpu().tolist()
                out.append('FRONT guard of %s overwritten, %s element(s) in front of the body' % (b.describe(), [b.g - k for k in at][:16]))
            if not back:
                at = (w[b.g + b.numel:] != s).nonzero().flatten().cpu().tolist()
                out.append('BACK guard of %s overwritten, %s element(s) behind the body' % (b.describe(), [k + 1 for k in at][:16]))
            if not body and b.package and not b.allowed and not (b.declined and untouched):
                at = (w[b.g:b.g + b.numel] == s).nonzero().flatten().cpu().tolist()
                out.append('%d element(s) of %s never written, flat indices %s' % (len(at), b.describe(), at[:16]))
        if out:
            out.append('launches since entry: %s' % (pw.kernels_since(self.c0),))
        return out


def _flat(ts):
    out = []
    for t in ts:
        if isinstance(t, (list, tuple)):
            out += _flat(t)
        elif t is not None:
            assert isinstance(t, torch.Tensor), type(t)
            out.append(t)
    return out


@contextlib.contextmanager
def guarded(dev):
    """See the module docstring.  Yields the Guard (``.blocks``, ``.assert_guarded``)."""
    assert not _ACTIVE and torch.empty is _REAL_EMPTY and torch.empty_like is _REAL_EMPTY_LIKE, 'guarded() does not nest'
    g = Guard(dev)
    _ACTIVE.append(g)
    torch.empty, torch.empty_like, ops._declined = g.empty, g.empty_like, g.declined
    failed = None
    try:
        yield g
    except Exception as e:          # (the guard's report comes first: a leak explains a wrong value, not the other way round)
        failed = e
    finally:
        torch.empty, torch.empty_like, ops._declined = _REAL_EMPTY, _REAL_EMPTY_LIKE, g.real_declined
        _ACTIVE.pop()
    bad = g.problems()
    g.blocks = []
    if bad:
        if failed is not None:
            bad.append('(the guarded code itself raised %s: %s)' % (type(failed).__name__, str(failed)[:400]))
        raise AssertionError('\n'.join(bad)) from failed
    if failed is not None:
        raise failed


def assert_guarded(*tensors, **kw):
    """Guard.assert_guarded of the active context."""
    assert _ACTIVE, 'assert_guarded outside guarded()'
    _ACTIVE[-1].assert_guarded(*tensors, **kw)


# ---- one direct run per newer family: forward, inverse, one autograd.grad; everything returned must be a guarded block -----------
def _ones(ts):
    return [torch.ones_like(t) for t in ts]


def _pyramid(xfm):
    def fwd(x):
        yl, yh = xfm(x)
        return [yl] + list(yh)
    return fwd


# Rows of tests/_view_cases.py whose gradient is a torch copy of a crop of the (guarded) kernel output: the synthesis ladder of a
# multi-level launch returns the odd-sized dx as a view of a larger tensor, and AFB2DMulti._backward (dwt/lowlevel.py) makes it
# contiguous
CROPPED_DX = ('small-fwd-35x35-f32-offset(1)',)


def _direct(x, fwd, inv, cropped_dx=False):
    """`fwd(x)` -> list of outputs, `inv(outs)` -> reconstruction (or None); one gradient through both.  `cropped_dx`: dx is a
    torch copy of a crop of the kernel's output (CROPPED_DX)."""
    x = x.requires_grad_(True)
    outs = fwd(x)
    rec = inv(outs) if inv is not None else None
    heads = list(outs) + ([rec] if rec is not None else [])
    dx, = torch.autograd.grad(heads, x, _ones(heads))
    assert_guarded(heads, [] if cropped_dx else dx, inputs=[x])
    return heads + [dx]


def direct_scat1d(dev):
    import _scat1d_cases as S
    mod = S.layer(dev, 'near_sym_a')
    for n in (S.lens('near_sym_a')[0], S.core_of('near_sym_a') + 1):
        _direct(S.dev_t(S._inputs(S.LEAD + (n,), 31)[0], S.F32, dev), lambda x: [mod(x)], None)


def direct_swt1d(dev):
    import _swt1d_cases as S
    wave, J = 'db4', 3
    xfm, ifm = S.modules(dev, wave, J)
    for n in (S.lens(wave, J)[0], S.lens(wave, J)[-3] + 1):
        shape = S.ROWS[0] + (n,)
        _direct(S.dev_t(S._inputs(shape, J, 11)[0], S.F32, dev), _pyramid(xfm), lambda o: ifm((o[0], o[1:])))


def direct_wpt1d(dev):
    import _wpt1d_cases as S
    wave, J = 'db4', 3
    xfm, ifm = S.modules(dev, wave, J)
    for n in S.lens(wave, J)[:2]:
        shape = S.ROWS[0] + (n,)
        _direct(S.dev_t(S._inputs(shape, J, 21)[0], S.F32, dev), lambda x: [xfm(x)], lambda o: ifm(o[0], size=n))


def direct_dtcwt1d(dev):
    import _dtcwt1d_cases as S
    for n, J in ((16, 1), (37, 3)):
        xfm, ifm = S.modules(dev, 'near_sym_a', 'qshift_a', J)
        _direct(S.rand((1, 3, n), S.F32, dev, n), _pyramid(xfm), lambda o: ifm((o[0], o[1:])))


def direct_dwt3d(dev):
    import _dwt3d_cases as S
    # (everything odd, two levels: dx is the crop of a 10 x 12 plane; even planes and db2: dx is the kernel's own output)
    for shape, wave, J in (((2, 1, 7, 9, 11), 'db4', 2), ((2, 3, 10, 12, 16), 'db2', 1)):
        xfm, ifm = S.modules(dev, wave, J, 'symmetric')
        _direct(S.rand(shape, S.F32, dev, 1), _pyramid(xfm), lambda o: ifm((o[0], o[1:])), cropped_dx=J == 2)


def direct_wpt2d(dev):
    import _wpt2d_cases as S
    for shape, J in (((1, 1, 5, 7), 1), ((1, 2, 37, 141), 2)):
        xfm, ifm = S.modules(dev, 'db4', J, 'symmetric')
        _direct(S.rand(shape, S.F32, dev, 1), lambda x: [xfm(x)], lambda o: ifm(o[0], size=shape[2:]))


DIRECT = {'scat1d': direct_scat1d, 'swt1d': direct_swt1d, 'wpt1d': direct_wpt1d, 'dtcwt1d': direct_dtcwt1d, 'dwt3d': direct_dwt3d,
          'wpt2d': direct_wpt2d}
