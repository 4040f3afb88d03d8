"""Tensor-level wrappers over the C ABI: allocate outputs with torch, pass raw device pointers and
the current HIP stream down, nothing else.  (PyTorch is plumbing here: memory + streams.)"""
import contextlib
import ctypes
import threading
import torch

from . import _lib

_DTYPES = {torch.float32: 0, torch.float16: 1, torch.float64: 2, torch.bfloat16: 3}   # bfloat16 takes the float16 kernels
_TEST_BACKEND = None   # set ONLY by tests: tests/emu_backend.py (host emulation of the kernel sources) and the recording stub of
                       # tests/_ask_cases.py (no kernel at all: it lists what the wrappers below ask the engine for)


def _backend():
    return _TEST_BACKEND if _TEST_BACKEND is not None else _lib.get()


def _check_tensor(t, name):
    if t.dtype not in _DTYPES:
        raise TypeError('%s: unsupported dtype %s (float16/bfloat16/float32/float64)' % (name, t.dtype))
    if not t.is_cuda and _TEST_BACKEND is None:
        raise RuntimeError('%s is on %s: pytorch_wavelets_amd runs on MI355X only (HIP kernels, '
                           'no CPU fallback). Move the module and its input to a cuda device.'
                           % (name, t.device))


class _NoGuard(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NOGUARD = _NoGuard()


def _device_of(t):
    """Make t's device current around a launch: the C ABI launches on the CURRENT HIP device with the stream it is
    handed, so a tensor on cuda:1 while cuda:0 is current must switch first (ATen does the same for the reference)."""
    return torch.cuda.device(t.device) if t.is_cuda else _NOGUARD


def _same_device(*ts):
    dev = None
    for t in ts:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError('pytorch_wavelets_amd: tensors on different devices (%s, %s)' % (dev, t.device))


def _call(name, ref, *args):
    """One C-ABI call with ref's device current."""
    with _device_of(ref):
        return getattr(_backend(), name)(*args)


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None


def _taps(h, ref):
    """1-D contiguous taps on ref's device in the accumulate dtype (float, or double for f64)."""
    acc = torch.float64 if ref.dtype == torch.float64 else torch.float32
    return h.detach().reshape(-1).to(device=ref.device, dtype=acc).contiguous()


def coeff_len(n, L, mode):
    return (n + 1) // 2 if mode == 2 else (n + L - 1) // 2


def synth_len(K, L, mode, crop=None):
    """Samples one synthesis level makes of K coefficients along an axis; `crop` (the analysis backward's input size) caps it."""
    n = 2 * K if mode == 2 else 2 * K - L + 2
    return n if crop is None else min(n, crop)


def _synth_hw(Kh, Kw, Lh, Lw, mode, out_hw=None):
    """synth_len along H and W; out_hw = the (H, W) crop or None."""
    crop_h, crop_w = (out_hw[0], out_hw[1]) if out_hw is not None else (None, None)
    return synth_len(Kh, Lh, mode, crop_h), synth_len(Kw, Lw, mode, crop_w)


def _outer_inner(shape, dim):
    """A dense tensor seen as (outer, shape[dim], inner)."""
    outer = inner = 1
    for v in shape[:dim]:
        outer *= v
    for v in shape[dim + 1:]:
        inner *= v
    return outer, inner


def _new_pyramid(x, nlev, L, mode, axes):
    """Uninitialised outputs of `nlev` analysis levels along the last `axes` (2: three bands per level, or 1) axes of x:
    ([high_0 ..] finest first, low, the highs' device pointers as the multi-level launchers take them)."""
    lead, size = tuple(x.shape[:-axes]), tuple(x.shape[-axes:])
    band = (3,) if axes == 2 else ()
    yh = []
    for _ in range(nlev):
        size = tuple(coeff_len(n, L, mode) for n in size)
        yh.append(torch.empty(lead + band + size, dtype=x.dtype, device=x.device))
    yl = torch.empty(lead + size, dtype=x.dtype, device=x.device)
    return yh, yl, (ctypes.c_void_p * nlev)(*[t.data_ptr() for t in yh])


def _plane_strides(t):
    """(plane stride, row stride) in elements of a (N,C,H,W) tensor whose (n,c) planes are uniformly spaced and whose
    columns have unit stride - or None when it has no such description (the caller then makes it dense).  The stride of a
    size-1 dimension carries no information (PyTorch leaves it arbitrary: a grayscale channels_last tensor reports
    stride(1) == 1 and still passes is_contiguous()), so only dimensions longer than 1 are consulted."""
    N, C, H, W = t.shape
    s0, s1, s2, s3 = t.stride()
    if W > 1 and s3 != 1:
        return None
    rs = s2 if H > 1 else W
    if rs < W:
        return None
    if C > 1:
        ps = s1
        if N > 1 and s0 != C * ps:
            return None
    elif N > 1:
        ps = s0
    else:
        ps = H * rs
    if ps < 0:
        return None
    return ps, rs


def _planes(t):
    """t (N,C,H,W) as (tensor, plane stride, row stride) with uniformly spaced planes of unit-stride rows (a copy only
    when t has no such layout)."""
    st = None if t.numel() == 0 else _plane_strides(t)
    if st is None:
        t = t.contiguous()
        st = (t.shape[2] * t.shape[3], t.shape[3])
    return t, st[0], st[1]


def _ll_pitch(kw, itemsize):
    """Row pitch (elements) of an inner-level LL buffer: the next multiple of a 128-byte cache line."""
    q = 128 // itemsize
    return (kw + q - 1) // q * q


def afb2d(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, pad_ll=False):
    """One analysis level: x (N,C,H,W) -> ll (N,C,Kh,Kw), highs (N,C,3,Kh,Kw).  x may be a row-padded view
    (unit column stride, uniform plane stride); with `pad_ll` the returned ll is such a view (row pitch = a multiple
    of a cache line) - the level loop uses it for the LL_j that only feed the next level."""
    _check_tensor(x, 'x')
    N, C, H, W = x.shape
    x, x_ps, x_rs = _planes(x)
    hwl, hwh, hhl, hhh = (_taps(h, x) for h in (h_w_lo, h_w_hi, h_h_lo, h_h_hi))
    Lw, Lh = hwl.numel(), hhl.numel()
    Kh, Kw = coeff_len(H, Lh, mode), coeff_len(W, Lw, mode)
    if pad_ll:
        ll = torch.empty((N, C, Kh, _ll_pitch(Kw, x.element_size())), dtype=x.dtype, device=x.device)[..., :Kw]
    else:
        ll = torch.empty((N, C, Kh, Kw), dtype=x.dtype, device=x.device)
    highs = torch.empty((N, C, 3, Kh, Kw), dtype=x.dtype, device=x.device)
    rc = _call('wl_dwt2d_analysis_strided', x, x.data_ptr(), x_ps, x_rs, ll.data_ptr(), ll.stride(1),
                                              ll.stride(2), highs.data_ptr(), _DTYPES[x.dtype], N * C, H, W,
                                              hwl.data_ptr(), hwh.data_ptr(), Lw, hhl.data_ptr(), hhh.data_ptr(), Lh,
                                              mode, _stream(x))
    _lib.check(rc, 'wl_dwt2d_analysis_strided')
    return ll, highs


def sfb2d(ll, highs, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode, out_hw=None):
    """One synthesis level: ll (N,C,Kh,Kw) [may be a strided crop], highs (N,C,3,Kh,Kw) or None
    -> y (N,C,OH,OW); out_hw crops the result (used by the analysis backward)."""
    _check_tensor(ll, 'll')
    N, C, Kh, Kw = ll.shape
    ll, ll_ps, ll_rs = _planes(ll)
    if highs is not None:
        if highs.dtype != ll.dtype:
            highs = highs.to(ll.dtype)
        highs = highs.contiguous()
        if tuple(highs.shape) != (N, C, 3, Kh, Kw):
            raise ValueError('highs %s does not match ll %s' % (tuple(highs.shape), tuple(ll.shape)))
        _same_device(ll, highs)
    gwl, gwh, ghl, ghh = (_taps(g, ll) for g in (g_w_lo, g_w_hi, g_h_lo, g_h_hi))
    Lw, Lh = gwl.numel(), ghl.numel()
    OH, OW = _synth_hw(Kh, Kw, Lh, Lw, mode, out_hw)
    y = torch.empty((N, C, OH, OW), dtype=ll.dtype, device=ll.device)
    rc = _call('wl_dwt2d_synthesis', ll, ll.data_ptr(), ll_ps, ll_rs,
                                       None if highs is None else highs.data_ptr(), y.data_ptr(),
                                       _DTYPES[ll.dtype], N * C, Kh, Kw, OH, OW, gwl.data_ptr(),
                                       gwh.data_ptr(), Lw, ghl.data_ptr(), ghh.data_ptr(), Lh, mode,
                                       _stream(ll))
    _lib.check(rc, 'wl_dwt2d_synthesis')
    return y


_CU_COUNT = {}
_HINTS = threading.local()


class TapVerdict(object):
    """A host-side property of filter buffers, used as a kernel-variant HINT ONLY: which variant to try first.  Correctness never
    rests on it - every variant that relies on a relation between the filter banks (quadrature-mirror highpass banks, the same
    bank on both axes) verifies that relation ON THE DEVICE against the taps as they are when the kernel runs and leaves the work
    to the two-bank variant queued behind it when it does not hold (csrc/wl_common.h, "tap-relation guards"), like the reference,
    which reads its buffers on every forward (dwt/transform2d.py:63-74, :131-148).  The verdict is cached under (data_ptr,
    _version, dtype, device, shape) of every buffer it depends on - one tuple compare per call, no device sync - and recomputed on
    the host when that key changes: in-place edits (mul_, copy_, load_state_dict), re-assigned attributes, .half() / .double() /
    .to(...) all change it.  What the key cannot see (writes through `.data`, whose alias has a version counter of its own; a
    re-assigned buffer that reuses an address) leaves a stale hint, which costs one empty launch and nothing else.  Buffers without
    a version counter (inference tensors) are keyed without it.  `fn` must be a module-level function (modules stay picklable)."""

    def __init__(self, fn):
        self.fn = fn
        self.key = None
        self.val = False

    def __call__(self, *bufs):
        try:
            key = tuple((b.data_ptr(), b._version, b.dtype, b.device, tuple(b.shape)) for b in bufs)
        except (RuntimeError, AttributeError):
            # inference tensors have no version counter: the key does without it - a hint may then outlive an in-place edit, which
            # costs an empty launch (the device verifies every relation), not a coefficient
            try:
                key = tuple((b.data_ptr(), -1, b.dtype, b.device, tuple(b.shape)) for b in bufs)
            except (RuntimeError, AttributeError):
                return False
        if key != self.key:
            self.val = bool(self.fn(*bufs))
            self.key = key
        return self.val


def is_qmf_pair(lo, hi):
    """g1[t] == (-1)**t * g0[L-1-t] exactly (the reconstruction pair of every orthogonal wavelet as pywt tabulates it), L even."""
    a, b = lo.detach().reshape(-1).double().cpu(), hi.detach().reshape(-1).double().cpu()
    if a.numel() != b.numel() or a.numel() % 2 or a.numel() == 0:
        return False
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(a.numel() // 2)
    return bool(torch.equal(b, sign * a.flip(0)))


def is_symmetric_taps(h):
    """h[t] == h[L-1-t] exactly."""
    a = h.detach().reshape(-1).double().cpu()
    return a.numel() > 0 and bool(torch.equal(a, a.flip(0)))


@contextlib.contextmanager
def qmf_hint(flag):
    """Inside this context the caller HINTS that the HIGHPASS banks handed to sfb2d_stream / afb2d_stream are the quadrature
    mirrors of the lowpass banks, hi[t] = (-1)**t * lo[L-1-t] (policy bit 1 of wl_dwt2d_synthesis_stream /
    wl_dwt2d_analysis_stream): DWTInverse / DWTForward set it from their buffers (TapVerdict).  The QMF kernel variant checks the
    relation on the device and the two-bank variant stands by behind it: a wrong hint is slow, not wrong."""
    prev = getattr(_HINTS, 'qmf', False), getattr(_HINTS, 'tapcache', None)
    _HINTS.qmf = bool(flag)
    _HINTS.tapcache = {} if flag else None      # the levels of one transform share their float32 taps and the lattice scratch (_hinted_taps)
    try:
        yield
    finally:
        _HINTS.qmf, _HINTS.tapcache = prev


def _hinted_taps(bufs, ref, L, syn):
    """The four banks of a hinted strip launch as float32 device taps + the lattice variant's device scratch (csrc/wl_lattice.h:
    a one-thread kernel leaves its verdict on the banks and the column lattice there; the lattice kernel and its armed two-bank
    fallback read it) + the `tap_state` word of the *_ex entry points (include/wavelets_hip.h): what the LIBRARY has examined
    into that scratch so far - its launchers set the bits when they run the one-thread kernel and only then, so a level that has no
    use for the scratch (8 / 10 taps on the strip kernels) never makes a later level of the same module call trust an unexamined,
    recycled block.  The cache lives in the qmf_hint context of that call (no user code runs between its levels) and is keyed
    on the buffers' addresses, dtypes and the data type: the levels of a transform then share one examination and - for a
    `.half()` module - one conversion of the taps.  The scratch stays referenced until the context ends: the allocator hands
    it out again on this stream only, behind the launches that read it."""
    cache = getattr(_HINTS, 'tapcache', None)
    # (no version counter in the key: the cache lives for ONE module call, during which nobody edits the buffers)
    key = (tuple((b.data_ptr(), b.dtype) for b in bufs), ref.device, ref.dtype, L, bool(syn))
    ent = cache.get(key) if cache is not None else None
    if ent is None:
        taps = tuple(_taps(b, ref) for b in bufs)
        # (8 taps: the shortest filter any launcher runs the lattice on - the smaller of WL_ROWS_LAT_MIN, csrc/wl_rows_api.inc, and
        # WL_IROWS_LAT_MIN, csrc/wl_idwt_rows.h)
        scratch = _new_tap_scratch(ref.device) if L >= 8 else None
        ent = [taps, scratch, ctypes.c_int(0)]
        if cache is not None:
            cache[key] = ent
    return ent


def _new_tap_scratch(device):
    """WL_TAP_SCRATCH_BYTES of device memory, contents undefined (a recycled block may hold another module's verdict: the library
    trusts it only after its own examination, tap_state).  A function of its own so that a test can hand out poisoned blocks."""
    return torch.empty(TAP_SCRATCH_FLOATS, dtype=torch.float32, device=device)


def _launch_taps(bufs, ref, L, syn, hinted):
    """The taps of one launch of an *_ex entry point: (taps, scratch pointer or None, state word).  Hinted: the entry of
    _hinted_taps (a hint is only ever set together with the tap cache - qmf_hint -, which keeps the scratch alive past this
    call); unhinted: converted taps, no scratch, a state word nobody reads."""
    if not hinted:
        return tuple(_taps(b, ref) for b in bufs), None, ctypes.c_int(0)
    taps, scratch, tstate = _hinted_taps(bufs, ref, L, syn)
    return taps, None if scratch is None else scratch.data_ptr(), tstate


def _fused_hint_bits(same, qmf):
    """Bits 2 and 3 of the `strips` argument of the fused (multi-level) launchers."""
    return (4 if same else 0) | (8 if qmf else 0)


def _strip_policy_bits(force, qmf):
    """The `policy` argument of the one-level strip launchers."""
    return (1 if force else 0) | (2 if qmf else 0)


def current_hints():
    """(qmf, same) as the calling module set them: an autograd Function keeps them in its ctx and re-installs them around its backward
    pass (`hints`), which runs on autograd's own thread, outside the module's contexts.  They stay HINTS there too: every variant they
    select verifies its relation on the device."""
    return bool(getattr(_HINTS, 'qmf', False)), bool(getattr(_HINTS, 'same', False))


@contextlib.contextmanager
def hints(qmf, same):
    with qmf_hint(qmf), same_banks_hint(same):
        yield


def banks_equal(lo_a, hi_a, lo_b, hi_b):
    """Are the two filter banks the same taps, element for element (whatever their shapes)?"""
    f = lambda t: t.detach().reshape(-1).double().cpu()   # noqa: E731
    return (lo_a.numel() == lo_b.numel() and hi_a.numel() == hi_b.numel() and lo_a.numel() > 0
            and bool(torch.equal(f(lo_a), f(lo_b))) and bool(torch.equal(f(hi_a), f(hi_b))))


@contextlib.contextmanager
def same_banks_hint(flag):
    """Inside this context the caller HINTS that the row and the column banks handed to afb2d_fused are the same taps (a
    transform built from one wavelet): bit 2 of the launcher's `strips` argument.  The streaming analysis kernel then runs its
    one-bank variant - one set of tap pairs in its scalar registers instead of two (wl_rows_api.inc: 10 and 12 taps no longer
    spill them) - which compares the two banks on the device first; the two-bank variant stands by behind it.  DWTForward sets it
    from its buffers (TapVerdict)."""
    prev = getattr(_HINTS, 'same', False)
    _HINTS.same = bool(flag)
    try:
        yield
    finally:
        _HINTS.same = prev


STREAM_FORCE = False   # tests: send every single-level analysis the strip kernel covers to it, whatever the shape
FUSED_STRIPS = 0   # default `strips` of the two streaming entry points below: 0 = the engine's policy (the planes must fill
                   # the chip), 1 / 2 = force the streaming kernels whatever the batch (tests pin their backward passes so)
# configurations the streaming launchers declined (WL_ERR_UNSUPPORTED for reasons only they can see: rows wider than the
# compute waves, LDS budget, schedule table, ...).  A decline depends on nothing but the key - every argument the launcher's
# decision can depend on is part of it: device (CU count), dtype, plane count, sizes, strides, tap counts, mode / extension,
# output placement - so the outputs of a doomed call are allocated once per configuration, not on every forward of the
# n = 3, 2, 1 ladder of the callers.  The ADDRESS of an input is no part of a key: where a launcher declines a base it cannot
# load from (afb2d_fused: 16 bytes; sfb2d_fused: 4 bytes; dtcwt_inv21: 2 * sizeof(T)), the wrapper tests it itself and returns
# before the key is written - a view one element into its buffer must not reroute the aligned tensors of its shape.
_FUSED_DECLINED = set()
_FUSED_DECLINED_MAX = 4096


def _remember_decline(key):
    """Memoise a launcher's decline - unless an engine option is set (generic_only / no_stream / scat_stream: the decline may be
    the option's, not the configuration's) - in a bounded set (a long-lived process that sees ever new shapes starts over)."""
    be = _backend()
    if be.wl_get_option(b'generic_only') or be.wl_get_option(b'no_stream') or be.wl_get_option(b'scat_stream'):
        return
    if len(_FUSED_DECLINED) >= _FUSED_DECLINED_MAX:
        _FUSED_DECLINED.clear()
    _FUSED_DECLINED.add(key)


def _declined(key, name, ref, *args, memo=True):
    """One C-ABI call of a launcher that may decline: True when it did (WL_ERR_UNSUPPORTED; remembered under `key` unless
    `memo` is false), False when it ran; any other failure raises."""
    rc = _call(name, ref, *args)
    if rc == _lib.WL_ERR_UNSUPPORTED:
        if memo:
            _remember_decline(key)
        return True
    _lib.check(rc, name)
    return False


def set_option(name, value):
    """wl_set_option of the C ABI ('generic_only', 'no_stream', 'scat_stream'); forgets the memoised declines, which may
    depend on the options."""
    _FUSED_DECLINED.clear()
    rc = _backend().wl_set_option(name.encode() if isinstance(name, str) else name, int(value))
    _lib.check(rc, 'wl_set_option')


def _num_cus(device):
    if device.type != 'cuda':
        return 2                      # the host emulation's tiny "chip" (tests/emu/wl_backend_emu.h)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _CU_COUNT:
        _CU_COUNT[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _CU_COUNT[idx]


def afb2d_fused(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, nlev, strips=None, whole=True):
    """`nlev` (1..3) analysis levels in ONE launch of the streaming kernel (one workgroup per plane, LL_j stay in LDS,
    HBM traffic = the algorithmic minimum).  Returns (yl, [yh_0..]) or None when the kernel does not cover the
    configuration (caller goes level by level).  strips: 0 = only when the planes alone fill the chip (the engine cuts
    some planes in two to fill whole rounds), 1 = force, whole planes only, 2 = force, every plane cut in two.  x may be a row-padded
    view (rows on 16-byte addresses; the width itself need not be a whole number of 16-byte pieces then).  `whole`: this launch is the
    entire transform (a one-level launch on rows of 2-3 KiB is taken only then: inside a longer pyramid the strip kernel is ahead)."""
    _check_tensor(x, 'x')
    if strips is None:
        strips = FUSED_STRIPS
    N, C, H, W = x.shape
    L = h_w_lo.numel()
    # the launcher's envelope, checked here first so that a decline costs no allocation
    # hints (bits 2, 3 of `strips`): the row and the column banks hold the same taps / each highpass bank is the quadrature mirror
    # of its lowpass bank - HINTS: the kernel variants that rely on them verify them on the device, the two-bank variant stands by
    # behind them, so a stale hint costs an empty launch, never a wrong coefficient.  With both, 10-20 taps run the LATTICE variant
    # (csrc/wl_lattice.h): the only fused form of 14, 16 and 20 taps.
    qmf, same = current_hints()
    # (periodization with 12 taps: its odd-cell instantiations are the lattice variant and the two-bank direct form, which spills)
    # (from 10 taps on: WL_ROWS_LAT_MIN of csrc/wl_rows_api.inc)
    lattice = (same and qmf and L in (10, 12, 14, 16, 18, 20)
               and (L > 12 or x.numel() >= LATTICE_MIN_ELEMS or (mode == 2 and L == 12)))
    # (float16- or bfloat16-ROUNDED 20-tap banks - the buffers of a `.half()` / bfloat16 module - are no orthogonal pair to within the lattice's tolerance (residue 9e-4,
    # csrc/wl_lattice.h): the examination rejects them and the armed two-bank 20-tap kernel, which spills, would do the work - 0.70 ms against
    # 0.32 on the strip kernels for 512x1x512^2 J = 2, tools/gpu_r6_per.py deep - the script: in the history up to cf61189)
    if L == 20 and h_w_lo.element_size() == 2 and strips == 0:      # (the engine's policy; a forced launch is taken)
        return None
    if (x.dtype == torch.float64 or nlev < 1 or nlev > 3 or h_h_lo.numel() != L or L % 2 or (L > 12 and not lattice)
            or (nlev > 1 and mode not in (0, 1, 2, 4)) or x.numel() == 0
            or (strips == 0 and 8 * N * C < 3 * _num_cus(x.device)) or strips > 2):
        return None
    # rows as whole 16-byte pieces: a dense x whose width is one, or a row-padded view (the ll that afb2d_stream(pad_ll=True) /
    # afb2d(pad_ll=True) return: any width, the pitch a whole number of pieces and wide enough for the row's last piece)
    es = x.element_size()
    # float32 rows of 2-3 KiB (three pieces per row, round 5): two and more levels per launch, or a one-level transform.  A single
    # level of a longer pyramid stays with the strip kernel (tools/gpu_r5v.py - in the history up to cf61189 -, same process: 128x3x768^2 J = 3 as strip + two fused levels
    # 0.438 ms, as fused + strip + fused 0.464; the last level of 64x3x1024^2 J = 2 on the padded ll 0.465 against 0.456 on the strip kernel)
    # periodization, float16, 12 / 16 / 20 taps (the odd-cell instantiations of the long filters): the strip kernels - tuned on config 5, two / four
    # planes per workgroup - are ahead (tools/gpu_r6_per.py deep, same process, script as above: 512x1x512^2 db8 J = 2 0.188 ms on two strip launches, 0.216
    # fused; J = 1 0.141 / 0.182; db6 0.176 / 0.186; config 5 2.45 / 2.49); float32 (db8 0.294 / 0.245) and 8 taps (0.165 / 0.168; three
    # levels 0.166 / 0.136) stay here
    if mode == 2 and es == 2 and L % 4 == 0 and L >= 12:
        return None
    # ... and rows of exactly 2 KiB (round 6: config 5's 1024-column float16 level, which has more columns than the workgroup has compute
    # waves for two levels; tools/gpu_r6_per.py, as above: the transform 2.51 ms with that level on the strip kernel, 2.68 on the fused one)
    if W * es >= 2048 and nlev < 2 and not whole:
        return None
    x, x_ps, x_rs = _planes(x)
    if (x_rs * es) % 16 or (x_ps * es) % 16 or x.data_ptr() % 16 or (W * es + 15) // 16 * 16 > x_rs * es:
        return None
    key = ('afb', x.device, x.dtype, N * C, H, W, x_ps, x_rs, L, mode, nlev, strips, lattice)
    if key in _FUSED_DECLINED:
        return None
    (hwl, hwh, hhl, hhh), scratch, tstate = _launch_taps((h_w_lo, h_w_hi, h_h_lo, h_h_hi), x, L, False, lattice)
    yh, yl, ptrs = _new_pyramid(x, nlev, L, mode, 2)
    if _declined(key, 'wl_dwt2d_analysis_fused_ex', x, x.data_ptr(), x_ps, x_rs, yl.data_ptr(), ptrs, _DTYPES[x.dtype], N * C, H, W, nlev,
                 hwl.data_ptr(), hwh.data_ptr(), hhl.data_ptr(), hhh.data_ptr(), L, mode, strips | _fused_hint_bits(same, qmf),
                 scratch, ctypes.byref(tstate), _stream(x)):
        return None
    return yl, yh


SMALL_PLANES = True   # planes of up to ~72 x 72 go to the several-planes-per-workgroup kernel first (False: A/B measurements)


def afb2d_small(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, nlev):
    """`nlev` (1..4) analysis levels of small planes in ONE launch, several planes per workgroup (wl_dwt2d_analysis_small):
    x (N,C,H,W) -> (yl, [yh_0..]) like afb2d_fused, or None when the kernel does not cover the configuration."""
    _check_tensor(x, 'x')
    N, C, H, W = x.shape
    L = h_w_lo.numel()
    if (not SMALL_PLANES or FUSED_STRIPS or STREAM_FORCE or x.dtype == torch.float64 or nlev < 1 or nlev > 4 or h_h_lo.numel() != L or L > 20 or x.numel() == 0
            or H * W > 5184 or mode not in _MODE_TO_EXT):
        return None
    key = ('afbsm', x.device, x.dtype, N * C, H, W, L, mode, nlev)
    if key in _FUSED_DECLINED:
        return None
    x = x.contiguous()
    hwl, hwh, hhl, hhh = (_taps(h, x) for h in (h_w_lo, h_w_hi, h_h_lo, h_h_hi))
    yh, yl, ptrs = _new_pyramid(x, nlev, L, mode, 2)
    if _declined(key, 'wl_dwt2d_analysis_small', x, x.data_ptr(), yl.data_ptr(), ptrs, _DTYPES[x.dtype], N * C, H, W, nlev,
                 hwl.data_ptr(), hwh.data_ptr(), hhl.data_ptr(), hhh.data_ptr(), L, mode, _stream(x)):
        return None
    return yl, yh


def sfb2d_small(yl, yh, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode):
    """All len(yh) (1..4) synthesis levels of small planes in ONE launch, several planes per workgroup
    (wl_dwt2d_synthesis_small): yl (N,C,h,w), yh = [finest .. coarsest] of (N,C,3,Kh_j,Kw_j) -> x (N,C,OH,OW) like sfb2d_fused,
    or None when the kernel does not cover the configuration."""
    _check_tensor(yl, 'yl')
    nlev = len(yh)
    N, C, h, w = yl.shape
    L = g_w_lo.numel()
    if (not SMALL_PLANES or FUSED_STRIPS or STREAM_FORCE or yl.dtype == torch.float64 or nlev < 1 or nlev > 4
            or g_h_lo.numel() != L or L % 2 or L > 20 or yl.numel() == 0 or mode not in _MODE_TO_EXT
            or any(t is None or t.dim() != 5 or t.dtype != yl.dtype or t.shape[:3] != (N, C, 3) or t.numel() == 0 for t in yh)):
        return None
    OH, OW = _synth_hw(yh[0].shape[3], yh[0].shape[4], L, L, mode)
    if OH < 1 or OW < 1 or OH * OW > 5184:
        return None
    key = ('sfbsm', yl.device, yl.dtype, N * C, h, w, tuple(tuple(t.shape[3:]) for t in yh), L, mode)
    if key in _FUSED_DECLINED:
        return None
    yl = yl.contiguous()
    yh = [t.contiguous() for t in yh]
    for t in yh:
        _same_device(yl, t)
    gwl, gwh, ghl, ghh = (_taps(g, yl) for g in (g_w_lo, g_w_hi, g_h_lo, g_h_hi))
    y = torch.empty((N, C, OH, OW), dtype=yl.dtype, device=yl.device)
    ptrs = (ctypes.c_void_p * nlev)(*[t.data_ptr() for t in yh])
    khs = (ctypes.c_int * nlev)(*[t.shape[3] for t in yh])
    kws = (ctypes.c_int * nlev)(*[t.shape[4] for t in yh])
    if _declined(key, 'wl_dwt2d_synthesis_small', yl, yl.data_ptr(), h, w, ptrs, khs, kws, y.data_ptr(), _DTYPES[yl.dtype], N * C, nlev,
                 gwl.data_ptr(), gwh.data_ptr(), ghl.data_ptr(), ghh.data_ptr(), L, mode, _stream(yl)):
        return None
    return y


def sfb2d_fused(yl, yh, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode, strips=None):
    """All len(yh) (1..3) synthesis levels in ONE launch of the streaming kernel: yl (N,C,h,w) [may be a strided crop],
    yh = [finest .. coarsest] of (N,C,3,Kh_j,Kw_j) -> x (N,C,OH,OW).  The intermediate low-passes never leave the
    chip.  Returns None when the kernel does not cover the configuration (caller goes level by level)."""
    _check_tensor(yl, 'yl')
    if strips is None:
        strips = FUSED_STRIPS
    nlev = len(yh)
    N, C, h, w = yl.shape
    L = g_w_lo.numel()
    es = yl.element_size()
    # (hints as in afb2d_fused: with "same banks" and "quadrature-mirror highpass" 10-20 taps run the lattice variant of the kernel)
    qmf, same = current_hints()
    # (from 8 taps on: WL_IROWS_LAT_MIN of csrc/wl_idwt_rows.h - the metric's inverse: -6 %)
    lattice = (same and qmf and L in (8, 10, 12, 14, 16, 18, 20)
               and (L > 12 or (nlev >= 1 and yh[0] is not None and yh[0].dim() == 5
                               and 4 * yh[0].shape[3] * yh[0].shape[4] * N * C >= (LATTICE_MIN_ELEMS if nlev == 1 else min(LATTICE_MIN_ELEMS, LATTICE_MIN_ELEMS_ML)))))
    # float16 data, 10 taps and more: the fused synthesis reads its coefficients one 2-byte element at a time and converts each - the per-level strip /
    # tile ladder is ahead (tools/gpu_r6_grid.py, 128x3x512^2 J = 3, fractions of the HBM roofline: db5 0.17 fused / 0.27 per level, db6 0.18 / 0.23,
    # db7 0.15 / 0.23, db9 0.14 / 0.23, bior4.4 0.15 / 0.27; up to 8 taps the two are level: haar 0.45 / 0.34, db2 0.28 / 0.27, db4 0.25 / 0.26)
    if es == 2 and L > IROWS_F16_MAXL and strips == 0:
        return None
    per = mode == 2          # periodization (round 6): every level exactly twice the level above, all 2K outputs kept (the PER instantiations)
    if per and not IROWS_PER:
        return None
    if per and strips == 0 and nlev >= 1 and yh[0] is not None and yh[0].dim() == 5:
        # The periodized loader brings the coefficients in ROW by row (rows that carry their wrapped cells), one LDS-DMA instruction per KiB or part
        # of one: it pays where the finest level's rows fill those instructions and the planes fill the chip.  Same-process A/B against the per-level
        # ladder (tools/gpu_r6_iper.py - in the history up to cf61189 -, profiles/r06g_*): 128x3x512^2 J=3 db4 0.230 -> 0.175 ms, db2 0.226 -> 0.164, 448^2 0.191 -> 0.143, 384^2 0.136 -> 0.118,
        # 512x3x512^2 0.848 -> 0.700; behind it: 256-column planes (+20-31 %), 144 planes (+23 %), 16-20 taps (0 to +6 %), float16 from 6 taps on (db4 +52 %)
        ow0 = 2 * yh[0].shape[4]
        if (L > 12 or N * C < _num_cus(yl.device) or (es == 4 and ow0 < 320)
                or (es == 2 and (L > 4 or not 384 <= ow0 <= 512))):
            return None
    if (yl.dtype == torch.float64 or nlev < 1 or nlev > 3 or g_h_lo.numel() != L or L % 2 or (L > 12 and not lattice)
            or yl.numel() == 0 or (strips == 0 and 8 * N * C < 3 * _num_cus(yl.device)) or strips > 2
            or any(t is None or t.dim() != 5 or t.dtype != yl.dtype or t.shape[:3] != (N, C, 3) or t.numel() == 0
                   or (t.shape[4] * es) % 4 or (t.shape[3] * t.shape[4] * es) % 4 for t in yh)):
        return None
    # the low-pass source of every level is its high-pass size or one larger (then the surplus row / column is dropped)
    sh, sw = h, w
    for t in reversed(yh):
        kh, kw = t.shape[3], t.shape[4]
        if not (kh <= sh <= kh + 1 and kw <= sw <= kw + 1) or kh < L // 2 or kw < L // 2 or (per and (sh, sw) != (kh, kw)):
            return None
        sh, sw = _synth_hw(kh, kw, L, L, mode)
    # the kernel copies the coarsest low-pass like a band plane: dense rows of the coarsest high-pass width
    kh, kw = yh[-1].shape[3], yh[-1].shape[4]
    if (h, w) != (kh, kw):
        yl = yl[..., :kh, :kw]
    st = _plane_strides(yl)
    if st is None or st[1] != kw or (st[0] * es) % 4:
        yl = yl.contiguous()
        st = (kh * kw, kw)
    yl_ps, yl_rs = st
    yh = [t.contiguous() for t in yh]
    for t in yh:
        _same_device(yl, t)
    key = ('sfb', yl.device, yl.dtype, N * C, kh, kw, tuple(tuple(t.shape[3:]) for t in yh), L, mode, strips, lattice)
    if key in _FUSED_DECLINED or yl.data_ptr() % 4 or any(t.data_ptr() % 4 for t in yh):
        return None
    (gwl, gwh, ghl, ghh), scratch, tstate = _launch_taps((g_w_lo, g_w_hi, g_h_lo, g_h_hi), yl, L, True, lattice)
    y = torch.empty((N, C, sh, sw), dtype=yl.dtype, device=yl.device)
    ptrs = (ctypes.c_void_p * nlev)(*[t.data_ptr() for t in yh])
    khs = (ctypes.c_int * nlev)(*[t.shape[3] for t in yh])
    kws = (ctypes.c_int * nlev)(*[t.shape[4] for t in yh])
    if _declined(key, 'wl_dwt2d_synthesis_fused_ex', yl, yl.data_ptr(), yl_ps, yl_rs, kh, kw, ptrs, khs, kws,
                 y.data_ptr(), _DTYPES[yl.dtype], N * C, nlev, gwl.data_ptr(), gwh.data_ptr(), ghl.data_ptr(),
                 ghh.data_ptr(), L, mode, strips | _fused_hint_bits(same, qmf), scratch, ctypes.byref(tstate), _stream(yl)):
        return None
    return y


# narrowest level (columns) the one-level strip kernels are asked for without `force`.  The launchers (csrc/wl_strip_api.inc) decide:
# rows of 2 KiB (analysis; float16: 256 columns) / 1 KiB (synthesis) and wider always, narrower ones when the launch can give every
# compute wave of its workgroups a plane's strip (several planes per workgroup, round 5), workgroups for every CU in both cases.
STRIP_MINW = 128
TAP_SCRATCH_FLOATS = 16   # WL_TAP_SCRATCH_FLOATS of csrc/wl_lattice.h
# Up to 12 taps the direct-form fused kernels exist too, and the lattice launch carries two short extra launches (the examination of the
# banks ~5 us, the armed fallback ~5 us): it pays from about 40 M elements on (128x3x512x512 = 100 M: inverse -6 % at 8 taps, -15 % at 12;
# 128x3x224x224 = 19 M: the extra launches are 15 % of a 65 us transform).  From 14 taps on the lattice is the only fused form.
LATTICE_MIN_ELEMS = 40000000
# ... two and three synthesis levels in one launch run long enough for the lattice earlier (tools/gpu_r5w.py, 8 taps, same box: 128x3x224^2 J = 2 / 3
# 0.064 / 0.057 -> 0.057 / 0.049 ms, 128x3x256^2 0.081 / 0.080 -> 0.071 / 0.069, 96x3x299^2 0.082 / 0.098 -> 0.067 / 0.081; at 64x3x224^2 - 10 M - it loses)
LATTICE_MIN_ELEMS_ML = 16000000
IROWS_F16_MAXL = 8      # longest filter the fused synthesis takes on float16 data under the engine's policy (99: A/B measurements)
IROWS_PER = True        # round 6: periodization on the fused synthesis kernel (False: A/B measurements)


def afb2d_stream(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, force=False, pad_ll=False):
    """One analysis level on the streaming strip kernel (wl_dwt2d_analysis_stream): x (N,C,H,W) -> (ll, highs) like afb2d,
    or None when the kernel does not cover the configuration (rows that are not whole 16-byte pieces, odd tap counts,
    float64, too few workgroups to fill the chip unless `force`).  `pad_ll`: an ll whose rows are no whole 16-byte pieces comes
    back as a view of a buffer with such a row pitch (what afb2d_fused needs of its input)."""
    _check_tensor(x, 'x')
    N, C, H, W = x.shape
    L = h_w_lo.numel()
    es = x.element_size()
    if (x.dtype == torch.float64 or h_h_lo.numel() != L or L % 2 or L > 20 or W < 2 * L or H < 2 or x.numel() == 0
            or (mode in (2, 6) and W % 4) or (mode == 2 and (H + (H & 1) < L - 1 or W + (W & 1) < L - 1))):
        return None
    if not force and W < STRIP_MINW:
        return None                      # the engine's policy: narrower rows stay on the tile kernels (the launcher decides the rest)
    x, x_ps, x_rs = _planes(x)
    qmf = current_hints()[0]
    key = ('afbs', x.device, x.dtype, N * C, H, W, x_ps, x_rs, L, mode, bool(force), qmf, bool(pad_ll))
    if key in _FUSED_DECLINED:
        return None
    (hwl, hwh, hhl, hhh), scratch, tstate = _launch_taps((h_w_lo, h_w_hi, h_h_lo, h_h_hi), x, L, False, qmf)
    Kh, Kw = coeff_len(H, L, mode), coeff_len(W, L, mode)
    q = 16 // es
    Kp = (Kw + q - 1) // q * q if pad_ll else Kw
    ll = torch.empty((N, C, Kh, Kp), dtype=x.dtype, device=x.device)
    if Kp != Kw:
        ll = ll[..., :Kw]
    highs = torch.empty((N, C, 3, Kh, Kw), dtype=x.dtype, device=x.device)
    if _declined(key, 'wl_dwt2d_analysis_stream_ex', x, x.data_ptr(), x_ps, x_rs, ll.data_ptr(), Kh * Kp, Kp, highs.data_ptr(),
                 _DTYPES[x.dtype], N * C, H, W, hwl.data_ptr(), hwh.data_ptr(), hhl.data_ptr(), hhh.data_ptr(), L, mode,
                 _strip_policy_bits(force, qmf), scratch, ctypes.byref(tstate), _stream(x)):
        return None
    return ll, highs


def sfb2d_stream(ll, highs, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode, out_hw=None, force=False):
    """One synthesis level on the streaming strip kernel (wl_dwt2d_synthesis_stream): like sfb2d, or None when the kernel
    does not cover the configuration (no highs, coefficient rows that are not whole 16-byte pieces, odd tap counts,
    float64, too few workgroups / narrow rows unless `force`)."""
    _check_tensor(ll, 'll')
    if highs is None or ll.dtype == torch.float64:
        return None
    N, C, Kh, Kw = ll.shape
    L = g_w_lo.numel()
    es = ll.element_size()
    if (g_h_lo.numel() != L or L % 2 or L > 20 or (mode == 2 and Kw % 4) or Kw < L or Kh < L // 2 or ll.numel() == 0
            or tuple(highs.shape) != (N, C, 3, Kh, Kw) or highs.dtype != ll.dtype
            or (mode == 2 and (2 * Kh < L - 2 or 2 * Kw < L - 2))):
        return None
    OH, OW = _synth_hw(Kh, Kw, L, L, mode, out_hw)
    if not force and (OW < STRIP_MINW or OW % 4):
        return None                      # the engine's policy: narrow rows / unaligned 4-column groups stay on the other kernels
    ll, ll_ps, ll_rs = _planes(ll)
    highs = highs.contiguous()
    _same_device(ll, highs)
    qmf = current_hints()[0]
    key = ('sfbs', ll.device, ll.dtype, N * C, Kh, Kw, ll_ps, ll_rs, OH, OW, L, mode, bool(force), qmf)
    if key in _FUSED_DECLINED:
        return None
    (gwl, gwh, ghl, ghh), scratch, tstate = _launch_taps((g_w_lo, g_w_hi, g_h_lo, g_h_hi), ll, L, True, qmf)
    y = torch.empty((N, C, OH, OW), dtype=ll.dtype, device=ll.device)
    if _declined(key, 'wl_dwt2d_synthesis_stream_ex', ll, ll.data_ptr(), ll_ps, ll_rs, highs.data_ptr(), y.data_ptr(), _DTYPES[ll.dtype],
                 N * C, Kh, Kw, OH, OW, gwl.data_ptr(), gwh.data_ptr(), ghl.data_ptr(), ghh.data_ptr(), L, mode,
                 _strip_policy_bits(force, qmf), scratch, ctypes.byref(tstate), _stream(ll)):
        return None
    return y


def sfb2d_best(ll, highs, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode, out_hw=None):
    """One synthesis level on whichever single-level kernel the engine prefers for the shape."""
    res = sfb2d_stream(ll, highs, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode, out_hw=out_hw, force=STREAM_FORCE)
    return res if res is not None else sfb2d(ll, highs, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode, out_hw=out_hw)


def afb2d_best(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, pad_ll=False, more_levels=False):
    """One analysis level on whichever single-level kernel the engine prefers for the shape: the streaming strip kernel
    (rows of 2 KiB and more, enough workgroups for the chip), else the tile kernels.  `more_levels`: the ll feeds another level -
    it comes back as a row-padded view (rows on 16-byte addresses) when its width is no whole number of 16-byte pieces, so that
    the fused multi-level kernel can take the remaining levels (afb2d_fused)."""
    if x.dim() == 4:                                                             # small planes: several per workgroup
        res = afb2d_small(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, 1)
        if res is not None:
            return res[0], res[1][0]
    res = afb2d_stream(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, force=STREAM_FORCE, pad_ll=more_levels)
    return res if res is not None else afb2d(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, pad_ll=pad_ll)


def afb2d_nonsep(x, filts, mode):
    """One non-separable analysis level: x (N,C,H,W), filts (4,1,Ly,Lx) point-spread functions as
    prep_filt_afb2d_nonsep builds them -> y (N,4C,Kh,Kw), channel 4c+b (reference dwt/lowlevel.py:524-597)."""
    _check_tensor(x, 'x')
    if filts.dim() != 4 or filts.shape[0] != 4 or filts.shape[1] != 1:
        raise ValueError('filts must be a (4, 1, Ly, Lx) tensor, got %s' % (tuple(filts.shape),))
    x = x.contiguous()
    N, C, H, W = x.shape
    Ly, Lx = filts.shape[2], filts.shape[3]
    f = _taps(filts, x)
    y = torch.empty((N, 4 * C, coeff_len(H, Ly, mode), coeff_len(W, Lx, mode)), dtype=x.dtype, device=x.device)
    if x.numel():
        rc = _call('wl_dwt2d_analysis_nonsep', x, x.data_ptr(), y.data_ptr(), _DTYPES[x.dtype], N * C, H, W,
                   f.data_ptr(), Ly, Lx, mode, _stream(x))
        _lib.check(rc, 'wl_dwt2d_analysis_nonsep')
    return y


def sfb2d_nonsep(coeffs, filts, mode, out_hw=None):
    """One non-separable synthesis level: coeffs (N,C,4,Kh,Kw) [or (N,4C,Kh,Kw)], filts (4,1,Ly,Lx) as
    prep_filt_sfb2d_nonsep builds them -> y (N,C,OH,OW) (reference dwt/lowlevel.py:746-798); out_hw crops."""
    _check_tensor(coeffs, 'coeffs')
    if filts.dim() != 4 or filts.shape[0] != 4 or filts.shape[1] != 1:
        raise ValueError('filts must be a (4, 1, Ly, Lx) tensor, got %s' % (tuple(filts.shape),))
    if coeffs.dim() == 5:
        if coeffs.shape[2] != 4:
            raise ValueError('coeffs must be (N, C, 4, H, W), got %s' % (tuple(coeffs.shape),))
        N, C, _, Kh, Kw = coeffs.shape
    else:
        if coeffs.dim() != 4 or coeffs.shape[1] % 4:
            raise ValueError('coeffs must be (N, C, 4, H, W) or (N, 4C, H, W), got %s' % (tuple(coeffs.shape),))
        N, C, Kh, Kw = coeffs.shape[0], coeffs.shape[1] // 4, coeffs.shape[2], coeffs.shape[3]
    coeffs = coeffs.contiguous()
    Ly, Lx = filts.shape[2], filts.shape[3]
    g = _taps(filts, coeffs)
    OH, OW = _synth_hw(Kh, Kw, Ly, Lx, mode, out_hw)
    y = torch.empty((N, C, OH, OW), dtype=coeffs.dtype, device=coeffs.device)
    if coeffs.numel():
        rc = _call('wl_dwt2d_synthesis_nonsep', coeffs, coeffs.data_ptr(), y.data_ptr(), _DTYPES[coeffs.dtype], N * C,
                   Kh, Kw, OH, OW, g.data_ptr(), Ly, Lx, mode, _stream(coeffs))
        _lib.check(rc, 'wl_dwt2d_synthesis_nonsep')
    return y


def afb2d_nonsep_bwd(dy, filts, mode, in_hw):
    """Gradient of afb2d_nonsep with respect to x: dy (N,4C,Kh,Kw) -> dx (N,C,H,W) - the adjoint of boundary gather +
    correlation in every mode, as autograd gives it upstream (dwt/lowlevel.py:524-597 is a plain ATen chain)."""
    _check_tensor(dy, 'dy')
    dy = dy.contiguous()
    H, W = in_hw
    N, C4 = dy.shape[:2]
    Ly, Lx = filts.shape[2], filts.shape[3]
    if tuple(dy.shape[2:]) != (coeff_len(H, Ly, mode), coeff_len(W, Lx, mode)) or C4 % 4:
        raise ValueError('afb2d_nonsep_bwd: dy %s does not belong to a %dx%d input' % (tuple(dy.shape), H, W))
    f = _taps(filts, dy)
    dx = torch.empty((N, C4 // 4, H, W), dtype=dy.dtype, device=dy.device)
    if dx.numel():
        rc = _call('wl_dwt2d_analysis_nonsep_bwd', dy, dy.data_ptr(), dx.data_ptr(), _DTYPES[dy.dtype], N * (C4 // 4), H, W,
                   f.data_ptr(), Ly, Lx, mode, _stream(dy))
        _lib.check(rc, 'wl_dwt2d_analysis_nonsep_bwd')
    return dx


def sfb2d_nonsep_bwd(dy, filts, mode, coeff_shape):
    """Gradient of sfb2d_nonsep with respect to the coefficients: dy (N,C,OH,OW) -> dc of shape coeff_shape
    ((N,C,4,Kh,Kw) or (N,4C,Kh,Kw))."""
    _check_tensor(dy, 'dy')
    dy = dy.contiguous()
    N, C = dy.shape[:2]
    Kh, Kw = coeff_shape[-2], coeff_shape[-1]
    Ly, Lx = filts.shape[2], filts.shape[3]
    g = _taps(filts, dy)
    dc = torch.empty((N, C, 4, Kh, Kw), dtype=dy.dtype, device=dy.device)
    if dc.numel():
        rc = _call('wl_dwt2d_synthesis_nonsep_bwd', dy, dy.data_ptr(), dc.data_ptr(), _DTYPES[dy.dtype], N * C, Kh, Kw,
                   g.data_ptr(), Ly, Lx, mode, _stream(dy))
        _lib.check(rc, 'wl_dwt2d_synthesis_nonsep_bwd')
    return dc.reshape(coeff_shape)


# ---------------------------------------------------------------------------------------------- single axis
EXT_ZERO, EXT_SYM, EXT_REFL, EXT_PERIODIC, EXT_PER, EXT_REPLICATE, EXT_PER_FOLD1 = 0, 1, 2, 3, 4, 5, 6
_MODE_TO_EXT = {0: EXT_ZERO, 1: EXT_SYM, 2: EXT_PER, 4: EXT_REFL, 6: EXT_PERIODIC}


def corr1d(x, dim, h0, h1, K, start, step, tap_step=1, ext=EXT_SYM, taps=None, out=None, out_offset=0, out_stride=1,
           ny=None):
    """y[.., out_offset + out_stride*k, ..] = sum_t h[t] * ext(x, start + step*k + tap_step*t) along axis `dim` of a
    dense tensor, k in [0,K).  h1 (optional) = a second tap set on the same samples -> returns (y0, y1).  `taps` =
    (offset, stride, count) selects a sub-sequence of the stored taps; `out` = tensors to write into (interleaved
    outputs of several calls); ny = length of the output axis (default out_offset + out_stride*K)."""
    _check_tensor(x, 'x')
    x = x.contiguous()
    dim = dim % x.dim()
    n = x.shape[dim]
    outer, inner = _outer_inner(x.shape, dim)
    t0 = _taps(h0, x)
    t1 = None if h1 is None else _taps(h1, x)
    off, ts, nt = taps if taps is not None else (0, 1, t0.numel())
    if ny is None:
        ny = out_offset + out_stride * K
    shape = list(x.shape)
    shape[dim] = ny
    if out is None:
        alloc = torch.empty if (out_stride == 1 and out_offset == 0 and ny == K) else torch.zeros
        out = (alloc(shape, dtype=x.dtype, device=x.device),
               None if h1 is None else alloc(shape, dtype=x.dtype, device=x.device))
    y0, y1 = out
    if x.numel() and K:
        rc = _call('wl_corr1d', x, x.data_ptr(), y0.data_ptr(), None if y1 is None else y1.data_ptr(), _DTYPES[x.dtype],
                   outer, n, inner, ny * inner, K, t0.data_ptr(), None if t1 is None else t1.data_ptr(), off, ts, nt,
                   start, step, tap_step, ext, out_offset, out_stride, _stream(x))
        _lib.check(rc, 'wl_corr1d')
    return (y0, y1) if h1 is not None else y0


def afb1d(x, h0, h1, mode, dim):
    """One analysis level along one axis: (lo, hi), each with coeff_len(n) samples along `dim` (taps = the stored,
    reversed ones).  y[k] = sum_j h[j] * ext(x, 2k + base + j)."""
    n, L = x.shape[dim], h0.numel()
    K = coeff_len(n, L, mode)
    if mode == 2:
        if n + (n & 1) < L - 1:
            # shorter than the filter: the reference folds the wrapped tail only once (dwt/lowlevel.py:146-150), which is
            # not the circular form - evaluated literally by the kernel
            return corr1d(x, dim, h0, h1, K, 1 - L, 2, 1, EXT_PER_FOLD1)
        base = L // 2 - L + 1            # roll by -(L//2), pad L-1 (:143-145); = wl_afb_base, also for odd L
    else:
        base = -((2 * (K - 1) - n + L) // 2)
    return corr1d(x, dim, h0, h1, K, base, 2, 1, _MODE_TO_EXT[mode])


def afb1d_fused(x, h0, h1, mode, J):
    """J (1..4) analysis levels along the LAST axis in ONE launch (wl_dwt1d_analysis_fused: every input sample read once, the
    intermediate lowpass signals stay in LDS): x (..., n) -> (lo, [hi_1 .. hi_J]) finest first, or None when the kernel does
    not cover the configuration (callers go level by level on afb1d)."""
    _check_tensor(x, 'x')
    L = h0.numel()
    n = x.shape[-1]
    if (x.dtype == torch.float64 or J < 1 or J > 4 or L % 2 or L > 20 or h1.numel() != L or x.numel() == 0 or n < L
            or mode not in _MODE_TO_EXT):
        return None
    x = x.contiguous()
    rows = x.numel() // n
    key = ('afb1d', x.device, x.dtype, rows, n, L, mode, J)
    if key in _FUSED_DECLINED:
        return None
    t0, t1 = _taps(h0, x), _taps(h1, x)
    his, lo, ptrs = _new_pyramid(x, J, L, mode, 1)
    if _declined(key, 'wl_dwt1d_analysis_fused', x, x.data_ptr(), lo.data_ptr(), ptrs, _DTYPES[x.dtype], rows, n, J, t0.data_ptr(),
                 t1.data_ptr(), L, mode, _stream(x)):
        return None
    return lo, his


def swt2d_level(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, dilation, ext):
    """One level of the stationary transform in ONE launch (wl_swt2d_level): x (N,C,H,W) - dense, or uniformly spaced planes
    of dense rows such as the ll channels `y[:, 0::4]` of the previous level - -> (N,4C,H,W) with channel 4c + 2r + b
    (r: band along W, b: band along H); taps = the stored (reversed) ones, dilated by `dilation`; `ext` an EXT_* code.
    None when the kernel does not cover the configuration (callers chain corr1d)."""
    _check_tensor(x, 'x')
    N, C, H, W = x.shape
    Lw, Lh = h_w_lo.numel(), h_h_lo.numel()
    if h_w_hi.numel() != Lw or h_h_hi.numel() != Lh or x.numel() == 0:
        return None
    st = _plane_strides(x)
    if st is None or st[1] != W:
        x = x.contiguous()
        st = (H * W, W)
    key = ('swt2d', x.device, x.dtype, N * C, H, W, st[0], Lw, Lh, dilation, ext)
    if key in _FUSED_DECLINED:
        return None
    taps = [_taps(h, x) for h in (h_w_lo, h_w_hi, h_h_lo, h_h_hi)]
    y = torch.empty((N, 4 * C, H, W), dtype=x.dtype, device=x.device)
    if _declined(key, 'wl_swt2d_level', x, x.data_ptr(), st[0], y.data_ptr(), _DTYPES[x.dtype], N * C, H, W,
                 taps[0].data_ptr(), taps[1].data_ptr(), taps[2].data_ptr(), taps[3].data_ptr(), Lw, Lh, dilation, ext, _stream(x)):
        return None
    return y


def iswt2d_level(y, h_w_lo, h_w_hi, h_h_lo, h_h_hi, dilation, ext, scale=1.0, ll=None, ll_mode=0):
    """The transpose of swt2d_level in ONE launch (wl_iswt2d_level): y (N,4C,H,W), channel 4c + 2r + b -> (N,C,H,W),
    scale * sum_{r,b} A_r^T A_b^T y[:, 2r+b::4] with the same taps, dilation and `ext` as the analysis.  scale 1 = the backward of
    a level; scale 1/4 with the synthesis taps and EXT_PERIODIC = one level of the inverse.  `ll` (N,C,H,W) - dense, or
    uniformly spaced planes of dense rows such as `y[:, 0::4]` of another level - with ll_mode 1 replaces the channels 4c + 0
    (y may then be None: the other bands are zeros), with ll_mode 2 is added to them.  y is read dense: a strided or expanded
    tensor (the cotangent of a `.sum()`, say) is copied once first.  None when the kernel does not cover the configuration
    (callers chain corr1d_adj)."""
    ref = y if y is not None else ll
    _check_tensor(ref, 'y')
    if (ll is None) != (ll_mode == 0) or (y is None and ll_mode != 1):
        raise ValueError('iswt2d_level: ll_mode %d does not go with the tensors given' % ll_mode)
    if y is not None:
        N, C4, H, W = y.shape
        if C4 % 4:
            raise ValueError('iswt2d_level: y has %d channels, not four sub-bands per input channel' % C4)
        C = C4 // 4
        y = y.contiguous()
    else:
        N, C, H, W = ll.shape
    ll_ps = 0
    if ll is not None:
        _same_device(y, ll)
        if tuple(ll.shape) != (N, C, H, W) or ll.dtype != ref.dtype:
            raise ValueError('iswt2d_level: ll is %s %s, expected %s %s' % (tuple(ll.shape), ll.dtype, (N, C, H, W), ref.dtype))
        st = None if ll.numel() == 0 else _plane_strides(ll)
        if st is None or st[1] != W:
            ll = ll.contiguous()
            st = (H * W, W)
        ll_ps = st[0]
    Lw, Lh = h_w_lo.numel(), h_h_lo.numel()
    if h_w_hi.numel() != Lw or h_h_hi.numel() != Lh or ref.numel() == 0:
        return None
    key = ('iswt2d', ref.device, ref.dtype, N * C, H, W, y is None, ll_ps, ll_mode, Lw, Lh, dilation, ext)
    if key in _FUSED_DECLINED:
        return None
    taps = [_taps(h, ref) for h in (h_w_lo, h_w_hi, h_h_lo, h_h_hi)]
    x = torch.empty((N, C, H, W), dtype=ref.dtype, device=ref.device)
    if _declined(key, 'wl_iswt2d_level', ref, None if y is None else y.data_ptr(), 4 * H * W, None if ll is None else ll.data_ptr(), ll_ps,
                 ll_mode, x.data_ptr(), _DTYPES[ref.dtype], N * C, H, W, taps[0].data_ptr(), taps[1].data_ptr(), taps[2].data_ptr(),
                 taps[3].data_ptr(), Lw, Lh, dilation, ext, float(scale), _stream(ref)):
        return None
    return x


def _outer_stride(t, dim):
    """Outer stride (elements) of t seen as (outer, K, inner) around axis `dim`: the axes from `dim` on packed, the axes before
    it one uniformly spaced index (every 4th channel of a level, say) - or None when t has no such description."""
    shape, st = t.shape, t.stride()
    inner = 1
    for k in range(t.dim() - 1, dim - 1, -1):
        if shape[k] > 1 and st[k] != inner:
            return None
        inner *= shape[k]
    os_, span = None, 1
    for k in range(dim - 1, -1, -1):
        if shape[k] == 1:
            continue
        if os_ is None:
            os_ = st[k]
            if os_ < inner:
                return None
        elif st[k] != os_ * span:
            return None
        span *= shape[k]
    return inner if os_ is None else os_


def _with_outer_stride(t, dim):
    """(t, outer stride) for the single-axis kernels - t itself where it has such a description, a dense copy otherwise;
    (None, 0) for None."""
    if t is None:
        return None, 0
    os_ = _outer_stride(t, dim) if t.numel() else None
    if os_ is None:
        t = t.contiguous()
        os_ = _outer_stride(t, dim) if t.numel() else 0
    return t, os_


def corr1d_adj(y0, y1, dim, h0, h1, n, start, tap_step=1, ext=EXT_SYM, scale=1.0):
    """The transpose of corr1d with step 1 (wl_corr1d_adj): y0 / y1 (same shape, K samples along `dim`; y1 / h1 may be None) ->
    dx with n samples along `dim`, dx = scale * (A_0^T y0 + A_1^T y1) where A_b x = sum_t h_b[t] * ext(x, start + k + tap_step*t).
    Every extension rule but the periodizations, pads of any length.  The inputs may be uniformly spaced along the axes before
    `dim` (no copy of every 4th channel of a level)."""
    _check_tensor(y0, 'y0')
    if ext not in (EXT_ZERO, EXT_SYM, EXT_REFL, EXT_PERIODIC, EXT_REPLICATE):
        raise ValueError('corr1d_adj: extension %r has no transpose here' % (ext,))
    if (y1 is None) != (h1 is None):
        raise ValueError('corr1d_adj: y1 and h1 go together')
    dim = dim % y0.dim()
    if y1 is not None:
        _same_device(y0, y1)
        if y1.shape != y0.shape or y1.dtype != y0.dtype:
            raise ValueError('corr1d_adj: y0 is %s %s, y1 is %s %s' % (tuple(y0.shape), y0.dtype, tuple(y1.shape), y1.dtype))
    y0, os0 = _with_outer_stride(y0, dim)
    y1, os1 = _with_outer_stride(y1, dim)
    K = y0.shape[dim]
    outer, inner = _outer_inner(y0.shape, dim)
    t0 = _taps(h0, y0)
    t1 = None if h1 is None else _taps(h1, y0)
    shape = list(y0.shape)
    shape[dim] = n
    dx = torch.empty(shape, dtype=y0.dtype, device=y0.device)
    if dx.numel():
        rc = _call('wl_corr1d_adj', y0, y0.data_ptr(), os0, None if y1 is None else y1.data_ptr(), os1, dx.data_ptr(),
                   _DTYPES[y0.dtype], outer, n, inner, K, t0.data_ptr(), None if t1 is None else t1.data_ptr(), t0.numel(), start,
                   tap_step, ext, float(scale), _stream(y0))
        _lib.check(rc, 'wl_corr1d_adj')
    return dx


def sfb1d_fused(lo, his, g0, g1, mode, out_len=None):
    """All len(his) (1..4) synthesis levels along the LAST axis in ONE launch (wl_dwt1d_synthesis_fused): lo (..., n_lo), his =
    [finest .. coarsest] (None = zeros) -> y (..., out_len) (default: the full reconstruction 2 n_hi[0] - L + 2), or None when
    the kernel does not cover the configuration (callers go level by level on sfb1d)."""
    _check_tensor(lo, 'lo')
    J, L = len(his), g0.numel()
    if (lo.dtype == torch.float64 or J < 1 or J > 4 or L % 2 or L > 20 or g1.numel() != L or lo.numel() == 0 or mode == 2
            or mode not in _MODE_TO_EXT or all(h is None for h in his)):
        return None
    lens = []
    for j, h in enumerate(his):
        if h is None:
            # a missing level has the length its neighbours imply: the coarser level's reconstruction (or lo) cropped by nothing
            return None
        if h.dtype != lo.dtype or h.shape[:-1] != lo.shape[:-1]:
            return None
        lens.append(h.shape[-1])
    full = synth_len(lens[0], L, mode)
    if out_len is None:
        out_len = full
    if out_len < 1 or out_len > full:
        return None
    key = ('sfb1d', lo.device, lo.dtype, lo.numel() // lo.shape[-1], lo.shape[-1], tuple(lens), L, mode, out_len)
    if key in _FUSED_DECLINED:
        return None
    lo = lo.contiguous()
    his = [h.contiguous() for h in his]
    for h in his:
        _same_device(lo, h)
    rows = lo.numel() // lo.shape[-1]
    t0, t1 = _taps(g0, lo), _taps(g1, lo)
    y = torch.empty(lo.shape[:-1] + (out_len,), dtype=lo.dtype, device=lo.device)
    ptrs = (ctypes.c_void_p * J)(*[h.data_ptr() for h in his])
    ns = (ctypes.c_int * J)(*lens)
    if _declined(key, 'wl_dwt1d_synthesis_fused', lo, lo.data_ptr(), lo.shape[-1], ptrs, ns, y.data_ptr(), out_len, _DTYPES[lo.dtype], rows, J,
                 t0.data_ptr(), t1.data_ptr(), L, mode, _stream(lo)):
        return None
    return y


def sfb1d(lo, hi, g0, g1, mode, dim, out_len=None):
    """One synthesis level along one axis (hi may be None = zeros); out_len crops (analysis backward)."""
    _check_tensor(lo, 'lo')
    lo = lo.contiguous()
    dim = dim % lo.dim()
    K, L = lo.shape[dim], g0.numel()
    if hi is not None:
        hi = hi.to(lo.dtype).contiguous()
        if hi.shape != lo.shape:
            raise ValueError('lo %s and hi %s differ in shape' % (tuple(lo.shape), tuple(hi.shape)))
        _same_device(lo, hi)
    ny = synth_len(K, L, mode, out_len)
    outer, inner = _outer_inner(lo.shape, dim)
    shape = list(lo.shape)
    shape[dim] = ny
    y = torch.empty(shape, dtype=lo.dtype, device=lo.device)
    t0, t1 = _taps(g0, lo), _taps(g1, lo)
    if y.numel():
        rc = _call('wl_synth1d', lo, lo.data_ptr(), None if hi is None else hi.data_ptr(), y.data_ptr(), _DTYPES[lo.dtype],
                   outer, K, inner, ny, t0.data_ptr(), t1.data_ptr(), L, mode, _stream(lo))
        _lib.check(rc, 'wl_synth1d')
    return y


# ---------------------------------------------------------------------------------------------- the depth axis of the 3-D DWT
def _axis_strides(t, dim):
    """(outer stride, axis stride) in elements of t seen as (outer, n, inner) around axis `dim`: the axes behind `dim` packed, the
    axis itself at any stride that clears a plane, the axes before it one uniformly spaced index - or None when t has no such
    description.  (Strides of size-1 axes carry no information and are not consulted.)"""
    shape, st = t.shape, t.stride()
    inner = 1
    for k in range(t.dim() - 1, dim, -1):
        if shape[k] > 1 and st[k] != inner:
            return None
        inner *= shape[k]
    as_ = st[dim] if shape[dim] > 1 else inner
    if as_ < inner:
        return None
    os_, span = None, 1
    for k in range(dim - 1, -1, -1):
        if shape[k] == 1:
            continue
        if os_ is None:
            os_ = st[k]
            if os_ < 0:
                return None
        elif st[k] != os_ * span:
            return None
        span *= shape[k]
    return (as_ * shape[dim] if os_ is None else os_), as_


def _depth_views(ts, dim):
    """Every tensor of `ts` (None stays None) with its (outer stride, axis stride) for the depth kernels - the tensor itself
    where it is a plane-strided view, one dense copy otherwise."""
    out, oss, ass = [], [], []
    for t in ts:
        if t is None:
            out.append(None), oss.append(0), ass.append(0)
            continue
        st = _axis_strides(t, dim) if t.numel() else None
        if st is None:
            t = t.contiguous()
            st = _axis_strides(t, dim) if t.numel() else (0, 0)
        out.append(t), oss.append(st[0]), ass.append(st[1])
    return out, oss, ass


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _i64_array(vs):
    return (ctypes.c_int64 * len(vs))(*vs)


def _depth_out(ref, dim, K, count):
    """`count` uninitialised tensors shaped like ref with K samples along `dim`, side by side in one allocation."""
    shape = list(ref.shape)
    shape[dim] = K
    buf = torch.empty([count] + shape, dtype=ref.dtype, device=ref.device)
    return [buf[i] for i in range(count)]


def _depth_align(ts):
    """What the launcher's choice between its 16-byte and its scalar body depends on besides sizes and strides: are all bases
    16-byte aligned?  (Part of the decline keys: a decline never depends on it today, and must not be remembered across it.)"""
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def afb_depth(srcs, h0, h1, mode, chunks=0, dim=1, out=None):
    """One analysis level along axis `dim` of up to four tensors of one shape in ONE launch of the streaming depth kernel
    (wl_dwt3d_depth_analysis): srcs[s] (outer.., n, inner..) -> (los, his), lists of tensors with coeff_len(n) samples along `dim`,
    taps = the stored (reversed) ones - what afb1d makes of each source.  The sources may be plane-strided views (the bands of
    the 2-D engine's (P,3,H',W') highs, every 4th channel): the axes behind `dim` packed, `dim` and the axes before it at any
    uniform stride; anything else is copied once.  `out` = (los, his): views to write into - the final layout of a transform
    (same rule; the caller owns their shapes) - instead of fresh tensors.  chunks: 0 = the engine's policy, c > 0 = c depth chunks.
    None when the kernel does not cover the configuration (float64, odd / unequal / more than 20 taps, periodization of a signal
    shorter than the filter): callers run afb1d per source."""
    nsrc = len(srcs)
    if not 1 <= nsrc <= 4:
        raise ValueError('afb_depth: one to four sources, not %d' % nsrc)
    ref = srcs[0]
    for t in srcs:
        _check_tensor(t, 'src')
        if t.shape != ref.shape or t.dtype != ref.dtype:
            raise ValueError('afb_depth: sources differ in shape or dtype')
    _same_device(*srcs)
    dim = dim % ref.dim()
    n, L = ref.shape[dim], h0.numel()
    if (ref.dtype == torch.float64 or L % 2 or L > 20 or h1.numel() != L or ref.numel() == 0 or mode not in _MODE_TO_EXT
            or (mode == 2 and n + (n & 1) < L - 1)):
        return None
    K = coeff_len(n, L, mode)
    outer, inner = _outer_inner(ref.shape, dim)
    srcs, s_os, s_as = _depth_views(srcs, dim)
    if out is None:
        both = _depth_out(ref, dim, K, 2 * nsrc)
        los, his = both[:nsrc], both[nsrc:]
    else:
        los, his = list(out[0]), list(out[1])
    l_st = [_axis_strides(t, dim) for t in los]
    h_st = [_axis_strides(t, dim) for t in his]
    if any(st is None for st in l_st + h_st):
        raise ValueError('afb_depth: an output view is not plane-strided')
    key = ('afb_depth', ref.device, ref.dtype, nsrc, outer, n, inner, tuple(s_os), tuple(s_as), tuple(l_st), tuple(h_st), L, mode,
           chunks, _depth_align(srcs + los + his))
    if key in _FUSED_DECLINED:
        return None
    t0, t1 = _taps(h0, ref), _taps(h1, ref)
    if _declined(key, 'wl_dwt3d_depth_analysis', ref, _ptr_array(srcs), _i64_array(s_os), _i64_array(s_as),
                 _ptr_array(los), _i64_array([st[0] for st in l_st]), _i64_array([st[1] for st in l_st]),
                 _ptr_array(his), _i64_array([st[0] for st in h_st]), _i64_array([st[1] for st in h_st]),
                 nsrc, _DTYPES[ref.dtype], outer, n, inner, t0.data_ptr(), L, t1.data_ptr(), L, mode, chunks, _stream(ref)):
        return None
    return los, his


def sfb_depth(los, his, g0, g1, mode, out_len=None, chunks=0, dim=1, out=None):
    """One synthesis level along axis `dim` of up to four band pairs in ONE launch of the streaming depth kernel
    (wl_dwt3d_depth_synthesis): los[s], his[s] (outer.., K, inner..; his[s] None = zeros) -> [y_s] with synth_len(K) samples along
    `dim`, or out_len of them (the crop of the analysis backward) - what sfb1d makes of each pair.  Views, `out` (a list of
    views to write into) and `chunks` as for afb_depth.  None when the kernel does not cover the configuration: callers run
    sfb1d per pair."""
    nsrc = len(los)
    if not 1 <= nsrc <= 4 or len(his) != nsrc:
        raise ValueError('sfb_depth: one to four (lo, hi) pairs')
    ref = los[0]
    for t in list(los) + [h for h in his if h is not None]:
        _check_tensor(t, 'band')
        if t.shape != ref.shape or t.dtype != ref.dtype:
            raise ValueError('sfb_depth: bands differ in shape or dtype')
    _same_device(*los, *his)
    dim = dim % ref.dim()
    K, L = ref.shape[dim], g0.numel()
    if (ref.dtype == torch.float64 or L % 2 or L > 20 or g1.numel() != L or ref.numel() == 0 or mode not in _MODE_TO_EXT
            or (mode == 2 and 2 * K < L - 2)):
        return None
    ny = synth_len(K, L, mode, out_len)
    if ny < 1:
        return None
    outer, inner = _outer_inner(ref.shape, dim)
    los, l_os, l_as = _depth_views(los, dim)
    his, h_os, h_as = _depth_views(his, dim)
    ys = _depth_out(ref, dim, ny, nsrc) if out is None else list(out)
    y_st = [_axis_strides(t, dim) for t in ys]
    if any(st is None for st in y_st):
        raise ValueError('sfb_depth: an output view is not plane-strided')
    key = ('sfb_depth', ref.device, ref.dtype, nsrc, outer, K, inner, ny, tuple(l_os), tuple(l_as), tuple(h is None for h in his),
           tuple(h_os), tuple(h_as), tuple(y_st), L, mode, chunks, _depth_align(los + his + ys))
    if key in _FUSED_DECLINED:
        return None
    t0, t1 = _taps(g0, ref), _taps(g1, ref)
    if _declined(key, 'wl_dwt3d_depth_synthesis', ref, _ptr_array(los), _i64_array(l_os), _i64_array(l_as),
                 _ptr_array(his), _i64_array(h_os), _i64_array(h_as),
                 _ptr_array(ys), _i64_array([st[0] for st in y_st]), _i64_array([st[1] for st in y_st]),
                 nsrc, _DTYPES[ref.dtype], outer, K, inner, ny, t0.data_ptr(), L, t1.data_ptr(), L, mode, chunks, _stream(ref)):
        return None
    return ys

# ---------------------------------------------------------------------------------------------- 1-D DTCWT
DT1D_PAD_NONE, DT1D_PAD_REPL, DT1D_PAD_ZERO = 0, 1, 2
DT1D_RULE_NONE, DT1D_RULE_CROP, DT1D_RULE_FOLD = 0, 1, 2
DT1D_CHUNK = 0     # tests: a forced chunk length of the two fused kernels (0 = the engine's policy), to put seams into short signals


def dtcwt1d_lengths(n, pads, qstart):
    """Output lengths [n_1 ..] of the analysis levels of an n-sample signal whose level inputs carry the end rules `pads`
    (pads[0] is ignored for a level-1 start: an odd n gets one more sample)."""
    ns = []
    for l, p in enumerate(pads):
        n = n + (n & 1) if l == 0 and not qstart else (n + (2 if p else 0)) // 2
        ns.append(n)
    return ns


def dtcwt1d_pads(n, J, qstart):
    """The transform's own end rules: one replicated sample either side wherever a q-shift level's input is no multiple of 4."""
    pads = []
    for l in range(J):
        if l == 0 and not qstart:
            pads.append(DT1D_PAD_NONE)
            n += n & 1
        else:
            pads.append(DT1D_PAD_REPL if n % 4 else DT1D_PAD_NONE)
            n = (n + (2 if pads[-1] else 0)) // 2
    return pads


def _dt1d_covered(taps, J, qstart):
    o0, o1, qa, qb, ra, rb = taps
    if not qstart and (o0.numel() % 2 == 0 or o1.numel() % 2 == 0 or max(o0.numel(), o1.numel()) > 19):
        return False
    if J > 1 or qstart:
        M = qa.numel()
        return M in (10, 14, 18) and all(t.numel() == M for t in (qb, ra, rb))
    return True


def dtcwt1d_fwd(x, taps, pads, qstart, want_hi, want_lo, chunk=None):
    """len(pads) (1..4) levels of the 1-D DTCWT analysis along the LAST axis in ONE launch (wl_dtcwt1d_analysis): x (..., n),
    taps = (h0o, h1o, h0a, h0b, h1a, h1b) as stored -> (los, his), lists over the levels with None where want_lo / want_hi is
    false (the last lowpass is always made); his[l] (..., n_l) = the flat (real, imaginary) pairs.  None when the kernel does
    not cover the configuration (callers compose the single-axis primitives)."""
    _check_tensor(x, 'x')
    J, n = len(pads), x.shape[-1]
    if x.dtype == torch.float64 or x.numel() == 0 or J < 1 or J > 4 or not _dt1d_covered(taps, J, qstart):
        return None
    chunk = DT1D_CHUNK if chunk is None else chunk
    rows = x.numel() // n
    pads = [DT1D_PAD_NONE if (l == 0 and not qstart) else int(p) for l, p in enumerate(pads)]
    sizes = tuple(t.numel() for t in taps)
    key = ('dt1d_fwd', x.device, x.dtype, rows, n, tuple(pads), bool(qstart), sizes, chunk)
    if key in _FUSED_DECLINED:
        return None
    x = x.contiguous()
    ns = dtcwt1d_lengths(n, pads, qstart)
    lead = tuple(x.shape[:-1])
    his = [torch.empty(lead + (ns[l],), dtype=x.dtype, device=x.device) if want_hi[l] else None for l in range(J)]
    los = [torch.empty(lead + (ns[l],), dtype=x.dtype, device=x.device) if (want_lo[l] or l == J - 1) else None for l in range(J)]
    tt = [_taps(t, x) for t in taps]
    if _declined(key, 'wl_dtcwt1d_analysis', x, x.data_ptr(), _ptr_array(his), _ptr_array(los), _DTYPES[x.dtype], rows, n, J,
                 int(bool(qstart)), (ctypes.c_int * J)(*pads), tt[0].data_ptr(), tt[1].data_ptr(), sizes[0], sizes[1],
                 tt[2].data_ptr(), tt[3].data_ptr(), tt[4].data_ptr(), tt[5].data_ptr(), sizes[2], chunk, _stream(x)):
        return None
    return los, his


def dtcwt1d_inv(lo, his, ns, rules, out_len, taps, qstart, chunk=None):
    """len(his) (1..4) levels of the 1-D DTCWT synthesis along the LAST axis in ONE launch (wl_dtcwt1d_synthesis): lo (..., n_lo),
    his[l] (..., ns[l]) flat (real, imaginary) pairs or None = zeros, finest first; rules[l] = end rule of the output of level
    l + 1 (rules[0]: of y), rules[J]: CROP = lo carries one surplus sample either side; taps = (g0o, g1o, g0a, g0b, g1a, g1b).
    Returns y (..., out_len), or None when the kernel does not cover the configuration."""
    _check_tensor(lo, 'lo')
    J = len(his)
    if lo.dtype == torch.float64 or lo.numel() == 0 or J < 1 or J > 4 or not _dt1d_covered(taps, J, qstart):
        return None
    for h in his:
        if h is not None:
            _check_tensor(h, 'yh')
            _same_device(lo, h)
            if h.dtype != lo.dtype:
                return None
    chunk = DT1D_CHUNK if chunk is None else chunk
    n_lo = lo.shape[-1]
    rows = lo.numel() // n_lo
    sizes = tuple(t.numel() for t in taps)
    key = ('dt1d_inv', lo.device, lo.dtype, rows, n_lo, tuple(ns), tuple(rules), out_len, bool(qstart), sizes, chunk)
    if key in _FUSED_DECLINED:
        return None
    lo = lo.contiguous()
    his = [None if h is None else h.contiguous() for h in his]
    y = torch.empty(tuple(lo.shape[:-1]) + (out_len,), dtype=lo.dtype, device=lo.device)
    tt = [_taps(t, lo) for t in taps]
    if _declined(key, 'wl_dtcwt1d_synthesis', lo, lo.data_ptr(), n_lo, _ptr_array(his), (ctypes.c_int * J)(*ns),
                 (ctypes.c_int * (J + 1))(*rules), y.data_ptr(), out_len, _DTYPES[lo.dtype], rows, J, int(bool(qstart)),
                 tt[0].data_ptr(), tt[1].data_ptr(), sizes[0], sizes[1], tt[2].data_ptr(), tt[3].data_ptr(), tt[4].data_ptr(),
                 tt[5].data_ptr(), sizes[2], chunk, _stream(lo)):
        return None
    return y


# ---------------------------------------------------------------------------------------------- wave tiles
# (csrc/wl_wave1d.h): what the launchers of the 1-D stationary and the 1-D wavelet packet transform share
WAVE1D_TILE = 1024   # positions a wave holds: 64 lanes x WL_WAVE1D_V
WAVE1D_MAXJ = 3      # WL_WAVE1D_MAXJ: levels per launch
WAVE1D_MAXL = 20     # WL_WAVE1D_MAXL: taps


def wave1d_covered(dtype, L, J=1):
    """What the envelope of every wave-tile launcher asks of the element type, the tap count and the levels of a launch."""
    return dtype != torch.float64 and L % 2 == 0 and L <= WAVE1D_MAXL and 1 <= J <= WAVE1D_MAXJ


def _wave1d_covered(t, n, L, L1, J):
    return wave1d_covered(t.dtype, L, J) and t.numel() != 0 and L1 == L and n < 1 << 30


# ---------------------------------------------------------------------------------------------- the 1-D stationary transform
SWT1D_FUSED = True   # up to three periodic levels per launch on the wave-tile kernels (csrc/wl_swt1d.h).  False: everything level
#                      by level on corr1d / corr1d_adj, for A/B measurements and tests.
SWT1D_MAXJ = WAVE1D_MAXJ


def swt1d_core(L, J):
    """Positions of a wave's tile that are still valid after J levels of an L-tap bank: what a tile stores, and what the tiles
    of a row advance by (the seams of a row lie at multiples of it, minus `origin`)."""
    return WAVE1D_TILE - (L - 1) * (2 ** J - 1)


def _swt1d_covered(t, L, L1, J):
    return _wave1d_covered(t, t.shape[-1], L, L1, J)


def swt1d_fwd(x, h0, h1, nlev, origin=0, scale=1.0):
    """`nlev` (1..3) levels of the periodic a-trous analysis along the LAST axis in ONE launch (wl_swt1d_analysis): x (..., n) ->
    (lo, [hi_1 .. hi_nlev]) finest first, all (..., n); level j has dilation 2**(j-1) and is multiplied by `scale`.  None when
    the launcher declines (float64, odd or long filters, more levels): callers go level by level on corr1d.  `origin` (tests)
    moves the tile seams."""
    _check_tensor(x, 'x')
    L, n = h0.numel(), x.shape[-1]
    if not _swt1d_covered(x, L, h1.numel(), nlev):
        return None
    x = x.contiguous()
    rows = x.numel() // n
    key = ('swt1d_fwd', x.device, x.dtype, rows, n, L, nlev)
    if key in _FUSED_DECLINED:
        return None
    t0, t1 = _taps(h0, x), _taps(h1, x)
    lo = torch.empty_like(x)
    his = [torch.empty_like(x) for _ in range(nlev)]
    if _declined(key, 'wl_swt1d_analysis', x, x.data_ptr(), lo.data_ptr(), _ptr_array(his), _DTYPES[x.dtype], rows, n, nlev,
                 t0.data_ptr(), t1.data_ptr(), L, EXT_PERIODIC, float(scale), int(origin), _stream(x)):
        return None
    return lo, his


def swt1d_adj(lo, his, g0, g1, scale, origin=0):
    """The transpose of swt1d_fwd in ONE launch (wl_swt1d_adjoint): lo (..., n), his = [finest .. coarsest] (None = zeros) ->
    y (..., n), per level, coarsest first, lo_{j-1} = scale * (A_0(g)^T lo_j + A_1(g)^T hi_j).  None when the launcher declines."""
    _check_tensor(lo, 'lo')
    J, L, n = len(his), g0.numel(), lo.shape[-1]
    if not _swt1d_covered(lo, L, g1.numel(), J):
        return None
    for h in his:
        if h is not None:
            _check_tensor(h, 'yh')
            _same_device(lo, h)
            if h.dtype != lo.dtype or h.shape != lo.shape:
                return None
    rows = lo.numel() // n
    key = ('swt1d_adj', lo.device, lo.dtype, rows, n, L, J)
    if key in _FUSED_DECLINED:
        return None
    lo = lo.contiguous()
    his = [None if h is None else h.contiguous() for h in his]
    t0, t1 = _taps(g0, lo), _taps(g1, lo)
    y = torch.empty_like(lo)
    if _declined(key, 'wl_swt1d_adjoint', lo, lo.data_ptr(), _ptr_array(his), y.data_ptr(), _DTYPES[lo.dtype], rows, n, J,
                 t0.data_ptr(), t1.data_ptr(), L, EXT_PERIODIC, float(scale), int(origin), _stream(lo)):
        return None
    return y


SWT1D_TAPGRAD_FUSED = True   # the tap gradients of the 1-D stationary transform in one launch on the wave-tile kernels
#                              (csrc/wl_swt1d_tapgrad.h).  False: lowlevel's composition - the chains level by level and rolled
#                              products summed in float64 -, for A/B measurements and tests.


def swt1d_tapgrad_core(L, J):
    """Positions of a wave's tile whose products the tap-gradient kernel sums, and what the tiles of a row advance by: the
    analysis chain and the adjoint chain eat max((L/2 - 1)(2^J - 1), (L/2)(2^J - 2)) positions in front and (L/2)(2^J - 1) behind."""
    return WAVE1D_TILE - max((L // 2 - 1) * (2 ** J - 1), (L // 2) * (2 ** J - 2)) - (L // 2) * (2 ** J - 1)


def swt1d_tapgrad(s, top, his, k0, k1, scale, origin=0):
    """The tap gradients of len(his) (1..3) periodic levels of the 1-D stationary transform along the LAST axis in ONE launch
    (wl_swt1d_tapgrad): s, top (..., n), his = [finest .. coarsest] (None = zeros), the taps k0 / k1 and the per-level scale ->
    (c0, c1), float32 (L,) each, with u_0 = s, u_j = scale A0_j(k0) u_{j-1}, v_J = top, v_{j-1} = scale (A0_j(k0)^T v_j +
    A1_j(k1)^T w_j) and d_j = 2^(j-1):
        c0[t] = scale sum_j sum_p u_{j-1}[p + (t - (L/2 - 1)) d_j] v_j[p],      c1[t] = the same with w_j[p].
    (s, top, his, k, scale) = (x, dlo, dhi, h, 1): the gradients of swt1d_fwd's taps; (dx, lo, hi, g, 1/2): those of swt1d_adj's
    with 1/2 per level.  The launch writes every tile's share, float32 (rows, tiles, 2, L), which is summed over rows and tiles
    in float64.  None when the launcher declines (float64, odd or long filters, more levels, the switch): callers compose.
    `origin` (tests) moves the tile seams."""
    _check_tensor(s, 's')
    _check_tensor(top, 'top')
    _same_device(s, top)
    J, L, n = len(his), k0.numel(), s.shape[-1]
    if top.dtype != s.dtype or top.shape != s.shape:
        raise ValueError('swt1d_tapgrad: top %s %s does not belong to s %s %s' % (tuple(top.shape), top.dtype, tuple(s.shape), s.dtype))
    if not SWT1D_TAPGRAD_FUSED or not _swt1d_covered(s, L, k1.numel(), J):
        return None
    for h in his:
        if h is not None:
            _check_tensor(h, 'his')
            _same_device(s, h)
            if h.dtype != s.dtype or h.shape != s.shape:
                return None
    rows = s.numel() // n
    key = ('swt1d_tapgrad', s.device, s.dtype, rows, n, L, J)
    if key in _FUSED_DECLINED:
        return None
    s, top = s.contiguous(), top.contiguous()
    his = [None if h is None else h.contiguous() for h in his]
    t0, t1 = _taps(k0, s), _taps(k1, s)
    tiles = -(-(n + int(origin)) // swt1d_tapgrad_core(L, J))
    part = torch.empty((rows, tiles, 2, L), dtype=torch.float32, device=s.device)
    if _declined(key, 'wl_swt1d_tapgrad', s, s.data_ptr(), top.data_ptr(), _ptr_array(his), part.data_ptr(), _DTYPES[s.dtype], rows,
                 n, J, t0.data_ptr(), t1.data_ptr(), L, EXT_PERIODIC, float(scale), int(origin), _stream(s)):
        return None
    c = part.sum((0, 1), dtype=torch.float64).to(torch.float32)
    return c[0], c[1]


# ---------------------------------------------------------------------------------------------- shrinkage of the 1-D stationary transform
SHRINK1D_FUSED = True   # SWT1DShrink forward and backward in one launch each on the wave-tile kernels (csrc/wl_shrink1d.h).  False:
#                         SWT1DForward, element-wise torch operations, SWT1DInverse and autograd, for A/B measurements and tests.
SHRINK1D_KINDS = {'soft': 0, 'hard': 1}   # WL_SHRINK_SOFT, WL_SHRINK_HARD


def shrink1d_core(L, J):
    """Positions of a wave's tile the shrinkage kernels store, and what the tiles of a row advance by: the analysis and the
    inverse behind it eat (L - 1)(2^J - 1) positions on either side."""
    return WAVE1D_TILE - 2 * (L - 1) * (2 ** J - 1)


def shrink1d_covered(x, h0, h1, g0, g1, J):
    """What the fused route asks: the switch, the element type, four even filters of one length up to 20 taps, 1..3 levels."""
    L = h0.numel()
    return (SHRINK1D_FUSED and h1.numel() == L and g0.numel() == L and g1.numel() == L
            and _wave1d_covered(x, x.shape[-1], L, L, J))


def _shrink1d_args(x, thr, taps, nlev, kind):
    """(rows, n, L) of a launch, or None outside the envelope of the kernels; thr must be the float32 (nlev, rows) table."""
    L, n = taps[0].numel(), x.shape[-1]
    if kind not in SHRINK1D_KINDS:
        raise ValueError("kind must be 'soft' or 'hard', not {!r}".format(kind))
    if any(t.numel() != L for t in taps) or not _wave1d_covered(x, n, L, L, nlev):
        return None
    rows = x.numel() // n
    if thr.dtype != torch.float32 or thr.numel() != nlev * rows:
        raise ValueError('shrink1d: the thresholds are %s %s, not float32 with %d x %d elements'
                         % (tuple(thr.shape), thr.dtype, nlev, rows))
    _same_device(x, thr)
    return rows, n, L


def shrink1d_fwd(x, thr, h0, h1, g0, g1, nlev, kind='soft', origin=0):
    """Analysis, shrinkage and inverse of `nlev` (1..3) periodic levels of the 1-D stationary transform along the LAST axis in
    ONE launch (wl_shrink1d_forward): x (..., n) and thr, float32 (nlev, rows) -> y (..., n).  None when the launcher declines
    (float64, odd, long or unequal filters, more levels): callers compose.  `origin` (tests) moves the tile seams."""
    _check_tensor(x, 'x')
    geom = _shrink1d_args(x, thr, (h0, h1, g0, g1), nlev, kind)
    if geom is None:
        return None
    rows, n, L = geom
    key = ('shrink1d_fwd', x.device, x.dtype, rows, n, L, nlev)
    if key in _FUSED_DECLINED:
        return None
    x, thr = x.contiguous(), thr.contiguous()
    t = [_taps(h, x) for h in (h0, h1, g0, g1)]
    y = torch.empty_like(x)
    if _declined(key, 'wl_shrink1d_forward', x, x.data_ptr(), y.data_ptr(), thr.data_ptr(), _DTYPES[x.dtype], rows, n, nlev,
                 t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), L, SHRINK1D_KINDS[kind], int(origin), _stream(x)):
        return None
    return y


def shrink1d_bwd(x, dy, thr, h0, h1, g0, g1, nlev, kind='soft', need_dthr=True, origin=0):
    """The backward of shrink1d_fwd in ONE launch (wl_shrink1d_backward), which recomputes the coefficients: x, dy (..., n) and
    thr -> (dx (..., n), dthr_part): dthr_part, float32 (rows, tiles, nlev), holds each tile's share of the threshold
    gradients (zeros for 'hard') - the caller sums over tiles -, or is None without `need_dthr` (the launch then gets a null
    pointer and skips the reduction).  None when the launcher declines."""
    _check_tensor(x, 'x')
    _check_tensor(dy, 'dy')
    _same_device(x, dy)
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise ValueError('shrink1d_bwd: dy %s %s does not belong to x %s %s' % (tuple(dy.shape), dy.dtype, tuple(x.shape), x.dtype))
    geom = _shrink1d_args(x, thr, (h0, h1, g0, g1), nlev, kind)
    if geom is None:
        return None
    rows, n, L = geom
    key = ('shrink1d_bwd', x.device, x.dtype, rows, n, L, nlev)
    if key in _FUSED_DECLINED:
        return None
    x, dy, thr = x.contiguous(), dy.contiguous(), thr.contiguous()
    t = [_taps(h, x) for h in (h0, h1, g0, g1)]
    dx = torch.empty_like(x)
    tiles = -(-(n + int(origin)) // shrink1d_core(L, nlev))
    part = torch.empty((rows, tiles, nlev), dtype=torch.float32, device=x.device) if need_dthr else None
    if _declined(key, 'wl_shrink1d_backward', x, x.data_ptr(), dy.data_ptr(), dx.data_ptr(), thr.data_ptr(),
                 part.data_ptr() if need_dthr else None, _DTYPES[x.dtype], rows, n, nlev, t[0].data_ptr(), t[1].data_ptr(),
                 t[2].data_ptr(), t[3].data_ptr(), L, SHRINK1D_KINDS[kind], int(origin), _stream(x)):
        return None
    return dx, part


# ---------------------------------------------------------------------------------------------- the 1-D scattering layer
SCAT1D_FUSED = True   # ScatLayer1D forward and backward in one launch each on the wave-tile kernels (csrc/wl_scat1d.h).  False:
#                       level 1 of the 1-D DTCWT plus element-wise torch operations and autograd, for A/B measurements and tests.
SCAT1D_PAIRS = ((5, 7), (5, 3), (13, 19), (9, 7))   # (L0, L1) the kernels are instantiated for: near_sym_a, legall, near_sym_b, antonini
# (no row is too short for the fused route: one wave serves one row, but it still wins 3.7x at rows of 64 samples, the shortest
# measured - DESIGN.md 4.30)


def scat1d_core(L0, L1):
    """Positions of a wave's tile the scattering kernels store, and what the tiles of a row advance by: the tile less the halo
    of the longer filter, rounded up to even, on either side."""
    return WAVE1D_TILE - 2 * ((max(L0, L1) // 2 + 1) // 2 * 2)


def scat1d_covered(x, h0o, h1o):
    """What the fused route asks: the switch, the element type, an instantiated tap pair, a row the kernels can index."""
    return (SCAT1D_FUSED and x.dtype != torch.float64 and (h0o.numel(), h1o.numel()) in SCAT1D_PAIRS and x.numel() != 0
            and x.shape[-1] < 1 << 29)


def scat1d_fwd(x, h0o, h1o, magbias, save, origin=0):
    """ScatLayer1D in ONE launch (wl_scat1d_forward): x (N, C, n) -> (Z (N, 2C, ceil(n/2)), dir): Z = [pair means of the lowpass
    x C, smoothed magnitudes of the highpass pairs x C]; dir (N, C, n + n % 2) = the pairs over their root, what the backward
    needs, or None without `save`.  None when the launcher declines (float64, other tap counts): callers compose the 1-D DTCWT.
    `origin` (tests) moves the tile seams."""
    _check_tensor(x, 'x')
    L0, L1 = h0o.numel(), h1o.numel()
    if x.ndim != 3 or x.dtype == torch.float64 or (L0, L1) not in SCAT1D_PAIRS or x.numel() == 0 or x.shape[-1] >= 1 << 29:
        return None
    N, C, n = x.shape
    key = ('scat1d_fwd', x.device, x.dtype, N, C, n, L0, L1)
    if key in _FUSED_DECLINED:
        return None
    x = x.contiguous()
    t0, t1 = _taps(h0o, x), _taps(h1o, x)
    ne = n + n % 2
    z = torch.empty((N, 2 * C, ne // 2), dtype=x.dtype, device=x.device)
    d = torch.empty((N, C, ne), dtype=x.dtype, device=x.device) if save else None
    if _declined(key, 'wl_scat1d_forward', x, x.data_ptr(), z.data_ptr(), d.data_ptr() if save else None, _DTYPES[x.dtype], N, C, n,
                 t0.data_ptr(), L0, t1.data_ptr(), L1, float(magbias), int(origin), _stream(x)):
        return None
    return z, d


def scat1d_bwd(dz, d, h0o, h1o, n, origin=0):
    """The backward of scat1d_fwd in ONE launch (wl_scat1d_backward): dz (N, 2C, ceil(n/2)) and the saved dir -> dx (N, C, n) by
    the reference's rule (ScatLayerj1_f.backward on one axis).  None when the launcher declines."""
    _check_tensor(dz, 'dz')
    _same_device(dz, d)
    L0, L1 = h0o.numel(), h1o.numel()
    N, C, ne = d.shape
    if dz.dtype != d.dtype or tuple(dz.shape) != (N, 2 * C, ne // 2) or ne != n + n % 2:
        raise ValueError('scat1d_bwd: dz %s %s does not belong to dir %s %s of rows of %d samples'
                         % (tuple(dz.shape), dz.dtype, tuple(d.shape), d.dtype, n))
    if dz.dtype == torch.float64 or (L0, L1) not in SCAT1D_PAIRS or dz.numel() == 0 or n >= 1 << 29:
        return None
    key = ('scat1d_bwd', dz.device, dz.dtype, N, C, n, L0, L1)
    if key in _FUSED_DECLINED:
        return None
    dz, d = dz.contiguous(), d.contiguous()
    t0, t1 = _taps(h0o, dz), _taps(h1o, dz)
    dx = torch.empty((N, C, n), dtype=dz.dtype, device=dz.device)
    if _declined(key, 'wl_scat1d_backward', dz, dz.data_ptr(), d.data_ptr(), dx.data_ptr(), _DTYPES[dz.dtype], N, C, n,
                 t0.data_ptr(), L0, t1.data_ptr(), L1, 0.0, int(origin), _stream(dz)):
        return None
    return dx


# ---------------------------------------------------------------------------------------------- the 2-D wavelet packet level
WPT_FUSED = True  # two packet levels per launch where the kernels take them (periodization, sizes multiples of 4, <= 12 taps):
#                    measured ahead of one launch per level.  False: everything level by level, for A/B measurements.


def _wpt_taps(t, taps):
    """The four tap vectors for a packet launch (the C entry takes ONE tap count), or None when they differ in length."""
    L = taps[0].numel()
    if t.numel() == 0 or any(h.numel() != L for h in taps):
        return None
    return [_taps(h, t) for h in taps]


def wpt2d_afb(x, h_w_lo, h_w_hi, h_h_lo, h_h_hi, mode, nlev=1):
    """`nlev` (1 or 2) packet analysis levels in ONE launch (wl_wpt2d_analysis): x (N,C,H,W) -> y (N,C,4**nlev,Kh,Kw) dense, band
    s = 2 b_W + b_H of a level (DWTForward's order), level 1 the most significant digit of the band index.  x may be any view
    with uniformly spaced planes and unit column stride (the previous level's y as (N,4C,Kh,Kw) is one); anything else is copied.
    None when the launcher declines (its envelope: include/wavelets_hip.h) or the tap counts differ: callers run afb2d per level."""
    _check_tensor(x, 'x')
    t = _wpt_taps(x, (h_w_lo, h_w_hi, h_h_lo, h_h_hi))
    if t is None:
        return None
    N, C, H, W = x.shape
    L = t[0].numel()
    x, x_ps, x_rs = _planes(x)
    key = ('wpt_afb', x.device, x.dtype, N * C, H, W, x_ps, x_rs, L, mode, nlev)
    if key in _FUSED_DECLINED:
        return None
    Kh, Kw = H, W
    for _ in range(nlev):
        Kh, Kw = coeff_len(Kh, L, mode), coeff_len(Kw, L, mode)
    y = torch.empty((N, C, 4 ** nlev, Kh, Kw), dtype=x.dtype, device=x.device)
    if _declined(key, 'wl_wpt2d_analysis', x, x.data_ptr(), x_ps, x_rs, y.data_ptr(), _DTYPES[x.dtype], N * C, H, W, nlev,
                 t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), L, mode, _stream(x)):
        return None
    return y


def wpt2d_sfb(y, g_w_lo, g_w_hi, g_h_lo, g_h_hi, mode, out_hw=None, nlev=1):
    """`nlev` (1 or 2) packet synthesis levels in ONE launch (wl_wpt2d_synthesis): y (N,C,4**nlev,Kh,Kw) -> x (N,C,OH,OW), the
    natural size of the synthesis or the crop out_hw = (OH, OW).  y is read dense (a view is copied once).  None when the launcher
    declines or the tap counts differ: callers run sfb2d per level."""
    _check_tensor(y, 'y')
    N, C, B, Kh, Kw = y.shape
    if B != 4 ** nlev:
        raise ValueError('wpt2d_sfb: %d bands are not the 4**%d of %d level(s)' % (B, nlev, nlev))
    t = _wpt_taps(y, (g_w_lo, g_w_hi, g_h_lo, g_h_hi))
    if t is None:
        return None
    L = t[0].numel()
    OH, OW = Kh, Kw
    for _ in range(nlev):
        OH, OW = synth_len(OH, L, mode), synth_len(OW, L, mode)
    if out_hw is not None:
        OH, OW = min(OH, out_hw[0]), min(OW, out_hw[1])
    if OH < 1 or OW < 1:
        return None
    key = ('wpt_sfb', y.device, y.dtype, N * C, Kh, Kw, OH, OW, L, mode, nlev)
    if key in _FUSED_DECLINED:
        return None
    y = y.contiguous()
    x = torch.empty((N, C, OH, OW), dtype=y.dtype, device=y.device)
    if _declined(key, 'wl_wpt2d_synthesis', y, y.data_ptr(), x.data_ptr(), _DTYPES[y.dtype], N * C, Kh, Kw, OH, OW, nlev,
                 t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), L, mode, _stream(y)):
        return None
    return x


# ---------------------------------------------------------------------------------------------- the 1-D wavelet packet transform
WPT1D_FUSED = True   # up to three periodization levels of the packet tree per launch on the wave-tile kernels (csrc/wl_wpt1d.h).
#                      False: everything level by level on afb1d / sfb1d, for A/B measurements and tests.
WPT1D_MAXJ = WAVE1D_MAXJ


def wpt1d_core(L, J):
    """Positions of a wave's tile that are stored after J packet levels of an L-tap bank, and what the tiles of a row advance
    by (the seams of a row lie at multiples of it, minus `origin`): the tile less a halo of (L/2)(2^J - 1) positions, rounded
    up to a multiple of 2^J, on either side."""
    q = 2 ** J
    return WAVE1D_TILE - 2 * (((L // 2) * (q - 1) + q - 1) // q * q)


def _wpt1d_covered(t, n, L, L1, mode, nlev):
    """The envelope of wl_wpt1d_analysis / wl_wpt1d_synthesis for rows of n samples (include/wavelets_hip.h)."""
    return _wave1d_covered(t, n, L, L1, nlev) and mode == 2 and n % 2 ** nlev == 0 and n >> (nlev - 1) >= L


def wpt1d_afb(x, h0, h1, mode, nlev, origin=0):
    """`nlev` (1..3) levels of the periodized packet analysis along the LAST axis in ONE launch (wl_wpt1d_analysis):
    x (..., n) -> y (..., 2**nlev, n / 2**nlev), band b = sum_j s_j 2**(nlev-j), s_j = 1 the highpass of level j.  None when the
    launcher declines (another mode, n no multiple of 2**nlev, a last level shorter than the filter, float64, odd, long or
    unequal filters): callers go level by level on afb1d.  `origin` (tests; a multiple of 2**nlev) moves the tile seams."""
    _check_tensor(x, 'x')
    L, n = h0.numel(), x.shape[-1]
    if not _wpt1d_covered(x, n, L, h1.numel(), mode, nlev):
        return None
    rows = x.numel() // n
    key = ('wpt1d_afb', x.device, x.dtype, rows, n, L, nlev)
    if key in _FUSED_DECLINED:
        return None
    x = x.contiguous()
    t0, t1 = _taps(h0, x), _taps(h1, x)
    y = torch.empty(tuple(x.shape[:-1]) + (2 ** nlev, n >> nlev), dtype=x.dtype, device=x.device)
    if _declined(key, 'wl_wpt1d_analysis', x, x.data_ptr(), y.data_ptr(), _DTYPES[x.dtype], rows, n, nlev, t0.data_ptr(),
                 t1.data_ptr(), L, mode, int(origin), _stream(x)):
        return None
    return y


def wpt1d_sfb(y, g0, g1, mode, nlev, origin=0):
    """The transpose of wpt1d_afb in ONE launch (wl_wpt1d_synthesis): y (..., 2**nlev, m) -> x (..., 2**nlev * m) - the inverse
    with the stored synthesis taps, the backward of the analysis with its own.  None when the launcher declines."""
    _check_tensor(y, 'y')
    if y.dim() < 2 or y.shape[-2] != 2 ** nlev:
        raise ValueError('wpt1d_sfb: %s is no (..., 2**%d, m) tensor' % (tuple(y.shape), nlev))
    L, n = g0.numel(), y.shape[-1] << nlev
    if not _wpt1d_covered(y, n, L, g1.numel(), mode, nlev):
        return None
    rows = y.numel() // n
    key = ('wpt1d_sfb', y.device, y.dtype, rows, n, L, nlev)
    if key in _FUSED_DECLINED:
        return None
    y = y.contiguous()
    t0, t1 = _taps(g0, y), _taps(g1, y)
    x = torch.empty(tuple(y.shape[:-2]) + (n,), dtype=y.dtype, device=y.device)
    if _declined(key, 'wl_wpt1d_synthesis', y, y.data_ptr(), x.data_ptr(), _DTYPES[y.dtype], rows, n, nlev, t0.data_ptr(),
                 t1.data_ptr(), L, mode, int(origin), _stream(y)):
        return None
    return x


# ---------------------------------------------------------------------------------------------- DTCWT
def dtcwt_fwd1(x, h0, h1, mode, skip_hps=False):
    """Level-1 forward: x (N,C,H,W) -> ll (N,C,He,We), highs (N,C,6,He/2,We/2,2) or None."""
    _check_tensor(x, 'x')
    x = x.contiguous()
    N, C, H, W = x.shape
    t0, t1 = _taps(h0, x), _taps(h1, x)
    He, We = H + (H & 1), W + (W & 1)
    ll = torch.empty((N, C, He, We), dtype=x.dtype, device=x.device)
    highs = None if skip_hps else torch.empty((N, C, 6, He // 2, We // 2, 2), dtype=x.dtype, device=x.device)
    rc = _call('wl_dtcwt_fwd_level1', x, x.data_ptr(), ll.data_ptr(), None if skip_hps else highs.data_ptr(),
                                        _DTYPES[x.dtype], N * C, H, W, t0.data_ptr(), t0.numel(), t1.data_ptr(),
                                        t1.numel(), mode, _stream(x))
    _lib.check(rc, 'wl_dtcwt_fwd_level1')
    return ll, highs


def dtcwt_fwd1_rot(x, h0, h1, h2, symmetric, scat=False, magbias=0.0):
    """Level 1 with the band-pass diagonal in one launch (wl_dtcwt_fwd_level1_rot): x (N,C,H,W) -> (ll (N,C,H,W),
    re (N,6,C,H/2,W/2), im) - or, scat=True, Z (N,7,C,H/2,W/2) of ScatLayerj1_rot_f.forward.  None when the kernel does
    not cover the configuration (odd sizes, filters longer than 19 taps): callers chain the single-axis filters."""
    _check_tensor(x, 'x')
    if x.dim() != 4 or x.numel() == 0:
        return None
    N, C, H, W = x.shape
    key = ('dtrot', x.device, x.dtype, N, C, H, W, h0.numel(), h1.numel(), h2.numel(), bool(symmetric), bool(scat))
    if key in _FUSED_DECLINED:
        return None
    x = x.contiguous()
    t0, t1, t2 = _taps(h0, x), _taps(h1, x), _taps(h2, x)
    h2_, w2_ = H // 2, W // 2
    if scat:
        ll = im = None
        re = torch.empty((N, 7, C, h2_, w2_), dtype=x.dtype, device=x.device)
    else:
        ll = torch.empty((N, C, H, W), dtype=x.dtype, device=x.device)
        re = torch.empty((N, 6, C, h2_, w2_), dtype=x.dtype, device=x.device)
        im = torch.empty_like(re)
    if _declined(key, 'wl_dtcwt_fwd_level1_rot', x, x.data_ptr(), None if ll is None else ll.data_ptr(), re.data_ptr(),
                 None if im is None else im.data_ptr(), _DTYPES[x.dtype], N, C, H, W, t0.data_ptr(), t0.numel(), t1.data_ptr(),
                 t1.numel(), t2.data_ptr(), t2.numel(), 1 if symmetric else 0, 1 if scat else 0, float(magbias), _stream(x)):
        return None
    return re if scat else (ll, re, im)


def dtcwt_fwd12(x, h0o, h1o, h0a, h0b, h1a, h1b, mode, force=False):
    """Levels 1 and 2 of the forward in one launch (wl_dtcwt_fwd_level12: the level-1 lowpass stays on chip):
    x (N,C,H,W) -> (highs1 (N,C,6,H/2,W/2,2), ll2 (N,C,H/2,W/2), highs2 (N,C,6,H/4,W/4,2)), or None when the engine
    declines (callers chain dtcwt_fwd1 / dtcwt_fwd2).  Exact for any taps (csrc/wl_dtcwt_fused.h: the rows above / below the
    plane meet the column lowpass taps in reverse order, so no symmetry of h0o is assumed)."""
    _check_tensor(x, 'x')
    N, C, H, W = x.shape
    if mode != 1 or H % 4 or W % 4 or x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        return None
    force = force or STREAM_FORCE
    key = ('dt12', x.device, x.dtype, N * C, H, W, h0o.numel(), h1o.numel(), h0a.numel(), mode)
    if not force and key in _FUSED_DECLINED:
        return None
    x = x.contiguous()
    t0, t1 = _taps(h0o, x), _taps(h1o, x)
    ta, tb, tc, td = (_taps(h, x) for h in (h0a, h0b, h1a, h1b))
    highs1 = torch.empty((N, C, 6, H // 2, W // 2, 2), dtype=x.dtype, device=x.device)
    ll2 = torch.empty((N, C, H // 2, W // 2), dtype=x.dtype, device=x.device)
    highs2 = torch.empty((N, C, 6, H // 4, W // 4, 2), dtype=x.dtype, device=x.device)
    # (a decline is remembered - unless it is the streaming kernels being switched off for a test / an A/B run)
    if _declined(key, 'wl_dtcwt_fwd_level12', x, x.data_ptr(), highs1.data_ptr(), ll2.data_ptr(), highs2.data_ptr(),
                 _DTYPES[x.dtype], N * C, H, W, t0.data_ptr(), t0.numel(), t1.data_ptr(), t1.numel(), ta.data_ptr(),
                 tb.data_ptr(), tc.data_ptr(), td.data_ptr(), ta.numel(), mode, 1 if force else 0, _stream(x), memo=not force):
        return None
    return highs1, ll2, highs2


def dtcwt_fwd2(x, h0a, h0b, h1a, h1b, skip_hps=False):
    """Level>=2 forward: x (N,C,H,W), H,W even -> ll (N,C,He/2,We/2), highs (N,C,6,He/4,We/4,2) or None."""
    _check_tensor(x, 'x')
    x = x.contiguous()
    N, C, H, W = x.shape
    ta, tb, tc, td = (_taps(h, x) for h in (h0a, h0b, h1a, h1b))
    He, We = H + (2 if H % 4 else 0), W + (2 if W % 4 else 0)
    ll = torch.empty((N, C, He // 2, We // 2), dtype=x.dtype, device=x.device)
    highs = None if skip_hps else torch.empty((N, C, 6, He // 4, We // 4, 2), dtype=x.dtype, device=x.device)
    rc = _call('wl_dtcwt_fwd_level2', x, x.data_ptr(), ll.data_ptr(), None if skip_hps else highs.data_ptr(),
                                        _DTYPES[x.dtype], N * C, H, W, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(),
                                        td.data_ptr(), ta.numel(), _stream(x))
    _lib.check(rc, 'wl_dtcwt_fwd_level2')
    return ll, highs


def dtcwt_inv1(ll, highs, g0, g1, mode):
    """Level-1 inverse: ll (N,C,H,W) or None, highs (N,C,6,H/2,W/2,2) or None -> y (N,C,H,W)."""
    ref = ll if ll is not None else highs
    _check_tensor(ref, 'coeffs')
    if highs is not None:
        highs = highs.contiguous()
        N, C = highs.shape[:2]
        H, W = 2 * highs.shape[3], 2 * highs.shape[4]
    else:
        N, C, H, W = ll.shape
    ps = rs = 0
    if ll is not None:
        if tuple(ll.shape) != (N, C, H, W):
            raise ValueError('lowpass %s does not match the highpass size %s' % (tuple(ll.shape), (N, C, H, W)))
        _same_device(ll, highs)
        ll, ps, rs = _planes(ll)
    t0, t1 = _taps(g0, ref), _taps(g1, ref)
    y = torch.empty((N, C, H, W), dtype=ref.dtype, device=ref.device)
    rc = _call('wl_dtcwt_inv_level1', ref, None if ll is None else ll.data_ptr(), ps, rs,
                                        None if highs is None else highs.data_ptr(), y.data_ptr(),
                                        _DTYPES[ref.dtype], N * C, H, W, t0.data_ptr(), t0.numel(), t1.data_ptr(),
                                        t1.numel(), mode, _stream(ref))
    _lib.check(rc, 'wl_dtcwt_inv_level1')
    return y


def dtcwt_inv2(ll, highs, g0a, g0b, g1a, g1b):
    """Level>=2 inverse: ll (N,C,h,w) or None, highs (N,C,6,h/2,w/2,2) or None -> y (N,C,2h,2w)."""
    ref = ll if ll is not None else highs
    _check_tensor(ref, 'coeffs')
    if highs is not None:
        highs = highs.contiguous()
        N, C = highs.shape[:2]
        h, w = 2 * highs.shape[3], 2 * highs.shape[4]
    else:
        N, C, h, w = ll.shape
    ps = rs = 0
    if ll is not None:
        if tuple(ll.shape) != (N, C, h, w):
            raise ValueError('lowpass %s does not match the highpass size %s' % (tuple(ll.shape), (N, C, h, w)))
        _same_device(ll, highs)
        ll, ps, rs = _planes(ll)
    ta, tb, tc, td = (_taps(g, ref) for g in (g0a, g0b, g1a, g1b))
    y = torch.empty((N, C, 2 * h, 2 * w), dtype=ref.dtype, device=ref.device)
    rc = _call('wl_dtcwt_inv_level2', ref, None if ll is None else ll.data_ptr(), ps, rs,
                                        None if highs is None else highs.data_ptr(), y.data_ptr(),
                                        _DTYPES[ref.dtype], N * C, h, w, ta.data_ptr(), tb.data_ptr(), tc.data_ptr(),
                                        td.data_ptr(), ta.numel(), _stream(ref))
    _lib.check(rc, 'wl_dtcwt_inv_level2')
    return y


def dtcwt_inv21(ll2, highs2, highs1, g0o, g1o, g0a, g0b, g1a, g1b, mode, force=False):
    """Levels 2 and 1 of the inverse in one launch (wl_dtcwt_inv_level21: the level-1 lowpass stays on chip):
    ll2 (N,C,h,w) [may be a strided crop], highs2 (N,C,6,h/2,w/2,2), highs1 (N,C,6,h,w,2) -> y (N,C,2h,2w), or None when the
    engine declines (callers chain dtcwt_inv2 / dtcwt_inv1)."""
    _check_tensor(ll2, 'll2')
    if highs2 is None or highs1 is None or highs1.dim() != 6 or highs2.dim() != 6:
        return None
    N, C, h, w = ll2.shape
    if (mode != 1 or h % 2 or w % 2 or ll2.dtype not in (torch.float32, torch.float16, torch.bfloat16) or highs1.dtype != ll2.dtype
            or highs2.dtype != ll2.dtype or tuple(highs2.shape) != (N, C, 6, h // 2, w // 2, 2)
            or tuple(highs1.shape) != (N, C, 6, h, w, 2) or ll2.numel() == 0):
        return None
    force = force or STREAM_FORCE
    _same_device(ll2, highs2, highs1)
    ll2, ps, rs = _planes(ll2)
    key = ('dti21', ll2.device, ll2.dtype, N * C, h, w, ps, rs, g0o.numel(), g1o.numel(), g0a.numel(), mode)
    if not force and key in _FUSED_DECLINED:
        return None
    highs2, highs1 = highs2.contiguous(), highs1.contiguous()
    # the kernel loads pairs of elements (wl_dtinv21_any): a base that is not on 2 * sizeof(T) - a view one element into its
    # buffer - is that tensor's affair, not the configuration's, and is declined here, where the memo does not hear of it
    pair = 2 * ll2.element_size()
    if ll2.data_ptr() % pair or highs2.data_ptr() % pair or highs1.data_ptr() % pair:
        return None
    t0, t1 = _taps(g0o, ll2), _taps(g1o, ll2)
    ta, tb, tc, td = (_taps(g, ll2) for g in (g0a, g0b, g1a, g1b))
    y = torch.empty((N, C, 2 * h, 2 * w), dtype=ll2.dtype, device=ll2.device)
    if _declined(key, 'wl_dtcwt_inv_level21', ll2, ll2.data_ptr(), ps, rs, highs2.data_ptr(), highs1.data_ptr(), y.data_ptr(),
                 _DTYPES[ll2.dtype], N * C, 2 * h, 2 * w, t0.data_ptr(), t0.numel(), t1.data_ptr(), t1.numel(), ta.data_ptr(),
                 tb.data_ptr(), tc.data_ptr(), td.data_ptr(), ta.numel(), mode, 1 if force else 0, _stream(ll2), memo=not force):
        return None
    return y


def scat_fwd1(x, h0, h1, mode, magbias, combine_colour, save, want_ll=False):
    """ScatLayer forward: x (N,C,H,W) -> Z (N,7,C,He/2,We/2) [(N,9,..) when combining colour] and, if
    `save`, (re/r, im/r) of shape (N,6,C,He/2,We/2); with `want_ll` also the full-resolution level-1 lowpass
    (N,C,He,We) from the same launch (ScatLayerj2's second scale filters it)."""
    _check_tensor(x, 'x')
    x = x.contiguous()
    N, C, H, W = x.shape
    t0, t1 = _taps(h0, x), _taps(h1, x)
    h2, w2 = (H + (H & 1)) // 2, (W + (W & 1)) // 2
    z = torch.empty((N, 9, h2, w2) if combine_colour else (N, 7, C, h2, w2), dtype=x.dtype, device=x.device)
    dx = dy = ll = None
    if save:
        dx = torch.empty((N, 6, C, h2, w2), dtype=x.dtype, device=x.device)
        dy = torch.empty_like(dx)
    if want_ll:
        ll = torch.empty((N, C, 2 * h2, 2 * w2), dtype=x.dtype, device=x.device)
    rc = _call('wl_scat_fwd_level1', x, x.data_ptr(), z.data_ptr(), None if dx is None else dx.data_ptr(),
               None if dy is None else dy.data_ptr(), None if ll is None else ll.data_ptr(), _DTYPES[x.dtype], N, C, H, W,
               t0.data_ptr(), t0.numel(), t1.data_ptr(), t1.numel(), mode, float(magbias),
               1 if combine_colour else 0, _stream(x))
    _lib.check(rc, 'wl_scat_fwd_level1')
    return (z, dx, dy, ll) if want_ll else (z, dx, dy)


def scat_fwd1_into(x, z, z_bs, z_ll_off, z_mag_off, h0, h1, mode, magbias, ll=None):
    """ScatLayer forward of x (N,C,H,W; H, W even) with its entries written into the caller's tensor `z` (contiguous): for
    image n, channel c the averaged lowpass at element n z_bs + z_ll_off + c q, magnitude o at n z_bs + z_mag_off + (o C + c) q,
    q = (H/2)(W/2) (z_ll_off < 0: no lowpass entry); `ll` (N,C,H,W, optional) receives the full-resolution lowpass (wl_scat_fwd_level1_into)."""
    _check_tensor(x, 'x')
    x = x.contiguous()
    N, C, H, W = x.shape
    q = (H // 2) * (W // 2)
    assert H % 2 == 0 and W % 2 == 0 and z.is_contiguous() and z.dtype == x.dtype and z.device == x.device
    last = (N - 1) * z_bs + max(z_ll_off + C * q, z_mag_off + 6 * C * q)
    assert N == 0 or (min(z_bs, z_mag_off) >= 0 and last <= z.numel()), 'entries outside z'
    t0, t1 = _taps(h0, x), _taps(h1, x)
    rc = _call('wl_scat_fwd_level1_into', x, x.data_ptr(), z.data_ptr(), z_bs, z_ll_off, z_mag_off,
               None if ll is None else ll.data_ptr(), _DTYPES[x.dtype], N, C, H, W, t0.data_ptr(), t0.numel(), t1.data_ptr(),
               t1.numel(), mode, float(magbias), _stream(x))
    _lib.check(rc, 'wl_scat_fwd_level1_into')


def scat_fwd2_into(x, z, z_bs, z_ll_off, z_mag_off, h0a, h0b, h1a, h1b, magbias):
    """Second scale of ScatLayerj2: fwd_j2plus of x (N,C,H,W; H, W multiples of 4), the 2x2 average of its lowpass and the
    smoothed magnitudes of its band-pass coefficients written into `z` like scat_fwd1_into (q = (H/4)(W/4)).  Returns False
    when the engine has no kernel for these taps / sizes (callers compose dtcwt_fwd2 + their own epilogue)."""
    _check_tensor(x, 'x')
    x = x.contiguous()
    N, C, H, W = x.shape
    q = (H // 4) * (W // 4)
    assert z.is_contiguous() and z.dtype == x.dtype and z.device == x.device
    last = (N - 1) * z_bs + max(z_ll_off + C * q, z_mag_off + 6 * C * q)
    assert N == 0 or (min(z_bs, z_ll_off, z_mag_off) >= 0 and last <= z.numel()), 'entries outside z'
    key = ('scat2', x.device, x.dtype, N, C, H, W, int(h0a.numel()), z_bs, z_ll_off, z_mag_off)
    if H % 4 or W % 4 or key in _FUSED_DECLINED:
        return False
    ta, tb, tc, td = (_taps(h, x) for h in (h0a, h0b, h1a, h1b))
    return not _declined(key, 'wl_scat_fwd_level2_into', x, x.data_ptr(), z.data_ptr(), z_bs, z_ll_off, z_mag_off, _DTYPES[x.dtype], N, C, H, W,
                         ta.data_ptr(), tb.data_ptr(), tc.data_ptr(), td.data_ptr(), ta.numel(), float(magbias), _stream(x))


def scat_bwd1(dz, drdx, drdy, h0, h1, mode, combine_colour):
    """ScatLayer backward in one launch: dz (gradient of Z), the saved re/r, im/r -> dx (N,C,He,We) (padded size).
    Returns None when the engine has no specialised kernel for these taps / dtype (callers compose the prologue
    and call dtcwt_inv1 instead)."""
    _check_tensor(dz, 'dz')
    dz = dz.contiguous()
    N, _, C, h2, w2 = drdx.shape
    if drdy.shape != drdx.shape or drdx.dtype != dz.dtype or drdy.dtype != dz.dtype:
        raise ValueError('scat_bwd1: drdx %s / drdy %s / dz dtype mismatch' % (tuple(drdx.shape), tuple(drdy.shape)))
    want = (N, 9, h2, w2) if combine_colour else (N, 7, C, h2, w2)
    if tuple(dz.shape) != want:
        raise ValueError('scat_bwd1: dz %s, expected %s' % (tuple(dz.shape), want))
    _same_device(dz, drdx, drdy)
    drdx, drdy = drdx.contiguous(), drdy.contiguous()
    t0, t1 = _taps(h0, dz), _taps(h1, dz)
    dx = torch.empty((N, C, 2 * h2, 2 * w2), dtype=dz.dtype, device=dz.device)
    if _declined(None, 'wl_scat_bwd_level1', dz, dz.data_ptr(), drdx.data_ptr(), drdy.data_ptr(), dx.data_ptr(), _DTYPES[dz.dtype],
                 N, C, 2 * h2, 2 * w2, t0.data_ptr(), t0.numel(), t1.data_ptr(), t1.numel(), mode,
                 1 if combine_colour else 0, _stream(dz), memo=False):
        return None
    return dx
