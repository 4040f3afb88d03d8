"""Shared checks of the 3-D DWT (DWT3DForward / DWT3DInverse, ops.afb_depth / ops.sfb_depth and the streaming depth kernels of
csrc/wl_dwt3d.h), run by the emulator (CPU) and the GPU test modules.

The expected answer is a numpy composition of the pinned per-axis oracle (``wo.afb1d`` / ``wo.sfb1d`` with ``axis=``): W, then H,
then D for the analysis, D, then H, then W for the synthesis; band s = 4 b_D + 2 b_W + b_H.  Gradients follow the reference's
rule for its 2-D transform (quirk Q9, oracle/wavelet_oracle.py): the backward of an analysis level is the synthesis with the
ANALYSIS taps cropped to the level's input, the backward of a synthesis level the analysis with the SYNTHESIS taps.

Tolerances (tests/_swt_inv_cases.py, tests/test_dwt_gpu.py, tests/_bf16_cases.py): float32 relative error below 1e-5 of
|ref|max; float16 3e-3 max(1, |ref|max); float64 1e-12 max(1, |ref|max); bfloat16 relative to |ref|max 4e-3 for a single rounding
to bfloat16 (one launch of a depth kernel) and 3e-2 for everything else (the modules: every 3-D level rounds twice, after the
2-D stage and after the depth stage) - the 2-byte types against the oracle on the rounded inputs with the float32 taps the
modules hold."""
import numpy as np
import torch

import pytorch_wavelets_amd as pw
from oracle import wavelet_oracle as wo
from pytorch_wavelets_amd import filters, ops
from pytorch_wavelets_amd.dwt import lowlevel as dwl

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
MODES = ('zero', 'symmetric', 'reflect', 'periodization', 'periodic')
BF_ONE, BF_MULTI = 4e-3, 3e-2
# pywt.dwtn keys over the axes (D, H, W) of band s = 1..7 (a: lowpass, d: highpass)
KEYS = {1: 'ada', 2: 'aad', 3: 'add', 4: 'daa', 5: 'dda', 6: 'dad', 7: 'ddd'}
TNAME = {F32: 'float', F16: '_Float16', BF16: '__bf16'}


def npy(t):
    return t.detach().cpu().double().numpy()


def taps(wave, syn=False, f32=False):
    """(lo, hi) as the oracle takes them: the stored analysis taps (reversed) or the synthesis taps; f32: rounded to float32,
    as a float32 module holds them."""
    t = filters.dwt_synthesis_taps(wave) if syn else filters.dwt_analysis_taps(wave)
    t = tuple(np.asarray(v, dtype=np.float64) for v in t)
    return tuple(v.astype(np.float32).astype(np.float64) for v in t) if f32 else t


def banks(wave, syn=False, f32=False):
    """Per-axis taps (depth, W, H) of `wave`: a name for the three axes or (depth name, in-plane name)."""
    wd, wp = (wave, wave) if isinstance(wave, str) else wave
    return taps(wd, syn, f32), taps(wp, syn, f32), taps(wp, syn, f32)


def level_ref(x, bk, mode):
    """One analysis level in numpy: x (N,C,D,H,W) -> the eight bands, index s = 4 b_D + 2 b_W + b_H."""
    hd, hw, hh = bk
    out = [None] * 8
    for bw, xw in enumerate(wo.afb1d(x, hw[0], hw[1], mode, axis=4)):
        for bh, xh in enumerate(wo.afb1d(xw, hh[0], hh[1], mode, axis=3)):
            for bd, xd in enumerate(wo.afb1d(xh, hd[0], hd[1], mode, axis=2)):
                out[4 * bd + 2 * bw + bh] = xd
    return out


def fwd_ref(x, J, bk, mode):
    yh, ll = [], np.asarray(x)
    for _ in range(J):
        b = level_ref(ll, bk, mode)
        ll = b[0]
        yh.append(np.stack(b[1:], axis=2))
    return ll, yh


def unlevel_ref(b, bk, mode, crop=None):
    """One synthesis level in numpy: the eight bands -> (N,C,D,H,W); crop = (D, H, W) or None."""
    gd, gw, gh = bk
    p = [wo.sfb1d(b[q], b[4 + q], gd[0], gd[1], mode, axis=2) for q in range(4)]
    lo = wo.sfb1d(p[0], p[1], gh[0], gh[1], mode, axis=3)
    hi = wo.sfb1d(p[2], p[3], gh[0], gh[1], mode, axis=3)
    y = wo.sfb1d(lo, hi, gw[0], gw[1], mode, axis=4)
    return y if crop is None else y[:, :, :crop[0], :crop[1], :crop[2]]


def inv_ref(yl, yh, bk, mode):
    ll = np.asarray(yl)
    for h in yh[::-1]:
        if h is None:
            h = np.zeros(ll.shape[:2] + (7,) + ll.shape[2:])
        ll = ll[:, :, :h.shape[3], :h.shape[4], :h.shape[5]]
        ll = unlevel_ref([ll] + [h[:, :, i] for i in range(7)], bk, mode)
    return ll


def fwd_grad_ref(dyl, dyh, in_shapes, bk, mode):
    """dx of the forward by the Q9 rule: in_shapes[j] = (D, H, W) of the input of level j; bk = the ANALYSIS taps."""
    d = dyl
    for h, shp in zip(dyh[::-1], in_shapes[::-1]):
        d = unlevel_ref([d] + [h[:, :, i] for i in range(7)], bk, mode, crop=shp)
    return d


def inv_grad_ref(dy, lo_shapes, bk, mode):
    """(dyl, [dyh_j]) of the inverse: lo_shapes[j] = (D, H, W) of the low-pass handed to level j before its 'unpad' (a dropped
    sample gets a zero gradient); bk = the SYNTHESIS taps."""
    d, grads = dy, []
    for shp in lo_shapes:
        b = level_ref(d, bk, mode)
        grads.append(np.stack(b[1:], axis=2))
        d = b[0]
        d = np.pad(d, [(0, 0), (0, 0)] + [(0, s - k) for s, k in zip(shp, d.shape[2:])])
    return d, grads


def close(a, ref, dtype, what='', chain=False):
    a = npy(a) if isinstance(a, torch.Tensor) else a
    assert tuple(a.shape) == tuple(ref.shape), (what, a.shape, ref.shape)
    err, top = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    bound = {F64: 1e-12 * max(1.0, top), F32: 1e-5 * top, F16: 3e-3 * max(1.0, top),
             BF16: (BF_MULTI if chain else BF_ONE) * top}[dtype]
    print('%s %s: max err %.3e, bound %.3e' % (what, dtype, err, bound))
    assert err <= bound, (what, err, bound)


def modules(dev, wave, J, mode, dtype=F32):
    """(DWT3DForward, DWT3DInverse) whose buffers are float64 for float64 data, float32 otherwise; wave: a name or (depth name,
    in-plane name) - then the 6-tuples of pywt filters."""
    fw = iw = wave
    if not isinstance(wave, str):
        wd, wp = (filters.Wavelet(w) for w in wave)
        fw = (wd.dec_lo, wd.dec_hi) + (wp.dec_lo, wp.dec_hi) * 2
        iw = (wd.rec_lo, wd.rec_hi) + (wp.rec_lo, wp.rec_hi) * 2
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64 if dtype == F64 else F32)
    try:
        return pw.DWT3DForward(J=J, wave=fw, mode=mode).to(dev), pw.DWT3DInverse(wave=iw, mode=mode).to(dev)
    finally:
        torch.set_default_dtype(prev)


def rand(shape, dtype, dev, seed):
    return torch.tensor(np.random.RandomState(seed).randn(*shape)).to(dtype).to(dev)


def names(ks):
    return [k for k in ks if not k.endswith(')')]          # (without armed fallbacks and helper launches)


def depth(ks):
    return [k.split('<')[0] for k in ks if 'Depth' in k]


# ---- 1: values and layout ----------------------------------------------------------------------------------------------
def check_forward(dev, shape, wave, J, mode, dtype=F32, seed=1):
    x = rand(shape, dtype, dev, seed)
    xfm, _ = modules(dev, wave, J, mode, dtype)
    c0 = pw.launch_count()
    yl, yh = xfm(x)
    ks = names(pw.kernels_since(c0))
    bk = banks(wave, f32=dtype != F64)
    rl, rh = fwd_ref(npy(x), J, bk, mode)
    Ls = (len(bk[0][0]), len(bk[2][0]), len(bk[1][0]))      # taps along (D, H, W)
    size = shape[2:]
    for j in range(J):
        size = tuple(ops.coeff_len(n, L, dwl.mode_to_int(mode)) for n, L in zip(size, Ls))
        assert tuple(yh[j].shape) == shape[:2] + (7,) + size and yh[j].dtype == dtype
        close(yh[j], rh[j], dtype, 'yh[%d] %s %s' % (j, wave, mode), chain=True)
    assert tuple(yl.shape) == shape[:2] + size
    close(yl, rl, dtype, 'yl %s %s' % (wave, mode), chain=True)
    return x, yl, yh, ks


def check_band_table(dev, shape, wave, mode):
    """Band s of yh[0] is the band pywt.dwtn calls KEYS[s] over (D, H, W); bands 1..3 with yl are the depth-lowpass of
    DWTForward's (yl, lh, hl, hh) of the N*C*D planes, slice by slice."""
    x = rand(shape, F32, dev, 2)
    xfm, _ = modules(dev, wave, 1, mode)
    yl, yh = xfm(x)
    hd, hw, hh = banks(wave, f32=True)
    xn = npy(x)
    for s, key in KEYS.items():
        b = xn
        for ax, letter, h in ((4, key[2], hw), (3, key[1], hh), (2, key[0], hd)):
            b = wo.afb1d(b, h[0], h[1], mode, axis=ax)['ad'.index(letter)]
        close(yh[0][:, :, s - 1], b, F32, 'band %d = %s' % (s, key))
    N, C, D, H, W = shape
    pl, ph = pw.DWTForward(J=1, wave=wave, mode=mode).to(dev)(x.reshape(N, C * D, H, W))
    pl = npy(pl).reshape(N, C, D, *pl.shape[-2:])
    ph = npy(ph[0]).reshape(N, C, D, 3, *ph[0].shape[-2:])
    close(yl, wo.afb1d(pl, hd[0], hd[1], mode, axis=2)[0], F32, 'yl = depth-lowpass of DWTForward ll')
    for b in range(3):
        close(yh[0][:, :, b], wo.afb1d(ph[:, :, :, b], hd[0], hd[1], mode, axis=2)[0], F32, 'band %d of DWTForward' % (b + 1))


# ---- 2: the new kernels really ran ---------------------------------------------------------------------------------------
def check_kernels_ran(dev):
    shape = (1, 2, 10, 12, 16)
    xfm, ifm = modules(dev, 'db4', 1, 'symmetric')
    x = rand(shape, F32, dev, 3).requires_grad_(True)
    c0 = pw.launch_count()
    yl, yh = xfm(x)
    ks = names(pw.kernels_since(c0))
    assert len(ks) >= 2 and ks[-1].startswith('WlAfbDepth<float, 8,') and depth(ks) == ['WlAfbDepth'], ks
    c0 = pw.launch_count()
    rec = ifm((yl, yh))
    ks = names(pw.kernels_since(c0))
    assert len(ks) >= 2 and ks[0].startswith('WlSfbDepth<float, 8,') and depth(ks) == ['WlSfbDepth'], ks
    c0 = pw.launch_count()
    torch.autograd.grad(rec, x, torch.ones_like(rec))
    ks = names(pw.kernels_since(c0))
    # backward of the inverse: 2-D analysis, depth analysis; backward of the forward: depth synthesis, 2-D synthesis
    assert len(ks) >= 4 and depth(ks) == ['WlAfbDepth', 'WlSfbDepth'], ks
    # float64: the generic single-axis kernels, and still the oracle's numbers
    x64, yl64, yh64, ks = check_forward(dev, shape, 'db4', 1, 'symmetric', F64)
    assert sum(k.startswith('WlCorr1d<double>') for k in ks) == 4 and not any('Depth' in k for k in ks), ks
    _, ifm64 = modules(dev, 'db4', 1, 'symmetric', F64)
    c0 = pw.launch_count()
    rec = ifm64((yl64, yh64))
    ks = names(pw.kernels_since(c0))
    assert sum(k.startswith('WlSynth1d<double>') for k in ks) == 4 and not any('Depth' in k for k in ks), ks
    close(rec, inv_ref(npy(yl64), [npy(h) for h in yh64], banks('db4', syn=True), 'symmetric'), F64, 'float64 inverse')


# ---- 3 / 4: the kernels on their own ---------------------------------------------------------------------------------------
def tap_tensors(wave, dev, syn=False):
    return tuple(torch.tensor(np.ascontiguousarray(v), dtype=F32, device=dev) for v in taps(wave, syn, f32=True))


def depth_pair(dev, shape, wave, mode, chunks, dtype=F32, dim=1, seed=4, srcs=None):
    """ops.afb_depth of `srcs` (default: two random tensors of `shape`) and ops.sfb_depth of its outputs, full length and cropped to
    n, each against the oracle -> every output tensor, for comparisons between chunk counts."""
    h, g = tap_tensors(wave, dev), tap_tensors(wave, dev, syn=True)
    hn, gn = taps(wave, f32=True), taps(wave, syn=True, f32=True)
    if srcs is None:
        srcs = [rand(shape, dtype, dev, seed + i) for i in range(2)]
    n = srcs[0].shape[dim]
    res = ops.afb_depth(srcs, h[0], h[1], dwl.mode_to_int(mode), chunks=chunks, dim=dim)
    assert res is not None, 'the depth analysis kernel declined'
    name_a = pw.last_kernel()
    los, his = res
    outs = list(los) + list(his)
    for s, lo, hi in zip(srcs, los, his):
        rl, rh = wo.afb1d(npy(s), hn[0], hn[1], mode, axis=dim)
        close(lo, rl, dtype, 'afb_depth lo %s %s n=%d chunks=%d' % (wave, mode, n, chunks))
        close(hi, rh, dtype, 'afb_depth hi %s %s n=%d chunks=%d' % (wave, mode, n, chunks))
    name_s = None
    for out_len in (None, n):
        ys = ops.sfb_depth(los, [his[0]] + [None] * (len(his) - 1), g[0], g[1], dwl.mode_to_int(mode), out_len=out_len, chunks=chunks,
                           dim=dim)
        assert ys is not None, 'the depth synthesis kernel declined'
        name_s = pw.last_kernel()
        for i, (lo, y) in enumerate(zip(los, ys)):
            hi = npy(his[0]) if i == 0 else np.zeros(tuple(lo.shape))
            ref = wo.sfb1d(npy(lo), hi, gn[0], gn[1], mode, axis=dim)
            if out_len is not None:
                ref = np.take(ref, np.arange(out_len), axis=dim)
            close(y, ref, dtype, 'sfb_depth %s %s K=%d chunks=%d out_len=%s' % (wave, mode, lo.shape[dim], chunks, out_len))
        outs += list(ys)
    return outs, name_a, name_s


def check_chunks(dev, n, wave, mode):
    """chunks = 1, 2, 3, 5 on (outer 3, n, inner 64): each against the oracle, all bit-identical to chunks = 1."""
    base, na, ns = depth_pair(dev, (3, n, 64), wave, mode, 1)
    L = len(taps(wave)[0])
    assert na == 'WlAfbDepth<float, %d, 4>' % L and ns == 'WlSfbDepth<float, %d, 4>' % L, (na, ns)
    for chunks in (2, 3, 5):
        outs, _, _ = depth_pair(dev, (3, n, 64), wave, mode, chunks)
        for a, b in zip(outs, base):
            assert torch.equal(a, b), 'chunks=%d differs from chunks=1 (%s %s n=%d)' % (chunks, wave, mode, n)
    return base


def check_vec_bodies(dev, dtype=F32):
    """Which body runs: the 16-byte one when inner, strides and bases allow it, the scalar one otherwise - same numbers."""
    V = 16 // torch.tensor([], dtype=dtype).element_size()
    T = TNAME[dtype]
    for inner, vec in ((1, 1), (5, 1), (64, V), (1027, 1)):
        _, na, ns = depth_pair(dev, (2, 9, inner), 'db2', 'symmetric', 0, dtype)
        assert na == 'WlAfbDepth<%s, 4, %d>' % (T, vec) and ns == 'WlSfbDepth<%s, 4, %d>' % (T, vec), (inner, na, ns)
    # sources with unequal outer strides: a dense tensor and every 4th channel of another, not copied
    big = rand((3, 8, 9, 64), dtype, dev, 8)
    srcs = [rand((3, 2, 9, 64), dtype, dev, 9), big[:, 0::4]]
    assert ops._axis_strides(srcs[1], 2) == (4 * 9 * 64, 64)
    _, na, _ = depth_pair(dev, None, 'db2', 'reflect', 2, dtype, dim=2, srcs=srcs)
    assert na == 'WlAfbDepth<%s, 4, %d>' % (T, V), na
    # a base one element into its buffer: the scalar body
    flat = rand((2 * 9 * 64 + 1,), dtype, dev, 10)
    off = flat[1:].view(2, 9, 64)
    _, na, _ = depth_pair(dev, None, 'db2', 'zero', 0, dtype, srcs=[off])
    assert na == 'WlAfbDepth<%s, 4, 1>' % T, na
    # an axis stride that is no 16-byte multiple (planes of 64 at a pitch of 65 elements)
    pitched = rand((2, 9, 65), dtype, dev, 11)[:, :, :64]
    assert ops._axis_strides(pitched, 1) == (9 * 65, 65)
    _, na, _ = depth_pair(dev, None, 'db2', 'periodization', 0, dtype, srcs=[pitched])
    assert na == 'WlAfbDepth<%s, 4, 1>' % T, na


# ---- 4a: every compiled instantiation ------------------------------------------------------------------------------------
GRID_WAVES = tuple('db%d' % i for i in range(1, 11))        # L = 2, 4, .., 20: one case of the dispatchers' switch each
GRID_DTYPES = (F32, F16, BF16)


def ntaps(wave):
    return len(taps(wave)[0])


def depth_vec(dtype, L, inner):
    """The body width the launcher has to pick for dense, aligned (outer, n, inner) data - the rule as DESIGN.md 4.25 states it,
    written out here and not read from a launch: 16-byte pieces (4 floats, 8 halves), 2-byte data of 14 taps and more 8-byte
    pieces (4 halves), and the scalar body where the inner size is no multiple of the piece."""
    if dtype == F32:
        vec = 4
    else:
        vec = 8 if L < 14 else 4
    return vec if inner % vec == 0 else 1


def check_depth_instantiation(dev, wave, dtype, inners=(64, 68, 5)):
    """WlAfbDepth<T, L, VEC> / WlSfbDepth<T, L, VEC> of one tap count and element type in every body it is compiled for: n = 2L + 3
    (odd, and long enough for periodization) on inner sizes 64 (the vector body), 68 (a multiple of 4, not of 8: 2-byte data under
    14 taps falls to the scalar body, from 14 taps on it stays on VEC = 4) and 5 (the scalar body); every mode; three chunks
    (two seams) against the oracle and bit for bit against one chunk.  The kernel names are built from (T, L, VEC)."""
    L = ntaps(wave)
    n = 2 * L + 3
    for inner in inners:
        vec = depth_vec(dtype, L, inner)
        want = ('WlAfbDepth<%s, %d, %d>' % (TNAME[dtype], L, vec), 'WlSfbDepth<%s, %d, %d>' % (TNAME[dtype], L, vec))
        for mode in MODES:
            base, na, ns = depth_pair(dev, (2, n, inner), wave, mode, 1, dtype)
            assert (na, ns) == want, (inner, mode, na, ns, want)
            outs, na, ns = depth_pair(dev, (2, n, inner), wave, mode, 3, dtype)
            assert (na, ns) == want, (inner, mode, na, ns, want)
            for a, b in zip(outs, base):
                assert torch.equal(a, b), 'chunks=3 differs from chunks=1 (%s %s %s inner=%d)' % (wave, dtype, mode, inner)


def check_module_instantiation(dev, wave, dtype):
    """One level of DWT3DForward / DWT3DInverse on the 2-byte depth kernels of this tap count: (1, 2, 2L + 3, 9, 16), symmetric."""
    L = ntaps(wave)
    shape = (1, 2, 2 * L + 3, 9, 16)
    _, _, _, ks = check_forward(dev, shape, wave, 1, 'symmetric', dtype)
    assert ks[-1].startswith('WlAfbDepth<%s, %d,' % (TNAME[dtype], L)) and depth(ks) == ['WlAfbDepth'], ks
    c0 = pw.launch_count()
    check_inverse(dev, shape, wave, 'symmetric', J=1, dtype=dtype)
    ks = names(pw.kernels_since(c0))
    # (check_inverse runs a forward for the shapes first: the last depth launch is the inverse's)
    assert [k for k in ks if 'Depth' in k][-1].startswith('WlSfbDepth<%s, %d,' % (TNAME[dtype], L)), ks


# ---- 5: inverse ----------------------------------------------------------------------------------------------------------
def check_inverse(dev, shape, wave, mode, J=2, drop=None, dtype=F32):
    """DWT3DInverse of random coefficients shaped like a forward's (odd sizes: the low-pass of a level is one sample longer
    than the next highs) against the numpy synthesis; drop = a level whose highs are None."""
    xfm, ifm = modules(dev, wave, J, mode, dtype)
    yl, yh = xfm(rand(shape, dtype, dev, 12))
    yl = rand(tuple(yl.shape), dtype, dev, 13)
    yh = [rand(tuple(h.shape), dtype, dev, 14 + j) for j, h in enumerate(yh)]
    if drop is not None:
        yh[drop] = None
    rec = ifm((yl, yh))
    ref = inv_ref(npy(yl), [None if h is None else npy(h) for h in yh], banks(wave, syn=True, f32=dtype != F64), mode)
    assert all(n % 2 == 0 for n in rec.shape[2:]), rec.shape
    close(rec, ref, dtype, 'inverse %s %s J=%d drop=%s' % (wave, mode, J, drop), chain=True)


def check_roundtrip(dev, shape, wave, mode, dtype=F32):
    xfm, ifm = modules(dev, wave, 1, mode, dtype)
    x = rand(shape, dtype, dev, 20)
    rec = ifm(xfm(x))
    D, H, W = shape[2:]
    close(rec[:, :, :D, :H, :W], npy(x), dtype, 'round trip %s %s %s' % (wave, mode, shape), chain=True)


# ---- 6: gradients --------------------------------------------------------------------------------------------------------
def check_gradients(dev, shape, wave, mode, J=2, dtype=F32):
    xfm, ifm = modules(dev, wave, J, mode, dtype)
    f32 = dtype != F64
    x = rand(shape, dtype, dev, 30).requires_grad_(True)
    yl, yh = xfm(x)
    cots = [rand(tuple(t.shape), dtype, dev, 31 + i) for i, t in enumerate([yl] + yh)]
    dx, = torch.autograd.grad([yl] + yh, x, cots)
    in_shapes = [shape[2:]] + [tuple(h.shape[3:]) for h in yh[:-1]]
    ref = fwd_grad_ref(npy(cots[0]), [npy(c) for c in cots[1:]], in_shapes, banks(wave, f32=f32), mode)
    close(dx, ref, dtype, 'dx %s %s' % (wave, mode), chain=True)
    # the inverse, with respect to yl and every yh[j]
    cl = yl.detach().clone().requires_grad_(True)
    ch = [h.detach().clone().requires_grad_(True) for h in yh]
    rec = ifm((cl, ch))
    dy = rand(tuple(rec.shape), dtype, dev, 40)
    grads = torch.autograd.grad(rec, [cl] + ch, dy)
    L = len(taps(wave if isinstance(wave, str) else wave[0])[0])
    m = dwl.mode_to_int(mode)
    lo_shapes = [tuple(ops.synth_len(k, L, m) for k in h.shape[3:]) for h in yh[1:]] + [tuple(yl.shape[2:])]
    rl, rh = inv_grad_ref(npy(dy), lo_shapes, banks(wave, syn=True, f32=f32), mode)
    close(grads[0], rl, dtype, 'dyl %s %s' % (wave, mode), chain=True)
    for j in range(J):
        close(grads[1 + j], rh[j], dtype, 'dyh[%d] %s %s' % (j, wave, mode), chain=True)


def check_dot_product(dev, shape, wave, J=2):
    """<A x, y> = <x, A^T y> through the real modules, 'zero' mode (where the Q9 backward is the exact adjoint), float64."""
    xfm, _ = modules(dev, wave, J, 'zero', F64)
    x = rand(shape, F64, dev, 50).requires_grad_(True)
    outs = xfm(x)
    outs = [outs[0]] + outs[1]
    ys = [rand(tuple(t.shape), F64, dev, 51 + i) for i, t in enumerate(outs)]
    dx, = torch.autograd.grad(outs, x, ys)
    lhs = sum(float((a.detach() * b).sum()) for a, b in zip(outs, ys))
    rhs = float((x.detach() * dx).sum())
    print('dot product: %.15e against %.15e' % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)


# ---- 7: other dtypes and views -------------------------------------------------------------------------------------------
def check_low_precision(dev, dtype, shape=(2, 3, 10, 12, 16)):
    """float16 / bfloat16 forward, inverse and backward of one level on the depth kernels' 2-byte instantiations.  bfloat16: a 3-D
    level is two kernels with the 2-D stage's bands stored in bfloat16 in between - two roundings, not the single rounding that
    the 4e-3 of tests/_bf16_cases.py stands for - so the modules take its bound for everything else, 3e-2; the depth kernels on
    their own (check_vec_bodies: one rounding) take 4e-3."""
    x, yl, yh, ks = check_forward(dev, shape, 'db2', 1, 'symmetric', dtype)
    assert ks[-1].startswith('WlAfbDepth<%s, 4,' % TNAME[dtype]), ks
    xfm, ifm = modules(dev, 'db2', 1, 'symmetric', dtype)
    c0 = pw.launch_count()
    rec = ifm((yl, yh))
    assert names(pw.kernels_since(c0))[0].startswith('WlSfbDepth<%s, 4,' % TNAME[dtype])
    assert rec.dtype == dtype
    ref = inv_ref(npy(yl), [npy(h) for h in yh], banks('db2', syn=True, f32=True), 'symmetric')
    close(rec, ref, dtype, 'inverse', chain=True)
    xg = x.clone().requires_grad_(True)
    gl, gh = xfm(xg)
    cots = [rand(tuple(gl.shape), dtype, dev, 60), rand(tuple(gh[0].shape), dtype, dev, 61)]
    dx, = torch.autograd.grad([gl, gh[0]], xg, cots)
    assert dx.dtype == dtype
    ref = fwd_grad_ref(npy(cots[0]), [npy(cots[1])], [shape[2:]], banks('db2', f32=True), 'symmetric')
    close(dx, ref, dtype, 'dx', chain=True)


def check_views(dev):
    """A non-contiguous input equals its .contiguous() twin exactly; so do cotangents that are views."""
    xfm, ifm = modules(dev, 'db2', 1, 'reflect')
    big = rand((2, 3, 10, 12, 18), F32, dev, 70)
    for v in (big[..., 1:-1], big[:, 1:], big[:, :, ::2]):
        assert not v.is_contiguous()
        a, b = xfm(v), xfm(v.contiguous())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0])
    x = big[..., 1:-1].contiguous().requires_grad_(True)
    yl, yh = xfm(x)
    cl = rand(tuple(yl.shape[:-1]) + (yl.shape[-1] + 2,), F32, dev, 71)[..., 1:-1]
    ch = rand((2,) + tuple(yh[0].shape), F32, dev, 72)[1]
    chs = rand(tuple(yh[0].shape[:2]) + (9,) + tuple(yh[0].shape[3:]), F32, dev, 73)[:, :, 1:8]
    for cot_h in (ch, chs):
        assert not cl.is_contiguous()
        d1, = torch.autograd.grad([yl, yh[0]], x, [cl, cot_h], retain_graph=True)
        d2, = torch.autograd.grad([yl, yh[0]], x, [cl.contiguous(), cot_h.contiguous()], retain_graph=True)
        assert torch.equal(d1, d2)
    # coefficient views into the inverse
    yv = rand(tuple(yh[0].shape[:2]) + (9,) + tuple(yh[0].shape[3:]), F32, dev, 74)[:, :, 1:8]
    assert torch.equal(ifm((cl, [yv])), ifm((cl.contiguous(), [yv.contiguous()])))


# ---- 8: API --------------------------------------------------------------------------------------------------------------
def check_api(dev):
    xfm, ifm = modules(dev, 'db4', 2, 'symmetric')
    sd = xfm.state_dict()
    assert list(sd) == ['h0_dep', 'h1_dep', 'h0_col', 'h1_col', 'h0_row', 'h1_row']
    assert [tuple(v.shape) for v in sd.values()] == [(1, 1, 8, 1, 1)] * 2 + [(1, 1, 8, 1)] * 2 + [(1, 1, 1, 8)] * 2
    ref2d = pw.DWTForward(J=1, wave='db4', mode='symmetric').state_dict()
    for k in ('h0_col', 'h1_col', 'h0_row', 'h1_row'):
        assert torch.equal(sd[k].cpu(), ref2d[k])
    assert torch.equal(sd['h0_dep'].reshape(-1).cpu(), ref2d['h0_col'].reshape(-1))       # stored reversed like the others
    sd = ifm.state_dict()
    assert list(sd) == ['g0_dep', 'g1_dep', 'g0_col', 'g1_col', 'g0_row', 'g1_row']
    assert [tuple(v.shape) for v in sd.values()] == [(1, 1, 8, 1, 1)] * 2 + [(1, 1, 8, 1)] * 2 + [(1, 1, 1, 8)] * 2
    assert pw.DWT3D is pw.DWT3DForward and pw.IDWT3D is pw.DWT3DInverse
    assert all(n in pw.__all__ for n in ('DWT3DForward', 'DWT3DInverse', 'DWT3D', 'IDWT3D'))
    x = rand((1, 2, 6, 8, 10), F32, dev, 80)
    for bad in (x[0], x[0, 0]):
        try:
            xfm(bad)
        except ValueError:
            pass
        else:
            raise AssertionError('a %d-D input did not raise' % bad.dim())
    x0, none = modules(dev, 'db4', 0, 'symmetric')[0](x)
    assert x0 is x and none == []
    assert ifm((x, [])) is x
    # another wavelet along the depth axis: db1 along D, db4 in the plane
    check_forward(dev, (1, 2, 6, 9, 11), ('db1', 'db4'), 2, 'symmetric')
    check_inverse(dev, (1, 2, 6, 9, 11), ('db1', 'db4'), 'symmetric', J=2)
    # the function-level pair
    h, g = taps('db2', f32=True), taps('db2', syn=True, f32=True)
    w = filters.Wavelet('db2')
    yl, yh = dwl.afb3d(x, (w.dec_lo, w.dec_hi), 'periodization')
    rl, rh = fwd_ref(npy(x), 1, (h, h, h), 'periodization')
    close(yl, rl, F32, 'afb3d yl')
    close(yh, rh[0], F32, 'afb3d yh')
    close(dwl.sfb3d(yl, yh, (w.rec_lo, w.rec_hi), 'periodization'), inv_ref(npy(yl), [npy(yh)], (g, g, g), 'periodization'), F32,
          'sfb3d')


def check_cpu_tensor_raises():
    """Without the emulator installed a CPU tensor meets the engine's usual error."""
    xfm = pw.DWT3DForward(J=1, wave='db2')
    try:
        xfm(torch.zeros(1, 1, 4, 4, 4))
    except RuntimeError as e:
        assert 'no CPU fallback' in str(e), e
    else:
        raise AssertionError('a CPU tensor did not raise')
