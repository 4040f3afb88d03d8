"""The return codes of the 2-D DWT entry points, of the other entries that share their dtype dispatch and of the per-level
DTCWT / ScatLayer entries for invalid arguments, on the host emulation with a chip of 8 compute units.  The Python layer never passes such arguments, so nothing
else sees the validation at the top of the entries or the ORDER of its checks.

Every entry starts from one valid small call (3 planes of 20 x 24, 4 taps, symmetric, float32, forced onto its kernel; real
tensors behind every pointer) that returns 0, and is then called with one mutation at a time - or a pair, which pins which
check comes first.  EXPECTED is what the library returned before the launchers took one request struct (the DWT entries) or
the typed argument struct of their kernel (the DTCWT / ScatLayer entries): a literal table."""
import ctypes as C

import pytest
import torch

import emu_backend
from pytorch_wavelets_amd import _capi

MODE, SHAPE, UNSUP, DTYPE, TAPS = -1, -2, -3, -4, -5      # include/wavelets_hip.h
F32, F64 = 0, 2
KH, KW = 11, 13                                           # wl_dwt_coeff_len(20 / 24, 4, symmetric)


def _buf():
    return torch.zeros(1 << 16)                           # far more than any call below would touch if it did launch


_KEEP = [_buf() for _ in range(12)]
X, LL, HI, Y, HI2 = (t.data_ptr() for t in _KEEP[:5])
T0, T1, T2, T3, T4, T5 = (t.data_ptr() for t in _KEEP[5:11])
Z = _KEEP[11].data_ptr()
TAPS4 = dict(t0=T0, t1=T1, t2=T2, t3=T3)

# entry -> (argument names in the order of the prototype, the valid call, generic name -> the entry's own argument(s),
#           further mutations of this entry alone)
ENTRIES = {
    'wl_dwt2d_analysis': (
        'x ll highs dtype planes H W t0 t1 Lw t2 t3 Lh mode stream',
        dict(x=X, ll=LL, highs=HI, dtype=F32, planes=3, H=20, W=24, Lw=4, Lh=4, mode=1, **TAPS4),
        dict(L=('Lw', 'Lh')), {}),
    'wl_dwt2d_analysis_strided': (
        'x x_ps x_rs ll ll_ps ll_rs highs dtype planes H W t0 t1 Lw t2 t3 Lh mode stream',
        dict(x=X, x_ps=480, x_rs=24, ll=LL, ll_ps=KH * KW, ll_rs=KW, highs=HI, dtype=F32, planes=3, H=20, W=24, Lw=4, Lh=4,
             mode=1, **TAPS4),
        dict(L=('Lw', 'Lh')),
        {'x_rs<W': dict(x_rs=23), 'll_rs<Kw': dict(ll_rs=KW - 1), 'L=0,x_rs<W': dict(Lw=0, Lh=0, x_rs=23)}),
    'wl_dwt2d_synthesis': (
        'll ll_ps ll_rs highs y dtype planes Kh Kw OH OW t0 t1 Lw t2 t3 Lh mode stream',
        dict(ll=LL, ll_ps=KH * KW, ll_rs=KW, highs=HI, y=Y, dtype=F32, planes=3, Kh=KH, Kw=KW, OH=20, OW=24, Lw=4, Lh=4,
             mode=1, **TAPS4),
        dict(L=('Lw', 'Lh'), H='Kh'), {'OH>full': dict(OH=21)}),
    'wl_dwt2d_analysis_stream_ex': (
        'x x_ps x_rs ll ll_ps ll_rs highs dtype planes H W t0 t1 t2 t3 L mode policy scratch state stream',
        dict(x=X, x_ps=480, x_rs=24, ll=LL, ll_ps=KH * KW, ll_rs=KW, highs=HI, dtype=F32, planes=3, H=20, W=24, L=4, mode=1,
             policy=1, **TAPS4),
        dict(force='policy'),
        {'x_rs<W': dict(x_rs=23), 'll_rs<Kw': dict(ll_rs=KW - 1), 'periodization,W%4': dict(mode=2, W=22, x_rs=22)}),
    'wl_dwt2d_synthesis_stream_ex': (
        'll ll_ps ll_rs highs y dtype planes Kh Kw OH OW t0 t1 t2 t3 L mode policy scratch state stream',
        dict(ll=LL, ll_ps=KH * KW, ll_rs=KW, highs=HI, y=Y, dtype=F32, planes=3, Kh=KH, Kw=KW, OH=20, OW=24, L=4, mode=1,
             policy=1, **TAPS4),
        dict(H='Kh', force='policy'),
        {'OH>full': dict(OH=21), 'highs=NULL': dict(highs=None), 'periodization,Kw%4': dict(mode=2)}),
    'wl_dwt2d_analysis_fused_ex': (
        'x x_ps x_rs yl yh dtype planes H W nlev t0 t1 t2 t3 L mode strips scratch state stream',
        dict(x=X, x_ps=480, x_rs=24, yl=LL, yh=[HI], dtype=F32, planes=3, H=20, W=24, nlev=1, L=4, mode=1, strips=1, **TAPS4),
        dict(force='strips'), {'x_rs<W': dict(x_rs=23), 'not forced, 2 planes': dict(strips=0, planes=2)}),
    'wl_dwt2d_synthesis_fused_ex': (
        'yl yl_ps yl_rs yl_h yl_w yh Kh Kw y dtype planes nlev t0 t1 t2 t3 L mode strips scratch state stream',
        dict(yl=LL, yl_ps=KH * KW, yl_rs=KW, yl_h=KH, yl_w=KW, yh=[HI], Kh=[KH], Kw=[KW], y=Y, dtype=F32, planes=3, nlev=1,
             L=4, mode=1, strips=1, **TAPS4),
        dict(H='yl_h', force='strips'), {'Kh[0]=0': dict(Kh=[0]), 'not forced, 2 planes': dict(strips=0, planes=2)}),
    'wl_dwt2d_analysis_small': (
        'x yl yh dtype planes H W nlev t0 t1 t2 t3 L mode stream',
        dict(x=X, yl=LL, yh=[HI], dtype=F32, planes=3, H=20, W=24, nlev=1, L=4, mode=1, **TAPS4), {}, {}),
    'wl_dwt2d_synthesis_small': (
        'yl yl_h yl_w yh Kh Kw y dtype planes nlev t0 t1 t2 t3 L mode stream',
        dict(yl=LL, yl_h=KH, yl_w=KW, yh=[HI], Kh=[KH], Kw=[KW], y=Y, dtype=F32, planes=3, nlev=1, L=4, mode=1, **TAPS4),
        dict(H='yl_h'), {'Kh[0]=0': dict(Kh=[0])}),
    'wl_dwt1d_analysis_fused': (
        'x lo yh dtype planes H nlev t0 t1 L mode stream',
        dict(x=X, lo=LL, yh=[HI], dtype=F32, planes=3, H=24, nlev=1, L=4, mode=1, t0=T0, t1=T1), {}, {}),
    'wl_dwt1d_synthesis_fused': (
        'lo n_lo yh n_hi y out_len dtype planes nlev t0 t1 L mode stream',
        dict(lo=LL, n_lo=KW, yh=[HI], n_hi=[KW], y=Y, out_len=24, dtype=F32, planes=3, nlev=1, L=4, mode=1, t0=T0, t1=T1),
        dict(H='n_lo'), {'OH>full': dict(out_len=25)}),
    # (the fused DTCWT inverse takes planes of 32 x 32 and more: its valid call is 3 planes of 32 x 32, near_sym_a + qshift_a)
    'wl_dtcwt_inv_level21': (
        'll2 ll2_ps ll2_rs highs2 highs1 y dtype planes H W t0 L0 t1 L1 t2 t3 t4 t5 LQ mode policy stream',
        dict(ll2=LL, ll2_ps=256, ll2_rs=16, highs2=HI2, highs1=HI, y=Y, dtype=F32, planes=3, H=32, W=32, L0=7, L1=5, LQ=10,
             mode=1, policy=1, t4=T4, t5=T5, **TAPS4),
        dict(L='L0'), {'ll2_rs<W/2': dict(ll2_rs=15), 'policy=2': dict(policy=2)}),
    # (the fused DTCWT forward of levels 1 + 2 as well: 3 planes of 32 x 32, near_sym_a + qshift_a)
    'wl_dtcwt_fwd_level12': (
        'x highs1 ll2 highs2 dtype planes H W t0 L0 t1 L1 t2 t3 t4 t5 LQ mode policy stream',
        dict(x=X, highs1=HI, ll2=LL, highs2=HI2, dtype=F32, planes=3, H=32, W=32, L0=5, L1=7, LQ=10, mode=1, policy=1,
             t4=T4, t5=T5, **TAPS4),
        dict(L='L0'), {'policy=2': dict(policy=2), 'LQ=12': dict(LQ=12)}),
    # the per-level DTCWT / ScatLayer entries: 3 planes of 32 x 32 (one image of three channels where the entry counts both),
    # near_sym_a / qshift_a tap counts, symmetric, float32
    'wl_dtcwt_fwd_level1': (
        'x ll highs dtype planes H W t0 L0 t1 L1 mode stream',
        dict(x=X, ll=LL, highs=HI, dtype=F32, planes=3, H=32, W=32, t0=T0, L0=5, t1=T1, L1=7, mode=1),
        dict(L=('L0', 'L1')), {'mode=7': dict(mode=7), 'L0=4': dict(L0=4), 'mode=7,L0=4': dict(mode=7, L0=4),
                                'H=0,L0=4': dict(H=0, L0=4), 'L=129,L0=4': dict(L1=129, L0=4), 'L0=4,dtype=99': dict(L0=4, dtype=99)}),
    'wl_scat_fwd_level1': (
        'x z drdx drdy ll dtype N C H W t0 L0 t1 L1 mode magbias combine stream',
        dict(x=X, z=Z, drdx=HI, drdy=HI2, ll=LL, dtype=F32, N=1, C=3, H=32, W=32, t0=T0, L0=5, t1=T1, L1=7, mode=1, magbias=0.01,
             combine=0),
        dict(L=('L0', 'L1'), planes='N'),
        {'mode=7': dict(mode=7), 'L0=4': dict(L0=4), 'combine,C=2': dict(combine=1, C=2), 'mode=7,C=0': dict(mode=7, C=0),
         'combine,C=2,L=0': dict(combine=1, C=2, L0=0, L1=0), 'L=129,L0=4': dict(L1=129, L0=4), 'L0=4,dtype=99': dict(L0=4, dtype=99)}),
    'wl_scat_fwd_level1_into': (
        'x z z_bs z_ll z_mag ll dtype N C H W t0 L0 t1 L1 mode magbias stream',
        dict(x=X, z=Z, z_bs=7 * 3 * 256, z_ll=0, z_mag=3 * 256, ll=LL, dtype=F32, N=1, C=3, H=32, W=32, t0=T0, L0=5, t1=T1, L1=7,
             mode=1, magbias=0.01),
        dict(L=('L0', 'L1'), planes='N'),
        {'mode=7': dict(mode=7), 'L0=4': dict(L0=4), 'z=NULL': dict(z=None), 'mode=7,z=NULL': dict(mode=7, z=None),
         'z=NULL,L=0': dict(z=None, L0=0, L1=0), 'L=129,L0=4': dict(L1=129, L0=4), 'L0=4,dtype=99': dict(L0=4, dtype=99)}),
    # (the second scale of ScatLayerj2 has the streaming kernel only, which takes planes of 128 columns and more that fill the
    # chip: its valid call is 8 planes of 32 x 128)
    'wl_scat_fwd_level2_into': (
        'x z z_bs z_ll z_mag dtype N C H W t0 t1 t2 t3 L magbias stream',
        dict(x=X, z=Z, z_bs=7 * 8 * 256, z_ll=0, z_mag=8 * 256, dtype=F32, N=1, C=8, H=32, W=128, L=10, magbias=0.01, **TAPS4),
        dict(planes='N'),
        {'L=11': dict(L=11), 'H=34': dict(H=34), 'z=NULL': dict(z=None), 'z=NULL,L=11': dict(z=None, L=11),
         'H=34,L=11': dict(H=34, L=11), 'H=34,dtype=99': dict(H=34, dtype=99), '3 planes of 32 x 32': dict(C=3, W=32)}),
    # (near_sym_b_bp: 13 / 19 / 19 taps)
    'wl_dtcwt_fwd_level1_rot': (
        'x ll re im dtype N C H W t0 L0 t1 L1 t2 L2 mode scat magbias stream',
        dict(x=X, ll=LL, re=HI, im=HI2, dtype=F32, N=1, C=3, H=32, W=32, t0=T0, L0=13, t1=T1, L1=19, t2=T2, L2=19, mode=1, scat=0,
             magbias=0.01),
        dict(L=('L0', 'L1', 'L2'), planes='N'),
        {'mode=7': dict(mode=7), 'L0=4': dict(L0=4), 'L2=21': dict(L2=21), 'H=31': dict(H=31), 'L2=129': dict(L2=129),
         'mode=7,C=0': dict(mode=7, C=0), 'L2=21,dtype=99': dict(L2=21, dtype=99), 'H=31,dtype=99': dict(H=31, dtype=99),
         'L2=129,L0=4': dict(L2=129, L0=4)}),
    'wl_dtcwt_fwd_level2': (
        'x ll highs dtype planes H W t0 t1 t2 t3 L stream',
        dict(x=X, ll=LL, highs=HI, dtype=F32, planes=3, H=32, W=32, L=10, **TAPS4), {},
        {'L=11': dict(L=11), 'H=31': dict(H=31), 'H=31,L=11': dict(H=31, L=11), 'L=11,dtype=99': dict(L=11, dtype=99)}),
    'wl_dtcwt_inv_level1': (
        'll ll_ps ll_rs highs y dtype planes H W t0 L0 t1 L1 mode stream',
        dict(ll=LL, ll_ps=1024, ll_rs=32, highs=HI, y=Y, dtype=F32, planes=3, H=32, W=32, t0=T0, L0=7, t1=T1, L1=5, mode=1),
        dict(L=('L0', 'L1')),
        {'L0=4': dict(L0=4), 'H=31': dict(H=31), 'll=highs=NULL': dict(ll=None, highs=None),
         'll=highs=NULL,L=0': dict(ll=None, highs=None, L0=0, L1=0), 'L=129,L0=4': dict(L1=129, L0=4),
         'L0=4,dtype=99': dict(L0=4, dtype=99)}),
    'wl_scat_bwd_level1': (
        'dz drdx drdy dx dtype N C H W t0 L0 t1 L1 mode combine stream',
        dict(dz=Z, drdx=HI, drdy=HI2, dx=Y, dtype=F32, N=1, C=3, H=32, W=32, t0=T0, L0=5, t1=T1, L1=7, mode=1, combine=0),
        dict(L=('L0', 'L1'), planes='N'),
        {'mode=7': dict(mode=7), 'L0=4': dict(L0=4), 'H=31': dict(H=31), 'combine,C=2': dict(combine=1, C=2),
         'mode=7,H=31': dict(mode=7, H=31), 'combine,C=2,L=0': dict(combine=1, C=2, L0=0, L1=0)}),
    'wl_dtcwt_inv_level2': (
        'll ll_ps ll_rs highs y dtype planes h w t0 t1 t2 t3 L stream',
        dict(ll=LL, ll_ps=256, ll_rs=16, highs=HI, y=Y, dtype=F32, planes=3, h=16, w=16, L=10, **TAPS4),
        dict(H='h'),
        {'L=11': dict(L=11), 'h=15': dict(h=15), 'll=highs=NULL': dict(ll=None, highs=None),
         'll=highs=NULL,L=11': dict(ll=None, highs=None, L=11), 'L=11,dtype=99': dict(L=11, dtype=99)}),
}

# generic mutations: name -> {generic argument: value}; an entry takes those whose arguments it has
GENERIC = {
    'mode=3': dict(mode=3), 'planes=-1': dict(planes=-1), 'H=0': dict(H=0), 'L=0': dict(L=0), 'L=129': dict(L=129),
    'dtype=f64': dict(dtype=F64), 'dtype=99': dict(dtype=99), 'policy=4': dict(policy=4),
    'strips=16': dict(strips=16), 'strips=-1': dict(strips=-1), 'nlev=0': dict(nlev=0),
    'not forced, 3 planes': dict(force=0),
    'mode=3,L=0': dict(mode=3, L=0), 'H=0,L=0': dict(H=0, L=0), 'L=0,dtype=99': dict(L=0, dtype=99),
}
# (8 x 3 planes = 3 x 8 compute units is exactly where the fused kernels start to pay: 'not forced, 3 planes' is a launch
# there, recorded as such; the same with 2 planes is the decline)
LAUNCHES = 'not forced, 3 planes'
# float64 is a valid dtype of the per-level entries that have a generic kernel: only the unknown dtype there
F64_LAUNCHES = {'wl_dwt2d_analysis', 'wl_dwt2d_analysis_strided', 'wl_dwt2d_synthesis', 'wl_dtcwt_fwd_level1',
                'wl_scat_fwd_level1', 'wl_scat_fwd_level1_into', 'wl_dtcwt_fwd_level1_rot', 'wl_dtcwt_fwd_level2',
                'wl_dtcwt_inv_level1', 'wl_dtcwt_inv_level2'}
# mode 3 (and 5) is a padding mode of the level-1 DTCWT / ScatLayer entries (zeros, like every mode but symmetric), and the
# level-1 inverse takes any: a launch there - their invalid mode is 'mode=7'
MODE3_LAUNCHES = {'wl_dtcwt_fwd_level1', 'wl_scat_fwd_level1', 'wl_scat_fwd_level1_into', 'wl_dtcwt_fwd_level1_rot',
                  'wl_dtcwt_inv_level1', 'wl_scat_bwd_level1'}

EXPECTED = {
    'wl_dwt2d_analysis': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE,
        'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS
    },
    'wl_dwt2d_analysis_strided': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE,
        'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'x_rs<W': SHAPE, 'll_rs<Kw': SHAPE, 'L=0,x_rs<W': TAPS
    },
    'wl_dwt2d_synthesis': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE,
        'mode=3,L=0': MODE, 'H=0,L=0': TAPS, 'L=0,dtype=99': TAPS, 'OH>full': SHAPE
    },
    'wl_dwt2d_analysis_stream_ex': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'policy=4': UNSUP, 'not forced, 3 planes': UNSUP, 'mode=3,L=0': MODE, 'H=0,L=0': SHAPE,
        'L=0,dtype=99': TAPS, 'x_rs<W': SHAPE, 'll_rs<Kw': SHAPE, 'periodization,W%4': UNSUP
    },
    'wl_dwt2d_synthesis_stream_ex': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'policy=4': UNSUP, 'not forced, 3 planes': UNSUP, 'mode=3,L=0': MODE, 'H=0,L=0': TAPS,
        'L=0,dtype=99': TAPS, 'OH>full': SHAPE, 'highs=NULL': UNSUP, 'periodization,Kw%4': UNSUP
    },
    'wl_dwt2d_analysis_fused_ex': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'strips=16': UNSUP, 'strips=-1': UNSUP, 'nlev=0': UNSUP, 'not forced, 3 planes': 0,
        'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'x_rs<W': SHAPE, 'not forced, 2 planes': UNSUP
    },
    'wl_dwt2d_synthesis_fused_ex': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'strips=16': UNSUP, 'strips=-1': UNSUP, 'nlev=0': UNSUP, 'not forced, 3 planes': 0,
        'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'Kh[0]=0': UNSUP, 'not forced, 2 planes': UNSUP
    },
    'wl_dwt2d_analysis_small': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'nlev=0': UNSUP, 'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS
    },
    'wl_dwt2d_synthesis_small': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'nlev=0': UNSUP, 'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'Kh[0]=0': SHAPE
    },
    'wl_dwt1d_analysis_fused': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'nlev=0': SHAPE, 'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS
    },
    'wl_dwt1d_synthesis_fused': {
        'valid': 0, 'mode=3': MODE, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'nlev=0': SHAPE, 'mode=3,L=0': MODE, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'OH>full': SHAPE
    },
    'wl_dtcwt_inv_level21': {
        'valid': 0, 'mode=3': UNSUP, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'policy=4': UNSUP, 'mode=3,L=0': TAPS, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'll2_rs<W/2': SHAPE,
        'policy=2': UNSUP
    },
    'wl_dtcwt_fwd_level12': {
        'valid': 0, 'mode=3': UNSUP, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP,
        'dtype=99': DTYPE, 'policy=4': UNSUP, 'mode=3,L=0': TAPS, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'policy=2': UNSUP,
        'LQ=12': UNSUP
    },
    'wl_dtcwt_fwd_level1': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE, 'mode=3,L=0': TAPS,
        'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'mode=7': MODE, 'L0=4': UNSUP, 'mode=7,L0=4': MODE, 'H=0,L0=4': SHAPE,
        'L=129,L0=4': TAPS, 'L0=4,dtype=99': UNSUP
    },
    'wl_scat_fwd_level1': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE, 'mode=3,L=0': TAPS,
        'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'mode=7': MODE, 'L0=4': UNSUP, 'combine,C=2': SHAPE, 'mode=7,C=0': MODE,
        'combine,C=2,L=0': SHAPE, 'L=129,L0=4': TAPS, 'L0=4,dtype=99': UNSUP
    },
    'wl_scat_fwd_level1_into': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE, 'mode=3,L=0': TAPS,
        'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'mode=7': MODE, 'L0=4': UNSUP, 'z=NULL': SHAPE, 'mode=7,z=NULL': MODE,
        'z=NULL,L=0': SHAPE, 'L=129,L0=4': TAPS, 'L0=4,dtype=99': UNSUP
    },
    'wl_scat_fwd_level2_into': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP, 'dtype=99': DTYPE,
        'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'L=11': TAPS, 'H=34': UNSUP, 'z=NULL': SHAPE, 'z=NULL,L=11': SHAPE,
        'H=34,L=11': TAPS, 'H=34,dtype=99': UNSUP, '3 planes of 32 x 32': UNSUP
    },
    'wl_dtcwt_fwd_level1_rot': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE, 'mode=3,L=0': TAPS,
        'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'mode=7': MODE, 'L0=4': UNSUP, 'L2=21': UNSUP, 'H=31': UNSUP, 'L2=129':
        TAPS, 'mode=7,C=0': MODE, 'L2=21,dtype=99': UNSUP, 'H=31,dtype=99': UNSUP, 'L2=129,L0=4': TAPS
    },
    'wl_dtcwt_fwd_level2': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE, 'H=0,L=0': SHAPE,
        'L=0,dtype=99': TAPS, 'L=11': TAPS, 'H=31': SHAPE, 'H=31,L=11': SHAPE, 'L=11,dtype=99': TAPS
    },
    'wl_dtcwt_inv_level1': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE, 'mode=3,L=0': TAPS,
        'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'L0=4': UNSUP, 'H=31': SHAPE, 'll=highs=NULL': SHAPE, 'll=highs=NULL,L=0':
        SHAPE, 'L=129,L0=4': TAPS, 'L0=4,dtype=99': UNSUP
    },
    'wl_scat_bwd_level1': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=f64': UNSUP, 'dtype=99': DTYPE,
        'mode=3,L=0': TAPS, 'H=0,L=0': SHAPE, 'L=0,dtype=99': TAPS, 'mode=7': MODE, 'L0=4': UNSUP, 'H=31': SHAPE,
        'combine,C=2': SHAPE, 'mode=7,H=31': MODE, 'combine,C=2,L=0': SHAPE
    },
    'wl_dtcwt_inv_level2': {
        'valid': 0, 'planes=-1': SHAPE, 'H=0': SHAPE, 'L=0': TAPS, 'L=129': TAPS, 'dtype=99': DTYPE, 'H=0,L=0': SHAPE,
        'L=0,dtype=99': TAPS, 'L=11': TAPS, 'h=15': SHAPE, 'll=highs=NULL': SHAPE, 'll=highs=NULL,L=11': SHAPE,
        'L=11,dtype=99': TAPS
    },
}


def _mutations(entry):
    _, base, alias, extra = ENTRIES[entry]
    out = {}
    for label, change in GENERIC.items():
        if (label == 'dtype=f64' and entry in F64_LAUNCHES) or (label == 'mode=3' and entry in MODE3_LAUNCHES):
            continue
        real = {}
        for k, v in change.items():
            names = alias.get(k, k)
            for n in ((names,) if isinstance(names, str) else names):
                real[n] = v
        if all(n in base for n in real):
            out[label] = real
    out.update(extra)
    return out


def _call(lib, entry, args):
    order, ctypes_ = ENTRIES[entry][0].split(), _capi.PROTOTYPES[entry][1]
    assert len(order) == len(ctypes_) and set(args) <= set(order)
    vals = []
    for name, ctype in zip(order, ctypes_):
        v = args.get(name)                                # (absent: stream, tap scratch and tap state are null)
        if isinstance(v, list):                           # an array of pointers / of ints
            v = ((C.c_void_p if ctype == C.POINTER(C.c_void_p) else C.c_int) * len(v))(*v)
        vals.append(v)
    return getattr(lib, entry)(*vals)


def codes(entry):
    """{'valid': rc of the valid call, mutation: its rc, ...} of one entry."""
    with emu_backend.emulated(), emu_backend.chip_of(8):
        lib = emu_backend.handle()
        base = ENTRIES[entry][1]
        got = {'valid': _call(lib, entry, base)}
        for label, change in _mutations(entry).items():
            got[label] = _call(lib, entry, dict(base, **change))
    return got


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_return_codes_of_invalid_arguments(entry):
    want = EXPECTED[entry]
    launched = {label for label, rc in want.items() if rc == 0}
    assert launched <= {'valid', LAUNCHES}, 'a mutation must not launch'
    assert codes(entry) == want
