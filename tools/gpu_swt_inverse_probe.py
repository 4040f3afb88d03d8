"""Timings of the transposed stationary level (wl_iswt2d_level) next to the forward level it mirrors (wl_swt2d_level), measured in
the same process: per case the forward level, the inverse level (scale 1/4, ll replaced) and the backward of SWTForward, with
device events after warm-up; median of the windows, fraction of 8 TB/s at 5 plane sizes per level (four sub-bands + one plane,
20 B/px in float32), and the kernels that ran.
usage: python tools/gpu_swt_inverse_probe.py [--out profiles/swt_inverse_probe.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_wavelets_amd as pw   # noqa: E402
from pytorch_wavelets_amd import filters, ops   # noqa: E402
from pytorch_wavelets_amd.dwt.transform2d import SWTForward, SWTInverse   # noqa: E402

PEAK = 8e12
SHAPE = (16, 3, 512, 512)
J = 2


def timeit(fn, reps=20, windows=7):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / reps)
    res.sort()
    return {'median_ms': res[len(res) // 2], 'min_ms': res[0], 'max_ms': res[-1]}


def names(fn):
    c0 = pw.launch_count()
    fn()
    return pw.kernels_since(c0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swt_inverse_probe.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this probe measures on the GPU only'
    dev = 'cuda:0'
    out = {'device': torch.cuda.get_device_name(0), 'shape': list(SHAPE), 'J': J, 'mode': 'periodic', 'peak_bytes_per_s': PEAK,
           'bytes_per_level': '5 plane sizes (four sub-bands + one plane)', 'cases': []}
    N, C, H, W = SHAPE
    for wave in ('db2', 'db4'):
        for dtype in (torch.float32, torch.float16):
            torch.manual_seed(0)
            h = [torch.tensor(v, dtype=torch.float32, device=dev) for v in filters.dwt_analysis_taps(wave)]
            g = [torch.tensor(v, dtype=torch.float32, device=dev) for v in filters.dwt_synthesis_taps(wave)]
            x = torch.randn(*SHAPE, device=dev).to(dtype)
            y = torch.randn(N, 4 * C, H, W, device=dev).to(dtype)
            ll = torch.randn(N, 4 * C, H, W, device=dev).to(dtype)[:, 0::4]
            level_bytes = 5 * x.numel() * x.element_size()
            case = {'wave': wave, 'dtype': str(dtype).split('.')[-1], 'bytes_per_level': level_bytes, 'levels': []}
            for d in (1, 2):
                def fwd():
                    return ops.swt2d_level(x, h[0], h[1], h[0], h[1], d, ops.EXT_PERIODIC)

                def inv():
                    return ops.iswt2d_level(y, g[0], g[1], g[0], g[1], d, ops.EXT_PERIODIC, 0.25, ll, 1)

                def bwd():
                    return ops.iswt2d_level(y, h[0], h[1], h[0], h[1], d, ops.EXT_PERIODIC, 1.0, ll, 2)
                row = {'dilation': d}
                for key, fn in (('forward_level', fwd), ('inverse_level', inv), ('backward_level_add', bwd), ('forward_level_again', fwd)):
                    t = timeit(fn)
                    t['kernels'] = names(fn)
                    t['fraction_of_peak'] = level_bytes / (t['median_ms'] * 1e-3) / PEAK
                    row[key] = t
                row['inverse_over_forward'] = row['inverse_level']['median_ms'] / row['forward_level']['median_ms']
                case['levels'].append(row)
            xfm = SWTForward(J=J, wave=wave, mode='periodic').to(dev)
            ifm = SWTInverse(wave=wave).to(dev)
            xr = x.clone().requires_grad_(True)
            ys = xfm(xr)
            cots = [torch.randn_like(v) for v in ys]
            coeffs = [v.detach() for v in ys]
            for key, fn in (('swt_forward', lambda: xfm(x)), ('swt_inverse', lambda: ifm(coeffs)),
                            ('swt_forward_backward_only', lambda: torch.autograd.grad(ys, xr, cots, retain_graph=True))):
                t = timeit(fn)
                t['kernels'] = names(fn)
                t['fraction_of_peak'] = J * level_bytes / (t['median_ms'] * 1e-3) / PEAK
                case[key] = t
            out['cases'].append(case)
            print(json.dumps(case), flush=True)
            del x, y, ll, xr, ys, cots, coeffs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
