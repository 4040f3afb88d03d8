"""Wavelet shrinkage on the MI355X: SWT1DShrink on the wave-tile kernels (csrc/wl_shrink1d.h: one launch per direction)
against the composition it replaces (ops.SHRINK1D_FUSED = False: SWT1DForward, element-wise torch operations, SWT1DInverse and
autograd), on the same tensors in the same process.

    python tools/gpu_shrink1d_probe.py [--out profiles/shrink1d_probe.json] [--reps N]

Per dtype (float32, float16), db4 (8 taps) and db10 (20), J = 1..3, soft shrinkage with a learned (J, 1, C) threshold, at
64 x 16 x 65536 (the shape of the other 1-D figures), and db4 J = 3 at a short-row cell, 4096 x 16 x 1024: the forward under
torch.no_grad() and forward + backward (the gradient reaches x and the thresholds), on both routes.  Times are medians of
device-event intervals over `reps` (>= 20) steps after warm-up, the two routes taking turns inside one timing loop; the spread of
a cell is the interquartile range of its steps.  A cell is a WIN of the fused route only when its median is below the
composition's by more than the two spreads together.  Next to each cell: the fused route's algorithmic bytes - 2 signal sizes
for the forward (x in, y out), 3 for the backward (x and dy in, dx out), so 5 for forward + backward - over the 8 TB/s HBM
roofline.  The parent process does not touch the GPU: every dtype is measured by a child of its own under a time limit, and the
first child that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
STEP_TIMEOUT_S = 300
SHAPE, SHORT_SHAPE = (64, 16, 65536), (4096, 16, 1024)
SIGNAL_SIZES = {'forward': 2, 'forward_backward': 5}


def _time_alternating(fns, reps, warm):
    """(median, interquartile range) in ms of the device-event time of every callable in `fns`, the callables taking turns."""
    import torch
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    out = []
    for t in ts:
        t = sorted(t)
        out.append((t[len(t) // 2], t[(3 * len(t)) // 4] - t[len(t) // 4]))
    return out


def _cell(fused, comp, nbytes):
    (mf, sf), (mc, sc) = fused, comp
    return {'fused_ms': round(mf, 4), 'fused_spread_ms': round(sf, 4), 'composed_ms': round(mc, 4), 'composed_spread_ms': round(sc, 4),
            'ratio': round(mc / mf, 3), 'fused_wins': bool(mc - mf > sf + sc),
            'fused_fraction_of_hbm_roofline': round(nbytes / HBM_BYTES_PER_S * 1e3 / mf, 3)}


def _measure(mod, x, reps):
    import torch
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import ops

    def with_flag(flag, fn):
        def run():
            ops.SHRINK1D_FUSED = flag
            try:
                return fn()
            finally:
                ops.SHRINK1D_FUSED = True
        return run

    size = x.numel() * x.element_size()
    r = {}
    with torch.no_grad():
        c0 = pw.launch_count()
        ya = mod(x)
        r['fused_kernels'] = pw.kernels_since(c0)
        c0 = pw.launch_count()
        yb = with_flag(False, lambda: mod(x))()
        r['composed_kernels'] = pw.kernels_since(c0)
        r['max_abs_diff_between_routes'] = float((ya.float() - yb.float()).abs().max())
        del yb
        t = _time_alternating([with_flag(True, lambda: mod(x)), with_flag(False, lambda: mod(x))], reps, 5)
        r['forward'] = _cell(t[0], t[1], SIGNAL_SIZES['forward'] * size)
    xg = x.clone().requires_grad_(True)
    cot = torch.ones_like(ya)
    del ya

    def step():
        mod(xg).backward(cot)
        xg.grad = None
        mod.thresh.grad = None
    t = _time_alternating([with_flag(True, step), with_flag(False, step)], reps, 3)
    r['forward_backward'] = _cell(t[0], t[1], SIGNAL_SIZES['forward_backward'] * size)
    del xg, cot
    torch.cuda.empty_cache()
    return r


def child(dtype_name, reps):
    import torch
    import pytorch_wavelets_amd as pw
    dev = torch.device('cuda:0')
    dtype = getattr(torch, dtype_name)
    res = {}
    for shape, cases in ((SHAPE, [(w, J) for w in ('db4', 'db10') for J in (1, 2, 3)]), (SHORT_SHAPE, [('db4', 3)])):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
        for wave, J in cases:
            # sigma = 1: a threshold of 1 keeps about a third of the coefficients of white noise at every level
            mod = pw.SWT1DShrink(J=J, wave=wave, thresh=torch.ones(J, 1, shape[1]), kind='soft', learn=True).to(dev)
            r = _measure(mod, x, reps)
            res['%s_%s_J%d' % ('x'.join(str(v) for v in shape), wave, J)] = r
            print(dtype_name, shape, wave, J, json.dumps({k: v for k, v in r.items() if not k.endswith('kernels')}), flush=True)
        del x
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--child', default=None, help='(internal) measure this dtype and print the result as JSON')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('gpu_shrink1d_probe: a median wants at least 20 timed steps')
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('gpu_shrink1d_probe: no GPU visible (this probe measures; it has no CPU form)')
        res = child(a.child, a.reps)
        res['device'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'shapes': [list(SHAPE), list(SHORT_SHAPE)], 'reps': a.reps, 'hbm_roofline_bytes_per_s': HBM_BYTES_PER_S,
           'algorithmic_bytes_in_signal_sizes': SIGNAL_SIZES,
           'stat': 'median ms of device-event intervals after warm-up, the two routes alternating in one loop; spread = interquartile range',
           'win': 'composed_ms - fused_ms > fused_spread_ms + composed_spread_ms',
           'routes': {'fused': 'ops.SHRINK1D_FUSED = True: one WlShrink1dFwd / WlShrink1dBwd launch',
                      'composed': 'ops.SHRINK1D_FUSED = False: SWT1DForward, element-wise torch operations, SWT1DInverse, autograd'}}
    for name in ('float32', 'float16'):
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--child', name,
               '--reps', str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:                               # a fault, an abort or the time limit: nothing more runs on the GPU
            raise SystemExit('gpu_shrink1d_probe: the %s step ended with status %d' % (name, p.returncode))
        out[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        out['device'] = out[name].pop('device')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
