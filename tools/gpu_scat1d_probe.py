"""The 1-D scattering layer on the MI355X: ScatLayer1D on the wave-tile kernels (csrc/wl_scat1d.h: one launch per direction)
against the composition it replaces (ops.SCAT1D_FUSED = False: level 1 of the 1-D DTCWT node, element-wise torch operations and
autograd), on the same tensors in the same process.

    python tools/gpu_scat1d_probe.py [--out profiles/scat1d_probe.json] [--reps N]

Per dtype (float32, float16), near_sym_a (5 / 7 taps) and near_sym_b (13 / 19), at 64 x 16 x 65536 (the shape of the other 1-D
figures) and at a short-row cell, 4096 x 16 x 1024: the forward under torch.no_grad() (inference), the forward of an input that
asks for a gradient (training: the directions are stored as well) and forward + backward, on both routes.  float32 near_sym_a
also sweeps the row length from 64 to 4096 samples at 2^26 samples in all: one wave serves one row, so this is where the fused
route can lose (it does not: ops.scat1d_covered sets no shortest row).  Times are medians of device-event intervals over `reps` (>= 20)
steps after warm-up, the two routes taking turns inside one timing loop; the spread of a cell is the interquartile range of its
steps.  A cell is a WIN of the fused route only when its median is below the composition's by more than the two spreads
together.  Next to each cell: the fused route's algorithmic bytes - 2 signal sizes for the inference forward (x in, Z out), 3 for
the training forward (the directions out) and for the backward (dZ and the directions in, dx out), so 6 for forward + backward -
over the 8 TB/s HBM roofline.  The parent process does not touch the GPU: every dtype is measured by a child of its own under a
time limit, and the first child that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
STEP_TIMEOUT_S = 300
SHAPES = ((64, 16, 65536), (4096, 16, 1024))
SWEEP_LENGTHS = (64, 128, 256, 512, 1024, 2048, 4096)
SWEEP_SAMPLES = 1 << 26
SIGNAL_SIZES = {'inference_forward': 2, 'training_forward': 3, 'forward_backward': 6}


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


def _measure(mod, x, reps, what):
    """The cells `what` of one layer on one input."""
    import torch
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import ops

    def with_flag(flag, fn):
        def run():
            ops.SCAT1D_FUSED = flag
            try:
                return fn()
            finally:
                ops.SCAT1D_FUSED = True
        return run

    size = x.numel() * x.element_size()
    r = {}
    with torch.no_grad():
        c0 = pw.launch_count()
        za = mod(x)
        r['fused_kernels'] = pw.kernels_since(c0)
        c0 = pw.launch_count()
        zb = with_flag(False, lambda: mod(x))()
        r['composed_kernels'] = pw.kernels_since(c0)
        r['max_abs_diff_between_routes'] = float((za.float() - zb.float()).abs().max())
        del zb
        if 'inference_forward' in what:
            t = _time_alternating([with_flag(True, lambda: mod(x)), with_flag(False, lambda: mod(x))], reps, 5)
            r['inference_forward'] = _cell(t[0], t[1], 2 * size)
    xg = x.clone().requires_grad_(True)
    if 'training_forward' in what:
        t = _time_alternating([with_flag(True, lambda: mod(xg)), with_flag(False, lambda: mod(xg))], reps, 5)
        r['training_forward'] = _cell(t[0], t[1], 3 * size)
    cot = torch.ones_like(za)
    del za

    def step():
        mod(xg).backward(cot)
        xg.grad = None
    if 'forward_backward' in what:
        t = _time_alternating([with_flag(True, step), with_flag(False, step)], reps, 3)
        r['forward_backward'] = _cell(t[0], t[1], 6 * size)
    del xg, cot
    torch.cuda.empty_cache()
    return r


def child(dtype_name, reps):
    import torch
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import ops
    dev = torch.device('cuda:0')
    dtype = getattr(torch, dtype_name)
    res = {}
    for shape in SHAPES:
        x = torch.randn(shape, generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
        for biort in ('near_sym_a', 'near_sym_b'):
            r = _measure(pw.ScatLayer1D(biort=biort).to(dev), x, reps, tuple(SIGNAL_SIZES))
            res['%s_%s' % ('x'.join(str(v) for v in shape), biort)] = r
            print(dtype_name, shape, biort, json.dumps({k: v for k, v in r.items() if not k.endswith('kernels')}), flush=True)
        del x
    if dtype_name == 'float32':
        sweep = {}
        mod = pw.ScatLayer1D().to(dev)
        for n in SWEEP_LENGTHS:
            x = torch.randn((SWEEP_SAMPLES // (16 * n), 16, n), generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
            r = _measure(mod, x, reps, ('inference_forward', 'forward_backward'))
            sweep[str(n)] = {k: v for k, v in r.items() if not k.endswith('kernels')}
            print(dtype_name, 'rows of', n, json.dumps(sweep[str(n)]), flush=True)
            del x
        res['length_sweep_near_sym_a'] = sweep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--child', default=None, help='(internal) measure this dtype and print the result as JSON')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('gpu_scat1d_probe: a median wants at least 20 timed steps')
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('gpu_scat1d_probe: no GPU visible (this probe measures; it has no CPU form)')
        res = child(a.child, a.reps)
        res['device'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'shapes': [list(s) for s in SHAPES], 'reps': a.reps, 'hbm_roofline_bytes_per_s': HBM_BYTES_PER_S,
           'algorithmic_bytes_in_signal_sizes': SIGNAL_SIZES,
           'stat': 'median ms of device-event intervals after warm-up, the two routes alternating in one loop; spread = interquartile range',
           'win': 'composed_ms - fused_ms > fused_spread_ms + composed_spread_ms',
           'length_sweep': 'float32, near_sym_a, (2^26 / (16 n), 16, n) for n = ' + ', '.join(str(n) for n in SWEEP_LENGTHS),
           'routes': {'fused': 'ops.SCAT1D_FUSED = True: one WlScat1dFwd / WlScat1dBwd launch',
                      'composed': 'ops.SCAT1D_FUSED = False: level 1 of the 1-D DTCWT node, element-wise torch operations, autograd'}}
    for name in ('float32', 'float16'):
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--child', name,
               '--reps', str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:                               # a fault, an abort or the time limit: nothing more runs on the GPU
            raise SystemExit('gpu_scat1d_probe: the %s step ended with status %d' % (name, p.returncode))
        out[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        out['device'] = out[name].pop('device')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
