"""Filter-tap gradients of the 1-D stationary transform on the MI355X: the one-launch kernel (csrc/wl_swt1d_tapgrad.h) against
the composition it replaces (ops.SWT1D_TAPGRAD_FUSED = False: both chains level by level and, per level and tap, a rolled product
summed in float64), on the same tensors in the same process.

    python tools/gpu_swt1d_tapgrad_probe.py [--out profiles/swt1d_tapgrad_probe.json] [--reps N]

Per dtype (float32, float16), db4 (8 taps) and db10 (20), J = 1 and 3, at 64 x 16 x 65536 (the shape of the other 1-D figures)
and at a short-row cell, 4096 x 16 x 1024:
  * `launch`: one tap gradient alone - ops.swt1d_tapgrad (the kernel plus the float64 sum of its partials) against
    lowlevel._swt1d_tapgrad_composed on the same (s, top, highs) -, with the kernel's algorithmic bytes, J + 2 signal sizes (s,
    the top and J highs in; the partials are about 4 % of one), over the 8 TB/s HBM roofline;
  * `forward_backward`: SWT1DForward + SWT1DInverse, forward and backward with the gradient reaching x and all four learned taps,
    on both routes, and the same step with fixed taps (buffers), which is what learning the filters is paid on top of.
Times are medians of device-event intervals over `reps` (>= 20) steps after warm-up, the variants taking turns inside one timing
loop; the spread of a cell is the interquartile range of its steps.  A cell is a WIN of the fused route only when its median is
below the composition's by more than the two spreads together.  The parent process does not touch the GPU: every dtype is measured
by a child of its own under a time limit, and the first child that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
STEP_TIMEOUT_S = 420
SHAPE, SHORT_SHAPE = (64, 16, 65536), (4096, 16, 1024)


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


def _cell(fused, comp):
    (mf, sf), (mc, sc) = fused, comp
    return {'fused_ms': round(mf, 4), 'fused_spread_ms': round(sf, 4), 'composed_ms': round(mc, 4), 'composed_spread_ms': round(sc, 4),
            'ratio': round(mc / mf, 3), 'fused_wins': bool(mc - mf > sf + sc)}


def _with_flag(flag, fn):
    from pytorch_wavelets_amd import ops

    def run():
        ops.SWT1D_TAPGRAD_FUSED = flag
        try:
            return fn()
        finally:
            ops.SWT1D_TAPGRAD_FUSED = True
    return run


def _measure(wave, J, x, reps):
    import torch
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import ops
    from pytorch_wavelets_amd.dwt import lowlevel
    dev = x.device
    size = x.numel() * x.element_size()
    r = {}
    fixed = (pw.SWT1DForward(J=J, wave=wave).to(dev), pw.SWT1DInverse(wave=wave).to(dev))
    learn = (pw.SWT1DForward(J=J, wave=wave, learn=True).to(dev), pw.SWT1DInverse(wave=wave, learn=True).to(dev))
    # one tap gradient alone: the inverse's (dx, lo, hi, g, 1/2)
    with torch.no_grad():
        lo, his = fixed[0](x)
    g0, g1 = fixed[1].g0, fixed[1].g1
    c0 = pw.launch_count()
    ca = ops.swt1d_tapgrad(x, lo, his, g0, g1, 0.5)
    r['fused_kernels'] = pw.kernels_since(c0)
    cb = lowlevel._swt1d_tapgrad_composed(x, lo, his, g0, g1, 0.5)
    r['max_abs_diff_between_routes'] = max(float((a.double() - b).abs().max()) for a, b in zip(ca, cb))
    r['max_abs_gradient'] = max(float(b.abs().max()) for b in cb)
    t = _time_alternating([lambda: ops.swt1d_tapgrad(x, lo, his, g0, g1, 0.5),
                           lambda: lowlevel._swt1d_tapgrad_composed(x, lo, his, g0, g1, 0.5)], reps, 3)
    r['launch'] = _cell(t[0], t[1])
    r['launch']['fused_fraction_of_hbm_roofline'] = round((J + 2) * size / HBM_BYTES_PER_S * 1e3 / t[0][0], 3)
    del lo, his
    # forward + backward of the pair of modules
    xg = x.clone().requires_grad_(True)
    cot = torch.ones_like(x)

    def step(mods):
        def run():
            yl, yh = mods[0](xg)
            mods[1]((yl, yh)).backward(cot)
            xg.grad = None
            for m in mods:
                for p in m.parameters():
                    p.grad = None
        return run
    c0 = pw.launch_count()
    step(learn)()
    r['step_kernels'] = pw.kernels_since(c0)
    t = _time_alternating([_with_flag(True, step(learn)), _with_flag(False, step(learn)), step(fixed)], reps, 3)
    r['forward_backward'] = _cell(t[0], t[1])
    r['forward_backward']['fixed_taps_ms'] = round(t[2][0], 4)
    r['forward_backward']['fixed_taps_spread_ms'] = round(t[2][1], 4)
    r['forward_backward']['fused_over_fixed_taps'] = round(t[0][0] / t[2][0], 3)
    del xg, cot
    torch.cuda.empty_cache()
    return r


def child(dtype_name, reps):
    import torch
    dev = torch.device('cuda:0')
    dtype = getattr(torch, dtype_name)
    res = {}
    for shape in (SHAPE, SHORT_SHAPE):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
        for wave in ('db4', 'db10'):
            for J in (1, 3):
                r = _measure(wave, J, x, reps)
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
        raise SystemExit('gpu_swt1d_tapgrad_probe: a median wants at least 20 timed steps')
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('gpu_swt1d_tapgrad_probe: no GPU visible (this probe measures; it has no CPU form)')
        res = child(a.child, a.reps)
        res['device'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'shapes': [list(SHAPE), list(SHORT_SHAPE)], 'reps': a.reps, 'hbm_roofline_bytes_per_s': HBM_BYTES_PER_S,
           'algorithmic_bytes_of_a_launch_in_signal_sizes': 'J + 2',
           'stat': 'median ms of device-event intervals after warm-up, the variants alternating in one loop; spread = interquartile range',
           'win': 'composed_ms - fused_ms > fused_spread_ms + composed_spread_ms',
           'routes': {'fused': 'ops.SWT1D_TAPGRAD_FUSED = True: one WlSwt1dTapGrad launch per transform node + the float64 sum of its partials',
                      'composed': 'ops.SWT1D_TAPGRAD_FUSED = False: the chains level by level, a rolled product per level and tap summed in float64',
                      'fixed_taps': 'the same forward + backward with the taps as buffers: no tap gradient'}}
    for name in ('float32', 'float16'):
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--child', name,
               '--reps', str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:                               # a fault, an abort or the time limit: nothing more runs on the GPU
            raise SystemExit('gpu_swt1d_tapgrad_probe: the %s step ended with status %d' % (name, p.returncode))
        out[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        out['device'] = out[name].pop('device')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
