"""The 1-D stationary transform on the MI355X: SWT1DForward / SWT1DInverse on the wave-tile kernels (csrc/wl_swt1d.h: up to three
levels per launch) against the level-by-level path they replace (ops.SWT1D_FUSED = False: one wl_corr1d / wl_corr1d_adj launch
per level), on the same tensors in the same process.

    python tools/gpu_swt1d_probe.py [--out profiles/swt1d_probe.json] [--reps N] [--shape N C L]

Per dtype (float32, float16), db4 and db10, J = 1, 2, 3, default 64 x 16 x 65536 (the shape of the 1-D DTCWT figures): forward,
inverse and forward + backward on both routes.  Times are medians of device-event intervals over `reps` (>= 20) steps after
warm-up, the two routes taking turns inside one timing loop; the spread of a cell is the interquartile range of its steps.  A
cell is a WIN of the fused route only when its median is below the composition's by more than the two spreads together.  Next to
each cell: the ratio the byte counts predict at best, 3J / (J + 2) (level by level 3 J N, fused (J + 2) N), as an expectation,
and the fused route's (J + 2) N bytes over the 8 TB/s HBM roofline.  The parent process does not touch the GPU: every dtype is
measured by a child of its own under a time limit, and the first child that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
STEP_TIMEOUT_S = 300


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


def _cell(fused, comp, J, nbytes=None):
    (mf, sf), (mc, sc) = fused, comp
    cell = {'fused_ms': round(mf, 4), 'fused_spread_ms': round(sf, 4), 'level_by_level_ms': round(mc, 4),
            'level_by_level_spread_ms': round(sc, 4), 'ratio': round(mc / mf, 3), 'ratio_expected_from_bytes': round(3.0 * J / (J + 2), 3),
            'fused_wins': bool(mc - mf > sf + sc)}
    if nbytes is not None:
        cell['fused_fraction_of_hbm_roofline'] = round(nbytes / HBM_BYTES_PER_S * 1e3 / mf, 3)
    return cell


def child(shape, dtype_name, reps):
    import torch
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import ops
    dev = torch.device('cuda:0')
    dtype = getattr(torch, dtype_name)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
    res = {}

    def with_flag(flag, fn):
        def run():
            ops.SWT1D_FUSED = flag
            try:
                return fn()
            finally:
                ops.SWT1D_FUSED = True
        return run

    for wave in ('db4', 'db10'):
        for J in (1, 2, 3):
            xfm, ifm = pw.SWT1DForward(J=J, wave=wave).to(dev), pw.SWT1DInverse(wave=wave).to(dev)
            nbytes = (J + 2) * x.numel() * x.element_size()
            r = {}
            with torch.no_grad():
                c0 = pw.launch_count()
                yl, yh = xfm(x)
                r['forward_kernels'] = pw.kernels_since(c0)
                c0 = pw.launch_count()
                rec = ifm((yl, yh))
                r['inverse_kernels'] = pw.kernels_since(c0)
                c0 = pw.launch_count()
                yl2, yh2 = with_flag(False, lambda: xfm(x))()
                rec2 = with_flag(False, lambda: ifm((yl, yh)))()
                r['level_by_level_kernels'] = pw.kernels_since(c0)
                r['max_abs_diff_between_routes'] = max([float((a.float() - b.float()).abs().max()) for a, b in zip([yl, rec] + yh, [yl2, rec2] + yh2)])
                r['round_trip_max_abs_err'] = float((rec.float() - x.float()).abs().max())
                del yl2, yh2, rec2, rec
                t = _time_alternating([with_flag(True, lambda: xfm(x)), with_flag(False, lambda: xfm(x))], reps, 5)
                r['forward'] = _cell(t[0], t[1], J, nbytes)
                t = _time_alternating([with_flag(True, lambda: ifm((yl, yh))), with_flag(False, lambda: ifm((yl, yh)))], reps, 5)
                r['inverse'] = _cell(t[0], t[1], J, nbytes)
            xg = x.clone().requires_grad_(True)
            cots = [torch.ones_like(yl)] + [torch.ones_like(h) for h in yh]
            del yl, yh

            def step():
                a, b = xfm(xg)
                torch.autograd.backward([a] + list(b), cots)
                xg.grad = None
            t = _time_alternating([with_flag(True, step), with_flag(False, step)], reps, 3)
            r['forward_backward'] = _cell(t[0], t[1], J)
            res['%s_J%d' % (wave, J)] = r
            print(dtype_name, wave, J, json.dumps({k: v for k, v in r.items() if not k.endswith('kernels')}), flush=True)
            del xg, cots
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs=3, default=[64, 16, 65536])
    ap.add_argument('--child', default=None, help='(internal) measure this dtype and print the result as JSON')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('gpu_swt1d_probe: a median wants at least 20 timed steps')
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('gpu_swt1d_probe: no GPU visible (this probe measures; it has no CPU form)')
        res = child(tuple(a.shape), a.child, a.reps)
        res['device'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'shape': a.shape, 'reps': a.reps, 'hbm_roofline_bytes_per_s': HBM_BYTES_PER_S,
           'algorithmic_bytes': 'fused: (J + 2) N (x once, J highpasses and one lowpass); level by level: 3 J N',
           'stat': 'median ms of device-event intervals after warm-up, the two routes alternating in one loop; spread = interquartile range',
           'win': 'level_by_level_ms - fused_ms > fused_spread_ms + level_by_level_spread_ms',
           'routes': {'fused': 'ops.SWT1D_FUSED = True: one WlSwt1dFwd / WlSwt1dAdj launch for up to three levels',
                      'level_by_level': 'ops.SWT1D_FUSED = False: one WlCorr1d / WlCorr1dAdj launch per level'}}
    for name in ('float32', 'float16'):
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--child', name,
               '--reps', str(a.reps), '--shape'] + [str(v) for v in a.shape]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:                               # a fault, an abort or the time limit: nothing more runs on the GPU
            raise SystemExit('gpu_swt1d_probe: the %s step ended with status %d' % (name, p.returncode))
        out[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        out['device'] = out[name].pop('device')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
