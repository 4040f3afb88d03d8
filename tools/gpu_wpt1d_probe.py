"""The 1-D wavelet packet transform on the MI355X: WPT1DForward / WPT1DInverse on the wave-tile kernels (csrc/wl_wpt1d.h: up to three
levels per launch) against the two routes they replace, on the same tensors in the same process:

  * level by level (ops.WPT1D_FUSED = False): one wl_corr1d / wl_synth1d launch per level inside the same autograd nodes, with a
    torch.stack per level;
  * the user's composition: DWT1DForward(J=1) + torch.stack per level (DWT1DInverse(J=1) on the band slices for the inverse).

    python tools/gpu_wpt1d_probe.py [--out profiles/wpt1d_probe.json] [--reps N]

Per dtype (float32, float16), db4 and db10, J = 1, 2, 3, 6 at 64 x 16 x 65536 (the shape of the other 1-D probes) and J = 6 at
4096 x 16 x 1024 (the second launch there has rows of 128 samples, far shorter than a tile): forward, inverse and forward +
backward on the three routes.  Times are medians of device-event intervals over `reps` (>= 20) steps after warm-up, the routes
taking turns inside one timing loop; the spread of a cell is the interquartile range of its steps.  A cell is a WIN of the fused
route over a baseline only when its median is below the baseline's by more than the two spreads together.  Next to each cell:
the fused route's 2 N bytes per launch, ceil(J / 3) launches, over the 8 TB/s HBM roofline.  The parent process does not touch
the GPU: every dtype is measured by a child of its own under a time limit, and the first child that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
STEP_TIMEOUT_S = 420
CELLS = [((64, 16, 65536), (1, 2, 3, 6)), ((4096, 16, 1024), (6,))]


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


def _cell(times, nbytes=None):
    (mf, sf), (ml, sl), (mc, sc) = times
    cell = {'fused_ms': round(mf, 4), 'fused_spread_ms': round(sf, 4),
            'level_by_level_ms': round(ml, 4), 'level_by_level_spread_ms': round(sl, 4),
            'composition_ms': round(mc, 4), 'composition_spread_ms': round(sc, 4),
            'ratio_to_level_by_level': round(ml / mf, 3), 'ratio_to_composition': round(mc / mf, 3),
            'fused_wins_level_by_level': bool(ml - mf > sf + sl), 'fused_wins_composition': bool(mc - mf > sf + sc)}
    if nbytes is not None:
        cell['fused_fraction_of_hbm_roofline'] = round(nbytes / HBM_BYTES_PER_S * 1e3 / mf, 3)
    return cell


def child(dtype_name, reps):
    import torch
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import ops
    dev = torch.device('cuda:0')
    dtype = getattr(torch, dtype_name)
    res = {}

    def with_flag(flag, fn):
        def run():
            ops.WPT1D_FUSED = flag
            try:
                return fn()
            finally:
                ops.WPT1D_FUSED = True
        return run

    for shape, levels in CELLS:
        x = torch.randn(shape, generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
        N, C, n = shape
        for wave in ('db4', 'db10'):
            for J in levels:
                xfm = pw.WPT1DForward(J=J, wave=wave, mode='periodization').to(dev)
                ifm = pw.WPT1DInverse(wave=wave, mode='periodization').to(dev)
                dwt1 = pw.DWT1DForward(J=1, wave=wave, mode='periodization').to(dev)
                idwt1 = pw.DWT1DInverse(wave=wave, mode='periodization').to(dev)

                def comp_fwd(v):
                    y = v
                    for j in range(J):
                        lo, hi = dwt1(y)
                        y = torch.stack([lo, hi[0]], 2).view(N, C << (j + 1), lo.shape[-1])
                    return y.view(N, C, 1 << J, y.shape[-1])

                def comp_inv(y):
                    for j in range(J, 0, -1):
                        y = y.reshape(N, C << (j - 1), 2, y.shape[-1])
                        y = idwt1((y[:, :, 0], [y[:, :, 1]]))
                    return y

                nbytes = -(-J // 3) * 2 * x.numel() * x.element_size()
                r = {}
                with torch.no_grad():
                    c0 = pw.launch_count()
                    y = xfm(x)
                    r['forward_kernels'] = pw.kernels_since(c0)
                    c0 = pw.launch_count()
                    rec = ifm(y)
                    r['inverse_kernels'] = pw.kernels_since(c0)
                    y2, rec2 = with_flag(False, lambda: xfm(x))(), with_flag(False, lambda: ifm(y))()
                    y3, rec3 = comp_fwd(x), comp_inv(y)
                    r['max_abs_diff_to_level_by_level'] = max(float((a.float() - b.float()).abs().max()) for a, b in ((y, y2), (rec, rec2)))
                    r['max_abs_diff_to_composition'] = max(float((a.float() - b.float()).abs().max()) for a, b in ((y, y3), (rec, rec3)))
                    r['round_trip_max_abs_err'] = float((rec.float() - x.float()).abs().max())
                    del y2, rec2, y3, rec3, rec
                    t = _time_alternating([with_flag(True, lambda: xfm(x)), with_flag(False, lambda: xfm(x)), lambda: comp_fwd(x)], reps, 5)
                    r['forward'] = _cell(t, nbytes)
                    t = _time_alternating([with_flag(True, lambda: ifm(y)), with_flag(False, lambda: ifm(y)), lambda: comp_inv(y)], reps, 5)
                    r['inverse'] = _cell(t, nbytes)
                xg = x.clone().requires_grad_(True)
                cot = torch.ones_like(y)
                del y

                def step(fwd):
                    def run():
                        fwd(xg).backward(cot)
                        xg.grad = None
                    return run
                t = _time_alternating([with_flag(True, step(xfm)), with_flag(False, step(xfm)), step(comp_fwd)], reps, 3)
                r['forward_backward'] = _cell(t, 2 * nbytes)
                res['%dx%dx%d_%s_J%d' % (N, C, n, wave, J)] = r
                print(dtype_name, shape, wave, J, json.dumps({k: v for k, v in r.items() if not k.endswith('kernels')}), flush=True)
                del xg, cot
                torch.cuda.empty_cache()
        del x
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--child', default=None, help='(internal) measure this dtype and print the result as JSON')
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit('gpu_wpt1d_probe: a median wants at least 20 timed steps')
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('gpu_wpt1d_probe: no GPU visible (this probe measures; it has no CPU form)')
        res = child(a.child, a.reps)
        res['device'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'cells': [{'shape': list(s), 'levels': list(l)} for s, l in CELLS], 'reps': a.reps, 'hbm_roofline_bytes_per_s': HBM_BYTES_PER_S,
           'algorithmic_bytes': 'fused: 2 N per launch, ceil(J / 3) launches (forward + backward: twice that); level by level: 2 N per '
                                'level plus the stack',
           'stat': 'median ms of device-event intervals after warm-up, the three routes alternating in one loop; spread = interquartile range',
           'win': 'baseline_ms - fused_ms > fused_spread_ms + baseline_spread_ms',
           'routes': {'fused': 'ops.WPT1D_FUSED = True: one WlWpt1dAfb / WlWpt1dSfb launch for up to three levels',
                      'level_by_level': 'ops.WPT1D_FUSED = False: one WlCorr1d / WlSynth1d launch and one stack per level',
                      'composition': 'DWT1DForward(J=1) + torch.stack per level; DWT1DInverse on the band slices'}}
    for name in ('float32', 'float16'):
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--child', name,
               '--reps', str(a.reps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:                               # a fault, an abort or the time limit: nothing more runs on the GPU
            raise SystemExit('gpu_wpt1d_probe: the %s step ended with status %d' % (name, p.returncode))
        out[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        out['device'] = out[name].pop('device')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
