"""The 2-D wavelet packet transform on the MI355X: WPT2DForward / WPT2DInverse on the packed-band kernels (csrc/wl_wpt2d.h)
against the composition a user could write before them - DWTForward(J=1) + torch.cat per level, DWTInverse per level - on the
same tensors in the same process, with each transform's algorithmic bytes over the HBM roofline.

    python tools/gpu_wpt2d_probe.py [--out profiles/wpt2d_probe.json] [--reps N] [--shape N C H W]

Per dtype (float32, float16), db4, periodization and symmetric, J = 2 and 3, default 64 x 3 x 512 x 512: forward, inverse and
forward + backward on three routes - (a) the composition, (b) ops.WPT_FUSED = False: one packet launch per level, (c)
ops.WPT_FUSED = True: two levels per launch where the kernels take them (periodization here; in symmetric mode (c) runs (b)'s
launches).  Times are medians of device-event intervals after warm-up; the three routes alternate inside one timing loop.  Bytes
are what a packet level must move - the volume read once and written once, 2 volume-sizes per level; the roofline is 8 TB/s.  The parent process does not touch the GPU: every dtype is measured by a child of its own under a time
limit, and the first child that fails ends the probe."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
STEP_TIMEOUT_S = 240


def _time_alternating(fns, reps, warm):
    """Median device-event time (ms) of every callable in `fns`, the callables taking turns inside the loop."""
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
    return [sorted(t)[len(t) // 2] for t in ts]


def _entry(ms, nbytes):
    return {'ms': round(ms, 4), 'fraction_of_hbm_roofline': round(nbytes / HBM_BYTES_PER_S * 1e3 / ms, 3)}


def child(shape, dtype_name, reps):
    import torch
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import ops
    from pytorch_wavelets_amd.dwt import lowlevel
    dev = torch.device('cuda:0')
    dtype = getattr(torch, dtype_name)
    N, C, H, W = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(0)).to(dtype).to(dev)
    res = {}
    for mode in ('periodization', 'symmetric'):
        m = lowlevel.mode_to_int(mode)
        dwt, idwt = pw.DWTForward(J=1, wave='db4', mode=mode).to(dev), pw.DWTInverse(wave='db4', mode=mode).to(dev)
        for J in (2, 3):
            xfm, ifm = pw.WPT2DForward(J=J, wave='db4', mode=mode).to(dev), pw.WPT2DInverse(wave='db4', mode=mode).to(dev)
            sizes = [(H, W)]
            for _ in range(J):
                sizes.append(tuple(ops.coeff_len(n, 8, m) for n in sizes[-1]))

            def compose_fwd(t):
                for _ in range(J):
                    yl, yh = dwt(t)
                    t = torch.cat([yl[:, :, None], yh[0]], 2).view(N, -1, yl.shape[-2], yl.shape[-1])
                return t.view(N, C, -1, t.shape[-2], t.shape[-1])

            def compose_inv(y):
                for j in range(J, 0, -1):
                    y = y.reshape(N, -1, 4, y.shape[-2], y.shape[-1])
                    y = idwt((y[:, :, 0], [y[:, :, 1:]]))[..., :sizes[j - 1][0], :sizes[j - 1][1]]
                return y

            def with_flag(flag, fn):
                def run():
                    ops.WPT_FUSED = flag
                    return fn()
                return run

            r = {}
            ops.WPT_FUSED = False
            with torch.no_grad():
                c0 = pw.launch_count()
                y = xfm(x)
                r['forward_kernels'] = pw.kernels_since(c0)
                c0 = pw.launch_count()
                rec = ifm(y, size=(H, W))
                r['inverse_kernels'] = pw.kernels_since(c0)
                c0 = pw.launch_count()
                yc = compose_fwd(x)
                r['composition_forward_kernels'] = pw.kernels_since(c0)
                r['forward_max_abs_diff_vs_composition'] = float((y.float() - yc.float()).abs().max())
                r['inverse_max_abs_diff_vs_composition'] = float((rec.float() - compose_inv(yc).float()).abs().max())
                nbytes = 2 * J * x.numel() * x.element_size()
                ops.WPT_FUSED = True
                c0 = pw.launch_count()
                y2 = xfm(x)
                r['forward_kernels_two_level'] = pw.kernels_since(c0)
                c0 = pw.launch_count()
                rec2 = ifm(y2, size=(H, W))
                r['inverse_kernels_two_level'] = pw.kernels_since(c0)
                r['two_level_max_abs_diff_vs_level_by_level'] = max(float((y2.float() - y.float()).abs().max()),
                                                                   float((rec2.float() - rec.float()).abs().max()))
                t = _time_alternating([lambda: compose_fwd(x), with_flag(False, lambda: xfm(x)), with_flag(True, lambda: xfm(x))], reps, 5)
                r['forward_composition'], r['forward_level_by_level'], r['forward_two_level'] = (_entry(v, nbytes) for v in t)
                t = _time_alternating([lambda: compose_inv(y), with_flag(False, lambda: ifm(y, size=(H, W))),
                                       with_flag(True, lambda: ifm(y, size=(H, W)))], reps, 5)
                r['inverse_composition'], r['inverse_level_by_level'], r['inverse_two_level'] = (_entry(v, nbytes) for v in t)
                del rec, yc, y2, rec2
            xg = x.clone().requires_grad_(True)
            cot = torch.ones_like(y)

            def step(fn):
                def run():
                    fn(xg).backward(cot)
                    xg.grad = None
                return run
            t = _time_alternating([step(compose_fwd), with_flag(False, step(xfm)), with_flag(True, step(xfm))], max(3, reps // 2), 3)
            r['forward_backward_composition_ms'], r['forward_backward_level_by_level_ms'], r['forward_backward_two_level_ms'] = (
                round(v, 4) for v in t)
            res['%s_J%d' % (mode, J)] = r
            print(dtype_name, mode, J, json.dumps({k: v for k, v in r.items() if not k.endswith('kernels')}), flush=True)
            del y, xg, cot
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs=4, default=[64, 3, 512, 512])
    ap.add_argument('--child', default=None, help='(internal) measure this dtype and print the result as JSON')
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('gpu_wpt2d_probe: no GPU visible (this probe measures; it has no CPU form)')
        res = child(tuple(a.shape), a.child, a.reps)
        res['device'] = torch.cuda.get_device_name(0)
        print('RESULT ' + json.dumps(res), flush=True)
        return
    out = {'shape': a.shape, 'wave': 'db4', 'reps': a.reps, 'hbm_roofline_bytes_per_s': HBM_BYTES_PER_S,
           'algorithmic_bytes': '2 volume-sizes per level',
           'stat': 'median ms of device-event intervals after 5 warm-up rounds; the three routes alternate in one loop',
           'routes': {'composition': '(a) DWTForward(J=1) + torch.cat per level / DWTInverse per level on band slices',
                      'level_by_level': '(b) ops.WPT_FUSED = False: one WlWptAfb<.., 1> / WlWptSfb<.., 1> launch per level',
                      'two_level': '(c) ops.WPT_FUSED = True: WlWptAfb<.., 2> / WlWptSfb<.., 2> for two levels where taken'}}
    for name in ('float32', 'float16'):
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), '--child', name,
               '--reps', str(a.reps), '--shape'] + [str(v) for v in a.shape]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:                               # a fault, an abort or the time limit: nothing more runs on the GPU
            raise SystemExit('gpu_wpt2d_probe: the %s step ended with status %d' % (name, p.returncode))
        out[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        out['device'] = out[name].pop('device')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
