"""float32 / float16 / bfloat16 on the MI355X: forward and inverse (or training step) times with device events after warm-up,
the kernels each direction launches (pw.kernels_since) and the output error against float32, for the four GPU configurations
of BASELINE.json and the near_sym_b / near_sym_b_bp rows of the README table.  The modules are converted to the data dtype
(`.to(dtype)`: rounded taps), as the float16 configuration of BASELINE.json is.

    python tools/gpu_bf16_probe.py [--out FILE.json] [--reps N] [--quick]

--quick: a few repetitions per row (for a `rocprofv3 --kernel-trace --stats` run, which gives the kernel durations)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_wavelets_amd as pw  # noqa: E402

DTYPES = [('float32', torch.float32), ('float16', torch.float16), ('bfloat16', torch.bfloat16)]


def _dwt(J, wave, mode):
    return lambda: (pw.DWTForward(J=J, wave=wave, mode=mode), pw.DWTInverse(wave=wave, mode=mode))


def _dtcwt(J, biort, qshift):
    return lambda: (pw.DTCWTForward(J=J, biort=biort, qshift=qshift), pw.DTCWTInverse(biort=biort, qshift=qshift))


def _scat(biort):
    return lambda: (pw.ScatLayer(biort=biort), None)


ROWS = [
    ('DWT J=3 db4 symmetric 128x3x512^2', (128, 3, 512, 512), _dwt(3, 'db4', 'symmetric')),
    ('DTCWT J=3 near_sym_a/qshift_a 64x3x512^2', (64, 3, 512, 512), _dtcwt(3, 'near_sym_a', 'qshift_a')),
    ('ScatLayer near_sym_a 256x3x256^2', (256, 3, 256, 256), _scat('near_sym_a')),
    ('DWT J=4 db8 periodization 32x16x2048^2', (32, 16, 2048, 2048), _dwt(4, 'db8', 'periodization')),
    ('DTCWT J=3 near_sym_b/qshift_b 64x3x512^2', (64, 3, 512, 512), _dtcwt(3, 'near_sym_b', 'qshift_b')),
    ('ScatLayer near_sym_b 256x3x256^2', (256, 3, 256, 256), _scat('near_sym_b')),
    ('ScatLayer near_sym_b_bp 256x3x256^2', (256, 3, 256, 256), _scat('near_sym_b_bp')),
]


def _flat(v):
    if torch.is_tensor(v):
        return [] if v.dim() == 0 else [v]
    return [t for u in v for t in _flat(u)]


def _time(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--quick', action='store_true')
    a = ap.parse_args()
    reps, warm = (3, 2) if a.quick else (a.reps, 5)
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'stat': 'median ms (device events)', 'rows': []}
    for name, shape, make in ROWS:
        g = torch.Generator().manual_seed(0)
        x32 = torch.randn(shape, generator=g).to(dev)
        row = {'row': name}
        ref = None
        for dname, dt in DTYPES:
            fwd, inv = (m.to(dev).to(dt) if m is not None else None for m in make())
            x = x32.to(dt)
            with torch.no_grad():
                c0 = pw.launch_count()
                out = fwd(x)
                kf = pw.kernels_since(c0)
                tf = _time(lambda: fwd(x), reps, warm)
                ent = {'fwd_ms': round(tf, 4), 'fwd_kernels': kf}
                if inv is not None:
                    c0 = pw.launch_count()
                    rec = inv(out)
                    ent['inv_kernels'] = pw.kernels_since(c0)
                    ent['inv_ms'] = round(_time(lambda: inv(out), reps, warm), 4)
                    outs = _flat(out) + [rec]
                else:
                    outs = _flat(out)
            if inv is None:   # ScatLayer: the training step (forward + backward) in place of an inverse
                xg = x.clone().requires_grad_(True)

                def step():
                    z = fwd(xg)
                    z.backward(torch.ones_like(z))
                c0 = pw.launch_count()
                step()
                ent['train_kernels'] = pw.kernels_since(c0)
                ent['train_ms'] = round(_time(step, reps, warm), 4)
            if ref is None:
                ref = [o.float() for o in outs]
            ent['rel_err_vs_float32'] = max(float((o.float() - r).abs().max() / r.abs().max().clamp_min(1e-30)) for o, r in zip(outs, ref))
            row[dname] = ent
            del out, outs
            torch.cuda.synchronize()
        for k in ('fwd_ms', 'inv_ms', 'train_ms'):
            if k in row['float16']:
                row['bf16_over_f16_' + k] = round(row['bfloat16'][k] / row['float16'][k], 3)
        res['rows'].append(row)
        print(json.dumps({kk: v for kk, v in row.items() if not isinstance(v, dict)}), {d: {k: v for k, v in row[d].items() if not k.endswith('kernels')} for d, _ in DTYPES}, flush=True)
        del x32
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
