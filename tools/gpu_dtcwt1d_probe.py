"""1-D DTCWT on the MI355X: the fused kernels (WlDt1dFwd / WlDt1dInv, one launch per direction) against the composition of the
single-axis primitives (dtcwt/lowlevel.py colfilter / coldfilt / colifilt on the (N, C, L, 1) view of the same tensors: 2 + 4 (J - 1)
launches, every intermediate lowpass through memory; lengths that need no padding, so no torch.cat), same process, variants
alternating in one loop, device events, medians.  64 x 16 x 65536, near_sym_a / qshift_a, J = 3 and 1, float32 and float16;
forward, inverse, forward + backward.  Fraction of the 8 TB/s roofline at the algorithmic bytes: the input once + the 2x redundant
outputs once (12 B per float32 input sample at J >= 2, 12 at J = 1 as well: lo + hi at full rate).  Writes profiles/dtcwt1d_probe.json (or --out FILE)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_wavelets_amd as pw                                   # noqa: E402
from pytorch_wavelets_amd.dtcwt import lowlevel as ll               # noqa: E402

DEV, SHAPE, REPS, WARM, PEAK = 'cuda:0', (64, 16, 65536), 30, 5, 8e12


def compose_fwd(x, m, J):
    v = x.unsqueeze(-1)
    lo, his = ll.colfilter(v, m.h0o), [ll.colfilter(v, m.h1o)]
    for _ in range(1, J):
        his.append(ll.coldfilt(lo, m.h1b, m.h1a, True))
        lo = ll.coldfilt(lo, m.h0b, m.h0a, False)
    return lo, his


def compose_inv(lo, his, m, swap=False):
    a, b, c, d = (m.g0a, m.g0b, m.g1a, m.g1b) if not swap else (m.g0b, m.g0a, m.g1b, m.g1a)
    for h in his[:0:-1]:
        lo = ll.colifilt(lo, b, a, False) + ll.colifilt(h, d, c, True)
    return ll.colfilter(lo, m.g0o) + ll.colfilter(his[0], m.g1o)


def timed(variants):
    ts = {k: [] for k in variants}
    for it in range(WARM + REPS):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if it >= WARM:
                ts[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in ts.items()}


def main():
    out = {'shape': SHAPE, 'filters': 'near_sym_a/qshift_a', 'reps': REPS, 'rows': []}
    for dtype in (torch.float32, torch.float16):
        for J in (3, 1):
            xf, xi = pw.DTCWT1DForward(J=J).to(DEV), pw.DTCWT1DInverse().to(DEV)
            x = torch.randn(SHAPE, device=DEV).to(dtype)
            xg = x.clone().requires_grad_(True)
            yl, yh = xf(x)
            c0 = pw.launch_count(); xf(x); kf = pw.kernels_since(c0)
            c0 = pw.launch_count(); xi((yl, yh)); ki = pw.kernels_since(c0)
            clo, chis = compose_fwd(x, xf, J)
            err = float((clo.squeeze(-1).float() - yl.float()).abs().max())
            cots = [torch.randn_like(t) for t in [yl] + list(yh)]

            def fb():
                o = xf(xg)
                torch.autograd.grad([o[0]] + list(o[1]), xg, cots)

            t = timed({'fused_fwd': lambda: xf(x), 'compose_fwd': lambda: compose_fwd(x, xf, J),
                       'fused_inv': lambda: xi((yl, yh)), 'compose_inv': lambda: compose_inv(clo, chis, xi),
                       'fused_fwd_bwd': fb,
                       'compose_fwd_plus_inverse_structure': lambda: compose_inv(*compose_fwd(x, xf, J), xi, swap=True)})
            nbytes = x.numel() * x.element_size() * 3                # in once, lo + hi (2x redundant) out once
            row = {'dtype': str(dtype), 'J': J, 'kernels_fwd': kf, 'kernels_inv': ki, 'ms': t, 'algorithmic_bytes': nbytes,
                   'max_abs_diff_fused_vs_compose_yl': err,
                   'roofline_fraction': {k: nbytes * (2 if 'bwd' in k or 'plus' in k else 1) / (v * 1e-3) / PEAK for k, v in t.items()},
                   'speedup': {d: t['compose_' + d] / t['fused_' + d] for d in ('fwd', 'inv')}}
            row['speedup']['fwd_bwd'] = t['compose_fwd_plus_inverse_structure'] / t['fused_fwd_bwd']
            out['rows'].append(row)
            print(json.dumps(row), flush=True)
    dst = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'dtcwt1d_probe.json')
    with open(dst, 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
