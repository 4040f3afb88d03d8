"""The 3-D DWT on the MI355X: the streaming depth kernels (csrc/wl_dwt3d.h) against the generic single-axis kernels on the same
tensors in the same process, each launch's algorithmic bytes over the HBM roofline, and the whole-module times.

    python tools/gpu_dwt3d_probe.py [--out profiles/dwt3d_probe.json] [--reps N] [--shape N C D H W]

Per dtype (float32, float16), db4, symmetric, J = 1, default 8 x 4 x 64 x 256 x 256:
  depth step, analysis:  ops.afb_depth of the 2-D level's four dense outputs into the final (yl, yh) layout (one WlAfbDepth launch)
                         against ops.afb1d along dim 2 per band (WlCorr1d; it needs dense inputs: once with the copies of the three
                         strided high bands that costs it, once on bands made dense beforehand);
  depth step, synthesis: ops.sfb_depth of (yl, yh) into the dense ll / highs (one WlSfbDepth launch) against ops.sfb1d per band pair
                         (WlSynth1d; dense band copies included / excluded likewise) - without the copies into the 2-D
                         layout that the generic path needs afterwards;
  modules:               DWT3DForward, DWT3DInverse, and forward + backward.
Times are medians of device-event intervals after warm-up; the two variants of a step alternate inside one timing loop.
Bytes are what the step must move (every input element read once, every output element written once); the roofline is 8 TB/s."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_wavelets_amd as pw  # noqa: E402
from pytorch_wavelets_amd import ops  # noqa: E402
from pytorch_wavelets_amd.dwt import lowlevel  # noqa: E402

HBM_BYTES_PER_S = 8e12


def _time_alternating(fns, reps, warm):
    """Median device-event time (ms) of every callable in `fns`, the callables taking turns inside the loop."""
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
    return {'ms': round(ms, 4), 'bytes': nbytes, 'roofline_ms': round(nbytes / HBM_BYTES_PER_S * 1e3, 4),
            'fraction_of_hbm_roofline': round(nbytes / HBM_BYTES_PER_S * 1e3 / ms, 3)}


def probe(shape, dtype, reps, warm, dev):
    N, C, D, H, W = shape
    mode = lowlevel.mode_to_int('symmetric')
    xfm = pw.DWT3DForward(J=1, wave='db4', mode='symmetric').to(dev)
    ifm = pw.DWT3DInverse(wave='db4', mode='symmetric').to(dev)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).to(dtype).to(dev)
    res = {}
    with torch.no_grad():
        # ---- the depth step of the analysis, on the 2-D level's real outputs
        ll, highs = lowlevel.AFB2DMulti.apply(x.reshape(N, C * D, H, W), xfm.h0_col, xfm.h1_col, xfm.h0_row, xfm.h1_row, mode, 1)
        Kh, Kw = ll.shape[-2:]
        hv = highs.view(N, C, D, 3, Kh, Kw)
        srcs = [ll.view(N, C, D, Kh, Kw)] + [hv[:, :, :, b] for b in range(3)]
        dense = [s.contiguous() for s in srcs]
        h0, h1 = xfm.h0_dep, xfm.h1_dep
        c0 = pw.launch_count()
        yl, yh = lowlevel._depth_analysis(ll, highs, C, h0, h1, mode)
        res['analysis_kernels'] = pw.kernels_since(c0)
        assert any('WlAfbDepth' in k for k in res['analysis_kernels']), res['analysis_kernels']
        c0 = pw.launch_count()
        ref = [ops.afb1d(s, h0, h1, mode, 2) for s in srcs]
        res['analysis_generic_kernels'] = pw.kernels_since(c0)
        err = max(float((yl - ref[0][0]).abs().max()), max(float((yh[:, :, 3 + b] - ref[b][1]).abs().max()) for b in range(4)))
        res['analysis_max_abs_diff_vs_generic'] = err
        nbytes = (sum(s.numel() for s in srcs) + yl.numel() + yh.numel()) * x.element_size()
        t = _time_alternating([lambda: lowlevel._depth_analysis(ll, highs, C, h0, h1, mode),
                               lambda: [ops.afb1d(s, h0, h1, mode, 2) for s in srcs],
                               lambda: [ops.afb1d(s, h0, h1, mode, 2) for s in dense]], reps, warm)
        res['analysis_depth_kernel'] = _entry(t[0], nbytes)
        res['analysis_generic_with_band_copies'] = _entry(t[1], nbytes)
        res['analysis_generic_dense_inputs'] = _entry(t[2], nbytes)
        del ref, dense
        # ---- the depth step of the synthesis
        g0, g1 = ifm.g0_dep, ifm.g1_dep
        los = [yl] + [yh[:, :, b] for b in range(3)]
        his = [yh[:, :, 3 + b] for b in range(4)]
        dlos, dhis = [t_.contiguous() for t_ in los], [t_.contiguous() for t_ in his]
        c0 = pw.launch_count()
        sl, sh = lowlevel._depth_synthesis(yl, yh, g0, g1, mode)
        res['synthesis_kernels'] = pw.kernels_since(c0)
        assert any('WlSfbDepth' in k for k in res['synthesis_kernels']), res['synthesis_kernels']
        ref = [ops.sfb1d(a, b, g0, g1, mode, 2) for a, b in zip(los, his)]
        res['synthesis_max_abs_diff_vs_generic'] = max(
            float((sl.view(N, C, -1, Kh, Kw) - ref[0]).abs().max()),
            max(float((sh.view(N, C, -1, 3, Kh, Kw)[:, :, :, b] - ref[1 + b]).abs().max()) for b in range(3)))
        nbytes = (yl.numel() + yh.numel() + sl.numel() + sh.numel()) * x.element_size()
        t = _time_alternating([lambda: lowlevel._depth_synthesis(yl, yh, g0, g1, mode),
                               lambda: [ops.sfb1d(a, b, g0, g1, mode, 2) for a, b in zip(los, his)],
                               lambda: [ops.sfb1d(a, b, g0, g1, mode, 2) for a, b in zip(dlos, dhis)]], reps, warm)
        res['synthesis_depth_kernel'] = _entry(t[0], nbytes)
        res['synthesis_generic_with_band_copies'] = _entry(t[1], nbytes)
        res['synthesis_generic_dense_inputs'] = _entry(t[2], nbytes)
        del ref, dlos, dhis, sl, sh, los, his, srcs, hv, ll, highs
        torch.cuda.empty_cache()
        # ---- the modules
        c0 = pw.launch_count()
        out = xfm(x)
        res['forward_kernels'] = pw.kernels_since(c0)
        c0 = pw.launch_count()
        ifm(out)
        res['inverse_kernels'] = pw.kernels_since(c0)
        vol = x.numel() * x.element_size()
        t = _time_alternating([lambda: xfm(x), lambda: ifm(out)], reps, warm)
        # what a level must move: the volume in, the eight bands out (about the volume again)
        res['module_forward'] = _entry(t[0], vol + (out[0].numel() + out[1][0].numel()) * x.element_size())
        res['module_inverse'] = _entry(t[1], vol + (out[0].numel() + out[1][0].numel()) * x.element_size())
        del out
    xg = x.clone().requires_grad_(True)

    def step():
        yl, yh = xfm(xg)
        torch.autograd.backward([yl, yh[0]], [yl.detach(), yh[0].detach()])
        xg.grad = None
    res['module_forward_backward_ms'] = round(_time_alternating([step], max(3, reps // 2), 2)[0], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--shape', type=int, nargs=5, default=[8, 4, 64, 256, 256])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('gpu_dwt3d_probe: no GPU visible (this probe measures; it has no CPU form)')
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'shape': a.shape, 'wave': 'db4', 'mode': 'symmetric', 'J': 1, 'reps': a.reps,
           'stat': 'median ms of device-event intervals after 5 warm-up rounds; variants of a step alternate in one loop',
           'hbm_roofline_bytes_per_s': HBM_BYTES_PER_S}
    for name, dt in (('float32', torch.float32), ('float16', torch.float16)):
        res[name] = probe(tuple(a.shape), dt, a.reps, 5, dev)
        print(name, json.dumps({k: v for k, v in res[name].items() if not k.endswith('kernels')}), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
