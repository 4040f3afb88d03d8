#!/usr/bin/env python
"""Benchmark of the hot path on synthetic data resident in HBM.  Default workload = BASELINE.json configs[1]:
DWTForward + DWTInverse, J=3 db4 symmetric, N x 3 x 512 x 512 fp32.

    python bench.py --gpus 1 --steps 20 --warmup 5                     # the metric
    python bench.py --gpus 1 --steps 20 --warmup 5 --full              # + roofline, other configs, CPU baseline
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR  # + the last step's outputs as DIR/<name>.npy
    python bench.py --config dtcwt|scat|cfg5 ...                       # the other BASELINE configs, same flow
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W [--config ...]

A "step" = one pass of the workload over this rank's batch (dwt / dtcwt: forward + inverse; scat, cfg5: forward).
The batch dimension shards with no data-path collective; the only collective is the one-off broadcast of the filter
banks from rank 0.  dwt / dtcwt / cfg5 scale weakly (the configured batch per GPU); scat is BASELINE configs[3]:
256 images split over the ranks (strong).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up (W steps + the clock ramp), times exactly K steps and prints the headline line (`value`,
`ms_per_step`).  --full adds everything else the line used to carry: the cold figure of a fresh process, the per-part
durations and the HBM roofline, the per-level tile kernels, device-copy / membench figures, the other configs and the
CPU baseline.
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

# multi-process GPU work on this pool needs dmabuf IPC (the host driver supports nothing else: without it RCCL's rendezvous fails with
# hipIpcGetMemHandle: invalid argument); already exported on the pool's boxes, kept for any environment that launches this file
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); a float4 copy reaches ~6300 GB/s


def algorithmic_bytes_fwd(N, C, H, W, J, L, itemsize, periodization=False):
    """every input element read once, every output element written once."""
    n_out = 0
    h, w = H, W
    for _ in range(J):
        h, w = ((h + 1) // 2, (w + 1) // 2) if periodization else ((h + L - 1) // 2, (w + L - 1) // 2)
        n_out += 3 * h * w
    n_out += h * w
    return N * C * (H * W + n_out) * itemsize


def source_digest():
    """sha256 over the engine's sources: profiles/*_hbm_traffic.json records the digest of the build it was measured
    on, and the roofline only quotes it when it matches what is running."""
    import hashlib
    h = hashlib.sha256()
    for d, exts in ((os.path.join(ROOT, 'pytorch_wavelets_amd', 'csrc'), ('.h', '.inc', '.hip')),
                    (os.path.join(ROOT, 'include'), ('.h',))):
        for f in sorted(os.listdir(d)):
            if f.endswith(exts):
                h.update(f.encode())
                h.update(open(os.path.join(d, f), 'rb').read())
    return h.hexdigest()[:16]


def cpu_baseline(args):
    """The reference's CPU path, restated: oracle/torch_cpu.py = its gather + grouped conv2d / conv_transpose2d
    formulation on PyTorch-CPU (the reference itself is Python on ATen and cannot travel to this box; the restatement is
    pinned to its golden vectors by tests/test_oracle_golden.py), on a bounded sample of the workload.
    The OpenMP C port of the numpy oracle (oracle/dwt_port.c) is timed next to it."""
    import numpy as np
    from oracle import torch_cpu as tc
    from pytorch_wavelets_amd import filters
    h0, h1 = filters.dwt_analysis_taps('db4')
    g0, g1 = filters.dwt_synthesis_taps('db4')
    ncores = os.cpu_count() or 1
    n = 16
    x = torch.randn(n, 3, 512, 512, generator=torch.Generator().manual_seed(0))

    def once():
        with torch.no_grad():
            yl, yh = tc.dwt_forward(x, 3, h0, h1, 'symmetric')
            return tc.dwt_inverse(yl, yh, g0, g1, 'symmetric')
    # ATen's grouped convolutions do not scale to hundreds of threads (256 threads measured 20x slower than 8 on the
    # MI355X host): time a few intra-op pool sizes for ~3 s each and report the best one, with the cores it used
    tried, best = {}, None
    for nt in sorted(set(t for t in (8, 16, 32, 64, ncores) if t <= ncores)):
        torch.set_num_threads(nt)
        once()
        reps, t0 = 0, time.perf_counter()
        while reps < 2 or time.perf_counter() - t0 < 3.0:
            once()
            reps += 1
        mp = x.numel() / ((time.perf_counter() - t0) / reps) / 1e6
        tried[str(nt)] = round(mp, 2)
        if best is None or mp > best[1]:
            best = (nt, mp, reps)
    out = {'value': round(best[1], 2), 'unit': 'Mpixels/s', 'cores': best[0], 'kind': 'port',
           'port_of': 'the reference\'s own formulation restated on PyTorch-CPU (oracle/torch_cpu.py)',
           'host_cores': ncores, 'mpix_s_by_torch_threads': tried,
           'sample': 'oracle/torch_cpu.py (the reference\'s conv2d / conv_transpose2d formulation on PyTorch-CPU, fp32), '
                     'fwd+inv J=3 db4 symmetric on %dx3x512x512, %d reps at the best thread count; the real reference '
                     'measured 23.0 Mpixels/s on the 8 vCPU of the authoring container with this torch build '
                     '(profiles/r02_reference_cpu_timing.json; BASELINE.md quotes 16.2 for an older torch)' % (n, best[2])}
    try:
        from oracle import dwt_port
        rng = np.random.RandomState(0)
        m = max(2, min(64, ncores))
        xp = rng.randn(m, 3, 512, 512).astype(np.float32)
        dwt_port.fwd_inv(xp, 3, h0, h1, g0, g1, 'symmetric', threads=ncores)
        reps, t0 = 0, time.perf_counter()
        while reps < 3 or time.perf_counter() - t0 < 5.0:
            dwt_port.fwd_inv(xp, 3, h0, h1, g0, g1, 'symmetric', threads=ncores)
            reps += 1
        out['c_port'] = {'value': round(xp.size / ((time.perf_counter() - t0) / reps) / 1e6, 2), 'unit': 'Mpixels/s',
                         'kind': 'port', 'sample': 'oracle/dwt_port.c (OpenMP, one plane per thread) on %dx3x512x512' % m}
    except Exception as e:   # the C port is optional
        out['c_port'] = {'error': str(e)[:80]}
    return out


def membench():
    """tools/micro/bin/membench (built by __graft_entry__.build()): what plain copy / read / write kernels reach on
    THIS box with the footprint of the forward launch, in the access forms the engine uses."""
    exe = os.path.join(ROOT, 'tools', 'micro', 'bin', 'membench')
    if not os.path.exists(exe):
        return None
    try:
        res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120)
        return json.loads(res.stdout.decode().strip().splitlines()[-1])
    except Exception as e:
        return {'error': str(e)[:80]}


class Workload(object):
    """One BASELINE config: modules, this rank's input, the parts of a step ('f' forward, 'i' inverse) and their
    algorithmic bytes."""
    scaling = 'weak'
    seq = 'fi'

    def run(self, part):
        with torch.no_grad():
            if part == 'f':
                self.coefs = self.xfm(self.x)
                return self.coefs
            self.rec = self.ifm(self.coefs)
            return self.rec

    def step(self):
        for p in self.seq:
            out = self.run(p)
        return out

    def outputs(self):
        """(name, tensor) of what a caller of the last step received: the forward's coefficients, then the inverse's
        reconstruction when the step has one."""
        outs = _named('forward', self.coefs)
        if 'i' in self.seq:
            outs.append(('inverse', self.rec))
        return outs


def _named(prefix, obj):
    if torch.is_tensor(obj):
        return [(prefix, obj)]
    if len(obj) == 2 and isinstance(obj[1], (list, tuple)):     # (yl, yh) of the DWT / DTCWT modules
        return [(prefix + '_yl', obj[0])] + [(prefix + '_yh%d' % j, h) for j, h in enumerate(obj[1]) if h is not None]
    return [a for i, o in enumerate(obj) for a in _named('%s_%d' % (prefix, i), o)]


DUMP_BUDGET = 60 << 20      # bytes of .npy data one --dump-outputs writes at most


def dump_outputs(named, outdir):
    """--dump-outputs: every array as outdir/<name>.npy, float32 (float64 stays float64).  An array larger than its share of
    DUMP_BUDGET is written as a fixed sample of its flattened elements: one element drawn (seed 0) from each of `cap` equal
    slices, so two runs with the same arguments write the same indices and can be compared element for element."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    share = DUMP_BUDGET // max(1, len(named))
    for name, t in named:
        t = t.detach()
        if t.is_complex():
            t = torch.view_as_real(t)
        dt = torch.float64 if t.dtype == torch.float64 else torch.float32
        cap = share // (8 if dt == torch.float64 else 4)
        n = t.numel()
        if n > cap:
            rng = np.random.RandomState(0)
            lo = np.arange(cap, dtype=np.int64) * n // cap
            hi = np.arange(1, cap + 1, dtype=np.int64) * n // cap
            idx = lo + (rng.random_sample(cap) * (hi - lo)).astype(np.int64)
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(outdir, name + '.npy'), t.to(dt).cpu().numpy())


class DwtWorkload(Workload):
    key = 'dwt'
    metric = 'Mpixels/s fwd+inv DWT J=3 db4, Nx3x512x512 fp32; % HBM roofline'
    dtype_name = 'f32'

    def __init__(self, pw, dev, rank, world, args, emu):
        self.N = args.batch or 128
        self.C, self.H, self.W, self.J = 3, (64 if emu else 512), (64 if emu else 512), 3
        self.xfm = pw.DWTForward(J=3, wave='db4', mode='symmetric').to(dev)
        self.ifm = pw.DWTInverse(wave='db4', mode='symmetric').to(dev)
        self.x = torch.randn(self.N, 3, self.H, self.W, device=dev, generator=torch.Generator(device=dev).manual_seed(1234 + rank))
        b = algorithmic_bytes_fwd(self.N, 3, self.H, self.W, 3, 8, 4)
        self.bytes = {'f': b, 'i': b}
        self.global_batch = world * self.N
        self.workload = ('DWTForward+DWTInverse J=3 db4 symmetric, %dx3x%dx%d fp32 per GPU (BASELINE configs[1])'
                         % (self.N, self.H, self.W))


class DtcwtWorkload(Workload):
    key = 'dtcwt'
    metric = 'Mpixels/s fwd+inv DTCWT J=3 near_sym_a/qshift_a, Nx3x512x512 fp32; % HBM roofline'
    dtype_name = 'f32'

    def __init__(self, pw, dev, rank, world, args, emu):
        self.N = args.batch or 64
        self.C, self.H, self.W, self.J = 3, (32 if emu else 512), (32 if emu else 512), 3
        self.xfm = pw.DTCWTForward(J=3, biort='near_sym_a', qshift='qshift_a').to(dev)
        self.ifm = pw.DTCWTInverse(biort='near_sym_a', qshift='qshift_a').to(dev)
        self.x = torch.randn(self.N, 3, self.H, self.W, device=dev, generator=torch.Generator(device=dev).manual_seed(1234 + rank))
        b = 20 * self.x.numel()      # out = exactly 4.0 P per plane -> 5 P x 4 B
        self.bytes = {'f': b, 'i': b}
        self.global_batch = world * self.N
        self.workload = ('DTCWTForward+DTCWTInverse J=3 near_sym_a qshift_a, %dx3x%dx%d fp32 per GPU (BASELINE configs[2])'
                         % (self.N, self.H, self.W))


class ScatWorkload(Workload):
    key = 'scat'
    metric = 'Mpixels/s ScatLayer (DTCWT scatternet, 6 orientations), 256x3x256x256 fp32 batch-sharded; % HBM roofline'
    dtype_name = 'f32'
    scaling = 'strong'
    seq = 'f'

    def __init__(self, pw, dev, rank, world, args, emu):
        from pytorch_wavelets_amd import parallel
        total = args.batch or 256
        lo, hi = parallel.shard_bounds(total, world, rank)
        self.N = hi - lo
        self.C, self.H, self.W = 3, (32 if emu else 256), (32 if emu else 256)
        self.xfm = pw.ScatLayer().to(dev)
        self.ifm = None
        self.x = torch.randn(self.N, 3, self.H, self.W, device=dev, generator=torch.Generator(device=dev).manual_seed(1234 + rank))
        self.bytes = {'f': 11 * self.x.numel()}     # read P, write 7P/4
        self.global_batch = total
        self.workload = ('ScatLayer near_sym_a, %dx3x%dx%d fp32 in total, %d images on this rank (BASELINE configs[3])'
                         % (total, self.H, self.W, self.N))


class Cfg5Workload(Workload):
    key = 'cfg5'
    metric = 'Mpixels/s DWTForward J=4 db8 periodization, Nx16x2048x2048 fp16; % HBM roofline'
    dtype_name = 'f16'
    seq = 'f'

    def __init__(self, pw, dev, rank, world, args, emu):
        self.N = args.batch or 32
        self.C, self.H, self.W, self.J = (2 if emu else 16), (128 if emu else 2048), (128 if emu else 2048), 4
        self.xfm = pw.DWTForward(J=4, wave='db8', mode='periodization').to(dev).half()
        self.ifm = pw.DWTInverse(wave='db8', mode='periodization').to(dev).half()
        self.x = torch.randn(self.N, self.C, self.H, self.W, device=dev, dtype=torch.float16,
                             generator=torch.Generator(device=dev).manual_seed(1234 + rank))
        b = 4 * self.x.numel()       # critically sampled: out = exactly P -> 2 P x 2 B
        self.bytes = {'f': b, 'i': b}
        self.global_batch = world * self.N
        self.workload = ('DWTForward J=4 db8 periodization, %dx%dx%dx%d fp16 per GPU (BASELINE configs[4]); the inverse is '
                         'timed beside it' % (self.N, self.C, self.H, self.W))


WORKLOADS = {w.key: w for w in (DwtWorkload, DtcwtWorkload, ScatWorkload, Cfg5Workload)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100,
                    help='timed steps (default 100: the ~0.3 ms the barrier / synchronize at either end of the timed region cost '
                         'are then under 1 %% of it; with 20 steps they were 4 %%)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--config', choices=sorted(WORKLOADS), default='dwt',
                    help='dwt = BASELINE configs[1] (the metric); dtcwt / scat / cfg5 = configs[2] / [3] / [4]')
    ap.add_argument('--batch', type=int, default=0, help='images per GPU (scat: in total); 0 = the BASELINE value')
    ap.add_argument('--full', action='store_true',
                    help='also measure the cold figure, the per-part roofline, the tile kernels, device copies, the other configs '
                         'and the CPU baseline (a plain run times the headline steps only)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the outputs of the last timed step as DIR/<name>.npy (float32; a fixed sample of a large array)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-other-configs', action='store_true', help='with --full: skip the context timings of the other configs')
    ap.add_argument('--emulate', action='store_true',
                    help='TEST ONLY: run the whole harness on CPU tensors through the host emulation of the kernels '
                         '(tests/emu) with the gloo backend - exercises the multi-rank control flow without a GPU')
    args = ap.parse_args()

    import __graft_entry__ as ge
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    emu = args.emulate
    if emu:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import emu_backend
        from pytorch_wavelets_amd import ops
        ops._TEST_BACKEND = emu_backend.handle()
    elif rank == 0:
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):     # (stdout carries the ONE JSON line and nothing else)
            ge.build()
    import pytorch_wavelets_amd as pw
    from pytorch_wavelets_amd import parallel
    if not emu:
        assert torch.cuda.is_available(), 'bench.py needs a GPU'
        dev = torch.device('cuda', local_rank)
        torch.cuda.set_device(dev)
    else:
        dev = torch.device('cpu')
    if world > 1:
        import torch.distributed as dist
        if emu:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=dev)   # nccl == RCCL on ROCm
        dist.barrier()   # (ranks > 0 load the library rank 0 has just built only after this point)

    def sync():
        if not emu:
            torch.cuda.synchronize()

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        sync()

    wl = WORKLOADS[args.config](pw, dev, rank, world, args, emu)
    if world > 1:
        parallel.broadcast_filter_banks(wl.xfm, src=0)
        if wl.ifm is not None:
            parallel.broadcast_filter_banks(wl.ifm, src=0)
    K = args.steps

    def timed_region():
        """W warmup steps, then EXACTLY K steps between barrier + synchronize on both sides; MAX over ranks."""
        # (the cyclic garbage collector is frozen + disabled ONCE, before the first region - see below: nothing may idle the
        # device between the warm-up and t0, a 45 ms gc.collect() there let the clocks the ramp had just raised fall again)
        for _ in range(args.warmup):
            wl.step()
        barrier()
        t0 = time.perf_counter()
        stamps = []
        for _ in range(K):
            out = wl.step()
            stamps.append(time.perf_counter())
        t_issued = time.perf_counter()
        barrier()
        dt = time.perf_counter() - t0
        host_issue.append((t_issued - t0) / K * 1e3)
        if os.environ.get('WL_BENCH_STAMPS'):
            print('[stamps] host ms per step: %s; drain %.2f ms' % (' '.join('%.2f' % ((b - a) * 1e3) for a, b in zip([t0] + stamps, stamps)),
                                                                   (t0 + dt - stamps[-1]) * 1e3), file=sys.stderr, flush=True)
        if world > 1:
            tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
            dt = float(tmax.item())
        return dt, out

    # The cyclic garbage collector stays out of everything that is timed (like timeit): a full collection of a process that has
    # imported torch takes 35-65 ms (the whole timed region of --config dtcwt is 6 ms).  Collect once NOW, freeze the survivors
    # (they are never scanned again) and switch the collector off until the timing is over - never between a warm-up and its
    # timed region (round 3 did that: the device idled for 45 ms and dropped the clocks the ramp steps had paid for).
    host_issue = []
    gc.collect()
    gc.freeze()
    gc.disable()
    # 1. cold (--full): a fresh process, W warmup steps, K timed steps - the number a one-shot caller sees
    if args.full:
        dt_cold, _ = timed_region()
    # 2. steady: the GPU takes ~20 ms of continuous work to reach its steady clocks (tools/gpu_rampup_probe.py: the first
    #    ~100 launches of a cold process run ~10 % slower); a job of any realistic length lives here.  `value` is this one,
    #    the cold figure is printed beside it.
    RAMP_STEPS = 0 if emu else 100
    for _ in range(RAMP_STEPS):
        wl.step()
    dt, out = timed_region()
    last_outputs = wl.outputs()      # (held: the measurements of --full below run the transforms again)

    def headline():
        """The result line of a plain run."""
        pixels = wl.x.numel() * world if wl.scaling == 'weak' else wl.global_batch * wl.C * wl.H * wl.W
        return {
            'metric': wl.metric,
            'value': round(pixels * K / dt / 1e6, 1),
            'unit': 'Mpixels/s',
            'n_gpus': world, 'steps': K, 'warmup': args.warmup,
            'ms_per_step': round(dt / K * 1e3, 4),
            'host_issue_ms_per_step': round(host_issue[-1], 4),
            'higher_is_better': True, 'scaling': wl.scaling, 'vs_baseline': None,
            'clock_ramp_steps_untimed': RAMP_STEPS,
            'dtype': wl.dtype_name,
            'data': 'synthetic (HOST EMULATION of the kernels: control-flow test, not a measurement)' if emu else 'synthetic',
            'config': {'workload': wl.workload, 'global_batch': wl.global_batch,
                       'parallelism': 'batch-sharded x%d, no data-path collective' % world,
                       'step': ' + '.join({'f': 'forward', 'i': 'inverse'}[p] for p in wl.seq)},
        }

    def finish(line):
        if rank == 0:
            gc.enable()
            gc.unfreeze()
            if args.dump_outputs:
                dump_outputs(last_outputs, args.dump_outputs)
            print(json.dumps(line), flush=True)
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()

    if not args.full:
        finish(headline() if rank == 0 else None)
        return

    err = None
    if wl.seq == 'fi':
        err = float((out - wl.x).abs().max() / wl.x.abs().max())

    # ---- per-part durations WITHOUT touching the stream between launches.  HIP events only bracket whole loops of K
    # iterations of a launch sequence: S = the step itself, S + 'f' = the step with the forward issued twice, S + 'i' with
    # the inverse twice.  duration(forward) = T(S + f) - T(S), duration(inverse) = T(S + i) - T(S): the kernels run in the
    # same back-to-back stream as in the timed region (the rocprofv3 trace of this command shows Start[k+1] == End[k]),
    # no event packet sits between two launches, and forward + inverse must add up to the step (reported as `closure`).
    # every kernel a part launches, by name (wl_kernel_history of the C ABI); the label of a multi-launch part is its FIRST
    # launch = the finest level, which moves 3/4 and more of the part's bytes (DWT levels halve twice; the DTCWT's level 1,
    # or levels 1 + 2 fused, carries 16 of its 20 bytes per pixel)
    kernel, launches = {}, {}
    for p in ('f', 'i') if wl.ifm is not None else ('f',):
        c0 = pw.launch_count()
        wl.run(p)
        launches[p] = pw.kernels_since(c0)
        # (the label: a kernel that does the transform's work - not the one-thread examination of the filter banks in front of a
        # lattice launch, "(aux)", nor the two-bank variant queued behind a hinted one, "(armed fallback)", which returns at once)
        prim = [k for k in launches[p] if not k.endswith(')')]
        order = prim if p == 'f' else prim[::-1]                    # (an inverse runs coarsest level first)
        kernel[p] = order[0] if order else pw.last_kernel()
    parts = [p for p in 'fi' if p == 'f' or wl.ifm is not None]

    def time_seq(seq, n):
        for _ in range(3):
            for p in seq:
                wl.run(p)
        sync()
        if emu:
            t0 = time.perf_counter()
            for _ in range(n):
                for p in seq:
                    wl.run(p)
            return (time.perf_counter() - t0) * 1e3 / n
        prefill(2.0)      # (the host queues the loop while the device is still busy: no launch gaps inside the bracket)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            for p in seq:
                wl.run(p)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    seqs = {'S': wl.seq}
    for p in parts:
        seqs['S+' + p] = wl.seq + p
    samples = {k: [] for k in seqs}
    for _ in range(1 if emu else 5):           # interleaved repetitions, medians: box noise hits every sequence alike
        for k, s in seqs.items():
            samples[k].append(time_seq(s, K))
    med = {k: sorted(v)[len(v) // 2] for k, v in samples.items()}
    part_ms = {p: max(med['S+' + p] - med['S'], 1e-6) for p in parts}
    closure = sum(part_ms[p] for p in wl.seq) / med['S']

    # the same transforms as one tile-kernel launch per level (the round-1 path), for the record (dwt only)
    tile = {}
    if wl.key == 'dwt':
        from pytorch_wavelets_amd.dwt import lowlevel as _ll
        _ll.FUSED_LEVELS = False
        try:
            for p in parts:
                base = time_seq(wl.seq, K)
                t_part = max(time_seq(wl.seq + p, K) - base, 1e-6)   # (a difference of two noisy loops: never zero or below - the emulated runs of the CPU tests met 0.0)
                tile[p] = {'avg_ms': round(t_part, 4)}
                wl.run(p)
                tile[p]['kernel'] = pw.last_kernel()
                tile[p]['frac'] = round(wl.bytes[p] / (t_part * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        finally:
            _ll.FUSED_LEVELS = True
    # what plain device copies of the same footprint achieve on this box
    copy_gbs, mb = None, None
    if not emu and rank == 0:
        with torch.no_grad():
            cdst = torch.empty_like(wl.x)
            copy_gbs = 2 * wl.x.numel() * wl.x.element_size() / (time_seq_fn(lambda: cdst.copy_(wl.x), K, sync) * 1e-3) / 1e9
            del cdst
        if world == 1:
            mb = membench()

    other = None
    if world == 1 and not args.no_other_configs and not emu and wl.key == 'dwt':
        other = other_configs(pw, dev, sync)

    # HBM traffic of the dominant kernels: only from a PMC summary measured on THIS build of the sources
    traffic = {}
    import glob
    tpaths = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_hbm_traffic.json' if wl.key == 'dwt'
                                           else 'r[0-9][0-9]_%s_hbm_traffic.json' % wl.key)), reverse=True)
    for tpath in ([] if emu else tpaths):      # newest round first; a file counts only if it was measured on this build
        try:
            tj = json.load(open(tpath))
            if tj.get('source_digest') == source_digest() and not traffic:
                for k, v in tj.get('kernels', {}).items():   # rocprof prints defaulted template arguments too
                    for p in parts:                          # (several instantiations may share the prefix: the largest one is the part's kernel)
                        if k.strip().startswith(kernel[p].rstrip('>')) and (v.get('hbm_bytes_corrected') or 0) > (traffic.get(p) or 0):
                            traffic[p] = v.get('hbm_bytes_corrected')
        except Exception:
            traffic = {}

    if rank == 0:
        per_rank_px = wl.x.numel()
        pixels = per_rank_px * world if wl.scaling == 'weak' else wl.global_batch * wl.C * wl.H * wl.W

        def block(p):
            gbs = wl.bytes[p] / (part_ms[p] * 1e-3) / 1e9
            b = {'kernel': kernel[p], 'launches': launches[p], 'achieved': round(gbs, 1), 'frac': round(gbs / HBM_PEAK_GBS, 4),
                 'avg_launch_ms': round(part_ms[p], 4), 'algorithmic_bytes_per_launch': wl.bytes[p],
                 'traffic': traffic.get(p)}
            if copy_gbs:
                best = max([copy_gbs] + [v for k, v in (mb or {}).items() if k.startswith('copy_') and isinstance(v, (int, float))])
                b['frac_of_device_copy'] = round(gbs / best, 4)
            if p in tile:
                b['per_level_tile_kernels'] = tile[p]
            return b
        roof = {'bound': 'hbm', 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                'how_timed': 'HIP events bracket whole loops of %d iterations of a launch sequence on the launch stream, never '
                             'single launches: T(step), T(step + forward), T(step + inverse), 5 interleaved repetitions each, '
                             'medians; duration(part) = T(step + part) - T(step).  closure = (sum of the parts of a step) / '
                             'T(step)' % K,
                'closure': round(closure, 4), 'step_ms_events': round(med['S'], 4)}
        roof.update(block('f'))
        if wl.key == 'cfg5':
            # config 5 is borderline VALU-bound - both bounds in the line.  VALU roofline of the arithmetic the
            # kernels execute: 17 packed FMAs (v_pk_fma_f32) per output sample at 16 taps (L row taps + L column taps + 1, on
            # (lo, hi) pairs), one output sample per input pixel and level (critically sampled: sum over 4 levels = 1.328 P);
            # a wave64 VALU instruction occupies its SIMD for 4 cycles; 256 CUs x 4 SIMDs at 2.4 GHz (MI355X_MICROARCH.md).
            # Round 5: with the lattice column pass (csrc/wl_lattice.h: K = L/2 rotations instead of L taps) it is L + L/2 + 0.5 = 12.5
            # per output sample - the VALU floor then lies under the HBM floor and the line says bound: "hbm".
            samples = wl.x.numel() * sum(0.25 ** j for j in range(wl.J))
            lattice = any(k.startswith('WlAfbStrip<') and k.rstrip('>').endswith(', 1, 1') for k in launches['f'])
            fma_per_sample = 12.5 if lattice else 17
            valu_min_ms = samples * fma_per_sample * 4 / 64 / (1024 * 2.4e9) * 1e3
            hbm_min_ms = wl.bytes['f'] / (HBM_PEAK_GBS * 1e9) * 1e3
            roof['bound'] = 'valu' if valu_min_ms > hbm_min_ms else 'hbm'
            roof['valu'] = {'bound': 'valu', 'unit': 'ms', 'min_ms_at_valu_peak': round(valu_min_ms, 4),
                            'min_ms_at_hbm_peak': round(hbm_min_ms, 4),
                            'frac': round(valu_min_ms / part_ms['f'], 4),
                            'what': '%g v_pk_fma_f32 per output sample (%s) x 1.328 samples per pixel, 4 cycles per wave64 '
                                    'instruction and SIMD, 1024 SIMDs at 2.4 GHz'
                                    % (fma_per_sample, 'lattice column pass' if lattice else 'direct form')}
            if 'i' in part_ms:
                roof['valu']['inverse_frac'] = round(valu_min_ms / part_ms['i'], 4)
        if wl.key == 'dwt':
            roof['launches_per_forward'] = len(launches['f'])
        if 'i' in part_ms:
            roof['inverse'] = block('i')
        if copy_gbs:
            roof['device_copy_gbs'] = round(copy_gbs, 1)
            roof['device_copy_kind'] = 'torch.Tensor.copy_ of the input footprint (read + write bytes / time); see membench'
        if mb is not None:
            roof['membench'] = mb
        out = headline()
        out.update({
            'step_ms_events': round(med['S'], 4),
            'timing_consistent': bool(abs(dt / K * 1e3 / med['S'] - 1.0) < 0.05),
            'cold': {'ms_per_step': round(dt_cold / K * 1e3, 4), 'value': round(pixels * K / dt_cold / 1e6, 1),
                     'what': 'the first %d steps of the process after %d warmup steps, before the %d ramp steps'
                             % (K, args.warmup, RAMP_STEPS)},
            'roofline': roof,
        })
        for p in parts:
            out['%s_mpix_s' % ('fwd' if p == 'f' else 'inv')] = round(per_rank_px / (part_ms[p] * 1e-3) / 1e6, 1)
        if err is not None:
            out['roundtrip_rel_err'] = err
        if other is not None:
            out['other_configs'] = other
        gc.enable()
        gc.unfreeze()
        if not args.no_cpu_baseline and world == 1 and not emu and wl.key == 'dwt':
            out['cpu_baseline'] = cpu_baseline(args)
        else:
            out['cpu_baseline'] = None
    finish(out if rank == 0 else None)


_PREFILL = {}


def prefill(ms):
    """Queue ~ms of device copies on the current stream (a 256 MiB copy takes ~0.1 ms)."""
    dev = torch.cuda.current_device()
    if dev not in _PREFILL:
        _PREFILL[dev] = (torch.empty(64 << 20, dtype=torch.float32, device='cuda'), torch.empty(64 << 20, dtype=torch.float32, device='cuda'))
    a, b = _PREFILL[dev]
    for _ in range(max(1, int(ms / 0.12))):
        b.copy_(a)


def time_seq_fn(fn, n, sync, prefill_ms=4.0):
    """ms per call of fn: HIP events around a loop of n calls on the launch stream, after 10 untimed calls.  Before the first
    event the stream is PRE-FILLED with ~prefill_ms of device copies, so that the host has the whole loop queued by the time the
    device reaches the first event: what is measured is kernel time back to back, not the host's launch path (round 3's
    10-iteration loops around two or three short launches carried ~40 us of launch gaps per call)."""
    for _ in range(10):
        fn()
    sync()
    was_on = gc.isenabled()      # (the probes under tools/ call this outside main(): a full collection inside a 20-call loop
    gc.disable()                 # reads as 2 ms per call - round 4 chased that through four GPU calls)
    try:
        prefill(prefill_ms)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
    finally:
        if was_on:
            gc.enable()
    return e0.elapsed_time(e1) / n


def other_configs(pw, dev, sync):
    """The other BASELINE configs and the paths around the hot path, timed once on rank 0 at N=1 as context (events
    around loops of launches, after 10 untimed calls).  Not the metric."""
    other = {}

    def frac(bytes_, ms):
        return round(bytes_ / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)

    def names(fn):
        c0 = pw.launch_count()
        fn()
        return pw.kernels_since(c0)
    with torch.no_grad():
        xd = torch.randn(64, 3, 512, 512, device=dev)
        dx, di = pw.DTCWTForward(J=3).to(dev), pw.DTCWTInverse().to(dev)
        dyl, dyh = dx(xd)
        tf, ti = time_seq_fn(lambda: dx(xd), 30, sync), time_seq_fn(lambda: di((dyl, dyh)), 30, sync)
        other['dtcwt_j3_near_sym_a_qshift_a_64x3x512x512_fp32'] = {
            'fwd_ms': round(tf, 4), 'inv_ms': round(ti, 4), 'fwd_inv_mpix_s': round(xd.numel() / (tf + ti) / 1e3, 1),
            'fwd_frac_of_hbm_peak_at_20B_per_px': frac(20 * xd.numel(), tf),
            'inv_frac_of_hbm_peak_at_20B_per_px': frac(20 * xd.numel(), ti),
            'fwd_kernels': names(lambda: dx(xd)), 'inv_kernels': names(lambda: di((dyl, dyh)))}
        d1x = pw.DTCWTForward(J=1).to(dev)
        t1f = time_seq_fn(lambda: d1x(xd), 30, sync)
        other['dtcwt_j1_near_sym_a_64x3x512x512_fp32'] = {'fwd_ms': round(t1f, 4), 'fwd_frac_of_hbm_peak_at_20B_per_px': frac(20 * xd.numel(), t1f),
                                                         'fwd_kernels': names(lambda: d1x(xd))}
        slw = pw.ScatLayer().to(dev)
        tsw = time_seq_fn(lambda: slw(xd), 30, sync)
        other['scatlayer_64x3x512x512_fp32'] = {'fwd_ms': round(tsw, 4), 'frac_of_hbm_peak_at_11B_per_px': frac(11 * xd.numel(), tsw),
                                               'fwd_kernels': names(lambda: slw(xd))}
        # round 6 (late): the 13 / 19-tap level-1 pair (near_sym_b; 14-tap q-shifts below) on the streaming level-1 kernels, and the
        # band-pass variant of the ScatLayer (near_sym_b_bp: 13 / 19 / 19 taps) on the lean kernel
        bx, bi = pw.DTCWTForward(J=3, biort='near_sym_b', qshift='qshift_b').to(dev), pw.DTCWTInverse(biort='near_sym_b', qshift='qshift_b').to(dev)
        byl, byh = bx(xd)
        tf, ti = time_seq_fn(lambda: bx(xd), 30, sync), time_seq_fn(lambda: bi((byl, byh)), 30, sync)
        other['dtcwt_j3_near_sym_b_qshift_b_64x3x512x512_fp32'] = {
            'fwd_ms': round(tf, 4), 'inv_ms': round(ti, 4), 'fwd_frac_of_hbm_peak_at_20B_per_px': frac(20 * xd.numel(), tf),
            'inv_frac_of_hbm_peak_at_20B_per_px': frac(20 * xd.numel(), ti),
            'fwd_kernels': names(lambda: bx(xd)), 'inv_kernels': names(lambda: bi((byl, byh)))}
        for tag, biort in (('near_sym_b', 'near_sym_b'), ('near_sym_b_bp', 'near_sym_b_bp')):
            slb = pw.ScatLayer(biort=biort).to(dev)
            tsb = time_seq_fn(lambda: slb(xd), 30, sync)
            other['scatlayer_%s_64x3x512x512_fp32' % tag] = {'fwd_ms': round(tsb, 4), 'frac_of_hbm_peak_at_11B_per_px': frac(11 * xd.numel(), tsb),
                                                            'fwd_kernels': names(lambda: slb(xd))}
        del xd, dyl, dyh, byl, byh
    # ---- training steps (forward + backward to the input): rows f1 of SURVEY 8(f).  Algorithmic bytes: the forward's, and for
    # the backward the gradients of every output read once + the input gradient written once (= the forward's number again);
    # ScatLayer also writes (forward) and reads (backward) the saved (re, im) / r: 6 planes of P/4 each, twice
    def train_step(mod, x, outs_of):
        xg = x.detach().requires_grad_(True)
        outs = outs_of(mod(xg))
        gos = [torch.randn_like(o) for o in outs]

        def step():
            xg2 = x.detach().requires_grad_(True)
            o = outs_of(mod(xg2))
            return torch.autograd.grad(o, xg2, gos)
        return step
    xt = torch.randn(128, 3, 512, 512, device=dev)
    m = pw.DWTForward(J=3, wave='db4', mode='symmetric').to(dev)
    st = train_step(m, xt, lambda r: [r[0]] + list(r[1]))
    t = time_seq_fn(st, 30, sync)
    b = 2 * algorithmic_bytes_fwd(128, 3, 512, 512, 3, 8, 4)
    other['train_dwt_j3_db4_128x3x512x512_fp32'] = {'fwd_bwd_ms': round(t, 4), 'frac_of_hbm_peak': frac(b, t), 'algorithmic_bytes': b,
                                                    'kernels': names(st)}
    del xt
    xt = torch.randn(64, 3, 512, 512, device=dev)
    m = pw.DTCWTForward(J=3).to(dev)
    st = train_step(m, xt, lambda r: [r[0]] + list(r[1]))
    t = time_seq_fn(st, 30, sync)
    b = 2 * 20 * xt.numel()
    other['train_dtcwt_j3_64x3x512x512_fp32'] = {'fwd_bwd_ms': round(t, 4), 'frac_of_hbm_peak': frac(b, t), 'algorithmic_bytes': b,
                                                 'kernels': names(st)}
    del xt
    xt = torch.randn(256, 3, 256, 256, device=dev)
    m = pw.ScatLayer().to(dev)
    st = train_step(m, xt, lambda r: [r])
    t = time_seq_fn(st, 30, sync)
    b = 46 * xt.numel()          # forward 4 (1 + 7/4 + 3) P, backward the same
    other['train_scatlayer_256x3x256x256_fp32'] = {'fwd_bwd_ms': round(t, 4), 'frac_of_hbm_peak_at_46B_per_px': frac(b, t),
                                                   'algorithmic_bytes': b, 'kernels': names(st)}
    for tag in ('near_sym_b', 'near_sym_b_bp'):    # round 6 (late): the 13 / 19-tap pair, and the band-pass layer on pairs of plain launches
        m = pw.ScatLayer(biort=tag).to(dev)
        st = train_step(m, xt, lambda r: [r])
        t = time_seq_fn(st, 20, sync)
        other['train_scatlayer_%s_256x3x256x256_fp32' % tag] = {'fwd_bwd_ms': round(t, 4), 'frac_of_hbm_peak_at_46B_per_px': frac(b, t),
                                                                'algorithmic_bytes': b, 'kernels': names(st)}
    del xt
    with torch.no_grad():
        xs = torch.randn(256, 3, 256, 256, device=dev)
        sl = pw.ScatLayer().to(dev)
        ts = time_seq_fn(lambda: sl(xs), 30, sync)
        other['scatlayer_256x3x256x256_fp32_one_gpu'] = {
            'fwd_ms': round(ts, 4), 'mpix_s': round(xs.numel() / ts / 1e3, 1),
            'frac_of_hbm_peak_at_11B_per_px': frac(11 * xs.numel(), ts), 'fwd_kernels': names(lambda: sl(xs))}
        # f2: ScatLayerj2 (three launches writing into its 49-entry output; 16.25 B per pixel = read x, write Z) and the
        # rotationally symmetric variant
        xs2 = xs[:64]
        s2 = pw.ScatLayerj2().to(dev)
        t2 = time_seq_fn(lambda: s2(xs2), 20, sync)
        sr = pw.ScatLayer(biort='near_sym_b_bp').to(dev)
        tr = time_seq_fn(lambda: sr(xs2), 20, sync)
        other['scatlayerj2_64x3x256x256_fp32'] = {'fwd_ms': round(t2, 4), 'mpix_s': round(xs2.numel() / t2 / 1e3, 1),
                                                  'frac_of_hbm_peak_at_16_25B_per_px': frac(16.25 * xs2.numel(), t2),
                                                  'fwd_kernels': names(lambda: s2(xs2))}
        other['scatlayer_rot_near_sym_b_bp_64x3x256x256_fp32'] = {
            'fwd_ms': round(tr, 4), 'mpix_s': round(xs2.numel() / tr / 1e3, 1),
            'frac_of_hbm_peak_at_11B_per_px': frac(11 * xs2.numel(), tr), 'fwd_kernels': names(lambda: sr(xs2))}
        s2r = pw.ScatLayerj2(biort='near_sym_b_bp', qshift='qshift_b_bp').to(dev)
        t2r = time_seq_fn(lambda: s2r(xs2), 20, sync)
        other['scatlayerj2_rot_near_sym_b_bp_64x3x256x256_fp32'] = {'fwd_ms': round(t2r, 4), 'mpix_s': round(xs2.numel() / t2r / 1e3, 1),
                                                                     'frac_of_hbm_peak_at_16_25B_per_px': frac(16.25 * xs2.numel(), t2r),
                                                                     'fwd_kernels': names(lambda: s2r(xs2))}
        del xs, xs2
        # f3: 1-D DWT and the stationary transform (generic single-axis kernels)
        x1 = torch.randn(64, 16, 65536, device=dev)
        d1 = pw.DWT1DForward(J=3, wave='db4', mode='symmetric').to(dev)
        t1 = time_seq_fn(lambda: d1(x1), 20, sync)
        i1 = pw.DWT1DInverse(wave='db4', mode='symmetric').to(dev)
        c1 = d1(x1)
        t1i = time_seq_fn(lambda: i1(c1), 20, sync)
        other['dwt1d_j3_db4_64x16x65536_fp32'] = {'fwd_ms': round(t1, 4), 'inv_ms': round(t1i, 4), 'msamples_s': round(x1.numel() / t1 / 1e3, 1),
                                                  'frac_of_hbm_peak_at_8B_per_sample': frac(8 * x1.numel(), t1),
                                                  'inv_frac_of_hbm_peak_at_8B_per_sample': frac(8 * x1.numel(), t1i),
                                                  'fwd_kernels': names(lambda: d1(x1)), 'inv_kernels': names(lambda: i1(c1))}
        del c1
        del x1
        from pytorch_wavelets_amd.dwt.transform2d import SWTForward
        xw = torch.randn(16, 3, 512, 512, device=dev)
        sw = SWTForward(J=2, wave='db2', mode='periodic').to(dev)
        tw = time_seq_fn(lambda: sw(xw), 20, sync)
        other['swt_j2_db2_periodic_16x3x512x512_fp32'] = {'fwd_ms': round(tw, 4), 'mpix_s': round(xw.numel() / tw / 1e3, 1),
                                                          'frac_of_hbm_peak_at_20B_per_px_and_level': frac(2 * 20 * xw.numel(), tw),
                                                          'fwd_kernels': names(lambda: sw(xw))}
        del xw
        # CNN-feature-map shapes (many small planes): the several-planes-per-workgroup kernels of round 4 (csrc/wl_dwt_small.h)
        xm = torch.randn(512, 16, 32, 32, device=dev)
        fm, im = pw.DWTForward(J=2, wave='db2', mode='symmetric').to(dev), pw.DWTInverse(wave='db2', mode='symmetric').to(dev)
        cm = fm(xm)
        tfm, tim = time_seq_fn(lambda: fm(xm), 30, sync), time_seq_fn(lambda: im(cm), 30, sync)
        bm = algorithmic_bytes_fwd(512, 16, 32, 32, 2, 4, 4)
        other['dwt_j2_db2_512x16x32x32_fp32'] = {'fwd_ms': round(tfm, 4), 'inv_ms': round(tim, 4), 'fwd_frac': frac(bm, tfm), 'inv_frac': frac(bm, tim),
                                                 'fwd_kernels': names(lambda: fm(xm)), 'inv_kernels': names(lambda: im(cm))}
        del xm, cm
        # wavelet pooling on ImageNet-style feature maps: several narrow planes per workgroup of the streaming kernels
        xm = torch.randn(64, 64, 112, 112, device=dev)
        fm, im = pw.DWTForward(J=1, wave='haar', mode='zero').to(dev), pw.DWTInverse(wave='haar', mode='zero').to(dev)
        cm = fm(xm)
        tfm, tim = time_seq_fn(lambda: fm(xm), 30, sync), time_seq_fn(lambda: im(cm), 30, sync)
        bm = algorithmic_bytes_fwd(64, 64, 112, 112, 1, 2, 4)
        other['dwt_j1_haar_64x64x112x112_fp32'] = {'fwd_ms': round(tfm, 4), 'inv_ms': round(tim, 4), 'fwd_frac': frac(bm, tfm), 'inv_frac': frac(bm, tim),
                                                   'fwd_kernels': names(lambda: fm(xm)), 'inv_kernels': names(lambda: im(cm))}
        del xm, cm
        xm = torch.randn(1024, 3, 128, 128, device=dev)
        slm = pw.ScatLayer().to(dev)
        tsm = time_seq_fn(lambda: slm(xm), 30, sync)
        other['scatlayer_1024x3x128x128_fp32'] = {'fwd_ms': round(tsm, 4), 'frac_of_hbm_peak_at_11B_per_px': frac(11 * xm.numel(), tsm),
                                                  'fwd_kernels': names(lambda: slm(xm))}
        del xm
        # outside the fused streaming envelope of round 2: wider images, longer filters; round 6: periodization at the metric's shape
        # (all levels in one launch of the fused analysis / synthesis kernels)
        for tag, shape, wave, L, mode in (('dwt_j3_db4_16x3x1024x1024_fp32', (16, 3, 1024, 1024), 'db4', 8, 'symmetric'),
                                          ('dwt_j3_db4_64x3x1024x1024_fp32', (64, 3, 1024, 1024), 'db4', 8, 'symmetric'),
                                          ('dwt_j3_db8_128x3x512x512_fp32', (128, 3, 512, 512), 'db8', 16, 'symmetric'),
                                          ('dwt_j3_db4_periodization_128x3x512x512_fp32', (128, 3, 512, 512), 'db4', 8, 'periodization'),
                                          ('dwt_j3_db9_128x3x512x512_fp32', (128, 3, 512, 512), 'db9', 18, 'symmetric')):
            xl = torch.randn(*shape, device=dev)
            fx, fi = pw.DWTForward(J=3, wave=wave, mode=mode).to(dev), pw.DWTInverse(wave=wave, mode=mode).to(dev)
            c = fx(xl)
            tf = time_seq_fn(lambda: fx(xl), 30, sync)
            ti = time_seq_fn(lambda: fi(c), 30, sync)
            b = algorithmic_bytes_fwd(shape[0], shape[1], shape[2], shape[3], 3, L, 4, periodization=mode == 'periodization')
            other[tag] = {'fwd_ms': round(tf, 4), 'inv_ms': round(ti, 4), 'fwd_frac': frac(b, tf), 'inv_frac': frac(b, ti),
                          'fwd_kernels': names(lambda: fx(xl)), 'inv_kernels': names(lambda: fi(c))}
            del xl, c
        xh = torch.randn(32, 16, 2048, 2048, device=dev, dtype=torch.float16)   # configs[4] at its full size (4.3 GB)
        hx = pw.DWTForward(J=4, wave='db8', mode='periodization').to(dev).half()
        hi = pw.DWTInverse(wave='db8', mode='periodization').to(dev).half()
        hyl, hyh = hx(xh)
        th = time_seq_fn(lambda: hx(xh), 5, sync)
        tih = time_seq_fn(lambda: hi((hyl, hyh)), 5, sync)
        other['dwt_j4_db8_periodization_32x16x2048x2048_fp16'] = {
            'fwd_ms': round(th, 4), 'inv_ms': round(tih, 4), 'fwd_mpix_s': round(xh.numel() / th / 1e3, 1),
            'fwd_frac_of_hbm_peak_at_4B_per_px': frac(4 * xh.numel(), th),
            'inv_frac_of_hbm_peak_at_4B_per_px': frac(4 * xh.numel(), tih),
            'fwd_kernels': names(lambda: hx(xh)), 'inv_kernels': names(lambda: hi((hyl, hyh)))}
        del xh, hyl, hyh
    return other


if __name__ == '__main__':
    main()
