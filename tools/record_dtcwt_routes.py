"""Record which kernels the DTCWT and the scattering layers take on the host emulation (tests/emu_backend.py) for the cases of
tests/_dtroute_cases.py, and write them to tests/golden/dtcwt_routes.json - the fixture tests/test_dtcwt_routes_emu.py
replays.  Run it on the commit whose routes are to be kept, BEFORE the launchers are changed:

    python tools/record_dtcwt_routes.py [--out FILE] [--tensors FILE]

--tensors also saves what every case computed (torch.save), for a one-off bit-for-bit comparison of two commits."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import _dtroute_cases as RC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=RC.GOLDEN)
    ap.add_argument('--tensors')
    args = ap.parse_args()
    entries, tensors = [], []
    for case in RC.CASES:
        entry, ts = RC.run_case(case)
        entries.append(entry)
        tensors.append(ts)
    steps = [e[s] for e in entries for s in RC.STEPS if s in e]
    routes = [s for s in steps if isinstance(s, list)]
    kernels = {k for r in routes for k in r}
    # what the fixture has to contain to be worth replaying
    for fam in RC.FAMILIES:
        assert any(k.startswith(fam) for k in kernels), 'no route through ' + fam
    for mode in RC.FUSED_MODES:
        assert any(RC.fused_mode(k) == mode for k in kernels), 'no route through WlDtFwd12Strip MODE %d' % mode
    with open(args.out, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(e, separators=(',', ':')) for e in entries) + '\n]\n')
    if args.tensors:
        torch.save(tensors, args.tensors)
    print('%d cases, %d distinct routes, %d distinct kernels, %d errors, %d bytes'
          % (len(entries), len({tuple(r) for r in routes}), len(kernels), sum(isinstance(s, dict) for s in steps),
             os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
