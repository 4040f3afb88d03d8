"""Record which kernels the 2-D DWT takes on the host emulation (tests/emu_backend.py) for the cases of
tests/_route_cases.py, and write them to tests/golden/dwt_routes.json - the fixture tests/test_dwt_routes_emu.py replays.
Run it on the commit whose routes are to be kept, BEFORE the Python layer is changed:

    python tools/record_dwt_routes.py [--out FILE] [--tensors FILE]

--tensors also saves what every case computed (torch.save), for a one-off bit-for-bit comparison of two commits."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import _route_cases as RC  # noqa: E402


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
    steps = [e[s] for e in entries for s in ('forward', 'inverse', 'backward') if s in e]
    routes = [s for s in steps if isinstance(s, list)]
    # what the fixture has to contain to be worth replaying
    for fam in RC.FAMILIES:
        assert any(k.startswith(fam + '<') for r in routes for k in r), 'no route through ' + fam
    assert any(isinstance(s, dict) for s in steps), 'no recorded error'
    fams = [{k.split('<')[0] for k in e['inverse'] if k.startswith('WlSfb')} for e in entries if isinstance(e.get('inverse'), list)]
    assert any(len(f) > 1 for f in fams), 'no inverse that mixes two kernel families'
    with open(args.out, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(e, separators=(',', ':')) for e in entries) + '\n]\n')
    if args.tensors:
        torch.save(tensors, args.tensors)
    print('%d cases, %d distinct routes, %d errors, %d bytes' % (len(entries), len({tuple(r) for r in routes}),
                                                                 sum(isinstance(s, dict) for s in steps), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
