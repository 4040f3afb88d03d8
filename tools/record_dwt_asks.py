"""Record what the 2-D DWT's Python dispatcher asks the engine for (the cases of tests/_ask_cases.py: a recording stub for the
engine, a patched chip size, tensors nobody reads) and write it to tests/golden/dwt_asks.json - the fixture
tests/test_dwt_asks.py replays.  Run it on the commit whose policy is to be kept, BEFORE the dispatcher is changed:

    python tools/record_dwt_asks.py [--out FILE] [--package DIR]

--package: the directory that holds the `pytorch_wavelets_amd` to record (a checkout of that commit), while the cases and this
tool are the ones of this tree.  Prints, per launcher, in how many cases it is asked / passed over - as the first choice (an
engine that takes everything) and anywhere in the ladder - and how often the fused launchers get the lattice scratch."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--package', default=ROOT)
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.package), os.path.join(ROOT, 'tests')]
    import _ask_cases as AC
    import pytorch_wavelets_amd as pw
    assert os.path.dirname(os.path.dirname(os.path.abspath(pw.__file__))) == os.path.abspath(args.package), pw.__file__

    entries = [AC.run_case(case) for case in AC.CASES]
    out = args.out or AC.GOLDEN
    with open(out, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(e, separators=(',', ':')) for e in entries) + '\n]\n')

    ladders = [[e[s] for s in AC.STEPS if s in e] for e in entries]          # per case: the ladders of its steps
    print('%d cases, %d steps, %d ask sequences, %d bytes' % (len(entries), sum(len(c) for c in ladders),
                                                              sum(len(l) for c in ladders for l in c), os.path.getsize(out)))
    print('%-32s %-22s %s' % ('launcher', 'first choice: yes / no', 'in the ladder: yes / no'))
    for name in AC.WRAPPERS:
        first = sum(any(a[0] == name for l in c for a in l[0]) for c in ladders)
        anywhere = sum(any(a[0] == name for l in c for seq in l for a in seq) for c in ladders)
        print('%-32s %4d / %-15d %4d / %d' % (name, first, len(entries) - first, anywhere, len(entries) - anywhere))
        assert 0 < first < len(entries) and 0 < anywhere < len(entries), name + ': not on both sides'
    # the lattice: hint bits 2 and 3 of `strips` (the argument before the scratch) and the scratch itself (null = no lattice)
    for name in ('wl_dwt2d_analysis_fused_ex', 'wl_dwt2d_synthesis_fused_ex'):
        asks = {json.dumps(a) for c in ladders for l in c for seq in l for a in seq if a[0] == name}
        hinted = [json.loads(a) for a in asks]
        # (the trailing arguments of the *_ex launchers: ..., strips, scratch, state, stream -> recorded ..., strips[, null], null)
        with_scratch = sum(a[-2] is not None for a in hinted)
        bits = sum((a[-2] if a[-2] is not None else a[-3]) & 12 == 12 for a in hinted)
        print('%-32s %d distinct asks: hint bits set %d / clear %d, lattice scratch handed %d / null %d'
              % (name, len(hinted), bits, len(hinted) - bits, with_scratch, len(hinted) - with_scratch))
        assert 0 < bits < len(hinted) and 0 < with_scratch < len(hinted), name + ': lattice not on both sides'


if __name__ == '__main__':
    main()
