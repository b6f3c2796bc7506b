"""Times mdx_mol_rings on a batch of synthetic drug-sized molecules (fused 5- and 6-rings with chains, about 30 atoms each) with device
events after a warm-up, checks the batch against ``rings_ref`` on this host and prints one JSON line.  One measurement, no threshold:
the numbers go into INTEGRATION.md's section "Ring and composition statistics".

    python tools/time_rings.py [--n 256] [--atoms 30] [--reps 50] [--out FILE]
"""
import sys
import time

import numpy as np

import evalbench as EB
from evalbench import ELEMENTS
from moldiff_amd import molpack
from moldiff_amd import rings as R


def main(argv=None):
    ap = EB.parser(reps=50, atoms=30)
    ap.add_argument('--n', type=int, default=256)
    args = EB.parse(ap, argv)
    mols, p, cm, _ = EB.batch(args.n, args.atoms, args.device)
    N = cm.N_cap
    device_ms, out = EB.timed(lambda: R.launch(cm, len(ELEMENTS), 4), args.reps)
    t0 = time.perf_counter()
    want = R.stack_ref(mols)
    host_s = time.perf_counter() - t0
    got = molpack.to_host(out)
    same = all(np.array_equal(got[k], want[k]) for k in got)
    row = {'molecules': len(mols), 'atoms': N, 'bonds': int(p['n_bonds'].sum()), 'rings': int(want['n_rings'].sum()),
           'device_ms_per_batch': round(device_ms, 4), 'includes': 'the zero-fill of the ten output tensors', 'host_ref_s': round(host_s, 3),
           'device_equals_host': bool(same), 'summary': R.summary(dict(want))}
    EB.report([row], args.out, 'tools/time_rings.py: one measurement, not gated')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
