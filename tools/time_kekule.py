"""Times one launch of the Kekulé assignment (mdx_mol_kekulize with the default tables) on the batch tools/time_rings.py and
tools/time_groups.py use -- synthetic drug-sized molecules, fused 5- and 6-rings with chains, about 30 atoms each -- with device events
after a warm-up, checks the batch against ``kekulize_ref`` on this host and prints one JSON line.  One measurement, no threshold: the
number goes into profiles/kekule_timing.txt and DESIGN.md.

    python tools/time_kekule.py [--n 256] [--atoms 30] [--reps 50] [--out FILE]
"""
import sys
import time

import numpy as np

import evalbench as EB
from moldiff_amd import kekule as K
from moldiff_amd import molpack


def main(argv=None):
    ap = EB.parser(reps=50, atoms=30)
    ap.add_argument('--n', type=int, default=256)
    args = EB.parse(ap, argv)
    mols, p, cm, _ = EB.batch(args.n, args.atoms, args.device)
    N, E = cm.N_cap, int(p['n_bonds'].sum())
    tables = K.KekuleTables()
    ms, out = EB.timed(lambda: K.launch(cm, tables), args.reps)
    t0 = time.perf_counter()
    want = K.stack_ref(mols, tables)
    host_s = time.perf_counter() - t0
    got = molpack.to_host(out)
    same = all(np.array_equal(got[k], want[k]) for k in K.STAT_KEYS)
    same = same and all(np.array_equal(got[k][:N], want[k]) for k in K.ATOM_KEYS) and np.array_equal(got['kek_order'][:E], want['kek_order'])
    s = K.summary(want)
    row = {'molecules': len(mols), 'atoms': N, 'bonds': E, 'aromatic_bonds': int(want['n_arom_bonds'].astype(np.int64).sum()),
           'components': int(want['n_components'].astype(np.int64).sum()), 'steps': int(want['steps'].astype(np.int64).sum()),
           'largest_steps': int(want['steps'].max()), 'fraction_kekulizable': s['fraction_kekulizable'],
           'device_ms_per_batch': round(ms, 4), 'includes': 'the zero-fill of the output tensors',
           'host_ref_s': round(host_s, 3), 'device_equals_host': bool(same)}
    EB.report([row], args.out, 'tools/time_kekule.py: one measurement, not gated')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
