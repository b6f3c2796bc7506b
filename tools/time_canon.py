"""Times mdx_mol_canon on the batch of tools/time_rings.py (256 synthetic drug-sized molecules), every molecule extended by a
para-substituted benzene ring, a CF3 and a tert-butyl group so that the search tree is not trivial, with device events after a warm-up;
checks the batch against ``canon_ref`` on this host and prints one JSON line.  One measurement, no threshold: the numbers go into
INTEGRATION.md's section "Canonical form".

    python tools/time_canon.py [--n 256] [--atoms 30] [--reps 50] [--out FILE]
"""
import sys
import time

import numpy as np

import evalbench as EB
from moldiff_amd import canon as C
from moldiff_amd import molpack


def main(argv=None):
    ap = EB.parser(reps=50, atoms=30)
    ap.add_argument('--n', type=int, default=256)
    args = EB.parse(ap, argv)
    mols, p, cm, _ = EB.batch(args.n, args.atoms, args.device, gen=EB.extended)
    ms, out = EB.timed(lambda: C.launch(cm), args.reps)
    t0 = time.perf_counter()
    want = C.stack_ref(mols)
    host_s = time.perf_counter() - t0
    got = molpack.to_host(out)
    N, E = int(p['n_atoms'].sum()), int(p['n_bonds'].sum())
    got.update({k: got[k][:N] for k in C.ATOM_KEYS}, canon_bond_type=got['canon_bond_type'][:E], canon_bond_index=got['canon_bond_index'][:, :E])
    same = all(np.array_equal(got[k], want[k]) for k in got)
    row = {'molecules': len(mols), 'atoms': N, 'bonds': E, 'nodes': int(want['n_nodes'].sum()), 'leaves': int(want['n_leaves'].sum()),
           'largest_tree': int(want['n_nodes'].max()), 'device_ms_per_batch': round(ms, 4),
           'window_ms': round(ms * args.reps, 2), 'includes': 'the zero-fill of the seven output tensors', 'host_ref_s': round(host_s, 3),
           'device_equals_host': bool(same), 'summary': C.summary(dict(want))}
    EB.report([row], args.out, 'tools/time_canon.py: one measurement, not gated')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
