"""Times one launch of the functional-group counts (mdx_mol_rings for the ring data, then mdx_mol_groups with the default pattern set)
on the batch tools/time_rings.py uses -- synthetic drug-sized molecules, fused 5- and 6-rings with chains, about 30 atoms each -- with
device events after a warm-up, checks the batch against ``groups_ref`` on this host and prints one JSON line.  One measurement, no
threshold: the numbers go into DESIGN.md and INTEGRATION.md's section "Functional-group counts".

    python tools/time_groups.py [--n 256] [--atoms 30] [--reps 50] [--out FILE]
"""
import sys
import time

import numpy as np

import evalbench as EB
from evalbench import ELEMENTS
from moldiff_amd import groups as G
from moldiff_amd import molpack
from moldiff_amd import rings as R


def main(argv=None):
    ap = EB.parser(reps=50, atoms=30)
    ap.add_argument('--n', type=int, default=256)
    args = EB.parse(ap, argv)
    mols, p, cm, _ = EB.batch(args.n, args.atoms, args.device)
    N = cm.N_cap
    pset = G.PatternSet.default()
    ring_data = R.launch(cm, len(ELEMENTS), 4)
    both_ms, out = EB.timed(lambda: G.launch(cm, pset), args.reps)                          # mdx_mol_rings, then mdx_mol_groups
    alone_ms, out2 = EB.timed(lambda: G.launch(cm, pset, ring_data=ring_data), args.reps)   # mdx_mol_groups on ring data already there
    t0 = time.perf_counter()
    want = G.stack_ref(mols, pset)
    host_s = time.perf_counter() - t0
    keys = ('status', 'n_embed', 'n_anchor', 'steps', 'pat_status')
    same = all(np.array_equal(molpack.to_host(o)[k], want[k]) for o in (out, out2) for k in keys)
    same = same and all(np.array_equal(molpack.to_host(o)['atom_hit'][:N], want['atom_hit']) for o in (out, out2))
    row = {'molecules': len(mols), 'atoms': N, 'bonds': int(p['n_bonds'].sum()), 'patterns': len(pset),
           'steps': int(want['steps'].astype(np.int64).sum()), 'embeddings': int(want['n_embed'].astype(np.int64).sum()),
           'device_ms_per_batch_with_rings': round(both_ms, 4), 'device_ms_per_batch_groups_alone': round(alone_ms, 4),
           'includes': 'the zero-fill of the output tensors, the table upload and the workspace allocation',
           'host_ref_s': round(host_s, 3), 'device_equals_host': bool(same),
           'mean_matches': {k: round(v['mean_matches'], 4) for k, v in G.summary(dict(want))['patterns'].items()}}
    EB.report([row], args.out, 'tools/time_groups.py: one measurement, not gated')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
