"""Times one launch of the functional-group counts (mdx_mol_rings for the ring data, then mdx_mol_groups with the default pattern set)
on the batch tools/time_rings.py uses -- synthetic drug-sized molecules, fused 5- and 6-rings with chains, about 30 atoms each -- with
device events after a warm-up, checks the batch against ``groups_ref`` on this host and prints one JSON line.  One measurement, no
threshold: the numbers go into DESIGN.md and INTEGRATION.md's section "Functional-group counts".

    python tools/time_groups.py [--n 256] [--atoms 30] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moldiff_amd import groups as G  # noqa: E402
from moldiff_amd import molpack  # noqa: E402
from moldiff_amd import rings as R  # noqa: E402

ELEMENTS = (6, 7, 8, 9, 15, 16, 17)


def drug_like(g, atoms):
    """two to four rings of 5 or 6 atoms, each fused to the previous one along a bond, then chains grown from random atoms"""
    size = int(g.choice([5, 6]))
    bonds = [(k, (k + 1) % size) for k in range(size)]
    n, last = size, (0, 1)
    for _ in range(int(g.integers(1, 4))):
        size = int(g.choice([5, 6]))
        new = list(range(n, n + size - 2))
        path = [last[0]] + new + [last[1]]
        bonds += [(path[k], path[k + 1]) for k in range(len(path) - 1)]
        last, n = (new[0], new[1]), n + size - 2
    while n < atoms:
        bonds.append((int(g.integers(0, n)), n))
        n += 1
    ele = g.choice(ELEMENTS, n, p=[0.7, 0.1, 0.12, 0.02, 0.01, 0.03, 0.02])
    idx = np.asarray(bonds, dtype=np.int64).T
    bt = g.choice([1, 2, 4], len(bonds), p=[0.6, 0.1, 0.3])
    return {'element': ele.astype(np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--atoms', type=int, default=30)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(args.device))
    g = np.random.default_rng(0)
    mols = [drug_like(g, max(12, int(g.normal(args.atoms, 5)))) for _ in range(args.n)]
    p = molpack.pack_mols(mols, ELEMENTS)
    cm = molpack.CompactMols.from_packed(molpack.to_device(p, args.device))
    N = cm.N_cap
    pset = G.PatternSet.default()
    ring_data = R.launch(cm, len(ELEMENTS), 4)
    both = lambda: G.launch(cm, pset)                          # mdx_mol_rings, then mdx_mol_groups
    alone = lambda: G.launch(cm, pset, ring_data=ring_data)    # mdx_mol_groups on ring data already there

    def timed(call):
        for _ in range(5):
            out = call()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            out = call()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.reps, out
    both_ms, out = timed(both)
    alone_ms, out2 = timed(alone)
    t0 = time.perf_counter()
    want = G.stack_ref(mols, pset)
    host_s = time.perf_counter() - t0
    keys = ('status', 'n_embed', 'n_anchor', 'steps', 'pat_status')
    same = all(np.array_equal(molpack.to_host(o)[k], want[k]) for o in (out, out2) for k in keys)
    same = same and all(np.array_equal(molpack.to_host(o)['atom_hit'][:N], want['atom_hit']) for o in (out, out2))
    print(json.dumps({'molecules': len(mols), 'atoms': N, 'bonds': int(p['n_bonds'].sum()), 'patterns': len(pset),
                      'steps': int(want['steps'].astype(np.int64).sum()), 'embeddings': int(want['n_embed'].astype(np.int64).sum()),
                      'device_ms_per_batch_with_rings': round(both_ms, 4), 'device_ms_per_batch_groups_alone': round(alone_ms, 4),
                      'includes': 'the zero-fill of the output tensors, the table upload and the workspace allocation',
                      'host_ref_s': round(host_s, 3), 'device_equals_host': bool(same),
                      'mean_matches': {k: round(v['mean_matches'], 4) for k, v in G.summary(dict(want))['patterns'].items()}}))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
