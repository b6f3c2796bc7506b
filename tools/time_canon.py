"""Times mdx_mol_canon on the batch of tools/time_rings.py (256 synthetic drug-sized molecules), every molecule extended by a
para-substituted benzene ring, a CF3 and a tert-butyl group so that the search tree is not trivial, with device events after a warm-up;
checks the batch against ``canon_ref`` on this host and prints one JSON line.  One measurement, no threshold: the numbers go into
INTEGRATION.md's section "Canonical form".

    python tools/time_canon.py [--n 256] [--atoms 30] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moldiff_amd import canon as C  # noqa: E402
from moldiff_amd import molpack  # noqa: E402
from time_rings import ELEMENTS, drug_like  # noqa: E402


def extended(g, atoms):
    """``drug_like`` + a para-substituted aromatic ring on a random atom carrying a CF3, and a tert-butyl on another"""
    m = drug_like(g, atoms)
    n = len(m['element'])
    nb = m['bond_index'].shape[1] // 2
    bonds = [(int(i), int(j), int(t)) for (i, j), t in zip(m['bond_index'][:, :nb].T, m['bond_type'][:nb])]
    ele = m['element'].tolist()
    a, b = (int(x) for x in g.choice(n, 2, replace=False))
    r = n                                                              # the ring r .. r + 5, attached at r, the CF3 at r + 3
    bonds += [(a, r, 1)] + [(r + k, r + (k + 1) % 6, 4) for k in range(6)] + [(r + 3, r + 6, 1)] + [(r + 6, r + 7 + k, 1) for k in range(3)]
    ele += [6] * 7 + [9] * 3
    t = r + 10                                                         # the tert-butyl: t and its three methyls
    bonds += [(b, t, 1)] + [(t, t + 1 + k, 1) for k in range(3)]
    ele += [6] * 4
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).T
    bt = np.asarray([t for _, _, t in bonds], dtype=np.int64)
    return {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--atoms', type=int, default=30)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(args.device))
    g = np.random.default_rng(0)
    mols = [extended(g, max(12, int(g.normal(args.atoms, 5)))) for _ in range(args.n)]
    p = molpack.pack_mols(mols, ELEMENTS)
    cm = molpack.CompactMols.from_packed(molpack.to_device(p, args.device))
    call = lambda: C.launch(cm)
    for _ in range(5):
        out = call()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.reps):
        out = call()
    stop.record()
    torch.cuda.synchronize()
    window_ms = start.elapsed_time(stop)
    t0 = time.perf_counter()
    want = C.stack_ref(mols)
    host_s = time.perf_counter() - t0
    got = molpack.to_host(out)
    N, E = int(p['n_atoms'].sum()), int(p['n_bonds'].sum())
    got.update({k: got[k][:N] for k in C.ATOM_KEYS}, canon_bond_type=got['canon_bond_type'][:E], canon_bond_index=got['canon_bond_index'][:, :E])
    same = all(np.array_equal(got[k], want[k]) for k in got)
    print(json.dumps({'molecules': len(mols), 'atoms': N, 'bonds': E, 'nodes': int(want['n_nodes'].sum()), 'leaves': int(want['n_leaves'].sum()),
                      'largest_tree': int(want['n_nodes'].max()), 'device_ms_per_batch': round(window_ms / args.reps, 4),
                      'window_ms': round(window_ms, 2), 'includes': 'the zero-fill of the seven output tensors', 'host_ref_s': round(host_s, 3),
                      'device_equals_host': bool(same), 'summary': C.summary(dict(want))}))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
