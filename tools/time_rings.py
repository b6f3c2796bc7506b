"""Times mdx_mol_rings on a batch of synthetic drug-sized molecules (fused 5- and 6-rings with chains, about 30 atoms each) with device
events after a warm-up, checks the batch against ``rings_ref`` on this host and prints one JSON line.  One measurement, no threshold:
the numbers go into INTEGRATION.md's section "Ring and composition statistics".

    python tools/time_rings.py [--n 256] [--atoms 30] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    call = lambda: R.launch(cm, len(ELEMENTS), 4)
    for _ in range(5):
        out = call()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.reps):
        out = call()
    stop.record()
    torch.cuda.synchronize()
    device_ms = start.elapsed_time(stop) / args.reps
    t0 = time.perf_counter()
    want = R.stack_ref(mols)
    host_s = time.perf_counter() - t0
    got = molpack.to_host(out)
    same = all(np.array_equal(got[k], want[k]) for k in got)
    print(json.dumps({'molecules': len(mols), 'atoms': N, 'bonds': int(p['n_bonds'].sum()), 'rings': int(want['n_rings'].sum()),
                      'device_ms_per_batch': round(device_ms, 4), 'includes': 'the zero-fill of the ten output tensors', 'host_ref_s': round(host_s, 3),
                      'device_equals_host': bool(same), 'summary': R.summary(dict(want))}))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
