"""Times one launch of the Kekulé assignment (mdx_mol_kekulize with the default tables) on the batch tools/time_rings.py and
tools/time_groups.py use -- synthetic drug-sized molecules, fused 5- and 6-rings with chains, about 30 atoms each -- with device events
after a warm-up, checks the batch against ``kekulize_ref`` on this host and prints one JSON line.  One measurement, no threshold: the
number goes into profiles/kekule_timing.txt and DESIGN.md.

    python tools/time_kekule.py [--n 256] [--atoms 30] [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moldiff_amd import kekule as K  # noqa: E402
from moldiff_amd import molpack  # noqa: E402
from time_groups import ELEMENTS, drug_like  # noqa: E402


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
    N, E = cm.N_cap, int(p['n_bonds'].sum())
    tables = K.KekuleTables()
    for _ in range(5):
        out = K.launch(cm, tables)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(args.reps):
        out = K.launch(cm, tables)
    stop.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop) / args.reps
    t0 = time.perf_counter()
    want = K.stack_ref(mols, tables)
    host_s = time.perf_counter() - t0
    got = molpack.to_host(out)
    same = all(np.array_equal(got[k], want[k]) for k in K.STAT_KEYS)
    same = same and all(np.array_equal(got[k][:N], want[k]) for k in K.ATOM_KEYS) and np.array_equal(got['kek_order'][:E], want['kek_order'])
    s = K.summary(want)
    print(json.dumps({'molecules': len(mols), 'atoms': N, 'bonds': E, 'aromatic_bonds': int(want['n_arom_bonds'].astype(np.int64).sum()),
                      'components': int(want['n_components'].astype(np.int64).sum()), 'steps': int(want['steps'].astype(np.int64).sum()),
                      'largest_steps': int(want['steps'].max()), 'fraction_kekulizable': s['fraction_kekulizable'],
                      'device_ms_per_batch': round(ms, 4), 'includes': 'the zero-fill of the output tensors',
                      'host_ref_s': round(host_s, 3), 'device_equals_host': bool(same)}))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
