"""Times one launch of the hydrogen placement (mdx_mol_hydrogens with the default tables) next to one launch of the Kekulé assignment
(mdx_mol_kekulize) on the same batch in the same run: 256 and 2,048 synthetic drug-sized molecules (the batch of tools/time_kekule.py
with Gaussian coordinates), device events after a warm-up.  Checks the smaller batch against ``addh_ref`` on this host, prints one JSON
line per size and writes them to profiles/hydrogens_timing.txt.  One measurement, no threshold; nothing is gated on it.

    python tools/time_hydrogens.py [--sizes 256 2048] [--atoms 30] [--reps 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moldiff_amd import hydrogens as H  # noqa: E402
from moldiff_amd import kekule as K  # noqa: E402
from moldiff_amd import molpack  # noqa: E402
from time_groups import ELEMENTS, drug_like  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        out = fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 2048])
    ap.add_argument('--atoms', type=int, default=30)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hydrogens_timing.txt'))
    args = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(args.device))
    lines, ok = [], True
    for n in args.sizes:
        g = np.random.default_rng(0)
        mols = [drug_like(g, max(12, int(g.normal(args.atoms, 5)))) for _ in range(n)]
        for m in mols:
            m['atom_pos'] = g.normal(0.0, 2.5, size=(len(m['element']), 3)).astype(np.float32)
        p = molpack.pack_mols(mols, ELEMENTS, positions=True)
        cm = molpack.CompactMols.from_packed(molpack.to_device(p, args.device))
        kt, ht = K.KekuleTables(), H.HydrogenTables()
        kek_ms, kek = timed(lambda: K.launch(cm, kt), args.reps)
        h_ms, out = timed(lambda: H.launch(cm, kek['kek_h'], kek['kek_order'], ht), args.reps)
        got = molpack.to_host(out)
        row = {'molecules': n, 'atoms': cm.N_cap, 'hydrogens_placed': int(got['n_h_placed'].astype(np.int64).sum()),
               'hydrogens_wanted': int(got['n_h_wanted'].astype(np.int64).sum()), 'kekulize_ms_per_batch': round(kek_ms, 4),
               'hydrogens_ms_per_batch': round(h_ms, 4), 'includes': 'the zero-fill of the output tensors', 'device': torch.cuda.get_device_name(0)}
        if n == min(args.sizes):   # the restatement is slow: the smaller batch only
            want = H.stack_ref(mols)
            same = all(np.array_equal(got[k], want[k]) for k in H.STAT_KEYS) and all(np.array_equal(got[k][:cm.N_cap], want[k]) for k in H.ATOM_KEYS)
            diff = float(np.abs(got['h_pos'][:cm.N_cap] - want['h_pos']).max(initial=0.0))
            row.update(integers_equal_host=bool(same), h_pos_max_abs_diff=diff)
            ok = ok and same and diff <= 1e-8
        lines.append(json.dumps(row))
        print(lines[-1])
    with open(args.out, 'w') as f:
        f.write('tools/time_hydrogens.py: one launch of mdx_mol_hydrogens beside one launch of mdx_mol_kekulize on the same batch, same run\n')
        f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
