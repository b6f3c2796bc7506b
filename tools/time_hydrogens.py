"""Times one launch of the hydrogen placement (mdx_mol_hydrogens with the default tables) next to one launch of the Kekulé assignment
(mdx_mol_kekulize) on the same batch in the same run: 256 and 2,048 synthetic drug-sized molecules (the batch of tools/time_kekule.py
with Gaussian coordinates), device events after a warm-up.  Checks the smaller batch against ``addh_ref`` on this host, prints one JSON
line per size and writes them to profiles/hydrogens_timing.txt.  One measurement, no threshold; nothing is gated on it.

    python tools/time_hydrogens.py [--sizes 256 2048] [--atoms 30] [--reps 50] [--out FILE]
"""
import sys

import numpy as np
import torch

import evalbench as EB
from moldiff_amd import hydrogens as H
from moldiff_amd import kekule as K
from moldiff_amd import molpack


def main(argv=None):
    ap = EB.parser(reps=50, atoms=30, out=EB.profile_path('hydrogens_timing.txt'))
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 2048])
    args = EB.parse(ap, argv)
    rows, ok = [], True
    for n in args.sizes:
        mols, p, cm, _ = EB.batch(n, args.atoms, args.device, pos_sigma=2.5)
        kt, ht = K.KekuleTables(), H.HydrogenTables()
        kek_ms, kek = EB.timed(lambda: K.launch(cm, kt), args.reps)
        h_ms, out = EB.timed(lambda: H.launch(cm, kek['kek_h'], kek['kek_order'], ht), args.reps)
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
        rows.append(row)
    EB.report(rows, args.out, 'tools/time_hydrogens.py: one launch of mdx_mol_hydrogens beside one launch of mdx_mol_kekulize on the same batch, same run')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
