"""Times mdx_mol_bestrms next to mdx_mol_canon on the same batch: the 256 molecules of tools/time_stereo.py (synthetic drug-sized graphs
with a para-substituted ring, a CF3 and a tert-butyl group, so that every probe has many atom maps) with random coordinates, each
against one and against eight noisy copies of itself, with device events after a warm-up; checks the one-target run against
``rmsd.stack_ref`` on this host and prints one JSON line.  One measurement, no threshold: the numbers go into INTEGRATION.md's section
"Best RMSD between conformers".

    python tools/time_bestrms.py [--size 256] [--atoms 30] [--reps 20] [--out FILE]
"""
import re
import sys

import numpy as np
import torch

import evalbench as EB
from evalbench import ELEMENTS
from moldiff_amd import canon as C
from moldiff_amd import molpack
from moldiff_amd import rmsd as R

COPIES = 8


def main(argv=None):
    ap = EB.parser(reps=20, atoms=30)
    ap.add_argument('--size', type=int, default=256)
    args = EB.parse(ap, argv)
    mols, p, cm, g = EB.batch(args.size, args.atoms, args.device, gen=EB.extended, pos_sigma=2.0)
    copies = [dict(m, atom_pos=(m['atom_pos'] + g.normal(size=m['atom_pos'].shape) * 0.2).astype(np.float32)) for m in mols for _ in range(COPIES)]
    canon_out = C.launch(cm)
    targets = C.canon_mols(copies, args.device, atomic_numbers=ELEMENTS)
    canon_ms = EB.timed(lambda: C.launch(cm), args.reps)[0]
    rows = []
    for k in (1, COPIES):
        pairs = [(m, COPIES * m + j) for m in range(args.size) for j in range(k)]
        ptr, tgt, _ = R._csr(pairs, args.size, len(copies))
        ptr, tgt = torch.from_numpy(ptr).to(args.device), torch.from_numpy(tgt).to(args.device)
        ms = EB.timed(lambda: R.launch(cm, canon_out, targets, ptr, tgt), args.reps)[0]
        rows.append({'targets_per_probe': k, 'pairs': len(pairs), 'bestrms_ms': round(ms, 4), 'ratio_to_canon': round(ms / canon_ms, 3)})
        if k == 1:
            got = molpack.to_host(R.launch(cm, canon_out, targets, ptr, tgt))
            want = R.stack_ref(mols, copies, pairs, atomic_numbers=ELEMENTS, canon_probes=molpack.dense(dict(canon_out), cm, p, C.LAYOUT),
                               canon_targets=targets, check=False)
    with open(EB.profile_path('bestrms_accuracy.txt')) as f:
        tol = 16.0 * float(re.search(r'max_abs_difference_in_unit (\S+)', f.read()).group(1))
    worst = max(float((np.abs(got[key] - want[key]) / want['unit']).max()) for key in R.FLOAT_KEYS)
    same = all(np.array_equal(got[key], want[key]) for key in ('status', 'n_nodes', 'n_aut', 'n_maps', 'pair_status')) and worst <= tol
    row = {'molecules': args.size, 'atoms': int(p['n_atoms'].sum()), 'bonds': int(p['n_bonds'].sum()), 'canon_ms': round(canon_ms, 4),
           'runs': rows, 'optimal_leaves': int(want['n_aut'].astype(np.int64).sum()), 'largest_difference_in_unit': worst,
           'tolerance': tol, 'includes': 'the zero-fill of the output tensors of each call', 'device_within_tolerance_of_host': bool(same)}
    EB.report([row], args.out, 'tools/time_bestrms.py: one measurement, not gated')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
