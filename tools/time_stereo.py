"""Times mdx_mol_stereo next to mdx_mol_canon on the same batches: the molecules of tools/time_canon.py (synthetic drug-sized graphs
with a para-substituted ring, a CF3 and a tert-butyl group, so that the search tree is not trivial) with random coordinates, at 256 and
2,048 molecules, with device events after a warm-up; checks the 256 batch against ``stereo_ref`` on this host and prints one JSON line.
One measurement, no threshold: the numbers go into INTEGRATION.md's section "Stereo perception".

    python tools/time_stereo.py [--sizes 256 2048] [--atoms 30] [--reps 50] [--out FILE]
"""
import sys

import numpy as np

import evalbench as EB
from evalbench import ELEMENTS
from moldiff_amd import canon as C
from moldiff_amd import molpack
from moldiff_amd import stereo as S


def main(argv=None):
    ap = EB.parser(reps=50, atoms=30)
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 2048])
    args = EB.parse(ap, argv)
    rows, same = [], True
    for size in args.sizes:
        mols, p, cm, _ = EB.batch(size, args.atoms, args.device, gen=EB.extended, pos_sigma=2.0)
        canon_out = C.launch(cm)
        canon_ms = EB.timed(lambda: C.launch(cm), args.reps)[0]
        stereo_ms = EB.timed(lambda: S.launch(cm, canon_out, atomic_numbers=ELEMENTS), args.reps)[0]
        row = {'molecules': size, 'atoms': int(p['n_atoms'].sum()), 'bonds': int(p['n_bonds'].sum()), 'canon_ms': round(canon_ms, 4),
               'stereo_ms': round(stereo_ms, 4), 'ratio': round(stereo_ms / canon_ms, 3)}
        if size == min(args.sizes):                                    # the smaller batch against the restatement
            got = molpack.to_host(molpack.dense(S.launch(cm, canon_out, atomic_numbers=ELEMENTS), cm, p, S.LAYOUT))
            keep = [m for m, x in enumerate(mols) if not S.near_threshold(x, atomic_numbers=ELEMENTS)]
            want = S.stack_ref(mols, atomic_numbers=ELEMENTS)
            for m in keep:
                a, b = S.mol_result(got, m), S.mol_result(want, m)
                same = same and all(np.array_equal(a[k], b[k]) for k in b)
            row.update(compared=len(keep), chiral=int(want['chiral'].sum()), centres=int(want['n_centres'].sum()),
                       stereo_bonds=int(want['n_stereo_bonds'].sum()), optimal_leaves=int(want['n_aut'].astype(np.int64).sum()))
        rows.append(row)
    EB.report([{'batches': rows, 'includes': 'the zero-fill of the output tensors of each call', 'device_equals_host': bool(same)}], args.out,
              'tools/time_stereo.py: one measurement, not gated')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
