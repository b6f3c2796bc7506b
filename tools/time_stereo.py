"""Times mdx_mol_stereo next to mdx_mol_canon on the same batches: the molecules of tools/time_canon.py (synthetic drug-sized graphs
with a para-substituted ring, a CF3 and a tert-butyl group, so that the search tree is not trivial) with random coordinates, at 256 and
2,048 molecules, with device events after a warm-up; checks the 256 batch against ``stereo_ref`` on this host and prints one JSON line.
One measurement, no threshold: the numbers go into INTEGRATION.md's section "Stereo perception".

    python tools/time_stereo.py [--sizes 256 2048] [--atoms 30] [--reps 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moldiff_amd import canon as C  # noqa: E402
from moldiff_amd import molpack  # noqa: E402
from moldiff_amd import stereo as S  # noqa: E402
from time_canon import extended  # noqa: E402
from time_rings import ELEMENTS  # noqa: E402


def timed(call, reps):
    """ms per call over `reps` calls between two device events, after five warm-up calls"""
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 2048])
    ap.add_argument('--atoms', type=int, default=30)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(args.device))
    rows, same = [], True
    for size in args.sizes:
        g = np.random.default_rng(0)
        mols = [extended(g, max(12, int(g.normal(args.atoms, 5)))) for _ in range(size)]
        for m in mols:
            m['atom_pos'] = (g.normal(size=(len(m['element']), 3)) * 2).astype(np.float32)
        p = molpack.pack_mols(mols, ELEMENTS, positions=True)
        cm = molpack.CompactMols.from_packed(molpack.to_device(p, args.device))
        canon_out = C.launch(cm)
        canon_ms = timed(lambda: C.launch(cm), args.reps)
        stereo_ms = timed(lambda: S.launch(cm, canon_out, atomic_numbers=ELEMENTS), args.reps)
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
    print(json.dumps({'batches': rows, 'includes': 'the zero-fill of the output tensors of each call', 'device_equals_host': bool(same)}))
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
