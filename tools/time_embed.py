"""Times one launch of conformer generation (mdx_mol_bounds + mdx_mol_embed with the default table and settings, after mdx_mol_kekulize and
mdx_mol_hydrogens on the same batch): 256 random molecules of 20-30 heavy atoms (the generator of tests/relax_cases.py) x 10
conformers, device events after a warm-up; alongside, the wall time of the restatement ``embed_ref`` on the first ``--ref`` molecules x
1 conformer for scale.  Prints one JSON line and writes it to profiles/embed_timing.txt.  One measurement, no threshold; nothing is
gated on it and nothing about throughput or sample quality is claimed beyond the line.

    python tools/time_embed.py [--size 256] [--confs 10] [--reps 3] [--ref 4] [--out FILE]
"""
import sys
import time

import numpy as np
import torch

import evalbench as EB
from moldiff_amd import embed as E
from moldiff_amd import hydrogens as H
from moldiff_amd import kekule as K
from moldiff_amd import molpack
from moldiff_amd import relax as R
from tests.relax_cases import random_mol


def main(argv=None):
    ap = EB.parser(reps=3, out=EB.profile_path('embed_timing.txt'))
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--confs', type=int, default=10)
    ap.add_argument('--ref', type=int, default=4)
    args = EB.parse(ap, argv)
    g = np.random.default_rng(0)
    mols = []
    while len(mols) < args.size:
        m = random_mol(g)
        if 20 <= len(m['element']) <= 30:
            mols.append(m)
    tb = R.ForceFieldTables()
    mols, p, cm, _ = EB.batch(args.size, None, args.device, mols=mols, elements=tb.atomic_numbers)
    kek = K.launch(cm, K.KekuleTables())
    hyd = H.launch(cm, kek['kek_h'], kek['kek_order'], H.HydrogenTables())
    hc = molpack.host(hyd['h_count'])
    n_all = [int(n) + int(np.clip(hc[int(a):int(a) + int(n)], 0, 4).sum()) for a, n in zip(p['atom_ptr'], p['n_atoms'])]
    cap = E._cap(max(n_all))
    ms, out = EB.timed(lambda: E.launch(cm, kek['kek_order'], hyd['h_count'], hyd['atom_flag'], args.confs, 0, tb, na_cap=cap), args.reps)
    got = molpack.to_host(dict(out))
    st = got['status'].reshape(-1)
    inputs = R._inputs(mols[:args.ref], tb)
    t0 = time.perf_counter()
    agree = True
    for m, (info, i) in enumerate(zip(mols[:args.ref], inputs)):
        ref = E.embed_ref(E.bounds_ref(info, i[0], i[1], i[3], tb), 0, 0, m)
        agree = agree and all(int(got[k][m, 0]) == ref[k] for k in E.CONF_KEYS)
    ref_s = time.perf_counter() - t0
    row = {'molecules': args.size, 'conformers': args.confs, 'na_cap': cap, 'atoms_with_hydrogens_mean': round(float(np.mean(n_all)), 1),
           'ok': int((st == E.STATUS_OK).sum()), 'failed': int((st == E.STATUS_FAILED).sum()), 'inconsistent': int((st == E.STATUS_INCONSISTENT).sum()),
           'fraction_failed': round(float((st == E.STATUS_FAILED).mean()), 4), 'attempts_mean': round(float(got['attempts'].mean()), 3),
           'evaluations_total': int(got['n_evals'].astype(np.int64).sum()), 'bounds_and_embed_ms_per_batch': round(ms, 3),
           'ms_per_conformer': round(ms / max(args.size * args.confs, 1), 4), 'restatement_conformers': len(inputs),
           'restatement_s_total': round(ref_s, 3), 'restatement_agrees_in_the_integers': bool(agree),
           'includes': 'the zero-fill of the outputs and the allocation of the workspaces', 'device': torch.cuda.get_device_name(0)}
    EB.report([row], args.out, 'tools/time_embed.py: one measurement, not gated')
    return 0


if __name__ == '__main__':
    sys.exit(main())
