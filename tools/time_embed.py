"""Times one launch of conformer generation (mdx_mol_bounds + mdx_mol_embed with the default table and settings, after mdx_mol_kekulize and
mdx_mol_hydrogens on the same batch): 256 random molecules of 20-30 heavy atoms (the generator of tests/relax_cases.py) x 10
conformers, device events after a warm-up; alongside, the wall time of the restatement ``embed_ref`` on the first ``--ref`` molecules x
1 conformer for scale.  Prints one JSON line and writes it to profiles/embed_timing.txt.  One measurement, no threshold; nothing is
gated on it and nothing about throughput or sample quality is claimed beyond the line.

    python tools/time_embed.py [--size 256] [--confs 10] [--reps 3] [--ref 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from moldiff_amd import embed as E  # noqa: E402
from moldiff_amd import hydrogens as H  # noqa: E402
from moldiff_amd import kekule as K  # noqa: E402
from moldiff_amd import molpack  # noqa: E402
from moldiff_amd import relax as R  # noqa: E402
from tests.relax_cases import random_mol  # noqa: E402
from time_hydrogens import timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--confs', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ref', type=int, default=4)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'embed_timing.txt'))
    args = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(args.device))
    g = np.random.default_rng(0)
    mols = []
    while len(mols) < args.size:
        m = random_mol(g)
        if 20 <= len(m['element']) <= 30:
            mols.append(m)
    tb = R.ForceFieldTables()
    p = molpack.pack_mols(mols, tb.atomic_numbers, positions=True)
    cm = molpack.CompactMols.from_packed(molpack.to_device(p, args.device))
    kek = K.launch(cm, K.KekuleTables())
    hyd = H.launch(cm, kek['kek_h'], kek['kek_order'], H.HydrogenTables())
    hc = molpack.host(hyd['h_count'])
    n_all = [int(n) + int(np.clip(hc[int(a):int(a) + int(n)], 0, 4).sum()) for a, n in zip(p['atom_ptr'], p['n_atoms'])]
    cap = E._cap(max(n_all))
    ms, out = timed(lambda: E.launch(cm, kek['kek_order'], hyd['h_count'], hyd['atom_flag'], args.confs, 0, tb, na_cap=cap), args.reps)
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
    print(json.dumps(row))
    if os.access(os.path.dirname(args.out), os.W_OK):
        with open(args.out, 'w') as f:
            f.write('tools/time_embed.py: one measurement, not gated\n' + json.dumps(row) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
