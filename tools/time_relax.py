"""Times one launch of the force-field relaxation (mdx_mol_relax with the default table, after mdx_mol_kekulize and mdx_mol_hydrogens on the
same batch) against the Python restatement ``relax_ref`` on this host: 256 synthetic drug-sized molecules (the batch of
tools/time_hydrogens.py: Gaussian coordinates, so crude geometries far from a minimum), device events after a warm-up, at ``--iters``
iterations at most; the restatement runs on the first ``--ref`` molecules only, with the same limit, and must agree with the device in
status, stop reason and the iteration and evaluation counts.  Prints one JSON line and writes it to profiles/relax_timing.txt.  One
measurement, no threshold; nothing is gated on it and nothing about throughput is claimed beyond the line.

    python tools/time_relax.py [--size 256] [--atoms 30] [--iters 200] [--reps 5] [--ref 4] [--out FILE]
"""
import sys
import time

import numpy as np
import torch

import evalbench as EB
from moldiff_amd import hydrogens as H
from moldiff_amd import kekule as K
from moldiff_amd import molpack
from moldiff_amd import relax as R


def main(argv=None):
    ap = EB.parser(reps=5, atoms=30, out=EB.profile_path('relax_timing.txt'))
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--iters', type=int, default=R.DEFAULT_MAX_ITERS)
    ap.add_argument('--ref', type=int, default=4)
    args = EB.parse(ap, argv)
    mols, p, cm, _ = EB.batch(args.size, args.atoms, args.device, pos_sigma=2.5)
    kek = K.launch(cm, K.KekuleTables())
    hyd = H.launch(cm, kek['kek_h'], kek['kek_order'], H.HydrogenTables())
    tb = R.ForceFieldTables()
    ms, out = EB.timed(lambda: R.launch(cm, kek['kek_order'], hyd['h_pos'], hyd['h_count'], hyd['atom_flag'], tb, args.iters), args.reps)
    got = R._dense({k: v for k, v in out.items()}, cm, p)
    got = molpack.to_host(got)
    hk, hh = molpack.to_host(molpack.dense(dict(kek), cm, p, K.LAYOUT)), molpack.to_host(H._dense(dict(hyd), cm, p))
    n_ref, agree, t0 = min(args.ref, args.size), True, time.perf_counter()
    for m in range(n_ref):
        hr = H.mol_result(hh, m)
        ref = R.relax_ref(mols[m], K.mol_result(hk, m)['kek_order'], hr['h_count'], hr['h_pos'], hr['atom_flag'], tb, args.iters)
        agree = agree and all(int(got[k][m]) == ref[k] for k in ('status', 'stop_reason', 'iterations', 'n_evals', 'n_all'))
    ref_s = time.perf_counter() - t0
    ok = got['status'] == R.STATUS_OK
    row = {'molecules': args.size, 'atoms_with_hydrogens': int(got['n_all'].astype(np.int64).sum()), 'max_iters': args.iters,
           'relaxed': int(ok.sum()), 'too_large': int((got['status'] == R.STATUS_TOO_LARGE).sum()), 'nonfinite': int((got['status'] == R.STATUS_NONFINITE).sum()),
           'iterations_total': int(got['iterations'].astype(np.int64).sum()), 'evaluations_total': int(got['n_evals'].astype(np.int64).sum()),
           'relax_ms_per_batch': round(ms, 3), 'relax_ms_per_molecule': round(ms / max(args.size, 1), 4),
           'restatement_molecules': n_ref, 'restatement_s_per_molecule': round(ref_s / max(n_ref, 1), 3), 'restatement_agrees': bool(agree),
           'includes': 'the zero-fill of the output tensors and the workspace allocation', 'device': torch.cuda.get_device_name(0)}
    EB.report([row], args.out, 'tools/time_relax.py: one measurement, not gated')
    return 0 if agree else 1


if __name__ == '__main__':
    sys.exit(main())
