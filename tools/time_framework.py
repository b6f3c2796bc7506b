"""Times the framework path on the batch of tools/time_canon.py (256 synthetic drug-sized molecules with an aromatic ring, a CF3 and a
tert-butyl group) with device events after a warm-up: mdx_mol_rings + mdx_mol_framework + the two mdx_mol_canon launches on the
framework and on the ring systems (``framework.keys`` without its copies to the host), mdx_mol_framework alone, and mdx_mol_rings alone
on the same batch in the same run; next to them ``framework_ref`` on this host.  Checks the batch against the host and prints one JSON
line.  One measurement, no threshold: the numbers go into profiles/framework_timing.txt.

    python tools/time_framework.py [--n 256] [--atoms 30] [--reps 50] [--mode 0] [--out FILE]
"""
import sys
import time

import numpy as np

import evalbench as EB
from evalbench import ELEMENTS
from moldiff_amd import canon as C
from moldiff_amd import framework as F
from moldiff_amd import molpack
from moldiff_amd import rings as R


def main(argv=None):
    ap = EB.parser(reps=50, atoms=30)
    ap.add_argument('--n', type=int, default=256)
    ap.add_argument('--mode', type=int, default=0)
    args = EB.parse(ap, argv)
    mols, p, cm, _ = EB.batch(args.n, args.atoms, args.device, gen=EB.extended)
    rings_only = lambda: R.launch(cm, len(ELEMENTS), 4)
    ring_data = rings_only()
    alone = lambda: F.launch(cm, ring_data, args.mode)

    def whole():
        res = F.launch(cm, rings_only(), args.mode)
        sy, _ = F.systems_compact(cm, res)                              # synchronises once: the number of systems
        return res, C.launch(F.framework_compact(cm, res), positions=False), C.launch(sy, positions=False)
    ms = {'rings_framework_two_canon': EB.timed(whole, args.reps)[0], 'framework_alone': EB.timed(alone, args.reps)[0],
          'rings_alone': EB.timed(rings_only, args.reps)[0]}
    res, fw_canon, sys_canon = whole()
    t0 = time.perf_counter()
    want = F.stack_ref(mols, args.mode)
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_keys = F.keys_ref(mols, want)
    host_keys_s = time.perf_counter() - t0
    got = molpack.to_host(res)
    N, E = int(p['n_atoms'].sum()), int(p['n_bonds'].sum())
    got.update({k: got[k][:N] for k in F.ATOM_KEYS}, **{k: got[k][:E] for k in F.BOND_KEYS}, **{k: got[k][:, :E] for k in F.INDEX_KEYS})
    same = all(np.array_equal(got[k], want[k]) for k in got)
    keys = F.keys(cm, res)
    same_keys = all(np.array_equal(keys[k], want_keys[k]) for k in keys)
    s = F.summary(want, want_keys, top_k=3)
    row = {'molecules': len(mols), 'atoms': N, 'bonds': E, 'mode': args.mode, 'systems': int(want['n_systems'].sum()),
           'framework_atoms': int(want['n_fw_atoms'].sum()), 'canon_nodes': int(fw_canon['n_nodes'].sum() + sys_canon['n_nodes'].sum()),
           'device_ms_per_batch': {k: round(v, 4) for k, v in ms.items()}, 'reps': args.reps,
           'includes': 'the zero-fill of the output tensors, the gather of the system records and its one sync',
           'host_framework_ref_s': round(host_s, 3), 'host_keys_ref_s': round(host_keys_s, 3), 'device_equals_host': bool(same),
           'keys_equal_host': bool(same_keys), 'n_distinct': s['n_distinct'], 'n_keyed': s['n_keyed'],
           'n_distinct_systems': s['n_distinct_systems'], 'top_systems': [(t['smiles'], t['count']) for t in s['top_systems']]}
    EB.report([row], args.out, 'tools/time_framework.py: one measurement, not gated')
    return 0 if same and same_keys else 1


if __name__ == '__main__':
    sys.exit(main())
