"""One-off behaviour check for changes to the host side of the five evaluation modules (rings, groups, kekule, canon, framework;
development tool): dumps what every public function that makes, joins or slices a results dict returns, one .npz per case, so that a
tree before and a tree after such a change can be compared array by array.

  python tools/eval_results_dump.py OUTDIR [--device cuda:0]   the host functions (stack_ref, empty, concat, mol_result, the key tuples)
                                                               on the fixed lists below; with --device also launch and <name>_mols on
                                                               the same lists and the five FeaturizeMol.<name>_batch methods on one
                                                               decoded batch of three molecules, with and without a `select` that
                                                               leaves the middle one out
  python tools/eval_results_dump.py --compare A B              key sets, dtypes, shapes and bytes of every case; exit status 1 on any
                                                               difference

The lists: the designed list and the list without any bond of tests/test_gpu_molpack.py, the empty list, and a list with an atom-less
molecule, which ``concat`` also gets in three parts, the middle one empty."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODULES = ('rings', 'groups', 'kekule', 'canon', 'framework')
TUPLES = ('MOL_KEYS', 'ATOM_KEYS', 'BOND_KEYS', 'SLOT_KEYS', 'STAT_KEYS', 'INDEX_KEYS', 'POS_KEYS', 'SET_KEYS')


def lists():
    from tests.test_gpu_molpack import BONDLESS, DESIGNED
    nothing = {'element': np.zeros(0, dtype=np.int64), 'atom_pos': np.zeros((0, 3), dtype=np.float32)}
    return {'designed': (DESIGNED, (2, 2, 2)), 'bondless': (BONDLESS, (1, 0, 2)), 'empty': ([], ()),
            'atomless': ([DESIGNED[1], nothing, DESIGNED[5]], (2, 0, 1))}


def split(mols, sizes):
    """`mols` cut into consecutive parts of the given sizes"""
    out, k = [], 0
    for s in sizes:
        out.append(mols[k:k + s])
        k += s
    assert k == len(mols)
    return out


def variants(name, mols):
    """(tag, keyword arguments shared by stack_ref and <name>_mols) per module"""
    if name == 'canon':
        return [('', {}), ('_labelled', {'atom_label': [np.arange(len(m['element'])) % 3 for m in mols]})]
    if name == 'framework':
        return [('', {}), ('_exo_generic', {'mode': 3, 'sys_bins': 3})]
    if name == 'rings':
        return [('', {}), ('_bins3', {'ring_bins': 3})]
    return [('', {})]


def save(outdir, case, results):
    """a results dict (numpy or torch, ints and tuples allowed) -> OUTDIR/case.npz; key order is recorded as well"""
    from moldiff_amd import molpack
    arrays = {k: np.asarray(v) if isinstance(v, (int, tuple, list)) else v for k, v in results.items()}
    arrays = molpack.to_host(arrays)
    assert '__order__' not in arrays
    arrays['__order__'] = np.asarray(list(results), dtype=str)
    with open(os.path.join(outdir, case.replace('/', '.') + '.npz'), 'wb') as f:
        np.savez(f, **arrays)
    print(case, len(results), 'keys', flush=True)


def dump_host(outdir):
    import importlib
    for name in MODULES:
        mod = importlib.import_module('moldiff_amd.' + name)
        save(outdir, f'{name}/tuples', {t: np.asarray(getattr(mod, t), dtype=str) for t in TUPLES if hasattr(mod, t)})
        save(outdir, f'{name}/empty', mod.empty())
        if name == 'framework':
            save(outdir, f'{name}/empty_with_keys', mod.empty(with_keys=True))
        for lname, (mols, sizes) in lists().items():
            for tag, kw in variants(name, mols):
                case = f'{name}/{lname}{tag}'
                res = mod.stack_ref(mols, **kw)
                save(outdir, case + '/stack_ref', res)
                if hasattr(mod, 'mol_result'):
                    for m in range(len(mols)):
                        save(outdir, f'{case}/mol_result{m}', mod.mol_result(res, m))
                if sizes:
                    parts, k = [], 0
                    for part in split(mols, sizes):
                        pkw = {key: v[k:k + len(part)] if key == 'atom_label' else v for key, v in kw.items()}
                        parts.append(mod.stack_ref(part, **pkw))
                        k += len(part)
                    save(outdir, case + '/concat', mod.concat(parts))
            if name == 'framework' and sizes:
                save(outdir, f'{name}/{lname}/concat_with_keys', mod.concat([mod.stats_mols(part) for part in split(mols, sizes)]))


def pred_of(mols, masks, elements, dev):
    """one-hot predictions that decode to `mols`, molecule k preceded by masks[k] mask-type atoms (tests/test_gpu_rings.py)"""
    import torch
    from moldiff_amd.harness import placeholder_from_sizes
    cls = {z: i for i, z in enumerate(elements)}
    pn, pp, ph = [], [], []
    for m, shift in zip(mols, masks):
        ids = np.concatenate([np.full(shift, 7), [cls[int(z)] for z in m['element']]]).astype(np.int64)
        n = len(ids)
        T = np.zeros((n, n), dtype=np.int64)
        nb = m['bond_index'].shape[1] // 2
        for (i, j), t in zip(m['bond_index'][:, :nb].T, m['bond_type'][:nb]):
            T[min(i, j) + shift, max(i, j) + shift] = t
        iu, ju = np.triu_indices(n, 1)
        pos = np.concatenate([np.zeros((shift, 3)), m['atom_pos']]).astype(np.float32)
        pn.append((10.0 * np.eye(8)[ids]).astype(np.float32)), pp.append(pos)
        ph.append((10.0 * np.eye(6)[T[iu, ju]]).astype(np.float32).reshape(-1, 6))
    ph_ = placeholder_from_sizes([len(x) for x in pn], dev)
    pred = [torch.from_numpy(np.concatenate(x)).to(dev) for x in (pn, pp, ph)]
    return (pred, ph_['batch_node'], ph_['halfedge_index'], ph_['batch_halfedge'], len(mols))


def dump_device(outdir, dev):
    import torch
    from moldiff_amd import canon, framework, groups, kekule, molpack, rings
    from moldiff_amd.postprocess import FeaturizeMol
    from tests.test_gpu_molpack import mol
    torch.cuda.set_device(torch.device(dev))
    Z = molpack.DEFAULT_ATOMIC_NUMBERS
    pset = groups.PatternSet.default()
    for lname, (mols, _) in lists().items():
        for name, mod, fn in (('rings', rings, rings.rings_mols), ('groups', groups, groups.groups_mols), ('kekule', kekule, kekule.kekulize_mols),
                              ('canon', canon, canon.canon_mols), ('framework', framework, framework.framework_mols)):
            for tag, kw in variants(name, mols):
                save(outdir, f'{name}/{lname}{tag}/mols', fn(mols, dev, **kw))
        res, cm, full = framework.framework_mols(mols, dev, with_cm=True)
        save(outdir, f'framework/{lname}/mols_with_cm', res)
        save(outdir, f'framework/{lname}/stats_mols', framework.stats_mols(mols, dev))
        # launch on the packed arrays, untrimmed
        cm = molpack.CompactMols.from_packed(molpack.to_device(molpack.pack_mols(mols, Z, positions=len(mols) > 0), dev))
        ring_data = rings.launch(cm, len(Z), 4)
        save(outdir, f'rings/{lname}/launch', ring_data)
        save(outdir, f'groups/{lname}/launch', groups.launch(cm, pset))
        save(outdir, f'kekule/{lname}/launch', kekule.launch(cm))
        save(outdir, f'canon/{lname}/launch', canon.launch(cm))
        save(outdir, f'canon/{lname}/launch_no_positions', canon.launch(cm, positions=False))
        lab = torch.arange(max(cm.N_cap, 1), dtype=torch.int32, device=dev) % 3
        save(outdir, f'canon/{lname}/launch_labelled', canon.launch(cm, atom_label=lab))
        save(outdir, f'framework/{lname}/launch', framework.launch(cm, ring_data))
        save(outdir, f'framework/{lname}/launch_no_positions', framework.launch(cm, ring_data, 3, 3, positions=False))
    # the batch methods on one decoded batch: a benzene behind two mask atoms, a two-atom molecule, a fused pair of rings
    feat = FeaturizeMol(list(Z), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    benzene = mol([6] * 6, [(k, (k + 1) % 6, 4) for k in range(6)], 1)
    fused = mol([6, 6, 7, 6, 6, 8, 6], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 0, 1), (3, 4, 2), (4, 5, 1), (5, 0, 1), (4, 6, 1)], 2)
    args = pred_of([benzene, mol([6, 8], [(0, 1, 2)], 3), fused], [2, 0, 1], Z, dev)
    for tag, select in (('', None), ('_select', torch.tensor([1, 0, 1], device=dev))):
        save(outdir, 'batch/rings' + tag, feat.rings_batch(*args, select=select))
        save(outdir, 'batch/groups' + tag, feat.groups_batch(*args, pset, select=select))
        save(outdir, 'batch/kekule' + tag, feat.kekulize_batch(*args, select=select))
        res, canonical, keep = feat.canon_batch(*args, select=select)
        save(outdir, 'batch/canon' + tag, res)
        save(outdir, 'batch/canon_compact' + tag, dict({k: v for k, v in canonical._asdict().items() if v is not None}, keep=keep))
        res, cm = feat.framework_batch(*args, mode=1, select=select)
        save(outdir, 'batch/framework' + tag, res)
    torch.cuda.synchronize()


def compare(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = []
    for name in names:
        if not (os.path.exists(os.path.join(a, name)) and os.path.exists(os.path.join(b, name))):
            bad.append(name + ': on one side only')
            continue
        with np.load(os.path.join(a, name)) as A, np.load(os.path.join(b, name)) as B:
            diff = [f'{k}: on one side only' for k in sorted(set(A.files) ^ set(B.files))]
            for k in sorted(set(A.files) & set(B.files)):
                x, y = A[k], B[k]
                if k == '__order__':
                    if x.tolist() != y.tolist():
                        print(f'{name}: key order differs (not counted)')
                elif x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                    diff.append(f'{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}' + ('' if x.shape != y.shape else ', values differ'))
            print(f'{name:60s} {len(A.files) - 1:3d} keys  {"equal" if not diff else "DIFFERENT: " + "; ".join(diff)}')
            bad += [f'{name}: {d}' for d in diff]
    print(f'{len(names)} cases: ' + ('ALL EQUAL' if not bad else f'{len(bad)} DIFFERENCES'))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    if len(sys.argv) == 4 and sys.argv[2] == '--device':
        dump_device(out, sys.argv[3])
    else:
        dump_host(out)
