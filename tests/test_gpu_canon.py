"""GPU tests of the canonical labelling (mdx_mol_canon through canon.canon_mols, canon.launch, FeaturizeMol.canon_batch and the sampling
entry point's --canonical).  The oracle is the plain restatement ``canon_ref``; every output is an integer (or a copied position) that
the definition makes unique, so every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import canon as C
from moldiff_amd import kekule as K
from moldiff_amd.harness import placeholder_from_sizes
from moldiff_amd.postprocess import FeaturizeMol
from .canon_cases import ELEMENTS, K5, NAMED, chain, decorated, mol, permuted, random_mol, ring

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
NOISY = mol([7] + [6] * 5, [(0, 9, 4), (2, 2, 4)] + ring(6, t=4) + [(-1, 3, 2)])          # pyridine with three ignored bonds
DOUBLED = mol([6, 6, 8], [(0, 1), (1, 0), (1, 2, 2), (2, 1, 2), (1, 2, 1)])                # bonds as a multiset
DEEP = mol(140, [(2 * k, 2 * k + 1) for k in range(70)])                                   # a node deeper than 64 after 66 nodes
IMIDAZOLE_LIKE = mol([7, 6, 7, 6, 6, 6], ring(5, t=4) + [(3, 5, 1)])
PYRIDONE_LIKE = mol([7] + [6] * 5 + [8, 6], ring(6, t=4) + [(1, 6, 2), (3, 7, 1)])


def same(got, ref, what, keys=None):
    got = molpack.to_host(got)
    for k in keys or ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape, ref[k].shape)
        bad = np.flatnonzero((got[k] != ref[k]).reshape(-1))
        assert len(bad) == 0, (what, k, bad[:8], got[k].reshape(-1)[bad[:8]], ref[k].reshape(-1)[bad[:8]])


def test_the_named_cases_the_caps_and_the_odd_molecules_as_one_batch():
    mols = list(NAMED.values()) + [mol(0, []), mol(1, []), NOISY, DOUBLED, K5, chain(256), chain(257), DEEP, mol([8], [])]
    want = C.stack_ref(mols)
    at = len(NAMED)
    assert want['status'][at:].tolist() == [0, 0, 0, 0, 0, 0, 1, 2, 0] and want['n_aut'][at:].tolist() == [1, 1, 2, 1, 120, 2, 0, 0, 1]
    assert want['n_aut'][:2].tolist() == [12, 2] and want['canon_n_bonds'][at + 2:at + 4].tolist() == [6, 5]
    got = molpack.to_host(C.canon_mols(mols, DEV))
    same(got, want, 'named')
    assert C.summary(got) == C.summary(want)
    again = molpack.to_host(C.canon_mols(mols[::-1], DEV))
    for m in range(len(mols)):                                         # independent of the place in the batch
        a, b = C.mol_result(got, m), C.mol_result(again, len(mols) - 1 - m)
        assert all(np.array_equal(a[k], b[k]) for k in a), m


def test_a_random_batch_and_its_permuted_copies():
    mols = [random_mol(3000 + s, 3, 35) for s in range(16)] + [decorated(random_mol(3100 + s, 3, 35)) for s in range(16)]
    copies = [permuted(m, 50 + k) for k, m in enumerate(mols)]
    both = mols + [c[0] for c in copies]
    want = C.stack_ref(both)
    assert (want['status'] == 0).all() and (want['n_aut'][16:32] >= 12).all() and (want['n_nodes'][16:32] > 20).all()
    got = molpack.to_host(C.canon_mols(both, DEV))
    same(got, want, 'random')
    for m in range(len(mols)):
        a, b = C.mol_result(got, m), C.mol_result(got, len(mols) + m)
        for k in ('n_nodes', 'n_leaves', 'n_aut', 'cert_hash', 'canon_atom_type', 'canon_bond_index', 'canon_bond_type'):
            assert np.array_equal(a[k], b[k]), (m, k)
        assert C.certificate(got, m) == C.certificate(got, len(mols) + m)
        new = copies[m][1]
        assert len(set(zip(a['orbit'].tolist(), b['orbit'][new].tolist()))) == len(set(a['orbit'].tolist()))


def test_the_node_budget_on_k5():
    for budget, status in ((206, 0), (205, 2), (1, 2), (1 << 20, 0)):
        want = C.stack_ref([K5, NAMED['benzene'], mol(1, [])], max_nodes=budget)
        assert want['status'].tolist() == [status, 0 if budget >= 19 else 2, 0]
        same(C.canon_mols([K5, NAMED['benzene'], mol(1, [])], DEV, max_nodes=budget), want, ('budget', budget))
    r = C.mol_result(C.stack_ref([K5], max_nodes=206), 0)
    assert (r['n_nodes'], r['n_leaves'], r['n_aut']) == (206, 120, 120)


def test_labels_positions_select_and_a_molecule_past_the_arrays():
    mols = [decorated(random_mol(4000 + s, 3, 30)) for s in range(24)]
    for s, m in enumerate(mols):
        m['atom_pos'] = np.random.default_rng(s).normal(size=(len(m['element']), 3)).astype(np.float32)
    labels = [np.random.default_rng(100 + s).integers(0, 3, len(m['element'])) * 32767 for s, m in enumerate(mols)]
    want = C.stack_ref(mols, atom_label=labels)
    plain = C.stack_ref(mols)
    assert 'canon_pos' in want and 'canon_atom_label' in want and not np.array_equal(want['n_aut'], plain['n_aut'])
    same(C.canon_mols(mols, DEV, atom_label=labels), want, 'labels and positions')
    same(C.canon_mols(mols, DEV), plain, 'positions only')
    # both NULL, and select: the masked molecule has status 0, rank -1 and zeros everywhere, its slots included
    p = molpack.pack_mols(mols, ELEMENTS)
    cm = molpack.CompactMols.from_packed(molpack.to_device(p, DEV))
    masked = 5
    select = torch.ones(len(mols), dtype=torch.int32, device=DEV)
    select[masked] = 0
    ref = {k: v.copy() for k, v in plain.items() if k != 'canon_pos'}
    a0, b0, na, nb = (int(p[k][masked]) for k in ('atom_ptr', 'bond_ptr', 'n_atoms', 'n_bonds'))
    for k in C.STAT_KEYS + ('cert_hash',):
        ref[k][masked] = 0
    ref['rank'][a0:a0 + na] = -1
    ref['orbit'][a0:a0 + na] = ref['canon_atom_type'][a0:a0 + na] = 0
    ref['canon_bond_type'][b0:b0 + nb] = 0
    ref['canon_bond_index'][:, b0:b0 + nb] = 0
    out = C.launch(cm, select=select, positions=False)
    assert 'canon_pos' not in out and 'canon_atom_label' not in out
    N, E = int(p['n_atoms'].sum()), int(p['n_bonds'].sum())
    out = dict(out, **{k: out[k][:N] for k in C.ATOM_KEYS}, canon_bond_type=out['canon_bond_type'][:E], canon_bond_index=out['canon_bond_index'][:, :E])
    same(out, ref, 'select', keys=C.STAT_KEYS + ('cert_hash',) + C.ATOM_KEYS + ('canon_bond_type', 'canon_bond_index'))
    # a molecule whose extent leaves the arrays: status 0, zeros, and nothing of it is written (the arrays hold a sentinel)
    short = cm._replace(N_cap=N - 1)
    seven = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    o = {'rank': seven(N), 'orbit': seven(N), 'canon_atom_type': seven(N), 'canon_bond_index': seven(2, cm.Eh_stride),
         'canon_bond_type': seven(cm.Eh_stride), 'mol_stats': seven(len(mols), 5)}
    h = torch.full((len(mols),), 7, dtype=torch.int64, device=DEV)
    ops, at = short.operands()
    _lib.check(_lib.lib().mdx_mol_canon(*ops, None, None, None, 1 << 16, at(o['rank']), at(o['orbit']), at(o['canon_atom_type']), None, None,
                                        at(o['canon_bond_index']), at(o['canon_bond_type']), at(o['mol_stats']), at(h), _lib.stream()))
    torch.cuda.synchronize()
    last = len(mols) - 1
    a0, b0 = int(p['atom_ptr'][last]), int(p['bond_ptr'][last])
    assert o['mol_stats'][last].tolist() == [0] * 5 and int(h[last]) == 0
    assert all(bool((o[k][a0:] == 7).all()) for k in C.ATOM_KEYS) and bool((o['canon_bond_type'][b0:] == 7).all())
    assert bool((o['canon_bond_index'][:, b0:] == 7).all())
    assert np.array_equal(o['rank'][:a0].cpu().numpy(), plain['rank'][:a0]) and np.array_equal(h[:last].cpu().numpy(), plain['cert_hash'][:last])
    # no molecule
    got, ref = molpack.to_host(C.canon_mols([], DEV)), C.empty()
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype for k in ref)
    with pytest.raises(ValueError, match='label'):
        C.canon_mols(mols[:1], DEV, atom_label=[np.full(len(mols[0]['element']), 65536)])
    with pytest.raises(ValueError, match='max_nodes'):
        C.canon_mols(mols[:1], DEV, max_nodes=0)


def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.lib()
    ARG = 1
    mols = [dict(NAMED['benzene'], atom_pos=np.zeros((6, 3), dtype=np.float32)), dict(NAMED['pyridine'], atom_pos=np.ones((6, 3), dtype=np.float32))]
    p = molpack.pack_mols(mols, ELEMENTS, positions=True)
    d = molpack.to_device(p, DEV)
    N, E = 12, int(d['bond_index'].shape[1])
    seven = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    o = {'rank': seven(N), 'orbit': seven(N), 'canon_atom_type': seven(N), 'canon_atom_label': seven(N),
         'canon_pos': torch.full((N, 3), 7.0, device=DEV), 'canon_bond_index': seven(2, E), 'canon_bond_type': seven(E),
         'mol_stats': seven(2, 5), 'cert_hash': torch.full((2,), 7, dtype=torch.int64, device=DEV)}
    label = d['atom_type'] + 3

    def call(B=2, N_cap=N, stride=E, nodes=100, null=(), pos=True, lab=True):
        q = lambda name, t: None if name in null else _lib.ptr(t)
        return L.mdx_mol_canon(B, q('atom_ptr', d['atom_ptr']), _lib.ptr(d['bond_ptr']), _lib.ptr(d['n_atoms']), _lib.ptr(d['n_bonds']),
                               q('atom_type', d['atom_type']), N_cap, _lib.ptr(d['bond_type']), q('bond_index', d['bond_index']), stride, None,
                               _lib.ptr(d['atom_pos']) if pos else None, _lib.ptr(label) if lab else None, nodes,
                               *(q(k, o[k]) for k in ('rank', 'orbit', 'canon_atom_type', 'canon_atom_label', 'canon_pos', 'canon_bond_index',
                                                      'canon_bond_type', 'mol_stats', 'cert_hash')), _lib.stream())
    for name in ('atom_ptr', 'atom_type', 'bond_index', 'rank', 'orbit', 'canon_atom_type', 'canon_bond_index', 'canon_bond_type', 'mol_stats',
                 'cert_hash'):
        assert call(null=(name,)) == ARG and b'null' in L.mdx_last_error(), name
    assert call(null=('canon_atom_label',)) == ARG and b'both or neither' in L.mdx_last_error()
    assert call(null=('canon_pos',)) == ARG and call(pos=False) == ARG and call(lab=False) == ARG
    assert call(B=-1) == ARG and call(N_cap=-1) == ARG and call(stride=-1) == ARG
    assert call(nodes=0) == ARG and b'max_nodes' in L.mdx_last_error() and call(nodes=(1 << 20) + 1) == ARG
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in o.values())
    assert call() == 0 and call(pos=False, lab=False, null=('canon_pos', 'canon_atom_label')) == 0
    torch.cuda.synchronize()
    ref = C.stack_ref(mols, atom_label=[np.asarray([3] * 6), np.asarray([4] + [3] * 5)], max_nodes=100)
    assert o['mol_stats'].cpu().numpy().tolist() == np.stack([ref[k] for k in C.STAT_KEYS], 1).tolist()
    assert np.array_equal(o['canon_atom_label'].cpu().numpy(), ref['canon_atom_label']) and np.array_equal(o['canon_pos'].cpu().numpy(), ref['canon_pos'])


def _pred_of(mols, masks):
    """one-hot predictions that decode to `mols`, molecule k preceded by masks[k] mask-type atoms (which the decode drops)"""
    cls = {z: i for i, z in enumerate(ELEMENTS)}
    pn, pp, ph = [], [], []
    for m, shift in zip(mols, masks):
        ids = np.concatenate([np.full(shift, 7), [cls[int(z)] for z in m['element']]]).astype(np.int64)
        n = len(ids)
        T = np.zeros((n, n), dtype=np.int64)
        nb = m['bond_index'].shape[1] // 2
        for (i, j), t in zip(m['bond_index'][:, :nb].T, m['bond_type'][:nb]):
            T[min(i, j) + shift, max(i, j) + shift] = t
        iu, ju = np.triu_indices(n, 1)
        pn.append((10.0 * np.eye(8)[ids]).astype(np.float32))
        pp.append(np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32))
        ph.append((10.0 * np.eye(6)[T[iu, ju]]).astype(np.float32).reshape(-1, 6))
    ph_ = placeholder_from_sizes([len(x) for x in pn], DEV)
    pred = [torch.from_numpy(np.concatenate(x)).to(DEV) for x in (pn, pp, ph)]
    return (pred, ph_['batch_node'], ph_['halfedge_index'], ph_['batch_halfedge'], len(mols))


def _check_layout(got, listed, decoded, masked=()):
    got = molpack.to_host(got)
    for m in range(len(decoded)):
        zero = m in masked
        for k in C.MOL_KEYS:
            assert got[k][m] == (0 if zero else listed[k][m]), (k, m)
        a0, la, na = int(got['atom_ptr'][m]), int(listed['atom_ptr'][m]), len(decoded[m]['element'])
        b0, lb, nb = int(got['bond_ptr'][m]), int(listed['bond_ptr'][m]), int(listed['n_bonds'][m])
        for k in ('orbit', 'canon_atom_type', 'canon_pos'):
            assert np.array_equal(got[k][a0:a0 + na], listed[k][la:la + na] * (not zero)), (k, m)
        assert np.array_equal(got['rank'][a0:a0 + na], np.full(na, -1) if zero else listed['rank'][la:la + na]), m
        assert np.array_equal(got['canon_bond_type'][b0:b0 + nb], listed['canon_bond_type'][lb:lb + nb] * (not zero)), m
        assert np.array_equal(got['canon_bond_index'][:, b0:b0 + nb], listed['canon_bond_index'][:, lb:lb + nb] * (not zero)), m


def test_canon_batch_on_the_decode_layout_equals_canon_mols_of_its_molecules():
    mols = [NAMED['benzene'], IMIDAZOLE_LIKE, NAMED['cubane'], random_mol(7, 10, 20), PYRIDONE_LIKE, NAMED['two_equal_fragments'],
            random_mol(8, 10, 20), K5]
    args = _pred_of(mols, masks=[2, 1, 0, 0, 3, 0, 1, 2])
    decoded = FEAT.decode_batch(*args)
    assert [len(d['element']) for d in decoded] == [len(m['element']) for m in mols]
    listed, ref = molpack.to_host(C.canon_mols(decoded, DEV)), C.stack_ref(decoded)
    same(listed, ref, 'canon_mols of the decoded list')
    assert ref['n_aut'].tolist()[:3] == [12, 1, 48] and (ref['status'] == 0).all()
    res, canonical, keep = FEAT.canon_batch(*args)
    _check_layout(res, listed, decoded)
    assert keep.tolist() == [1] * 8 and canonical.atom_ptr is res['atom_ptr'] and canonical.N_cap == res['rank'].shape[0]
    select = torch.tensor([1, 1, 1, 1, 1, 0, 1, 1], device=DEV)
    res, canonical, keep = FEAT.canon_batch(*args, select=select, max_nodes=205)          # K5 is abandoned, molecule 5 masked
    listed2 = molpack.to_host(C.canon_mols(decoded, DEV, max_nodes=205))
    assert listed2['status'].tolist() == [0] * 7 + [2]
    _check_layout(res, listed2, decoded, masked=(5,))
    assert keep.tolist() == [1, 1, 1, 1, 1, 0, 1, 0]


def test_the_kekule_kernel_on_the_canonical_arrays_of_permuted_copies():
    base = [IMIDAZOLE_LIKE, PYRIDONE_LIKE, NAMED['pyridine'], NAMED['benzene'], random_mol(11, 10, 24, elements=(6, 7), types=(4, 1, 2)),
            mol([7, 6, 7, 6, 6, 7, 6, 6, 6, 6], ring(5, t=4) + ring(5, 5, t=4) + [(4, 9, 1)]), K5]
    outs = []
    for s in range(3):
        mols = base if s == 0 else [permuted(m, 31 * s + k)[0] for k, m in enumerate(base)]
        cm = molpack.CompactMols.from_packed(molpack.to_device(molpack.pack_mols(mols, ELEMENTS), DEV))
        res = C.launch(cm, max_nodes=205)
        canonical, keep = C.canonical_compact(cm, res)
        assert keep.tolist() == [1] * 6 + [0]
        kek = molpack.to_host(K.launch(canonical, select=keep))
        outs.append(kek)
        if s == 0:                                                     # what the host path gives for the canonical molecules
            host_res = C.stack_ref(mols, max_nodes=205)
            for m in range(6):
                want = K.kekulize_ref(C.canonical_mol(mols[m], C.mol_result(host_res, m)))
                a0, b0 = int(cm.atom_ptr[m]), int(cm.bond_ptr[m])
                assert np.array_equal(kek['kek_h'][a0:a0 + want['n_atoms']], want['kek_h'])
                assert np.array_equal(kek['kek_order'][b0:b0 + want['n_bonds']], want['kek_order'])
            assert kek['n_double'][:4].tolist() == [2, 2, 3, 3] and kek['n_hydrogens'][0] > 0
    for other in outs[1:]:
        assert all(np.array_equal(outs[0][k], other[k]) for k in outs[0])


def _sample(tmp_path, name, extra):
    from moldiff_amd import sample_drug3d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log_dir = sample_drug3d.main(['--config', os.path.join(root, 'configs', 'sample_MolDiff_simple.yml'), '--outdir', str(tmp_path / name),
                                  '--device', DEV, '--recipe-weights', '--num_steps', '2', '--num_mols', '4', '--batch_size', '8'] + extra)
    return log_dir, torch.load(os.path.join(log_dir, 'samples_all.pt'), weights_only=False)


def test_entry_point_writes_the_canonical_files(tmp_path):
    new = {'canon.json', 'canon.npz', 'samples.smi'}
    kek = {'kekule.json', 'kekule.npz', 'samples_kekule.sdf'}
    # the seed is sample.seed + sum(ord(outdir)): the directory names are permutations of each other, so the runs sample the same molecules
    d0, pool0 = _sample(tmp_path, 'abc', ['--largest_fragment', '0.2'])
    assert not (new | kek) & set(os.listdir(d0)) and not any('smiles' in m for m in pool0['finished'] + pool0['failed'])
    d1, pool = _sample(tmp_path, 'bca', ['--largest_fragment', '0.2', '--canonical', '--kekulize', '--canonical_max_nodes', '500'])
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new | kek) and new | kek <= set(os.listdir(d1))
    assert len(pool['finished']) >= 2 and [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    ref = C.stack_ref(pool['finished'], max_nodes=500)     # untrained weights decode to nearly complete graphs: mostly abandoned
    saved = molpack.load_npz(os.path.join(d1, 'canon.npz'))
    assert set(saved) == set(ref) and all(np.array_equal(saved[k], ref[k]) and saved[k].dtype == ref[k].dtype for k in ref)
    with open(os.path.join(d1, 'canon.json')) as f:
        got = json.load(f)
    want = C.summary(ref)
    print('finished', len(pool['finished']), 'status', ref['status'].tolist(), 'n_nodes', ref['n_nodes'].tolist())
    assert got['n_molecules'] == len(pool['finished']) and got['n_distinct'] == want['n_distinct'] and got['nodes_hist'] == want['nodes_hist']
    texts = C.smiles_mols(pool['finished'], ref)
    assert [m['smiles'] for m in pool['finished']] == texts
    with open(os.path.join(d1, 'samples.smi')) as f:
        lines = f.read().splitlines()
    assert lines == ['%s\t%d' % (t, m['mol_id']) for t, m in zip(texts, pool['finished']) if t]
