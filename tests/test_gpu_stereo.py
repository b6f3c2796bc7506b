"""GPU tests of the stereo perception (mdx_mol_stereo through stereo.stereo_mols, stereo.launch and FeaturizeMol.stereo_batch).  The
oracle is the plain restatement ``stereo_ref``; both sides compute the geometry in float64 with the same operation order, so every
comparison is exact.  A random molecule whose reference has a volume within 1e-6 of its threshold or a cosine within 1e-6 of
+-bond_tol is left out (float64 error of these few-operation expressions is about 1e-15, so the band is ample); at most 5 % may be, and
the share is asserted.  Fixtures are never left out."""
import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import canon as C
from moldiff_amd import stereo as S
from moldiff_amd.postprocess import FeaturizeMol
from .canon_cases import ELEMENTS, mol
from .stereo_cases import fixtures, moved, random_3d, with_pos

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIX = fixtures()
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)


def same(got, ref, what, keys=None, skip=()):
    """every key equal, molecule by molecule, but for the molecules of `skip`"""
    got = molpack.to_host(got)
    for k in keys or ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape, ref[k].shape)
    for m in range(len(ref['status'])):
        if m in skip:
            continue
        a, b = S.mol_result(got, m), S.mol_result(ref, m)
        for k in b:
            assert np.array_equal(a[k], b[k]), (what, m, k, a[k], b[k])


def test_the_fixtures_an_empty_and_a_one_atom_molecule_as_one_batch():
    mols = list(FIX.values()) + [with_pos(mol(0, []), np.zeros((0, 3))), with_pos(mol(1, []), [[1, 2, 3]])]
    want_c = C.stack_ref(mols)
    want = S.stack_ref(mols, want_c)
    assert (want['status'] == 0).all() and want['chiral'].sum() >= 6 and want['n_flat'].sum() >= 2 and want['n_stereo_bonds'].sum() >= 4
    got_c, got = S.stereo_mols(mols, DEV, with_canon=True)
    same(got, want, 'fixtures')
    got_c, got = molpack.to_host(got_c), molpack.to_host(got)
    assert all(np.array_equal(got_c[k], want_c[k], equal_nan=True) for k in want_c)
    assert S.summary(got, got_c) == S.summary(want, want_c) and np.array_equal(got['n_aut'], got_c['n_aut'])
    assert [S.iso_certificate(got_c, got, m) for m in range(len(mols))] == [S.iso_certificate(want_c, want, m) for m in range(len(mols))]
    assert C.smiles_mols(mols[:4], got_c, stereo=got)[:2] == ['C[C@H](F)Cl', 'C[C@@H](F)Cl']


def random_batch():
    mols = [random_3d(7000 + s) for s in range(64)]
    return mols, {m for m, x in enumerate(mols) if S.near_threshold(x)}


def test_a_random_batch_and_the_place_in_the_batch():
    mols, out = random_batch()
    assert len(out) / len(mols) <= 0.05, len(out)
    want = S.stack_ref(mols)
    assert want['n_centres'].sum() > 10 and want['n_stereo_bonds'].sum() > 5 and (want['n_aut'] > 1).sum() > 5
    same(S.stereo_mols(mols, DEV), want, 'random', skip=out)
    first = FIX['butane_pp']
    shuffled = [first] + mols[1:63] + [first]
    got = molpack.to_host(S.stereo_mols(shuffled, DEV))
    a, b = S.mol_result(got, 0), S.mol_result(got, 63)
    assert all(np.array_equal(a[k], b[k]) for k in a) and a['chiral'] == 1


def test_select_status_one_status_two_and_a_molecule_past_the_arrays():
    mols = [FIX['neopentane'], FIX['chfclbr'], FIX['butane_pp'], FIX['butene_z'], FIX['centre4']]
    p = molpack.pack_mols(mols, ELEMENTS, positions=True)
    cm = molpack.CompactMols.from_packed(molpack.to_device(p, DEV))
    N, E = int(p['n_atoms'].sum()), int(p['n_bonds'].sum())

    def dense(out):
        out = dict(out, **{k: out[k][:N] for k in S.ATOM_KEYS}, **{k: out[k][:E] for k in S.BOND_KEYS})
        return dict(out, n_atoms=cm.n_atoms, n_bonds=cm.n_bonds, atom_ptr=cm.atom_ptr, bond_ptr=cm.bond_ptr)
    plain = S.stack_ref(mols)

    def blank(ref, m, status):
        a0, b0, na, nb = (int(p[k][m]) for k in ('atom_ptr', 'bond_ptr', 'n_atoms', 'n_bonds'))
        for k in S.STAT_KEYS + ('stereo_hash', 'mirror_hash'):
            ref[k][m] = 0
        ref['status'][m] = status
        for k in S.ATOM_KEYS:
            ref[k][a0:a0 + na] = -1 if k == 'stereo_rank' else 0
        for k in S.BOND_KEYS:
            ref[k][b0:b0 + nb] = 0
        return ref
    copy = lambda: {k: v.copy() for k, v in plain.items()}
    # select: the masked molecule has status 0, stereo_rank -1 and zeros
    select = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32, device=DEV)
    c = C.launch(cm, select=select)
    same(dense(S.launch(cm, c, select=select)), blank(copy(), 2, 0), 'select')
    # canon gave up on neopentane (41 nodes) with a budget of 5: status 1 here, and the same from the restatement
    c5 = C.launch(cm, max_nodes=5)
    assert c5['status'].tolist() == [2, 0, 0, 0, 0]
    same(dense(S.launch(cm, c5)), blank(copy(), 0, 1), 'status 1')
    same(S.stack_ref(mols, C.stack_ref(mols, max_nodes=5)), blank(copy(), 0, 1), 'status 1 on the host')
    # stereo's own budget below canon's: status 2
    c = C.launch(cm)
    same(dense(S.launch(cm, c, max_nodes=5)), blank(copy(), 0, 2), 'status 2')
    same(S.stack_ref(mols, C.stack_ref(mols), max_nodes=5), blank(copy(), 0, 2), 'status 2 on the host')
    # a molecule whose extent leaves the arrays: status 0, and nothing of it is written (the arrays hold a sentinel)
    short = cm._replace(N_cap=N - 1)
    seven = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    o = dict({k: seven(N) for k in S.ATOM_KEYS}, **{k: seven(cm.Eh_stride) for k in S.BOND_KEYS}, mol_stats=seven(len(mols), 9))
    h = {k: torch.full((len(mols),), 7, dtype=torch.int64, device=DEV) for k in ('stereo_hash', 'mirror_hash')}
    ops, at = short.operands()
    rank, cstat = c['rank'].contiguous(), c['status'].contiguous()
    _lib.check(_lib.lib().mdx_mol_stereo(*ops, None, at(cm.atom_pos), None, at(rank), at(cstat), 51, 1, 0.1, 0.1, 1 << 16, at(o['canon_tetra']),
                                         at(o['canon_bond_stereo']), at(o['mirror_tetra']), at(o['mirror_bond_stereo']), at(o['stereo_rank']),
                                         at(o['atom_tetra']), at(o['bond_stereo']), at(o['mol_stats']), at(h['stereo_hash']), at(h['mirror_hash']),
                                         _lib.stream()))
    torch.cuda.synchronize()
    last = len(mols) - 1
    a0, b0 = int(p['atom_ptr'][last]), int(p['bond_ptr'][last])
    assert o['mol_stats'][last].tolist() == [0] * 9 and int(h['stereo_hash'][last]) == 0 and int(h['mirror_hash'][last]) == 0
    assert all(bool((o[k][a0:] == 7).all()) for k in S.ATOM_KEYS) and all(bool((o[k][b0:] == 7).all()) for k in S.BOND_KEYS)
    assert np.array_equal(o['stereo_rank'][:a0].cpu().numpy(), plain['stereo_rank'][:a0])
    assert np.array_equal(h['stereo_hash'][:last].cpu().numpy(), plain['stereo_hash'][:last])
    # no molecule
    got, ref = molpack.to_host(S.stereo_mols([], DEV)), S.empty()
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype for k in ref)
    with pytest.raises(ValueError, match='atom_pos'):
        S.stereo_mols([mol(2, [(0, 1)])], DEV)
    with pytest.raises(ValueError, match='flat_tol'):
        S.stereo_mols(mols[:1], DEV, flat_tol=1.5)
    with pytest.raises(ValueError, match='same pair'):
        S.stereo_mols([with_pos(mol(2, [(0, 1), (1, 0)]), np.zeros((2, 3)))], DEV)


def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.lib()
    ARG = 1
    mols = [FIX['chfclbr'], FIX['butene_e']]
    p = molpack.pack_mols(mols, ELEMENTS, positions=True)
    d = molpack.to_device(p, DEV)
    cm = molpack.CompactMols.from_packed(d)
    c = C.launch(cm)
    rank, cstat = c['rank'].contiguous(), c['status'].contiguous()
    N, E = 8, int(d['bond_index'].shape[1])
    seven = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    o = dict({k: seven(N) for k in S.ATOM_KEYS}, **{k: seven(E) for k in S.BOND_KEYS}, mol_stats=seven(2, 9),
             stereo_hash=torch.full((2,), 7, dtype=torch.int64, device=DEV), mirror_hash=torch.full((2,), 7, dtype=torch.int64, device=DEV))
    outs = ('canon_tetra', 'canon_bond_stereo', 'mirror_tetra', 'mirror_bond_stereo', 'stereo_rank', 'atom_tetra', 'bond_stereo', 'mol_stats',
            'stereo_hash', 'mirror_hash')

    def call(B=2, N_cap=N, stride=E, nodes=100, null=(), flat=0.1, bond=0.1):
        q = lambda name, t: None if name in null else _lib.ptr(t)
        return L.mdx_mol_stereo(B, q('atom_ptr', d['atom_ptr']), _lib.ptr(d['bond_ptr']), _lib.ptr(d['n_atoms']), _lib.ptr(d['n_bonds']),
                                q('atom_type', d['atom_type']), N_cap, _lib.ptr(d['bond_type']), q('bond_index', d['bond_index']), stride, None,
                                q('atom_pos', d['atom_pos']), None, q('rank', rank), q('canon_status', cstat), 51, 1, flat, bond, nodes,
                                *(q(k, o[k]) for k in outs), _lib.stream())
    for name in ('atom_ptr', 'atom_type', 'bond_index', 'atom_pos', 'rank', 'canon_status') + outs:
        assert call(null=(name,)) == ARG and b'null' in L.mdx_last_error(), name
    assert call(B=-1) == ARG and call(N_cap=-1) == ARG and call(stride=-1) == ARG
    assert call(nodes=0) == ARG and b'max_nodes' in L.mdx_last_error() and call(nodes=(1 << 20) + 1) == ARG
    assert call(flat=-0.5) == ARG and b'flat_tol' in L.mdx_last_error() and call(bond=float('nan')) == ARG and b'bond_tol' in L.mdx_last_error()
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in o.values())
    assert call() == 0
    torch.cuda.synchronize()
    ref = S.stack_ref(mols)
    assert o['mol_stats'].cpu().numpy().tolist() == np.stack([ref[k] for k in S.STAT_KEYS], 1).tolist()
    assert np.array_equal(o['canon_tetra'].cpu().numpy(), ref['canon_tetra']) and np.array_equal(o['mirror_hash'].cpu().numpy(), ref['mirror_hash'])


def test_atom_labels_on_both_sides():
    mols = [FIX['neopentane'], FIX['gem_dimethyl'], FIX['butane_meso'], FIX['dimethylcyclohexane_cis'], random_3d(7100, 8, 12)]
    labels = [np.arange(len(m['element'])) % 2 * 40000 + 3 for m in mols]
    want_c = C.stack_ref(mols, atom_label=labels)
    want, plain = S.stack_ref(mols, want_c, atom_label=labels), S.stack_ref(mols)
    assert not np.array_equal(want['n_aut'], plain['n_aut']) and not np.array_equal(want['n_stereogenic'], plain['n_stereogenic'])
    assert not S.near_threshold(mols[-1])
    same(S.stereo_mols(mols, DEV, atom_label=labels), want, 'labels')
    same(S.stereo_mols(mols, DEV), plain, 'no labels')


def test_stereo_batch_on_the_decode_layout_equals_stereo_mols_of_its_molecules():
    from .test_gpu_canon import _pred_of
    mols = [FIX['chfclbr'], FIX['butene_z'], FIX['butane_mm'], FIX['dimethylcyclohexane_trans'], FIX['neopentane'], random_3d(7200, 6, 10)]
    args = _pred_of(mols, masks=[2, 0, 1, 0, 3, 1])
    decoded = FEAT.decode_batch(*args)
    assert [len(d['element']) for d in decoded] == [len(m['element']) for m in mols]
    left_out = {m for m, d in enumerate(decoded) if S.near_threshold(d)}
    assert len(left_out) <= 1
    listed_c, listed = (molpack.to_host(r) for r in S.stereo_mols(decoded, DEV, with_canon=True))
    same(listed, S.stack_ref(decoded), 'stereo_mols of the decoded list', skip=left_out)
    select = torch.tensor([1, 1, 1, 0, 1, 1], device=DEV)
    for sel, masked in ((None, ()), (select, (3,))):
        res_c, res = FEAT.stereo_batch(*args, select=sel)
        res = molpack.to_host(res)
        for m in range(len(decoded)):
            zero = m in masked
            for k in S.MOL_KEYS:
                assert res[k][m] == (0 if zero else listed[k][m]), (k, m)
            a0, la, na = int(res['atom_ptr'][m]), int(listed['atom_ptr'][m]), len(decoded[m]['element'])
            b0, lb, nb = int(res['bond_ptr'][m]), int(listed['bond_ptr'][m]), int(listed['n_bonds'][m])
            for k in S.ATOM_KEYS:
                want = listed[k][la:la + na] * (not zero) - (zero and k == 'stereo_rank')
                assert np.array_equal(res[k][a0:a0 + na], want), (k, m)
            for k in S.BOND_KEYS:
                assert np.array_equal(res[k][b0:b0 + nb], listed[k][lb:lb + nb] * (not zero)), (k, m)
        assert molpack.to_host(res_c)['n_aut'].tolist() == [0 if m in masked else int(listed_c['n_aut'][m]) for m in range(len(decoded))]


def test_entry_point_writes_the_stereo_files(tmp_path):
    import json
    import os
    from .test_gpu_canon import _sample
    new = {'stereo.json', 'stereo.npz', 'canon.json', 'canon.npz', 'samples.smi', 'kekule.json', 'kekule.npz', 'samples_kekule.sdf'}
    d0, pool0 = _sample(tmp_path, 'abc', ['--largest_fragment', '0.2'])
    d1, pool = _sample(tmp_path, 'bca', ['--largest_fragment', '0.2', '--stereo', '--kekulize', '--canonical_max_nodes', '500', '--stereo_flat_tol', '0.05'])
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new) and new <= set(os.listdir(d1))
    assert len(pool['finished']) >= 2 and [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    canon_ref = C.stack_ref(pool['finished'], max_nodes=500)     # untrained weights decode to nearly complete graphs: mostly abandoned
    ref = S.stack_ref(pool['finished'], canon_ref, flat_tol=0.05, max_nodes=500)
    saved = molpack.load_npz(os.path.join(d1, 'stereo.npz'))
    left_out = {m for m, x in enumerate(pool['finished']) if S.near_threshold(x, flat_tol=0.05)}
    assert set(saved) == set(ref) and len(left_out) <= 1
    same(saved, ref, 'stereo.npz', skip=left_out)
    with open(os.path.join(d1, 'stereo.json')) as f:
        got = json.load(f)
    assert got['n_molecules'] == len(pool['finished']) and got['flat_tol'] == 0.05 and got['bond_tol'] == 0.1
    assert got['n_no_canon'] == int((canon_ref['status'] != 0).sum())
    if not left_out:
        assert [m['smiles'] for m in pool['finished']] == C.smiles_mols(pool['finished'], canon_ref, stereo=ref)
