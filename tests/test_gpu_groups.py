"""GPU tests of the substructure matcher (mdx_mol_groups through groups.groups_mols, groups.launch, FeaturizeMol.groups_batch and the
sampling entry point's --groups).  The oracle is the plain Python restatement ``groups_ref``; every output is an integer that the
definitions make unique, so every comparison is exact."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import groups as G
from moldiff_amd.harness import placeholder_from_sizes
from moldiff_amd.postprocess import FeaturizeMol

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)


def mol(ele, bonds):
    ele = [6] * ele if isinstance(ele, int) else ele
    bonds = [tuple(b) + (1,) * (3 - len(b)) for b in bonds]
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
            'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def ring(n, first=0, t=1):
    return [(first + k, first + (k + 1) % n, t) for k in range(n)]


def ladder(rungs):
    return mol(2 * rungs, [(k, k + 1) for k in range(rungs - 1)] + [(rungs + k, rungs + k + 1) for k in range(rungs - 1)] +
               [(k, rungs + k) for k in range(rungs)])


def random_mol(seed, n, extra=0.3):
    """connected: a random spanning tree plus extra * n further bonds; the first 7 atoms and 4 bonds carry every element and type"""
    g = np.random.default_rng(seed)
    bonds = {(int(g.integers(0, k)), k) for k in range(1, n)}
    while len(bonds) < n - 1 + int(extra * n):
        i, j = sorted(int(x) for x in g.choice(n, 2, replace=False))
        bonds.add((i, j))
    ele = g.choice(ELEMENTS, n, p=[0.5, 0.15, 0.15, 0.05, 0.05, 0.05, 0.05])
    ele[:7] = ELEMENTS[:n]
    bt = g.choice([1, 1, 2, 3, 4], len(bonds))
    bt[:4] = [1, 2, 3, 4][:len(bonds)]
    return mol(ele, [(i, j, int(t)) for (i, j), t in zip(sorted(bonds), bt)])


def relabelled(m, seed):
    g = np.random.default_rng(seed)
    n, nb = len(m['element']), m['bond_index'].shape[1] // 2
    new = g.permutation(n)
    ele = np.empty(n, dtype=np.int64)
    ele[new] = m['element']
    order = g.permutation(nb)
    idx = new[m['bond_index'][:, :nb]][:, order]
    bt = m['bond_type'][:nb][order]
    return {'element': ele, 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}, new


def wild(name, na, bonds):
    return {'name': name, 'atoms': [{} for _ in range(na)], 'bonds': [[i, j, '*'] for i, j in bonds]}


def wild_path(k):
    return wild(f'path{k}', k, [(i, i + 1) for i in range(k - 1)])


CUBE = [(k, (k + 1) % 4) for k in range(4)] + [(4 + k, 4 + (k + 1) % 4) for k in range(4)] + [(k, k + 4) for k in range(4)]
# P = 32: the default set, a pattern of 8 atoms and 12 bonds, a single-atom pattern, shapes with closing bonds, every kind of constraint
EXTRA = [wild('cube', 8, CUBE), wild('atom', 1, []), wild_path(2), wild_path(4), wild_path(6), wild('triangle', 3, [(0, 1), (1, 2), (0, 2)]),
         wild('square', 4, [(0, 1), (1, 2), (2, 3), (3, 0)]), wild('k4', 4, list(itertools.combinations(range(4), 2))),
         {'name': 'star', 'atoms': [{'deg': [3, 4, 7]}, {}, {}, {}], 'bonds': [[0, 1, '*'], [0, 2, '*'], [0, 3, '*']]},
         {'name': 'ring_atom_5_6', 'atoms': [{'ring': [5, 6]}]},
         {'name': 'bridge', 'atoms': [{'ring': 'ring'}, {'ring': 'ring'}], 'bonds': [[0, 1, '*', 'none']]},
         {'name': 'multiple', 'atoms': [{'h': [0, 1]}, {'elem': ['C', 'N', 'P', 'S']}], 'bonds': [[0, 1, [2, 3]]]},
         {'name': 'unordered', 'atoms': [{'elem': ['C']}, {}, {'arom': True}, {}], 'bonds': [[2, 3, '*'], [1, 2, [4]], [0, 1, '*', 'ring']]}]
BIG = G.PatternSet(G.PatternSet.default().patterns + G.PatternSet(EXTRA).patterns)

ACETAMIDE = mol([6, 6, 8, 7], [(0, 1), (1, 2, 2), (1, 3)])
METHYL_ACETATE = mol([6, 6, 8, 8, 6], [(0, 1), (1, 2, 2), (1, 3), (3, 4)])
CHLOROPYRIDINE = mol([7, 6, 6, 6, 6, 6, 17], ring(6, t=4) + [(3, 6)])
RANDOM = random_mol(41, 14)
K12 = mol(12, list(itertools.combinations(range(12), 2)))
BATCH = [ACETAMIDE,                                                                   # 0
         METHYL_ACETATE,                                                              # 1
         mol(6, ring(6, t=4)),                                                        # 2 benzene
         mol([7, 6, 6, 6, 6, 6], ring(6, t=4)),                                       # 3 pyridine
         mol(3, ring(3)),                                                             # 4 a triangle
         mol(0, []),                                                                  # 5 no atom
         mol([6, 6, 6, 8, 7, 7], ring(3) + [(4, 5, 3)]),                              # 6 two fragments and a lone atom
         CHLOROPYRIDINE,                                                              # 7
         mol([7, 6, 6, 6, 6, 6, 17], [(0, 7, 1), (2, 2, 3)] + ring(6, t=4) + [(3, 6)] + [(-1, 3, 2)]),   # 8 = 7 with three ignored bonds
         RANDOM,                                                                      # 9 masked out in the second launch
         relabelled(RANDOM, 5)[0],                                                    # 10 a relabelled copy of 9
         random_mol(40, 40),                                                          # 11 every element and bond type
         mol(8, CUBE),                                                                # 12 cubane: the 8-atom, 12-bond pattern occurs
         mol(10, ring(10, t=4) + [(0, 5, 4)]),                                        # 13 naphthalene
         mol([6, 16, 8, 8, 7, 6, 8], [(0, 1), (1, 2, 2), (1, 3, 2), (1, 4), (4, 5), (5, 6, 2)]),   # 14 sulfonamide and amide
         random_mol(42, 256, extra=0.1),                                              # 15 the largest molecule measured
         mol(257, [(k, k + 1) for k in range(256)]),                                  # 16 one atom too many
         mol(200, [(k, k + 1) for k in range(199)] + [(k, k + 2) for k in range(198)] + [(k, k + 3) for k in range(116)]),   # 17 513 bonds
         ladder(66),                                                                  # 18 65 rings: the ring data are not measured
         ladder(33),                                                                  # 19
         K12,                                                                         # 20 over the budget for the long wildcards
         mol([6, 8], [(0, 1, 7)]),                                                    # 21 a bond type outside 1 .. 4
         CHLOROPYRIDINE]                                                              # 22 = 7, elsewhere
MASKED = 9


@pytest.fixture(scope='module')
def want():
    """groups_ref of every molecule of BATCH with the 32 patterns, computed once"""
    return G.stack_ref(BATCH, BIG)


def same(got, ref, what, keys=None):
    got = molpack.to_host(got)
    for k in keys or ref:
        if k == 'names':
            assert got[k].tolist() == ref[k].tolist(), what
            continue
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        bad = np.flatnonzero((got[k] != ref[k]).reshape(len(ref[k]), -1).any(1)) if ref[k].size else []
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:4]], ref[k][bad[:4]])


def test_one_launch_over_the_whole_list_equals_the_restatement(want):
    assert len(BIG) == 32 and BIG.needs_rings
    cube, atom = BIG.names.index('cube'), BIG.names.index('atom')
    assert (len(BIG.patterns[cube].atoms), len(BIG.patterns[cube].bonds), len(BIG.patterns[atom].atoms)) == (8, 12, 1)
    assert want['status'].tolist() == [0] * 16 + [1, 1, 2] + [0] * 4
    assert want['n_embed'][12, cube] == 48 and want['aut'][cube] == 48 and want['n_embed'][15, atom] == 256
    assert sorted(set(BATCH[11]['element'])) == list(ELEMENTS) and sorted(set(BATCH[11]['bond_type'].tolist())) == [1, 2, 3, 4]
    over = {n for n, s in zip(BIG.names, want['pat_status'][20]) if s == 3}
    assert over == {'cube', 'path6'} and not want['pat_status'][:20].any()          # the clique, at the default budget
    nm = dict(zip(BIG.names, G.n_match(want)[14].tolist()))
    assert (nm['sulfonamide'], nm['amide'], nm['carbonyl'], nm['amine_1h']) == (1, 1, 1, 1)
    got = G.groups_mols(BATCH, DEV, BIG)
    same(got, want, 'groups_mols')
    g = molpack.to_host(got)
    for k in G.MOL_KEYS:                                  # one molecule at three places, once with ignored bonds around it
        assert np.array_equal(g[k][7], g[k][22]) and np.array_equal(g[k][7], g[k][8]), k
    ptr = g['atom_ptr']
    hit = lambda m: g['atom_hit'][ptr[m]:ptr[m] + g['n_atoms'][m]]
    assert np.array_equal(hit(7), hit(22)) and np.array_equal(hit(7), hit(8)) and hit(7).any()
    for k in G.MOL_KEYS:                                  # a relabelled copy: the same counts, atom_hit permuted
        assert np.array_equal(g[k][9], g[k][10]), k
    assert np.array_equal(hit(9), hit(10)[relabelled(RANDOM, 5)[1]]) and hit(9).any()
    # the same arrays with a mask: the masked molecule has status 0 and zeros everywhere, its slots included; the others are unchanged
    p = molpack.pack_mols(BATCH, ELEMENTS)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    select = torch.ones(len(BATCH), dtype=torch.int32, device=DEV)
    select[MASKED] = 0
    N = int(p['n_atoms'].sum())
    out = G.launch(molpack.CompactMols.from_packed(d), BIG, select=select)
    ref = {k: v.copy() for k, v in want.items()}
    for k in G.MOL_KEYS:
        ref[k][MASKED] = 0
    a0 = int(p['atom_ptr'][MASKED])
    ref['atom_hit'][a0:a0 + int(p['n_atoms'][MASKED])] = 0
    assert want['n_embed'][MASKED].any()
    same(out, ref, 'select', keys=[k for k in G.MOL_KEYS + G.SLOT_KEYS if k != 'n_atoms'])
    # a second call gives the same bytes
    again = molpack.to_host(G.groups_mols(BATCH, DEV, BIG))
    assert all(g[k].tobytes() == again[k].tobytes() for k in g)


def test_budget_flags_exactly_the_pattern_that_exceeds_it():
    pset = G.PatternSet([wild_path(2), wild_path(3), wild_path(4), wild_path(5)])
    count = 1 + 11 * (1 + 11 + 110 + 990)                 # one start atom of the 12-clique against the 5-atom path, from the definition
    mols = [K12, BATCH[4], RANDOM]
    for steps, flagged in ((count - 1, [0, 0, 0, 3]), (count, [0, 0, 0, 0])):
        ref = G.stack_ref(mols, pset, max_steps=steps)
        assert ref['pat_status'].tolist() == [flagged, [0] * 4, [0] * 4]
        same(G.groups_mols(mols, DEV, pset, max_steps=steps), ref, ('budget', steps))
    assert ref['n_embed'][0].tolist() == [132, 1320, 11880, 95040] and ref['steps'][0, 3] == 12 * count
    # the smallest budget: a start atom with a neighbour is over it
    same(G.groups_mols(mols, DEV, pset, max_steps=1), G.stack_ref(mols, pset, max_steps=1), 'budget 1')


def test_without_ring_constraints_no_ring_data_are_needed():
    pset = G.PatternSet([p for p in BIG.patterns if not p.needs_rings])
    assert 20 < len(pset) < 32 and not pset.needs_rings
    mols = BATCH[:15] + [BATCH[18], BATCH[21]]
    ref = G.stack_ref(mols, pset)
    assert ref['status'].tolist() == [0] * 17                                       # the ladder of 65 rings is measured here
    same(G.groups_mols(mols, DEV, pset), ref, 'no ring data')
    other = {z: v for z, v in zip(ELEMENTS, (3, 5, 1, 1, 5, 6, 2))}                 # another table of normal valences
    ref2 = G.stack_ref(mols, pset, normal_valence=other)
    assert not np.array_equal(ref2['n_embed'], ref['n_embed'])
    same(G.groups_mols(mols, DEV, pset, normal_valence=other), ref2, 'normal valences')


def test_no_molecule_and_host_side_refusals():
    got = molpack.to_host(G.groups_mols([], DEV, BIG))
    ref = G.empty(BIG)
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape for k in ref)
    with pytest.raises(ValueError, match='same pair'):
        G.groups_mols([BATCH[1], mol(3, [(0, 1), (1, 2), (1, 0)])], DEV, BIG)
    with pytest.raises(ValueError, match='element'):
        G.groups_mols([mol([6, 5], [(0, 1)])], DEV, BIG)
    with pytest.raises(ValueError, match='max_steps'):
        G.groups_mols(BATCH[:2], DEV, BIG, max_steps=(1 << 20) + 1)


def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.lib()
    ARG = 1
    pset = G.PatternSet([wild_path(3), wild('atom', 1, [])])
    p = molpack.pack_mols(BATCH[:5], ELEMENTS)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    N, E = int(p['n_atoms'].sum()), int(d['bond_index'].shape[1])
    seven = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    o = {'n_embed': seven(5, 2), 'n_anchor': seven(5, 2), 'steps': seven(5, 2), 'pat_status': seven(5, 2), 'status': seven(5),
         'atom_hit': seven(N)}
    ws = torch.zeros(L.mdx_mol_groups_ws_bytes(32), dtype=torch.uint8, device=DEV)
    nv = pset.valence_table()
    ringed = G.PatternSet([{'name': 'r', 'atoms': [{'ring': 'ring'}]}]).pack()
    unordered = pset.pack().copy()
    unordered[0, 42:50] = [1, 2, 30, 0x7f, 0, 2, 30, 0x7f]                          # bonds 1-2 and 0-2: atom 1 has no earlier neighbour
    bad_mask = pset.pack().copy()
    bad_mask[0, 2] = 1 << 7                                                         # class 7 of 7 elements

    def call(B=5, N_cap=N, stride=E, ne=7, nbt=4, table=None, P=2, steps=100, null=None, rings=(None, None, None), ws_bytes=None, valence=nv):
        table = pset.pack() if table is None else table
        q = lambda name, t: None if null == name else _lib.ptr(t)
        return L.mdx_mol_groups(B, q('atom_ptr', d['atom_ptr']), _lib.ptr(d['bond_ptr']), _lib.ptr(d['n_atoms']), _lib.ptr(d['n_bonds']),
                                _lib.ptr(d['atom_type']), N_cap, _lib.ptr(d['bond_type']), _lib.ptr(d['bond_index']), stride, None, ne, nbt,
                                None if null == 'normal_valence' else valence.ctypes.data, None if null == 'patterns' else table.ctypes.data,
                                P, steps, *rings, *(q(k, o[k]) for k in ('n_embed', 'n_anchor', 'steps', 'pat_status', 'status', 'atom_hit')),
                                None if null == 'ws' else _lib.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _lib.stream())
    assert call(P=0) == ARG and b'1 .. 32 patterns' in L.mdx_last_error()
    assert call(P=33) == ARG
    assert call(steps=0) == ARG and b'max_steps' in L.mdx_last_error()
    assert call(steps=(1 << 20) + 1) == ARG
    assert call(null='atom_ptr') == ARG and b'null' in L.mdx_last_error()
    assert call(null='status') == ARG and call(null='atom_hit') == ARG and call(null='patterns') == ARG and call(null='ws') == ARG
    assert call(null='normal_valence') == ARG
    assert call(table=unordered) == ARG and b'not ordered' in L.mdx_last_error()
    assert call(table=bad_mask) == ARG and b'elem_mask' in L.mdx_last_error()
    assert call(table=ringed, P=1) == ARG and b'no ring data' in L.mdx_last_error()
    assert call(rings=(_lib.ptr(o['atom_hit']), None, None)) == ARG and b'all three' in L.mdx_last_error()
    assert call(B=-1) == ARG and call(N_cap=-1) == ARG and call(stride=-1) == ARG and call(ne=0) == ARG and call(ne=33) == ARG
    assert call(nbt=0) == ARG and call(nbt=17) == ARG and call(ws_bytes=128 * 3 - 1) == ARG
    assert call(valence=np.full(7, 65, dtype=np.int32)) == ARG
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in o.values())
    assert call(B=0) == 0                                              # no molecule: accepted, nothing written
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in o.values())
    table = pset.pack()
    assert call(table=table) == 0                                      # and the same operands, unbroken, are accepted;
    table[:] = -1                                                      # the caller's table is free once the call has returned
    torch.cuda.synchronize()
    ref = G.stack_ref(BATCH[:5], pset, max_steps=100)
    for k in ('n_embed', 'n_anchor', 'steps', 'pat_status', 'status', 'atom_hit'):
        assert o[k].cpu().numpy().tolist() == ref[k].tolist(), k


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
        pn.append((10.0 * np.eye(8)[ids]).astype(np.float32)), pp.append(np.zeros((n, 3), dtype=np.float32))
        ph.append((10.0 * np.eye(6)[T[iu, ju]]).astype(np.float32).reshape(-1, 6))
    ph_ = placeholder_from_sizes([len(x) for x in pn], DEV)
    pred = [torch.from_numpy(np.concatenate(x)).to(DEV) for x in (pn, pp, ph)]
    return (pred, ph_['batch_node'], ph_['halfedge_index'], ph_['batch_halfedge'], len(mols))


def test_groups_batch_on_the_decode_layout_equals_groups_mols_of_its_molecules():
    mols = [BATCH[5], BATCH[6], BATCH[13], BATCH[12], BATCH[11], BATCH[9], BATCH[14], BATCH[0]]
    args = _pred_of(mols, masks=[2, 1, 0, 0, 3, 0, 1, 2])
    decoded = FEAT.decode_batch(*args)
    assert [len(d['element']) for d in decoded] == [0, 6, 10, 8, 40, 14, 7, 4]
    listed, ref = molpack.to_host(G.groups_mols(decoded, DEV, BIG)), G.stack_ref(decoded, BIG)
    same(listed, ref, 'groups_mols of the decoded list')
    assert ref['n_embed'].any(1).tolist() == [False] + [True] * 7

    def check(got, masked=()):
        got = molpack.to_host(got)
        assert got['names'].tolist() == BIG.names and np.array_equal(got['aut'], ref['aut'])
        for m in range(len(mols)):
            a0, la, na = int(got['atom_ptr'][m]), int(listed['atom_ptr'][m]), len(decoded[m]['element'])
            zero = m in masked
            for k in G.MOL_KEYS:
                assert np.array_equal(got[k][m], np.zeros_like(listed[k][m]) if zero else listed[k][m]), (k, m)
            assert np.array_equal(got['atom_hit'][a0:a0 + na], listed['atom_hit'][la:la + na] * (not zero)), m
    check(FEAT.groups_batch(*args, BIG))
    check(FEAT.groups_batch(*args, BIG, select=torch.tensor([1, 1, 1, 1, 1, 0, 1, 1], device=DEV)), masked=(5,))
    got = molpack.to_host(FEAT.groups_batch(*args, G.PatternSet([wild_path(4)]), max_steps=30))
    want = G.stack_ref(decoded, G.PatternSet([wild_path(4)]), max_steps=30)
    assert 0 < (want['pat_status'] == 3).sum() < 8 and np.array_equal(got['pat_status'], want['pat_status'])
    assert np.array_equal(got['n_embed'], want['n_embed'])
    with pytest.raises(ValueError, match='another featuriser'):
        FEAT.groups_batch(*args, G.PatternSet([wild_path(2)], atomic_numbers=(6, 7, 8)))


def _same_numbers(got, ref):
    if isinstance(ref, dict):
        assert set(got) == set(ref)
        for k in ref:
            _same_numbers(got[k], ref[k])
    elif isinstance(ref, list):
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            _same_numbers(a, b)
    else:
        assert got == ref or (np.isnan(got) and np.isnan(ref)), (got, ref)


def _sample(tmp_path, name, extra):
    from moldiff_amd import sample_drug3d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log_dir = sample_drug3d.main(['--config', os.path.join(root, 'configs', 'sample_MolDiff_simple.yml'), '--outdir', str(tmp_path / name),
                                  '--device', DEV, '--recipe-weights', '--num_steps', '2', '--num_mols', '6', '--batch_size', '8'] + extra)
    return log_dir, torch.load(os.path.join(log_dir, 'samples_all.pt'), weights_only=False)


def test_entry_point_writes_groups_of_the_finished_molecules(tmp_path):
    # the seed is sample.seed + sum(ord(outdir)): the two directory names are permutations of each other, so both runs sample the same
    # molecules; the first run is without the option
    d0, pool0 = _sample(tmp_path, 'ab', ['--largest_fragment', '0.2'])
    d1, pool = _sample(tmp_path, 'ba', ['--largest_fragment', '0.2', '--groups'])
    assert len(pool['finished']) >= 2 and [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    new = {'groups.json', 'groups.npz'}
    assert not new & set(os.listdir(d0)) and sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new)
    for d_a, d_b in ((d0, d1), (d0 + '_SDF', d1 + '_SDF')):          # without the option nothing changes: every other file is the same bytes
        assert sorted(os.listdir(d_a)) == sorted(f for f in os.listdir(d_b) if f not in new)
        for f in sorted(os.listdir(d_a)):
            if f == 'samples_all.pt':                                 # a pickle of the same molecules: compared as molecules
                continue
            with open(os.path.join(d_a, f), 'rb') as a, open(os.path.join(d_b, f), 'rb') as b:
                assert a.read() == b.read(), f
    for a, b in zip(pool0['finished'] + pool0['failed'], pool['finished'] + pool['failed']):
        assert set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    ref = G.stack_ref(pool['finished'])
    saved = molpack.load_npz(os.path.join(d1, 'groups.npz'))
    assert set(saved) == set(ref) and all(np.array_equal(saved[k], ref[k]) and saved[k].dtype == ref[k].dtype for k in ref)
    with open(os.path.join(d1, 'groups.json')) as f:
        got = json.load(f)
    print('finished', len(pool['finished']), got['n_measured'], got['n_skipped'])
    _same_numbers(got, G.summary(ref))
    # untrained weights bond nearly every pair of atoms: most of these molecules are beyond the caps and are counted as skipped
    assert got['n_measured'] + sum(got['n_skipped'].values()) == len(pool['finished'])
