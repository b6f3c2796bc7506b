"""Host tests of moldiff_amd/rings.py: ``rings_ref`` against literal answers and against a brute-force oracle written here (every simple
cycle, rank by length), its invariances, caps and status codes, ``summary`` / ``compare`` and the command line with --ref.  No GPU."""
import itertools
import json

import numpy as np
import pytest
import torch

from moldiff_amd import molpack
from moldiff_amd import rings as R

ELEMENTS = (6, 7, 8, 9, 15, 16, 17)


def mol(ele, bonds):
    """ele: atomic numbers or an atom count (all carbon); bonds: (i, j) or (i, j, type), type 1 by default"""
    ele = [6] * ele if isinstance(ele, int) else ele
    bonds = [tuple(b) + (1,) * (3 - len(b)) for b in bonds]
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
            'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def ring(n, first=0, t=1):
    return [(first + k, first + (k + 1) % n, t) for k in range(n)]


def ladder(rungs):
    """2 x rungs atoms: rungs - 1 four-rings"""
    return mol(2 * rungs, [(k, k + 1) for k in range(rungs - 1)] + [(rungs + k, rungs + k + 1) for k in range(rungs - 1)] +
               [(k, rungs + k) for k in range(rungs)])


CHAIN = mol(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
BENZENE = mol(6, ring(6, t=4))
NAPHTHALENE = mol(10, ring(10, t=4) + [(0, 5, 4)])
NORBORNANE = mol(7, ring(6) + [(0, 6), (6, 3)])
CUBANE = mol(8, ring(4) + ring(4, 4) + [(k, k + 4) for k in range(4)])
SPIRO = mol(5, [(0, 1), (1, 2), (2, 0), (0, 3), (3, 4), (4, 0)])
BRIDGED = mol(12, ring(6, t=4) + ring(6, 6, t=4) + [(0, 6, 1)])            # biphenyl: bond 12 joins the two rings
TEN_RING = mol(10, ring(10))
TWO_FRAGMENTS = mol([6, 6, 6, 8, 7, 7], ring(3) + [(4, 5, 3)])             # a 3-ring, a lone atom, a triple bond
EMPTY = mol(0, [])


def sizes(res):
    """the ring sizes a ring_hist stands for, the last bin as its lower end"""
    return [3 + k for k, c in enumerate(res['ring_hist']) for _ in range(c)]


def consistent(res):
    assert res['ring_hist'].sum() == res['n_rings'] and res['n_ring_bonds'] == (res['bond_ring_min'] > 0).sum()
    assert res['n_ring_atoms'] == (res['atom_ring_min'] > 0).sum()


def test_literal_molecules():
    want = [(CHAIN, []), (BENZENE, [6]), (NAPHTHALENE, [6, 6]), (NORBORNANE, [5, 5]), (CUBANE, [4] * 5), (SPIRO, [3, 3]),
            (BRIDGED, [6, 6]), (TEN_RING, [9]), (TWO_FRAGMENTS, [3]), (EMPTY, [])]
    for m, s in want:
        res = R.rings_ref(m)
        assert res['status'] == 0 and sizes(res) == s and res['n_rings'] == len(s), (s, res)
        consistent(res)
    r = R.rings_ref(CHAIN)
    assert r['n_ring_atoms'] == 0 and r['n_rotatable'] == 2 and not r['bond_ring_min'].any() and r['elem_count'].tolist() == [5, 0, 0, 0, 0, 0, 0]
    assert r['bond_count'].tolist() == [4, 0, 0, 0]
    r = R.rings_ref(BENZENE)
    assert r['n_ring_atoms'] == 6 and r['n_ring_bonds'] == 6 and r['n_rotatable'] == 0 and r['bond_ring_min'].tolist() == [6] * 6
    assert r['bond_count'].tolist() == [0, 0, 0, 6] and r['atom_ring_min'].tolist() == [6] * 6
    r = R.rings_ref(NAPHTHALENE)
    assert r['n_ring_atoms'] == 10 and r['n_ring_bonds'] == 11
    r = R.rings_ref(NORBORNANE)
    assert r['bond_ring_min'].tolist() == [5] * 8 and r['n_ring_atoms'] == 7           # the 6-ring is the sum of the two 5-rings
    r = R.rings_ref(CUBANE)
    assert r['n_rings'] == 5 and r['ring_hist'].tolist() == [0, 5, 0, 0, 0, 0, 0] and r['bond_ring_min'].tolist() == [4] * 12
    r = R.rings_ref(SPIRO)
    assert r['atom_ring_min'].tolist() == [3] * 5 and r['n_rotatable'] == 0
    r = R.rings_ref(BRIDGED)
    assert r['bond_ring_min'].tolist() == [6] * 12 + [0] and r['n_ring_bonds'] == 12 and r['n_ring_atoms'] == 12 and r['n_rotatable'] == 1
    r = R.rings_ref(TEN_RING)
    assert r['ring_hist'].tolist() == [0] * 6 + [1] and r['bond_ring_min'].tolist() == [10] * 10
    assert R.rings_ref(TEN_RING, ring_bins=8)['ring_hist'].tolist() == [0] * 7 + [1]
    assert R.rings_ref(TEN_RING, ring_bins=1)['ring_hist'].tolist() == [1]
    r = R.rings_ref(TWO_FRAGMENTS)
    assert r['n_rings'] == 1 and r['n_ring_atoms'] == 3 and r['elem_count'].tolist() == [3, 2, 1, 0, 0, 0, 0]
    assert r['bond_count'].tolist() == [3, 0, 1, 0] and r['atom_ring_min'].tolist() == [3, 3, 3, 0, 0, 0]
    r = R.rings_ref(EMPTY)
    assert r['n_atoms'] == 0 and r['n_rings'] == 0 and len(r['bond_ring_min']) == 0 and len(r['atom_ring_min']) == 0


def test_rotatable_rule():
    # C-C-C-C: only the middle bond has two atoms of degree >= 2
    assert R.rings_ref(mol(4, [(0, 1), (1, 2), (2, 3)]))['n_rotatable'] == 1
    # a double bond in the middle is not rotatable; a triple bond at either end of a single bond blocks it
    assert R.rings_ref(mol(4, [(0, 1), (1, 2, 2), (2, 3)]))['n_rotatable'] == 0
    assert R.rings_ref(mol(5, [(0, 1, 3), (1, 2), (2, 3), (3, 4)]))['n_rotatable'] == 1          # 1-2 blocked, 2-3 counts
    # no amide exclusion: C-C(=O)-N-C counts both C-C(=O)... the C-N bond has degrees 3 and 2
    assert R.rings_ref(mol([6, 6, 8, 7, 6], [(0, 1), (1, 2, 2), (1, 3), (3, 4)]))['n_rotatable'] == 1
    # ignored bonds do not add to a degree
    assert R.rings_ref(mol(4, [(0, 1), (1, 2), (2, 3), (0, 0), (3, 9)]))['n_rotatable'] == 1


def relabelled(m, seed):
    g = np.random.default_rng(seed)
    n, nb = len(m['element']), m['bond_index'].shape[1] // 2
    new = g.permutation(n)
    ele = np.empty(n, dtype=np.int64)
    ele[new] = m['element']
    order = g.permutation(nb)
    idx = new[m['bond_index'][:, :nb]][:, order]
    idx = np.where(g.random(nb) < 0.5, idx[::-1], idx)
    bt = m['bond_type'][:nb][order]
    return {'element': ele, 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}, new, order


def random_graph(g, n, p):
    pairs = [pq for pq in itertools.combinations(range(n), 2) if g.random() < p]
    return mol(g.choice(ELEMENTS, n).tolist(), [(i, j, int(g.integers(1, 5))) for i, j in pairs])


def test_invariant_under_relabelling_reordering_and_flipping():
    g = np.random.default_rng(5)
    for k, m in enumerate([NAPHTHALENE, CUBANE, BRIDGED, TWO_FRAGMENTS] + [random_graph(g, 9, 0.35) for _ in range(20)]):
        a = R.rings_ref(m)
        m2, new, order = relabelled(m, 100 + k)
        b = R.rings_ref(m2)
        for key in R.MOL_KEYS:
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a['bond_ring_min'][order], b['bond_ring_min']) and np.array_equal(a['atom_ring_min'], b['atom_ring_min'][new])


def brute_force(n, bonds):
    """every simple cycle of a small graph as a bit set of its bonds -> (ring sizes of a minimum cycle basis: the rank gained per
    length, smallest cycle through every bond)"""
    adj = {a: [] for a in range(n)}
    for e, (x, y) in enumerate(bonds):
        adj[x].append((y, e))
        adj[y].append((x, e))
    cycles = set()

    def walk(start, a, used_atoms, used_bonds):
        for b, e in adj[a]:
            if used_bonds >> e & 1:
                continue
            if b == start and len(used_atoms) >= 3:
                cycles.add(used_bonds | 1 << e)
            elif b > start and b not in used_atoms:
                walk(start, b, used_atoms | {b}, used_bonds | 1 << e)
    for s in range(n):
        walk(s, s, {s}, 0)
    got, basis = [], {}
    for c in sorted(cycles, key=lambda c: bin(c).count('1')):
        v = c
        while v:
            hb = v.bit_length() - 1
            if hb not in basis:
                basis[hb] = v
                got.append(bin(c).count('1'))
                break
            v ^= basis[hb]
    smallest = [min([bin(c).count('1') for c in cycles if c >> e & 1], default=0) for e in range(len(bonds))]
    return got, smallest


def test_agrees_with_brute_force_on_random_graphs():
    g = np.random.default_rng(11)
    planted = [mol(7, ring(7)), mol(8, ring(8) + [(0, 3)]), mol(9, ring(9) + [(0, 4)]), mol(9, ring(9) + [(0, 3), (4, 8)]),
               mol(9, ring(4) + ring(5, 4) + [(0, 4)]), mol(8, ring(8) + [(0, 4), (2, 6)])]
    graphs = planted + [random_graph(g, int(g.integers(3, 10)), float(g.choice([0.15, 0.25, 0.4, 0.6]))) for _ in range(300)]
    seen_sizes = set()
    for k, m in enumerate(graphs):
        n, nb = len(m['element']), m['bond_index'].shape[1] // 2
        bonds = [tuple(int(v) for v in m['bond_index'][:, e]) for e in range(nb)]
        want_sizes, want_min = brute_force(n, bonds)
        res = R.rings_ref(m, ring_bins=8)
        consistent(res)
        assert res['status'] == 0 and sizes(res) == want_sizes, (k, bonds, sizes(res), want_sizes)
        assert res['bond_ring_min'].tolist() == want_min, (k, bonds)
        seen_sizes.update(want_sizes)
    assert seen_sizes >= {3, 4, 5, 6, 7}
    # the complete graph on 9 atoms has 28 independent rings, all triangles
    assert sizes(R.rings_ref(random_graph(g, 9, 2.0))) == [3] * 28


def test_caps_and_status_codes():
    r = R.rings_ref(ladder(33))
    assert r['status'] == 0 and r['n_rings'] == 32 and r['ring_hist'].tolist() == [0, 32, 0, 0, 0, 0, 0]
    r = R.rings_ref(ladder(65))
    assert r['status'] == 0 and r['n_rings'] == 64 and r['ring_hist'].tolist() == [0, 64, 0, 0, 0, 0, 0] and r['n_ring_atoms'] == 130
    r = R.rings_ref(ladder(66))
    assert r['status'] == 2 and r['n_atoms'] == 132
    assert all(not np.any(r[k]) for k in R.MOL_KEYS + R.SLOT_KEYS if k not in ('status', 'n_atoms'))
    assert R.rings_ref(mol(256, [(k, k + 1) for k in range(255)]))['status'] == 0
    r = R.rings_ref(mol(257, [(k, k + 1) for k in range(256)]))
    assert r['status'] == 1 and not r['elem_count'].any() and not r['bond_count'].any() and r['n_rotatable'] == 0
    assert R.rings_ref(mol(200, [(k, k + 1) for k in range(199)] + [(k, k + 2) for k in range(198)] +
                           [(k, k + 3) for k in range(116)]))['status'] == 1                         # 513 bonds
    with pytest.raises(ValueError, match='same pair'):
        R.rings_ref(mol(3, [(0, 1), (1, 2), (1, 0)]))
    with pytest.raises(ValueError, match='element'):
        R.rings_ref(mol([6, 5], [(0, 1)]))
    with pytest.raises(ValueError, match='ring_bins'):
        R.rings_ref(BENZENE, ring_bins=65)


def test_summary_and_compare_on_hand_made_inputs():
    res = R.stack_ref([BENZENE, CHAIN, TWO_FRAGMENTS, ladder(66), EMPTY])
    assert res['status'].tolist() == [0, 0, 0, 2, 0] and res['atom_ptr'].tolist() == [0, 6, 11, 17, 149]
    assert len(res['bond_ring_min']) == 6 + 4 + 4 + 196 and len(res['atom_ring_min']) == 149
    s = R.summary(res)
    assert s['n_measured'] == 4 and s['n_skipped'] == {'too_large': 0, 'too_many_rings': 1}
    assert s['mean_rings'] == 2 / 4 and s['ring_size']['counts'] == [1, 0, 0, 1, 0, 0, 0] and s['ring_size']['fractions'][0] == 0.5
    assert s['element']['counts'] == [14, 2, 1, 0, 0, 0, 0] and s['bond_type']['counts'] == [7, 0, 1, 6]
    assert s['ring_atom_fraction'] == 9 / 17 and s['mean_rotatable'] == 2 / 4
    none = R.summary(R.empty())
    assert none['n_measured'] == 0 and np.isnan(none['mean_rings']) and np.isnan(none['ring_atom_fraction'])
    other = R.stack_ref([CUBANE, SPIRO])
    assert R.compare(res, res) == {'ring_size': 0.0, 'element': 0.0, 'bond_type': 0.0}
    c = R.compare(res, other)
    assert 0 < c['ring_size'] <= 1 and 0 < c['element'] < 1 and 0 < c['bond_type'] < 1
    assert c == R.compare(R.summary(res), R.summary(other))
    assert R.compare(R.stack_ref([BENZENE]), R.stack_ref([SPIRO]))['ring_size'] == 1.0       # disjoint supports
    joined = R.concat([R.stack_ref([BENZENE, CHAIN]), R.stack_ref([TWO_FRAGMENTS, ladder(66), EMPTY])])
    assert all(np.array_equal(joined[k], res[k]) for k in res)


def test_command_line_with_ref(tmp_path, capsys):
    pool = {'finished': [BENZENE, NAPHTHALENE, CHAIN], 'failed': [SPIRO]}
    torch.save(pool, str(tmp_path / 'samples_all.pt'))
    assert R.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'a.npz'), '--ref']) == 0
    printed = json.loads(capsys.readouterr().out)
    assert printed['n_measured'] == 3 and printed['ring_size']['counts'] == [0, 0, 0, 3, 0, 0, 0]
    saved = molpack.load_npz(str(tmp_path / 'a.npz'))
    want = R.stack_ref(pool['finished'])
    assert set(saved) == set(want) and all(np.array_equal(saved[k], want[k]) for k in want)
    assert R.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'b.npz'), '--ref', '--part', 'failed']) == 0
    capsys.readouterr()
    assert R.main(['compare', str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')]) == 0
    got = json.loads(capsys.readouterr().out)
    assert got['ring_size'] == 1.0 and got['element'] == 0.0
