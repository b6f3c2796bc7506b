"""Host tests of moldiff_amd/groups.py: ``groups_ref`` against counts written out by hand and against plain enumeration of all injective
maps written here, its independence of atom and bond order, the step budget, ``PatternSet``'s refusals, the numbers, the command line and
the wiring of the C entry.  No GPU."""
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from moldiff_amd import molpack
from moldiff_amd import groups as G
from moldiff_amd import rings as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)
NORMAL = [4, 3, 2, 1, 3, 2, 1]


def mol(ele, bonds):
    ele = [6] * ele if isinstance(ele, int) else ele
    bonds = [tuple(b) + (1,) * (3 - len(b)) for b in bonds]
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
            'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def ring(n, first=0, t=1):
    return [(first + k, first + (k + 1) % n, t) for k in range(n)]


def clique(n):
    return mol(n, list(itertools.combinations(range(n), 2)))


def wild_path(k, name=None):
    return {'name': name or f'path{k}', 'atoms': [{} for _ in range(k)], 'bonds': [[i, i + 1, '*'] for i in range(k - 1)]}


ACETAMIDE = mol([6, 6, 8, 7], [(0, 1), (1, 2, 2), (1, 3)])                         # CH3-C(=O)-NH2
METHYL_ACETATE = mol([6, 6, 8, 8, 6], [(0, 1), (1, 2, 2), (1, 3), (3, 4)])         # CH3-C(=O)-O-CH3
ACETIC_ACID = mol([6, 6, 8, 8], [(0, 1), (1, 2, 2), (1, 3)])
BENZENE = mol(6, ring(6, t=4))
PYRIDINE = mol([7, 6, 6, 6, 6, 6], ring(6, t=4))
CHLOROBENZENE = mol([6] * 6 + [17], ring(6, t=4) + [(0, 6)])
TRIANGLE = mol(3, ring(3))
DEFAULT = G.PatternSet.default()


def matches(m, pset=DEFAULT, **kw):
    r = G.stack_ref([m], pset, **kw)
    assert r['status'][0] == 0 and not r['pat_status'].any()
    return dict(zip(pset.names, G.n_match(r)[0].tolist()))


def only(counts):
    return {k: v for k, v in counts.items() if v}


def test_default_set_on_literal_molecules():
    assert len(DEFAULT) == 19 and DEFAULT.needs_rings and len(set(DEFAULT.names)) == 19
    aut = dict(zip(DEFAULT.names, DEFAULT.automorphisms().tolist()))
    assert aut['benzene'] == 12 and aut['pyridine'] == 2 and aut['ether'] == 2 and aut['sulfonamide'] == 2 and aut['amide'] == 1
    assert only(matches(ACETAMIDE)) == {'carbonyl': 1, 'amide': 1, 'amine_2h': 1, 'donor': 1, 'acceptor': 2}
    # the ether pattern is C-O-C with two single bonds: the bridging O of an ester is one
    assert only(matches(METHYL_ACETATE)) == {'ether': 1, 'carbonyl': 1, 'ester': 1, 'acceptor': 2}
    assert only(matches(ACETIC_ACID)) == {'hydroxyl': 1, 'carbonyl': 1, 'carboxylic_acid': 1, 'donor': 1, 'acceptor': 2}
    assert only(matches(BENZENE)) == {'benzene': 1}
    assert only(matches(PYRIDINE)) == {'pyridine': 1, 'acceptor': 1}
    assert only(matches(CHLOROBENZENE)) == {'halogen': 1, 'aryl_halide': 1, 'benzene': 1}
    assert only(matches(mol([6, 6, 17], [(0, 1), (1, 2)]))) == {'halogen': 1, 'alkyl_halide': 1}
    assert only(matches(mol([6, 6, 7], [(0, 1), (1, 2, 3)]))) == {'nitrile': 1, 'acceptor': 1}
    assert only(matches(mol([6, 16, 6], [(0, 1), (1, 2)]))) == {'sulfide': 1}
    # methanesulfonamide CH3-S(=O)(=O)-NH2
    assert only(matches(mol([6, 16, 8, 8, 7], [(0, 1), (1, 2, 2), (1, 3, 2), (1, 4)]))) == {'amine_2h': 1, 'sulfonamide': 1, 'donor': 1, 'acceptor': 3}
    # trimethylamine, dimethylamine; naphthalene has two six-rings of aromatic bonds, and the 10-ring around it is no embedding of six
    assert only(matches(mol([7, 6, 6, 6], [(0, 1), (0, 2), (0, 3)]))) == {'amine_0h': 1}
    assert only(matches(mol([6, 7, 6], [(0, 1), (1, 2)]))) == {'amine_1h': 1, 'donor': 1, 'acceptor': 1}
    assert only(matches(mol(10, ring(10, t=4) + [(0, 5, 4)]))) == {'benzene': 2}
    # a six-ring of single bonds is no benzene; a 6-cycle of aromatic bonds whose bonds lie in a smaller ring is none either
    assert only(matches(mol(6, ring(6)))) == {}
    r = G.groups_ref(ACETAMIDE, DEFAULT)
    bit = {n: 1 << k for k, n in enumerate(DEFAULT.names)}
    assert r['atom_hit'].tolist() == [0, bit['carbonyl'] | bit['amide'], bit['acceptor'], bit['amine_2h'] | bit['donor'] | bit['acceptor']]
    assert r['n_anchor'].tolist() == [int(v > 0) for v in r['n_embed']][:17] + [1, 2]


def test_triangle_against_a_path_counts_embeddings_not_atom_sets():
    pset = G.PatternSet([wild_path(3)])
    r = G.groups_ref(TRIANGLE, pset)
    assert r['n_embed'].tolist() == [6] and pset.automorphisms().tolist() == [2] and r['n_anchor'].tolist() == [3]
    assert G.n_match(G.stack_ref([TRIANGLE], pset)).tolist() == [[3]]               # RDKit's uniquified count would be 1
    # steps: 3 start candidates + 3 x deg 2 (atom 1) + 6 partial embeddings of two atoms x deg 2 (atom 2)
    assert r['steps'].tolist() == [3 + 6 + 12] and r['atom_hit'].tolist() == [1, 1, 1]
    with pytest.raises(AssertionError, match='multiple'):
        G.n_match({'n_embed': np.asarray([[5]]), 'aut': np.asarray([2])})


# ---- plain enumeration -----------------------------------------------------------------------------------------------------------

def molecule_facts(m):
    cls = [ELEMENTS.index(int(z)) for z in m['element']]
    n, nb = len(cls), m['bond_index'].shape[1] // 2
    rg = R.rings_ref(m)
    bond, deg, val2, arom = {}, [0] * n, [0] * n, [False] * n
    for e in range(nb):
        i, j, t = int(m['bond_index'][0, e]), int(m['bond_index'][1, e]), int(m['bond_type'][e])
        bond[(i, j)] = bond[(j, i)] = (t, G.ring_class(rg['bond_ring_min'][e]))
        for a in (i, j):
            deg[a] += 1
            val2[a] += 3 if t == 4 else 2 * t
            arom[a] |= t == 4
    hyd = [max(0, NORMAL[cls[a]] - (val2[a] + 1) // 2) for a in range(n)]
    return cls, bond, deg, hyd, [G.ring_class(v) for v in rg['atom_ring_min']], arom


def brute_force(m, pat):
    """n_embed, the anchors and steps of one pattern by enumeration of all injective maps of its first k atoms, k = 1 .. atoms"""
    cls, bond, deg, hyd, arc, arom = molecule_facts(m)
    n, na = len(cls), len(pat.atoms)

    def valid(img):
        for k, a in enumerate(img):
            em, dm, hm, rm, ar = pat.atoms[k]
            if not (em >> cls[a] & 1 and dm >> min(deg[a], 7) & 1 and hm >> min(hyd[a], 4) & 1 and rm >> arc[a] & 1):
                return False
            if ar and ar != (1 if arom[a] else 2):
                return False
        for i, j, tm, rm in pat.bonds:
            if i < len(img) and j < len(img):
                b = bond.get((img[i], img[j]))
                if b is None or not (tm >> b[0] & 1 and rm >> b[1] & 1):
                    return False
        return True
    steps, embed, anchors = n, 0, set()
    for k in range(1, na + 1):
        for img in itertools.permutations(range(n), k):
            if not valid(img):
                continue
            if k == na:
                embed += 1
                anchors.add(img[0])
            else:
                steps += deg[img[min(i for i, j, _, _ in pat.bonds if j == k)]]
    return embed, anchors, steps


def random_molecule(g):
    n = int(g.integers(1, 10))
    p = float(g.choice([0.2, 0.35, 0.5, 0.8]))
    pairs = [pq for pq in itertools.combinations(range(n), 2) if g.random() < p]
    return mol(g.choice([6, 6, 6, 7, 8, 17], n).tolist(), [(i, j, int(g.choice([1, 1, 1, 2, 4]))) for i, j in pairs])


def random_pattern(g, name):
    na = int(g.integers(1, 5))
    pairs = {(int(g.integers(0, k)), k) for k in range(1, na)}                    # a spanning tree, then further bonds
    loose = g.random() < 0.4                                                       # a shape with few constraints and more closing bonds
    pairs |= {pq for pq in itertools.combinations(range(na), 2) if g.random() < (0.6 if loose else 0.3)}
    label = g.permutation(na)                                                      # listed in an order PatternSet has to mend
    atoms = []
    for _ in range(na):
        at = {}
        if loose and g.random() < 0.8:
            atoms.append(at)
            continue
        if g.random() < 0.6:
            at['elem'] = [['C'], ['C', 'N'], ['O'], ['N', 'O', 'Cl']][int(g.integers(0, 4))]
        if g.random() < 0.3:
            at['deg'] = sorted({int(v) for v in g.integers(1, 5, 2)})
        if g.random() < 0.3:
            at['h'] = sorted({int(v) for v in g.integers(0, 4, 2)})
        if g.random() < 0.3:
            at['ring'] = ['ring', 'none', [3], [3, 4], [0, 5, 6]][int(g.integers(0, 5))]
        if g.random() < 0.2:
            at['arom'] = bool(g.random() < 0.5)
        atoms.append(at)
    bonds = []
    for i, j in sorted(pairs):
        b = [int(label[i]), int(label[j]), '*' if loose or g.random() < 0.5 else sorted({int(v) for v in g.integers(1, 5, 2)})]
        if g.random() < 0.3:
            b.append(['ring', 'none', [3], [4, 5]][int(g.integers(0, 4))])
        bonds.append(b)
    return {'name': name, 'atoms': atoms, 'bonds': bonds}


def test_agrees_with_enumeration_of_all_injective_maps():
    g = np.random.default_rng(23)
    seen = {'embed': 0, 'ring': 0, 'h': 0, 'closure': 0}
    for k in range(300):
        m = random_molecule(g)
        pset = G.PatternSet([random_pattern(g, f'p{q}') for q in range(3)])
        got = G.groups_ref(m, pset)
        assert got['status'] == 0 and not got['pat_status'].any()
        hit = got['atom_hit'].view(np.uint32)
        for q, pat in enumerate(pset.patterns):
            embed, anchors, steps = brute_force(m, pat)
            assert (int(got['n_embed'][q]), int(got['steps'][q]), int(got['n_anchor'][q])) == (embed, steps, len(anchors)), (k, q)
            assert {a for a in range(len(hit)) if hit[a] >> q & 1} == anchors, (k, q)
            assert embed % pat.automorphisms() == 0
            seen['embed'] += embed > 0
            seen['ring'] += embed > 0 and pat.needs_rings
            seen['h'] += embed > 0 and any(a[2] != 0x1f for a in pat.atoms)
            seen['closure'] += embed > 0 and len(pat.bonds) > len(pat.atoms) - 1
    assert seen['embed'] > 100 and min(seen.values()) >= 10, seen


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
    return {'element': ele, 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}, new


def test_invariant_under_relabelling_and_bond_order():
    g = np.random.default_rng(7)
    extra = G.PatternSet([wild_path(4), {'name': 'tri', 'atoms': [{}, {}, {}], 'bonds': [[0, 1, '*'], [1, 2, '*'], [0, 2, '*']]}])
    mols = [ACETAMIDE, METHYL_ACETATE, CHLOROBENZENE, mol(10, ring(10, t=4) + [(0, 5, 4)])] + [random_molecule(g) for _ in range(20)]
    for k, m in enumerate(mols):
        for pset, steps in ((DEFAULT, G.DEFAULT_MAX_STEPS), (extra, 40)):          # 40: some random molecules exceed it, others do not
            a = G.groups_ref(m, pset, max_steps=steps)
            m2, new = relabelled(m, 300 + k)
            b = G.groups_ref(m2, pset, max_steps=steps)
            for key in G.MOL_KEYS:
                assert np.array_equal(a[key], b[key]), (k, key)
            assert np.array_equal(a['atom_hit'], b['atom_hit'][new]), k


def test_budget_is_charged_per_start_atom_in_steps():
    def start_count(n, k):
        """steps of one start atom of an n-clique against a wildcard path of k atoms, from the definition: 1 + SUM over j = 1 .. k - 1 of
        (partial embeddings of j atoms from this start: (n-1)(n-2) ... j - 1 factors) x (degree n - 1)"""
        return 1 + sum((n - 1) * int(np.prod([n - 1 - i for i in range(j - 1)])) for j in range(1, k))
    # The 12-clique against the 8-atom wildcard path: one start atom's count is 4,368,233, beyond the largest budget the entry
    # accepts (2^20), so no legal budget measures this pair: it is flagged at the largest one -- checked here at a budget that ends
    # the search early, the flag being monotone in the budget -- and the largest budget is refused beyond.
    assert start_count(12, 8) == 4368233 > G.MAX_STEPS_LIMIT
    K12 = clique(12)
    r = G.groups_ref(K12, G.PatternSet([wild_path(8)]), max_steps=5000)
    assert r['status'] == 0 and r['pat_status'].tolist() == [3]
    assert r['n_embed'].tolist() == [0] and r['n_anchor'].tolist() == [0] and r['steps'].tolist() == [0] and not r['atom_hit'].any()
    with pytest.raises(ValueError, match='max_steps'):
        G.groups_ref(K12, G.PatternSet([wild_path(8)]), max_steps=start_count(12, 8))
    with pytest.raises(ValueError, match='max_steps'):
        G.groups_ref(K12, G.PatternSet([wild_path(2)]), max_steps=0)
    # the exact threshold, on the same clique with the longest wildcard path whose count a quick test can enumerate: 5 atoms
    count = start_count(12, 5)
    assert count == 1 + 11 * (1 + 11 + 110 + 990)
    pset = G.PatternSet([wild_path(5), wild_path(2)])
    below, at = G.groups_ref(K12, pset, max_steps=count - 1), G.groups_ref(K12, pset, max_steps=count)
    assert below['pat_status'].tolist() == [3, 0] and below['n_embed'].tolist() == [0, 132] and below['steps'].tolist() == [0, 12 * 12]
    assert below['atom_hit'].tolist() == [2] * 12 and below['n_anchor'].tolist() == [0, 12]
    assert at['pat_status'].tolist() == [0, 0] and at['n_embed'].tolist() == [12 * 11 * 10 * 9 * 8, 132]
    assert at['steps'].tolist() == [12 * count, 144] and at['atom_hit'].tolist() == [3] * 12 and at['n_anchor'].tolist() == [12, 12]


def test_pattern_set_refusals_and_reordering():
    ok = {'name': 'a', 'atoms': [{}, {}], 'bonds': [[0, 1, '*']]}
    with pytest.raises(ValueError, match='not connected'):
        G.PatternSet([{'name': 'd', 'atoms': [{}, {}, {}], 'bonds': [[0, 1, '*']]}])
    with pytest.raises(ValueError, match='1 .. 8 atoms'):
        G.PatternSet([wild_path(9)])
    with pytest.raises(ValueError, match='at most 12 bonds'):
        G.PatternSet([{'name': 'k6', 'atoms': [{}] * 6, 'bonds': [[i, j, '*'] for i, j in itertools.combinations(range(6), 2)][:13]}])
    with pytest.raises(ValueError, match='1 .. 32 patterns'):
        G.PatternSet([dict(ok, name=f'p{k}') for k in range(33)])
    with pytest.raises(ValueError, match='1 .. 32 patterns'):
        G.PatternSet([])
    with pytest.raises(ValueError, match='element'):
        G.PatternSet([{'name': 'b', 'atoms': [{'elem': ['B']}]}])
    with pytest.raises(ValueError, match='element'):
        G.PatternSet([{'name': 'br', 'atoms': [{'elem': [35]}]}])
    with pytest.raises(ValueError, match='same pair'):
        G.PatternSet([{'name': 'dup', 'atoms': [{}, {}], 'bonds': [[0, 1, '*'], [1, 0, [1]]]}])
    with pytest.raises(ValueError, match='share a name'):
        G.PatternSet([ok, ok])
    with pytest.raises(ValueError, match='not among'):
        G.PatternSet([{'name': 't', 'atoms': [{}, {}], 'bonds': [[0, 1, [5]]]}])
    with pytest.raises(ValueError, match='unknown key'):
        G.PatternSet([{'name': 'c', 'atoms': [{'charge': 1}]}])
    # a ring constraint with no ring data
    ringed = G.PatternSet([{'name': 'r', 'atoms': [{'ring': 'ring'}]}])
    assert ringed.needs_rings and not G.PatternSet([ok]).needs_rings
    with pytest.raises(ValueError, match='no ring data'):
        G.groups_ref(BENZENE, ringed, ring_data=False)
    assert G.groups_ref(BENZENE, G.PatternSet([ok]), ring_data=False)['n_embed'].tolist() == [12]
    assert G.groups_ref(BENZENE, ringed)['n_embed'].tolist() == [6]
    # atoms listed out of order are reordered (atom 0 stays); the packed table is what the header lays out
    p = G.PatternSet([{'name': 'chain', 'atoms': [{'elem': ['O']}, {'elem': ['N']}, {'elem': ['C']}], 'bonds': [[1, 2, [1]], [2, 0, [2], 'none']]}])
    pat = p.patterns[0]
    assert [a[0] for a in pat.atoms] == [4, 1, 2] and pat.bonds == [(0, 1, 4, 1), (1, 2, 2, 0x7f)] and pat.parent == [-1, 0, 1]
    t = p.pack()
    assert t.shape == (1, 90) and t.dtype == np.int32 and t[0, :2].tolist() == [3, 2]
    assert t[0, 2:7].tolist() == [4, 0xff, 0x1f, 0x7f, 0] and t[0, 42:50].tolist() == [0, 1, 4, 1, 1, 2, 2, 0x7f] and not t[0, 50:].any()
    assert p.valence_table().tolist() == NORMAL and p.valence_table({z: 5 for z in ELEMENTS}).tolist() == [5] * 7
    with pytest.raises(ValueError, match='normal valence'):
        p.valence_table({6: 4})


def test_caps_and_status_codes():
    assert G.groups_ref(mol(256, [(k, k + 1) for k in range(255)]), DEFAULT)['status'] == 0
    r = G.groups_ref(mol(257, [(k, k + 1) for k in range(256)]), DEFAULT)
    assert r['status'] == 1 and r['n_atoms'] == 257 and not r['n_embed'].any() and not r['steps'].any() and not r['atom_hit'].any()
    rungs = 66                                                                       # 65 rings: mdx_mol_rings does not measure it
    ladder = mol(2 * rungs, [(k, k + 1) for k in range(rungs - 1)] + [(rungs + k, rungs + k + 1) for k in range(rungs - 1)] +
                 [(k, rungs + k) for k in range(rungs)])
    r = G.groups_ref(ladder, DEFAULT)
    assert r['status'] == 2 and not r['n_embed'].any() and not r['steps'].any()
    assert G.groups_ref(ladder, G.PatternSet([wild_path(2)]))['status'] == 0          # no ring constraint: no ring data are asked for
    with pytest.raises(ValueError, match='same pair'):
        G.groups_ref(mol(3, [(0, 1), (1, 2), (1, 0)]), DEFAULT)
    with pytest.raises(ValueError, match='element'):
        G.groups_ref(mol([6, 5], [(0, 1)]), DEFAULT)
    # ignored bonds, and a bond type outside 1 .. 4: in the graph, without valence, matching no pattern bond
    assert only(matches(mol([6, 6, 8, 7], [(0, 1), (1, 2, 2), (1, 3), (0, 0), (3, 9)]))) == only(matches(ACETAMIDE))
    r = G.groups_ref(mol([6, 8], [(0, 1, 7)]), G.PatternSet([wild_path(2), {'name': 'o', 'atoms': [{'elem': ['O'], 'deg': [1], 'h': [2]}]}]))
    assert r['n_embed'].tolist() == [0, 1]


def test_summary_compare_concat_and_files(tmp_path, capsys):
    a = G.stack_ref([ACETAMIDE, METHYL_ACETATE, BENZENE, mol(257, [(k, k + 1) for k in range(256)])])
    s = G.summary(a)
    assert s['n_measured'] == 3 and s['n_skipped'] == {'too_large': 1, 'no_ring_data': 0}
    assert s['patterns']['carbonyl'] == {'n_measured': 3, 'n_over_budget': 0, 'mean_matches': 2 / 3, 'fraction_with_match': 2 / 3,
                                         'counts': [1, 2, 0, 0, 0, 0, 0, 0, 0]}
    assert s['patterns']['acceptor']['mean_matches'] == 4 / 3 and s['patterns']['acceptor']['counts'][:3] == [1, 0, 2]
    none = G.summary(G.empty())
    assert none['n_measured'] == 0 and np.isnan(none['patterns']['amide']['mean_matches'])
    b = G.stack_ref([BENZENE, PYRIDINE])
    c = G.compare(a, b)
    assert list(c) == DEFAULT.names and c['halogen'] == 0.0 and 0 < c['carbonyl'] <= 1 and c == G.compare(G.summary(a), G.summary(b))
    joined = G.concat([G.stack_ref([ACETAMIDE, METHYL_ACETATE]), G.stack_ref([BENZENE, mol(257, [(k, k + 1) for k in range(256)])])])
    assert set(joined) == set(a) and all(np.array_equal(joined[k], a[k]) for k in a)
    with pytest.raises(ValueError, match='different pattern sets'):
        G.concat([a, G.stack_ref([BENZENE], G.PatternSet([wild_path(2)]))])
    over = G.summary(G.stack_ref([clique(12), TRIANGLE], G.PatternSet([wild_path(5)]), max_steps=100))
    assert over['patterns']['path5'] == {'n_measured': 1, 'n_over_budget': 1, 'mean_matches': 0.0, 'fraction_with_match': 0.0,
                                         'counts': [1] + [0] * 8}
    # the command line, on the Python path
    pool = {'finished': [ACETAMIDE, BENZENE], 'failed': [PYRIDINE]}
    torch.save(pool, str(tmp_path / 'samples_all.pt'))
    assert G.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'a.npz'), '--ref']) == 0
    printed = json.loads(capsys.readouterr().out)
    assert printed['n_measured'] == 2 and printed['patterns']['benzene']['mean_matches'] == 0.5
    saved, want = molpack.load_npz(str(tmp_path / 'a.npz')), G.stack_ref(pool['finished'])
    assert set(saved) == set(want) and all(np.array_equal(saved[k], want[k]) for k in want)
    assert G.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'b.npz'), '--ref', '--part', 'failed']) == 0
    capsys.readouterr()
    assert G.main(['compare', str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')]) == 0
    got = json.loads(capsys.readouterr().out)
    assert got['pyridine'] == 1.0 and got['halogen'] == 0.0


def test_header_exports_and_binding_agree():
    from moldiff_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'moldiff_hip.h')).read()
    proto = re.search(r'\bint mdx_mol_groups\(([^;]*)\);', hdr).group(1)
    params = [p.strip() for p in proto.replace('\n', ' ').split(',')]
    assert len(params) == 29 and params[0] == 'int32_t B' and params[-1] == 'void* stream' and params[-2] == 'size_t ws_bytes'
    assert 'size_t mdx_mol_groups_ws_bytes(int32_t P);' in hdr
    assert {'mdx_mol_groups', 'mdx_mol_groups_ws_bytes'} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert hasattr(L, 'mdx_mol_groups') and len(L.mdx_mol_groups.argtypes) == 29
    # pointers are void pointers, the scalars have the header's widths
    import ctypes
    width = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t}
    for p, t in zip(params, L.mdx_mol_groups.argtypes):
        assert t is (ctypes.c_void_p if '*' in p else width[p.split()[0]]), p
    assert L.mdx_mol_groups_ws_bytes(1) == 256 and L.mdx_mol_groups_ws_bytes(32) == 128 * 33
    for name, value in (('ATOMS', G.PAT_ATOMS), ('BONDS', G.PAT_BONDS), ('PATTERNS', G.MAX_PATTERNS), ('RECORD', G.RECORD)):
        assert re.search(rf'#define MDX_GROUPS_{name} {value}\b', hdr), name
    with open(os.path.join(ROOT, 'moldiff_amd', 'csrc', 'Makefile')) as f:
        assert 'mdx_groups.o' in f.read()


def test_groups_argument_leaves_the_parser_of_build_parser_alone():
    from moldiff_amd import sample_drug3d
    options = lambda ap: sorted(s for a in ap._actions for s in a.option_strings)
    before = options(sample_drug3d.build_parser())
    ap = sample_drug3d.add_groups_argument(sample_drug3d.build_parser())
    assert options(sample_drug3d.build_parser()) == before and '--groups' not in before
    assert sorted(set(options(ap)) - set(before)) == ['--groups']
    base = ['--config', 'c.yml']
    assert ap.parse_args(base).groups is None and ap.parse_args(base + ['--groups']).groups is True
    assert ap.parse_args(base + ['--groups', 'p.yml']).groups == 'p.yml'
    without = vars(ap.parse_args(base))
    assert {k: v for k, v in without.items() if k != 'groups'} == vars(sample_drug3d.build_parser().parse_args(base))
    opt = sample_drug3d.groups_option
    assert opt(None, {}) == (False, None) and opt(True, {}) == (True, None) and opt('p.yml', {'groups': True}) == (True, 'p.yml')
    assert opt(None, {'groups': True}) == (True, None) and opt(None, {'groups': 'q.yml'}) == (True, 'q.yml') and opt(None, {'groups': False}) == (False, None)
