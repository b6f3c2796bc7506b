"""Host tests of the canonical labelling (moldiff_amd/canon.py): the restatement ``canon_ref`` against the figures of the definition, a
brute force over all atom permutations, networkx where it imports, permuted copies, the fingerprint key it replaces for exact
uniqueness, the Kekulé assignment of the canonical form, the SMILES writer and its round trip, the refusals and the command line.
No GPU."""
import itertools

import numpy as np
import pytest
import torch

from moldiff_amd import canon as C
from moldiff_amd import kekule as K
from moldiff_amd import similarity
from .canon_cases import K5, NAMED, brute_force, cert, chain, fold, mol, permuted, random_mol, read_smiles, ring
from .util import run_host_check

SMALL = dict(NAMED, **{f'random{seed}': random_mol(seed) for seed in range(200)})
SAME_KEYS = ('status', 'n_nodes', 'n_leaves', 'n_aut', 'cert_hash', 'canon_n_bonds', 'canon_atom_type', 'canon_bond_index', 'canon_bond_type')


@pytest.fixture(scope='module')
def small_refs():
    """canon_ref and the brute force of every small case, computed once"""
    return {name: (C.canon_ref(m), brute_force(m)) for name, m in SMALL.items()}


def test_the_figures_of_the_definition():
    r = C.canon_ref(NAMED['benzene'])
    assert (r['status'], r['n_aut']) == (0, 12) and r['orbit'].tolist() == [0] * 6
    r = C.canon_ref(K5, max_nodes=206)
    assert (r['status'], r['n_nodes'], r['n_leaves'], r['n_aut']) == (0, 206, 120, 120)
    assert sum(120 // np.prod(range(1, 5 - k + 1), dtype=int) for k in range(5)) == 206         # 5! / (5 - k)! nodes at level k
    r = C.canon_ref(K5, max_nodes=205)
    assert r['status'] == 2 and r['rank'].tolist() == [-1] * 5 and r['n_nodes'] == r['n_aut'] == r['cert_hash'] == 0
    r = C.canon_ref(chain(256))
    assert (r['status'], r['n_aut']) == (0, 2) and np.array_equal(r['orbit'], np.minimum(np.arange(256), 255 - np.arange(256)))
    r = C.canon_ref(chain(257))
    assert r['status'] == 1 and (r['rank'] == -1).all() and not r['orbit'].any()
    for m in (mol(0, []), mol(1, [])):
        r = C.canon_ref(m)
        assert (r['status'], r['n_nodes'], r['n_leaves'], r['n_aut']) == (0, 1, 1, 1)
    # a node deeper than 64 long before the budget: 70 separate bonds lose two atoms of the one big cell per level
    assert C.canon_ref(mol(140, [(2 * k, 2 * k + 1) for k in range(70)]), max_nodes=1 << 20)['status'] == 2
    assert C.canon_ref(mol(24, [(i, j) for i in range(24) for j in range(i + 1, 24)]), max_nodes=1000)['status'] == 2


def test_against_the_brute_force_over_all_permutations(small_refs):
    for name, (r, (form, n_aut, orbit)) in small_refs.items():
        assert r['status'] == 0, name
        assert r['n_aut'] == n_aut, (name, r['n_aut'], n_aut)
        assert r['orbit'].tolist() == orbit.tolist(), (name, r['orbit'], orbit)
        assert sorted(r['rank'].tolist()) == list(range(len(orbit))), name
    names = list(SMALL)
    certs = {name: cert(SMALL[name]) for name in names}
    isomorphic = 0
    for a, b in itertools.combinations(names, 2):
        same = small_refs[a][1][0] == small_refs[b][1][0]
        isomorphic += same
        assert (certs[a] == certs[b]) == same, (a, b)
    print('isomorphic pairs among the small cases', isomorphic)
    assert isomorphic >= 10                                            # the set does hold graphs that are equal up to order
    assert certs['broken_symmetry'] != certs['one_label_changed'] and certs['mirror'] != certs['broken_symmetry']
    assert small_refs['mirror'][0]['n_aut'] == 2 and small_refs['broken_symmetry'][0]['n_aut'] == 1
    assert small_refs['two_equal_fragments'][0]['n_aut'] == 2 and small_refs['star'][0]['n_aut'] == 24
    assert small_refs['cubane'][0]['n_aut'] == 48


def test_with_labels_against_the_brute_force():
    for seed in range(40):
        m = random_mol(seed)
        lab = np.random.default_rng(1000 + seed).integers(0, 2, len(m['element'])) * 65535
        r = C.canon_ref(m, atom_label=lab)
        form, n_aut, orbit = brute_force(m, lab)
        assert r['n_aut'] == n_aut and r['orbit'].tolist() == orbit.tolist(), seed
        assert np.array_equal(r['canon_atom_label'], lab[np.argsort(r['rank'])])
    # a doubled bond is a multiset member: it differs from the single one and from a bond of twice the type
    one, two, dbl = mol(2, [(0, 1, 1)]), mol(2, [(0, 1, 1), (1, 0, 1)]), mol(2, [(0, 1, 2)])
    assert len({cert(one), cert(two), cert(dbl)}) == 3 and C.canon_ref(two)['canon_n_bonds'] == 2
    # ignored bonds leave no trace
    noisy = mol(3, [(0, 1), (2, 2), (1, 7), (1, 2), (-1, 0)])
    clean = mol(3, [(0, 1), (1, 2)])
    a, b = C.canon_ref(noisy), C.canon_ref(clean)
    assert a['canon_n_bonds'] == 2 and a['cert_hash'] == b['cert_hash'] and a['n_bonds'] == 5
    assert a['canon_bond_index'][:, 2:].tolist() == [[0] * 3] * 2 and np.array_equal(a['canon_bond_index'][:, :2], b['canon_bond_index'])


def test_against_networkx_on_larger_molecules():
    nx = pytest.importorskip('networkx')
    from networkx.algorithms.isomorphism import GraphMatcher
    mols = [random_mol(500 + s, 20, 30) for s in range(15)]
    mols += [permuted(m, 900 + k)[0] for k, m in enumerate(mols)]

    def graph(m):
        g = nx.Graph()
        g.add_nodes_from((a, {'z': int(z)}) for a, z in enumerate(m['element']))
        nb = m['bond_index'].shape[1] // 2
        g.add_edges_from((int(m['bond_index'][0, e]), int(m['bond_index'][1, e]), {'t': int(m['bond_type'][e])}) for e in range(nb))
        return g
    match = lambda a, b: GraphMatcher(a, b, node_match=lambda x, y: x['z'] == y['z'], edge_match=lambda x, y: x['t'] == y['t'])
    graphs = [graph(m) for m in mols]
    refs = [C.canon_ref(m) for m in mols]
    certs = [cert(m) for m in mols]
    for m, g, r in zip(mols, graphs, refs):
        auts = list(match(g, g).isomorphisms_iter())
        assert r['status'] == 0 and r['n_aut'] == len(auts)
        assert r['orbit'].tolist() == [min(p[v] for p in auts) for v in range(len(m['element']))]
    for a, b in itertools.combinations(range(len(mols)), 2):
        assert (certs[a] == certs[b]) == match(graphs[a], graphs[b]).is_isomorphic(), (a, b)


def test_order_independence(small_refs):
    cases = dict(SMALL, K5=K5, chain40=chain(40))
    for k, (name, m) in enumerate(cases.items()):
        m = dict(m, atom_pos=np.random.default_rng(k).normal(size=(len(m['element']), 3)).astype(np.float32))
        r = C.canon_ref(m)
        for s in range(5):
            m2, new, _ = permuted(m, 10 * k + s)
            r2 = C.canon_ref(m2)
            for key in SAME_KEYS:
                assert np.array_equal(r[key], r2[key]), (name, s, key)
            # the positions are permuted alike: both orders put an atom of the same orbit at every rank
            assert sorted(map(tuple, r['canon_pos'].tolist())) == sorted(map(tuple, r2['canon_pos'].tolist()))
            # the orbit partitions correspond under the permutation
            assert len(set(zip(r['orbit'].tolist(), r2['orbit'][new].tolist()))) == len(set(r['orbit'].tolist())) == len(set(r2['orbit'].tolist()))
            assert np.array_equal(C.canonical_mol(m, r)['element'], C.canonical_mol(m2, r2)['element'])


def test_separation_from_the_fingerprint_key():
    spec = similarity.FingerprintSpec()
    key = lambda name: int(similarity.fingerprint_ref(NAMED[name], spec)['key'])
    assert key('six_ring') == key('two_three_rings') and key('cubane') == key('cuneane')
    assert cert(NAMED['six_ring']) != cert(NAMED['two_three_rings']) and cert(NAMED['cubane']) != cert(NAMED['cuneane'])
    res = C.stack_ref([NAMED['six_ring'], NAMED['two_three_rings'], NAMED['cubane'], NAMED['cuneane'], permuted(NAMED['cubane'], 3)[0],
                       chain(257)])
    s = C.summary(res)
    assert (s['n_molecules'], s['n_measured'], s['n_too_large'], s['n_distinct']) == (6, 5, 1, 4) and s['uniqueness'] == 0.8
    assert s['max_n_aut'] == 72 and sum(s['nodes_hist']) == 5
    ref = C.stack_ref([permuted(NAMED['cuneane'], 5)[0], NAMED['benzene']])
    assert C.novelty(res, ref) == 0.8 and C.novelty(ref, res) == 0.5
    cmp = C.compare(res, ref)
    assert cmp['novelty'] == [0.8, 0.5] and cmp['uniqueness'] == [0.8, 1.0]
    both = C.concat([res, ref])
    assert C.summary(both)['n_distinct'] == 5 and C.certificate(both, 6) == C.certificate(res, 3)
    assert C.certificate(res, 5) is None and C.canonical_mol(chain(257), C.mol_result(res, 5)) is None
    assert C.summary(C.empty())['n_molecules'] == 0


IMIDAZOLE_LIKE = mol([7, 6, 7, 6, 6, 6], ring(5, t=4) + [(3, 5, 1)])            # 4-methylimidazole: which N takes the hydrogen
PYRIDONE_LIKE = mol([7] + [6] * 5 + [8, 6], ring(6, t=4) + [(1, 6, 2), (3, 7, 1)])
TWO_RINGS = mol([7, 6, 7, 6, 6, 7, 6, 6, 6, 6], ring(5, t=4) + ring(5, 5, t=4) + [(4, 9, 1)])


def canonical_kekule(m):
    """-> (the canonical molecule, its Kekulé result, its SMILES)"""
    cm = C.canonical_mol(m, C.canon_ref(m))
    kr = K.kekulize_ref(cm)
    return cm, kr, C.smiles(cm, kr)


def written_cert(cm, kr):
    """the full certificate of the Kekulé graph a string is written from: bond orders as types, class + 8 h + 64 charge as labels"""
    nb = cm['bond_index'].shape[1] // 2
    written = dict(cm, bond_type=np.concatenate([kr['kek_order'][:nb], kr['kek_order'][:nb]]).astype(np.int64))
    return cert(written, fold(written, kr['kek_h'], kr['charge']))


def test_the_kekule_structure_of_the_canonical_form_does_not_depend_on_the_atom_order():
    for k, m in enumerate((IMIDAZOLE_LIKE, PYRIDONE_LIKE, TWO_RINGS, NAMED['pyridine'])):
        cm, kr, text = canonical_kekule(m)
        assert bool(K.kekulizable(kr))
        if k < 3:
            assert any((kr['atom_flag'] & 3) == K.ROLE_MAY)
        for s in range(5):
            m2 = permuted(m, 77 * k + s)[0]
            cm2, kr2, text2 = canonical_kekule(m2)
            for key in ('kek_order', 'charge', 'kek_h'):
                assert np.array_equal(kr[key], kr2[key]), (k, s, key)
            assert text2 == text
    assert text.count('=') == 3 and text.count('N') == 1                # pyridine


def test_smiles_of_permuted_copies_and_of_different_molecules():
    texts = {}
    simple = [m for m in SMALL.values() if len({(min(i, j), max(i, j)) for i, j in m['bond_index'].T.tolist()}) == m['bond_index'].shape[1] // 2]
    for k, m in enumerate(simple):
        cm, kr, text = canonical_kekule(m)
        if text is None:
            assert not bool(K.kekulizable(kr))
            continue
        for s in range(2):
            assert canonical_kekule(permuted(m, 5 * k + s)[0])[2] == text
        texts.setdefault(text, []).append(written_cert(cm, kr))     # an aromatic bond and the double bond it becomes are one string
    assert len(texts) >= 100
    for text, certs in texts.items():                                  # one string, one molecule
        assert len(set(certs)) == 1, text
    # the reverse is promised per DECODED graph only: the atom order comes from the graph with its aromatic bonds, so an aromatic
    # input and the input that spells the same double bonds out may be written in two orders
    assert C.smiles(None, None) is None
    assert canonical_kekule(mol(5, ring(5, t=4)))[2] is None           # an all-carbon aromatic five-ring has no Kekulé structure


# a carbon bonded to every atom of a chain of twelve nitrogens: the walk starts at the carbon (the lowest label) and opens a ring
# closure to all but one of the twelve there, more than nine at once
WHEEL = mol([6] + [7] * 12, [(0, k) for k in range(1, 13)] + [(k, k + 1) for k in range(1, 12)])


def test_smiles_round_trip():
    ammonium = mol([7, 6, 6, 6, 6], [(0, 1), (0, 2), (0, 3), (0, 4)])
    cases = {'bracket': mol([15, 6, 6, 6, 6], [(0, 1), (0, 2), (0, 3), (0, 4)]), 'imidazole': IMIDAZOLE_LIKE, 'charged': ammonium, 'pyridinium': mol([7] + [6] * 6, ring(6, t=4) + [(0, 6, 1)]),
             'fragments': mol([6, 8, 6, 8, 7], [(0, 1, 2), (2, 3, 2)]), 'closures': WHEEL, 'triple': mol([6, 6, 7], [(0, 1), (1, 2, 3)]),
             'sulfur': mol([16, 6, 6, 8, 8, 17], [(0, 1), (0, 2), (0, 3, 2), (0, 4, 2), (1, 5)]), 'pyridone': PYRIDONE_LIKE,
             'cubane': NAMED['cubane'], 'two_rings': TWO_RINGS}
    seen = {}
    for name, m in cases.items():
        cm, kr, text = canonical_kekule(m)
        assert text is not None, name
        seen[name] = text
        back, hs, charge = read_smiles(text)
        assert cert(back, fold(back, hs, charge)) == written_cert(cm, kr), (name, text)
    print(seen)
    assert '[P]' in seen['bracket'] and '[' not in seen['imidazole'] and '[N+]' in seen['charged'] and '[N+]' in seen['pyridinium'] and '.' in seen['fragments']
    assert '%10' in seen['closures'] and '%11' in seen['closures'] and '#' in seen['triple'] and seen['fragments'].count('.') == 2
    assert '[' not in seen['sulfur'] and '[' not in seen['cubane']


def test_refusals():
    for bad in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match='max_nodes'):
            C.canon_ref(NAMED['benzene'], max_nodes=bad)
        with pytest.raises(ValueError, match='max_nodes'):
            C.stack_ref([NAMED['benzene']], max_nodes=bad)
    assert C.canon_ref(K5, max_nodes=1 << 20)['status'] == 0
    for lab in ([0, 0, 0, 0, 0, 65536], [0, 0, 0, 0, 0, -1], [0] * 5):
        with pytest.raises(ValueError, match='label'):
            C.canon_ref(NAMED['benzene'], atom_label=lab)
    assert C.canon_ref(NAMED['benzene'], atom_label=[65535] * 6)['n_aut'] == 12
    with pytest.raises(ValueError, match='atomic numbers'):
        C.canon_ref(mol([6, 5], [(0, 1)]))
    with pytest.raises(ValueError, match='atomic numbers'):
        C.stack_ref([mol([6, 35], [(0, 1)])])


def test_command_line(tmp_path, capsys):
    import json
    mols = [NAMED['benzene'], permuted(NAMED['benzene'], 1)[0], NAMED['pyridine'], chain(257)]
    torch.save({'finished': mols, 'failed': []}, tmp_path / 'samples_all.pt')
    assert C.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'a.npz'), '--ref']) == 0
    got = json.loads(capsys.readouterr().out)
    assert (got['n_molecules'], got['n_measured'], got['n_distinct'], got['n_too_large']) == (4, 3, 2, 1)
    torch.save(mols[2:], tmp_path / 'list.pt')
    assert C.main(['stats', str(tmp_path / 'list.pt'), '--out', str(tmp_path / 'b.npz'), '--ref', '--max_nodes', '100']) == 0
    capsys.readouterr()
    assert C.main(['compare', str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')]) == 0
    cmp = json.loads(capsys.readouterr().out)
    assert cmp['novelty'] == [2 / 3, 0.0] and cmp['uniqueness'] == [2 / 3, 1.0]


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/canon_host_check.cpp over csrc/mdx_canon_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('canon_host_check', tmp_path)
