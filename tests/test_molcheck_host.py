"""Host half of the molecule quality check (moldiff_amd/molcheck.py): ``check_ref`` against scipy's connected components, the
naming and tie-break rules, the valence arithmetic, the default table's keys and the refusals of bad arguments.  CPU only."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from moldiff_amd import molcheck as MC
from moldiff_amd import sample_drug3d


def mol(elements, bonds=(), pos=None):
    """decoded-molecule dict from atomic numbers and (i, j, type) bonds, mirrored like decode_output's layout"""
    n = len(elements)
    b = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    t = np.asarray([t for _, _, t in bonds], dtype=np.int64)
    return {'element': np.asarray(elements, dtype=np.int64), 'atom_pos': np.zeros((n, 3), np.float32) if pos is None else pos,
            'bond_index': np.concatenate([b, b[::-1]], axis=1), 'bond_type': np.concatenate([t, t])}


def test_fragments_match_scipy_on_random_small_graphs():
    g = np.random.default_rng(20240611)
    for _ in range(300):
        n = int(g.integers(1, 30))
        iu, ju = np.triu_indices(n, 1)
        on = g.random(iu.shape[0]) < g.choice([0.02, 0.08, 0.2])
        bonds = [(int(i), int(j), int(g.integers(1, 5))) for i, j in zip(iu[on], ju[on])]
        g.shuffle(bonds)
        r = MC.check_ref(mol([6] * n, bonds, g.standard_normal((n, 3)).astype(np.float32)))
        adj = coo_matrix((np.ones(len(bonds)), ([b[0] for b in bonds], [b[1] for b in bonds])), shape=(n, n))
        k, lab = connected_components(adj, directed=False)
        assert r['n_components'] == k and r['largest_size'] == np.bincount(lab).max() and r['n_atoms'] == n
        # naming rule: an atom's label is the smallest index of its fragment
        want = np.array([np.flatnonzero(lab == lab[i]).min() for i in range(n)])
        assert np.array_equal(r['component'], want)
        sizes = np.bincount(want, minlength=n)
        assert r['largest_label'] == int(np.flatnonzero(sizes == sizes.max()).min())


def test_tie_goes_to_the_smaller_label_and_empty_molecule():
    r = MC.check_ref(mol([6, 6, 6, 6, 6], [(1, 3, 1), (0, 4, 1)]))      # fragments {0,4}, {1,3}, {2}
    assert r['component'].tolist() == [0, 1, 2, 1, 0] and (r['n_components'], r['largest_size'], r['largest_label']) == (3, 2, 0)
    r = MC.check_ref(mol([], []))
    assert (r['n_components'], r['largest_size'], r['largest_label'], r['n_overvalent']) == (0, 0, -1, 0)
    assert r['min_dist'] == np.inf and r['max_bond_len'] == 0.0
    assert MC.check_ref(mol([8]))['min_dist'] == np.inf


def test_valence_arithmetic_and_aromatic_halves():
    assert MC.bond_weight2([1, 2, 3, 4], 4).tolist() == [2, 4, 6, 3]
    star = lambda k, t: mol([6] * (k + 1), [(0, i + 1, t) for i in range(k)])
    r = MC.check_ref(star(1, 4))                     # one aromatic bond: 3/2 -> 1
    assert r['valence2'].tolist() == [3, 3] and r['valence'].tolist() == [1.5, 1.5] and r['n_overvalent'] == 0
    assert MC.check_ref(mol([9, 6], [(0, 1, 4)]))['n_overvalent'] == 0      # F: 3 // 2 = 1 <= 1
    r = MC.check_ref(star(3, 4))                     # ring-fusion carbon: 9/2 -> 4, clean
    assert r['valence2'][0] == 9 and r['n_overvalent'] == 0
    m = mol([6] * 5, [(0, 1, 4), (0, 2, 4), (0, 3, 4), (0, 4, 1)])          # 11/2 -> 5, over
    assert MC.check_ref(m)['valence2'][0] == 11 and MC.check_ref(m)['n_overvalent'] == 1
    assert MC.check_ref(m, {**MC.DEFAULT_MAX_VALENCE, 6: 5})['n_overvalent'] == 0   # the caller's table decides
    r = MC.check_ref(mol([6, 8, 7], [(0, 1, 2), (1, 2, 3)]))               # C=O#N: O has 5
    assert r['valence2'].tolist() == [4, 10, 6] and r['n_overvalent'] == 1
    for z, v in MC.DEFAULT_MAX_VALENCE.items():      # every element at its table value and one above
        assert MC.check_ref(mol([z] + [6] * v, [(0, i + 1, 1) for i in range(v)]))['n_overvalent'] == 0
        assert MC.check_ref(mol([z] + [6] * (v + 1), [(0, i + 1, 1) for i in range(v + 1)]))['n_overvalent'] == 1


def test_distances_are_float64_of_the_stored_coordinates():
    pos = np.array([[0, 0, 0], [3, 4, 0], [3, 4, 12], [3, 4, 12]], dtype=np.float32)
    r = MC.check_ref(mol([6, 6, 6, 6], [(0, 2, 1), (0, 1, 1)], pos))
    assert r['min_dist'] == 0.0 and r['max_bond_len'] == 13.0


def test_restrict_ref_keeps_order_and_reindexes():
    m = mol([6, 7, 8, 9, 16], [(4, 1, 2), (0, 2, 1), (1, 3, 1)], np.arange(15, dtype=np.float32).reshape(5, 3))
    r = MC.check_ref(m)
    f = MC.restrict_ref(m, r['component'], r['largest_label'])
    assert r['largest_label'] == 1 and f['element'].tolist() == [7, 9, 16] and f['atom_pos'][:, 0].tolist() == [3, 9, 12]
    assert f['bond_index'].tolist() == [[2, 0, 0, 1], [0, 1, 2, 0]] and f['bond_type'].tolist() == [2, 1, 2, 1]
    assert MC.check_ref(f)['n_components'] == 1
    assert len(MC.restrict_ref(m, r['component'], -1)['element']) == 0


def test_default_table_covers_exactly_the_featurisers_elements():
    assert sorted(MC.DEFAULT_MAX_VALENCE) == sorted(sample_drug3d.ELEMENT_SYMBOL) == [6, 7, 8, 9, 15, 16, 17]
    assert MC.valence_table([6, 7, 8, 9, 15, 16, 17]) == [4, 4, 2, 1, 7, 6, 1]


def test_bad_arguments_are_refused():
    for f in (0, 0.0, -0.5, 1.0001, 2, 'x', float('nan')):
        with pytest.raises(ValueError):
            MC.fragment_fraction(f)
    assert MC.fragment_fraction(0.75) == (3, 4) and MC.fragment_fraction(1) == (1, 1) and MC.fragment_fraction(0.1) == (1, 10)
    with pytest.raises(ValueError):
        MC.accept_rule('sanitize')
    table = {z: v for z, v in MC.DEFAULT_MAX_VALENCE.items() if z != 15}
    with pytest.raises(ValueError, match='15'):
        MC.valence_table([6, 7, 8, 9, 15, 16, 17], table)
    with pytest.raises(ValueError, match='15'):
        MC.check_ref(mol([6, 15]), table)
    # the entry point refuses them before it touches a device, from the command line and from the config alike
    for extra in (['--accept', 'sanitize'], ['--largest_fragment', '0'], ['--largest_fragment', '1.5']):
        with pytest.raises(ValueError):
            sample_drug3d.main(['--config', 'configs/sample_MolDiff_simple.yml'] + extra)
    for cfg in ({'accept': 'sanitize'}, {'largest_fragment': 0}, {'largest_fragment': 1.5}):
        with pytest.raises(ValueError):
            sample_drug3d.quality_options(None, None, cfg)
    assert sample_drug3d.quality_options(None, None, {}) == ('connected', None, False)
    assert sample_drug3d.quality_options('valence', None, {'largest_fragment': 0.5}) == ('valence', 0.5, True)
