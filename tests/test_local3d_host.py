"""CPU tests of the local 3D geometry statistics' host half (moldiff_amd/local3d.py): pattern syntax and canonical form, the numpy /
float64 restatement ``local3d_ref`` on hand-built lattice molecules, the Jensen-Shannon divergence, ``frequent_patterns``, the
statistics container and the sampling entry point's option.  Lattice coordinates make every expected value exact in float64 up to
the last bit of atan2 / degrees, so values are compared within 1e-9 degrees."""
import numpy as np
import pytest

from moldiff_amd import local3d as L3
from moldiff_amd import sample_drug3d
from .util import run_host_check


def mol(ele, bonds, pos):
    """a decoded molecule dict: every bond once, then all of them flipped"""
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'atom_pos': np.asarray(pos, dtype=np.float32).reshape(len(ele), 3),
            'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.asarray(bt + bt, dtype=np.int64)}


CHAIN_POS = [[1, 0, 0], [0, 0, 0], [0, 0, 1], [0, 1, 1]]            # the +90 degree example
CHAIN = mol([6, 6, 7, 8], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], CHAIN_POS)
TRIANGLE = mol([6, 6, 6], [(0, 1, 1), (1, 2, 1), (0, 2, 1)], [[0, 0, 0], [1, 0, 0], [0, 1, 0]])
SQUARE = mol([6, 6, 6, 6], [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)], [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])


def test_parse_pattern_and_canonical_form():
    assert L3.parse_pattern('C:C-N') == (6, 4, 6, 1, 7)
    assert L3.parse_pattern('Cl-C') == (17, 1, 6) and L3.parse_pattern('C#N') == (6, 3, 7) and L3.parse_pattern('C=O') == (6, 2, 8)
    assert L3.parse_pattern('C:C:C:C') == (6, 4, 6, 4, 6, 4, 6) and L3.parse_pattern((6, 1, 7)) == (6, 1, 7)
    assert L3.canonical(L3.parse_pattern('N-C:C')) == L3.canonical(L3.parse_pattern('C:C-N')) == (6, 4, 6, 1, 7)
    assert L3.pattern_text((6, 4, 6, 1, 17)) == 'C:C-Cl'
    spec = L3.Local3DSpec(angles=['N-C:C'])
    assert spec.patterns['angles'] == ((6, 4, 6, 1, 7),) and spec.row_of('angles', 'C:C-N') == spec.row_of('angles', 'N-C:C') == 0
    for bad in ('C~C', 'X-C', 'C-', 'C', 'C-C-C-C-C', 'c:c'):
        with pytest.raises(ValueError):
            L3.parse_pattern(bad)


def test_spec_refuses_duplicates_wrong_kinds_and_bad_bins():
    with pytest.raises(ValueError, match='duplicate'):
        L3.Local3DSpec(angles=['N-C:C', 'C:C-N'])
    with pytest.raises(ValueError, match='duplicate'):
        L3.Local3DSpec(lengths=['C-C', 'C-C'])
    with pytest.raises(ValueError):
        L3.Local3DSpec(lengths=['C-C-C'])
    with pytest.raises(ValueError):
        L3.Local3DSpec(lengths=['C-C'], atomic_numbers=[7, 8])
    with pytest.raises(ValueError):
        L3.Local3DSpec(lengths=[(6, 5, 6)])
    with pytest.raises(ValueError):
        L3.Local3DSpec(length_bins=(2.0, 1.0, 10))
    with pytest.raises(ValueError):
        L3.Local3DSpec(angle_bins=(0, 180, 0))
    with pytest.raises(ValueError):
        L3.Local3DSpec(lengths=[(6, 1, z) for z in (6, 7, 8, 9, 15, 16, 17)] * 10)   # duplicates come first
    many = [(a, b, c) for a in (6, 7, 8, 9, 15, 16, 17) for b in (1, 2, 3, 4) for c in (6, 7, 8, 9, 15, 16, 17) if a <= c]
    assert len(many) > 64
    with pytest.raises(ValueError, match='more than 64'):
        L3.Local3DSpec(lengths=many)
    s = L3.Local3DSpec(lengths=['C-C'], angles=['C-C-C', 'C-C=N'], dihedrals=['C-C-C-C'], length_bins=(1, 2, 10))
    assert s.kind_ptr == [0, 1, 3, 4] and s.hist_size == 10 + 2 * 180 + 180
    assert s.hist_slice('angles', 1) == slice(10 + 180, 10 + 360) and s.hist_slice('dihedrals') == slice(370, 550)
    assert L3.Local3DSpec.from_dict(s.to_dict()) == s


def test_chain_gives_plus_90_in_either_numbering():
    spec = L3.Local3DSpec(lengths=['C-C', 'C=N', 'N-O'], angles=['C-C=N', 'O-N=C'], dihedrals=['C-C=N-O'])
    rev = mol([8, 7, 6, 6], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], CHAIN_POS[::-1])
    for m in (CHAIN, rev):
        r = L3.local3d_ref(m, spec)
        assert r['n_items'].tolist() == [3, 2, 1]
        assert [v.tolist() for v in r['values']['lengths']] == [[1.0], [1.0], [1.0]]
        assert np.allclose(np.concatenate(r['values']['angles']), [90.0, 90.0], atol=1e-9)
        assert np.allclose(r['values']['dihedrals'][0], [90.0], atol=1e-9)          # the sign: +90, not -90
        assert r['outside'].tolist() == [0] * 6 and r['hist'].sum() == 6
        assert r['hist'][spec.hist_slice('dihedrals', 0)][135] == 1                 # bins of 2 degrees: -180 + 2 * 135 <= 90
    mirror = mol([6, 6, 7, 8], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], np.asarray(CHAIN_POS) * [1, -1, 1])
    assert np.allclose(L3.local3d_ref(mirror, spec)['values']['dihedrals'][0], [-90.0], atol=1e-9)


def test_triangle_square_and_atoms_with_few_bonds():
    spec = L3.Local3DSpec(lengths=['C-C', 'C:C'], angles=['C-C-C', 'C:C:C'], dihedrals=['C-C-C-C', 'C:C:C:C'])
    t = L3.local3d_ref(TRIANGLE, spec)
    assert t['n_items'].tolist() == [3, 3, 0] and len(t['values']['angles'][0]) == 3 and len(t['values']['dihedrals'][0]) == 0
    assert np.allclose(sorted(t['values']['angles'][0]), [45, 45, 90], atol=1e-9)
    s = L3.local3d_ref(SQUARE, spec)
    assert s['n_items'].tolist() == [4, 4, 4]
    assert np.allclose(s['values']['angles'][1], [90] * 4, atol=1e-9) and np.allclose(s['values']['dihedrals'][1], [0] * 4, atol=1e-9)
    # atoms with 0 and 1 bonds: an isolated atom and a two-atom molecule give no angle and no dihedral
    lone = mol([6, 6, 8], [(0, 1, 1)], [[0, 0, 0], [1.5, 0, 0], [5, 5, 5]])
    r = L3.local3d_ref(lone, spec)
    assert r['n_items'].tolist() == [1, 0, 0] and r['values']['lengths'][0].tolist() == [1.5]
    empty = {'element': np.zeros(0, dtype=np.int64), 'atom_pos': np.zeros((0, 3), dtype=np.float32)}
    assert L3.local3d_ref(empty, spec)['n_items'].tolist() == [0, 0, 0]
    one = {'element': np.asarray([6]), 'atom_pos': np.zeros((1, 3), dtype=np.float32), 'bond_index': np.zeros((2, 0), dtype=np.int64),
           'bond_type': np.zeros(0, dtype=np.int64)}
    assert L3.local3d_ref(one, spec)['n_items'].tolist() == [0, 0, 0]
    # a star: 3 neighbours -> 3 angles, no dihedral; unmatched items are counted in n_items but in no histogram
    star = mol([7, 6, 6, 8], [(0, 1, 1), (0, 2, 1), (0, 3, 1)], [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    r = L3.local3d_ref(star, spec)
    assert r['n_items'].tolist() == [3, 3, 0] and r['hist'].sum() == 0 and r['outside'].sum() == 0


def test_outside_and_last_bin_follow_numpy_histogram():
    spec = L3.Local3DSpec(lengths=['C-C'], length_bins=(1.0, 2.0, 4))
    m = mol([6] * 5, [(0, 1, 1), (0, 2, 1), (0, 3, 1), (0, 4, 1)], [[0, 0, 0], [0.5, 0, 0], [0, 2, 0], [0, 0, 1.25], [np.nan, 0, 0]])
    r = L3.local3d_ref(m, spec)
    assert r['hist'].tolist() == [0, 1, 0, 1] and r['outside'].tolist() == [2]      # 2.0 sits in the last bin; 0.5 and NaN outside


def test_jsd():
    a, b = np.array([4, 0, 2, 0]), np.array([0, 3, 0, 9])
    assert L3.jsd_counts(a, a) == 0.0 and L3.jsd_counts(a, 7 * a) == 0.0
    assert L3.jsd_counts(a, b) == pytest.approx(1.0, abs=1e-12)
    c = np.array([1, 2, 3, 4])
    assert L3.jsd_counts(a, c) == pytest.approx(L3.jsd_counts(c, a), abs=1e-15) and 0 < L3.jsd_counts(a, c) < 1
    assert L3.jsd_counts(a, c) == pytest.approx(L3.jsd_counts(a, 5 * c), abs=1e-15)
    assert np.isnan(L3.jsd_counts(a, np.zeros(4))) and np.isnan(L3.jsd_counts(np.zeros(4), a))
    # by hand: p = (1, 0), q = (1/2, 1/2) -> 0.5 * log2(4/3) + 0.5 * (0.5 * log2(2/3) + 0.5 * log2 2) = 0.31127812...
    assert L3.jsd_counts([1, 0], [1, 1]) == pytest.approx(0.5 * np.log2(4 / 3) + 0.25 * np.log2(2 / 3) + 0.25, abs=1e-15)


def test_frequent_patterns():
    mols = [CHAIN, TRIANGLE, SQUARE, SQUARE]
    assert L3.frequent_patterns(mols, 'lengths') == [((6, 4, 6), 8), ((6, 1, 6), 4), ((6, 2, 7), 1), ((7, 1, 8), 1)]
    assert L3.frequent_patterns(mols, 'lengths', top=1) == [((6, 4, 6), 8)]
    assert L3.frequent_patterns(mols, 'angles')[:2] == [((6, 4, 6, 4, 6), 8), ((6, 1, 6, 1, 6), 3)]
    assert L3.frequent_patterns(mols, 'dihedrals') == [((6, 4, 6, 4, 6, 4, 6), 8), ((6, 1, 6, 2, 7, 1, 8), 1)]
    assert L3.frequent_patterns([], 'angles') == []


def test_stats_npz_round_trip_add_counts_and_jsd(tmp_path):
    spec = L3.Local3DSpec(lengths=['C-C', 'C:C'], angles=['C:C:C', 'C-C-C'], dihedrals=['C:C:C:C'])
    a, b = L3.Local3DStats.from_ref([TRIANGLE, SQUARE], spec), L3.Local3DStats.from_ref([SQUARE, CHAIN], spec)
    s = a + b
    assert np.array_equal(s.hist, a.hist + b.hist) and np.array_equal(s.n_items, a.n_items + b.n_items)
    assert s.n_items.tolist() == [3 + 4 + 4 + 3, 3 + 4 + 4 + 2, 0 + 4 + 4 + 1]
    assert s.counts('lengths', 'C:C').sum() == 8 and s.counts('angles', 'C:C:C')[90] == 8 and s.counts('dihedrals', 'C:C:C:C')[90] == 8
    path = str(tmp_path / 'stats.npz')
    s.save(path)
    t = L3.Local3DStats.load(path)
    assert t.spec == spec and np.array_equal(t.hist, s.hist) and np.array_equal(t.outside, s.outside) and np.array_equal(t.n_items, s.n_items)
    j = a.jsd(b)
    assert j['lengths']['patterns']['C:C'] == 0.0                       # both hold squares only: the same distribution
    assert j['angles']['patterns']['C:C:C'] == 0.0 and np.isnan(j['angles']['patterns']['C-C-C'])   # b has no C-C-C angle
    assert j['angles']['mean'] == 0.0 and set(j) == set(L3.KINDS)
    with pytest.raises(ValueError):
        a + L3.Local3DStats(L3.Local3DSpec(lengths=['C-C']))
    assert 'C:C:C:C' in L3.compare_table(a, b)


def test_command_line_stats_ref_and_compare(tmp_path, capsys):
    import torch
    (tmp_path / 'p.yml').write_text("lengths: ['C-C', 'C:C']\nangles: ['C:C:C']\nlength_bins: [0.5, 2.5, 20]\n")
    torch.save({'finished': [TRIANGLE, SQUARE], 'failed': [CHAIN]}, tmp_path / 'samples_all.pt')
    out = str(tmp_path / 'a.npz')
    assert L3.main(['stats', str(tmp_path / 'samples_all.pt'), '--patterns', str(tmp_path / 'p.yml'), '--out', out, '--ref']) == 0
    st = L3.Local3DStats.load(out)
    assert st.spec.bins['lengths'] == (0.5, 2.5, 20) and st.n_items.tolist() == [7, 7, 4] and st.counts('lengths', 'C-C').sum() == 3
    assert L3.main(['compare', out, out]) == 0
    text = capsys.readouterr().out
    assert 'C:C:C' in text and '0.0000' in text


def test_entry_point_option_the_flag_wins_and_absence_changes_nothing():
    ap = sample_drug3d.build_parser()
    base = ['--config', 'c.yml']
    assert ap.parse_args(base).local3d is None
    assert ap.parse_args(base + ['--local3d', 'p.yml']).local3d == 'p.yml'
    assert sample_drug3d.local3d_option(None, {}) is None
    assert sample_drug3d.local3d_option(None, {'local3d': 'from_yaml.yml'}) == 'from_yaml.yml'
    assert sample_drug3d.local3d_option('flag.yml', {'local3d': 'from_yaml.yml'}) == 'flag.yml'
    assert sample_drug3d.local3d_option('flag.yml', {}) == 'flag.yml'
    # every other argument keeps its name and default
    with_flag, without = vars(ap.parse_args(base + ['--local3d', 'p.yml'])), vars(ap.parse_args(base))
    assert {k: v for k, v in with_flag.items() if k != 'local3d'} == {k: v for k, v in without.items() if k != 'local3d'}
    assert set(without) == {'config', 'outdir', 'device', 'batch_size', 'recipe_weights', 'num_mols', 'scaffold', 'num_steps', 'resample',
                            'jump_length', 'accept', 'largest_fragment', 'local3d'}


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/local3d_host_check.cpp over csrc/mdx_local3d_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('local3d_host_check', tmp_path)
