"""Host tests of moldiff_amd/molpack.py: the one parser and packer of molecule dicts behind local3d, similarity, rings and groups.
The expected arrays are written out; no GPU."""
import numpy as np
import pytest
import torch

from moldiff_amd import molpack

ELEMENTS = (6, 7, 8)


def mol(ele, bonds, types=None, pos=None):
    """every bond once and then flipped, as decode_batch leaves it"""
    idx = np.asarray(bonds, dtype=np.int64).reshape(-1, 2).T
    bt = np.asarray(types if types is not None else [1] * len(bonds), dtype=np.int64)
    out = {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}
    if pos is not None:
        out['atom_pos'] = np.asarray(pos, dtype=np.float64)
    return out


CON = mol([6, 8, 7], [(0, 1), (1, 2)], [1, 2], [[0, 0, 0], [1.5, 0, 0], [1.5, 0.25, -2]])
LONE = {'element': np.asarray([7]), 'atom_pos': np.asarray([[3.0, 4.0, 5.0]])}          # no bond_index key at all


def same(p, want):
    assert list(p) == list(want)
    for k, (dtype, value) in want.items():
        assert p[k].dtype == dtype and p[k].shape == np.asarray(value).shape and np.array_equal(p[k], value), k
        assert p[k].flags['C_CONTIGUOUS'], k


def test_mol_graph_drops_the_flipped_half_and_maps_elements():
    cls, bi, bt = molpack.mol_graph(CON, ELEMENTS)
    assert cls.dtype == np.int64 and cls.tolist() == [0, 2, 1]
    assert bi.dtype == np.int64 and bi.tolist() == [[0, 1], [1, 2]] and bt.tolist() == [1, 2]
    ele, bi2, bt2 = molpack.mol_graph(CON)                       # without a table: the atomic numbers themselves
    assert ele.tolist() == [6, 8, 7] and np.array_equal(bi2, bi) and np.array_equal(bt2, bt)
    for info in (LONE, dict(LONE, bond_index=np.zeros((2, 0), dtype=np.int64), bond_type=np.zeros(0, dtype=np.int64))):
        cls, bi, bt = molpack.mol_graph(info, ELEMENTS)
        assert cls.tolist() == [1] and bi.shape == (2, 0) and bt.shape == (0,) and bi.dtype == bt.dtype == np.int64


def test_unknown_element_raises():
    with pytest.raises(ValueError, match=r"element\(s\) \[5, 9\] are not among the spec's atomic numbers"):
        molpack.mol_graph(mol([6, 9, 5, 9], [(0, 1)]), ELEMENTS)
    with pytest.raises(ValueError, match='element'):
        molpack.pack_mols([CON, mol([16], [])], ELEMENTS)


def test_pack_two_molecules_with_and_without_positions():
    i32, f32 = np.int32, np.float32
    want = {'atom_ptr': (i32, [0, 3]), 'bond_ptr': (i32, [0, 2]), 'n_atoms': (i32, [3, 1]), 'n_bonds': (i32, [2, 0]),
            'atom_type': (i32, [0, 2, 1, 1]), 'bond_type': (i32, [1, 2]), 'bond_index': (i32, [[0, 1], [1, 2]])}
    same(molpack.pack_mols([CON, LONE], ELEMENTS), want)
    items = list(want.items())
    with_pos = dict(items[:5] + [('atom_pos', (f32, [[0, 0, 0], [1.5, 0, 0], [1.5, 0.25, -2], [3, 4, 5]]))] + items[5:])
    same(molpack.pack_mols([CON, LONE], ELEMENTS, positions=True), with_pos)
    # the second molecule's bonds keep molecule-local indices and start at bond_ptr
    p = molpack.pack_mols([LONE, CON, CON], ELEMENTS)
    assert p['atom_ptr'].tolist() == [0, 1, 4] and p['bond_ptr'].tolist() == [0, 0, 2] and p['bond_index'].tolist() == [[0, 1, 0, 1], [1, 2, 1, 2]]


def test_pack_without_any_bond_keeps_one_spare_column():
    i32, f32 = np.int32, np.float32
    empty = lambda *shape: np.zeros(shape, dtype=np.int64)
    same(molpack.pack_mols([], ELEMENTS, positions=True),
         {'atom_ptr': (i32, empty(0)), 'bond_ptr': (i32, empty(0)), 'n_atoms': (i32, empty(0)), 'n_bonds': (i32, empty(0)),
          'atom_type': (i32, empty(0)), 'atom_pos': (f32, empty(0, 3)), 'bond_type': (i32, empty(0)), 'bond_index': (i32, [[0], [0]])})
    same(molpack.pack_mols([LONE], ELEMENTS),
         {'atom_ptr': (i32, [0]), 'bond_ptr': (i32, [0]), 'n_atoms': (i32, [1]), 'n_bonds': (i32, [0]), 'atom_type': (i32, [1]),
          'bond_type': (i32, empty(0)), 'bond_index': (i32, [[0], [0]])})
    p = molpack.pack_mols([LONE, mol([6, 6], []), {'element': np.zeros(0, dtype=np.int64)}], ELEMENTS)
    assert p['bond_index'].shape == (2, 1) and p['n_bonds'].tolist() == [0, 0, 0] and p['n_atoms'].tolist() == [1, 2, 0]
    assert p['atom_ptr'].tolist() == [0, 1, 3] and p['atom_type'].tolist() == [1, 0, 0] and 'atom_pos' not in p


def test_check_simple():
    molpack.check_simple(molpack.pack_mols([CON, LONE, CON], ELEMENTS))
    molpack.check_simple(molpack.pack_mols([], ELEMENTS))
    with pytest.raises(ValueError, match='molecule 1: two bonds between the same pair of atoms'):
        molpack.check_simple(molpack.pack_mols([CON, mol([6, 6, 6], [(0, 1), (1, 2), (1, 0)])], ELEMENTS))
    # bonds that are ignored never count: twice the same bond out of range, twice the same self-bond, beside one real bond
    molpack.check_simple(molpack.pack_mols([mol([6, 6], [(0, 5), (0, 5), (1, 1), (1, 1), (-1, 0), (-1, 0), (0, 1)])], ELEMENTS))
    # the pair is what counts, not the molecule: the same local indices in two molecules are two different bonds
    molpack.check_simple(molpack.pack_mols([mol([6, 6], [(0, 1)]), mol([6, 6], [(0, 1)])], ELEMENTS))


def test_host_helpers_and_files(tmp_path):
    res = {'a': torch.arange(6, dtype=torch.int32).reshape(2, 3).t(), 'b': np.asarray(['x', 'yz'])}
    h = molpack.to_host(res)
    assert isinstance(h['a'], np.ndarray) and h['a'].flags['C_CONTIGUOUS'] and h['a'].tolist() == [[0, 3], [1, 4], [2, 5]]
    assert molpack.host([1, 2]).tolist() == [1, 2]
    path = str(tmp_path / 'r.npz')
    molpack.save_npz(res, path)
    back = molpack.load_npz(path)
    assert set(back) == {'a', 'b'} and np.array_equal(back['a'], h['a']) and back['b'].tolist() == ['x', 'yz']
    torch.save({'finished': [CON, LONE], 'failed': [LONE]}, tmp_path / 'samples_all.pt')
    torch.save([CON], tmp_path / 'plain.pt')
    assert len(molpack.load_mols(tmp_path / 'samples_all.pt', 'finished')) == 2 and len(molpack.load_mols(tmp_path / 'samples_all.pt', 'failed')) == 1
    assert len(molpack.load_mols(tmp_path / 'plain.pt', 'finished')) == 1
    with pytest.raises(ValueError, match='2\\^31'):
        molpack.to_device(dict(molpack.pack_mols([LONE], ELEMENTS), n_bonds=np.asarray([1 << 31], dtype=np.int64)), 'cpu')
    d = molpack.to_device(molpack.pack_mols([CON, LONE], ELEMENTS, positions=True), 'cpu')
    cm = molpack.CompactMols.from_packed(d)
    assert (cm.B, cm.N_cap, cm.Eh_stride) == (2, 4, 2) and cm.atom_pos.shape == (4, 3) and cm.bond_index is d['bond_index']
    assert molpack.CompactMols.from_packed(molpack.to_device(molpack.pack_mols([], ELEMENTS), 'cpu'))[:1] == (0,)
