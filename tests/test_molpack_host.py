"""Host tests of moldiff_amd/molpack.py: the one parser and packer of molecule dicts behind local3d, similarity, rings and groups, and
the one results table (``Layout``, ``stack``, ``concat``, ``mol_slice``) behind rings, groups, kekule, canon and framework.
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


# ---- the results table: a made-up layout, none of the five modules' -----------------------------------------------------------------

TOY = molpack.Layout(mol=('score', 'tag', 'hist', 'n_atoms', 'n_bonds'), atom=('colour',), bond=('order',), index=('ends',), pos=('where',),
                     optional=('mark',), wide=('hist',), int64=('tag',))
W = {'hist': 3}
I32, I64, F32 = np.int32, np.int64, np.float32


def toy_ref(score, tag, hist, colour, order, ends, where, mark=None):
    r = {'score': score, 'tag': tag, 'hist': np.asarray(hist, dtype=I32), 'n_atoms': len(colour), 'n_bonds': len(order),
         'colour': np.asarray(colour, dtype=I32), 'order': np.asarray(order, dtype=I32), 'ends': np.asarray(ends, dtype=I32).reshape(2, len(order)),
         'where': np.asarray(where, dtype=F32).reshape(len(colour), 3)}
    if mark is not None:
        r['mark'] = np.asarray(mark, dtype=I32)
    return r


def toy_refs(marked=True):
    m = (lambda *v: list(v)) if marked else (lambda *v: None)
    return [toy_ref(5, -(1 << 40), [1, 0, 2], [7], [], [[], []], [[1, 2, 3]], m(9)),
            toy_ref(6, (1 << 40) + 1, [0, 4, 0], [1, 2, 3], [2, 1], [[0, 1], [1, 2]], [[0, 0, 0], [0, 0, 1.5], [0, 2, 0]], m(8, 7, 6)),
            toy_ref(-1, 3, [9, 9, 9], [4, 5], [3], [[1], [0]], [[4, 4, 4], [5, 5, 5]], m(5, 4))]


def same_table(got, want):
    assert list(got) == list(want)
    for k, (dtype, value) in want.items():
        value = np.asarray(value)
        assert isinstance(got[k], np.ndarray) and got[k].dtype == dtype and got[k].shape == value.shape and np.array_equal(got[k], value), k


def test_ptr_is_the_exclusive_running_sum():
    for counts, want in (([], []), ([3], [0]), ([2, 0, 5, 1], [0, 2, 2, 7]), (np.asarray([4, 4], dtype=np.int32), [0, 4])):
        got = molpack.ptr(counts)
        assert got.dtype == I32 and got.shape == (len(want),) and got.tolist() == want


def test_stack_of_nothing_of_a_bondless_molecule_and_of_three():
    z = lambda *shape: np.zeros(shape)
    nothing = {'score': (I32, z(0)), 'tag': (I64, z(0)), 'hist': (I32, z(0, 3)), 'n_atoms': (I32, z(0)), 'n_bonds': (I32, z(0)),
               'colour': (I32, z(0)), 'order': (I32, z(0)), 'where': (F32, z(0, 3)), 'ends': (I32, z(2, 0)), 'atom_ptr': (I32, z(0)),
               'bond_ptr': (I32, z(0))}
    same_table(molpack.stack([], TOY, W), nothing)
    items = list(nothing.items())
    same_table(molpack.stack([], TOY, W, optional=('mark',)), dict(items[:6] + [('mark', (I32, z(0)))] + items[6:]))
    same_table(molpack.stack(toy_refs()[:1], TOY, W, optional=('mark',)),
               {'score': (I32, [5]), 'tag': (I64, [-(1 << 40)]), 'hist': (I32, [[1, 0, 2]]), 'n_atoms': (I32, [1]), 'n_bonds': (I32, [0]),
                'colour': (I32, [7]), 'mark': (I32, [9]), 'order': (I32, z(0)), 'where': (F32, [[1, 2, 3]]), 'ends': (I32, z(2, 0)),
                'atom_ptr': (I32, [0]), 'bond_ptr': (I32, [0])})
    three = {'score': (I32, [5, 6, -1]), 'tag': (I64, [-(1 << 40), (1 << 40) + 1, 3]), 'hist': (I32, [[1, 0, 2], [0, 4, 0], [9, 9, 9]]),
             'n_atoms': (I32, [1, 3, 2]), 'n_bonds': (I32, [0, 2, 1]), 'colour': (I32, [7, 1, 2, 3, 4, 5]), 'mark': (I32, [9, 8, 7, 6, 5, 4]),
             'order': (I32, [2, 1, 3]), 'where': (F32, [[1, 2, 3], [0, 0, 0], [0, 0, 1.5], [0, 2, 0], [4, 4, 4], [5, 5, 5]]),
             'ends': (I32, [[0, 1, 1], [1, 2, 0]]), 'atom_ptr': (I32, [0, 1, 4]), 'bond_ptr': (I32, [0, 0, 2])}
    same_table(molpack.stack(toy_refs(), TOY, W, optional=('mark',)), three)
    del three['mark']
    same_table(molpack.stack(toy_refs(marked=False), TOY, W), three)
    # a position key is held only when every ref holds it
    refs = toy_refs(marked=False)
    del refs[1]['where']
    del three['where']
    same_table(molpack.stack(refs, TOY, W), three)


def test_concat_equals_stack_of_the_joined_refs():
    refs = toy_refs()
    stack = lambda rs: molpack.stack(rs, TOY, W, optional=('mark',))
    whole = {k: (v.dtype, v) for k, v in stack(refs).items()}
    for cut in (1, 2, 0, 3):                                        # 0 and 3: one part is empty
        same_table(molpack.concat([stack(refs[:cut]), stack(refs[cut:])], TOY), whole)
    same_table(molpack.concat([stack(refs[:1]), stack([]), stack(refs[1:2]), stack(refs[2:])], TOY), whole)
    same_table(molpack.concat([{k: torch.from_numpy(v) for k, v in stack(refs).items()}], TOY), whole)
    with pytest.raises(KeyError, match='mark'):
        molpack.concat([stack(refs[:2]), molpack.stack(toy_refs(marked=False)[2:], TOY, W)], TOY)


def test_mol_slice_gives_every_ref_back():
    for marked in (True, False):
        refs = toy_refs(marked)
        table = molpack.stack(refs, TOY, W, optional=('mark',) if marked else ())
        for m, ref in enumerate(refs):
            got = molpack.mol_slice(table, m, TOY)
            assert set(got) == set(ref)
            for k in ref:
                if k in ('score', 'tag', 'n_atoms', 'n_bonds'):
                    assert type(got[k]) is int and got[k] == ref[k], (m, k)
                else:
                    assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (m, k)


def test_a_layout_without_n_bonds_counts_bonds_by_bond_ptr_and_the_array_length():
    bare = molpack.Layout(mol=('n_atoms',), atom=('colour',), bond=('order',))
    assert not bare.has_n_bonds and bare.has_bond_ptr and TOY.has_n_bonds
    assert not molpack.Layout(mol=('n_atoms',), atom=('colour',)).has_bond_ptr
    refs = [{'n_atoms': 2, 'colour': np.asarray([1, 2], dtype=I32), 'order': np.asarray([5, 6, 7], dtype=I32)},
            {'n_atoms': 0, 'colour': np.zeros(0, dtype=I32), 'order': np.zeros(0, dtype=I32)},
            {'n_atoms': 1, 'colour': np.asarray([3], dtype=I32), 'order': np.asarray([8, 9], dtype=I32)}]
    whole = {'n_atoms': (I32, [2, 0, 1]), 'colour': (I32, [1, 2, 3]), 'order': (I32, [5, 6, 7, 8, 9]), 'atom_ptr': (I32, [0, 2, 2]),
             'bond_ptr': (I32, [0, 3, 3])}
    same_table(molpack.stack(refs, bare), whole)
    for cut in (0, 1, 2, 3):
        same_table(molpack.concat([molpack.stack(refs[:cut], bare), molpack.stack(refs[cut:], bare)], bare), whole)
    table = molpack.stack(refs, bare)
    assert [molpack.mol_slice(table, m, bare)['order'].tolist() for m in range(3)] == [[5, 6, 7], [], [8, 9]]
    # without any per-bond key there is no bond_ptr either
    same_table(molpack.stack(refs, molpack.Layout(mol=('n_atoms',), atom=('colour',))),
               {'n_atoms': (I32, [2, 0, 1]), 'colour': (I32, [1, 2, 3]), 'atom_ptr': (I32, [0, 2, 2])})
