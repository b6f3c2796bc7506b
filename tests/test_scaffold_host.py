"""Host side of scaffold-constrained sampling: the mol-block reader, the Scaffold container's rules and validation, and the inputs
(with their float64 restatement) that tests/test_gpu_scaffold.py checks the merge kernel against.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from moldiff_amd import Scaffold, _lib
from moldiff_amd.postprocess import FeaturizeMol
from moldiff_amd.sample_drug3d import mol_block, read_mol_block
from moldiff_amd.scaffold import scaffold_for_sizes
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)

# ---- inputs of the GPU "merged rows against the formula" test, shared so that the exclusion cap is checked for exactly them --------
FORMULA_SIZES = [24, 19, 22, 17, 25, 21, 23, 18, 20, 26, 16, 22]   # 253 atoms, 2,683 half-edges
FORMULA_SEED = 4242
MARGIN = 1e-4        # the fp64 class test may skip rows whose two best Gumbel-plus-logit scores lie closer than this
SKIP_CAP = 0.005     # ... but no more than this share of the rows


def formula_levels(T):
    return (T - 1, T // 2, 0)


def formula_inputs(T=1000):
    """Known molecule, masks (about half the atoms fixed; half-edges by the default rule) and explicit noise per level."""
    g = U.rng(FORMULA_SEED)
    bn, hei, bh, _, _ = U.graph_from_sizes(FORMULA_SIZES)
    N, Eh = int(bn.numel()), int(bh.numel())
    inp = {'bn': bn, 'hei': hei, 'bh': bh,
           'node_mask': torch.from_numpy(g.random(N) < 0.5),
           'node_type': torch.from_numpy(g.integers(0, 8, N)), 'halfedge_type': torch.from_numpy(g.integers(0, 6, Eh)),
           'node_pos': U.t32(2.0 * g.standard_normal((N, 3))), 'noise': {}}
    inp['halfedge_mask'] = inp['node_mask'][hei[0]] & inp['node_mask'][hei[1]]
    for k in formula_levels(T):
        inp['noise'][k] = (U.t32(g.standard_normal((N, 3))), U.t32(g.random((N, 8), dtype=np.float32)),
                           U.t32(g.random((Eh, 6), dtype=np.float32)))
    return inp


def classes_fp64(q_mats, v0, k, u):
    """float64 restatement of q(v_k | v_0): Gumbel-max over log(onehot(v0) Qbar[k] + 1e-30).clamp_min(-32) with the uniforms u.
    -> (class ids, margin between the two best scores)"""
    Q = q_mats[k].double()
    logits = torch.log(Q[v0] + 1e-30).clamp_min(-32.0)            # onehot(v0) @ Q = row v0 of Q
    z = -torch.log(-torch.log(u.double() + 1e-30) + 1e-30) + logits
    top = z.topk(2, dim=-1).values
    return z.argmax(-1), top[:, 0] - top[:, 1]


def test_fp64_class_test_skips_at_most_half_a_percent_of_its_rows():
    m = U.moldiff('MolDiff_simple')
    inp = formula_inputs(m.num_timesteps)
    for k in formula_levels(m.num_timesteps):
        _, un, uh = inp['noise'][k]
        nm, hm = inp['node_mask'], inp['halfedge_mask']
        _, mn = classes_fp64(m.node_transition.q_mats, inp['node_type'][nm], k, un[nm])
        _, mh = classes_fp64(m.edge_transition.q_mats, inp['halfedge_type'][hm], k, uh[hm])
        margins = torch.cat([mn, mh])
        share = float((margins < MARGIN).double().mean())
        print(f'level {k}: {int(margins.numel())} fixed rows, share within {MARGIN} of a tie = {share:.2e}')
        assert margins.numel() > 500 and share <= SKIP_CAP


# ---- mol block ------------------------------------------------------------------------------------------------------------------

def _info():
    idx = np.array([[0, 1, 2, 2, 0], [1, 2, 3, 4, 4]], dtype=np.int64)
    bt = np.array([1, 2, 4, 1, 3], dtype=np.int64)
    return {'element': np.array([6, 7, 8, 17, 16]),
            'atom_pos': np.array([[0.12345, -1.5, 2.0], [1.00004, 0.0, -0.33336], [-12.5, 3.25, 0.00005], [4.0, 5.0, 6.0],
                                  [-0.1, 0.2, -0.3]], dtype=np.float32),
            'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}


def test_read_mol_block_round_trips_elements_coordinates_and_bonds():
    info = _info()
    back = read_mol_block(mol_block(info))
    assert np.array_equal(back['element'], info['element'])
    assert back['atom_pos'].shape == (5, 3) and np.abs(back['atom_pos'] - info['atom_pos']).max() <= 0.5e-4 + 1e-6
    assert np.array_equal(back['bond_index'], info['bond_index']) and np.array_equal(back['bond_type'], info['bond_type'])
    assert mol_block(back) == mol_block(info)            # and the printed form is a fixed point
    empty = {'element': np.array([6, 6]), 'atom_pos': np.zeros((2, 3), np.float32), 'bond_index': np.zeros((2, 0), np.int64),
             'bond_type': np.zeros(0, np.int64)}
    assert read_mol_block(mol_block(empty))['bond_index'].shape == (2, 0)
    with pytest.raises(ValueError, match='unknown element'):
        read_mol_block(mol_block(info).replace(' Cl ', ' Br '))
    with pytest.raises(ValueError, match='V2000'):
        read_mol_block('no counts line here\n')


# ---- the container ----------------------------------------------------------------------------------------------------------------

def _batch():
    # three molecules of 3, 2 and 4 atoms; half-edges per molecule in row-major upper-triangle order:
    #   mol 0: (0,1) (0,2) (1,2)   mol 1: (3,4)   mol 2: (5,6) (5,7) (5,8) (6,7) (6,8) (7,8)
    bn, hei, bh, _, _ = U.graph_from_sizes([3, 2, 4])
    assert hei.tolist() == [[0, 0, 1, 3, 5, 5, 5, 6, 6, 7], [1, 2, 2, 4, 6, 7, 8, 7, 8, 8]]
    node_mask = torch.tensor([True, True, False, True, True, True, False, True, True])
    sc = Scaffold(node_mask, torch.zeros(9, dtype=torch.int64), torch.zeros(9, 3), torch.zeros(10, dtype=torch.int64))
    return hei, sc


def test_default_halfedge_mask_is_both_end_points_fixed():
    hei, sc = _batch()
    nm, nt, npos, ht, hm = sc.resolve(9, hei, 8, 6)
    assert hm.tolist() == [True, False, False, True, False, True, True, False, False, True]
    assert hm.dtype == torch.bool and nm.dtype == torch.bool and all(t.is_contiguous() for t in (nm, nt, npos, ht, hm))
    sc.halfedge_mask = torch.tensor([True, False, False, False, False, True, False, False, False, False])   # a subset is allowed
    assert sc.resolve(9, hei, 8, 6)[4].tolist() == sc.halfedge_mask.tolist()


def test_validation_errors():
    hei, sc = _batch()
    import dataclasses
    new = lambda **kw: dataclasses.replace(sc, **kw)
    with pytest.raises(ValueError, match='shape'):
        new(node_pos=torch.zeros(8, 3)).resolve(9, hei, 8, 6)
    with pytest.raises(ValueError, match='shape'):
        new(halfedge_type=torch.zeros(9, dtype=torch.int64)).resolve(9, hei, 8, 6)
    with pytest.raises(TypeError, match='int64'):
        new(node_type=torch.zeros(9, dtype=torch.int32)).resolve(9, hei, 8, 6)
    with pytest.raises(TypeError, match='bool'):
        new(node_mask=sc.node_mask.to(torch.uint8)).resolve(9, hei, 8, 6)
    nt = torch.zeros(9, dtype=torch.int64)
    nt[2] = 99                                           # a free row: ignored ...
    new(node_type=nt).resolve(9, hei, 8, 6)
    with pytest.raises(ValueError, match='node_type'):   # ... unless the scaffold carries the whole start molecule
        new(node_type=nt).resolve(9, hei, 8, 6, every_row=True)
    nt[3] = 8
    with pytest.raises(ValueError, match=r'node_type: class id outside \[0, 8\)'):
        new(node_type=nt).resolve(9, hei, 8, 6)
    ht = torch.zeros(10, dtype=torch.int64)
    ht[0] = -1
    with pytest.raises(ValueError, match='halfedge_type'):
        new(halfedge_type=ht).resolve(9, hei, 8, 6)
    hm = torch.zeros(10, dtype=torch.bool)
    hm[1] = True                                         # (0, 2): atom 2 is free
    with pytest.raises(ValueError, match='free end point'):
        new(halfedge_mask=hm).resolve(9, hei, 8, 6)


def test_scaffold_for_sizes_puts_the_scaffold_first_in_every_molecule():
    info = read_mol_block(mol_block(_info()))
    sizes = [5, 7, 6]
    sc = scaffold_for_sizes(info, sizes, FEAT)
    bn, hei, bh, _, _ = U.graph_from_sizes(sizes)
    nm, nt, npos, ht, hm = sc.resolve(int(bn.numel()), hei, 8, 6)
    off = 0
    for n in sizes:
        assert nm[off:off + 5].all() and not nm[off + 5:off + n].any()
        assert nt[off:off + 5].tolist() == [0, 1, 2, 6, 5]                       # C N O Cl S in the featurizer's list
        assert float(npos[off:off + 5].mean(0).abs().max()) < 1e-6               # centred on the scaffold's own centroid
        assert torch.allclose(npos[off + 1] - npos[off], torch.from_numpy(info['atom_pos'][1] - info['atom_pos'][0]), atol=1e-6)
        off += n
    want = {(0, 1): 1, (1, 2): 2, (2, 3): 4, (2, 4): 1, (0, 4): 3}
    off = 0
    for m, n in enumerate(sizes):
        sel = bh == m
        for (i, j), t, fixed in zip((hei[:, sel] - off).T.tolist(), ht[sel].tolist(), hm[sel].tolist()):
            assert fixed == (j < 5)                                              # i < j: internal half-edges only, "no bond" included
            assert t == (want.get((i, j), 0) if fixed else 0)
        off += n
    with pytest.raises(ValueError, match='at least'):
        scaffold_for_sizes(info, [5, 4], FEAT)
    bad = dict(info, element=np.array([6, 7, 8, 17, 35]))
    with pytest.raises(ValueError, match='35'):
        scaffold_for_sizes(bad, sizes, FEAT)


def test_sampler_arguments_are_checked_before_any_device_work():
    m = U.moldiff('MolDiff_simple')
    bn, hei, bh, _, _ = U.graph_from_sizes([3, 2, 4])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.sampler(3, bn, hei, bh, scaffold=_batch()[1])


def test_merge_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'moldiff_hip.h')).read()
    assert 'mdx_scaffold_merge' in set(re.findall(r'\b(mdx_[a-z_0-9]+)\s*\(', hdr))
    assert 'mdx_scaffold_merge' in _lib.EXPORTS
    L = _lib.lib()
    assert L.mdx_scaffold_merge.argtypes is not None and len(L.mdx_scaffold_merge.argtypes) == 13
    # argument checks that need no device: a null handle and class counts outside 2..8
    tb = _lib.MdxScaffoldTables(None, None, None, 9, 6, 1000)
    assert L.mdx_scaffold_merge(None, tb, 0, None, None, None, 0.0, None, None, None, None, None, None) == 1
