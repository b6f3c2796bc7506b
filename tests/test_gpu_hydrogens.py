"""GPU tests of the explicit-hydrogen placement (mdx_mol_hydrogens through hydrogens.addh_mols, hydrogens.launch,
FeaturizeMol.addh_batch and the sampling entry point's --hydrogens).  The oracle is the plain restatement ``addh_ref``.  Integers are
compared exactly; ``h_pos`` and ``min_contact`` to 1e-8 Angstrom absolute: float64 (1.1e-16) at coordinate scale 1e2, amplified by
at most 1 / deg_tol = 1e3 over about a hundred operations is 1e-9, and the bound leaves a margin of ten for fused contraction.  The
largest difference seen on an MI355X is 0 (profiles/hydrogens_accuracy.txt): the kernel is built without contraction and repeats the
restatement operation by operation.  A random molecule with a decision within 1e-6 of its threshold would be left out; the host test
asserts that the seeded set holds none."""
import json
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import hydrogens as H
from moldiff_amd import kekule as K
from moldiff_amd.harness import default_config, placeholder_from_sizes
from moldiff_amd.postprocess import FeaturizeMol
from . import hydrogens_cases as HC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
TOL = 1e-8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = H.MOL_KEYS + H.ATOM_KEYS + ('atom_ptr',)


def same(got, ref, what, skip=()):
    """integers exact, floats within TOL -> the largest float difference.  skip: molecules left out of every comparison"""
    got = molpack.to_host(got)
    assert set(got) == set(ref), (what, set(got) ^ set(ref))
    keep_m = np.asarray([m not in skip for m in range(len(ref['status']))], dtype=bool)
    keep_a = np.repeat(keep_m, ref['n_atoms'])
    worst = 0.0
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape, ref[k].shape)
        keep = keep_m if len(ref[k]) == len(keep_m) and k not in H.ATOM_KEYS + ('h_pos',) else keep_a
        g, r = got[k][keep], ref[k][keep]
        if k in H.FLOAT_KEYS:
            inf = np.isinf(r)
            assert np.array_equal(np.isinf(g), inf), (what, k)
            diff = float(np.abs(g[~inf] - r[~inf]).max(initial=0.0))
            print(what, k, 'max abs diff', diff)
            assert diff <= TOL, (what, k, diff)
            worst = max(worst, diff)
        else:
            bad = np.flatnonzero(g != r)
            assert len(bad) == 0, (what, k, bad[:8], g[bad[:8]], r[bad[:8]])
    return worst


def test_the_named_molecules_as_one_batch():
    names, mols, n_h, order = HC.named_lists()
    want = HC.named_ref()
    got = H.addh_mols(mols, DEV, n_h, order)
    worst = same(got, want, 'named')
    at = names.index
    g = molpack.to_host(got)
    assert g['n_degenerate'][[at('flat_ch'), at('collinear_ch2'), at('coincident')]].tolist() == [1, 1, 2] and g['n_no_room'][at('no_room')] == 1
    out = os.path.join(ROOT, 'profiles', 'hydrogens_accuracy.txt')
    if os.access(os.path.dirname(out), os.W_OK):
        with open(out, 'w') as f:
            f.write('mdx_mol_hydrogens against addh_ref, the %d named molecules as one batch (tests/test_gpu_hydrogens.py, MI355X)\n' % len(mols))
            f.write('largest absolute difference of h_pos and min_contact: %.3e Angstrom (bound %.0e); every integer output equal\n' % (worst, TOL))
    # the Kekulé counts made on the device give the same as the ones made on the host
    plain = [m for m, k in zip(mols, names) if k not in ('pyridinium', 'no_room', 'clamped', 'bad_bond')]
    kek, res = H.addh_mols(plain, DEV, with_kekule=True)
    same(res, H.stack_ref(plain), 'device kekule')
    assert np.array_equal(molpack.to_host(kek)['kek_h'], K.stack_ref(plain)['kek_h'])


def test_the_random_batch_its_reverse_and_a_second_run():
    mols, n_h, order = HC.random_set()
    left_out = {m for m in range(len(mols)) if H.near_threshold(mols[m], n_h[m], order[m], band=1e-6)}
    assert not left_out
    got = molpack.to_host(H.addh_mols(mols, DEV, n_h, order))
    same(got, HC.random_ref(), 'random', skip=left_out)
    back = molpack.to_host(H.addh_mols(mols[::-1], DEV, n_h[::-1], order[::-1]))
    for m in range(len(mols)):
        a, b = H.mol_result(got, m), H.mol_result(back, len(mols) - 1 - m)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), m
    again = molpack.to_host(H.addh_mols(mols, DEV, n_h, order))
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def _operands(mols, n_h, order):
    p = molpack.pack_mols(mols, ELEMENTS, positions=True)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    cat = lambda xs: torch.from_numpy(np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1) for x in xs] + [np.zeros(1, dtype=np.int32)])).to(DEV)
    return p, molpack.CompactMols.from_packed(d), cat(n_h), cat(order)


def test_select_sizes_a_molecule_past_the_arrays_and_other_tables():
    sizes = (0, 1, 255, 256, 257)
    mols = [HC.chain(n) for n in sizes] + [HC.named()['formamide'][0], HC.named()['propane'][0]]
    counts = [HC.kekule_counts(m) for m in mols]
    n_h, order = [c[0] for c in counts], [c[1] for c in counts]
    want = H.stack_ref(mols, n_h, order)
    assert want['status'].tolist() == [0, 0, 0, 0, 1, 0, 0] and want['n_h_placed'].tolist() == [0, 4, 512, 514, 0, 3, 8]
    assert want['min_contact'][:2].tolist() == [np.inf, np.inf] and want['min_contact'][4] == 0.0
    same(H.addh_mols(mols, DEV, n_h, order), want, 'sizes')
    # select: the masked molecule has status 0 and zeros everywhere, its slots included; the others are unchanged
    p, cm, h_dev, o_dev = _operands(mols, n_h, order)
    N = int(p['n_atoms'].sum())
    masked = 5
    select = torch.ones(len(mols), dtype=torch.int32, device=DEV)
    select[masked] = 0
    ref = {k: v.copy() for k, v in want.items()}
    a0, na = int(p['atom_ptr'][masked]), int(p['n_atoms'][masked])
    for k in H.STAT_KEYS + ('min_contact',):
        ref[k][masked] = 0
    for k in H.ATOM_KEYS + ('h_pos',):
        ref[k][a0:a0 + na] = 0
    out = molpack.to_host(H.launch(cm, h_dev, o_dev, select=select))
    for k in H.STAT_KEYS:
        assert np.array_equal(out[k], ref[k]), k
    for k in H.ATOM_KEYS:
        assert np.array_equal(out[k][:N], ref[k]), k
    assert np.abs(out['h_pos'][:N] - ref['h_pos']).max() <= TOL and np.array_equal(np.isinf(out['min_contact']), np.isinf(ref['min_contact']))
    assert out['min_contact'][masked] == 0.0 and not out['h_pos'][a0:a0 + na].any()
    # a molecule whose extent leaves the arrays: status 0, zeros, and nothing of it is written (the arrays hold a sentinel)
    short = cm._replace(N_cap=N - 1)                                    # the last molecule (propane) reaches past N_cap
    tb = H.HydrogenTables()
    hp = torch.full((N, 4, 3), 7.0, dtype=torch.float64, device=DEV)
    hc, fl = (torch.full((N,), 7, dtype=torch.int32, device=DEV) for _ in range(2))
    stats = torch.full((len(mols), len(H.STAT_KEYS)), 7, dtype=torch.int32, device=DEV)
    mc = torch.full((len(mols),), 7.0, dtype=torch.float64, device=DEV)
    ops, at = short.operands()
    _lib.check(_lib.lib().mdx_mol_hydrogens(*ops, None, at(cm.atom_pos), at(h_dev), at(o_dev), 7, 4, tb.xh_length.ctypes.data, tb.planar, 1e-3, 1.5,
                                            at(hp), at(hc), at(fl), at(stats), at(mc), _lib.stream()))
    torch.cuda.synchronize()
    last = len(mols) - 1
    a0 = int(p['atom_ptr'][last])
    assert stats[last].tolist() == [0] * len(H.STAT_KEYS) and float(mc[last]) == 0.0
    assert bool((hp[a0:] == 7.0).all()) and bool((hc[a0:] == 7).all()) and bool((fl[a0:] == 7).all())
    assert np.array_equal(hc[:a0].cpu().numpy(), want['h_count'][:a0]) and np.array_equal(stats[:last, 2].cpu().numpy(), want['n_h_placed'][:last])
    # no molecule, through the module and through the entry (accepted, nothing written); a refused call leaves the outputs alone
    got, ref = molpack.to_host(H.addh_mols([], DEV)), H.empty()
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape for k in ref)
    L = _lib.lib()
    call = lambda B, deg: L.mdx_mol_hydrogens(B, *ops[1:], None, at(cm.atom_pos), at(h_dev), at(o_dev), 7, 4, tb.xh_length.ctypes.data, tb.planar,
                                              deg, 1.5, at(hp), at(hc), at(fl), at(stats), at(mc), _lib.stream())
    stats.fill_(7)
    assert call(0, 1e-3) == 0 and call(len(mols), 2.0) == 1 and b'deg_tol' in L.mdx_last_error()
    torch.cuda.synchronize()
    assert bool((stats == 7).all())
    # another length table and another planar mask change the results as the reference says
    other = H.HydrogenTables(xh_length={**H.DEFAULT_XH_LENGTH, 6: 1.5, 7: 0.75}, planar=())
    want2 = H.stack_ref(mols, n_h, order, other)
    assert (want2['atom_flag'] != want['atom_flag']).any() and want2['min_contact'][5] != want['min_contact'][5]
    same(H.addh_mols(mols, DEV, n_h, order, other), want2, 'other tables')
    want3 = H.stack_ref(mols, n_h, order, clash_tol=2.4)
    assert want3['n_clash'].sum() > want['n_clash'].sum()
    same(H.addh_mols(mols, DEV, n_h, order, clash_tol=2.4), want3, 'other clash_tol')


def test_addh_batch_on_a_two_step_sample_equals_addh_mols_of_its_molecules():
    import moldiff_amd as M
    model = M.MolDiff(default_config('MolDiff_simple'), 8, 6).eval()
    model.load_state_dict(M.recipe_state_dict(model, 20230807), strict=True)
    model = model.to(DEV)
    sizes = [9, 14, 6, 11]
    ph = placeholder_from_sizes(sizes, DEV)
    out = model.sample(len(sizes), ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], seed=11, return_traj=False, num_steps=2)
    args = (out['pred'], ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], len(sizes))
    decoded = FEAT.decode_batch(*args)
    listed = molpack.to_host(H.addh_mols(decoded, DEV))
    assert listed['n_atoms'].sum() > 0
    select = torch.tensor([1, 0, 1, 1], device=DEV)
    for sel, masked in ((None, ()), (select, (1,))):
        kek, res = FEAT.addh_batch(*args, select=sel)
        res = molpack.to_host(res)
        for m in range(len(sizes)):
            zero = m in masked
            for k in H.MOL_KEYS + ('min_contact',):
                assert res[k][m] == (0 if zero else listed[k][m]), (k, m)
            a0, la, na = int(res['atom_ptr'][m]), int(listed['atom_ptr'][m]), len(decoded[m]['element'])
            for k in H.ATOM_KEYS + ('h_pos',):
                assert np.array_equal(res[k][a0:a0 + na], listed[k][la:la + na] * (not zero)), (k, m)
    with pytest.raises(ValueError, match='another featuriser'):
        FEAT.addh_batch(*args, H.HydrogenTables(atomic_numbers=(6, 7, 8)))


def test_entry_point_writes_the_all_atom_files(tmp_path):
    from moldiff_amd import rmsd
    from .test_gpu_kekule import _sample
    new = {'hydrogens.json', 'hydrogens.npz', 'samples_allatom.sdf'}
    d0, pool0 = _sample(tmp_path, 'abc', ['--largest_fragment', '0.2', '--kekulize'])
    assert not new & set(os.listdir(d0))
    d1, pool = _sample(tmp_path, 'bca', ['--largest_fragment', '0.2', '--hydrogens', '--clash_tol', '1.25'])     # implies --kekulize
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new) and new <= set(os.listdir(d1))
    assert len(pool['finished']) >= 2 and [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    saved = molpack.load_npz(os.path.join(d1, 'hydrogens.npz'))
    ref = H.stack_ref(pool['finished'], clash_tol=1.25)
    near = {m for m, info in enumerate(pool['finished'])
            if H.near_threshold(info, K.kekulize_ref(info)['kek_h'], K.kekulize_ref(info)['kek_order'], clash_tol=1.25)}
    assert len(near) <= 1
    same(saved, ref, 'entry point', skip=near)
    with open(os.path.join(d1, 'hydrogens.json')) as f:
        got = json.load(f)
    want = json.loads(json.dumps(H.summary(saved, 1.25)))
    assert got.keys() == want.keys() and all(got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]) for k in want)
    assert got['n_molecules'] == len(pool['finished']) and got['clash_tol'] == 1.25
    kek = K.stack_ref(pool['finished'])
    written = [k for k in range(len(pool['finished'])) if K.kekulizable(kek)[k] and (K.mol_result(kek, k)['kek_order'] >= 1).all()]
    back = rmsd.read_sdf(os.path.join(d1, 'samples_allatom.sdf'))
    assert len(back) == len(written)
    for b, k in zip(back, written):
        m = pool['finished'][k]
        assert np.array_equal(b['element'], m['element']) and np.array_equal(b['bond_index'], m['bond_index'])
    with open(os.path.join(d1, 'samples_allatom.sdf')) as f:
        blocks = [b for b in f.read().split('$$$$\n') if b.strip()]
    for b, k in zip(blocks, written):
        lines = b.splitlines()
        assert int(lines[3][0:3]) == len(pool['finished'][k]['element']) + int(saved['n_h_placed'][k])
