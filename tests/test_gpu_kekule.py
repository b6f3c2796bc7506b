"""GPU tests of the Kekulé assignment (mdx_mol_kekulize through kekule.kekulize_mols, kekule.launch, FeaturizeMol.kekulize_batch and the
sampling entry point's --kekulize / --accept kekule).  The oracle is the plain Python restatement ``kekulize_ref``; every output is an
integer that the definition makes unique, so every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import kekule as K
from moldiff_amd.harness import placeholder_from_sizes
from moldiff_amd.postprocess import FeaturizeMol
from .test_kekule_host import NAMED, grid, mol, random_aromatic, ring

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
OUT_KEYS = K.STAT_KEYS + K.ATOM_KEYS + K.BOND_KEYS

THREE = mol(6 + 5 + 6, ring(6) + ring(5, 6) + ring(6, 11) + [(5, 6, 1), (10, 11, 1)])     # benzene - all-carbon 5-ring - benzene
STAR = mol(5, [(0, 1, 4), (0, 2, 4), (0, 3, 4), (0, 4, 4)])                               # an atom with four aromatic bonds
NOISY = mol([7] + [6] * 5, [(0, 9, 4), (2, 2, 4)] + ring(6) + [(-1, 3, 2)])                 # pyridine with three ignored bonds
AMMONIUM = mol([7, 6, 6, 6, 6], [(0, 1), (0, 2), (0, 3), (0, 4)])
ODD_TYPE = mol([6, 8], [(0, 1, 7)])
RANDOM = [random_aromatic(seed) for seed in range(256)]


@pytest.fixture(scope='module')
def random_want():
    """kekulize_ref of the 256 random molecules, computed once"""
    return K.stack_ref(RANDOM)


def same(got, ref, what, keys=None):
    got = molpack.to_host(got)
    for k in keys or ref:
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        bad = np.flatnonzero(got[k] != ref[k])
        assert len(bad) == 0, (what, k, bad[:8], got[k][bad[:8]], ref[k][bad[:8]])


def test_the_named_molecules_as_one_batch():
    mols = list(NAMED.values()) + [THREE, STAR, NOISY, AMMONIUM, ODD_TYPE, mol(0, []), mol(1, [])]
    want = K.stack_ref(mols)
    assert want['n_failed'][:len(NAMED)].tolist() == [0] * 12 + [1, 1, 0]
    got = K.kekulize_mols(mols, DEV)
    same(got, want, 'named')
    # three components, one of them the all-carbon 5-ring
    r = K.mol_result(molpack.to_host(got), len(NAMED))
    assert (r['n_components'], r['n_failed'], r['n_double']) == (3, 1, 6)
    assert ((r['atom_flag'] & K.FLAG_UNSOLVED) != 0).tolist() == [False] * 6 + [True] * 5 + [False] * 6
    assert r['kek_order'].tolist() == [2, 1, 2, 1, 2, 1] + [0] * 5 + [2, 1, 2, 1, 2, 1] + [1, 1]
    # other tables reach the device too
    stiff = K.KekuleTables(flexible=(), charged_valence={7: 4, 8: 3, 16: 3})
    want2 = K.stack_ref(mols, stiff)
    assert not np.array_equal(want2['n_failed'], want['n_failed'])
    same(K.kekulize_mols(mols, DEV, stiff), want2, 'other tables')


def test_a_random_batch_and_its_reverse(random_want):
    feasible = K.kekulizable(random_want)
    share = feasible.mean()
    print('kekulizable share', share, 'largest steps', int(random_want['steps'].max()))
    assert 0.25 <= share <= 0.75                       # both outcomes hold at least a quarter of the batch
    got = molpack.to_host(K.kekulize_mols(RANDOM, DEV))
    same(got, random_want, 'random')
    back = molpack.to_host(K.kekulize_mols(RANDOM[::-1], DEV))
    for m in range(len(RANDOM)):
        a, b = K.mol_result(got, m), K.mol_result(back, len(RANDOM) - 1 - m)
        assert all(np.array_equal(a[k], b[k]) for k in a), m
    again = molpack.to_host(K.kekulize_mols(RANDOM, DEV))
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def test_the_budget_thresholds_on_the_grids():
    g88, g79 = grid(8, 8), grid(7, 9)
    S = int(K.kekulize_ref(g88, max_steps=1 << 20)['steps'])
    assert S == 28584
    for steps, over in ((S, 0), (S - 1, 1)):
        want = K.stack_ref([g88, NAMED['benzene'], g79], max_steps=steps)
        assert want['n_over_budget'].tolist() == [over, 0, 0] and want['n_failed'].tolist() == [0, 0, 1]
        assert want['steps'].tolist() == [0 if over else S, 3, 14501]
        same(K.kekulize_mols([g88, NAMED['benzene'], g79], DEV, max_steps=steps), want, ('budget', steps))
    same(K.kekulize_mols([g88, THREE], DEV, max_steps=1), K.stack_ref([g88, THREE], max_steps=1), 'budget 1')


def test_sizes_select_and_a_molecule_past_the_arrays():
    chain = lambda n, t: mol(n, [(k, k + 1, t) for k in range(n - 1)])
    dense = mol(200, [(k, k + 1) for k in range(199)] + [(k, k + 2) for k in range(198)] + [(k, k + 3) for k in range(116)])   # 513 bonds
    mols = [chain(65, 4), chain(257, 1), dense, chain(64, 4), chain(256, 1), NAMED['indole'], grid(8, 8)]
    want = K.stack_ref(mols)
    assert want['status'].tolist() == [1, 1, 1, 0, 0, 0, 0] and want['n_double'].tolist() == [0, 0, 0, 32, 0, 4, 32]
    for m in range(3):
        r = K.mol_result(want, m)
        assert all(r[k] == 0 for k in K.STAT_KEYS[1:]) and not any(r[k].any() for k in K.ATOM_KEYS + K.BOND_KEYS)
    same(K.kekulize_mols(mols, DEV), want, 'sizes')
    # select: the masked molecule has status 0 and zeros everywhere, its slots included; the others are unchanged
    p = molpack.pack_mols(mols, ELEMENTS)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    masked = 5
    select = torch.ones(len(mols), dtype=torch.int32, device=DEV)
    select[masked] = 0
    ref = {k: v.copy() for k, v in want.items()}
    a0, b0 = int(p['atom_ptr'][masked]), int(p['bond_ptr'][masked])
    for k in K.STAT_KEYS:
        ref[k][masked] = 0
    for k in K.ATOM_KEYS:
        ref[k][a0:a0 + int(p['n_atoms'][masked])] = 0
    ref['kek_order'][b0:b0 + int(p['n_bonds'][masked])] = 0
    out = K.launch(molpack.CompactMols.from_packed(d), select=select)
    N, E = int(p['n_atoms'].sum()), int(p['n_bonds'].sum())
    out = dict(out, **{k: out[k][:N] for k in K.ATOM_KEYS}, kek_order=out['kek_order'][:E])
    same(out, ref, 'select', keys=OUT_KEYS)
    # a molecule whose extent leaves the arrays: status 0, zeros, and nothing of it is written (the arrays hold a sentinel)
    cm = molpack.CompactMols.from_packed(d)
    short = cm._replace(N_cap=N - 3)                                    # the last molecule (the grid) reaches past N_cap
    L = _lib.lib()
    tb = K.KekuleTables()
    sent = {k: torch.full((N,), 7, dtype=torch.int32, device=DEV) for k in K.ATOM_KEYS}
    sent['kek_order'] = torch.full((max(cm.Eh_stride, 1),), 7, dtype=torch.int32, device=DEV)
    stats = torch.full((len(mols), len(K.STAT_KEYS)), 7, dtype=torch.int32, device=DEV)
    ops, at = short.operands()
    _lib.check(L.mdx_mol_kekulize(*ops, None, 7, 4, tb.normal_valence.ctypes.data, tb.charged_valence.ctypes.data, tb.flexible, 1 << 16,
                                  at(sent['kek_order']), at(sent['val']), at(sent['charge']), at(sent['kek_h']), at(sent['atom_flag']),
                                  at(stats), _lib.stream()))
    torch.cuda.synchronize()
    last = len(mols) - 1
    a0, b0 = int(p['atom_ptr'][last]), int(p['bond_ptr'][last])
    assert stats[last].tolist() == [0] * len(K.STAT_KEYS)
    assert all(bool((sent[k][a0:] == 7).all()) for k in K.ATOM_KEYS) and bool((sent['kek_order'][b0:] == 7).all())
    got = {k: stats[:, c].cpu().numpy() for c, k in enumerate(K.STAT_KEYS)}
    assert all(np.array_equal(got[k][:last], want[k][:last]) for k in K.STAT_KEYS)
    assert all(np.array_equal(sent[k][:a0].cpu().numpy(), want[k][:a0]) for k in K.ATOM_KEYS)
    # no molecule
    got = molpack.to_host(K.kekulize_mols([], DEV))
    ref = K.empty()
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape for k in ref)
    with pytest.raises(ValueError, match='same pair'):
        K.kekulize_mols([mol(3, [(0, 1, 4), (1, 2, 4), (1, 0, 4)])], DEV)


def test_argument_errors_leave_the_outputs_untouched():
    L = _lib.lib()
    ARG = 1
    mols = [NAMED['benzene'], NAMED['pyridine'], NAMED['ring5']]
    p = molpack.pack_mols(mols, ELEMENTS)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    N, E = int(p['n_atoms'].sum()), int(d['bond_index'].shape[1])
    seven = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)
    o = {'kek_order': seven(E), 'val': seven(N), 'charge': seven(N), 'kek_h': seven(N), 'atom_flag': seven(N), 'mol_stats': seven(3, 11)}
    tb = K.KekuleTables()
    V, Vc = tb.normal_valence.copy(), tb.charged_valence.copy()

    def call(B=3, N_cap=N, stride=E, ne=7, nbt=4, v=V, vc=Vc, flexible=2, steps=100, null=None):
        q = lambda name, t: None if null == name else _lib.ptr(t)
        return L.mdx_mol_kekulize(B, q('atom_ptr', d['atom_ptr']), _lib.ptr(d['bond_ptr']), _lib.ptr(d['n_atoms']), _lib.ptr(d['n_bonds']),
                                  q('atom_type', d['atom_type']), N_cap, _lib.ptr(d['bond_type']), q('bond_index', d['bond_index']), stride, None,
                                  ne, nbt, None if null == 'normal_valence' else v.ctypes.data,
                                  None if null == 'charged_valence' else vc.ctypes.data, flexible, steps,
                                  *(q(k, o[k]) for k in ('kek_order', 'val', 'charge', 'kek_h', 'atom_flag', 'mol_stats')), _lib.stream())
    for name in ('atom_ptr', 'atom_type', 'bond_index', 'normal_valence', 'charged_valence', 'kek_order', 'val', 'charge', 'kek_h', 'atom_flag',
                 'mol_stats'):
        assert call(null=name) == ARG and b'null' in L.mdx_last_error(), name
    assert call(B=-1) == ARG and call(N_cap=-1) == ARG and call(stride=-1) == ARG
    assert call(ne=0) == ARG and call(ne=33) == ARG and call(nbt=0) == ARG and call(nbt=17) == ARG
    assert call(steps=0) == ARG and b'max_steps' in L.mdx_last_error() and call(steps=(1 << 20) + 1) == ARG
    assert call(v=np.full(7, 65, dtype=np.int32)) == ARG and b'0 .. 64' in L.mdx_last_error()
    assert call(vc=np.full(7, -1, dtype=np.int32)) == ARG
    assert call(flexible=1 << 7) == ARG and b'flexible' in L.mdx_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in o.values())
    assert call(B=0) == 0                                              # no molecule: accepted, nothing written
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in o.values())
    v2 = V.copy()
    assert call(v=v2) == 0                                             # the same operands, unbroken, are accepted;
    v2[:] = -1                                                         # the caller's tables are free once the call has returned
    torch.cuda.synchronize()
    ref = K.stack_ref(mols, max_steps=100)
    assert o['mol_stats'].cpu().numpy().tolist() == np.stack([ref[k] for k in K.STAT_KEYS], 1).tolist()
    for k in K.ATOM_KEYS:
        assert o[k].cpu().numpy().tolist() == ref[k].tolist(), k
    assert o['kek_order'].cpu().numpy()[:len(ref['kek_order'])].tolist() == ref['kek_order'].tolist()


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


def test_kekulize_batch_on_the_decode_layout_equals_kekulize_mols_of_its_molecules():
    mols = [NAMED['indole'], THREE, NAMED['n_methylpyridinium'], RANDOM[3], NAMED['ring7'], NAMED['pyridone'], RANDOM[17], AMMONIUM]
    args = _pred_of(mols, masks=[2, 1, 0, 0, 3, 0, 1, 2])
    decoded = FEAT.decode_batch(*args)
    assert [len(d['element']) for d in decoded] == [len(m['element']) for m in mols]
    listed, ref = molpack.to_host(K.kekulize_mols(decoded, DEV)), K.stack_ref(decoded)
    same(listed, ref, 'kekulize_mols of the decoded list')
    assert 0 < K.kekulizable(ref).sum() < len(mols) and ref['n_charged'].sum() >= 2

    def check(got, masked=()):
        got = molpack.to_host(got)
        for m in range(len(mols)):
            zero = m in masked
            for k in K.MOL_KEYS:
                assert got[k][m] == (0 if zero else listed[k][m]), (k, m)
            a0, la, na = int(got['atom_ptr'][m]), int(listed['atom_ptr'][m]), len(decoded[m]['element'])
            b0, lb, nb = int(got['bond_ptr'][m]), int(listed['bond_ptr'][m]), int(listed['n_bonds'][m])
            for k in K.ATOM_KEYS:
                assert np.array_equal(got[k][a0:a0 + na], listed[k][la:la + na] * (not zero)), (k, m)
            assert np.array_equal(got['kek_order'][b0:b0 + nb], listed['kek_order'][lb:lb + nb] * (not zero)), m
    check(FEAT.kekulize_batch(*args))
    check(FEAT.kekulize_batch(*args, select=torch.tensor([1, 1, 1, 1, 1, 0, 1, 1], device=DEV)), masked=(5,))
    with pytest.raises(ValueError, match='another featuriser'):
        FEAT.kekulize_batch(*args, K.KekuleTables(atomic_numbers=(6, 7, 8)))


def _sample(tmp_path, name, extra):
    from moldiff_amd import sample_drug3d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log_dir = sample_drug3d.main(['--config', os.path.join(root, 'configs', 'sample_MolDiff_simple.yml'), '--outdir', str(tmp_path / name),
                                  '--device', DEV, '--recipe-weights', '--num_steps', '2', '--num_mols', '4', '--batch_size', '8'] + extra)
    return log_dir, torch.load(os.path.join(log_dir, 'samples_all.pt'), weights_only=False)


def test_entry_point_writes_the_kekule_files_and_accepts_by_the_rule(tmp_path):
    from moldiff_amd.sample_drug3d import read_mol_block
    new = {'kekule.json', 'kekule.npz', 'samples_kekule.sdf'}
    # the seed is sample.seed + sum(ord(outdir)): the directory names are permutations of each other, so the runs sample the same molecules
    d0, pool0 = _sample(tmp_path, 'abc', ['--largest_fragment', '0.2'])
    assert not new & set(os.listdir(d0))                                # without the options none of them is written
    assert not any('kekulizable' in m for m in pool0['finished'] + pool0['failed'])
    with open(os.path.join(d0, 'quality.json')) as f:
        assert 'kekulizable' not in json.load(f)['counts']
    # --kekulize alone: the same molecules are finished, and the three files describe them
    d1, pool = _sample(tmp_path, 'bca', ['--largest_fragment', '0.2', '--kekulize'])
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new) and new <= set(os.listdir(d1))
    assert len(pool['finished']) >= 2 and [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    ref = K.stack_ref(pool['finished'])
    saved = molpack.load_npz(os.path.join(d1, 'kekule.npz'))
    assert set(saved) == set(ref) and all(np.array_equal(saved[k], ref[k]) and saved[k].dtype == ref[k].dtype for k in ref)
    with open(os.path.join(d1, 'kekule.json')) as f:
        got = json.load(f)
    ok = K.kekulizable(ref)
    print('finished', len(pool['finished']), 'kekulizable', int(ok.sum()), 'status', ref['status'].tolist())
    assert got['n_molecules'] == len(pool['finished']) and got['n_kekulizable'] == int(ok.sum())
    assert [m['kekulizable'] for m in pool['finished']] == ok.tolist()
    with open(os.path.join(d1, 'samples_kekule.sdf')) as f:
        blocks = [b for b in f.read().split('$$$$\n') if b.strip()]
    written = [m for k, m in enumerate(pool['finished']) if ok[k] and (K.mol_result(ref, k)['kek_order'] >= 1).all()]
    assert len(blocks) == len(written)
    for b, m in zip(blocks, written):
        back = read_mol_block(b)
        assert 4 not in back['bond_type'] and np.array_equal(back['element'], m['element']) and np.array_equal(back['bond_index'], m['bond_index'])
    with open(os.path.join(d1, 'quality.json')) as f:
        q = json.load(f)
    everyone = pool['finished'] + pool['failed']
    assert q['accept'] == 'connected' and q['counts']['kekulizable'] == sum(m['kekulizable'] for m in everyone)
    # --accept kekule: 'valence' and kekulizable, judged from the same device results
    d2, pool2 = _sample(tmp_path, 'cab', ['--largest_fragment', '0.2', '--accept', 'kekule'])
    assert not new & set(os.listdir(d2))
    everyone = pool2['finished'] + pool2['failed']
    assert [bool(K.kekulizable(K.kekulize_ref(m))) for m in everyone] == [m['kekulizable'] for m in everyone]
    assert all(m['kekulizable'] and m['n_overvalent'] == 0 for m in pool2['finished'])
    assert all(not m['kekulizable'] or m['n_overvalent'] > 0 or m['n_components'] != 1 for m in pool2['failed'] if not m['salvaged'])
    with open(os.path.join(d2, 'quality.json')) as f:
        q = json.load(f)
    print('accept kekule: finished', len(pool2['finished']), 'failed', len(pool2['failed']), q['counts'])
    assert q['accept'] == 'kekule' and q['counts']['kekulizable'] == sum(m['kekulizable'] for m in everyone) >= q['counts']['finished']
