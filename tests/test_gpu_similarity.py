"""GPU tests of the set-level similarity (mdx_mol_fingerprint and mdx_fp_tanimoto through similarity.fingerprint_mols,
FeaturizeMol.fingerprint_batch, similarity.tanimoto / summary and the sampling entry point's --similarity).  The oracles are the numpy
restatements ``fingerprint_ref``, ``tanimoto_ref`` and ``summary_ref``; everything is integer arithmetic or one correctly rounded fp32
division per pair, so every comparison is exact (row_max by its bit pattern)."""
import json
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import similarity as S
from moldiff_amd.harness import placeholder_from_sizes
from moldiff_amd.postprocess import FeaturizeMol

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
LDS_ATOMS = 1024          # include/moldiff_hip.h: a larger molecule keeps its id arrays in the workspace
SPECS = [S.FingerprintSpec(radius=r, nbits=b) for b in (32, 96, 2048) for r in (0, 2)]


def mol(ele, bonds):
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
            'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def random_mol(seed, n, extra=0.3):
    """connected: a random spanning tree plus extra * n further bonds; the first 7 atoms and 4 bonds carry every element and type"""
    g = np.random.default_rng(seed)
    bonds = {(int(g.integers(0, k)), k) for k in range(1, n)}
    while len(bonds) < n - 1 + int(extra * n):
        i, j = sorted(int(x) for x in g.choice(n, 2, replace=False))
        bonds.add((i, j))
    ele = g.choice(ELEMENTS, n)
    ele[:7] = ELEMENTS[:n]
    bt = g.integers(1, 5, len(bonds))
    bt[:4] = [1, 2, 3, 4][:len(bonds)]
    return mol(ele, [(i, j, int(t)) for (i, j), t in zip(sorted(bonds), bt)])


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
    return {'element': ele, 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}


RING = mol([6, 6, 7, 6, 6, 8], [(k, (k + 1) % 6, 4) for k in range(6)])
BATCH = [mol([], []),                                                                          # 0 no atom
         mol([8], []),                                                                         # 1 one atom
         mol([6, 8], [(0, 1, 2)]),                                                             # 2 two atoms
         RING,                                                                                 # 3 a 6-ring
         random_mol(40, 40),                                                                   # 4 every element and bond type
         random_mol(41, 12),                                                                   # 5 masked out below
         mol([6, 6, 7, 6, 6, 8], [(0, 6, 1), (2, 2, 3)] + [(k, (k + 1) % 6, 4) for k in range(6)] + [(-1, 3, 2)]),   # 6 = the ring
         random_mol(42, LDS_ATOMS + 1, extra=0.1),                                             # 7 one atom above the LDS limit
         RING]                                                                                 # 8 the ring again, elsewhere
SELECT = np.asarray([1, 1, 1, 1, 1, 0, 1, 1, 1], dtype=np.int32)


@pytest.fixture(scope='module')
def refs():
    """fingerprint_ref of every molecule of BATCH per spec, computed once"""
    return {spec: [S.fingerprint_ref(m, spec) for m in BATCH] for spec in SPECS}


def same_set(got, want_fps, what, masked=()):
    g = got.cpu()
    for m, w in enumerate(want_fps):
        if m in masked:
            assert not g.bits[m].any() and g.n_on[m] == 0 and g.key[m] == 0, (what, m)
            continue
        assert np.array_equal(g.bits[m], w['bits']), (what, m)
        assert g.n_on[m] == w['n_on'] and g.key[m] == w['key'], (what, m, g.n_on[m], w['n_on'], g.key[m], w['key'])


# ---- 1. fingerprints ----------------------------------------------------------------------------------------------------------------------

def test_fingerprints_of_the_dense_list_equal_the_restatement(refs):
    assert len(BATCH[7]['element']) == LDS_ATOMS + 1 and sorted(set(BATCH[4]['element'])) == list(ELEMENTS)
    assert sorted(set(BATCH[4]['bond_type'].tolist())) == [1, 2, 3, 4]
    for spec in SPECS:
        want = refs[spec]
        got = S.fingerprint_mols(BATCH, spec, DEV)
        same_set(got, want, ('fingerprint_mols', spec.nbits, spec.radius))
        assert got.n_atoms.cpu().tolist() == [len(m['element']) for m in BATCH]
        g = got.cpu()
        assert np.array_equal(g.bits[3], g.bits[8]) and np.array_equal(g.bits[3], g.bits[6]) and g.key[3] == g.key[8] == g.key[6]
        assert not g.bits[0].any() and g.n_on[0] == 0 and g.key[0] == 0
        # the same arrays with a mask: molecule 5 gets a zero row, n_on 0 and key 0, the others are unchanged
        p = molpack.pack_mols(BATCH, spec.atomic_numbers)
        d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
        bits, n_on, key = S.launch(molpack.CompactMols.from_packed(d), spec, select=torch.from_numpy(SELECT).to(DEV))
        same_set(S.FingerprintSet(spec, bits, n_on, key, d['n_atoms']), want, ('select', spec.nbits, spec.radius), masked=(5,))


def test_relabelled_copies_agree_on_the_device():
    spec = S.FingerprintSpec()
    base = [BATCH[4], BATCH[7], BATCH[5]]
    got = S.fingerprint_mols(base + [relabelled(m, 7 + k) for k, m in enumerate(base)], spec, DEV).cpu()
    for k in range(3):
        assert np.array_equal(got.bits[k], got.bits[3 + k]) and got.key[k] == got.key[3 + k] and got.n_on[k] == got.n_on[3 + k] > 0
    assert len(set(got.key.tolist())) == 3


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


def test_fingerprint_batch_on_the_decode_layout_equals_the_restatement():
    mols = [BATCH[0], BATCH[1], BATCH[2], BATCH[3], BATCH[4], BATCH[5], BATCH[3]]
    args = _pred_of(mols, masks=[2, 1, 0, 0, 3, 0, 1])             # no atom = two mask atoms, one atom = one of each
    decoded = FEAT.decode_batch(*args)
    assert [len(d['element']) for d in decoded] == [0, 1, 2, 6, 40, 12, 6]
    select = torch.tensor([1, 1, 1, 1, 1, 0, 1], device=DEV)
    for spec in SPECS:
        want = [S.fingerprint_ref(d, spec) for d in decoded]      # the same atoms and bonds, bonds in the decode's order
        got = FEAT.fingerprint_batch(*args, spec)
        same_set(got, want, ('fingerprint_batch', spec.nbits, spec.radius))
        assert got.n_atoms.cpu().tolist() == [0, 1, 2, 6, 40, 12, 6]
        g = got.cpu()
        assert np.array_equal(g.bits[3], g.bits[6]) and g.key[3] == g.key[6]
        same_set(S.fingerprint_mols(decoded, spec, DEV), want, ('fingerprint_mols', spec.nbits, spec.radius))
        masked = FEAT.fingerprint_batch(*args, spec, select=select)
        same_set(masked, want, ('select', spec.nbits, spec.radius), masked=(5,))
        assert masked.n_atoms.cpu().tolist() == [0, 1, 2, 6, 40, 0, 6]
    with pytest.raises(ValueError, match='another featuriser'):
        FEAT.fingerprint_batch(*args, S.FingerprintSpec(atomic_numbers=(6, 7, 8)))


# ---- 2. Tanimoto ---------------------------------------------------------------------------------------------------------------------------

def random_rows(seed, n, words):
    """rows of density 0.01 and 0.5 in turn, then planted: an all-zero row, a duplicate of row 1 (a tie) and one all-ones row"""
    g = np.random.default_rng(seed)
    dens = np.where(np.arange(n) % 2 == 0, 0.01, 0.5)[:, None]
    b = np.packbits(g.random((n, words * 32)) < dens, axis=1, bitorder='little').view(np.uint32).reshape(n, words).copy()
    if n > 4:
        b[2] = 0
        b[n - 1] = b[1]
        b[n // 2] = 0xffffffff
    return b


def device_set(bits):
    spec = S.FingerprintSpec(nbits=32 * bits.shape[1])
    n_on = S.popcount(bits).sum(1).astype(np.int32)
    z = np.zeros(len(bits), dtype=np.int64)
    return S.FingerprintSet(spec, bits, n_on, z, z.astype(np.int32)).to(DEV), n_on


def check_tanimoto(a, b, exclude, what):
    da, na = device_set(a)
    db, nb = (da, na) if b is a else device_set(b)
    want = S.tanimoto_ref(a, na, b, nb, exclude)
    got = [x.cpu().numpy() for x in S.tanimoto(da, db, exclude)]
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, 'row_max')
    assert np.array_equal(got[1], want[1]), (what, 'row_argmax', np.flatnonzero(got[1] != want[1])[:5])
    assert np.array_equal(got[2], want[2]), (what, 'row_sum', np.flatnonzero(got[2] != want[2])[:5])
    return want


@pytest.mark.parametrize('words', [1, 3, 64])
def test_tanimoto_equals_the_restatement(words):
    for Na, Nb in ((1, 1), (2, 65), (63, 64), (65, 130), (130, 1)):
        a, b = random_rows(1000 + Na, Na, words), random_rows(2000 + Nb, Nb, words)
        if Na > 4 and Nb > 4:
            a[3] = b[1]                                    # identical to two columns: 1.0, attained first at j = 1
        want = check_tanimoto(a, b, False, (Na, Nb, words))
        if Na > 4 and Nb > 4:
            assert want[0][3] == 1.0 and want[1][3] == 1 and want[0][2] == 0.0 and want[1][2] == 0 and want[2][2] == 0
    for n in (1, 2, 65, 130):
        a = random_rows(3000 + n, n, words)
        want = check_tanimoto(a, a, True, ('self', n, words))
        if n > 4:
            assert want[1][1] == n - 1 and want[1][n - 1] == 1 and want[0][1] == 1.0     # the duplicate pair finds each other
        if n == 1:
            assert want[1].tolist() == [-1]
    # no columns: -1 / 0 / 0
    a = random_rows(5, 7, words)
    want = check_tanimoto(a, a[:0], False, ('Nb = 0', words))
    assert want[1].tolist() == [-1] * 7 and not want[0].any() and not want[2].any()
    assert all(x.numel() == 0 for x in S.tanimoto(device_set(a[:0])[0], device_set(a)[0]))


def test_tanimoto_rows_wider_than_a_chunk_and_workgroups_that_walk_several_tiles():
    # more than 64 words per row: both tiles are staged chunk by chunk
    for words in (65, 160):
        a, b = random_rows(11, 65, words), random_rows(12, 130, words)
        check_tanimoto(a, b, False, (65, 130, words))
        check_tanimoto(a, a, True, ('self', 65, words))
    # 47 x 47 tiles are more than the 2,048 workgroups aimed at: a workgroup then keeps its partials over two column tiles
    a, b = random_rows(13, 3000, 3), random_rows(14, 2990, 3)
    check_tanimoto(a, b, False, (3000, 2990, 3))
    check_tanimoto(a, a, True, ('self', 3000, 3))


def test_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    ARG = 1
    a, na = device_set(random_rows(1, 5, 3))
    b, nb = device_set(random_rows(2, 6, 3))
    row_max = torch.full((5,), 7.0, dtype=torch.float32, device=DEV)
    row_argmax, row_sum = torch.full((5,), 7, dtype=torch.int32, device=DEV), torch.full((5,), 7, dtype=torch.int64, device=DEV)
    ws = torch.zeros(5, dtype=torch.int64, device=DEV)
    call = lambda nbits, excl, ws_bytes=40: L.mdx_fp_tanimoto(
        _lib.ptr(a.bits), _lib.ptr(a.n_on), 5, _lib.ptr(b.bits), _lib.ptr(b.n_on), 6, nbits, excl, _lib.ptr(row_max), _lib.ptr(row_argmax),
        _lib.ptr(row_sum), _lib.ptr(ws), ws_bytes, _lib.stream())
    assert call(100, 0) == ARG and b'nbits' in L.mdx_last_error()
    assert call(96, 1) == ARG and b'Na == Nb' in L.mdx_last_error()
    assert call(96, 0, ws_bytes=39) == ARG and b'workspace' in L.mdx_last_error()
    spec = S.FingerprintSpec(nbits=96)
    p = molpack.pack_mols(BATCH[:5], spec.atomic_numbers)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    bits, n_on, key = torch.full((5, 3), 7, dtype=torch.int32, device=DEV), torch.full((5,), 7, dtype=torch.int32, device=DEV), \
        torch.full((5,), 7, dtype=torch.int64, device=DEV)
    N = int(p['n_atoms'].sum())
    fws = torch.zeros(N, dtype=torch.int64, device=DEV)
    fp = lambda nbits, radius, key_rounds, ws_bytes: L.mdx_mol_fingerprint(
        5, _lib.ptr(d['atom_ptr']), _lib.ptr(d['bond_ptr']), _lib.ptr(d['n_atoms']), _lib.ptr(d['n_bonds']), _lib.ptr(d['atom_type']), N,
        _lib.ptr(d['bond_type']), _lib.ptr(d['bond_index']), int(d['bond_index'].shape[1]), None, radius, key_rounds, nbits,
        _lib.ptr(bits), _lib.ptr(n_on), _lib.ptr(key), _lib.ptr(fws), ws_bytes, _lib.stream())
    assert fp(100, 2, 8, 8 * N) == ARG and fp(96, 3, 2, 8 * N) == ARG and fp(96, 2, 8, 8 * N - 1) == ARG and fp(32800, 2, 8, 8 * N) == ARG
    torch.cuda.synchronize()
    assert (row_max == 7).all() and (row_argmax == 7).all() and (row_sum == 7).all()
    assert (bits == 7).all() and (n_on == 7).all() and (key == 7).all()
    assert call(96, 0) == 0 and fp(96, 2, 8, 8 * N) == 0             # and the same operands, unbroken, are accepted
    torch.cuda.synchronize()
    assert (row_argmax >= 0).all() and (n_on[1:] > 0).all() and n_on[0] == 0


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------

def same_summary(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), (k, got[k], want[k])


def test_summary_equals_summary_ref_on_planted_duplicates():
    spec = S.FingerprintSpec()
    base = [random_mol(500 + k, 5 + k % 30) for k in range(110)]
    own = base + [relabelled(base[k], k) for k in range(20)]                                    # 130 molecules, 20 of them copies
    reference = [relabelled(base[k], 100 + k) for k in range(15, 40)] + [random_mol(900 + k, 20) for k in range(40)]
    dev_own, dev_ref = S.fingerprint_mols(own, spec, DEV), S.fingerprint_mols(reference, spec, DEV)
    ref_own, ref_ref = S.FingerprintSet.from_ref(own, spec), S.FingerprintSet.from_ref(reference, spec)
    want = S.summary_ref(ref_own, ref_ref)
    assert want['n'] == 130 and want['uniqueness'] == 110 / 130 and want['novelty'] == (130 - 25 - 5) / 130
    same_summary(S.summary(dev_own, dev_ref), want)
    same_summary(S.summary(dev_own), S.summary_ref(ref_own))
    same_summary(S.summary(S.fingerprint_mols(own[:1], spec, DEV), dev_ref), S.summary_ref(S.FingerprintSet.from_ref(own[:1], spec), ref_ref))
    with pytest.raises(ValueError, match='different specs'):
        S.summary(dev_own, S.fingerprint_mols(reference, S.FingerprintSpec(nbits=1024), DEV))


def _sample(tmp_path, name, extra):
    from moldiff_amd import sample_drug3d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log_dir = sample_drug3d.main(['--config', os.path.join(root, 'configs', 'sample_MolDiff_simple.yml'), '--outdir', str(tmp_path / name),
                                  '--device', DEV, '--recipe-weights', '--num_steps', '2', '--num_mols', '6', '--batch_size', '8'] + extra)
    return log_dir, torch.load(os.path.join(log_dir, 'samples_all.pt'), weights_only=False)


def test_entry_point_writes_similarity_json_of_the_finished_molecules(tmp_path):
    # the seed is sample.seed + sum(ord(outdir)): the two directory names are permutations of each other, so both runs sample the same
    # molecules; the first run, without the option, supplies the reference set of the second
    spec = S.FingerprintSpec()
    d0, pool0 = _sample(tmp_path, 'ab', ['--largest_fragment', '0.2'])
    assert len(pool0['finished']) >= 2
    reference = S.FingerprintSet.from_ref(pool0['finished'][:2] + [random_mol(1, 20)], spec)
    reference.save(str(tmp_path / 'reference.npz'))
    d1, pool = _sample(tmp_path, 'ba', ['--largest_fragment', '0.2', '--similarity', str(tmp_path / 'reference.npz')])
    assert [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    new = {'similarity.json', 'fingerprints.npz'}
    assert not new & set(os.listdir(d0)) and sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new)
    own = S.FingerprintSet.from_ref(pool['finished'], spec)
    want = S.summary_ref(own, reference)
    with open(os.path.join(d1, 'similarity.json')) as f:
        got = json.load(f)
    print('finished', len(pool['finished']), got)
    same_summary(got, want)
    assert got['n'] == len(pool['finished']) and got['novelty'] <= 1 - 2 / got['n'] and got['sim_with_ref'] > 0
    saved = S.FingerprintSet.load(os.path.join(d1, 'fingerprints.npz'))
    assert saved.spec == spec and all(np.array_equal(getattr(saved, k), getattr(own, k)) for k in ('bits', 'n_on', 'key', 'n_atoms'))
