"""GPU tests of the molecule quality check (mdx_mol_check / mdx_mol_keep_component through FeaturizeMol.check_batch, and the
sampling entry point's --accept / --largest_fragment).

Inputs are `pred` tensors built from chosen class ids (logit = 10 * one_hot) and chosen coordinates on placeholder batches, so the
decode is deterministic; the host form ``FeaturizeMol.decode_output`` + ``molcheck.check_ref`` is the reference.  Every integer
output is compared exactly.  The two distances are compared with the float64 value from the same fp32 coordinates within
4 * 2^-24 relative: three subtractions, three squares, two adds and a square root in fp32 are 3.5 half-ulps, rounded up (a
coincident pair gives exactly 0).
"""
import json
import os

import numpy as np
import pytest
import torch

from moldiff_amd import molcheck as MC
from moldiff_amd.harness import placeholder_from_sizes
from moldiff_amd.postprocess import FeaturizeMol

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FEAT = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
MASK = 7                      # the mask node type: decode drops it
C, N_, O_, F_, P_, S_, CL = range(7)
RTOL = 4 * 2.0 ** -24
KEYS = ('element', 'atom_pos', 'atom_prob', 'bond_type', 'bond_prob', 'bond_index')
INTS = ('n_components', 'largest_size', 'largest_label', 'n_overvalent', 'n_atoms')


def M(cls, bonds=(), pos=None, seed=0):
    """one molecule: atom classes, (i, j, type) bonds in ORIGINAL indices, (n,3) coordinates (default: seeded normal)"""
    n = len(cls)
    if pos is None:
        pos = 2.0 * np.random.default_rng([seed, n]).standard_normal((n, 3))
    return {'cls': np.asarray(cls, dtype=np.int64), 'bonds': list(bonds), 'pos': np.asarray(pos, dtype=np.float32).reshape(n, 3)}


def pack(mols):
    """-> (pred tensors on the host as numpy, per-molecule host decode by FeaturizeMol.decode_output)"""
    pn, pp, ph, host = [], [], [], []
    for m in mols:
        n = len(m['cls'])
        T = np.zeros((n, n), dtype=np.int64)
        for i, j, t in m['bonds']:
            T[min(i, j), max(i, j)] = t
        iu, ju = np.triu_indices(n, 1)
        a = (10.0 * np.eye(8)[m['cls']]).astype(np.float32)
        e = (10.0 * np.eye(6)[T[iu, ju]]).astype(np.float32).reshape(-1, 6)
        pn.append(a), pp.append(m['pos']), ph.append(e)
        host.append(FEAT.decode_output(a, m['pos'], e, np.stack([iu, ju])))
    return [np.concatenate(pn), np.concatenate(pp), np.concatenate(ph)], host


def run(mols, **kw):
    pred, host = pack(mols)
    ph = placeholder_from_sizes([len(m['cls']) for m in mols], DEV)
    dev = [torch.from_numpy(p).to(DEV) for p in pred]
    got, rep = FEAT.check_batch(dev, ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], len(mols), **kw)
    return got, rep, host, (dev, ph)


def close(got, want):
    got, want = float(got), float(want)
    return got == want if (want == 0.0 or np.isinf(want)) else abs(got - want) <= RTOL * want


def same_mol(a, b):
    for k in KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.astype(x.dtype).tobytes(), k


def compare(got, rep, host, max_valence=None):
    """check_batch without salvage == host decode + check_ref, molecule by molecule"""
    refs = [MC.check_ref(h, max_valence, 4) for h in host]
    for m, (g, h, r) in enumerate(zip(got, host, refs)):
        for k in ('element', 'bond_type', 'bond_index'):
            assert np.array_equal(g[k], h[k]), (m, k)
        assert g['atom_pos'].tobytes() == h['atom_pos'].tobytes(), m
        for k in INTS:
            assert int(rep[k][m]) == r[k], (m, k, int(rep[k][m]), r[k])
        assert np.array_equal(g['component'], r['component']) and np.array_equal(g['valence'], r['valence']), m
        print(f"mol {m}: min_dist {float(rep['min_dist'][m])!r} vs {r['min_dist']!r}; max_bond_len "
              f"{float(rep['max_bond_len'][m])!r} vs {r['max_bond_len']!r}")
        assert close(rep['min_dist'][m], r['min_dist']) and close(rep['max_bond_len'][m], r['max_bond_len']), m
        assert not rep['salvaged'][m]
    return refs


def path(n, seed, cut_last=False):
    """path graph whose consecutive atoms are far apart in index (seeded permutation); cut_last: its last atom stands alone"""
    p = np.random.default_rng(seed).permutation(n)
    k = n - 2 if cut_last else n - 1
    return M([C] * n, [(int(p[i]), int(p[i + 1]), 1) for i in range(k)], seed=seed)


def test_smallest_molecules_and_edge_cases():
    ring = [(i, (i + 1) % 6, 4) for i in range(6)]
    mols = [M([MASK, MASK, MASK], [(0, 1, 1)]),                              # 0: nothing survives
            M([MASK, O_]),                                                   # 1: one survivor, no bond
            M([C, O_], [(0, 1, 2)]),                                         # 2: two atoms, bonded
            M([C, O_]),                                                      # 3: two atoms, unbonded
            M([C, C, C, C], [(1, 2, 1), (0, 3, 1)]),                         # 4: two fragments of equal size: label 0 wins
            M([C] * 7, ring),                                                # 5: ring + isolated atom 6
            M([C, C, MASK, C, C], [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)]),   # 6: chain cut by a mask atom; NEW indices
            M([C, N_, O_], [(0, 1, 1)], pos=[[1, 2, 3], [4, 6, 3], [1, 2, 3]])]    # 7: coincident pair -> exactly 0
    got, rep, host, _ = run(mols)
    refs = compare(got, rep, host)
    assert rep['n_atoms'].tolist() == [0, 1, 2, 2, 4, 7, 4, 3]
    assert rep['n_components'].tolist() == [0, 1, 1, 2, 2, 2, 2, 2]
    assert rep['largest_label'].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and rep['largest_size'].tolist() == [0, 1, 2, 1, 2, 6, 2, 2]
    assert np.isinf(rep['min_dist'][0]) and np.isinf(rep['min_dist'][1]) and rep['max_bond_len'][1] == 0 == rep['max_bond_len'][3]
    assert got[4]['component'].tolist() == [0, 1, 1, 0] and got[6]['component'].tolist() == [0, 0, 2, 2]
    assert got[5]['valence'].tolist() == [3.0] * 6 + [0.0] and rep['n_overvalent'][5] == 0
    assert rep['min_dist'][7] == 0.0 and rep['max_bond_len'][7] == 5.0


@pytest.mark.parametrize('n,cut', [(70, False), (300, False), (300, True), (513, True)])
def test_long_paths_cross_the_wave_chunk_and_lds_boundaries(n, cut):
    """70 > one wave, 300 > one 256-atom chunk, 513 > the kernel's LDS capacity (labels in the workspace); many sweeps"""
    got, rep, host, _ = run([M([C, C], [(0, 1, 1)]), path(n, n, cut), M([O_, C], [(0, 1, 2)])])
    compare(got, rep, host)
    assert rep['n_components'].tolist() == [1, 2 if cut else 1, 1] and rep['largest_size'][1] == n - cut


def test_every_element_at_its_limit_and_one_above_and_aromatic_rounding():
    star = lambda z, k, t=1: M([z] + [C] * k, [(0, i + 1, t) for i in range(k)], seed=z)
    limits = MC.valence_table(FEAT.atomic_numbers.tolist())
    mols = [star(z, v + d) for z, v in enumerate(limits) for d in (0, 1)]
    mols += [M([C] * 6, [(i, (i + 1) % 6, 4) for i in range(6)]),        # benzene-like ring: 3 each
             M([F_, C], [(0, 1, 4)]),                                    # 3/2 -> 1: clean for F
             star(C, 3, 4),                                              # fused aromatic atom: 9/2 -> 4, clean
             M([C] * 5, [(0, 1, 4), (0, 2, 4), (0, 3, 4), (0, 4, 1)])]   # 11/2 -> 5: over
    got, rep, host, _ = run(mols)
    compare(got, rep, host)
    assert rep['n_overvalent'].tolist() == [0, 1] * 7 + [0, 0, 0, 1]
    assert got[-1]['valence'][0] == 5.5 and got[-2]['valence'][0] == 4.5
    table = {**MC.DEFAULT_MAX_VALENCE, 6: 5}                            # a caller's table flips the last verdict only
    got, rep, host, _ = run(mols, max_valence=table)
    compare(got, rep, host, table)
    assert rep['n_overvalent'].tolist() == [0, 0] + [0, 1] * 6 + [0, 0, 0, 0]
    with pytest.raises(ValueError):
        run(mols[:1], max_valence={6: 4})


def random_batch(seed=5, count=64, density=2.2):
    g = np.random.default_rng(seed)
    mols = []
    for _ in range(count):
        n = int(g.integers(2, 41))
        cls = g.choice(8, n, p=[.5, .12, .12, .05, .04, .05, .04, .08])
        iu, ju = np.triu_indices(n, 1)
        on = g.random(iu.shape[0]) < density / n
        bonds = [(int(i), int(j), int(g.choice([1, 2, 3, 4], p=[.6, .15, .05, .2]))) for i, j in zip(iu[on], ju[on])]
        mols.append(M(cls, bonds, 1.5 * g.standard_normal((n, 3))))
    return mols


def test_packing_independence_bit_for_bit():
    others = random_batch(11, 8)
    x = random_batch(12, 1)[0]
    outs = []
    for where in (None, 0, 4, 8):
        mols = [x] if where is None else others[:where] + [x] + others[where:]
        got, rep, _, _ = run(mols)
        k = 0 if where is None else where
        outs.append(b''.join(np.asarray(rep[key][k]).tobytes() for key in INTS + ('min_dist', 'max_bond_len')) +
                    got[k]['component'].tobytes() + got[k]['valence'].tobytes())
    assert len(mols) == 9 and all(o == outs[0] for o in outs)


@pytest.fixture(scope='module')
def rand64():
    mols = random_batch()
    got, rep, host, io = run(mols)
    return mols, got, rep, host, io


def test_random_batch_of_64(rand64):
    mols, got, rep, host, _ = rand64
    refs = compare(got, rep, host)
    # the classes the seed and the bond density were chosen for (on the host, from check_ref alone)
    assert sum(r['n_components'] == 1 for r in refs) >= 8 and sum(r['n_components'] > 1 for r in refs) >= 8
    assert sum(r['n_overvalent'] > 0 for r in refs) >= 8 and sum(len(m['cls']) > len(h['element']) for m, h in zip(mols, host)) >= 8


@pytest.mark.parametrize('f', [0.5, 0.75, 1.0])
def test_largest_fragment(rand64, f):
    mols, plain, rep0, host, (dev, ph) = rand64
    got, rep, _, _ = run(mols, largest_fragment=f)
    for k in INTS + ('min_dist', 'max_bond_len'):      # the report describes the molecule as decoded
        assert rep[k].tobytes() == rep0[k].tobytes(), k
    want = (rep0['n_components'] > 1) & (rep0['largest_size'] >= f * rep0['n_atoms'])
    assert np.array_equal(rep['salvaged'], want) and (f == 1.0 or want.sum() >= 3)
    for m, h in enumerate(host):
        if want[m]:
            r = MC.check_ref(h)
            same_mol(got[m], MC.restrict_ref(h | {k: plain[m][k] for k in ('atom_prob', 'bond_prob')}, r['component'], r['largest_label']))
            keep = r['component'] == r['largest_label']
            assert np.array_equal(got[m]['valence'], r['valence'][keep]) and not got[m]['component'].any()
            assert len(got[m]['element']) == r['largest_size'] < r['n_atoms']
        else:
            same_mol(got[m], plain[m])
            assert np.array_equal(got[m]['component'], plain[m]['component']) and np.array_equal(got[m]['valence'], plain[m]['valence'])
    # the kernels once more on the restricted arrays: one fragment, the same valences atom by atom
    graph, d = FEAT._decode_device(dev, ph['batch_node'], ph['halfedge_index'], len(mols), None)
    FEAT._check_device(graph, d, None, f)
    ri, _, pa = (t.cpu().numpy() for t in FEAT._check_device(graph, d))
    node_ptr = np.concatenate([[0], np.cumsum([len(m['cls']) for m in mols])])
    for m in np.flatnonzero(want):
        assert ri[0, m] == 1 and ri[1, m] == ri[4, m] == len(got[m]['element'])
        assert np.array_equal(pa[1, node_ptr[m]:node_ptr[m] + ri[4, m]] / 2.0, got[m]['valence'])


def test_decode_batch_is_unchanged_by_a_check_on_the_same_graph_handle(rand64):
    mols, _, _, host, (dev, ph) = rand64
    from moldiff_amd import _lib
    graph = _lib.graph_for_halfedges(ph['halfedge_index'], ph['batch_node'], len(mols))
    args = (dev, ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], len(mols), graph)
    before = FEAT.decode_batch(*args)
    FEAT.check_batch(*args, largest_fragment=0.5)
    after = FEAT.decode_batch(*args)
    for a, b, h in zip(before, after, host):
        same_mol(a, b)
        assert set(a) == set(KEYS) and np.array_equal(a['bond_index'], h['bond_index']) and np.array_equal(a['element'], h['element'])


def test_too_small_workspace_is_refused():
    from moldiff_amd import _lib
    ph = placeholder_from_sizes([4, 5], DEV)
    graph = _lib.graph_for_halfedges(ph['halfedge_index'], ph['batch_node'], 2)
    ws, _ = graph.workspace(torch.device(DEV))
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = _lib.ptr(z)
    rc = _lib.lib().mdx_mol_check(graph.h, *([p] * 6), 7, 4, *([p] * 9), ws, 8 * 9, _lib.stream())
    assert rc == 1 and b'workspace too small' in _lib.lib().mdx_last_error()
    rc = _lib.lib().mdx_mol_keep_component(graph.h, *([p] * 11), ws, 8 * 9, _lib.stream())
    assert rc == 1 and b'workspace too small' in _lib.lib().mdx_last_error()
    assert _lib.lib().mdx_mol_check(graph.h, None, *([p] * 5), 7, 4, *([p] * 9), ws, 1 << 20, _lib.stream()) == 1


# ---- the sampling entry point (recipe weights are synthetic: these runs test plumbing, not chemistry) ------------------------------

def _sample(tmp_path, name, extra, monkeypatch=None):
    from moldiff_amd import sample_drug3d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    drawn = []
    if monkeypatch is not None:
        real = sample_drug3d.placeholder_from_sizes
        monkeypatch.setattr(sample_drug3d, 'placeholder_from_sizes', lambda s, d=None: (drawn.append(np.asarray(s).copy()), real(s, d))[1])
    log_dir = sample_drug3d.main(['--config', os.path.join(root, 'configs', 'sample_MolDiff_simple.yml'), '--outdir', str(tmp_path / name),
                                  '--device', DEV, '--recipe-weights', '--num_steps', '5', '--num_mols', '4', '--batch_size', '8'] + extra)
    pool = torch.load(os.path.join(log_dir, 'samples_all.pt'), weights_only=False)
    sdf = {f: open(os.path.join(log_dir + '_SDF', f)).read() for f in sorted(os.listdir(log_dir + '_SDF'))}
    return log_dir, pool, sdf, drawn


def test_entry_point_accept_connected_is_the_default_rule_plus_a_report(tmp_path):
    # the seed is sample.seed + sum(ord(outdir)): the two directory names are permutations of each other
    d0, p0, sdf0, _ = _sample(tmp_path, 'ab', [])
    d1, p1, sdf1, _ = _sample(tmp_path, 'ba', ['--accept', 'connected'])
    for part in ('finished', 'failed'):
        assert [i['mol_id'] for i in p0[part]] == [i['mol_id'] for i in p1[part]]
        assert all(set(i) - {'traj_file'} == set(KEYS) | {'mol_id'} for i in p0[part])
        for a, b in zip(p0[part], p1[part]):
            same_mol(a, b)
    assert sdf0 == sdf1 and len(p0['finished']) + len(p0['failed']) > 0
    assert not os.path.exists(os.path.join(d0, 'quality.json'))
    q = json.load(open(os.path.join(d1, 'quality.json')))
    every = p1['finished'] + p1['failed']
    refs = [MC.check_ref(i) for i in every]
    for i, r in zip(every, refs):
        assert (i['n_components'], i['n_overvalent'], i['salvaged']) == (r['n_components'], r['n_overvalent'], False)
        assert close(i['min_dist'], r['min_dist']) and close(i['max_bond_len'], r['max_bond_len'])
    assert q['counts'] == {'sampled': len(every), 'connected': sum(r['n_components'] == 1 for r in refs),
                           'valence_clean': sum(r['n_atoms'] > 0 and r['n_overvalent'] == 0 for r in refs),
                           'finished': len(p1['finished']), 'salvaged': 0, 'failed': len(p1['failed'])}
    assert q['counts']['connected'] == q['counts']['finished']
    assert q['fractions']['finished'] == len(p1['finished']) / len(every) and q['accept'] == 'connected'


def test_entry_point_valence_rule_with_salvage(tmp_path, monkeypatch):
    d, pool, _, drawn = _sample(tmp_path, 'out', ['--accept', 'valence', '--largest_fragment', '0.5'], monkeypatch)
    # per batch the entry point packs the rank's slice, perhaps a few trajectories, then the whole batch (= the slice on one rank)
    full, i = [], 0
    while i < len(drawn):
        step = 1 if np.array_equal(drawn[i], drawn[i + 1]) else 2
        assert np.array_equal(drawn[i], drawn[i + step])
        full.append(drawn[i])
        i += step + 1
    size_of = np.concatenate(full)
    for info in pool['finished']:
        r = MC.check_ref(info)
        assert r['n_components'] == 1 and r['n_overvalent'] == 0
    for info in pool['finished'] + pool['failed']:
        if info['salvaged']:
            assert info['n_components'] > 1 and len(info['element']) < size_of[info['mol_id']]
            assert MC.check_ref(info)['n_components'] == 1
    q = json.load(open(os.path.join(d, 'quality.json')))
    assert q['counts']['salvaged'] == sum(i['salvaged'] for i in pool['finished'] + pool['failed'])
    assert q['counts']['finished'] == len(pool['finished']) and q['largest_fragment'] == 0.5 and q['accept'] == 'valence'
