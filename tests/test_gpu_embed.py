"""GPU tests of conformer generation (mdx_mol_bounds and mdx_mol_embed through embed.embed_mols, embed.launch and embed.global3d_mols).
The oracle is the restatement ``bounds_ref`` / ``embed_ref``, which repeats the device's operations and reduction tree.  The bounds are
compared bit for bit: the device does only + - x / sqrt, min and max on host-derived table values.  A run is compared in its integers
exactly and in its positions to 1e-6 Angstrom, the tolerance of test_gpu_relax.py, which is not derived: it allows rounding at 1e-15 to
grow by 1e9 over the run; the largest difference seen goes to profiles/embed_accuracy.txt.  A conformer with a decision within 1e-9
(relative) of its threshold may be left out, at most 10 % of the set; the host test asserts that the reference alone leaves out none.
At full length nothing is followed: the violation is recomputed on the host from the returned positions."""
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import embed as E
from moldiff_amd import relax as R
from . import embed_cases as EC
from . import relax_cases as RC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POS_TOL = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = EC.K


def run(cases, ids=None, **kw):
    ids = list(range(len(cases))) if ids is None else ids
    return molpack.to_host(E.embed_mols([c[0] for c in cases], DEV, K, EC.SEED, inputs=[c[1:] for c in cases], mol_ids=ids, **kw))


def conformer(res, m, c):
    a0, n = int(res['atom_ptr'][m]), int(res['n_atoms'][m])
    out = {k: res[k][m, c] for k in E.CONF_KEYS + E.VALUE_KEYS}
    out['pos'], out['h_pos'] = res['pos'][c, a0:a0 + n], res['h_pos'][c, a0:a0 + n]
    return out


def test_bounds_equal_the_restatement_bit_for_bit():
    cases = EC.all_cases()
    got = run(cases, max_iters=0, keep_bounds=True)
    for m, b in enumerate(EC.bounds()):
        for k in E.BOUNDS_KEYS:
            assert got['bounds_' + k][m] == b[k], (m, k, got['bounds_' + k][m], b[k])
        na = b['n_all']
        assert got['lower'][m, :na, :na].tobytes() == np.ascontiguousarray(b['lower']).tobytes(), m
        assert got['upper'][m, :na, :na].tobytes() == np.ascontiguousarray(b['upper']).tobytes(), m
        assert np.array_equal(got['cls'][m, :na, :na], b['cls']), m
    c = EC.inconsistent()
    bad = run([c], tables=EC.absurd_tables(), keep_bounds=True)
    ref = E.bounds_ref(c[0], c[1], c[2], c[4], EC.absurd_tables())
    assert all(bad['bounds_' + k][0] == ref[k] for k in E.BOUNDS_KEYS) and ref['status'] == E.STATUS_INCONSISTENT
    assert (bad['status'] == E.STATUS_INCONSISTENT).all() and not bad['pos'].any() and not bad['attempts'].any()


@pytest.mark.parametrize('max_iters', [5, 50])
def test_runs_follow_the_restatement(max_iters):
    cases, refs, bounds = EC.all_cases(), EC.refs(max_iters), EC.bounds()
    near = {(m, c) for m, row in enumerate(refs) for c, (_, tr) in enumerate(row) if E.near_threshold(bounds[m], trace=tr)}
    assert len(near) <= len(cases) * K // 10
    got = run(cases, max_iters=max_iters)
    worst = 0.0
    for m, row in enumerate(refs):
        for c, (ref, _) in enumerate(row):
            if (m, c) in near:
                continue
            r = conformer(got, m, c)
            for k in E.CONF_KEYS:
                assert r[k] == ref[k], (m, c, k, r[k], ref[k])
            for k in ('pos', 'h_pos'):
                diff = float(np.abs(r[k] - ref[k]).max(initial=0.0))
                worst = max(worst, diff)
                print('molecule', m, 'conformer', c, k, 'max abs diff', diff)
                assert diff <= POS_TOL, (m, c, k, diff)
    out = os.path.join(ROOT, 'profiles', 'embed_accuracy.txt')
    if max_iters == 50 and os.access(os.path.dirname(out), os.W_OK):
        with open(out, 'w') as f:
            f.write('mdx_mol_embed against embed_ref, %d named and random molecules x %d conformers as one batch, max_iters 50 per stage '
                    '(tests/test_gpu_embed.py, MI355X)\n' % (len(cases), K))
            f.write('largest absolute difference of the embedded positions: %.3e Angstrom (bound %.0e); statuses, attempts, iteration and '
                    'evaluation counts equal; %d conformer(s) left out for near-threshold decisions\n' % (worst, POS_TOL, len(near)))
    assert worst <= 1e-8 or max_iters != 50, 'positions agree to the bound but not to 1e-8: find out why (see the docstring)'


def test_full_length_results_stand_without_following_the_trajectory_and_do_not_depend_on_the_batch():
    cases, bounds = EC.all_cases(), EC.bounds()
    got = run(cases)
    n_ok = 0
    for m, b in enumerate(bounds):
        for c in range(K):
            r = conformer(got, m, c)
            if r['status'] != E.STATUS_OK:
                continue
            n_ok += 1
            viol = E.violation_ref(E.allatom(r['pos'], r['h_pos'], b['h']), b)
            assert viol <= E.DEFAULT_VIOL_TOL and abs(viol - r['max_violation']) <= 1e-10 * max(viol, 1e-300), (m, c, viol, r['max_violation'])
        if b['n_all'] > 2:
            assert not np.array_equal(conformer(got, m, 0)['pos'], conformer(got, m, 1)['pos']), m
    assert n_ok >= len(cases) * K * 3 // 4
    ids = list(range(len(cases)))
    back = run(cases[::-1], ids[::-1])                                  # the same (seed, id, conformer) at another place of the batch
    for m in range(len(cases)):
        for c in range(K):
            a, b = conformer(got, m, c), conformer(back, len(cases) - 1 - m, c)
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), (m, c)
    again = run(cases)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    other = run(cases[:3], [7, 8, 9])                                   # another id: other random numbers
    assert not np.array_equal(other['pos'][0, :int(got['n_atoms'][0])], got['pos'][0, :int(got['n_atoms'][0])])


def test_sizes_select_a_molecule_past_the_arrays_no_molecule_and_refused_calls():
    ladder = RC.ladder()
    cases = ladder + [EC.named()['formamide'], EC.named()['propane']]
    want = EC.ladder_bounds()
    got = run(cases, max_iters=2, max_attempts=1, na_cap=256)
    assert [w['status'] for w in want] == [0] * 9 + [1] and [w['n_all'] for w in want[:9]] == list(RC.LADDER)
    for m, w in enumerate(want):
        assert all(got['bounds_' + k][m] == w[k] for k in E.BOUNDS_KEYS), (m, [(k, got['bounds_' + k][m], w[k]) for k in E.BOUNDS_KEYS])
        for c in (0, K - 1):
            ref = E.embed_ref(w, c, EC.SEED, m, max_iters=2, max_attempts=1)
            r = conformer(got, m, c)
            assert all(r[k] == ref[k] for k in E.CONF_KEYS), (m, c, [(k, r[k], ref[k]) for k in E.CONF_KEYS])
            assert np.abs(r['pos'] - ref['pos']).max(initial=0.0) <= POS_TOL
    # the arrays by hand: select, then a molecule whose extent leaves the arrays
    mols = [c[0] for c in cases]
    p = molpack.pack_mols(mols, R.ForceFieldTables().atomic_numbers, positions=True)
    cm = molpack.CompactMols.from_packed({k: torch.from_numpy(v).to(DEV) for k, v in p.items()})
    cat = lambda xs, dt: torch.from_numpy(np.concatenate([np.asarray(x, dtype=dt).reshape(-1) for x in xs] + [np.zeros(1, dtype=dt)])).to(DEV)
    order, h_count, flag = cat([c[1] for c in cases], np.int32), cat([c[2] for c in cases], np.int32), cat([c[4] for c in cases], np.int32)
    ids = torch.arange(len(cases), dtype=torch.int64, device=DEV)
    N, masked = int(p['n_atoms'].sum()), len(cases) - 2
    select = torch.ones(len(cases), dtype=torch.int32, device=DEV)
    select[masked] = 0
    out = molpack.to_host(E.launch(cm, order, h_count, flag, K, EC.SEED, mol_ids=ids, select=select, max_iters=2, max_attempts=1))
    a0, na = int(p['atom_ptr'][masked]), int(p['n_atoms'][masked])
    for k in E.CONF_KEYS + E.VALUE_KEYS:
        assert not out[k][masked].any() and np.array_equal(np.delete(out[k], masked, 0), np.delete(got[k], masked, 0)), k
    assert not out['pos'][:, a0:a0 + na].any() and not out['h_pos'][:, a0:a0 + na].any() and not out['bounds_n_all'][masked]
    keep = np.r_[0:a0, a0 + na:N]
    assert np.array_equal(out['pos'][:, :N][:, keep], got['pos'][:, keep])
    tb = R.ForceFieldTables()
    B, cap = len(cases), 256
    short = cm._replace(N_cap=N - 1)
    ws = torch.zeros(17 * B * cap * cap, dtype=torch.uint8, device=DEV)
    bstats = torch.full((B, len(E.BOUNDS_KEYS)), 7, dtype=torch.int32, device=DEV)
    cstats = torch.full((B, K, len(E.CONF_KEYS)), 7, dtype=torch.int32, device=DEV)
    values = torch.full((B, K, len(E.VALUE_KEYS)), 7.0, dtype=torch.float64, device=DEV)
    po, hp = torch.full((K, N - 1, 3), 7.0, dtype=torch.float64, device=DEV), torch.full((K, N - 1, 4, 3), 7.0, dtype=torch.float64, device=DEV)   # the conformer stride is N_cap
    hist = torch.empty(B * K * E.HIST_PER_ATOM * cap, dtype=torch.float64, device=DEV)
    ops, at = short.operands()
    L = _lib.lib()
    bounds = lambda nB, tol, ws_bytes: L.mdx_mol_bounds(nB, *ops[1:], None, at(order), at(h_count), at(flag), 7, 4, tb.rows.ctypes.data, len(tb.rows), tol, 0.04,
                                                        0.06, 0.6, cap, at(ws), ws_bytes, at(bstats), _lib.stream())
    embed = lambda nB, viol, hist_ptr: L.mdx_mol_embed(nB, *ops[1:], None, at(h_count), at(ids), at(ws), ws.numel(), cap, at(bstats), K, EC.SEED, 2, 1, 1e-3, 1.0,
                                                       viol, at(po), at(hp), at(cstats), at(values), hist_ptr, hist.numel() * 8, _lib.stream())
    # refused calls write nothing and say why
    assert bounds(B, -1.0, ws.numel()) == 1 and b'tol12' in L.mdx_last_error()
    assert bounds(B, 0.01, ws.numel() - 1) == 1 and b'workspace' in L.mdx_last_error()
    assert embed(B, 0.0, at(hist)) == 1 and b'viol_tol' in L.mdx_last_error()
    assert embed(B, 0.1, None) == 1 and b'null' in L.mdx_last_error()
    assert bounds(0, 0.01, ws.numel()) == 0 and embed(0, 0.1, at(hist)) == 0
    torch.cuda.synchronize()
    assert bool((bstats == 7).all()) and bool((cstats == 7).all()) and bool((values == 7.0).all()) and bool((po == 7.0).all()) and bool((hp == 7.0).all())
    _lib.check(bounds(B, 0.01, ws.numel()))
    _lib.check(embed(B, 0.1, at(hist)))
    torch.cuda.synchronize()
    last = B - 1
    a0 = int(p['atom_ptr'][last])
    assert bstats[last].tolist() == [0] * len(E.BOUNDS_KEYS) and not cstats[last].any() and not values[last].any()
    assert bool((po[:, a0:] == 7.0).all()) and bool((hp[:, a0:] == 7.0).all())
    assert np.array_equal(cstats[:last].cpu().numpy()[:, :, 4], got['n_evals'][:last]) and np.array_equal(po[:, :a0].cpu().numpy(), got['pos'][:, :a0])
    none = molpack.to_host(E.embed_mols([], DEV, K, EC.SEED, inputs=[]))
    assert none['status'].shape == (0, K) and none['pos'].shape == (K, 0, 3)


def test_global3d_equals_the_chain_of_the_existing_modules():
    from moldiff_amd import canon, rmsd
    names, cases = EC.named_lists()
    mols = [c[0] for c in cases]
    g = E.global3d_mols(mols, DEV, K, EC.SEED, relax_iters=30)
    p, cm, ops, emb = E.embed_mols(mols, DEV, K, EC.SEED, with_inputs=True)
    emb_h = molpack.to_host(dict(emb))
    assert all(np.array_equal(emb_h[k], g[k]) for k in E.CONF_KEYS + E.VALUE_KEYS + tuple('bounds_' + b for b in E.BOUNDS_KEYS) + ('n_atoms', 'atom_ptr'))
    assert np.array_equal(emb_h['pos'], g['embed_pos']) and np.array_equal(emb_h['h_pos'], g['embed_h_pos'])
    B = len(mols)
    for c in range(K):
        moved = [dict(info, atom_pos=emb_h['pos'][c, int(p['atom_ptr'][m]):int(p['atom_ptr'][m]) + len(info['element'])].astype(np.float32)) for m, info in enumerate(mols)]
        hp = lambda m: emb_h['h_pos'][c, int(p['atom_ptr'][m]):int(p['atom_ptr'][m]) + len(mols[m]['element'])]
        inputs = [(molpack.host(ops[0])[int(p['bond_ptr'][m]):int(p['bond_ptr'][m]) + int(p['n_bonds'][m])],
                   molpack.host(ops[2])[int(p['atom_ptr'][m]):int(p['atom_ptr'][m]) + len(mols[m]['element'])], hp(m),
                   molpack.host(ops[3])[int(p['atom_ptr'][m]):int(p['atom_ptr'][m]) + len(mols[m]['element'])]) for m in range(B)]
        rel = molpack.to_host(R.relax_mols(moved, DEV, max_iters=30, inputs=inputs))
        targets = [dict(info, atom_pos=R.mol_result(rel, m)['pos'].astype(np.float32)) for m, info in enumerate(mols)]
        pr = molpack.to_host(rmsd.pairs_mols(mols, targets, [(m, m) for m in range(B)], DEV))
        assert np.array_equal(pr['msd'], g['msd'][:, c]) and np.array_equal(pr['msd_mirror'], g['msd_mirror'][:, c]), c
        ok = (emb_h['status'][:, c] == 0) & (rel['status'] == 0) & (pr['pair_status'] == rmsd.STATUS_OK)
        assert np.array_equal(ok, g['ok'][:, c]) and np.array_equal(rel['pos'], g['pos'][c]) and np.array_equal(rel['h_pos'], g['h_pos'][c])
    want = E.spread(g['msd'], g['ok'])
    for m in range(B):
        assert all(np.array_equal(g[k][m], want[k][m], equal_nan=True) for k in want)
        if g['ok'][m].any():
            assert np.isfinite(g['rmsd_max'][m]) and g['rmsd_max'][m] >= g['rmsd_median'][m] >= g['rmsd_min'][m] >= 0.0, names[m]
    assert (g['n_matched'] > 0).sum() >= B // 2
    s = E.summary(g)
    assert s['n_molecules'] == B and s['n_conformers'] == K and 0.0 <= s['fraction_ok'] <= 1.0
    # the parts of two batches join to the whole (the ids keep the random numbers) and nothing joins to nothing
    ids = list(range(B))
    whole = E.global3d_mols(mols, DEV, K, EC.SEED, relax_iters=30, mol_ids=ids)
    joined = E.concat([E.global3d_mols(mols[:4], DEV, K, EC.SEED, relax_iters=30, mol_ids=ids[:4]),
                       E.global3d_mols(mols[4:], DEV, K, EC.SEED, relax_iters=30, mol_ids=ids[4:])])
    assert set(joined) == set(whole) == set(E.empty(K)) and all(np.array_equal(joined[k], whole[k], equal_nan=True) for k in whole)
    none = E.global3d_mols([], DEV, K, EC.SEED)
    assert all(np.asarray(none[k]).shape == np.asarray(v).shape for k, v in E.empty(K).items()) and E.summary(E.empty(K))['n_molecules'] == 0
    with pytest.raises(ValueError, match='2\\^56'):
        E.embed_mols(mols[:1], DEV, K, EC.SEED, mol_ids=[1 << 56])


def test_embed_batch_on_a_two_step_sample_equals_embed_mols_of_its_molecules():
    import moldiff_amd as M
    from moldiff_amd.harness import default_config, placeholder_from_sizes
    from moldiff_amd.postprocess import FeaturizeMol
    feat = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    model = M.MolDiff(default_config('MolDiff_simple'), 8, 6).eval()
    model.load_state_dict(M.recipe_state_dict(model, 20230807), strict=True)
    model = model.to(DEV)
    sizes = [9, 14, 6, 11]
    ph = placeholder_from_sizes(sizes, DEV)
    out = model.sample(len(sizes), ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], seed=11, return_traj=False, num_steps=2)
    args = (out['pred'], ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], len(sizes))
    decoded = feat.decode_batch(*args)
    listed = molpack.to_host(E.embed_mols(decoded, DEV, 2, EC.SEED, max_iters=20))
    _, _, res = feat.embed_batch(*args, n_confs=2, seed=EC.SEED, max_iters=20)
    res = molpack.to_host(res)
    for k in E.CONF_KEYS + E.VALUE_KEYS + tuple('bounds_' + b for b in E.BOUNDS_KEYS):
        assert np.array_equal(res[k], listed[k]), k
    for m in range(len(sizes)):
        a0, la, na = int(res['atom_ptr'][m]), int(listed['atom_ptr'][m]), len(decoded[m]['element'])
        assert np.array_equal(res['pos'][:, a0:a0 + na], listed['pos'][:, la:la + na]) and np.array_equal(res['h_pos'][:, a0:a0 + na], listed['h_pos'][:, la:la + na]), m


def test_command_line_stats_and_compare(tmp_path, capsys):
    import json
    from moldiff_amd import rmsd
    cases = EC.named()
    mols = [dict(cases[k][0], mol_id=10 + q) for q, k in enumerate(('propane', 'formamide'))]
    torch.save({'finished': mols, 'failed': []}, str(tmp_path / 'samples_all.pt'))
    out, sdf = str(tmp_path / 'global3d.npz'), str(tmp_path / 'conformers.sdf')
    assert E.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', out, '--sdf', sdf, '--confs', '2', '--seed', '3', '--device', DEV]) == 0
    printed = json.loads(capsys.readouterr().out)
    saved = molpack.load_npz(out)
    direct = E.global3d_mols(mols, DEV, 2, 3, mol_ids=[10, 11])
    assert set(saved) == set(direct) and all(np.array_equal(saved[k], direct[k], equal_nan=True) for k in direct)
    want = json.loads(json.dumps(E.summary(saved)))
    same = lambda a, b: a == b or (a != a and b != b)
    assert printed.keys() == want.keys() and all(same(printed[k], want[k]) for k in want) and printed['n_molecules'] == 2
    back = rmsd.read_sdf(sdf)
    assert len(back) == int(saved['ok'].sum()) > 0
    assert E.main(['compare', out, out]) == 0
    cmp = json.loads(capsys.readouterr().out)
    assert cmp['rmsd_median'] == 0.0 and cmp['fraction_ok'][0] == cmp['fraction_ok'][1]
    with pytest.raises(SystemExit):
        E.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', out, '--ref'])


def test_entry_point_writes_the_global3d_files(tmp_path):
    import json
    from moldiff_amd import rmsd
    from .test_gpu_kekule import _sample
    new = {'global3d.json', 'global3d.npz', 'conformers.sdf'}
    # the directory names are permutations of each other, so the runs sample the same molecules
    d0, pool0 = _sample(tmp_path, 'abc', ['--largest_fragment', '0.2', '--hydrogens'])
    assert not new & set(os.listdir(d0))
    d1, pool = _sample(tmp_path, 'bca', ['--largest_fragment', '0.2', '--global3d', '2', '--global3d_seed', '5'])   # implies --hydrogens
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new) and new <= set(os.listdir(d1))
    assert len(pool['finished']) >= 2 and [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    for name in ('hydrogens.npz', 'kekule.npz'):
        a, b = molpack.load_npz(os.path.join(d0, name)), molpack.load_npz(os.path.join(d1, name))
        assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a), name
    for name in ('samples_allatom.sdf', 'samples_kekule.sdf'):
        with open(os.path.join(d0, name)) as fa, open(os.path.join(d1, name)) as fb:
            assert fa.read() == fb.read(), name
    saved = molpack.load_npz(os.path.join(d1, 'global3d.npz'))
    mols = pool['finished']
    direct = E.global3d_mols(mols, DEV, 2, 5, mol_ids=[int(m['mol_id']) for m in mols])
    assert set(saved) == set(direct) and all(np.array_equal(saved[k], direct[k], equal_nan=True) for k in direct)
    assert saved['msd'].shape == (len(mols), 2) and (saved['n_matched'] <= 2).all()
    with open(os.path.join(d1, 'global3d.json')) as f:
        got = json.load(f)
    want = json.loads(json.dumps(E.summary(saved)))
    same = lambda a, b: a == b or (a != a and b != b)
    assert got.keys() == want.keys() and all(same(got[k], want[k]) for k in want) and got['n_molecules'] == len(mols) and got['n_conformers'] == 2
    back = rmsd.read_sdf(os.path.join(d1, 'conformers.sdf'))
    assert len(back) <= int(saved['ok'].sum())
    for b in back:
        assert any(np.array_equal(b['element'], m['element']) for m in mols)
