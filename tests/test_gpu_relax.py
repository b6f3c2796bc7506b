"""GPU tests of the force-field relaxation (mdx_mol_relax through relax.relax_mols, relax.launch and FeaturizeMol.relax_batch).  The oracle is the plain
restatement ``relax_ref`` / ``energy_ref``, which repeats the device's operations and reduction tree.  An evaluation is compared to 1e-10
of the sum of absolute term energies (components) or of absolute gradient contributions (an atom's gradient): at most 3e4 terms x
1.1e-16 is 3e-12, a margin of 30.  A run is compared in its integers exactly and in its positions to 1e-6 Angstrom, a tolerance that is
not derived: it allows rounding at 1e-15 to grow by 1e9 over the run; the largest difference seen goes to profiles/relax_accuracy.txt.
A molecule with a decision within 1e-9 (relative) of its threshold may be left out, at most 10 % of a set; the host test asserts that
the reference alone leaves out none.  The size ladder and the other-table case add a coarser look after one to three iterations:
the integers exactly, positions to the same 1e-6, and the 14 energies to 1e-10 of the largest of them (or of 1 kcal/mol), which is
not the derived evaluation bound and is not meant as one."""
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import relax as R
from . import relax_cases as RC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)
EVAL_TOL, POS_TOL = 1e-10, 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = R.MOL_KEYS + ('atom_ptr',)


def run(cases, **kw):
    return molpack.to_host(R.relax_mols([c[0] for c in cases], DEV, inputs=[c[1:] for c in cases], **kw))


def allatom(res, case, key, hkey):
    h = np.clip(np.asarray(case[2]), 0, 4)
    return np.concatenate([res[key].reshape(-1, 3)] + [res[hkey][a, :h[a]].reshape(-1, 3) for a in range(len(h))])


def test_evaluation_of_the_named_and_random_sets_as_one_batch():
    cases = RC.all_cases()
    got = run(cases, max_iters=0)
    worst_e = worst_g = 0.0
    for m, (c, ev, (ref, _)) in enumerate(zip(cases, RC.evals(), RC.refs(0))):
        r = R.mol_result(got, m)
        for k in R.MOL_KEYS:
            assert r[k] == ref[k], (m, k, r[k], ref[k])
        if ref['status'] != R.STATUS_OK:
            assert not r['energy'].any() and not r['pos'].any() and not r['grad'].any()
            continue
        for q in range(5):
            bound = EVAL_TOL * ev['abs_components'][q]
            diff = abs(r['energy'][q] - ev['components'][q])
            worst_e = max(worst_e, diff / max(ev['abs_components'][q], 1e-300))
            print('molecule', m, R.COMPONENTS[q], 'diff', diff, 'bound', bound)
            assert diff <= bound, (m, q, diff, bound)
        assert abs(r['energy'][5] - ev['total']) <= EVAL_TOL * sum(ev['abs_components'])
        assert np.array_equal(r['energy'][:6], r['energy'][6:12])
        g = allatom(r, c, 'grad', 'h_grad')
        for a in range(ev['n_all']):
            diff = float(np.abs(g[a] - np.asarray(ev['grad'][a])).max())
            worst_g = max(worst_g, diff / max(ev['abs_grad'][a], 1e-300))
            assert diff <= EVAL_TOL * ev['abs_grad'][a], (m, a, diff, ev['abs_grad'][a])
    print('worst relative differences', worst_e, worst_g)


@pytest.mark.parametrize('max_iters', [5, 200])
def test_runs_follow_the_restatement(max_iters):
    cases = RC.all_cases()
    refs = RC.refs(max_iters)
    near = {m for m, (_, tr) in enumerate(refs) if R.near(tr, 1e-9)}
    assert len(near) <= len(cases) // 10
    got = run(cases, max_iters=max_iters)
    worst = 0.0
    for m, (c, (ref, _)) in enumerate(zip(cases, refs)):
        if m in near:
            continue
        r = R.mol_result(got, m)
        for k in R.MOL_KEYS:
            assert r[k] == ref[k], (m, k, r[k], ref[k])
        for k in ('pos', 'h_pos'):
            diff = float(np.abs(r[k] - ref[k]).max(initial=0.0))
            worst = max(worst, diff)
            print('molecule', m, k, 'max abs diff', diff)
            assert diff <= POS_TOL, (m, k, diff)
    out = os.path.join(ROOT, 'profiles', 'relax_accuracy.txt')
    if max_iters == 200 and os.access(os.path.dirname(out), os.W_OK):
        with open(out, 'w') as f:
            f.write('mdx_mol_relax against relax_ref, %d named and random molecules as one batch, max_iters 200 (tests/test_gpu_relax.py, MI355X)\n' % len(cases))
            f.write('largest absolute difference of the relaxed positions: %.3e Angstrom (bound %.0e); statuses, stop reasons, iteration and '
                    'evaluation counts equal; %d molecule(s) left out for near-threshold decisions\n' % (worst, POS_TOL, len(near)))
    assert worst <= 1e-8 or max_iters != 200, 'positions agree to the bound but not to 1e-8: find out why (see the docstring)'


def test_results_stand_without_following_the_trajectory():
    cases = RC.all_cases()
    got = run(cases, max_iters=200)
    for m, c in enumerate(cases):
        r = R.mol_result(got, m)
        if r['status'] != R.STATUS_OK:
            continue
        x = allatom(r, c, 'pos', 'h_pos')
        ev = R.energy_ref(*c, positions=x)
        for q in range(5):
            assert abs(r['energy'][6 + q] - ev['components'][q]) <= EVAL_TOL * ev['abs_components'][q], (m, q)
        gg = R._vdot(ev['grad'], ev['grad'])
        rms = np.sqrt(gg / (3.0 * ev['n_all']))
        assert abs(r['energy'][12] - rms) <= EVAL_TOL * max(ev['abs_grad']), (m, r['energy'][12], rms)
        assert r['energy'][11] <= r['energy'][5]
        if r['stop_reason'] == R.STOP_CONVERGED:
            assert r['energy'][12] <= R.DEFAULT_GTOL


def test_the_reversed_batch_and_a_second_run_are_byte_identical():
    cases = RC.all_cases()
    got = run(cases, max_iters=30)
    back = run(cases[::-1], max_iters=30)
    for m in range(len(cases)):
        a, b = R.mol_result(got, m), R.mol_result(back, len(cases) - 1 - m)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), m
    again = run(cases, max_iters=30)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def _operands(cases):
    mols = [c[0] for c in cases]
    p = molpack.pack_mols(mols, ELEMENTS, positions=True)
    cm = molpack.CompactMols.from_packed({k: torch.from_numpy(v).to(DEV) for k, v in p.items()})
    cat = lambda xs, dt, tail: torch.from_numpy(np.concatenate([np.asarray(x, dtype=dt).reshape((-1,) + tail) for x in xs] + [np.zeros((1,) + tail, dtype=dt)])).to(DEV)
    return p, cm, cat([c[1] for c in cases], np.int32, ()), cat([c[3] for c in cases], np.float64, (4, 3)), cat([c[2] for c in cases], np.int32, ()), \
        cat([c[4] for c in cases], np.int32, ())


def test_sizes_select_a_molecule_past_the_arrays_no_molecule_a_refused_call_and_other_tables():
    ladder = RC.ladder()
    cases = ladder + [RC.named()['formamide'], RC.named()['propane']]
    want = RC.ladder_refs(1) + [R.relax_ref(*c, max_iters=1) for c in cases[len(ladder):]]
    assert [w['status'] for w in want] == [0] * 9 + [1, 0, 0] and [w['n_all'] for w in want[:10]] == list(RC.LADDER) + [0]
    got = run(cases, max_iters=1)
    for m, w in enumerate(want):
        r = R.mol_result(got, m)
        assert all(r[k] == w[k] for k in R.MOL_KEYS), (m, [(k, r[k], w[k]) for k in R.MOL_KEYS if r[k] != w[k]])
        assert np.abs(r['pos'] - w['pos']).max(initial=0.0) <= POS_TOL and np.abs(r['energy'] - w['energy']).max() <= EVAL_TOL * max(1.0, np.abs(w['energy']).max())
    # select: the masked molecule has status 0 and zeros everywhere, its slots included; the others are unchanged
    p, cm, order, h_pos, h_count, flag = _operands(cases)
    N, masked = int(p['n_atoms'].sum()), len(cases) - 2
    select = torch.ones(len(cases), dtype=torch.int32, device=DEV)
    select[masked] = 0
    out = molpack.to_host(R.launch(cm, order, h_pos, h_count, flag, max_iters=1, select=select))
    a0, na = int(p['atom_ptr'][masked]), int(p['n_atoms'][masked])
    for k in R.STAT_KEYS:
        assert out[k][masked] == 0 and np.array_equal(np.delete(out[k], masked), np.delete(got[k], masked)), k
    assert not out['energy'][masked].any() and not out['pos'][a0:a0 + na].any() and not out['h_pos'][a0:a0 + na].any()
    keep = np.r_[0:a0, a0 + na:N]
    assert np.array_equal(out['pos'][:N][keep], got['pos'][keep])
    # a molecule whose extent leaves the arrays: status 0, zeros, and nothing of it is written (the arrays hold a sentinel)
    tb = R.ForceFieldTables()
    short = cm._replace(N_cap=N - 1)
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=DEV)
    po, hp, go, hg, en = f64(N, 3), f64(N, 4, 3), f64(N, 3), f64(N, 4, 3), f64(len(cases), len(R.ENERGY_KEYS))
    stats = torch.full((len(cases), len(R.STAT_KEYS)), 7, dtype=torch.int32, device=DEV)
    ws = torch.empty(len(cases) * R.WS_DOUBLES, dtype=torch.float64, device=DEV)
    ops, at = short.operands()
    L = _lib.lib()
    call = lambda B, gtol, ws_ptr: L.mdx_mol_relax(B, *ops[1:], None, at(cm.atom_pos), at(order), at(h_pos), at(h_count), at(flag), 7, 4, tb.rows.ctypes.data,
                                                   len(tb.rows), 1e-3, gtol, 0.3, 1, at(po), at(hp), at(go), at(hg), at(stats), at(en), ws_ptr, ws.numel() * 8,
                                                   _lib.stream())
    _lib.check(call(len(cases), 1e-2, at(ws)))
    torch.cuda.synchronize()
    last = len(cases) - 1
    a0 = int(p['atom_ptr'][last])
    assert stats[last].tolist() == [0] * len(R.STAT_KEYS) and not en[last].any()
    assert bool((po[a0:] == 7.0).all()) and bool((hp[a0:] == 7.0).all()) and bool((go[a0:] == 7.0).all()) and bool((hg[a0:] == 7.0).all())
    assert np.array_equal(stats[:last, 2].cpu().numpy(), got['iterations'][:last]) and np.array_equal(po[:a0].cpu().numpy(), got['pos'][:a0])
    # no molecule, through the module and through the entry; a refused call writes nothing and says why
    none, ref = molpack.to_host(R.relax_mols([], DEV)), R.empty()
    assert set(none) == set(ref) and all(none[k].shape == ref[k].shape for k in ref)
    stats.fill_(7)
    assert call(0, 1e-2, at(ws)) == 0 and call(len(cases), -1.0, at(ws)) == 1 and b'gtol' in L.mdx_last_error()
    assert call(len(cases), 1e-2, None) == 1 and b'null' in L.mdx_last_error()
    torch.cuda.synchronize()
    assert bool((stats == 7).all())
    # another parameter table changes the results as the reference says
    import yaml
    with open(R.DEFAULT_TABLE) as f:
        table = yaml.safe_load(f)
    table['elements'][6]['variants']['tetrahedral']['r'] = 0.8
    del table['elements'][7]['variants']['trigonal']
    other = R.ForceFieldTables(table=table)
    sub = cases[len(ladder):]
    want2 = [R.relax_ref(*c, other, max_iters=3) for c in sub]
    assert want2[0]['n_fallback'] == 1 and want2[1]['energy'][5] != want[-1]['energy'][5]
    got2 = run(sub, tables=other, max_iters=3)
    for m, w in enumerate(want2):
        r = R.mol_result(got2, m)
        assert all(r[k] == w[k] for k in R.MOL_KEYS) and np.abs(r['pos'] - w['pos']).max() <= POS_TOL
        assert np.abs(r['energy'] - w['energy']).max() <= EVAL_TOL * np.abs(w['energy']).max()


def test_relax_batch_on_a_two_step_sample_equals_relax_mols_of_its_molecules():
    import moldiff_amd as M
    from moldiff_amd.harness import default_config, placeholder_from_sizes
    from moldiff_amd.postprocess import FeaturizeMol
    feat = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    model = M.MolDiff(default_config('MolDiff_simple'), 8, 6).eval()
    model.load_state_dict(M.recipe_state_dict(model, 20230807), strict=True)
    model = model.to(DEV)
    sizes = [9, 14, 6, 11]
    ph = placeholder_from_sizes(sizes, DEV)
    out = model.sample(len(sizes), ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], seed=11, return_traj=False, num_steps=2)
    args = (out['pred'], ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'], len(sizes))
    decoded = feat.decode_batch(*args)
    listed = molpack.to_host(R.relax_mols(decoded, DEV, max_iters=20))
    assert listed['n_atoms'].sum() > 0 and (listed['n_all'] >= listed['n_atoms']).all()
    select = torch.tensor([1, 0, 1, 1], device=DEV)
    for sel, masked in ((None, ()), (select, (1,))):
        _, _, res = feat.relax_batch(*args, select=sel, max_iters=20)
        res = molpack.to_host(res)
        for m in range(len(sizes)):
            zero = m in masked
            for k in R.MOL_KEYS:
                assert res[k][m] == (0 if zero else listed[k][m]), (k, m)
            assert np.array_equal(res['energy'][m], listed['energy'][m] * (not zero)), m
            a0, la, na = int(res['atom_ptr'][m]), int(listed['atom_ptr'][m]), len(decoded[m]['element'])
            for k in R.ATOM_FLOAT_KEYS:
                assert np.array_equal(res[k][a0:a0 + na], listed[k][la:la + na] * (not zero)), (k, m)
    with pytest.raises(ValueError, match='another featuriser'):
        feat.relax_batch(*args, R.ForceFieldTables(atomic_numbers=(6, 7, 8)))


def test_entry_point_writes_the_relaxation_files(tmp_path):
    import json
    from moldiff_amd import hydrogens as H
    from moldiff_amd import kekule as K
    from moldiff_amd import rmsd
    from .test_gpu_kekule import _sample
    new = {'relax.json', 'relax.npz', 'samples_relaxed.sdf'}
    # the directory names are permutations of each other, so the runs sample the same molecules
    d0, pool0 = _sample(tmp_path, 'abc', ['--largest_fragment', '0.2', '--hydrogens'])
    assert not new & set(os.listdir(d0))
    d1, pool = _sample(tmp_path, 'bca', ['--largest_fragment', '0.2', '--relax', '--relax_iters', '5', '--relax_gtol', '0.02'])   # implies --hydrogens
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new) and new <= set(os.listdir(d1))
    assert len(pool['finished']) >= 2 and [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']]
    for name in ('hydrogens.npz', 'kekule.npz'):
        a, b = molpack.load_npz(os.path.join(d0, name)), molpack.load_npz(os.path.join(d1, name))
        assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a), name
    saved = molpack.load_npz(os.path.join(d1, 'relax.npz'))
    mols = pool['finished']
    assert len(saved['status']) == len(mols) and (saved['iterations'] <= 5).all()
    inputs = R._inputs(mols, R.ForceFieldTables())
    left = 0
    for m, (info, inp) in enumerate(zip(mols, inputs)):
        kr = K.kekulize_ref(info)
        if H.near_threshold(info, kr['kek_h'], kr['kek_order']) or R.near_threshold(info, *inp, max_iters=5, gtol=0.02):
            left += 1
            continue
        ref, r = R.relax_ref(info, *inp, max_iters=5, gtol=0.02), R.mol_result(saved, m)
        assert all(r[k] == ref[k] for k in R.MOL_KEYS), (m, [(k, r[k], ref[k]) for k in R.MOL_KEYS if r[k] != ref[k]])
        assert np.abs(r['pos'] - ref['pos']).max() <= POS_TOL and np.abs(r['h_pos'] - ref['h_pos']).max() <= POS_TOL, m
    assert left <= 1
    with open(os.path.join(d1, 'relax.json')) as f:
        got = json.load(f)
    want = json.loads(json.dumps(R.summary(saved)))
    same = lambda a, b: a == b or (a != a and b != b) or (isinstance(a, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a))
    assert got.keys() == want.keys() and all(same(got[k], want[k]) for k in want) and got['n_molecules'] == len(mols)
    kek = K.stack_ref(mols)
    written = [k for k in range(len(mols)) if K.kekulizable(kek)[k] and (K.mol_result(kek, k)['kek_order'] >= 1).all() and saved['status'][k] == 0]
    back = rmsd.read_sdf(os.path.join(d1, 'samples_relaxed.sdf'))
    assert len(back) == len(written)
    for b, k in zip(back, written):
        assert np.array_equal(b['element'], mols[k]['element']) and np.array_equal(b['bond_index'], mols[k]['bond_index'])
        assert np.abs(np.asarray(b['atom_pos'], dtype=np.float64) - R.mol_result(saved, k)['pos']).max() <= 1e-4     # the four decimals of a mol block
