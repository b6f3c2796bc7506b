"""GPU tests of scaffold-constrained sampling (MolDiff.sample(..., scaffold=, start_step=), mdx_scaffold_merge).

There is no reference to compare with (the reference has no conditional sampling): the merged rows are checked against the
formulas of q(x_k | x_0) -- the product's own training-side add_noise bit for bit, and a float64 restatement -- and the chain
against the invariants of replacement conditioning (free rows untouched, fixed rows end on the known molecule, results do not
depend on sharding, absent keywords change nothing).
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moldiff_amd import Scaffold, _lib
from moldiff_amd.postprocess import FeaturizeMol
from moldiff_amd.sample_drug3d import mol_block, read_mol_block
from tests import test_scaffold_host as H
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = 1000


@pytest.fixture(scope='module', autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f'\n[test_gpu_scaffold] wall time of this file: {time.time() - t0:.1f} s')


def _model():
    return U.moldiff('MolDiff_simple', DEV)


def _random_scaffold(sizes, seed, frac=0.5, all_rows=None):
    """Random known molecule for a packed batch on the device (atom classes 0..6, bond classes 0..4: nothing the decoder drops)."""
    g = U.rng(seed)
    bn, hei, bh, _, _ = U.graph_from_sizes(sizes, DEV)
    N, Eh = int(bn.numel()), int(bh.numel())
    mask = g.random(N) < frac if all_rows is None else np.full(N, all_rows)
    sc = Scaffold(torch.from_numpy(mask).to(DEV), torch.from_numpy(g.integers(0, 7, N)).to(DEV),
                  U.t32(1.5 * g.standard_normal((N, 3))).to(DEV), torch.from_numpy(g.integers(0, 5, Eh)).to(DEV))
    return (bn, hei, bh), sc


def _snapshot(sm, frames):
    st = {k: v.clone() for k, v in sm.state().items()}
    st.update(node_ids=sm.node_ids[:frames].clone(), half_ids=sm.half_ids[:frames].clone(), pos_traj=sm.pos_traj[:frames].clone(),
              **{f'pred{j}': p.clone() for j, p in enumerate(sm.preds)})
    return st


@U.both_paths
def test_absent_keywords_and_an_all_false_mask_change_nothing():
    m = _model()
    sizes = [9, 14, 11, 7, 16, 12, 10, 13]
    (bn, hei, bh), sc = _random_scaffold(sizes, 1, all_rows=False)
    runs = []
    for kw in ({}, dict(scaffold=None, start_step=None), dict(scaffold=sc)):
        sm = m.sampler(len(sizes), bn, hei, bh, seed=17, **kw)
        sm.init()
        for i in range(30):
            sm.step(i)
        runs.append(_snapshot(sm, 31))
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert torch.equal(v, other[k]), k


def _onehot_state(g, N, Eh):
    hn = F.one_hot(torch.from_numpy(g.integers(0, 8, N)), 8).float().to(DEV)
    hh = F.one_hot(torch.from_numpy(g.integers(0, 6, Eh)), 6).float().to(DEV)
    pos = U.t32(g.standard_normal((N, 3))).to(DEV)
    return hn, pos, hh, torch.log(hn.clamp(min=1e-30)), torch.log(hh.clamp(min=1e-30))


def test_free_rows_are_untouched_by_the_merge():
    m = _model()
    sizes = [9, 14, 11, 7, 16, 12]
    (bn, hei, bh), sc = _random_scaffold(sizes, 2)
    N, Eh = int(bn.numel()), int(bh.numel())
    g = U.rng(3)
    state = _onehot_state(g, N, Eh)
    nz = {}

    def noise(draw):   # fresh values per draw index, the same for both samplers
        if draw not in nz:
            gd = U.rng(1000 + draw)
            nz[draw] = (U.t32(gd.standard_normal((N, 3))).to(DEV), U.t32(gd.random((N, 8), dtype=np.float32)).to(DEV),
                        U.t32(gd.random((Eh, 6), dtype=np.float32)).to(DEV))
        return nz[draw]

    i, got = 400, []
    for kw in ({}, dict(scaffold=sc)):
        sm = m.sampler(len(sizes), bn, hei, bh, noise=noise, **kw)
        sm.set_state(*state, frame=i)
        sm.step(i)
        got.append(dict(_snapshot(sm, 0), ids_n=sm.node_ids[sm.pcur].clone(), ids_h=sm.half_ids[sm.pcur].clone()))
    assert sorted(nz) == [i + 1, T + 1 + i]     # the scaffold asked the callable for a draw index of its own
    nm, _, _, _, hm = sc.resolve(N, hei, 8, 6)
    plain, cond = got
    for k, mask in (('h_node', nm), ('pos', nm), ('log_node', nm), ('ids_n', nm), ('h_halfedge', hm), ('log_halfedge', hm), ('ids_h', hm)):
        assert torch.equal(plain[k][~mask], cond[k][~mask]), k
    for j in range(3):   # the prediction is the denoiser's own before the end of the chain
        assert torch.equal(plain[f'pred{j}'], cond[f'pred{j}'])
    assert not torch.equal(plain['pos'][nm], cond['pos'][nm])   # and the fixed rows were in fact replaced


def test_merged_rows_follow_the_formula_of_q_xk_given_x0():
    """k = T-1 (init), the middle of the chain and k = 0, with explicit noise.  Classes: bit-equal to the training-side add_noise on the
    device (same row function), and to the float64 restatement outside its 1e-4 margin (skipped share <= 0.5 %, as the host test
    established for these inputs).  Positions against float64 from the fp32 alphas_bar: |err| <= 4 * 2^-23 (|a x0| + |b eps|) --
    four fp32 roundings (sqrt, subtract, multiply, add) of 2^-24 each, times 2 for a sqrtf that is not correctly rounded."""
    m = _model()
    inp = H.formula_inputs(T)
    bn, hei, bh = (inp[k].to(DEV) for k in ('bn', 'hei', 'bh'))
    N, Eh, B = int(bn.numel()), int(bh.numel()), len(H.FORMULA_SIZES)
    sc = Scaffold(inp['node_mask'].to(DEV), inp['node_type'].to(DEV), inp['node_pos'].to(DEV), inp['halfedge_type'].to(DEV))
    nm, hm = inp['node_mask'], inp['halfedge_mask']
    chain_noise = (torch.zeros(N, 3, device=DEV), torch.full((N, 8), 0.5, device=DEV), torch.full((Eh, 6), 0.5, device=DEV))
    log_off = float(torch.log(torch.tensor([1e-30], dtype=torch.float32))[0])
    abar = m.pos_transition.alphas_bar.cpu()
    for k in H.formula_levels(T):
        eps, un, uh = inp['noise'][k]
        scaffold_draw = 2 * T + 1 if k == T - 1 else T + 1 + (T - 2 - k)
        noise = lambda draw: tuple(x.to(DEV) for x in inp['noise'][k]) if draw == scaffold_draw else chain_noise
        sm = m.sampler(B, bn, hei, bh, noise=noise, scaffold=sc)
        if k == T - 1:
            sm.init()
        else:
            i = T - 2 - k
            sm.set_state(*_onehot_state(U.rng(5), N, Eh), frame=i)
            sm.step(i)
        st = {kk: v.cpu() for kk, v in sm.state().items()}
        ids_n, ids_h = sm.node_ids[sm.pcur].cpu().long(), sm.half_ids[sm.pcur].cpu().long()
        tt = torch.full((B,), k, dtype=torch.int64, device=DEV)
        skipped = total = 0
        for tr, v0, batch, u, mask, oh, lg, ids, K in (
                (m.node_transition, inp['node_type'], bn, un, nm, st['h_node'], st['log_node'], ids_n, 8),
                (m.edge_transition, inp['halfedge_type'], bh, uh, hm, st['h_halfedge'], st['log_halfedge'], ids_h, 6)):
            cls = oh.argmax(-1)
            ref_oh, ref_lvt, _ = tr.add_noise(v0.to(DEV), tt, batch, u.to(DEV))
            assert torch.equal(cls[mask], ref_oh.argmax(-1).cpu()[mask])
            assert torch.equal(oh[mask], ref_oh.cpu()[mask]) and torch.equal(lg[mask], ref_lvt.cpu()[mask])
            c64, margin = H.classes_fp64(tr.q_mats.cpu(), v0[mask], k, u[mask])
            sure = margin >= H.MARGIN
            assert torch.equal(cls[mask][sure], c64[sure])
            skipped += int((~sure).sum()); total += int(sure.numel())
            # the four things a step writes for a row agree with each other
            assert torch.equal(oh[mask], F.one_hot(cls[mask], K).float())
            assert torch.equal(lg[mask], torch.where(oh[mask] > 0, torch.zeros(()), torch.full((), log_off)))
            assert torch.equal(ids[mask], cls[mask])
        print(f'level {k}: fp64 class test skipped {skipped} of {total} rows')
        assert skipped <= H.SKIP_CAP * total
        a, b = abar[k].double().sqrt(), (1.0 - abar[k].double()).sqrt()
        x0, e64 = inp['node_pos'].double(), eps.double()
        err = (st['pos'].double() - (a * x0 + b * e64)).abs()
        bound = 4 * 2.0 ** -23 * ((a * x0).abs() + (b * e64).abs())
        print(f'level {k}: max position error / bound = {float((err[nm] / bound[nm]).max()):.3f}')
        assert bool((err[nm] <= bound[nm]).all())


def test_end_of_chain_returns_the_scaffold_exactly():
    m = _model()
    sizes = [9, 14, 11, 7, 16, 12, 10, 13]
    g = U.rng(7)
    bn, hei, bh, _, _ = U.graph_from_sizes(sizes, DEV)
    N, Eh = int(bn.numel()), int(bh.numel())
    fixed_per_mol = [s // 2 for s in sizes]                      # the first half of every molecule's atoms
    off = np.concatenate([[0], np.cumsum(sizes)])
    mask = np.zeros(N, dtype=bool)
    for o, kf in zip(off, fixed_per_mol):
        mask[o:o + kf] = True
    sc = Scaffold(torch.from_numpy(mask).to(DEV), torch.from_numpy(g.integers(0, 7, N)).to(DEV),
                  U.t32(1.5 * g.standard_normal((N, 3))).to(DEV), torch.from_numpy(g.integers(0, 5, Eh)).to(DEV))
    out = m.sample(len(sizes), bn, hei, bh, seed=11, scaffold=sc)
    nm, nt, x0, ht, hm = sc.resolve(N, hei, 8, 6)
    assert out['traj'][1].shape[0] == T + 1
    assert torch.equal(out['traj'][1][-1][nm], x0[nm]) and torch.equal(out['pred'][1][nm], x0[nm])
    assert torch.equal(out['traj'][0][-1].dense()[nm], F.one_hot(nt[nm], 8).float())
    assert torch.equal(out['traj'][2][-1].dense()[hm], F.one_hot(ht[hm], 6).float())
    for pred, v0, msk in ((out['pred'][0], nt, nm), (out['pred'][2], ht, hm)):
        p = torch.softmax(pred[msk], dim=-1)
        assert torch.equal(p.argmax(-1), v0[msk]) and bool((p.max(-1).values == 1.0).all())
    assert torch.isfinite(out['pred'][1]).all() and not torch.equal(out['pred'][1][~nm], x0[~nm])
    feat = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    mols = feat.decode_batch(out['pred'], bn, hei, bh, len(sizes))
    ele = np.asarray(feat.atomic_numbers)
    nt_c, x0_c, ht_c, hei_c, bh_c = nt.cpu().numpy(), x0.cpu().numpy(), ht.cpu().numpy(), hei.cpu().numpy(), bh.cpu().numpy()
    for j, (info, o, kf) in enumerate(zip(mols, off, fixed_per_mol)):
        # fixed atoms come first and none of them is a mask-type atom, so they keep their indices through the decoder's compaction
        assert np.array_equal(info['element'][:kf], ele[nt_c[o:o + kf]])
        assert np.array_equal(info['atom_pos'][:kf], x0_c[o:o + kf]) and bool((info['atom_prob'][:kf] == 1.0).all())
        sel = (bh_c == j)
        want = {(int(a - o), int(b - o)): int(t) for a, b, t in zip(hei_c[0, sel], hei_c[1, sel], ht_c[sel]) if b - o < kf and t > 0}
        nb = info['bond_index'].shape[1] // 2
        got = {(int(a), int(b)): (int(t), float(p)) for a, b, t, p in zip(info['bond_index'][0, :nb], info['bond_index'][1, :nb],
                                                                          info['bond_type'][:nb], info['bond_prob'][:nb]) if b < kf}
        assert {k: v[0] for k, v in got.items()} == want and all(v[1] == 1.0 for v in got.values())


def test_philox_draws_have_the_distribution_of_q_xk_given_x0():
    """Without explicit noise: 21,000 atoms and 21,000 half-edges (7,000 molecules of 3 atoms) that all share one v0 / x0, noised to a
    middle level by the library's own per-molecule Philox streams.  5-sigma bounds: a class count is Binomial(n, p_j) with p = row v0 of
    q_mats[k]: |count_j - n p_j| <= 5 sqrt(n p_j (1 - p_j)); a position component is a x0 + b N(0, 1): |mean - a x0| <= 5 b / sqrt(n) and
    |var - b^2| <= 5 b^2 sqrt(2 / (n - 1)) (the variance of a normal sample's variance)."""
    m = _model()
    n_mol, k = 7000, T // 2
    bn, hei, bh, _, _ = U.graph_from_sizes([3] * n_mol, DEV)
    N, Eh = int(bn.numel()), int(bh.numel())
    v0n, v0h = 2, 1
    x0 = torch.tensor([1.5, -2.0, 0.5])
    sc = Scaffold(torch.zeros(N, dtype=torch.bool, device=DEV), torch.full((N,), v0n, dtype=torch.int64, device=DEV),
                  x0.repeat(N, 1).to(DEV), torch.full((Eh,), v0h, dtype=torch.int64, device=DEV))
    sm = m.sampler(n_mol, bn, hei, bh, seed=2024, scaffold=sc, start_step=k + 1, return_traj=False)
    sm.init()                                                   # every row <- q(x_k | x_0), draws from mdx_noise
    st = {kk: v.cpu() for kk, v in sm.state().items()}
    for oh, tr, v0, n, K in ((st['h_node'], m.node_transition, v0n, N, 8), (st['h_halfedge'], m.edge_transition, v0h, Eh, 6)):
        p = tr.q_mats[k].cpu().double()[v0]
        counts = torch.bincount(oh.argmax(-1), minlength=K).double()
        bound = 5.0 * torch.sqrt(n * p * (1.0 - p))
        print(f'K = {K}: counts {counts.tolist()}, expected {(n * p).tolist()}, 5-sigma {bound.tolist()}')
        assert n >= 20000 and bool(((counts - n * p).abs() <= bound).all())
    ab = m.pos_transition.alphas_bar[k].cpu().double()
    a, b = ab.sqrt(), (1.0 - ab).sqrt()
    pos = st['pos'].double()
    mean, var = pos.mean(0), pos.var(0, unbiased=True)
    print(f'position mean {mean.tolist()} (a x0 = {(a * x0.double()).tolist()}), variance {var.tolist()} (b^2 = {float(b * b)})')
    assert bool(((mean - a * x0.double()).abs() <= 5.0 * b / np.sqrt(N)).all())
    assert bool(((var - b * b).abs() <= 5.0 * b * b * np.sqrt(2.0 / (N - 1))).all())


def _cond_chain(m, sizes, sc_parts, mol_ids, seed, steps):
    bn, hei, bh, _, _ = U.graph_from_sizes(sizes, DEV)
    sm = m.sampler(len(sizes), bn, hei, bh, seed=seed, mol_ids=mol_ids, return_traj=False, scaffold=Scaffold(*sc_parts))
    sm.init()
    for i in range(steps):
        sm.step(i)
    st = sm.state()
    return [st[k].cpu() for k in ('pos', 'h_node', 'log_node')], [st[k].cpu() for k in ('h_halfedge', 'log_halfedge')]


@U.both_paths
def test_conditioned_chain_is_shard_invariant():
    m = _model()
    sizes = [9, 14, 11, 7, 16, 12]
    ids = np.arange(200, 206)
    _, sc = _random_scaffold(sizes, 8)
    n_lo = sum(sizes[:3])
    e_lo = sum(s * (s - 1) // 2 for s in sizes[:3])
    parts = lambda ns, es: (sc.node_mask[ns], sc.node_type[ns], sc.node_pos[ns], sc.halfedge_type[es])
    full = _cond_chain(m, sizes, parts(slice(None), slice(None)), ids, 99, 30)
    lo = _cond_chain(m, sizes[:3], parts(slice(0, n_lo), slice(0, e_lo)), ids[:3], 99, 30)
    hi = _cond_chain(m, sizes[3:], parts(slice(n_lo, None), slice(e_lo, None)), ids[3:], 99, 30)
    for f, a, b in zip(full[0], lo[0], hi[0]):
        assert torch.equal(f[:n_lo], a) and torch.equal(f[n_lo:], b)
    for f, a, b in zip(full[1], lo[1], hi[1]):
        assert torch.equal(f[:e_lo], a) and torch.equal(f[e_lo:], b)
    assert bool(sc.node_mask.any()) and not bool(sc.node_mask.all())     # fixed and free rows were both compared


def test_partial_chain_starts_from_the_noised_molecule_and_an_all_true_mask_ends_on_it():
    m = _model()
    sizes = [9, 14, 11, 7]
    s = 12
    (bn, hei, bh), sc = _random_scaffold(sizes, 9, all_rows=True)
    N, Eh = int(bn.numel()), int(bh.numel())
    out = m.sample(len(sizes), bn, hei, bh, seed=4, scaffold=sc, start_step=s)
    assert [t.shape[0] for t in out['traj']] == [s + 1] * 3
    assert torch.equal(out['traj'][1][-1], sc.node_pos) and torch.equal(out['pred'][1], sc.node_pos)
    assert torch.equal(out['traj'][0][-1].dense(), F.one_hot(sc.node_type, 8).float())
    assert torch.equal(out['traj'][2][-1].dense(), F.one_hot(sc.halfedge_type, 6).float())
    # all-false mask (SDEdit-style): the initial state is add_noise(x0, s - 1) under explicit noise, the chain is free afterwards
    free = Scaffold(torch.zeros_like(sc.node_mask), sc.node_type, sc.node_pos, sc.halfedge_type)
    g = U.rng(10)
    nz = (U.t32(g.standard_normal((N, 3))).to(DEV), U.t32(g.random((N, 8), dtype=np.float32)).to(DEV),
          U.t32(g.random((Eh, 6), dtype=np.float32)).to(DEV))
    sm = m.sampler(len(sizes), bn, hei, bh, noise=lambda draw: nz, scaffold=free, start_step=s)
    sm.init()
    st = sm.state()
    tt = torch.full((len(sizes),), s - 1, dtype=torch.int64, device=DEV)
    oh_n, lg_n, _ = m.node_transition.add_noise(sc.node_type, tt, bn, nz[1])
    oh_h, lg_h, _ = m.edge_transition.add_noise(sc.halfedge_type, tt, bh, nz[2])
    assert torch.equal(st['h_node'], oh_n) and torch.equal(st['log_node'], lg_n)
    assert torch.equal(st['h_halfedge'], oh_h) and torch.equal(st['log_halfedge'], lg_h)
    # positions: torch's own fp32 evaluation of the same expression (its sqrt is another library's) -- within the roundings of one
    # evaluation of it, 4 * 2^-23 (|a x0| + |b eps|) as derived for the formula test, doubled for the two evaluations compared
    ref = m.pos_transition.add_noise(sc.node_pos, tt, bn, nz[0])
    ab = m.pos_transition.alphas_bar[s - 1]
    bound = 2 * 4 * 2.0 ** -23 * ((ab.sqrt() * sc.node_pos).abs() + ((1 - ab).sqrt() * nz[0]).abs())
    print(f'partial chain: positions bit-equal to torch add_noise: {torch.equal(st["pos"], ref)}')
    assert bool(((st['pos'] - ref).abs() <= bound).all())
    for i in range(T - s, T):
        sm.step(i)
    res = sm.result()
    assert res['traj'][1].shape[0] == s + 1 and torch.isfinite(res['traj'][1]).all()
    assert not torch.equal(res['traj'][1][-1], sc.node_pos)     # nothing was held: the molecule moved
    with pytest.raises(ValueError, match='start_step'):
        m.sampler(len(sizes), bn, hei, bh, scaffold=sc, start_step=T + 1)
    with pytest.raises(ValueError, match='needs a scaffold'):
        m.sampler(len(sizes), bn, hei, bh, start_step=5)


def test_continuous_space_refuses_both_keywords():
    import copy
    import moldiff_amd as M
    from moldiff_amd.harness import default_config
    cfg = copy.deepcopy(default_config('MolDiff_simple'))
    cfg.diff.categorical_space = 'continuous'
    cfg.diff.scaling = [1., 4., 8.]
    mc = M.MolDiff(cfg, 8, 6).eval().to(DEV)
    (bn, hei, bh), sc = _random_scaffold([5, 6], 12)
    with pytest.raises(NotImplementedError):
        mc.sampler(2, bn, hei, bh, scaffold=sc)
    with pytest.raises(NotImplementedError):
        mc.sample(2, bn, hei, bh, start_step=10)


def test_cli_scaffold_runs_end_to_end(tmp_path):
    import glob
    import os
    import yaml
    from moldiff_amd import sample_drug3d
    idx = np.array([[0, 1, 2, 3, 4, 0], [1, 2, 3, 4, 5, 5]], dtype=np.int64)
    bt = np.array([4, 4, 4, 4, 4, 4], dtype=np.int64)
    ring = np.array([[np.cos(a), np.sin(a), 0.0] for a in np.arange(6) * np.pi / 3], dtype=np.float32) * 1.39 + np.float32(3.0)
    scaf = {'element': np.array([6, 6, 7, 6, 6, 8]), 'atom_pos': ring, 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
            'bond_type': np.concatenate([bt, bt])}
    sp = tmp_path / 'scaffold.mol'
    sp.write_text(mol_block(scaf))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, 'configs', 'sample_MolDiff_simple.yml')))
    cfg['sample'].update(num_mols=1, batch_size=2)
    cp = tmp_path / 'sample.yml'
    cp.write_text(yaml.safe_dump(cfg))
    log_dir = sample_drug3d.main(['--config', str(cp), '--outdir', str(tmp_path / 'out'), '--device', DEV, '--recipe-weights',
                                  '--scaffold', str(sp)])
    pool = torch.load(str(log_dir) + '/samples_all.pt', weights_only=False)
    mols = pool['finished'] + pool['failed']
    assert len(mols) >= 2
    given = read_mol_block(sp.read_text())
    centred = (given['atom_pos'].astype(np.float64) - given['atom_pos'].astype(np.float64).mean(0)).astype(np.float32)
    want = {(int(a), int(b)): int(t) for a, b, t in zip(idx[0], idx[1], bt)}

    def starts_with_scaffold(info, atol):
        assert len(info['element']) >= 6 and np.array_equal(np.asarray(info['element'][:6]), given['element'])
        assert np.abs(np.asarray(info['atom_pos'][:6]) - centred).max() <= atol
        nb = info['bond_index'].shape[1] // 2
        got = {(int(a), int(b)): int(t) for a, b, t in zip(info['bond_index'][0, :nb], info['bond_index'][1, :nb], info['bond_type'][:nb])
               if a < 6 and b < 6}
        assert got == want

    for info in mols:
        starts_with_scaffold(info, 0.0)
    files = glob.glob(str(log_dir) + '_SDF/*.sdf')
    assert len(files) == len(pool['finished'])
    for f in files:
        starts_with_scaffold(read_mol_block(open(f).read()), 0.5e-4 + 1e-6)
