"""GPU tests of strided sampling (MolDiff.sample(..., num_steps=, timesteps=), mdx_sample_jump_full and the stand-alone jump posteriors).

There is no reference to compare with (the reference's loop visits every level).  What is pinned: a schedule that visits every level is
the existing chain bit for bit; a stride-1 move inside a strided schedule is the full chain's step at that level (noise is keyed by the
level); the jump posteriors follow their float64 restatement (tests/test_schedule_host.py); the one-call jump step is the composition
of the stand-alone kernels; chains at reduced step counts are finite, decodable, shard-invariant and compose with scaffolds and
partial chains.  What a reduced step count does to sample QUALITY is not tested: no trained checkpoint is available.
"""
import glob
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moldiff_amd import Scaffold, _lib
from moldiff_amd.postprocess import FeaturizeMol
from moldiff_amd.schedule import make_schedule, pairs
from tests import test_schedule_host as H
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = 1000
SIZES8 = [9, 14, 11, 7, 16, 12, 10, 13]


@pytest.fixture(scope='module', autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f'\n[test_gpu_schedule] wall time of this file: {time.time() - t0:.1f} s')


def _model():
    return U.moldiff('MolDiff_simple', DEV)


def _random_scaffold(sizes, seed, frac=0.5, all_rows=None):
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
              t=sm.t.clone(), **{f'pred{j}': p.clone() for j, p in enumerate(sm.preds)})
    return st


def _onehot_state(g, N, Eh):
    hn = F.one_hot(torch.from_numpy(g.integers(0, 8, N)), 8).float().to(DEV)
    hh = F.one_hot(torch.from_numpy(g.integers(0, 6, Eh)), 6).float().to(DEV)
    pos = U.t32(g.standard_normal((N, 3))).to(DEV)
    return hn, pos, hh, torch.log(hn.clamp(min=1e-30)), torch.log(hh.clamp(min=1e-30))


# ---- a schedule that visits every level is the existing chain ---------------------------------------------------------------------

@U.both_paths
@pytest.mark.parametrize('variant', ['plain', 'uncertainty', 'scaffold'])
def test_a_stride_of_one_is_the_existing_chain_bit_for_bit(variant):
    m = _model()
    (bn, hei, bh), sc = _random_scaffold(SIZES8, 1)
    extra = {'plain': {}, 'uncertainty': dict(bond_predictor=U.bondpred(DEV), guidance=['uncertainty', 1e-4]), 'scaffold': dict(scaffold=sc)}[variant]
    runs = []
    for kw in ({}, dict(num_steps=T), dict(timesteps=list(range(T - 1, -1, -1)))):
        sm = m.sampler(len(SIZES8), bn, hei, bh, seed=17, **extra, **kw)
        assert (sm.jump is None) == (not kw)
        sm.init()
        for i in range(30):
            sm.step(i)
        runs.append(_snapshot(sm, 31))
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert torch.equal(v, other[k]), k
    assert torch.isfinite(runs[0]['pos']).all()


def test_a_stride_one_move_inside_a_strided_schedule_is_the_full_chains_step_at_that_level():
    """Noise is keyed by the level left (draw T - t), not by the iteration count: teacher-forced to the same state, the move 500 -> 499 as
    iteration 1 of the schedule [999, 500, 499, 200, 0] equals loop iteration 499 of the full chain in every bit."""
    m = _model()
    bn, hei, bh, _, _ = U.graph_from_sizes(SIZES8, DEV)
    N, Eh = int(bn.numel()), int(bh.numel())
    state = _onehot_state(U.rng(3), N, Eh)
    got = []
    for kw, it in ((dict(timesteps=[999, 500, 499, 200, 0]), 1), ({}, 499)):
        sm = m.sampler(len(SIZES8), bn, hei, bh, seed=23, **kw)
        sm.set_state(*state, frame=it)
        sm.step(it)
        got.append(dict(_snapshot(sm, 0), ids_n=sm.node_ids[sm.pcur].clone(), ids_h=sm.half_ids[sm.pcur].clone(),
                        eps=sm.eps.clone(), u_n=sm.u_n.clone(), u_h=sm.u_h.clone()))
    assert bool((got[0]['t'][:len(SIZES8)] == 500).all())
    for k, v in got[0].items():
        assert torch.equal(v, got[1][k]), k


# ---- the stand-alone jump posteriors against float64 ---------------------------------------------------------------------------------

def test_standalone_jump_posteriors_follow_the_float64_restatement():
    """Inputs of tests/test_schedule_host.py (one (t, s) pair per molecule, s = 0, stride-1 pairs and t = 0 among them), through the
    keyword-only t_prev= of the two transition classes.
    Positions against float64 from the stored fp32 coefficients: a = c0 x0, b = ct x_t, c = sd eps; the kernel rounds a, b, a + b, c and
    (a + b) + c once each (no contraction), so |err| <= 2^-24 (|a| + |b| + |a + b| + |c| + |a + b + c|) <= 3 * 2^-24 (|a| + |b| + |c|) to
    first order; the second-order terms are covered by the factor (1 + 2^-20).
    Classes: Gumbel-max of the device log-posterior (fp32 log-softmax of the logits as its v0 input) bit-equal to the float64
    Gumbel-argmax outside the 1e-4 margin; the skipped share <= 0.5 %, as the host test established for these inputs."""
    m = _model()
    inp = H.jump_inputs()
    d = {k: v.to(DEV) for k, v in inp.items()}
    tt, ss, row = H.pair_rows(inp['t'], inp['s'])
    pt = m.pos_transition
    got = pt.get_prev_from_recon(d['x_t'], d['x0'], d['t'], d['bn'], eps=d['eps'], t_prev=d['s']).cpu().double()
    c0, ct, sd = (x.cpu().double()[row][inp['bn']].unsqueeze(-1) for x in pt.jump_coefs(tt, ss))
    a, b, c = c0 * inp['x0'].double(), ct * inp['x_t'].double(), sd * inp['eps'].double()
    last = (inp['t'][inp['bn']] == 0).unsqueeze(-1)
    want = torch.where(last, a + b, a + b + c)
    bound = 3 * 2.0 ** -24 * (a.abs() + b.abs() + c.abs()) * (1 + 2.0 ** -20)
    err = (got - want).abs()
    print(f'positions: max error / bound = {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all())
    # without the keyword nothing changes: stride-1 pairs through the keyword equal the one-step call bit for bit
    t1 = torch.tensor([500, 1, 999, 0, 37, 2, 750, 3, 640, 120, 5, 64], device=DEV)
    one = pt.get_prev_from_recon(d['x_t'], d['x0'], t1, d['bn'], eps=d['eps'])
    assert torch.equal(one, pt.get_prev_from_recon(d['x_t'], d['x0'], t1, d['bn'], eps=d['eps'], t_prev=t1 - 1))
    skipped = total = 0
    for tr, batch, lg, lvt, u in ((m.node_transition, 'bn', 'logits_n', 'log_vt_n', 'u_n'), (m.edge_transition, 'bh', 'logits_h', 'log_vt_h', 'u_h')):
        log_v0 = F.log_softmax(d[lg], dim=-1)
        post = tr.q_v_posterior(log_v0, d[lvt], d['t'], d[batch], v0_prob=True, t_prev=d['s'])
        cls = _lib.gumbel_argmax(post, d[u]).cpu()
        rb = inp[batch]
        p64 = H.posterior_fp64(tr.q_mats.detach().cpu(), tr.jump_mats(tt, ss).cpu(), inp[lg], inp[lvt], inp['t'][rb], inp['s'][rb], row[rb])
        c64, margin = H.classes_fp64(p64, inp[u])
        sure = margin >= H.MARGIN
        print(f'K = {tr.num_classes}: max |log posterior - fp64| = {float((post.cpu().double() - p64).abs().max()):.3e}, '
              f'skipped {int((~sure).sum())} of {int(sure.numel())} rows')
        assert torch.equal(cls[sure], c64[sure])
        skipped += int((~sure).sum()); total += int(sure.numel())
        one = tr.q_v_posterior(log_v0, d[lvt], t1, d[batch], v0_prob=True)
        assert torch.equal(one, tr.q_v_posterior(log_v0, d[lvt], t1, d[batch], v0_prob=True, t_prev=t1 - 1))
    assert skipped <= H.SKIP_CAP * total


# ---- the one-call jump step is the composition of the stand-alone kernels ---------------------------------------------------------------

@U.both_paths
def test_fused_jump_step_equals_the_composed_standalone_kernels():
    """Teacher-forced iterations of the schedule [999, 300, 120, 0]: T-1 -> far below, a mid-chain jump, a jump onto level 0 and the final
    t == 0 iteration.  The state the call wrote is bit-equal to the stand-alone jump posteriors (is_logits form: the log-softmax is the
    kernel's own) plus gumbel_argmax applied to that call's own predictions and noise; the time tensor holds tau_j."""
    m = _model()
    sch = [999, 300, 120, 0]
    bn, hei, bh, _, _ = U.graph_from_sizes(SIZES8, DEV)
    N, Eh, B = int(bn.numel()), int(bh.numel()), len(SIZES8)
    tt, ss = (list(x) for x in zip(*pairs(sch)))
    pt, ntr, etr = m.pos_transition, m.node_transition, m.edge_transition
    c0, ct, sd = pt.jump_coefs(tt, ss)
    for j, (t, s) in enumerate(zip(tt, ss)):
        sm = m.sampler(B, bn, hei, bh, seed=31, timesteps=sch)
        hn, pos, hh, ln, lh = _onehot_state(U.rng(40 + j), N, Eh)
        sm.set_state(hn, pos, hh, ln, lh, frame=j)
        sm.step(j)
        st = sm.state()
        tv = torch.full((B,), t, dtype=torch.int64, device=DEV)
        sv, rv = torch.full_like(tv, s), torch.full_like(tv, j)
        assert torch.equal(sm.t[:B], tv)
        assert torch.equal(st['pos'], _lib.pos_posterior_jump(c0, ct, sd, pos, sm.preds[1], sm.eps, tv, rv, bn))
        for tr, batch, pred, lvt, u, oh, lg, ids in ((ntr, bn, sm.preds[0], ln, sm.u_n, st['h_node'], st['log_node'], sm.node_ids[sm.pcur]),
                                                     (etr, bh, sm.preds[2], lh, sm.u_h, st['h_halfedge'], st['log_halfedge'], sm.half_ids[sm.pcur])):
            post = _lib.cat_posterior_jump(tr.q_mats, tr.jump_mats(tt, ss), pred, lvt, tv, sv, rv, batch, is_logits=True)
            cls, onehot = _lib.gumbel_argmax(post, u, want_onehot=True)
            assert torch.equal(lg, post) and torch.equal(oh, onehot) and torch.equal(ids.long(), cls)
        if t == 0:   # the existing t == 0 branch: log x0_hat and the posterior mean (torch's own fp32 evaluation: a few ulp apart)
            assert float((st['log_node'] - F.log_softmax(sm.preds[0], -1)).abs().max()) < 1e-5
            mean = pt.coef_x0[0] * sm.preds[1] + pt.coef_xt[0] * pos
            assert float((st['pos'] - mean).abs().max()) <= 2.0 ** -22 * float(mean.abs().max())


# ---- whole chains at reduced step counts ----------------------------------------------------------------------------------------------

def test_whole_chains_at_20_and_50_steps_are_finite_decodable_and_shard_invariant():
    m = _model()
    sizes = [9, 14, 11, 7, 16, 12]
    ids = np.arange(300, 306)
    feat = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    n_lo, e_lo = sum(sizes[:3]), sum(s * (s - 1) // 2 for s in sizes[:3])

    def run(sz, mol_ids, steps):
        bn, hei, bh, _, _ = U.graph_from_sizes(sz, DEV)
        out = m.sample(len(sz), bn, hei, bh, seed=5, mol_ids=mol_ids, num_steps=steps)
        return out, (bn, hei, bh)

    for steps in (20, 50):
        full, (bn, hei, bh) = run(sizes, ids, steps)
        assert [x.shape[0] for x in full['traj']] == [steps + 1] * 3
        assert all(bool(torch.isfinite(p).all()) for p in full['pred']) and bool(torch.isfinite(full['traj'][1]).all())
        mols = feat.decode_batch(full['pred'], bn, hei, bh, len(sizes))
        assert len(mols) == len(sizes) and all(np.isfinite(info['atom_pos']).all() for info in mols)
        lo, _ = run(sizes[:3], ids[:3], steps)
        hi, _ = run(sizes[3:], ids[3:], steps)
        for k, cut in ((0, n_lo), (1, n_lo), (2, e_lo)):
            assert torch.equal(full['pred'][k][:cut], lo['pred'][k]) and torch.equal(full['pred'][k][cut:], hi['pred'][k])
            dense = lambda x: x.dense() if hasattr(x, 'dense') else x
            assert torch.equal(dense(full['traj'][k][-1])[:cut], dense(lo['traj'][k][-1]))
            assert torch.equal(dense(full['traj'][k][-1])[cut:], dense(hi['traj'][k][-1]))
        short = m.sample(len(sizes), bn, hei, bh, seed=5, mol_ids=ids, num_steps=steps, return_traj=False)
        assert short['traj'][1].shape[0] == 1 and all(torch.equal(a, b) for a, b in zip(short['pred'], full['pred']))


# ---- composition with scaffolds and partial chains ------------------------------------------------------------------------------------------

def test_scaffold_and_schedule_compose():
    m = _model()
    sizes = [9, 14, 11, 7, 16, 12]
    (bn, hei, bh), sc = _random_scaffold(sizes, 2)
    N, Eh = int(bn.numel()), int(bh.numel())
    nm, nt, x0, ht, hm = sc.resolve(N, hei, 8, 6)
    steps = 20
    sch = make_schedule(T - 1, steps)
    asked = []

    def noise(draw):   # fresh values per draw index
        asked.append(draw)
        gd = U.rng(1000 + draw)
        return (U.t32(gd.standard_normal((N, 3))).to(DEV), U.t32(gd.random((N, 8), dtype=np.float32)).to(DEV),
                U.t32(gd.random((Eh, 6), dtype=np.float32)).to(DEV))

    out = m.sample(len(sizes), bn, hei, bh, noise=noise, scaffold=sc, num_steps=steps)
    # prior, its merge; then per iteration the move leaving level t (T - t) and, but for the last, the merge after it (T + (T - t))
    want = [0, 2 * T + 1]
    for j, t in enumerate(sch):
        want += [T - t] + ([T + (T - t)] if j + 1 < len(sch) else [])
    assert asked == want
    assert out['traj'][1].shape[0] == steps + 1
    assert torch.equal(out['traj'][1][-1][nm], x0[nm]) and torch.equal(out['pred'][1][nm], x0[nm])
    assert torch.equal(out['traj'][0][-1].dense()[nm], F.one_hot(nt[nm], 8).float())
    assert torch.equal(out['traj'][2][-1].dense()[hm], F.one_hot(ht[hm], 6).float())
    assert bool(torch.isfinite(out['pred'][1]).all()) and not torch.equal(out['pred'][1][~nm], x0[~nm])
    # one jump iteration with and without the scaffold: free rows are untouched by the merge, fixed rows were replaced
    state = _onehot_state(U.rng(3), N, Eh)
    got = []
    for kw in ({}, dict(scaffold=sc)):
        sm = m.sampler(len(sizes), bn, hei, bh, noise=noise, num_steps=steps, **kw)
        sm.set_state(*state, frame=7)
        asked.clear()
        sm.step(7)
        got.append(dict(_snapshot(sm, 0), ids_n=sm.node_ids[sm.pcur].clone(), ids_h=sm.half_ids[sm.pcur].clone()))
    assert asked == [T - sch[7], T + (T - sch[7])]
    plain, cond = got
    for k, mask in (('h_node', nm), ('pos', nm), ('log_node', nm), ('ids_n', nm), ('h_halfedge', hm), ('log_halfedge', hm), ('ids_h', hm)):
        assert torch.equal(plain[k][~mask], cond[k][~mask]), k
    assert not torch.equal(plain['pos'][nm], cond['pos'][nm])
    # the merged rows are q(x_s | x_0) at the level the jump landed on: classes bit-equal to the training-side add_noise there
    s = sch[8]
    un, uh = noise(T + (T - sch[7]))[1:]
    tt = torch.full((len(sizes),), s, dtype=torch.int64, device=DEV)
    assert torch.equal(cond['h_node'][nm], m.node_transition.add_noise(nt, tt, bn, un)[0][nm])
    assert torch.equal(cond['h_halfedge'][hm], m.edge_transition.add_noise(ht, tt, bh, uh)[0][hm])


def test_start_step_and_num_steps_span_the_right_levels():
    m = _model()
    sizes = [9, 14, 11, 7]
    s0, steps = 200, 10
    (bn, hei, bh), sc = _random_scaffold(sizes, 9, all_rows=True)
    sm = m.sampler(len(sizes), bn, hei, bh, seed=4, scaffold=sc, start_step=s0, num_steps=steps)
    assert sm.sched == make_schedule(s0 - 1, steps) and sm.sched[0] == s0 - 1 and sm.sched[-1] == 0
    sm.init()
    seen = []
    for j in range(steps):
        sm.step(j)
        seen.append(int(sm.t[0]))
    assert seen == sm.sched
    with pytest.raises(IndexError):
        sm.step(steps)
    out = m.sample(len(sizes), bn, hei, bh, seed=4, scaffold=sc, start_step=s0, num_steps=steps)
    assert [t.shape[0] for t in out['traj']] == [steps + 1] * 3
    assert torch.equal(out['traj'][1][-1], sc.node_pos) and torch.equal(out['pred'][1], sc.node_pos)     # all-true mask: ends on the molecule
    assert torch.equal(out['traj'][0][-1].dense(), F.one_hot(sc.node_type, 8).float())
    free = Scaffold(torch.zeros_like(sc.node_mask), sc.node_type, sc.node_pos, sc.halfedge_type)
    out = m.sample(len(sizes), bn, hei, bh, seed=4, scaffold=free, start_step=s0, timesteps=[199, 60, 59, 0])
    assert out['traj'][1].shape[0] == 5 and bool(torch.isfinite(out['traj'][1]).all()) and not torch.equal(out['traj'][1][-1], sc.node_pos)
    for kw in (dict(num_steps=s0 + 1), dict(timesteps=[T - 1, 0]), dict(num_steps=5, timesteps=[199, 0])):
        with pytest.raises(ValueError):
            m.sampler(len(sizes), bn, hei, bh, scaffold=sc, start_step=s0, **kw)
    with pytest.raises(ValueError):
        m.sampler(len(sizes), bn, hei, bh, num_steps=1)


def test_continuous_space_refuses_the_keywords():
    import copy
    import moldiff_amd as M
    from moldiff_amd.harness import default_config
    cfg = copy.deepcopy(default_config('MolDiff_simple'))
    cfg.diff.categorical_space = 'continuous'
    cfg.diff.scaling = [1., 4., 8.]
    mc = M.MolDiff(cfg, 8, 6).eval().to(DEV)
    bn, hei, bh, _, _ = U.graph_from_sizes([5, 6], DEV)
    with pytest.raises(NotImplementedError):
        mc.sampler(2, bn, hei, bh, num_steps=20)
    with pytest.raises(NotImplementedError):
        mc.sample(2, bn, hei, bh, timesteps=[T - 1, 0])


def test_cli_num_steps_runs_end_to_end(tmp_path):
    import os
    import yaml
    from moldiff_amd import sample_drug3d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, 'configs', 'sample_MolDiff_simple.yml')))
    cfg['sample'].update(num_mols=2, batch_size=4, save_traj_prob=1)
    cp = tmp_path / 'sample.yml'
    cp.write_text(yaml.safe_dump(cfg))
    log_dir = sample_drug3d.main(['--config', str(cp), '--outdir', str(tmp_path / 'out'), '--device', DEV, '--recipe-weights',
                                  '--num_steps', '20'])
    pool = torch.load(str(log_dir) + '/samples_all.pt', weights_only=False)
    assert len(pool['finished']) + len(pool['failed']) >= 4
    files = glob.glob(str(log_dir) + '_SDF/traj_mol*.sdf')
    assert len(files) >= len(pool['finished']) and (files or not pool['finished'])
    for f in files:
        txt = open(f).read()
        assert txt.count('$$$$') == 21 and txt.count('M  END') == 21
    # the config key does the same, and the flag wins over it
    cfg['sample']['num_steps'] = 30
    cp.write_text(yaml.safe_dump(cfg))
    for argv, frames in (([], 31), (['--num_steps', '20'], 21)):
        log_dir = sample_drug3d.main(['--config', str(cp), '--outdir', str(tmp_path / f'out{frames}'), '--device', DEV, '--recipe-weights'] + argv)
        for f in glob.glob(str(log_dir) + '_SDF/traj_mol*.sdf'):
            assert open(f).read().count('$$$$') == frames


def test_other_class_counts_take_the_standalone_jump_launches():
    """7 atom / 5 bond classes: the one-call step composes the stand-alone kernels (no fused transition launch for these counts).  A
    stride of 1 is the existing chain bit for bit, and a jump iteration equals the stand-alone jump posteriors plus gumbel_argmax."""
    import copy
    import moldiff_amd as M
    from moldiff_amd.harness import default_config
    mk = M.MolDiff(copy.deepcopy(default_config('MolDiff_simple')), 7, 5).eval()
    mk.load_state_dict(M.recipe_state_dict(mk, 99), strict=True)
    mk = mk.to(DEV)
    sizes = [6, 9, 7]
    bn, hei, bh, _, _ = U.graph_from_sizes(sizes, DEV)
    N, Eh, B = int(bn.numel()), int(bh.numel()), len(sizes)
    runs = []
    for kw in ({}, dict(num_steps=T)):
        sm = mk.sampler(B, bn, hei, bh, seed=3, **kw)
        sm.init()
        for i in range(10):
            sm.step(i)
        runs.append(_snapshot(sm, 11))
    for k, v in runs[0].items():
        assert torch.equal(v, runs[1][k]), k
    sch = [999, 400, 0]
    tt, ss = (list(x) for x in zip(*pairs(sch)))
    g = U.rng(8)
    hn = F.one_hot(torch.from_numpy(g.integers(0, 7, N)), 7).float().to(DEV)
    hh = F.one_hot(torch.from_numpy(g.integers(0, 5, Eh)), 5).float().to(DEV)
    pos = U.t32(g.standard_normal((N, 3))).to(DEV)
    ln, lh = torch.log(hn.clamp(min=1e-30)), torch.log(hh.clamp(min=1e-30))
    sm = mk.sampler(B, bn, hei, bh, seed=3, timesteps=sch)
    sm.set_state(hn, pos, hh, ln, lh, frame=1)
    sm.step(1)
    st = sm.state()
    tv = torch.full((B,), 400, dtype=torch.int64, device=DEV)
    sv, rv = torch.zeros_like(tv), torch.ones_like(tv)
    c0, ct, sd = mk.pos_transition.jump_coefs(tt, ss)
    assert torch.equal(st['pos'], _lib.pos_posterior_jump(c0, ct, sd, pos, sm.preds[1], sm.eps, tv, rv, bn))
    for tr, batch, pred, lvt, u, oh, lg in ((mk.node_transition, bn, sm.preds[0], ln, sm.u_n, st['h_node'], st['log_node']),
                                            (mk.edge_transition, bh, sm.preds[2], lh, sm.u_h, st['h_halfedge'], st['log_halfedge'])):
        post = _lib.cat_posterior_jump(tr.q_mats, tr.jump_mats(tt, ss), pred, lvt, tv, sv, rv, batch, is_logits=True)
        assert torch.equal(lg, post) and torch.equal(oh, _lib.gumbel_argmax(post, u, want_onehot=True)[1])
