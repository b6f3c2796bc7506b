"""Host side of strided sampling (MolDiff.sample(..., num_steps=, timesteps=)): the schedules, the jump tables of
q(x_s | x_t, x_0) for s < t - 1, and the synthetic inputs (with their float64 restatement) that tests/test_gpu_schedule.py checks the
jump kernels against.  There is no reference to compare with (the reference's loop visits every level): the tables are checked
against float64 restatements written here and against the identities an exact posterior of the same forward process satisfies.
No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moldiff_amd import _lib
from moldiff_amd.schedule import check_schedule, make_schedule, pairs, resolve_schedule
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
U24 = 2.0 ** -24     # unit roundoff of fp32: one rounding to nearest changes a value by at most this, relatively
IRREGULAR = [999, 700, 699, 400, 120, 119, 30, 1, 0]

# ---- inputs of the GPU "stand-alone jump posteriors" test, shared so that the exclusion cap is checked for exactly them ------------
JUMP_SIZES = [24, 19, 22, 17, 25, 21, 23, 18, 20, 26, 16, 22]   # 253 atoms, 2,596 half-edges
JUMP_PAIRS = [(999, 0), (999, 420), (640, 300), (500, 499), (37, 0), (3, 1), (1, 0), (2, 0), (0, -1), (750, 749), (999, 998), (120, 30)]
JUMP_SEED = 777
MARGIN = 1e-4        # the fp64 class test may skip rows whose two best Gumbel-plus-logit scores lie closer than this
SKIP_CAP = 0.005     # ... but no more than this share of the rows


def jump_inputs():
    """One (t, s) pair per molecule; random decoder logits, random one-hot v_t (as its log row), fixed uniforms; positions, x0_hat, eps."""
    g = U.rng(JUMP_SEED)
    bn, hei, bh, _, _ = U.graph_from_sizes(JUMP_SIZES)
    N, Eh = int(bn.numel()), int(bh.numel())
    t = torch.tensor([p[0] for p in JUMP_PAIRS], dtype=torch.int64)
    s = torch.tensor([p[1] for p in JUMP_PAIRS], dtype=torch.int64)
    log_rows = lambda n, K: torch.log(F.one_hot(torch.from_numpy(g.integers(0, K, n)), K).float().clamp(min=1e-30))
    return {'bn': bn, 'hei': hei, 'bh': bh, 't': t, 's': s,
            'logits_n': U.t32(3.0 * g.standard_normal((N, 8))), 'logits_h': U.t32(3.0 * g.standard_normal((Eh, 6))),
            'log_vt_n': log_rows(N, 8), 'log_vt_h': log_rows(Eh, 6),
            'u_n': U.t32(g.random((N, 8), dtype=np.float32)), 'u_h': U.t32(g.random((Eh, 6), dtype=np.float32)),
            'x_t': U.t32(2.0 * g.standard_normal((N, 3))), 'x0': U.t32(2.0 * g.standard_normal((N, 3))),
            'eps': U.t32(g.standard_normal((N, 3)))}


def posterior_fp64(q_mats, qT_jump, logits, log_vt, t, s, row):
    """float64 restatement of the jump posterior, per row (t, s, row: per-ROW level read, level written and table row):
    log_softmax(logits) = log v0_hat;  log(sum_j e^{log v_t[j]} Q_{t|s}[k,j] + 1e-30).clamp(-32) + log(sum_j e^{log v0_hat[j]} Qbar_s[j,k]
    + 1e-30).clamp(-32), normalised;  log v0_hat itself where t == 0.  The tables are the stored fp32 ones, widened."""
    l0 = torch.log_softmax(logits.double(), dim=-1)
    Q1 = qT_jump.double()[row]                                   # (n,K,K): Q1[j,k] = Q_{t|s}[k,j]
    Q0 = q_mats.double()[s.clamp(min=0)]
    f1 = (log_vt.double().exp().unsqueeze(-1) * Q1).sum(dim=1)
    f2 = (l0.exp().unsqueeze(-1) * Q0).sum(dim=1)
    out = torch.log(f1 + 1e-30).clamp_min(-32.0) + torch.log(f2 + 1e-30).clamp_min(-32.0)
    out = out - torch.logsumexp(out, dim=-1, keepdim=True)
    return torch.where((t == 0).unsqueeze(-1), l0, out)


def classes_fp64(log_post, u):
    """Gumbel-max over a float64 log-posterior with the uniforms u -> (class ids, margin between the two best scores)"""
    z = -torch.log(-torch.log(u.double() + 1e-30) + 1e-30) + log_post
    top = z.topk(2, dim=-1).values
    return z.argmax(-1), top[:, 0] - top[:, 1]


def pair_rows(t, s):
    """distinct (t, s) pairs and each graph's row among them, as the t_prev= keyword builds them (t == 0 pairs with -1)"""
    s = torch.where(t == 0, torch.full_like(s, -1), s)
    uniq, row = torch.unique(torch.stack([t, s], dim=1), dim=0, return_inverse=True)
    return uniq[:, 0].tolist(), uniq[:, 1].tolist(), row


# ---- schedules ----------------------------------------------------------------------------------------------------------------------

def test_uniform_schedules_have_the_right_ends_length_and_order():
    for top, m in ((999, 2), (999, 3), (999, 20), (999, 50), (999, 100), (999, 250), (999, 999), (11, 7), (1, 2), (499, 77)):
        sch = make_schedule(top, m)
        assert len(sch) == m and sch[0] == top and sch[-1] == 0
        assert all(isinstance(v, int) for v in sch) and all(b < a for a, b in zip(sch, sch[1:]))
    assert make_schedule(T - 1, T) == list(range(T - 1, -1, -1))
    assert make_schedule(9, 4) == [9, 6, 3, 0] and make_schedule(10, 4) == [10, 7, 3, 0]   # nearest multiples of top / (m - 1)
    assert pairs([9, 6, 3, 0]) == [(9, 6), (6, 3), (3, 0), (0, -1)]
    assert resolve_schedule(999) is None
    assert resolve_schedule(999, num_steps=3) == [999, 500, 0]
    assert resolve_schedule(999, timesteps=np.array(IRREGULAR)) == IRREGULAR
    assert resolve_schedule(11, timesteps=(11, 5, 0)) == [11, 5, 0]     # a partial chain from start_step = 12


def test_invalid_schedules_raise():
    for top, m in ((999, 1), (999, 0), (999, -3), (999, 1001), (5, 7), (0, 2), (999, 2.5), (999, '3'), (999.0, 3), (999, True)):
        with pytest.raises(ValueError):
            make_schedule(top, m)
    for ts in ([998, 5, 0], [999, 5, 1], [999, 5, 5, 0], [999, 5, 7, 0], [], [999, 5.0, 0], [999, 'a', 0], 7, [999, True, 0], [999, -1, 0]):
        with pytest.raises(ValueError):
            check_schedule(ts, 999)
    with pytest.raises(ValueError, match='not both'):
        resolve_schedule(999, num_steps=10, timesteps=[999, 0])
    with pytest.raises(ValueError, match='start at level 11'):
        resolve_schedule(11, timesteps=[999, 0])


# ---- jump tables --------------------------------------------------------------------------------------------------------------------

def _tables(m, sch):
    tt, ss = (list(x) for x in zip(*pairs(sch)))
    return tt, ss, m.pos_transition.jump_coefs(tt, ss), m.node_transition.jump_mats(tt, ss), m.edge_transition.jump_mats(tt, ss)


def test_full_schedule_tables_are_the_one_step_tables_bit_for_bit():
    m = U.moldiff('MolDiff_simple')
    keys = sorted(m.state_dict())
    _, _, (c0, ct, sd), qn, qe = _tables(m, make_schedule(T - 1, T))
    flip = lambda x: x.detach().flip(0)                          # table row j is level T - 1 - j
    pt = m.pos_transition
    assert torch.equal(c0, flip(pt.coef_x0)) and torch.equal(ct, flip(pt.coef_xt)) and torch.equal(sd, flip(pt.std))
    assert torch.equal(qn, flip(m.node_transition.transpopse_q_onestep_mats))
    assert torch.equal(qe, flip(m.edge_transition.transpopse_q_onestep_mats))
    assert all(x.dtype == torch.float32 and x.is_contiguous() for x in (c0, ct, sd, qn, qe))
    assert sorted(m.state_dict()) == keys                        # nothing was registered


def _one_step64(tr, l):
    b = float(tr.betas[l])
    K = tr.num_classes
    return b * np.tile(np.asarray(tr.init_prob, dtype=np.float64)[None, :], (K, 1)) + (1.0 - b) * np.eye(K)


@pytest.mark.parametrize('name', ['uniform50', 'irregular'])
def test_strided_tables_match_float64_and_preserve_the_marginals(name):
    """Q_{t|s}: the float64 product Q_{s+1} ... Q_t (left to right) of the float64 one-step matrices, rounded once -- bit-equal.  Its rows
    sum to 1 in exact arithmetic; each of the K stored entries carries one rounding of relative size 2^-24, so the float64 sum of a
    stored row is within 2^-24 * (sum of the entries) = 2^-24 (1 + 2^-24) of 1 (1e-12 is added for the float64 evaluation itself).
    Gaussian rows, evaluated in float64 from the stored fp32 (c0, ct, sd) and the float64 abar:
      c0 + ct sqrt(abar_t) = sqrt(abar_s): each stored coefficient is off by at most 2^-24 of itself, so the left side is within
          2^-24 (|c0| + |ct| sqrt(abar_t)) of the right one;
      sd^2 + ct^2 (1 - abar_t) = 1 - abar_s: squaring a value with relative error d gives relative error 2 d + d^2, so the left side is
          within (2^-23 + 2^-48) (sd^2 + ct^2 (1 - abar_t)) of the right one.
    Both hold in exact arithmetic for every s < t (q(x_s | x_0) is recovered by integrating q(x_s | x_t, x_0) over q(x_t | x_0)), with
    abar_{-1} = 1 for the last move; 1e-12 absolute is added for the float64 evaluation of the table entries and of the test.
    The identities alone leave a one-parameter family (any sd with a matching split passes them), so the three coefficients are also
    compared, bit for bit, with a float64 restatement of c0 = sqrt(abar_s)(1 - a)/(1 - abar_t), ct = sqrt(a)(1 - abar_s)/(1 - abar_t),
    sd = sqrt((1 - abar_s)(1 - a)/(1 - abar_t)), a = abar_t / abar_s, from the test's own abar, rounded once to fp32."""
    m = U.moldiff('MolDiff_simple')
    sch = make_schedule(T - 1, 50) if name == 'uniform50' else IRREGULAR
    tt, ss, (c0, ct, sd), qn, qe = _tables(m, sch)
    for tr, q in ((m.node_transition, qn), (m.edge_transition, qe)):
        for j, (t, s) in enumerate(zip(tt, ss)):
            if s == t - 1:
                assert torch.equal(q[j], tr.transpopse_q_onestep_mats[t].detach())
            else:
                prod = _one_step64(tr, s + 1)
                for l in range(s + 2, t + 1):
                    prod = prod @ _one_step64(tr, l)
                assert torch.equal(q[j], torch.from_numpy(np.ascontiguousarray(prod.T).astype(np.float32))), (t, s)
        rows = q.double().sum(dim=-2)                            # stored transposed: row k of Q_{t|s} is column k
        worst = float((rows - 1.0).abs().max())
        print(f'{name} K = {tr.num_classes}: max |row sum - 1| = {worst:.3e}')
        assert worst <= U24 * (1.0 + U24) + 1e-12
    from moldiff_amd.diffusion import get_beta_schedule
    from moldiff_amd.harness import default_config
    betas = get_beta_schedule(num_timesteps=T, **default_config('MolDiff_simple').diff.diff_pos)
    abar = np.concatenate([np.cumprod(1.0 - np.asarray(betas, dtype=np.float64)), [1.0]])     # abar[-1] = 1: the level below 0
    at, as_ = abar[np.asarray(tt)], abar[np.asarray(ss)]
    c0, ct, sd = (x.double().numpy() for x in (c0, ct, sd))
    # the identities are two equations for three values: pin all three by an independent float64 restatement from abar, rounded once
    far = np.asarray(ss) < np.asarray(tt) - 1
    a64 = at / as_
    want = [np.sqrt(as_) * (1.0 - a64) / (1.0 - at), np.sqrt(a64) * (1.0 - as_) / (1.0 - at), np.sqrt((1.0 - as_) * (1.0 - a64) / (1.0 - at))]
    for got, w, one_step in zip((c0, ct, sd), want, (m.pos_transition.coef_x0, m.pos_transition.coef_xt, m.pos_transition.std)):
        assert np.array_equal(got[far], w[far].astype(np.float32).astype(np.float64))
        assert np.array_equal(got[~far], one_step.detach().double().numpy()[np.asarray(tt)[~far]])     # stride 1: the copied rows
    e1 = np.abs(c0 + ct * np.sqrt(at) - np.sqrt(as_))
    b1 = U24 * (np.abs(c0) + np.abs(ct) * np.sqrt(at)) + 1e-12
    e2 = np.abs(sd ** 2 + ct ** 2 * (1.0 - at) - (1.0 - as_))
    b2 = (2 * U24 + U24 ** 2) * (sd ** 2 + ct ** 2 * (1.0 - at)) + 1e-12
    print(f'{name}: mean identity error / bound max {float((e1 / b1).max()):.3f}, variance identity {float((e2 / b2).max()):.3f}')
    assert (e1 <= b1).all() and (e2 <= b2).all()
    assert any(s < t - 1 for t, s in zip(tt, ss)) and any(s == t - 1 and t > 0 for t, s in zip(tt, ss)) == (name == 'irregular')


def test_jump_tables_refuse_pairs_that_are_not_a_downward_move():
    m = U.moldiff('MolDiff_simple')
    for t, s in (([5], [5]), ([5], [6]), ([1000], [3]), ([5], [-1]), ([0], [-2]), ([-1], [-2]), ([5, 4], [3])):
        with pytest.raises(ValueError):
            m.pos_transition.jump_coefs(t, s)
        with pytest.raises(ValueError):
            m.node_transition.jump_mats(t, s)


def test_fp64_class_test_of_the_jump_posterior_skips_at_most_half_a_percent_of_its_rows():
    """The condition is on the inputs: with these logits, one-hot rows, uniforms and (t, s) pairs the float64 Gumbel-max decides all
    but <= 0.5 % of the rows by more than 1e-4.  (An fp32 evaluation of the posterior is off by a few 1e-6: logf / expf of a few ulp on
    terms of size <= 32 each, i.e. <= 64 * 2^-23 = 8e-6, the Gumbel transform likewise -- far inside the margin.)"""
    m = U.moldiff('MolDiff_simple')
    inp = jump_inputs()
    tt, ss, row = pair_rows(inp['t'], inp['s'])
    assert (0 in ss) and any(s == t - 1 and t > 0 for t, s in zip(tt, ss)) and any(s < t - 1 for t, s in zip(tt, ss))
    for tr, batch, lg, lvt, u in ((m.node_transition, inp['bn'], inp['logits_n'], inp['log_vt_n'], inp['u_n']),
                                  (m.edge_transition, inp['bh'], inp['logits_h'], inp['log_vt_h'], inp['u_h'])):
        post = posterior_fp64(tr.q_mats.detach(), tr.jump_mats(tt, ss), lg, lvt, inp['t'][batch], inp['s'][batch], row[batch])
        assert torch.isfinite(post).all() and float((post.exp().sum(-1) - 1.0).abs().max()) < 1e-12
        _, margin = classes_fp64(post, u)
        for g, (t, s) in enumerate(JUMP_PAIRS):
            mg = margin[batch == g]
            print(f'K = {tr.num_classes}, pair ({t}, {s}): {int(mg.numel())} rows, share within {MARGIN} of a tie = '
                  f'{float((mg < MARGIN).double().mean()):.2e}')
        share = float((margin < MARGIN).double().mean())
        print(f'K = {tr.num_classes}: {int(margin.numel())} rows, share within {MARGIN} of a tie = {share:.2e}')
        assert margin.numel() > 200 and share <= SKIP_CAP


def test_stride_one_posterior_restatement_is_the_one_step_formula():
    """the float64 restatement with a stride-1 table row equals the module's own torch statement of q(v_{t-1} | v_t, v_0) in float64"""
    m = U.moldiff('MolDiff_simple')
    tr = m.node_transition
    inp = jump_inputs()
    t = torch.tensor([500] * len(JUMP_SIZES))
    s = t - 1
    tt, ss, row = pair_rows(t, s)
    l0 = torch.log_softmax(inp['logits_n'].double(), dim=-1)
    bn = inp['bn']
    with torch.no_grad():                                        # float64 inputs promote the fp32 tables: a float64 evaluation
        want = tr.q_v_posterior_autograd(l0, inp['log_vt_n'].double(), t, bn)
    got = posterior_fp64(tr.q_mats.detach(), tr.jump_mats(tt, ss), inp['logits_n'], inp['log_vt_n'], t[bn], s[bn], row[bn])
    assert want.dtype == torch.float64 and float((want - got).abs().max()) < 1e-12


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------

def test_jump_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'moldiff_hip.h')).read()
    declared = set(re.findall(r'\b(mdx_[a-z_0-9]+)\s*\(', hdr))
    L = _lib.lib()
    for name in ('mdx_sample_jump_full', 'mdx_pos_posterior_jump', 'mdx_cat_posterior_jump'):
        assert name in declared and name in _lib.EXPORTS and getattr(L, name).argtypes is not None
    assert len(L.mdx_sample_jump_full.argtypes) == len(L.mdx_sample_step_full.argtypes) + 2
    # argument checks that need no device: null handles, a class count outside 2..8
    assert L.mdx_sample_jump_full(*([None] * 4), 0, 0, *([None] * 13), 0, None) == 1
    assert L.mdx_cat_posterior_jump(None, None, 9, None, 0, None, None, None, None, None, 4, None, None) != 0
