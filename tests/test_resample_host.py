"""Host side of RePaint-style resampling (MolDiff.sample(..., resample=, jump_length=)): the path over schedule positions, the noise
windows, the forward tables of q(x_t | x_s), and the synthetic inputs (with their float64 restatement) that
tests/test_gpu_resample.py checks the forward-jump kernel against.  There is no reference to compare with (the reference's chain only
walks down): the tables are checked against the identities the forward process satisfies.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from moldiff_amd import _lib
from moldiff_amd.schedule import (check_draw_range, draw_index, make_schedule, path_draws, path_windows, resampling_path, resolve_path,
                                  window_width)
from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 1000
U24 = 2.0 ** -24     # unit roundoff of fp32

# ---- inputs of the GPU "kernel against the formula" test, shared so that the tie share is established for exactly them ----------------
FORWARD_SIZES = [2, 5, 9, 3]                                     # 19 atoms, 50 half-edges
FORWARD_PAIRS = [(499, 500), (120, 640), (0, 999), (998, 999), (0, 1)]   # (s, t): stride 1, far pairs, t = T - 1, the bottom of the chain
FORWARD_SEED = 20240
MARGIN = 1e-4        # the project's fp64 margin: a row whose two best Gumbel-plus-logit scores lie closer may be decided either way


def forward_inputs():
    """Per (s, t) pair: the class ids and positions of a state at level s and explicit noise for the move up to level t."""
    g = U.rng(FORWARD_SEED)
    bn, hei, bh, _, _ = U.graph_from_sizes(FORWARD_SIZES)
    N, Eh = int(bn.numel()), int(bh.numel())
    inp = {'bn': bn, 'hei': hei, 'bh': bh, 'pairs': {}}
    for pair in FORWARD_PAIRS:
        inp['pairs'][pair] = {'ids_n': torch.from_numpy(g.integers(0, 8, N)), 'ids_h': torch.from_numpy(g.integers(0, 6, Eh)),
                              'pos': U.t32(2.0 * g.standard_normal((N, 3))), 'eps': U.t32(g.standard_normal((N, 3))),
                              'u_n': U.t32(g.random((N, 8), dtype=np.float32)), 'u_h': U.t32(g.random((Eh, 6), dtype=np.float32))}
    return inp


def classes_fp64(qT_jump, ids, u):
    """float64 restatement of the class half of a forward jump: Gumbel-max over log(Q_{t|s}[x_s, k] + 1e-30).clamp_min(-32) with the
    uniforms u.  qT_jump: the stored fp32 (K,K) table Q_{t|s}^T, widened.  -> (class ids, margin between the two best scores)"""
    Q = qT_jump.double().T                                       # Q[x_s, k] = q(x_t = k | x_s)
    logits = torch.log(Q[ids] + 1e-30).clamp_min(-32.0)
    z = -torch.log(-torch.log(u.double() + 1e-30) + 1e-30) + logits
    top = z.topk(2, dim=-1).values
    return z.argmax(-1), top[:, 0] - top[:, 1]


def positions_fp64(c_a, c_s, pos, eps):
    """float64 restatement of the position half from the stored fp32 coefficients -> (x_t, |c_a x| + |c_s eps|)"""
    a, b = float(c_a) * pos.double(), float(c_s) * eps.double()
    return a + b, a.abs() + b.abs()


def test_no_row_of_the_forward_inputs_is_within_the_margin_of_a_tie():
    """The seed is chosen so that the float64 Gumbel-max decides EVERY row of these inputs by more than 1e-4: the GPU test then
    compares every row and skips nothing.  (An fp32 evaluation of the scores is off by a few 1e-6, see tests/test_schedule_host.py.)"""
    m = U.moldiff('MolDiff_simple')
    inp = forward_inputs()
    assert int(inp['bn'].numel()) == 19 and int(inp['bh'].numel()) == 50
    for (s, t), d in inp['pairs'].items():
        mn = classes_fp64(m.node_transition.jump_mats([t], [s])[0], d['ids_n'], d['u_n'])[1]
        mh = classes_fp64(m.edge_transition.jump_mats([t], [s])[0], d['ids_h'], d['u_h'])[1]
        margins = torch.cat([mn, mh])
        share = float((margins < MARGIN).double().mean())
        print(f'pair ({s} -> {t}): {int(margins.numel())} rows, smallest margin {float(margins.min()):.3e}, share within {MARGIN} = {share}')
        assert margins.numel() == 69 and share == 0.0


# ---- the path -----------------------------------------------------------------------------------------------------------------------

def _d(*ps):
    return [('down', p) for p in ps]


def test_path_of_seven_positions_in_blocks_of_three_walked_twice():
    want = _d(0, 1, 2) + [('up', 3, 0)] + _d(0, 1, 2) + _d(3, 4, 5) + [('up', 6, 3)] + _d(3, 4, 5) + _d(6)
    assert resampling_path(7, 3, 2) == want
    assert path_windows(want) == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0]


def test_short_last_block_plain_schedule_and_counts():
    # m = 6, jump_length = 4: blocks [0, 4] and the short [4, 5]
    assert resampling_path(6, 4, 2) == _d(0, 1, 2, 3) + [('up', 4, 0)] + _d(0, 1, 2, 3) + _d(4) + [('up', 5, 4)] + _d(4) + _d(5)
    for m in (2, 6, 7, 100):
        for J in {1, min(2, m - 1), m - 1}:
            assert resampling_path(m, J, 1) == _d(*range(m))      # resample = 1: the m down-moves of today
    for m, J, R in ((7, 3, 2), (6, 4, 2), (2, 1, 5), (100, 10, 10), (101, 10, 3), (12, 11, 4), (9, 1, 3)):
        path = resampling_path(m, J, R)
        downs, ups = [mv for mv in path if mv[0] == 'down'], [mv for mv in path if mv[0] == 'up']
        assert len(downs) == R * (m - 1) + 1                      # denoiser evaluations
        assert len(ups) == (R - 1) * -(-(m - 1) // J)             # up-moves: (R - 1) ceil((m - 1) / J)
        assert path[-1] == ('down', m - 1) and path.count(('down', m - 1)) == 1
        # the walk is continuous: every move starts where the one before it ended
        at = 0
        for mv in path:
            if mv[0] == 'down':
                assert mv[1] == at
                at += 1
            else:
                assert mv[1] == at and mv[2] < mv[1] and mv[1] - mv[2] <= J
                at = mv[2]
        assert at == m
        w = path_windows(path)
        assert max(w) == R - 1 and w[-1] == 0
        assert all(wk >= 1 for wk, mv in zip(w, path) if mv[0] == 'up')


def test_invalid_paths_raise():
    for m, J, R in ((7, 3, 0), (7, 3, -1), (7, 0, 2), (7, 7, 2), (7, -2, 2), (1, 1, 2), (7, 3, True), (7, True, 2), (7, 2.0, 2), (7, 3, '2'),
                    (7.0, 3, 2)):
        with pytest.raises(ValueError):
            resampling_path(m, J, R)
    assert resolve_path(7) is None and resolve_path(7, None, None) is None
    assert resolve_path(7, 3, 2) == resampling_path(7, 3, 2) and resolve_path(7, 3, 1) == _d(*range(7))
    for kw in (dict(jump_length=3), dict(resample=2), dict(resample=1)):
        with pytest.raises(ValueError, match='both or neither'):
            resolve_path(7, **kw)


# ---- the noise windows ---------------------------------------------------------------------------------------------------------------

def test_draw_indices_follow_the_window_layout_and_window_zero_is_todays():
    W = window_width(T)
    assert W == 3 * T + 2
    # window 0: what the plain / strided / scaffold chains use (model.py: 0, T - t, T + (T - t), 2T + 1)
    assert draw_index(T, 'prior') == 0 and draw_index(T, 'init_merge') == 2 * T + 1
    for t in (0, 1, 500, T - 1):
        assert draw_index(T, 'down', t) == T - t and draw_index(T, 'merge', t) == T + (T - t)
        assert draw_index(T, 'up', t) == 2 * T + 2 + t
        for k in (1, 2, 9):
            for kind in ('down', 'merge', 'up'):
                assert draw_index(T, kind, t, k) == draw_index(T, kind, t) + k * W
    # the layout is collision-free: every (kind, level) of a window has an index of its own inside [0, W)
    used = [0, 2 * T + 1] + [draw_index(T, kind, t) for kind in ('down', 'merge', 'up') for t in range(T)]
    assert len(set(used)) == len(used) and min(used) == 0 and max(used) == W - 1
    with pytest.raises(ValueError):
        draw_index(T, 'up', T)
    # the whole sequence of a path: resample = 1 is the sequence the chain asks for today (tests/test_gpu_schedule.py states it)
    sch = make_schedule(T - 1, 20)
    want = [0, 2 * T + 1]
    for j, t in enumerate(sch):
        want += [T - t] + ([T + (T - t)] if j + 1 < len(sch) else [])
    assert path_draws(resampling_path(20, 5, 1), sch, T, scaffold=True) == want
    assert path_draws(resampling_path(20, 5, 1), sch, T) == [0] + [T - t for t in sch]
    # m = 7, J = 3, R = 2 with a scaffold: second walks and the up-moves that open them sit in window 1
    sch = make_schedule(T - 1, 7)
    d = lambda p, w=0: [T - sch[p] + w * W] + ([T + (T - sch[p]) + w * W] if p < 6 else [])
    want = ([0, 2 * T + 1] + d(0) + d(1) + d(2) + [2 * T + 2 + sch[0] + W] + d(0, 1) + d(1, 1) + d(2, 1)
            + d(3) + d(4) + d(5) + [2 * T + 2 + sch[3] + W] + d(3, 1) + d(4, 1) + d(5, 1) + d(6))
    got = path_draws(resampling_path(7, 3, 2), sch, T, scaffold=True)
    assert got == want and len(set(got)) == len(got)              # fresh noise on every visit
    assert path_draws(resampling_path(7, 3, 2), sch, T, scaffold=True, partial=True) == want[1:]
    # int32 draw index: resample * W must stay below 2^31
    check_draw_range(T, 10)
    check_draw_range(T, (2 ** 31 - 1) // W)
    with pytest.raises(ValueError, match='31-bit'):
        check_draw_range(T, (2 ** 31 - 1) // W + 1)


# ---- the forward tables -------------------------------------------------------------------------------------------------------------

def test_forward_tables_satisfy_the_identities_of_the_forward_process():
    """Classes: q(x_t | x_0) = sum_{x_s} q(x_s | x_0) q(x_t | x_s), i.e. q_mats[s] @ Q_{t|s} = q_mats[t] with Q_{t|s} = jump_mats(t, s)^T.
    All three tables are float64 products rounded once to fp32 (relative error <= 2^-24 per entry; the float64 products themselves
    differ by their association only, ~1e-16) and every entry is >= 0, so evaluated in float64 from the stored values the left side
    is within (2 * 2^-24 + 2^-48) of itself and the right side within 2^-24: |diff| <= 3 * 2^-24 (1 + 2^-24) q_mats[t] + 1e-12.
    Positions, with abar in float64 from the test's own betas and (c_a, c_s) the stored fp32 values (relative error <= 2^-24 each):
      sqrt(abar_s) c_a = sqrt(abar_t):            |diff| <= 2^-24 sqrt(abar_t) + 1e-12;
      (1 - abar_s) c_a^2 + c_s^2 = 1 - abar_t:    squaring a value of relative error d gives 2 d + d^2, so
                                                  |diff| <= (2^-23 + 2^-48) ((1 - abar_s) c_a^2 + c_s^2) + 1e-12.
    (1e-12 covers the float64 evaluation.)  The identities leave sqrt(a) vs another split unpinned, so (c_a, c_s) are also compared
    bit for bit with sqrt(a), sqrt(1 - a), a = abar_t / abar_s, evaluated here in float64 and rounded once."""
    m = U.moldiff('MolDiff_simple')
    from moldiff_amd.diffusion import get_beta_schedule
    from moldiff_amd.harness import default_config
    betas = get_beta_schedule(num_timesteps=T, **default_config('MolDiff_simple').diff.diff_pos)
    abar = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    ss, tt = [p[0] for p in FORWARD_PAIRS], [p[1] for p in FORWARD_PAIRS]
    keys = sorted(m.state_dict())
    ca, cs = m.pos_transition.forward_coefs(tt, ss)
    assert ca.dtype == cs.dtype == torch.float32 and ca.shape == cs.shape == (len(tt),) and ca.is_contiguous()
    for j, (s, t) in enumerate(FORWARD_PAIRS):
        for tr in (m.node_transition, m.edge_transition):
            Q = tr.jump_mats([t], [s])[0].double().T
            qs, qt = tr.q_mats[s].detach().double(), tr.q_mats[t].detach().double()
            err, bound = (qs @ Q - qt).abs(), 3 * U24 * (1 + U24) * qt + 1e-12
            print(f'({s} -> {t}) K = {tr.num_classes}: max marginal error / bound = {float((err / bound).max()):.3f}')
            assert bool((err <= bound).all())
        a64 = abar[t] / abar[s]
        assert float(ca[j]) == float(np.float32(np.sqrt(a64))) and float(cs[j]) == float(np.float32(np.sqrt(1.0 - a64)))
        c_a, c_s = float(ca[j]), float(cs[j])
        e1, b1 = abs(np.sqrt(abar[s]) * c_a - np.sqrt(abar[t])), U24 * np.sqrt(abar[t]) + 1e-12
        lhs = (1.0 - abar[s]) * c_a ** 2 + c_s ** 2
        e2, b2 = abs(lhs - (1.0 - abar[t])), (2 * U24 + U24 ** 2) * lhs + 1e-12
        print(f'({s} -> {t}): mean identity error / bound {e1 / b1:.3f}, variance identity {e2 / b2:.3f}')
        assert e1 <= b1 and e2 <= b2
    assert sorted(m.state_dict()) == keys                        # nothing was registered
    for t, s in (([5], [5]), ([5], [6]), ([1000], [3]), ([0], [-1]), ([5], [-1]), ([5, 4], [3])):
        with pytest.raises(ValueError):
            m.pos_transition.forward_coefs(t, s)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------

def test_forward_jump_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'moldiff_hip.h')).read()
    assert 'mdx_forward_jump' in set(re.findall(r'\b(mdx_[a-z_0-9]+)\s*\(', hdr))
    assert 'no reference line' in hdr[hdr.index('resampling (RePaint'):hdr.index('int mdx_forward_jump')].lower()
    assert 'mdx_forward_jump' in _lib.EXPORTS
    L = _lib.lib()
    assert L.mdx_forward_jump.argtypes is not None and len(L.mdx_forward_jump.argtypes) == 12
    # argument checks that need no device: a null handle, class counts outside 2..8
    tb = _lib.MdxForwardTables(None, None, None, None, 9, 6, 1)
    assert L.mdx_forward_jump(None, tb, 0, None, None, None, None, None, 0.0, None, None, None) == 1
    assert b'null' in L.mdx_last_error()
