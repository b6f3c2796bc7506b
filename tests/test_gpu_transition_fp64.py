"""GPU: the row kernels of csrc/mdx_transition.hip against the float64 restatement of tests/transition_ref.py, at every class count
K = 2..8 the dispatch instantiates, at row counts around a block boundary (1, 255, 256, 257, 1000), with t == 0 and t == 1 rows in
every launch of more than one row, one empty molecule, and on two table sets: the shipped ones and a sparse-prior one on which the
-32 clamp (and the gate of the loss backward) really acts (tests/transition_ref.py: transition).

Every tolerance is a derived rounding bound or `4 x the measured error of an fp32 CPU evaluation of the same formula against float64`
(tests/test_transition_ref_host.py prints those yardsticks and checks the caps on skipped rows for exactly these inputs).  The factor 4
allows for expf / logf differing by an ulp or two between the host libm and the device over the few rounded operations per entry.
Each test prints the reference's error next to the device's."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moldiff_amd import _lib
from moldiff_amd.schedule import pairs
from tests import test_schedule_host as H
from tests import transition_ref as R
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FACTOR = 4.0
OK, UNSUPPORTED = 0, 4          # MDX_OK, MDX_ERR_UNSUPPORTED (include/moldiff_hip.h)


@functools.lru_cache(maxsize=None)
def _tr(K, tables='model'):
    return copy.deepcopy(R.transition(K, tables)).to(DEV)


def _d(*xs):
    return tuple(x.to(DEV) for x in xs)


def _check_posterior(outs, ref, e_ref, last, t0_want, what):
    """|device - float64| <= 4 x the fp32 CPU oracle's error on the same input + one fp32 ulp of the largest |log p|; rows at t == 0
    within 2 ulp (at the row's largest magnitude) of t0_want.  Returns the worst device error / tolerance."""
    tol = FACTOR * e_ref + float(R.ulp32(ref.abs().max()))
    worst = 0.0
    for o in outs:
        o = o.cpu().double()
        assert torch.isfinite(o).all(), what
        e_dev = float((o - ref).abs().max())
        assert e_dev <= tol, f'{what}: device {e_dev:.3e}, fp32 oracle {e_ref:.3e}, tolerance {tol:.3e}'
        worst = max(worst, e_dev / tol)
        if bool(last.any()):
            want = t0_want[last].double()
            assert bool(((o[last] - want).abs() <= 2 * R.ulp32(want.abs().amax(dim=-1, keepdim=True))).all()), what
    return worst, tol


@pytest.mark.parametrize('is_logits', [0, 1])
@pytest.mark.parametrize('K', R.KS)
def test_cat_posterior_follows_float64_at_every_class_count(K, is_logits):
    """mdx_cat_posterior through _lib.cat_posterior and (log-probability form) q_v_posterior(v0_prob=True).
    Measured on MI355X, worst launch per parameter (device error / tolerance): between 0.34 and 0.78 over the 14 parameters.  The
    worst, K = 2 on one row at scale 0.3: device 9.1e-07, fp32 CPU oracle 5.4e-08, tolerance 1.17e-06 (the ulp term carries it: one
    row under-samples the oracle's error); at 255+ rows, K = 5: device 2.4e-06, oracle 1.2e-06; K = 7 sparse tables: 5.2e-06, 2.1e-06."""
    worst, line = 0.0, ''
    for tables in R.TABLES:
        tr = _tr(K, tables)
        for scale in R.SCALES:
            for vt in ('soft', 'real'):
                for n in R.ROWS:
                    case = R.posterior_case(K, n, scale, vt)
                    in0, ref, last, e_ref = R.posterior_reference(K, case, is_logits, tables)
                    a, lvt, t, batch = _d(in0, case['log_vt'], case['t'], case['batch'])
                    outs = [_lib.cat_posterior(tr.q_mats, tr.transpopse_q_onestep_mats, a, lvt, t, batch, is_logits=bool(is_logits))]
                    if not is_logits:
                        outs.append(tr.q_v_posterior(a, lvt, t, batch, v0_prob=True))
                    t0_want = F.log_softmax(case['logits'], dim=-1)          # fp32: the kernel's log-softmax, or the input itself
                    what = f'K={K} {tables} scale={scale} log_vt={vt} n={n}'
                    w, tol = _check_posterior(outs, ref, e_ref, last, t0_want, what)
                    if w > worst:
                        worst = w
                        line = f'{what}: device {w * tol:.3e}, fp32 oracle {e_ref:.3e}, tolerance {tol:.3e}'
    print(f'\ncat_posterior K = {K} is_logits = {is_logits}: worst device error / tolerance {worst:.3f} ({line})')


@pytest.mark.parametrize('K', [2, 5, 7])
def test_cat_posterior_jump_row_form_follows_float64(K):
    """the per-graph `row` form (mdx_cat_posterior_jump): one (t, s) pair per molecule through the keyword t_prev= and through
    _lib.cat_posterior_jump on logits; same rule as cat_posterior."""
    worst = 0.0
    for tables in R.TABLES:
        tr, tr_dev = R.transition(K, tables), _tr(K, tables)
        for scale in R.SCALES:
            for n in R.ROWS:
                case = R.posterior_case(K, n, scale, 'real')
                t, b = case['t'], case['batch']
                s = R.jump_levels(t)
                tt, ss, row = H.pair_rows(t, s)
                qj = tr.jump_mats(tt, ss)
                rows = (tr.q_mats.detach()[s[b].clamp(min=0)], qj[row[b]], t[b] == 0)
                lg, lvt, td, sd, rd, bd = _d(case['logits'], case['log_vt'], t, s, row, b)
                for is_logits in (0, 1):
                    in0, ref, last, e_ref = R.posterior_reference(K, case, is_logits, tables, rows)
                    if is_logits:
                        out = _lib.cat_posterior_jump(tr_dev.q_mats, qj.to(DEV), lg, lvt, td, sd, rd, bd, is_logits=True)
                    else:
                        out = tr_dev.q_v_posterior(in0.to(DEV), lvt, td, bd, v0_prob=True, t_prev=sd)
                    w, _ = _check_posterior([out], ref, e_ref, last, F.log_softmax(case['logits'], dim=-1),
                                            f'K={K} {tables} scale={scale} n={n} is_logits={is_logits}')
                    worst = max(worst, w)
    print(f'\ncat_posterior_jump (row form) K = {K}: worst device error / tolerance {worst:.3f}')


@pytest.mark.parametrize('kn,ke', [(7, 5), (2, 2)])
def test_cat_posterior_jump_launch_scalar_form_follows_float64(kn, ke):
    """The launch-scalar form has no entry point of its own: it is what mdx_sample_jump_full launches for class counts other than 8 / 6.
    Teacher-forced iterations of the schedule [999, 300, 2, 1, 0] (t = 999, 300, 2, 1 and 0; every molecule shares the level), on a
    graph whose half-edge count (257) and one whose atom count (257) cross a block: the log rows the call wrote against the float64
    posterior of the call's own predictions, same rule as cat_posterior; the classes are the stand-alone Gumbel-max of those rows."""
    mk = copy.deepcopy(R.other_model(kn, ke)).to(DEV)
    sch = [999, 300, 2, 1, 0]
    tt, ss = (list(x) for x in zip(*pairs(sch)))
    worst = 0.0
    for sizes in ([23, 3, 0, 2, 1, 1, 1], [2] * 127 + [3]):
        bn, hei, bh, _, _ = U.graph_from_sizes(sizes, DEV)
        N, Eh, Bm = int(bn.numel()), int(bh.numel()), len(sizes)
        assert 257 in (N, Eh)
        for j, (t, s) in enumerate(zip(tt, ss)):
            g = U.rng(50 + j)
            hn = F.one_hot(torch.from_numpy(g.integers(0, kn, N)), kn).float().to(DEV)
            hh = F.one_hot(torch.from_numpy(g.integers(0, ke, Eh)), ke).float().to(DEV)
            pos = U.t32(g.standard_normal((N, 3))).to(DEV)
            ln, lh = torch.log(hn.clamp(min=1e-30)), torch.log(hh.clamp(min=1e-30))
            sm = mk.sampler(Bm, bn, hei, bh, seed=3, timesteps=sch)
            sm.set_state(hn, pos, hh, ln, lh, frame=j)
            sm.step(j)
            st = sm.state()
            for K, tr, n, pred, lvt, log_next, oh, u in ((kn, mk.node_transition, N, sm.preds[0], ln, st['log_node'], st['h_node'], sm.u_n),
                                                         (ke, mk.edge_transition, Eh, sm.preds[2], lh, st['log_halfedge'], st['h_halfedge'], sm.u_h)):
                qj = tr.jump_mats(tt, ss).cpu()
                last = torch.full((n,), t == 0)
                rows = (tr.q_mats.detach().cpu()[max(s, 0)].expand(n, K, K), qj[j].expand(n, K, K), last)
                case = {'logits': pred.cpu(), 'log_vt': lvt.cpu()}
                _, ref, _, e_ref = R.posterior_reference(K, case, True, rows=rows)
                w, _ = _check_posterior([log_next], ref, e_ref, last, F.log_softmax(case['logits'], dim=-1), f'K={K} t={t} s={s} n={n}')
                worst = max(worst, w)
                assert torch.equal(oh, _lib.gumbel_argmax(log_next, u, want_onehot=True)[1])
    print(f'\ncat_posterior_jump (launch-scalar form) K = {kn} / {ke}: worst device error / tolerance {worst:.3f}')


@pytest.mark.parametrize('K', R.KS)
def test_gumbel_argmax_draws_the_float64_class(K):
    """On the fp32 rounding of the float64 posterior: classes bit-equal to the float64 Gumbel-max outside MARGIN (skipped share <=
    SKIP_CAP: the host test established it for these inputs); the one-hot row has exactly one 1, at the class; uniforms at the
    extremes of the noise kernel (0 and 1 - 2^-24) draw the float64 class; two bit-equal best scores go to the lower index."""
    skipped = total = 0
    for logp, u, c64, margin in R.gumbel_reference(K):
        cls, oh = _lib.gumbel_argmax(*_d(logp, u), want_onehot=True)
        cls, oh = cls.cpu(), oh.cpu()
        sure = margin >= R.MARGIN
        assert torch.equal(cls[sure], c64[sure])
        assert torch.equal(oh, F.one_hot(cls, K).float())
        skipped += int((~sure).sum()); total += int(sure.numel())
    print(f'\ngumbel_argmax K = {K}: skipped {skipped} of {total} rows')
    assert skipped <= R.SKIP_CAP * total
    logp, u, c64, _, tie_logp, tie_u, want = R.gumbel_edge_rows(K)
    assert torch.equal(_lib.gumbel_argmax(*_d(logp, u)).cpu(), c64)
    cls, oh = _lib.gumbel_argmax(*_d(tie_logp, tie_u), want_onehot=True)
    assert torch.equal(cls.cpu(), want) and torch.equal(oh.cpu(), F.one_hot(want, K).float())


@pytest.mark.parametrize('C', R.WIDTHS)
def test_gaussian_posterior_follows_float64_at_every_width(C):
    """mdx_gauss_posterior directly (every width, C = 3 included) and through _lib.pos_posterior (C = 3: mdx_pos_posterior) inside the
    derived rounding bound 3 * 2^-24 (|a| + |b| + |c|)(1 + 2^-20) of tests/transition_ref.py gauss64; no noise term at t == 0."""
    pt = U.moldiff('MolDiff', DEV).pos_transition
    c0, ct, sd = (x.detach().cpu() for x in (pt.coef_x0, pt.coef_xt, pt.std))
    worst = 0.0
    for n in R.ROWS:
        case = R.gauss_case(C, n)
        tb = case['t'][case['batch']]
        want, bound = R.gauss64(c0[tb], ct[tb], sd[tb], case['x0'], case['xt'], case['eps'], tb == 0)
        xt, x0, eps, t, batch = _d(case['xt'], case['x0'], case['eps'], case['t'], case['batch'])
        direct = torch.full_like(xt, float('nan'))
        assert _lib.lib().mdx_gauss_posterior(*(_lib.ptr(x) for x in (pt.coef_x0, pt.coef_xt, pt.std, xt, x0, eps, t, batch)), n, C,
                                              _lib.ptr(direct), _lib.stream()) == OK
        for got in (direct, _lib.pos_posterior(pt.coef_x0, pt.coef_xt, pt.std, xt, x0, eps, t, batch)):
            err = (got.cpu().double() - want).abs()
            assert bool((err <= bound).all()), (C, n, float((err / bound).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((tb == 0).any()) or n == 1
    print(f'\ngauss_posterior C = {C}: worst error / bound {worst:.3f}')


@pytest.mark.parametrize('scale', R.SCALES)
@pytest.mark.parametrize('K', [2, 6])
def test_uncertainty_gradient_follows_float64(K, scale):
    """mdx_guidance_uncertainty_grad directly: -sigmoid(lse) softmax.  Relative to the row's largest entry, pooled over the row counts,
    within 4 x the error of the same expression evaluated by torch in fp32 on the CPU; rows with lse < -40 (sigmoid underflows,
    expf(-lse) overflows at -100 and below) finite and below 1e-15.
    Measured on MI355X (device / fp32 CPU torch): K = 2: 1.7e-07 / 2.0e-07, 2.4e-07 / 2.4e-07, 1.8e-06 / 1.8e-06 at scales 0.3, 3, 40;
    K = 6: 1.9e-07 / 2.6e-07, 2.7e-07 / 2.7e-07, 9.1e-07 / 9.1e-07; rows below -40 at most 3.4e-18."""
    xs, gots = [], []
    for n in R.ROWS:
        x = R.uncertainty_case(K, n, scale).to(DEV)
        out = torch.full_like(x, float('nan'))
        assert _lib.lib().mdx_guidance_uncertainty_grad(_lib.ptr(x), K, x.shape[0], _lib.ptr(out), _lib.stream()) == OK
        xs.append(x.cpu()); gots.append(out.cpu())
    x, got = torch.cat(xs), torch.cat(gots)
    e_ref, _ = R.uncertainty_errors(R.uncertainty_grad(x, torch.float32)[0], x)
    e_dev, low = R.uncertainty_errors(got, x)
    print(f'\nuncertainty_grad K = {K} scale {scale}: device {e_dev:.3e}, fp32 CPU torch {e_ref:.3e} (relative to the row\'s largest entry); '
          f'{int(low.shape[0])} rows with lse < -40, largest magnitude {float(low.abs().max()):.3e}')
    assert torch.isfinite(got).all() and low.shape[0] >= len(R.ROWS) * len(R.SATURATED)
    assert float(low.abs().max()) < 1e-15
    assert e_dev <= FACTOR * e_ref


@pytest.mark.parametrize('n', [1, 255, 257, 1000])
def test_add_inplace_is_the_fp32_sum(n):
    g = U.rng(17 + n)
    dst, src = U.t32(g.standard_normal(n) * 10.0 ** g.integers(-3, 4, n)), U.t32(g.standard_normal(n))
    want = dst + src
    d, s = _d(dst, src)
    guard = torch.full((n + 64,), 7.0, device=DEV)      # the destination lies inside a sentinel-filled buffer
    guard[32:32 + n] = d
    assert _lib.lib().mdx_add_inplace(guard[32:].data_ptr(), _lib.ptr(s), n, _lib.stream()) == OK
    assert torch.equal(guard[32:32 + n].cpu(), want) and bool((guard[:32] == 7.0).all()) and bool((guard[32 + n:] == 7.0).all())


@pytest.mark.parametrize('K', R.KS)
def test_cat_add_noise_draws_the_float64_class(K):
    """mdx_op_cat_add_noise: classes equal the float64 draw outside MARGIN (share <= SKIP_CAP); log_v0 within 2 ulp of the float64
    value's fp32 rounding; log_vt and the one-hot row exact functions of the class; class ids -1 and K are clamped to 0 and K - 1."""
    off = _lib.log_eps32()
    skipped = total = 0
    for tables, case, c64, margin, lv0_64 in R.noise_reference(K):
        tr = _tr(K, tables)
        oh, lvt, lv0 = (x.cpu() for x in _lib.cat_add_noise(tr.q_mats, *_d(case['v'], case['t'], case['batch'], case['u']), K))
        cls = oh.argmax(-1)
        sure = margin >= R.MARGIN
        assert torch.equal(cls[sure], c64[sure])
        assert torch.equal(oh, F.one_hot(cls, K).float())
        assert torch.equal(lvt, torch.where(oh == 1, torch.zeros(()), torch.full((), off)))
        assert bool(((lv0.double() - lv0_64.float().double()).abs() <= 2 * R.ulp32(lv0_64) * (lv0_64 != 0)).all())
        skipped += int((~sure).sum()); total += int(sure.numel())
    print(f'\ncat_add_noise K = {K}: skipped {skipped} of {total} rows')
    assert skipped <= R.SKIP_CAP * total
    case = R.noise_case(K, 257)
    v = case['v'].clone()
    v[::5], v[1::5] = -1, K
    tr = R.transition(K)
    c64, margin, lv0_64 = R.add_noise64(tr.q_mats.detach()[case['t'][case['batch']]], v, case['u'])
    oh, lvt, lv0 = (x.cpu() for x in _lib.cat_add_noise(_tr(K).q_mats, *_d(v, case['t'], case['batch'], case['u']), K))
    sure = margin >= R.MARGIN
    assert int(sure.sum()) >= 250 and torch.equal(oh.argmax(-1)[sure], c64[sure])
    assert torch.equal(lv0.argmax(-1), v.clamp(0, K - 1)) and bool((lv0.max(-1).values == 0).all())


@pytest.mark.parametrize('K', R.KS)
def test_cat_loss_rows_and_gradient_follow_float64(K):
    """mdx_op_cat_loss directly, against torch autograd in float64 on the CPU over the reference's formula (tests/transition_ref.py
    cat_loss_tail).  Rows within NEAR of the clamp are left out (<= 0.5 %: the host test); pooled over table sets and row counts:
    per-row loss within 4 x the fp32 CPU torch tail's error against float64, the gradient in relative L2 and max-norm within 4 x the
    same tail's.  Separately: t == 0 rows are the NLL with gradient softmax - onehot; every gradient row sums to zero within 8 ulp of
    its largest entry; rows on the zero-gradient side of the -32 gate occur."""
    ref = R.loss_reference(K)
    rows, grads = [], []
    for r in ref:
        tr, c = _tr(K, r['tables']), r['case']
        n = c['batch'].numel()
        lg, lvt, lv0, t, b = _d(c['logits'], c['log_vt'], c['log_v0'], c['t'], c['batch'])
        row, dl = torch.full((n,), float('nan'), device=DEV), torch.full((n, K), float('nan'), device=DEV)
        assert _lib.lib().mdx_op_cat_loss(_lib.ptr(tr.q_mats), _lib.ptr(tr.transpopse_q_onestep_mats), K, R.T, *(_lib.ptr(x) for x in (lg, lvt, lv0, t, b)),
                                          n, _lib.ptr(row), _lib.ptr(dl), _lib.stream()) == OK
        rows.append(row.cpu()); grads.append(dl.cpu())
        assert torch.isfinite(rows[-1]).all() and torch.isfinite(grads[-1]).all()
    y_row, y_l2, y_max = R.loss_errors([r['row32'] for r in ref], [r['g32'] for r in ref], ref)
    d_row, d_l2, d_max = R.loss_errors(rows, grads, ref)
    near = torch.cat([r['near'] for r in ref])
    gated = torch.cat([r['gated'] for r in ref])
    print(f'\ncat_loss K = {K}: rows device {d_row:.3e} / fp32 CPU tail {y_row:.3e}; gradient L2 {d_l2:.3e} / {y_l2:.3e}; max-norm {d_max:.3e} / '
          f'{y_max:.3e}; {int(near.sum())} of {int(near.numel())} rows left out, {int((gated & ~near).sum())} compared rows with a class under the clamp')
    assert float(near.double().mean()) <= R.FLAG_CAP and int((gated & ~near).sum()) > 0
    assert d_row <= FACTOR * y_row
    assert d_l2 <= FACTOR * y_l2 and d_max <= FACTOR * y_max
    gmax = float(torch.cat([r['g64'] for r in ref]).abs().max())
    for r, row, dl in zip(ref, rows, grads):
        c = r['case']
        dl64 = dl.double()
        assert bool((dl64.sum(-1).abs() <= 8 * R.ulp32(dl64.abs().amax(-1).clamp_min(2.0 ** -126))).all())
        last = c['t'][c['batch']] == 0
        if bool(last.any()):
            lr = torch.log_softmax(c['logits'].double(), -1)[last]
            onehot = (c['log_v0'][last] == 0).double()
            nll = -(c['log_v0'][last].double().exp() * lr).sum(-1)
            assert float((row.double()[last] - nll).abs().max()) <= FACTOR * y_row
            assert float((dl64[last] - (lr.exp() - onehot)).abs().max()) <= FACTOR * y_max * gmax


@pytest.mark.parametrize('kind', ['plain', 'jump'])
@pytest.mark.parametrize('regime', list(R.FUSED_SIZES))
def test_fused_step_equals_the_standalone_kernels_in_every_index_regime(regime, kind):
    """step_transition_kernel / step_jump_kernel serve 3N position components, N atom rows and Eh half-edge rows with one thread index.
    Teacher-forced steps with injected noise on MolDiff_simple, t = 0 included: next positions, log rows, one-hot rows and class bytes
    bit-equal to the stand-alone launches on the call's own network outputs."""
    m = U.moldiff('MolDiff_simple', DEV)
    sizes = R.FUSED_SIZES[regime]
    bn, hei, bh, _, _ = U.graph_from_sizes(sizes, DEV)
    N, Eh, Bm = int(bn.numel()), int(bh.numel()), len(sizes)
    assert {'Eh<N': Eh < N, 'N<Eh<3N': N < Eh < 3 * N, 'Eh>3N': Eh > 3 * N}[regime]
    pt, ntr, etr = m.pos_transition, m.node_transition, m.edge_transition

    def noise(draw):
        g = U.rng(2000 + draw)
        return (U.t32(g.standard_normal((N, 3))).to(DEV), U.t32(g.random((N, 8), dtype=np.float32)).to(DEV),
                U.t32(g.random((Eh, 6), dtype=np.float32)).to(DEV))

    sch = [999, 300, 1, 0]
    tt, ss = (list(x) for x in zip(*pairs(sch)))
    moves = [(j, t, s) for j, (t, s) in enumerate(zip(tt, ss))] if kind == 'jump' else [(0, 999, 998), (998, 1, 0), (999, 0, -1)]
    if kind == 'jump':
        c0, ct, sd = pt.jump_coefs(tt, ss)
    for it, t, s in moves:
        sm = m.sampler(Bm, bn, hei, bh, noise=noise, **(dict(timesteps=sch) if kind == 'jump' else {}))
        g = U.rng(60 + it)
        hn = F.one_hot(torch.from_numpy(g.integers(0, 8, N)), 8).float().to(DEV)
        hh = F.one_hot(torch.from_numpy(g.integers(0, 6, Eh)), 6).float().to(DEV)
        pos = U.t32(g.standard_normal((N, 3))).to(DEV)
        ln, lh = torch.log(hn.clamp(min=1e-30)), torch.log(hh.clamp(min=1e-30))
        sm.set_state(hn, pos, hh, ln, lh, frame=it)
        sm.step(it)
        st = sm.state()
        tv = torch.full((Bm,), t, dtype=torch.int64, device=DEV)
        sv, rv = torch.full_like(tv, s), torch.full_like(tv, it)
        assert torch.equal(sm.t[:Bm], tv)
        if kind == 'jump':
            want_pos = _lib.pos_posterior_jump(c0, ct, sd, pos, sm.preds[1], sm.eps, tv, rv, bn)
        else:
            want_pos = _lib.pos_posterior(pt.coef_x0, pt.coef_xt, pt.std, pos, sm.preds[1], sm.eps, tv, bn)
        assert torch.equal(st['pos'], want_pos) and torch.isfinite(want_pos).all()
        for tr, batch, pred, lvt, u, oh, lg, ids in ((ntr, bn, sm.preds[0], ln, sm.u_n, st['h_node'], st['log_node'], sm.node_ids[sm.pcur]),
                                                     (etr, bh, sm.preds[2], lh, sm.u_h, st['h_halfedge'], st['log_halfedge'], sm.half_ids[sm.pcur])):
            if kind == 'jump':
                post = _lib.cat_posterior_jump(tr.q_mats, tr.jump_mats(tt, ss), pred, lvt, tv, sv, rv, batch, is_logits=True)
            else:
                post = _lib.cat_posterior(tr.q_mats, tr.transpopse_q_onestep_mats, pred, lvt, tv, batch, is_logits=True)
            cls, onehot = _lib.gumbel_argmax(post, u, want_onehot=True)
            assert torch.equal(lg, post) and torch.equal(oh, onehot) and torch.equal(ids.long(), cls)
            assert torch.isfinite(post).all()


def test_empty_calls_touch_nothing_and_unsupported_class_counts_are_refused():
    """n = 0: every entry point returns MDX_OK and leaves a sentinel-filled output untouched.  K = 1 and K = 9: mdx_cat_posterior,
    mdx_cat_posterior_jump, mdx_op_cat_loss and mdx_op_cat_add_noise return MDX_ERR_UNSUPPORTED, outputs untouched.  Every pointer is
    valid and every buffer large enough for 4 rows of 9 classes, so a missing check cannot fault."""
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream
    n, KM, Tt = 4, 9, 3
    g = U.rng(1)
    tab = torch.softmax(U.t32(g.standard_normal((Tt, KM, KM))), -1).to(DEV)
    coef = U.t32(g.random(Tt)).to(DEV)
    a, b2, c = (U.t32(g.standard_normal((n, KM))).to(DEV) for _ in range(3))
    u = U.t32(g.random((n, KM), dtype=np.float32)).to(DEV)
    t = torch.tensor([0, 1, 2, 1], device=DEV)
    z = torch.zeros(n, dtype=torch.int64, device=DEV)
    v = torch.zeros(n, dtype=torch.int64, device=DEV)
    outs = [torch.full((n, KM), 7.0, device=DEV) for _ in range(3)]
    row = torch.full((n,), 7.0, device=DEV)
    cls = torch.full((n,), 7, dtype=torch.int64, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((o == 7.0).all()) for o in outs) and bool((row == 7.0).all()) and bool((cls == 7).all())

    o0, o1, o2 = (P(o) for o in outs)
    off = _lib.log_eps32()
    for K, m_, want in ((4, 0, OK), (1, n, UNSUPPORTED), (9, n, UNSUPPORTED)):
        assert L.mdx_cat_posterior(P(tab), P(tab), K, Tt, P(a), 1, P(b2), P(t), P(z), m_, o0, S()) == want
        assert L.mdx_cat_posterior_jump(P(tab), P(tab), K, P(a), 1, P(b2), P(t), P(z), P(z), P(z), m_, o0, S()) == want
        assert L.mdx_op_cat_loss(P(tab), P(tab), K, Tt, P(a), P(b2), P(c), P(t), P(z), m_, P(row), o0, S()) == want
        assert L.mdx_op_cat_add_noise(P(tab), K, Tt, P(v), P(t), P(z), P(u), m_, off, o0, o1, o2, S()) == want
        assert untouched(), K
    assert L.mdx_pos_posterior(P(coef), P(coef), P(coef), P(a), P(b2), P(c), P(t), P(z), 0, o0, S()) == OK
    assert L.mdx_gauss_posterior(P(coef), P(coef), P(coef), P(a), P(b2), P(c), P(t), P(z), 0, 5, o0, S()) == OK
    assert L.mdx_pos_posterior_jump(P(coef), P(coef), P(coef), P(a), P(b2), P(c), P(t), P(z), P(z), 0, o0, S()) == OK
    assert L.mdx_gumbel_argmax(P(a), P(u), 4, 0, P(cls), o0, S()) == OK
    assert L.mdx_guidance_uncertainty_grad(P(a), 4, 0, o0, S()) == OK
    assert L.mdx_add_inplace(o0, P(a), 0, S()) == OK
    assert untouched()
