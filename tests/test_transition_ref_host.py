"""Host side of tests/test_gpu_transition_fp64.py: the float64 restatement of tests/transition_ref.py is tied to the fp32 CPU oracle
(which the goldens pin to the real reference) on the inputs of test_transition_kernels_vs_oracle; the fp32 CPU evaluations' own
distance from float64 is recorded (the GPU tests' yardsticks); and the caps the GPU tests rely on -- rows inside the Gumbel margin,
loss rows near the clamp -- are checked for exactly the GPU tests' inputs.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import moldiff_oracle as O
from tests import transition_ref as R
from tests import util as U


@pytest.mark.parametrize('part,K', [('node', 8), ('edge', 6)])
def test_restatement_equals_the_oracle_on_the_inputs_of_the_existing_kernel_test(part, K):
    """Inputs of tests/test_gpu_sampling.py::test_transition_kernels_vs_oracle (same generator, same draws in the same order).
    posterior: |oracle - float64| < 2e-5, the bound that test holds the device to; positions: inside the derived rounding bound of
    gauss64 (torch's CPU mul / add do not contract); Gumbel-max: the oracle's classes are the float64 classes outside MARGIN."""
    m = U.moldiff('MolDiff')
    tabs = U.tables(U.params(m))
    r = U.rng(21)
    bn, hei, bh, ei, be = U.graph_from_sizes([6, 9, 3, 12])
    N, Eh = len(bn), len(bh)
    t = torch.tensor([0, 1, 600, 999])
    for p, k, n, batch, tr in (('node', 8, N, bn, m.node_transition), ('edge', 6, Eh, bh, m.edge_transition)):
        logits = U.t32(r.standard_normal((n, k), dtype=np.float32) * 2)
        lvt = F.log_softmax(U.t32(r.standard_normal((n, k), dtype=np.float32) * 3), -1)
        u = U.t32(r.random((n, k), dtype=np.float32))
        if p != part:
            continue
        log_v0 = F.log_softmax(logits, -1)
        ref = O.cat_posterior(tabs[p], log_v0, lvt, t, batch)
        Q0, Q1, last = R.onestep_rows(tr, t, batch)
        p64 = R.posterior64(Q0, Q1, log_v0, lvt, last, False)
        err = float((ref.double() - p64).abs().max())
        print(f'K = {k}: max |fp32 oracle - float64| = {err:.3e} on {n} rows')
        assert err < 2e-5 and float((p64.exp().sum(-1) - 1).abs()[~last].max()) < 1e-12
        # the logits form (tests/test_schedule_host.py's posterior_fp64) is the same function of the logits
        assert float((R.posterior64(Q0, Q1, logits, lvt, last, True) - R.posterior64(Q0, Q1, F.log_softmax(logits.double(), -1), lvt, last, False)).abs().max()) < 1e-12
        c64, margin = R.gumbel_classes64(ref, u)
        sure = margin >= R.MARGIN
        assert torch.equal(O.gumbel_argmax(ref, u)[sure], c64[sure]) and int(sure.sum()) >= 0.9 * n
    if part == 'node':
        x_t, x0, eps = (U.t32(r.standard_normal((N, 3), dtype=np.float32)) for _ in range(3))
        ref = O.pos_posterior(tabs['pos'], x_t, x0, t, bn, eps)
        pt, tb = m.pos_transition, t[bn]
        want, bound = R.gauss64(pt.coef_x0.detach()[tb], pt.coef_xt.detach()[tb], pt.std.detach()[tb], x0, x_t, eps, tb == 0)
        err = (ref.double() - want).abs()
        print(f'positions: max |fp32 oracle - float64| / bound = {float((err / bound).max()):.3f}')
        assert bool((err <= bound).all())


@pytest.mark.parametrize('K', [8, 6])
def test_record_the_fp32_oracles_posterior_error(K):
    """The yardstick of the GPU posterior test, printed per input set: max |fp32 CPU oracle - float64|."""
    for tables, scale, vt in ((tb, s, v) for tb in R.TABLES for s in R.SCALES for v in ('soft', 'real')):
        errs = [R.posterior_reference(K, R.posterior_case(K, n, scale, vt), True, tables)[3] for n in R.ROWS]
        print(f'K = {K} {tables} tables, scale {scale} log_vt {vt}: max |fp32 oracle - float64| per row count {R.ROWS} = ' + ' '.join(f'{e:.2e}' for e in errs))
        assert all(np.isfinite(e) for e in errs)


@pytest.mark.parametrize('K', R.KS)
def test_gumbel_inputs_leave_at_most_half_a_percent_of_rows_inside_the_margin(K):
    ref = R.gumbel_reference(K)
    margin = torch.cat([m for _, _, _, m in ref])
    share = float((margin < R.MARGIN).double().mean())
    print(f'K = {K}: {int(margin.numel())} rows, share within {R.MARGIN} of a tie = {share:.2e}')
    assert share <= R.SKIP_CAP
    logp, u, cls, mg, tie_logp, tie_u, want = R.gumbel_edge_rows(K)
    assert float(mg.min()) >= R.MARGIN                           # the rows with extreme uniforms are all decided
    assert bool((u == 0).any(-1).all()) and bool((u == 1.0 - 2.0 ** -24).any(-1).all()) and float(u.max()) < 1.0
    z = -torch.log(-torch.log(tie_u + 1e-30) + 1e-30) + tie_logp    # fp32: the two best scores are bit-equal, torch takes the lower
    top = z.topk(2, dim=-1).values
    assert bool((top[:, 0] == top[:, 1]).all()) and torch.equal(z.argmax(-1), want)


@pytest.mark.parametrize('K', R.KS)
def test_add_noise_inputs_leave_at_most_half_a_percent_of_rows_inside_the_margin(K):
    ref = R.noise_reference(K)
    margin = torch.cat([m for _, _, _, m, _ in ref])
    share = float((margin < R.MARGIN).double().mean())
    print(f'K = {K}: {int(margin.numel())} rows, share within {R.MARGIN} of a tie = {share:.2e}')
    assert share <= R.SKIP_CAP
    assert all(bool((c['t'][c['batch']] == 0).any()) and bool((c['t'][c['batch']] == 1).any()) for _, c, _, _, _ in ref if c['batch'].numel() > 1)


@pytest.mark.parametrize('K', R.KS)
def test_loss_inputs_flag_at_most_half_a_percent_of_rows_and_reach_the_clamp(K):
    """Records the yardsticks of the GPU loss test (the fp32 CPU torch tail against float64, flagged rows left out) and checks what
    that test relies on: <= 0.5 % of the rows near the clamp, rows on the zero-gradient side of the -32 gate present, t == 0 and
    t == 1 rows in every launch of more than one row."""
    ref = R.loss_reference(K)
    near = torch.cat([r['near'] for r in ref])
    gated = torch.cat([r['gated'] for r in ref])
    e_row, e_l2, e_max = R.loss_errors([r['row32'] for r in ref], [r['g32'] for r in ref], ref)
    print(f'K = {K}: {int(near.numel())} rows, {int(near.sum())} near the clamp, {int(gated.sum())} with a class under it; fp32 CPU tail vs '
          f'float64: rows {e_row:.3e}, gradient L2 {e_l2:.3e}, max-norm {e_max:.3e}')
    assert float(near.double().mean()) <= R.FLAG_CAP
    assert int((gated & ~near).sum()) >= 10
    for r in ref:
        assert torch.isfinite(r['row64']).all() and torch.isfinite(r['g64']).all()
        assert float(r['g64'].sum(-1).abs().max()) < 1e-12 * max(1.0, float(r['g64'].abs().max()))      # rows of d/d logits sum to 0
    assert all(bool((r['case']['t'][r['case']['batch']] == 0).any()) and bool((r['case']['t'][r['case']['batch']] == 1).any()) for r in ref if r['case']['batch'].numel() > 1)


@pytest.mark.parametrize('K', [2, 6])
def test_record_the_fp32_error_of_the_uncertainty_gradient(K):
    for scale in R.SCALES:
        x = torch.cat([R.uncertainty_case(K, n, scale) for n in R.ROWS])
        g32 = R.uncertainty_grad(x, torch.float32)[0]
        rel, low = R.uncertainty_errors(g32, x)
        print(f'K = {K} scale {scale}: fp32 CPU torch vs float64, max relative to the row\'s largest entry = {rel:.3e}; '
              f'{int(low.shape[0])} rows with lse < -40')
        assert np.isfinite(rel) and low.shape[0] >= len(R.ROWS) * len(R.SATURATED)
        g64 = R.uncertainty_grad64(x)
        assert float((g64.sum(-1) + torch.sigmoid(torch.logsumexp(x.double(), -1))).abs().max()) < 1e-15     # rows sum to -sigmoid(lse)


def test_row_cases_have_the_asked_levels_and_an_empty_molecule():
    for n in R.ROWS:
        t, batch = R.rows_case(n, 3)
        assert t.shape == (R.B,) and t[:3].tolist() == [0, 1, 2] and int(t.max()) == R.T - 1 and batch.shape == (n,)
        assert bool((batch[1:] >= batch[:-1]).all()) and not bool((batch == R.EMPTY).any())
        assert n == 1 or set(batch.tolist()) == set(range(R.B)) - {R.EMPTY}
    for name, sizes in R.FUSED_SIZES.items():
        N, Eh = sum(sizes), sum(s * (s - 1) // 2 for s in sizes)
        assert {'Eh<N': Eh < N, 'N<Eh<3N': N < Eh < 3 * N, 'Eh>3N': Eh > 3 * N}[name]
