"""CPU test of the minimiser that relax_ref and embed_ref share (moldiff_amd/relax.py: lbfgs_ref), on its own: a convex quadratic
E = 1/2 sum_a w_a |x_a - c_a|^2 with unequal weights, whose minimum c is known and whose gradient is w_a (x_a - c_a).  At a point with
rms gradient <= gtol every component of the gradient is at most gtol sqrt(D n) in magnitude, so every coordinate lies within
gtol sqrt(D n) / min w of the minimum: that is the bound asked for."""
import numpy as np
import pytest

from moldiff_amd import relax as R

GTOL = 1e-6


def quadratic(n, D):
    rng = np.random.default_rng(100 * D + n)
    return rng.uniform(0.5, 4.0, size=(n, 1)), rng.normal(size=(n, D))


def run(n, D, start, max_step):
    w, c = quadratic(n, D)
    calls, trace = [], []

    def evaluate(x):
        calls.append(x.copy())
        d = x - c
        return R.block_sum((0.5 * (w * d * d).sum(axis=1)).tolist()), w * d, len(calls)
    r = R.lbfgs_ref(c + start, evaluate, 500, GTOL, max_step, trace)
    assert r['n_evals'] == len(calls) and r['first'] == 1 and r['x'].shape == (n, D)
    return w, c, r, trace


@pytest.mark.parametrize('n,D', [(5, 3), (3, 4)])
def test_a_convex_quadratic_is_minimised_with_and_without_the_step_cap(n, D):
    offset = np.random.default_rng(7).normal(size=(n, D))
    for max_step, capped in ((10.0, False), (0.05, True)):
        w, c, r, trace = run(n, D, offset, max_step)
        assert r['stop_reason'] == R.STOP_CONVERGED and r['rms'] <= GTOL and 0 < r['iterations'] == len(r['energies']) <= 500
        assert np.abs(r['x'] - c).max() <= GTOL * np.sqrt(D * n) / w.min()
        assert np.array_equal(r['grad'], w * (r['x'] - c)) and r['energy'] == r['energies'][-1] and r['extra'] <= r['n_evals']
        e = [float(R.block_sum((0.5 * (w * offset * offset).sum(axis=1)).tolist()))] + r['energies']
        assert all(b <= a for a, b in zip(e, e[1:]))
        assert any(k == 'cap' and v > th for k, v, th in trace) == capped
        assert {k for k, _, _ in trace} <= {'rms', 'descent', 'cap', 'armijo', 'curvature'} and trace[0][0] == 'rms'
        steps = [v for k, v, _ in trace if k == 'cap']
        assert len(steps) >= r['iterations']


@pytest.mark.parametrize('n,D', [(5, 3), (3, 4)])
def test_a_start_at_the_minimum_takes_no_iteration_and_one_evaluation(n, D):
    w, c, r, trace = run(n, D, np.zeros((n, D)), 0.3)
    assert (r['stop_reason'], r['iterations'], r['n_evals'], r['energies']) == (R.STOP_CONVERGED, 0, 1, [])
    assert r['energy'] == 0.0 and r['rms'] == 0.0 and np.array_equal(r['x'], c) and trace == [('rms', 0.0, GTOL)]


def test_a_start_that_is_not_finite_and_no_atom():
    assert R.lbfgs_ref(np.zeros((2, 3)), lambda x: (float('nan'), x, None), 5, GTOL, 0.3, []) is None
    assert R.lbfgs_ref(np.zeros((2, 3)), lambda x: (0.0, x + float('inf'), None), 5, GTOL, 0.3, []) is None
    r = R.lbfgs_ref(np.zeros((0, 4)), lambda x: (0.0, x, None), 5, GTOL, 0.3, [])
    assert (r['iterations'], r['n_evals'], r['rms']) == (0, 1, 0.0)
