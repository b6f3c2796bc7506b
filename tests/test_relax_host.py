"""CPU tests of the force-field relaxation's plain restatement (moldiff_amd/relax.py: energy_ref, relax_ref) and of the host half of the
device entry (tools/relax_host_check.cpp under the host sanitizers).  No test depends on the parameter values being right: they check
that the gradient is the energy's, that the energy has the invariances of an energy, that the minimiser descends and stops as stated."""
import math

import numpy as np
import pytest

from moldiff_amd import relax as R
from . import relax_cases as RC
from .util import run_host_check


def _positions(c):
    return np.asarray(R._stage(*c, R.ForceFieldTables()).pos)


def _measured():
    names, cases = RC.named_lists()
    return [(k, c) for k, c in zip(names, cases) if k not in RC.DEGENERATE]


def test_gradient_agrees_with_central_differences():
    """h = 1e-5 Angstrom, 1e-5 kcal/mol/Angstrom absolute: truncation h^2 f''' / 6 is about 2e-7 and rounding E eps / h about 1e-8"""
    for name, c in _measured():
        x, e = _positions(c), R.energy_ref(*c)
        for a in range(e['n_all']):
            for k in range(3):
                hi, lo = x.copy(), x.copy()
                hi[a, k] += 1e-5
                lo[a, k] -= 1e-5
                fd = (R.energy_ref(*c, positions=hi)['total'] - R.energy_ref(*c, positions=lo)['total']) / (hi[a, k] - lo[a, k])
                assert abs(fd - e['grad'][a][k]) <= 1e-5, (name, a, k, fd, e['grad'][a][k])


def test_net_force_net_torque_and_rigid_motion():
    """net force and torque below 1e-9 of the absolute-contribution sum; the energy after a rigid motion within 1e-9 of the sum of
    absolute term energies.  For the two molecules that sit at their minimum only that last comparison is left to
    test_exact_zeros_take_no_iteration: their energy is the square of a cancelled difference, which no sum of absolute terms bounds."""
    rot = np.asarray([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])   # orthogonal
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-15)
    named = _measured()
    cases = [c for _, c in named] + RC.random_set()[:6]
    at_minimum = {m for m, (k, _) in enumerate(named) if k in ('f2_at_rest', 'methane_ideal')}
    for m, c in enumerate(cases):
        x, e = _positions(c), R.energy_ref(*c)
        g, scale = np.asarray(e['grad']), sum(e['abs_grad'])
        assert np.abs(g.sum(axis=0)).max() <= 1e-9 * scale, m
        assert np.abs(np.cross(x, g).sum(axis=0)).max() <= 1e-9 * scale * max(1.0, np.abs(x).max()), m
        moved = R.energy_ref(*c, positions=x @ rot.T + np.asarray([0.5, -1.25, 2.0]))
        assert m in at_minimum or abs(moved['total'] - e['total']) <= 1e-9 * sum(e['abs_components']), m
        assert moved['counts'] == e['counts']


def test_exact_zeros_take_no_iteration():
    """F-F at its rest length (float32 coordinates: off by at most 6e-8 Angstrom, so 1/2 k d^2 < 1e-9 kcal/mol with k < 1e3) and methane
    with the table's C-H length and the exact tetrahedral angle: every component is 0 or below 1e-9 kcal/mol in magnitude (the
    general angle form is a sum that may round to just below 0)"""
    ideal, tb = RC.ideal_methane()
    for c, tables in ((RC.named()['f2_at_rest'], None), (ideal, tb)):
        r = R.relax_ref(*c, tables)
        assert (r['status'], r['stop_reason'], r['iterations'], r['n_evals']) == (R.STATUS_OK, R.STOP_CONVERGED, 0, 1)
        assert all(abs(v) <= 1e-9 for v in r['energy'][:6]) and r['energy'][2] == 0.0 and r['energy'][3] == 0.0 and r['energy'][4] == 0.0
        assert r['energy'][13] == 0.0


def test_descent_convergence_and_the_stretched_bond():
    names = RC.named_lists()[0]
    for m, (r, _) in enumerate(RC.refs(200)):
        e = [r['energy'][5]] + r['energies']
        assert all(b <= a for a, b in zip(e, e[1:])), m
        if r['status'] == R.STATUS_OK:
            assert len(r['energies']) == r['iterations'] and r['energy'][11] <= r['energy'][5]
            assert (r['energy'][12] <= R.DEFAULT_GTOL) == (r['stop_reason'] == R.STOP_CONVERGED)
        if m < len(names) and names[m] not in RC.DEGENERATE:
            assert r['status'] == R.STATUS_OK and r['stop_reason'] == R.STOP_CONVERGED and r['iterations'] <= 200, names[m]
    r = RC.refs(200)[names.index('ethane_stretched')][0]
    tb = R.ForceFieldTables()
    rest = tb.pair(tb.type_of[0, 0][0], tb.type_of[0, 0][0], 0)[0]
    assert abs(np.linalg.norm(r['pos'][0] - r['pos'][1]) - rest) <= 0.1      # a sanity bound, not an accuracy claim
    r = RC.refs(200)[names.index('coincident')][0]
    assert r['status'] == R.STATUS_NONFINITE and not r['energy'].any() and not r['pos'].any()


def test_statuses_and_term_counts_of_the_size_ladder():
    got = RC.ladder_refs(1)
    assert [r['status'] for r in got] == [0] * 9 + [R.STATUS_TOO_LARGE]
    for n, r in zip(RC.LADDER, got):
        assert r['n_all'] == n and r['n_ff_bonds'] == max(n - 1, 0) and r['n_angles'] == max(n - 2, 0) and r['n_torsions'] == max(n - 3, 0)
        assert r['n_inversions'] == 0 and r['n_pairs'] == max(n - 2, 0) * max(n - 3, 0) // 2 and r['n_fallback'] == 0
    assert got[0]['stop_reason'] == R.STOP_CONVERGED and got[1]['stop_reason'] == R.STOP_CONVERGED and got[1]['iterations'] == 0
    last = got[-1]
    assert all(last[k] == 0 for k in R.STAT_KEYS[1:]) and not last['energy'].any() and not last['pos'].any() and last['n_atoms'] == 254
    stacked = R.stack_ref([c[0] for c in RC.ladder()[:5]], [c[1:] for c in RC.ladder()[:5]], max_iters=1)
    assert stacked['energy'].shape == (5, 14) and stacked['pos'].shape == (10, 3) and stacked['h_pos'].shape == (10, 4, 3)
    assert R.mol_result(stacked, 4)['n_all'] == 4 and set(R.empty()) == set(stacked)


def test_validation_raises_as_the_c_side_refuses():
    import yaml
    with open(R.DEFAULT_TABLE) as f:
        good = yaml.safe_load(f)
    tb = R.ForceFieldTables(table=good)
    assert tb.rows.shape == (19, 11) and tb.type_of[4, 1] == (tb.type_of[4, 0][0], True) and tb.type_of[0, 3][1] is False

    def changed(path, value):
        t = yaml.safe_load(yaml.safe_dump(good))
        d = t['elements']
        for k in path[:-1]:
            d = d[k]
        if value is None:
            del d[path[-1]]
        else:
            d[path[-1]] = value
        return t
    for path, value in (((1,), None), ((6,), None), ((6, 'variants', 'tetrahedral'), None), ((6, 'variants', 'tetrahedral', 'r'), 0.0),
                        ((6, 'variants', 'tetrahedral', 'theta0'), 181.0), ((6, 'x'), float('nan')), ((6, 'D'), -1.0), ((6, 'Z'), 0.0), ((6, 'chi'), 0.0),
                        ((6, 'V'), -1.0), ((6, 'K_inv'), 1e4), ((6, 'variants', 'square'), {'r': 1.0, 'theta0': 90.0}),
                        ((1, 'variants', 'linear'), {'r': 0.3, 'theta0': 180.0})):
        with pytest.raises(ValueError):
            R.ForceFieldTables(table=changed(path, value))
    with pytest.raises(ValueError):
        R.ForceFieldTables(atomic_numbers=(6, 35))
    c = RC.named()['ethane']
    for kw in (dict(gtol=0.0), dict(gtol=float('nan')), dict(max_iters=-1), dict(max_iters=100001), dict(max_step=0.0), dict(deg_tol=1.0)):
        with pytest.raises(ValueError):
            R.relax_ref(*c, **kw)
    with pytest.raises(ValueError):
        R.relax_ref(c[0], c[1][:0], *c[2:])


def test_no_decision_of_the_seeded_sets_is_near_its_threshold():
    """the GPU tests may leave out at most 10 % of a set for near-threshold decisions; the reference alone leaves out none"""
    for max_iters in (0, 5, 200):
        for m, (_, trace) in enumerate(RC.refs(max_iters)):
            close = [(k, v, th) for k, v, th in trace if math.isfinite(v) and abs(v - th) <= 1e-9 * max(abs(v), abs(th), 1e-300 if th else 1.0)]
            assert not close, (max_iters, m, close[:3])
    assert not R.near_threshold(*RC.named()['formamide'], max_iters=5)


def test_summary_and_compare():
    cases = RC.all_cases()
    res = R._stack([r for r, _ in RC.refs(200)])
    s = R.summary(res)
    assert s['n_molecules'] == len(cases) and s['n_measured'] == len(cases) - 1 and s['n_too_large'] == 0
    assert abs(s['fraction_converged'] + s['fraction_maxiter'] + s['fraction_linesearch'] - 1.0) < 1e-12 and s['fraction_nonfinite'] == 1 / len(cases)
    assert sum(s['strain_hist']) == s['n_measured'] == sum(s['rmsd_heavy_hist']) and s['strain_median'] >= 0.0
    assert set(s['components_initial']) == set(R.COMPONENTS)
    both = R.compare(res, R._stack([r for r, _ in RC.refs(5)]))
    assert both['strain'] > 0.0 and R.compare(res, res)['strain'] == 0.0 and R.compare(s, s)['rmsd_heavy'] == 0.0
    joined = R.concat([res, res])
    assert len(joined['status']) == 2 * len(cases) and joined['pos'].shape[0] == 2 * res['pos'].shape[0]
    assert np.array_equal(R.mol_result(joined, len(cases) + 3)['pos'], R.mol_result(res, 3)['pos'])


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/relax_host_check.cpp over csrc/mdx_relax_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('relax_host_check', tmp_path)
