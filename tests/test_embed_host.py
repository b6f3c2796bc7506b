"""CPU tests of the conformer-generation restatement (moldiff_amd/embed.py: bounds_ref, embed_ref): the properties the bounds and the
minimisation must have whatever the device does.  The triangle inequality is asked for to 1e-12 relative: a smoothed entry is a
left-to-right sum of at most 255 rounded additions (255 x 1.1e-16 = 3e-14), a margin of 30."""
import numpy as np

from moldiff_amd import embed as E
from moldiff_amd import relax, rmsd
from . import embed_cases as EC
from . import philox_ref
from . import relax_cases as RC
from .util import run_host_check

TRI_TOL = 1e-12


def test_smoothed_bounds_satisfy_the_triangle_inequality_on_every_triple():
    names, _ = EC.named_lists()
    for name, b in zip(names, EC.bounds()):
        assert b['status'] == E.STATUS_OK, name
        L, U = b['lower'], b['upper']
        assert np.array_equal(L, L.T) and np.array_equal(U, U.T) and not L.diagonal().any() and not U.diagonal().any(), name
        assert (L <= U).all() and (L >= 0).all() and (U <= b['upper0']).all() and (L >= b['lower0']).all(), name
        via = U[:, :, None] + U[None, :, :]          # via[i, k, j] = U[i, k] + U[k, j]
        assert (U[:, None, :] <= via * (1.0 + TRI_TOL)).all(), name
        low = L[:, :, None] - U[None, :, :]          # low[i, k, j] = L[i, k] - U[k, j]
        assert (L[:, None, :] >= low - TRI_TOL * np.abs(U).max()).all(), name


def test_pair_counts_equal_the_topology_counts_of_relax_where_the_definitions_coincide():
    cases = EC.named()
    for name in EC.ACYCLIC + ('benzene',):
        c = cases[name]
        b = E.bounds_ref(c[0], c[1], c[2], c[4])
        ev = relax.energy_ref(*c)
        assert b['n_all'] == ev['n_all'] and b['n_12'] == ev['counts'][0] and b['n_13'] == ev['counts'][1], (name, b['n_12'], b['n_13'], ev['counts'])
    for name in ('ethane', 'propane'):                                  # every quadruple of a staggered alkane contributes a torsion
        c = cases[name]
        assert E.bounds_ref(c[0], c[1], c[2], c[4])['n_14'] == relax.energy_ref(*c)['counts'][2], name


def test_ring_angles_are_substituted_on_the_four_rings():
    cases = EC.named()
    want = {'cyclopropane': 3, 'cyclobutane': 4, 'cyclopentane': 5, 'benzene': 0, 'propane': 0}
    for name, n in want.items():
        c = cases[name]
        b = E.bounds_ref(c[0], c[1], c[2], c[4])
        assert b['n_ring_angles'] == n and b['status'] == E.STATUS_OK, (name, b['n_ring_angles'])
    c = cases['cyclobutane']
    b = E.bounds_ref(c[0], c[1], c[2], c[4])
    tb = relax.ForceFieldTables()
    r = tb.pair(tb.type_of[0, 0][0], tb.type_of[0, 0][0], 0)[0]
    diagonal = E._b13(r, r, E.RING_C0[1])                                # 90 degrees, not the tetrahedral angle
    assert b['cls'][0, 2] == E.P13 and b['lower0'][0, 2] == diagonal - E.DEFAULT_TOL13 and b['upper0'][0, 2] == diagonal + E.DEFAULT_TOL13


def test_an_absurd_radius_gives_inconsistent_bounds_and_no_conformer():
    c = EC.inconsistent()
    assert E.bounds_ref(c[0], c[1], c[2], c[4])['status'] == E.STATUS_OK
    b = E.bounds_ref(c[0], c[1], c[2], c[4], EC.absurd_tables())
    assert b['status'] == E.STATUS_INCONSISTENT
    r = E.embed_ref(b)
    assert r['status'] == E.STATUS_INCONSISTENT and r['attempts'] == 0 and not r['pos'].any()
    big = RC.ladder()[-1]
    assert E.bounds_ref(big[0], big[1], big[2], big[4])['status'] == E.STATUS_TOO_LARGE
    small = EC.named()['propane']
    assert E.bounds_ref(small[0], small[1], small[2], small[4], na_cap=10)['status'] == E.STATUS_TOO_LARGE


def test_philox_restatement_equals_the_reference_of_the_noise_tests():
    ctr = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [0xFFFFFFFF, 7, 0xDEADBEEF, 0x80000001], [12345, 2, 99, (5 << 8) | 3]], dtype=np.uint32)
    for k0, k1 in ((0, 0), (20241021, 0), (0x9ABCDEF0, 0x12345678)):
        want = philox_ref.philox4x32_10(ctr, k0, k1)
        for row, w in zip(ctr.tolist(), want.tolist()):
            assert list(E.philox4x32_10(row, k0, k1)) == w
    assert E.u53(0, 0) == 0.0 and E.u53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 and E.u53(1 << 31, 0) == 0.5
    x = E.start_coords(5, 8.0, 7, 3, 1, 0)
    assert (np.abs(x) <= 4.0).all() and len(np.unique(x)) == 20 and not np.array_equal(x, E.start_coords(5, 8.0, 7, 3, 1, 1))


def test_full_length_runs_reach_ok_within_the_violation_tolerance_and_never_go_uphill():
    names, _ = EC.named_lists()
    for name, b, row in zip(names, EC.bounds(), EC.refs(E.DEFAULT_MAX_ITERS)):
        for c, (r, _) in enumerate(row):
            assert r['status'] == E.STATUS_OK and r['max_violation'] <= E.DEFAULT_VIOL_TOL, (name, c, r['status'], r['max_violation'])
            h = b['h']
            assert E.violation_ref(E.allatom(r['pos'], r['h_pos'], h), b) == r['max_violation']
            assert r['iterations_a'] + r['iterations_b'] == len(r['errors'])
            a = r['errors'][:r['iterations_a']]
            bb = r['errors'][r['iterations_a']:]
            assert all(y <= x for x, y in zip(a, a[1:])) and all(y <= x for x, y in zip(bb, bb[1:])), (name, c)


def test_the_gradient_equals_a_central_difference_of_the_error():
    h = 1e-5
    for name in ('propane', 'formamide', 'cyclobutane'):
        case = EC.named()[name]
        b = E.bounds_ref(case[0], case[1], case[2], case[4])
        x = E.start_coords(b['n_all'], 6.0, 11, 0, 0, 0)
        for w4 in (E.W4_A, E.W4_B):
            _, g, _ = E.error_ref(x, b['lower'], b['upper'], w4)
            scale = np.abs(g).max()
            for a in range(b['n_all']):
                for k in range(4):
                    xp, xm = x.copy(), x.copy()
                    xp[a, k] += h
                    xm[a, k] -= h
                    fd = (E.error_ref(xp, b['lower'], b['upper'], w4)[0] - E.error_ref(xm, b['lower'], b['upper'], w4)[0]) / (2.0 * h)
                    assert abs(fd - g[a, k]) <= 1e-6 * scale, (name, w4, a, k, fd, g[a, k])


def test_no_case_is_near_a_threshold_at_the_caps_the_device_test_uses():
    for max_iters in (5, 50):
        for m, (b, row) in enumerate(zip(EC.bounds(), EC.refs(max_iters))):
            for c, (_, trace) in enumerate(row):
                assert not E.near_threshold(b, trace=trace), (max_iters, m, c)


def test_the_statistics_over_conformers_equal_those_of_global_3d():
    rng = np.random.default_rng(5)
    msd = rng.uniform(0.0, 4.0, size=(4, 5))
    ok = rng.uniform(size=(4, 5)) < 0.7
    ok[2] = False
    got = E.spread(msd, ok)
    pairs = dict(msd=msd.reshape(-1), pair_status=np.where(ok.reshape(-1), rmsd.STATUS_OK, 1).astype(np.int32), pair_ptr=np.arange(5) * 5)
    want = rmsd._spread(pairs, 4)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.isnan(got['rmsd_max'][2]) and got['n_matched'][2] == 0
    d = np.sqrt(msd[0][ok[0]])
    assert got['rmsd_max'][0] == d.max() and got['rmsd_min'][0] == d.min() and got['rmsd_median'][0] == np.median(d)


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/embed_host_check.cpp over csrc/mdx_embed_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('embed_host_check', tmp_path)
