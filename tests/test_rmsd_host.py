"""Host tests of the best RMSD: ``rmsd.best_rms_ref`` against a brute force over all atom permutations with a Kabsch of its own, its
invariances and relations at every fixture, ``conformers`` and ``global_3d`` on hand-made batches, the SDF path, the argument checks, the
header and the stand-alone host check.  No GPU."""
import os
import re

import numpy as np
import pytest

from moldiff_amd import canon as C
from moldiff_amd import rmsd as R
from .canon_cases import mol
from .rmsd_cases import brute_force, cases, flat, kabsch_3x3, neopentane, noisy, relabelled
from .stereo_cases import centre_h, moved, reflected, with_pos
from .util import run_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases()
PROBES, TARGETS, PAIRS, NAMES = flat(CASES)
REF = R.stack_ref(PROBES, TARGETS, PAIRS)            # computed once, shared, left unchanged
# numpy's SVD and the brute force's measured residual are both honest float64 evaluations: a few hundred ulp of the pair's unit
TOL = 1e-12


def rows(name):
    k = NAMES.index(name)
    return range(REF['pair_ptr'][k], REF['pair_ptr'][k + 1])


def close(a, b, unit):
    return abs(a - b) <= TOL * max(unit, 1e-300)


def test_against_the_brute_force_over_all_permutations():
    seen = 0
    for name, (probe, targets) in CASES.items():
        if len(probe['element']) > 7:
            continue
        for r, t in zip(rows(name), targets):
            msd, mirror, n_maps = brute_force(probe, t)
            assert REF['n_maps'][r] == n_maps == C.canon_ref(probe)['n_aut'], name
            assert close(REF['msd'][r], msd, REF['unit'][r]) and close(REF['msd_mirror'][r], mirror, REF['unit'][r]), (name, REF['msd'][r], msd)
            seen += 1
    assert seen >= 20
    one = R.best_rms_ref(*[CASES['six_ring_turned'][0], CASES['six_ring_turned'][1][0]])
    r = rows('six_ring_turned')[0]
    assert one['n_maps'] == 12 and one['status'] == 0 and one['msd'] == REF['msd'][r] and one['msd_first'] == REF['msd_first'][r]


def test_invariance_under_motion_relabelling_and_the_swap():
    for name in ('neopentane', 'six_ring_turned', 'butane_pp_mm', 'planar', 'collinear', 'two_atoms', 'moved_copy', 'gem_dimethyl', 'chain70'):
        probe, target = CASES[name][0], CASES[name][1][0]
        base = R.best_rms_ref(probe, target)
        # the float32 rounding of the moved coordinates is all that may differ: 1e-6 of the unit
        near = lambda a, b: abs(a - b) <= 2e-6 * base['unit']
        for k, (p, t) in enumerate(((moved(probe, 41), target), (probe, moved(target, 43)), (moved(probe, 45), moved(target, 47)))):
            got = R.best_rms_ref(p, t)
            assert got['n_maps'] == base['n_maps'] and near(got['msd'], base['msd']) and near(got['msd_mirror'], base['msd_mirror']), (name, k)
        swapped = R.best_rms_ref(target, probe)
        assert swapped['n_maps'] == base['n_maps'] and near(swapped['msd'], base['msd']) and near(swapped['msd_mirror'], base['msd_mirror']), name
        exact = R.best_rms_ref(relabelled(probe, np.roll(np.arange(len(probe['element'])), 1)), target)    # the same floats in another order
        assert close(exact['msd'], base['msd'], base['unit']) and close(exact['msd_mirror'], base['msd_mirror'], base['unit']), name


def test_the_relations_at_every_fixture():
    for name, (probe, targets) in CASES.items():
        for r, t in zip(rows(name), targets):
            if REF['pair_status'][r] != 0:
                assert name == 'over257' and REF['pair_status'][r] == 1 and REF['msd'][r] == 0 and REF['n_maps'][r] == 0
                continue
            u = REF['unit'][r]
            assert REF['msd'][r] <= REF['msd_first'][r] + TOL * u and REF['msd'][r] >= 0 and REF['msd_mirror'][r] >= 0, name
            q = R.best_rms_ref(probe, reflected(t))
            assert close(q['msd'], REF['msd_mirror'][r], u) and close(q['msd_mirror'], REF['msd'][r], u), name
    for name in ('planar', 'collinear', 'two_atoms', 'planar_symmetric'):
        for r in rows(name):
            assert close(REF['msd'][r], REF['msd_mirror'][r], REF['unit'][r]), name
    for name in ('identical', 'moved_copy'):
        r = rows(name)[0]
        assert REF['msd'][r] <= 1e-12 * REF['unit'][r] + (1e-7 if name == 'moved_copy' else 0), name     # float32 rounding of the motion
    r = rows('chfclbr_mirror')[0]
    assert REF['msd_mirror'][r] <= TOL * REF['unit'][r] and REF['msd'][r] > 0.1
    r = rows('butane_pp_mm')[0]
    assert REF['msd_mirror'][r] <= TOL * REF['unit'][r] and REF['msd'][r] > 0.5
    shuffled, plain = rows('neopentane')
    assert REF['msd_first'][shuffled] > 50 * REF['msd'][shuffled] and REF['n_maps'][shuffled] == 24
    # the permuted target holds the very points of the unpermuted one under other names: the search finds the unpermuted value
    assert close(REF['msd'][shuffled], REF['msd'][plain], REF['unit'][plain]) and REF['msd'][plain] > 1e-3
    assert len(rows('nine_targets')) == 9 and REF['n_nodes'][NAMES.index('cap256')] >= 1


def butane(dihedral):
    """C-C-C-C with the given dihedral angle in degrees"""
    a = np.deg2rad(dihedral)
    c0 = [-0.77 - 1.53 * np.cos(np.deg2rad(68.0)), 1.53 * np.sin(np.deg2rad(68.0)), 0.0]
    y, x = 1.53 * np.sin(np.deg2rad(68.0)), 0.77 + 1.53 * np.cos(np.deg2rad(68.0))
    return with_pos(mol(4, [(0, 1), (1, 2), (2, 3)]), [c0, [-0.77, 0, 0], [0.77, 0, 0], [x, y * np.cos(a), y * np.sin(a)]])


def conformer_batch_and_summary():
    """-> (the batch, its summary at tol 0.3, every integer entry derived by hand): butane anti (A) and gauche (B), three more copies of
    A in other atom orders, and CHFClBr with its mirror image"""
    A, B = butane(180.0), butane(60.0)
    chf, chf_m = centre_h(), centre_h(flip=True)
    mols = [A, B, moved(A, 1), moved(A, 2), moved(A, 3), chf, chf_m]
    # groups: the five butanes, the two CHFClBr.  Pairs: 10 + 1.  A leads; B is 0.5 A away from it: a second leader; the copies join A.
    # CHFClBr: msd 0.1875 (rmsd 0.433 > 0.3): two leaders, and its mirror value is 0: the one mirror pair.  The anti conformer is planar, so
    # both values of a butane pair agree up to the float32 rounding of the moved copies, and gauche is further than tol from anti: no
    # butane pair is a mirror pair.  Duplicates: 4 + 1, of which the three copies joined a leader.
    d_ab = np.sqrt(brute_force(A, B)[0])
    want = {'n_molecules': 7, 'n_grouped': 7, 'n_left_out': 0, 'n_groups': 2, 'n_pairs': 11, 'n_pairs_measured': 11,
            'conformers_per_group': [2, 2], 'n_duplicates': 5, 'share_geometric_duplicates': 3 / 5, 'mean_pairwise_rmsd': (4 * d_ab + np.sqrt(0.1875)) / 11,
            'n_mirror_pairs': 1, 'tol': 0.3}
    return mols, want


def test_conformers_on_a_hand_made_batch():
    mols, want = conformer_batch_and_summary()
    assert np.sqrt(brute_force(mols[0], mols[1])[0]) > 0.4
    got = R.conformers(mols, tol=0.3)
    for k, v in want.items():
        assert got[k] == (pytest.approx(v, abs=2e-6) if isinstance(v, float) else v), (k, got[k], v)
    hist = [0] * R.RMSD_BINS
    hist[0], hist[1], hist[int(np.sqrt(brute_force(mols[0], mols[1])[0]) / 0.25)] = 6, 1, 4
    assert got['rmsd_hist'] == hist and got['mean_first_minus_best'] >= 0
    capped = R.conformers(mols, tol=0.3, max_group=3)
    assert capped['n_left_out'] == 2 and capped['n_grouped'] == 5 and capped['n_pairs'] == 4 and capped['conformers_per_group'] == [2, 2]
    wide = R.conformers(mols, tol=0.5)
    assert wide['conformers_per_group'] == [2, 1] and wide['n_mirror_pairs'] == 1        # enantiomers closer than tol still count
    assert R.compare(R.conformer_results(mols, tol=0.3), R.conformer_results(mols, tol=0.3))['rmsd'] == 0.0


def test_global_3d_and_empty_inputs():
    neo = neopentane()
    targets = [noisy(neo, 1, 0.05), moved(noisy(neo, 2, 0.2), 3), noisy(neo, 4, 0.1), centre_h()]
    got = R.global_3d([neo, centre_h(flip=True), with_pos(mol([8, 8], [(0, 1)]), np.eye(3)[:2])], targets)
    d = np.sqrt([brute_force(neo, t)[0] for t in targets[:3]])
    assert got['n_matched'].tolist() == [3, 1, 0]
    assert np.allclose([got['rmsd_max'][0], got['rmsd_min'][0], got['rmsd_median'][0]], [d.max(), d.min(), np.median(d)], atol=1e-9)
    assert got['rmsd_max'][1] == pytest.approx(np.sqrt(0.1875)) and all(np.isnan(got[k][2]) for k in ('rmsd_max', 'rmsd_min', 'rmsd_median'))
    empty = R.stack_ref([], [], [])
    assert len(empty['status']) == 0 and len(empty['msd']) == 0 and empty['pair_ptr'].tolist() == [0]
    assert R.conformers([])['n_groups'] == 0 and R.global_3d([], [])['n_matched'].shape == (0,)
    s = R.summary(R.conformer_results([neo]))
    assert s['n_pairs'] == 0 and np.isnan(s['mean_pairwise_rmsd']) and s['conformers_per_group'] == []
    b = R.between([neo, centre_h(), neo], [noisy(neo, 1), neo])
    assert b['n_compared'] == 2 and b['share_same_constitution'] == 0.5 and b['max_rmsd'] == pytest.approx(np.sqrt(brute_force(neo, noisy(neo, 1))[0]))


def test_value_errors():
    neo, chf = neopentane(), centre_h()
    with pytest.raises(ValueError, match='certificates'):
        R.best_rms_ref(neo, chf)
    with pytest.raises(ValueError, match='certificates'):
        R.stack_ref([neo], [chf], [(0, 0)])
    with pytest.raises(ValueError, match='tol'):
        R.conformers([neo], tol=-0.1)
    with pytest.raises(ValueError, match='tol'):
        R.conformers([neo], tol=float('nan'))
    for bad in ([(1, 0)], [(0, 1)], [(-1, 0)]):
        with pytest.raises(ValueError, match='out of range'):
            R.stack_ref([neo], [neo], bad)
    with pytest.raises(ValueError, match='max_nodes'):
        R.best_rms_ref(neo, neo, max_nodes=0)
    with pytest.raises(ValueError, match='atom_pos'):
        R.best_rms_ref(mol(2, [(0, 1)]), mol(2, [(0, 1)]))
    with pytest.raises(ValueError, match='max_group'):
        R.conformers([neo], max_group=0)
    assert R.best_rms_ref(neo, neo, max_nodes=5)['status'] == 1          # canon itself gave up: no canonical form
    assert R.probe_ref(neo, C.canon_ref(neo), [np.zeros((5, 3))], max_nodes=5)['pair_status'].tolist() == [2]
    assert R.probe_ref(neo, C.canon_ref(neo), [np.zeros((4, 3))])['pair_status'].tolist() == [3]


SDF = """
  made by hand

  6  5  0  0  0  0  0  0  0  0999 V2000
    0.0000    0.0000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0
    0.8660    0.8660    0.8660 F   0  0  0  0  0  0  0  0  0  0  0  0
    0.6300   -0.6300   -0.6300 H   0  0  0  0  0  0  0  0  0  0  0  0
    0.8660   -0.8660   -0.8660 Cl  0  0  0  0  0  0  0  0  0  0  0  0
   -0.8660    0.8660   -0.8660 C   0  0  0  0  0  0  0  0  0  0  0  0
   -0.6300   -0.6300    0.6300 H   0  0  0  0  0  0  0  0  0  0  0  0
  1  2  1  0
  1  3  1  0
  1  4  1  0
  1  5  1  0
  1  6  1  0
M  END
$$$$
"""


def test_the_sdf_path_drops_hydrogens_and_the_command_line(tmp_path, capsys):
    import torch
    from moldiff_amd.molpack import load_npz
    path = tmp_path / 'conf.sdf'
    path.write_text(SDF.lstrip('\n') + SDF.lstrip('\n'))
    read = R.read_sdf(str(path))
    assert len(read) == 2 and read[0]['element'].tolist() == [6, 9, 17, 6] and read[0]['bond_index'][:, :3].tolist() == [[0, 0, 0], [1, 2, 3]]
    assert np.allclose(read[0]['atom_pos'][2], [0.866, -0.866, -0.866])
    chf = centre_h()
    torch.save({'finished': [chf, neopentane()]}, tmp_path / 'samples_all.pt')
    assert R.main(['against', str(tmp_path / 'samples_all.pt'), '--sdf', str(path), '--out', str(tmp_path / 'g.npz'), '--ref']) == 0
    g = load_npz(tmp_path / 'g.npz')
    assert g['n_matched'].tolist() == [2, 0] and g['rmsd_max'][0] == pytest.approx(np.sqrt(brute_force(chf, read[0])[0]), abs=1e-9)
    mols, want = conformer_batch_and_summary()
    torch.save({'finished': mols}, tmp_path / 'a.pt')
    assert R.main(['stats', str(tmp_path / 'a.pt'), '--out', str(tmp_path / 'a.npz'), '--tol', '0.3', '--ref']) == 0
    assert R.summary(load_npz(tmp_path / 'a.npz'))['conformers_per_group'] == want['conformers_per_group']
    assert R.main(['compare', str(tmp_path / 'a.npz'), str(tmp_path / 'a.npz')]) == 0
    assert R.main(['between', str(tmp_path / 'a.pt'), str(tmp_path / 'a.pt'), '--ref']) == 0
    assert '"share_same_constitution": 1.0' in capsys.readouterr().out


def test_the_entry_point_is_declared_and_registered():
    from moldiff_amd import _lib
    with open(os.path.join(ROOT, 'include', 'moldiff_hip.h')) as f:
        hdr = f.read()
    proto = re.search(r'\bint mdx_mol_bestrms\(([^;]*)\);', hdr).group(1)
    params = [p.strip() for p in proto.split(',')]
    assert len(params) == 30 and params[-1] == 'void* stream' and '#define MDX_BESTRMS_STATS 3' in hdr and len(R.STAT_KEYS) == 3
    assert 'NO CONFORMER GENERATION' in hdr and 'sign(det H) s3' in hdr and 'mdx_mol_bestrms' in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert hasattr(L, 'mdx_mol_bestrms') and len(L.mdx_mol_bestrms.argtypes) == 30


def test_host_validation_and_the_solver_under_the_host_sanitizers(tmp_path):
    """tools/bestrms_host_check.cpp over csrc/mdx_bestrms_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('bestrms_host_check', tmp_path)
