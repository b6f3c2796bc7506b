"""GPU tests of the best RMSD: ``mdx_mol_bestrms`` through ``rmsd.pairs_mols`` / ``launch`` / ``conformers`` against the host
restatement.  The integer columns are compared exactly; the three float columns as mean squared deviations in the unit (Ga + Gb) / n
of the pair, to 16 times the figure of profiles/bestrms_accuracy.txt (numpy's SVD against a float64 restatement of the device's sums and
solver, measured on the CPU by tools/bestrms_accuracy.py).  No pair is left out of any comparison."""
import json
import os
import re

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import canon as C
from moldiff_amd import rmsd as R
from moldiff_amd.postprocess import FeaturizeMol
from .canon_cases import ELEMENTS, mol
from .rmsd_cases import cases, flat, moved, neopentane, noisy, random_batch
from .stereo_cases import with_pos

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
# the summaries hold roots: a difference d between two mean squared deviations moves the root by at most sqrt(d), and d is at most the
# tolerance of the float columns (below 1e-14) times the pair's unit, which is below 100 A^2 for every molecule here: below 1e-6 A
ROOT_TOL = 1e-6
INT_KEYS = ('status', 'n_nodes', 'n_aut', 'n_atoms', 'n_maps', 'pair_status', 'pair_target', 'pair_ptr')


def tolerance():
    with open(os.path.join(ROOT, 'profiles', 'bestrms_accuracy.txt')) as f:
        figure = float(re.search(r'max_abs_difference_in_unit (\S+)', f.read()).group(1))
    tol = 16.0 * figure
    assert 0.0 < tol < 1e-10, tol
    return tol


def same(got, ref, what):
    """every integer column exactly, every float column of every pair within the tolerance in the pair's unit"""
    got = molpack.to_host(got)
    for k in INT_KEYS:
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    tol = tolerance()
    unit = np.where(ref['unit'] > 0, ref['unit'], 1.0)
    for k in R.FLOAT_KEYS:
        assert got[k].dtype == np.float64 and got[k].shape == ref[k].shape, (what, k)
        d = np.abs(got[k] - ref[k]) / unit
        print('%s %s: largest difference %.3e of %.3e allowed' % (what, k, d.max() if len(d) else 0.0, tol))
        assert np.isfinite(got[k]).all() and (d <= tol).all(), (what, k, int(d.argmax()), float(d.max()), tol)


def test_the_fixtures_an_empty_and_a_one_atom_molecule_as_one_batch():
    table = dict(cases())
    table['empty'] = (with_pos(mol([], []), np.zeros((0, 3))), [with_pos(mol([], []), np.zeros((0, 3)))])
    table['one_atom'] = (with_pos(mol([8], []), [[1.0, 2.0, 3.0]]), [with_pos(mol([8], []), [[-4.0, 0.0, 1.0]])])
    probes, targets, pairs, names = flat(table)
    ref = R.stack_ref(probes, targets, pairs)
    assert ref['status'][names.index('over257')] == 1 and ref['n_aut'][names.index('neopentane')] == 24
    assert ref['n_aut'][names.index('six_ring_turned')] == 12 and ref['n_atoms'][names.index('cap256')] == 256
    same(R.pairs_mols(probes, targets, pairs, DEV), ref, 'fixtures')


def test_a_random_batch_and_the_place_in_the_batch():
    probes, targets, pairs, _ = flat(random_batch())
    ref = R.stack_ref(probes, targets, pairs)
    assert (ref['pair_status'] == 0).all() and ref['n_aut'].max() >= 2 and len(pairs) == 128
    got = molpack.to_host(R.pairs_mols(probes, targets, pairs, DEV))
    same(got, ref, 'random')
    # the same probe first and last: bit-identical rows (neopentane with nine targets: three rounds of the four waves)
    neo, tg = cases()['nine_targets']
    probes2, pairs2 = [neo] + probes + [neo], [(0, k) for k in range(9)] + [(m + 1, j + 9) for m, j in pairs] + [(len(probes) + 1, k) for k in range(9)]
    again = molpack.to_host(R.pairs_mols(probes2, tg + targets, pairs2, DEV))
    for k in R.FLOAT_KEYS + ('n_maps', 'pair_status'):
        assert again[k][:9].tobytes() == again[k][-9:].tobytes(), k
        assert again[k][9:-9].tobytes() == got[k].tobytes(), k
    assert again['n_maps'][:9].tolist() == [24] * 9 and (again['msd'][:9] > 0).all()


def _packed(mols):
    p = molpack.pack_mols(mols, ELEMENTS, positions=True)
    return p, molpack.CompactMols.from_packed(molpack.to_device(p, DEV))


def test_select_the_three_statuses_and_no_pairs():
    neo = neopentane()
    probes = [neo, cases()['chfclbr_mirror'][0], cases()['butane_pp_mm'][0], cases()['gem_dimethyl'][0]]
    targets = [noisy(neo, 1), cases()['chfclbr_mirror'][1][0], cases()['butane_pp_mm'][1][0], cases()['gem_dimethyl'][1][0],
               with_pos(mol(4, [(0, 1), (0, 2), (0, 3)]), np.arange(12).reshape(4, 3))]
    pairs = [(0, 0), (0, 0), (1, 1), (3, 3), (3, 4)]          # probe 2 has no pair; the last target has one atom fewer than its probe
    ref = R.stack_ref(probes, targets, pairs, check=False)
    assert ref['pair_status'].tolist() == [0, 0, 0, 0, 3] and ref['pair_ptr'].tolist() == [0, 2, 3, 3, 5]
    same(R.pairs_mols(probes, targets, pairs, DEV, check=False), ref, 'status 3 and a probe without pairs')
    with pytest.raises(ValueError, match='certificates'):
        R.pairs_mols(probes, targets, pairs, DEV)
    p, cm = _packed(probes)
    t = C.canon_mols(targets, DEV)
    ptr, tgt = (torch.from_numpy(ref[k]).to(DEV) for k in ('pair_ptr', 'pair_target'))
    full = lambda out: dict(out, n_atoms=cm.n_atoms)

    def blank(m, status):
        out = {k: v.copy() for k, v in ref.items()}
        a, b = ref['pair_ptr'][m], ref['pair_ptr'][m + 1]
        for k in R.FLOAT_KEYS + ('n_maps',):
            out[k][a:b] = 0
        out['pair_status'][a:b] = status
        out['status'][m], out['n_nodes'][m], out['n_aut'][m] = status, 0, 0
        return out
    # select: the masked probe has status 0 and zeros
    select = torch.tensor([0, 1, 1, 1], dtype=torch.int32, device=DEV)
    same(full(R.launch(cm, C.launch(cm, select=select), t, ptr, tgt, select=select)), blank(0, 0), 'select')
    # canon gave up on neopentane (41 nodes) with a budget of 5: status 1 here, and the same from the restatement
    c5 = C.launch(cm, max_nodes=5)
    assert c5['status'].tolist() == [2, 0, 0, 0]
    same(full(R.launch(cm, c5, t, ptr, tgt)), blank(0, 1), 'status 1')
    same(R.stack_ref(probes, targets, pairs, canon_probes=C.stack_ref(probes, max_nodes=5), check=False), blank(0, 1), 'status 1 on the host')
    # its own budget below canon's: status 2
    same(full(R.launch(cm, C.launch(cm), t, ptr, tgt, max_nodes=5)), blank(0, 2), 'status 2')
    same(R.stack_ref(probes, targets, pairs, max_nodes=5, canon_probes=C.stack_ref(probes), canon_targets=C.stack_ref(targets), check=False),
         blank(0, 2), 'status 2 on the host')
    # no molecule, no pair
    got = molpack.to_host(R.pairs_mols([], [], [], DEV))
    want = R.stack_ref([], [], [])
    assert all(got[k].shape == want[k].shape for k in INT_KEYS + R.FLOAT_KEYS)
    got = molpack.to_host(R.pairs_mols(probes, targets, [], DEV))
    assert got['status'].tolist() == [0, 0, 0, 0] and got['n_aut'].tolist() == [24, 1, 2, 2] and len(got['msd']) == 0


def test_memory_guards_and_argument_errors():
    L = _lib.lib()
    neo = neopentane()
    probes = [cases()['chfclbr_mirror'][0], neo, neo]
    targets = [cases()['chfclbr_mirror'][1][0], noisy(neo, 1), noisy(neo, 2)]
    ref = R.stack_ref(probes, targets, [(0, 0), (1, 1), (1, 2), (2, 1)])
    p, cm = _packed(probes)
    N = int(p['n_atoms'].sum())
    c, t = C.launch(cm), C.canon_mols(targets, DEV)
    rank, cstat, tpos = c['rank'].contiguous(), c['status'].contiguous(), t['canon_pos'].contiguous()
    ROWS = 8                                                       # the pair arrays hold 8 rows, the list fills 4
    ptr = torch.tensor([0, 1, 3, 4], dtype=torch.int32, device=DEV)
    tgt = torch.tensor([0, 1, 2, 1, 99, 99, 99, 99], dtype=torch.int32, device=DEV)

    def fresh():
        o = {k: torch.full((ROWS,), 7.0, dtype=torch.float64, device=DEV) for k in R.FLOAT_KEYS}
        return dict(o, pair_stats=torch.full((ROWS, 2), 7, dtype=torch.int32, device=DEV), mol_stats=torch.full((3, 3), 7, dtype=torch.int32, device=DEV))
    outs = R.FLOAT_KEYS + ('pair_stats', 'mol_stats')

    def call(o, cm=cm, B=3, ptr=ptr, rows=ROWS, T=3, atoms=None, nodes=1 << 16, null=()):
        ops, at = cm.operands()
        q = lambda name, x: None if name in null else at(x)
        return L.mdx_mol_bestrms(B, *ops[1:], None, q('atom_pos', cm.atom_pos), None, q('rank', rank), q('canon_status', cstat), q('pair_ptr', ptr),
                                 q('pair_target', tgt), rows, T, q('tgt_ptr', t['atom_ptr']), q('tgt_n', t['n_atoms']), q('tgt_pos', tpos),
                                 int(tpos.shape[0]) if atoms is None else atoms, nodes, *(q(k, o[k]) for k in outs), _lib.stream())
    # argument errors leave every output untouched
    o = fresh()
    for name in ('atom_pos', 'rank', 'canon_status', 'pair_ptr', 'pair_target', 'tgt_ptr', 'tgt_n', 'tgt_pos') + outs:
        assert call(o, null=(name,)) == 1 and b'null' in L.mdx_last_error(), name
    assert call(o, rows=-1) == 1 and call(o, T=-1) == 1 and call(o, atoms=-1) == 1 and call(o, B=-1) == 1
    assert call(o, nodes=0) == 1 and b'max_nodes' in L.mdx_last_error() and call(o, nodes=(1 << 20) + 1) == 1
    assert call(o, rows=1 << 31) == 1 and call(o, B=0) == 0
    torch.cuda.synchronize()
    assert all(bool((x == 7).all()) for x in o.values())
    # the list fills 4 of 8 rows: the rows behind it stay untouched
    assert call(o) == 0
    torch.cuda.synchronize()
    tol = tolerance()
    for k in R.FLOAT_KEYS:
        assert bool((o[k][4:] == 7).all()) and (np.abs(o[k][:4].cpu().numpy() - ref[k]) <= tol * ref['unit']).all(), k
    assert bool((o['pair_stats'][4:] == 7).all()) and o['pair_stats'][:4].tolist() == [[1, 0], [24, 0], [24, 0], [24, 0]]
    assert o['mol_stats'].tolist() == [[0, 1, 1], [0, 41, 24], [0, 41, 24]]
    # a probe whose extent leaves the atom arrays: nothing is written for it; a pair extent past the rows is no pair; a target outside
    # tgt_pos and a target index outside 0 .. T - 1 are status 3
    o = fresh()
    assert call(o, cm=cm._replace(N_cap=N - 1)) == 0
    torch.cuda.synchronize()
    assert bool((o['msd'][3:] == 7).all()) and bool((o['pair_stats'][3:] == 7).all()) and o['mol_stats'][2].tolist() == [7, 7, 7]
    assert o['pair_stats'][:3].tolist() == [[1, 0], [24, 0], [24, 0]]
    o = fresh()
    assert call(o, rows=3) == 0                                      # probe 2's pair 3 lies past the 3 rows
    torch.cuda.synchronize()
    assert bool((o['msd'][3:] == 7).all()) and o['mol_stats'].tolist() == [[0, 1, 1], [0, 41, 24], [0, 41, 24]]
    o = fresh()
    assert call(o, atoms=int(tpos.shape[0]) - 1, T=2) == 0           # target 2 ends past the atoms given and is past T as well
    torch.cuda.synchronize()
    assert o['pair_stats'][:4].tolist() == [[1, 0], [24, 0], [0, 3], [24, 0]] and float(o['msd'][2]) == 0.0
    bad = torch.tensor([0, 1, -5, 4], dtype=torch.int32, device=DEV)     # probe 1 ends before it starts, probe 2 starts below 0
    o = fresh()
    assert call(o, ptr=bad) == 0
    torch.cuda.synchronize()
    assert bool((o['msd'][1:] == 7).all()) and o['pair_stats'][0].tolist() == [1, 0] and o['mol_stats'][1].tolist() == [0, 41, 24]


def test_conformers_global_3d_and_conformer_batch():
    from .test_gpu_canon import _pred_of
    from .test_rmsd_host import conformer_batch_and_summary
    mols, want = conformer_batch_and_summary()
    got = R.conformers(mols, tol=0.3, device=DEV)
    assert {k: got[k] for k, v in want.items() if not isinstance(v, float)} == {k: v for k, v in want.items() if not isinstance(v, float)}
    host = R.conformers(mols, tol=0.3)
    assert set(got) == set(host)
    for k, v in host.items():
        assert got[k] == (pytest.approx(v, abs=ROOT_TOL, nan_ok=True) if isinstance(v, float) else v), k
    g_dev, g_host = R.global_3d(mols[:3], mols, DEV), R.global_3d(mols[:3], mols)
    for k in g_host:
        assert np.allclose(g_dev[k], g_host[k], rtol=1e-7, atol=1e-7, equal_nan=True), k       # roots of values near zero
    assert g_host['n_matched'].tolist() == [5, 5, 5]
    none = R.global_3d(mols[:1], [neopentane()], DEV)
    assert none['n_matched'].tolist() == [0] and np.isnan(none['rmsd_max'][0])
    # the decode layout: positions come from the predictions, so the reference is the host summary of the decoded list
    args = _pred_of(mols, masks=[k % 3 for k in range(len(mols))])
    decoded = FEAT.decode_batch(*args)
    got, host = FEAT.conformer_batch(*args), R.conformers(decoded)
    assert set(got) == set(host)
    for k, v in host.items():
        assert got[k] == (pytest.approx(v, abs=ROOT_TOL, nan_ok=True) if isinstance(v, float) else v), k
    select = torch.ones(len(mols), dtype=torch.int32, device=DEV)
    select[0] = 0
    masked = FEAT.conformer_batch(*args, select=select)
    assert masked['n_grouped'] == host['n_grouped'] - 1 and masked['n_molecules'] == host['n_molecules']


def test_entry_point_writes_the_conformer_files(tmp_path):
    from moldiff_amd import sample_drug3d
    run = lambda name, extra: sample_drug3d.main(
        ['--config', os.path.join(ROOT, 'configs', 'sample_MolDiff_simple.yml'), '--outdir', str(tmp_path / name), '--device', DEV,
         '--recipe-weights', '--num_steps', '2', '--num_mols', '8', '--batch_size', '8', '--largest_fragment', '0.2'] + extra)
    d0, d1 = run('abc', []), run('bca', ['--conformers', '--conformer_tol', '0.7', '--canonical_max_nodes', '500'])
    new = {'conformers.json', 'conformers.npz', 'canon.json', 'canon.npz'}
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f not in new) and new <= set(os.listdir(d1))
    pool = torch.load(os.path.join(d1, 'samples_all.pt'), weights_only=False)
    with open(os.path.join(d1, 'conformers.json')) as f:
        got = json.load(f)
    want = R.summary(R.conformer_results(pool['finished'], None, 0.7, max_nodes=500))
    assert set(got) == set(want) and got['tol'] == 0.7 and got['n_molecules'] == len(pool['finished'])
    for k, v in want.items():
        assert got[k] == (pytest.approx(v, abs=ROOT_TOL, nan_ok=True) if isinstance(v, float) else v), k
    saved = molpack.load_npz(os.path.join(d1, 'conformers.npz'))
    assert set(saved) == set(R.conformer_results([], None, 0.7)) and float(saved['tol'].reshape(-1)[0]) == 0.7
