"""Host tests of the explicit-hydrogen placement (moldiff_amd/hydrogens.py: addh_ref and everything around it).  No GPU: the plain
restatement is checked against the geometry the definition promises -- lengths, ideal angles, flags, equivariance, contacts -- and the
argument validation of the device entry runs as a stand-alone program under the host sanitizers."""
import json
import math

import numpy as np
import pytest

from moldiff_amd import hydrogens as H
from moldiff_amd import kekule as K
from moldiff_amd import molpack, rmsd
from . import hydrogens_cases as HC
from .util import run_host_check

TET = math.degrees(math.acos(-1.0 / 3.0))


def ref(name):
    info, n_h, order = HC.named()[name]
    return info, H.addh_ref(info, n_h, order)


def angle(a, b, c):
    """the angle a-b-c in degrees"""
    u, v = np.asarray(a, dtype=np.float64) - b, np.asarray(c, dtype=np.float64) - b
    return math.degrees(math.acos(max(-1.0, min(1.0, float(u @ v) / math.sqrt(float(u @ u) * float(v @ v))))))


def dihedral(a, b, c, d):
    """the dihedral a-b-c-d in degrees, in [0, 180]"""
    a, b, c, d = (np.asarray(x, dtype=np.float64) for x in (a, b, c, d))
    n1, n2 = np.cross(b - a, c - b), np.cross(c - b, d - c)
    return math.degrees(math.acos(max(-1.0, min(1.0, float(n1 @ n2) / math.sqrt(float(n1 @ n1) * float(n2 @ n2))))))


def hs(r, a):
    return [r['h_pos'][a, k] for k in range(int(r['h_count'][a]))]


def test_the_generator_keeps_clear_of_every_threshold():
    """the cap of the issue: near_threshold(band=1e-6) for at most 2 % of the 256; the seed is chosen so that it is none"""
    mols, n_h, order = HC.random_set()
    assert len(mols) == HC.RANDOM_COUNT == 256 and all(2 <= len(m['element']) <= 24 for m in mols)
    near = sum(H.near_threshold(m, h, o, band=1e-6) for m, h, o in zip(mols, n_h, order))
    assert near == 0
    r = HC.random_ref()
    assert (r['status'] == 0).all() and r['n_h_placed'].sum() > 1500 and r['n_world_frame'].sum() > 0 and r['n_clash'].sum() > 0
    flags = r['atom_flag'] & 3
    assert all((flags == g).any() for g in (H.GEOM_TETRAHEDRAL, H.GEOM_TRIGONAL, H.GEOM_LINEAR))


def test_every_placed_hydrogen_lies_at_its_table_length():
    tb = H.HydrogenTables()
    length = dict(zip(tb.atomic_numbers, tb.xh_length.tolist()))
    sets = [(m, H.mol_result(HC.named_ref(), k)) for k, m in enumerate(HC.named_lists()[1])]
    sets += [(m, H.mol_result(HC.random_ref(), k)) for k, m in enumerate(HC.random_set()[0])]
    seen = 0
    for info, r in sets:
        pos = np.asarray(info['atom_pos'], dtype=np.float32).astype(np.float64)
        for a in range(len(pos)):
            for q in hs(r, a):
                assert abs(math.dist(q, pos[a]) - length[int(info['element'][a])]) <= 1e-12
                seen += 1
            assert not r['h_pos'][a, int(r['h_count'][a]):].any()          # unplaced slots are 0
    assert seen > 2000


def test_the_ideal_angles():
    info, r = ref('methane')
    h = hs(r, 0)
    assert len(h) == 4 and all(abs(angle(h[i], info['atom_pos'][0], h[j]) - TET) < 1e-9 for i in range(4) for j in range(i))
    info, r = ref('ethane')
    for a, b in ((0, 1), (1, 0)):
        h = hs(r, a)
        assert len(h) == 3 and all(abs(angle(h[i], info['atom_pos'][a], h[j]) - TET) < 1e-9 for i in range(3) for j in range(i))
        assert all(abs(angle(q, info['atom_pos'][a], info['atom_pos'][b]) - TET) < 1e-9 for q in h)
    info, r = ref('ethene')
    for a, b in ((0, 1), (1, 0)):
        h = hs(r, a)
        assert len(h) == 2 and abs(angle(h[0], info['atom_pos'][a], h[1]) - 120.0) < 1e-9
        assert all(abs(angle(q, info['atom_pos'][a], info['atom_pos'][b]) - 120.0) < 1e-9 for q in h)
    info, r = ref('ethyne')
    assert all(abs(angle(hs(r, a)[0], info['atom_pos'][a], info['atom_pos'][1 - a]) - 180.0) < 1e-6 for a in (0, 1))
    info, r = ref('hcn')
    assert r['h_count'].tolist() == [1, 0] and abs(angle(hs(r, 0)[0], info['atom_pos'][0], info['atom_pos'][1]) - 180.0) < 1e-6
    # formamide: the mask flattens N; both N-H at 120 degrees to N-C, in the amide plane (z = 0); the first anti to O
    info, r = ref('formamide')
    assert (r['atom_flag'] & 3).tolist() == [H.GEOM_TRIGONAL] * 3
    h = hs(r, 2)
    assert len(h) == 2 and all(abs(angle(q, info['atom_pos'][2], info['atom_pos'][0]) - 120.0) < 1e-9 and abs(q[2]) < 1e-12 for q in h)
    assert abs(dihedral(info['atom_pos'][1], info['atom_pos'][0], info['atom_pos'][2], h[0]) - 180.0) < 1e-6
    assert abs(dihedral(info['atom_pos'][1], info['atom_pos'][0], info['atom_pos'][2], h[1])) < 1e-6
    # without the mask the same nitrogen is pyramidal
    n_h, order = HC.named()['formamide'][1:]
    r2 = H.addh_ref(info, n_h, order, H.HydrogenTables(planar=()))
    assert (r2['atom_flag'] & 3).tolist() == [H.GEOM_TRIGONAL, H.GEOM_TRIGONAL, H.GEOM_TETRAHEDRAL]
    assert all(abs(angle(q, info['atom_pos'][2], info['atom_pos'][0]) - TET) < 1e-9 for q in hs(r2, 2))
    # pyrrole and benzene: every X-H on the negative bisector of the ring angle, so the angles to both neighbours are equal, in plane
    for name in ('pyrrole', 'benzene', 'pyridinium'):
        info, r = ref(name)
        n = len(info['element'])
        assert r['h_count'].tolist() == [1] * n and (r['atom_flag'] & 3).tolist() == [H.GEOM_TRIGONAL] * n
        for a in range(n):
            p, q = info['atom_pos'].astype(np.float64), hs(r, a)[0]
            left, right = angle(q, p[a], p[(a - 1) % n]), angle(q, p[a], p[(a + 1) % n])
            assert abs(left - right) < 1e-9 and abs(left + right + angle(p[(a - 1) % n], p[a], p[(a + 1) % n]) - 360.0) < 1e-9 and abs(q[2]) < 1e-12
    # a methyl next to a real reference atom: the first hydrogen anti to r, the lowest-index other neighbour of the neighbour
    info, r = ref('propane')
    p = info['atom_pos']
    assert abs(dihedral(p[2], p[1], p[0], hs(r, 0)[0]) - 180.0) < 1e-6 and abs(dihedral(p[0], p[1], p[2], hs(r, 2)[0]) - 180.0) < 1e-6
    assert sorted(round(dihedral(p[2], p[1], p[0], q)) for q in hs(r, 0)) == [60, 60, 180]
    h = hs(r, 1)                                                            # the central CH2: H-C-H tetrahedral, mirror images in the CCC plane
    assert len(h) == 2 and abs(angle(h[0], p[1], h[1]) - TET) < 1e-9 and abs(h[0][2] + h[1][2]) < 1e-12 and h[0][2] > 0
    info, r = ref('isobutane')
    q = hs(r, 0)[0]
    assert all(abs(angle(q, info['atom_pos'][0], info['atom_pos'][k]) - TET) < 1e-6 for k in (1, 2, 3))
    info, r = ref('dimethylamine')                                          # d = 2, h = 1, tetrahedral: the side of u1 x u2
    assert r['h_count'].tolist() == [1, 3, 3] and (r['atom_flag'] & 3).tolist() == [0, 0, 0]
    u1, u2 = (info['atom_pos'][k].astype(np.float64) - info['atom_pos'][0] for k in (1, 2))
    assert float(np.cross(u1, u2) @ (hs(r, 0)[0] - info['atom_pos'][0])) > 0


def test_flags_and_counts_of_the_special_cases():
    stats = lambda r: [int(r[k]) for k in H.STAT_KEYS]
    for name, h in (('methane', 4), ('ammonia', 3), ('water', 2)):             # lone atoms: the world frame
        _, r = ref(name)
        assert stats(r) == [0, h, h, 0, 0, 1, 0] and r['atom_flag'].tolist() == [H.FLAG_WORLD_FRAME] and r['min_contact'] == math.inf
    _, r = ref('ethane')                                                        # neither carbon has a reference atom
    assert stats(r) == [0, 6, 6, 0, 0, 2, 0] and r['atom_flag'].tolist() == [H.FLAG_WORLD_FRAME] * 2
    _, r = ref('flat_ch')
    assert stats(r) == [0, 10, 9, 0, 1, 0, 0] and r['atom_flag'].tolist() == [H.FLAG_DEGENERATE, 0, 0, 0] and r['h_count'].tolist() == [0, 3, 3, 3]
    _, r = ref('collinear_ch2')                                                 # and the ends find no reference that is not collinear
    assert stats(r) == [0, 8, 6, 0, 1, 2, 0] and r['atom_flag'].tolist() == [H.FLAG_DEGENERATE, H.FLAG_WORLD_FRAME, H.FLAG_WORLD_FRAME]
    _, r = ref('no_room')
    assert stats(r) == [0, 13, 12, 1, 0, 0, 0] and r['atom_flag'].tolist() == [H.FLAG_NO_ROOM, 0, 0, 0, 0] and r['h_count'][0] == 0
    _, r = ref('clamped')
    assert stats(r) == [0, 4, 4, 0, 0, 1, 0] and r['atom_flag'].tolist() == [H.FLAG_CLAMPED | H.FLAG_WORLD_FRAME]
    _, r = ref('coincident')
    assert stats(r) == [0, 6, 0, 0, 2, 0, 0] and r['atom_flag'].tolist() == [H.FLAG_DEGENERATE] * 2 and not r['h_pos'].any()
    _, r = ref('bad_bond')                                                      # the bond to atom 5 of a two-atom molecule is ignored
    _, e = ref('ethane')
    assert stats(r) == stats(e) and r['h_count'].tolist() == [3, 3]
    info, n_h, order = HC.named()['ethane']
    assert H.addh_ref(info, [-2, 9], order)['atom_flag'].tolist() == [H.FLAG_CLAMPED, H.FLAG_CLAMPED | H.FLAG_NO_ROOM]
    assert H.addh_ref(info, n_h, [0])['h_count'].tolist() == [3, 3]            # order 0 on a valid bond counts as 1
    big = H.addh_ref(HC.chain(257), np.zeros(257), np.ones(256))
    assert big['status'] == H.STATUS_TOO_LARGE and not big['h_pos'].any() and big['min_contact'] == 0.0
    with pytest.raises(ValueError, match='one count per atom'):
        H.addh_ref(info, [3], order)


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_rotation_and_translation_equivariance_in_float64():
    """float64 positions on the host: rounding at coordinate scale <= 1e2, amplified by at most 1 / deg_tol: 1e-9 Angstrom"""
    rng = np.random.default_rng(5)
    mols, n_h, order = HC.random_set()
    ref_all, used = HC.random_ref(), 0
    for k, info in enumerate(mols):
        r = H.mol_result(ref_all, k)
        if r['n_world_frame']:
            continue
        R, t = _rotation(rng), rng.normal(0.0, 10.0, size=3)
        p64 = info['atom_pos'].astype(np.float64)
        r0 = H.addh_ref(dict(info, atom_pos=p64), n_h[k], order[k])
        r1 = H.addh_ref(dict(info, atom_pos=p64 @ R.T + t), n_h[k], order[k])
        assert np.array_equal(r0['h_count'], r['h_count']) and np.array_equal(r1['h_count'], r['h_count']) and np.array_equal(r1['atom_flag'], r['atom_flag'])
        placed = np.arange(H.MAX_H)[None, :] < r['h_count'][:, None]
        assert np.abs((r0['h_pos'] @ R.T + t) - r1['h_pos'])[placed].max(initial=0.0) <= 1e-9
        assert r0['n_clash'] == r1['n_clash'] and (r0['min_contact'] == r1['min_contact'] or abs(r0['min_contact'] - r1['min_contact']) <= 1e-9)
        used += 1
    assert used >= 200


def test_contacts_of_ethane_and_the_brute_force_count():
    # Both carbons of ethane take the same world axis as their reference, so by the placement rule the two methyls face each other:
    # the shortest 1-4 H...H pair has dihedral 0 and length D - 2 L cos(theta), from the same length and angle
    info, r = ref('ethane')
    L, D = 1.09, 1.5
    assert abs(r['min_contact'] - (D + 2.0 * L / 3.0)) <= 1e-12 and r['n_clash'] == 0
    n_h, order = HC.named()['ethane'][1:]
    # the pairs: the 9 H...H across the bond and nothing else; H to the far carbon is a 1-3 pair and H to its own carbon a 1-2 pair
    trace = []
    H.addh_ref(info, n_h, order, trace=trace)
    lengths = sorted(v for kind, v in trace if kind == 'contact')
    along, across = D + 2.0 * L / 3.0, L * H.SIN_TET                            # the offset along the bond, the distance from the axis
    gauche = math.sqrt(along ** 2 + 3.0 * across ** 2)                          # dihedral 120 degrees: the chord is sqrt(3) times the radius
    assert len(lengths) == 9 and all(abs(v - along) <= 1e-12 for v in lengths[:3]) and all(abs(v - gauche) <= 1e-12 for v in lengths[3:])
    assert H.addh_ref(info, n_h, order, clash_tol=2.3)['n_clash'] == 3 and H.addh_ref(info, n_h, order, clash_tol=3.0)['n_clash'] == 9
    # brute force on the random set: all atoms, all pairs with an H, minus parent, parent's neighbours, parent's other hydrogens
    mols = HC.random_set()[0]
    for k, m in enumerate(mols):
        r = H.mol_result(HC.random_ref(), k)
        pos = m['atom_pos'].astype(np.float64)
        n, nb = len(pos), m['bond_index'].shape[1] // 2
        bonded = {(int(i), int(j)) for i, j in m['bond_index'].T}
        atoms = [(a, None, pos[a]) for a in range(n)] + [(a, x, r['h_pos'][a, x]) for a in range(n) for x in range(int(r['h_count'][a]))]
        count, shortest = 0, math.inf
        for x in range(len(atoms)):
            for y in range(x + 1, len(atoms)):
                (a, ka, pa), (b, kb, pb) = atoms[x], atoms[y]
                if ka is None and kb is None:
                    continue
                if a == b or ((ka is None or kb is None) and (a, b) in bonded):
                    continue
                dist = math.dist(pa, pb)
                count += dist < H.DEFAULT_CLASH_TOL
                shortest = min(shortest, dist)
        assert count == r['n_clash'] and (shortest == r['min_contact'] or abs(shortest - r['min_contact']) <= 1e-12), k


def test_sdf_round_trip_and_the_block_counts(tmp_path):
    names, mols, n_h, order = HC.named_lists()
    pick = [names.index(k) for k in ('formamide', 'benzene', 'pyrrole', 'propane', 'flat_ch', 'no_room', 'hcn')] + [None]
    some = [mols[k] for k in pick[:-1]] + [K_UNSOLVED]
    kek = K.stack_ref(some)
    h = H.stack_ref(some)
    assert K.kekulizable(kek).tolist() == [True] * 7 + [False]
    path = str(tmp_path / 'allatom.sdf')
    assert H.write_sdf(path, some, kek, h) == 7                                 # the unsolved ring is skipped
    back = rmsd.read_sdf(path)                                                   # strips the hydrogens again
    assert len(back) == 7
    with open(path) as f:
        blocks = [b for b in f.read().split('$$$$\n') if b.strip()]
    for k, (b, m) in enumerate(zip(blocks, some)):
        r, kr = H.mol_result(h, k), K.mol_result(kek, k)
        n, nb, placed = len(m['element']), m['bond_index'].shape[1] // 2, int(r['n_h_placed'])
        lines = b.splitlines()
        assert (int(lines[3][0:3]), int(lines[3][3:6])) == (n + placed, nb + placed)
        assert [ln[31:34].strip() for ln in lines[4:4 + n + placed]].count('H') == placed
        parents = [int(ln[0:3]) - 1 for ln in lines[4 + n + placed + nb:4 + n + 2 * placed + nb]]
        assert parents == [a for a in range(n) for _ in range(int(r['h_count'][a]))]
        assert np.array_equal(back[k]['element'], m['element']) and np.array_equal(back[k]['bond_index'], m['bond_index'])
        assert back[k]['bond_type'][:nb].tolist() == kr['kek_order'].tolist()
        assert np.abs(back[k]['atom_pos'] - m['atom_pos']).max() <= 5.1e-5       # the four decimals of the block
    r = H.mol_result(h, 4)
    assert r['n_h_placed'] < r['n_h_wanted']                                     # unplaced hydrogens: still written, and counted
    s = H.summary(h)
    assert s['n_molecules'] == 8 and 0 < s['fraction_fully_hydrogenated'] < 1 and s['fraction_degenerate'] > 0
    json.dumps(s)


K_UNSOLVED = HC.mol([6] * 5, HC._ring(5, 1.25), HC._cycle(5, HC.AROMATIC))     # the all-carbon aromatic 5-ring: no Kekulé structure


def test_summary_compare_concat_and_the_command_line(tmp_path):
    import torch
    names, mols, n_h, order = HC.named_lists()
    full = HC.named_ref()
    s = H.summary(full)
    assert s['n_molecules'] == len(mols) and s['n_measured'] == len(mols) and sum(s['min_contact_hist']) == s['n_with_contact']
    assert s['n_with_contact'] == int(np.isfinite(full['min_contact']).sum()) and s['fraction_world_frame'] > 0 and s['fraction_no_room'] > 0
    assert abs(s['mean_hydrogens'] - full['n_h_placed'].sum() / len(mols)) < 1e-12
    parts = [H.stack_ref(mols[:5], n_h[:5], order[:5]), H.stack_ref(mols[5:], n_h[5:], order[5:])]
    joined = H.concat(parts)
    assert set(joined) == set(full) and all(np.array_equal(joined[k], full[k]) and joined[k].dtype == full[k].dtype for k in full)
    e = H.empty()
    assert set(e) == set(full) and e['h_pos'].shape == (0, 4, 3) and H.summary(e)['n_molecules'] == 0
    assert H.compare(full, full)['min_contact'] == 0.0
    # the command line on the host path: the Kekulé counts are made there
    plain = [m for m, k in zip(mols, names) if k not in ('pyridinium', 'no_room', 'clamped', 'bad_bond')]
    torch.save({'finished': plain}, str(tmp_path / 'samples_all.pt'))
    out, sdf = str(tmp_path / 'h.npz'), str(tmp_path / 'h.sdf')
    assert H.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', out, '--sdf', sdf, '--ref']) == 0
    saved = molpack.load_npz(out)
    want = H.stack_ref(plain)
    assert set(saved) == set(want) and all(np.array_equal(saved[k], want[k]) for k in want)
    assert len(rmsd.read_sdf(sdf)) == len(plain)
    assert H.main(['compare', out, out]) == 0


def test_table_validation_raises():
    with pytest.raises(ValueError, match='X-H length'):
        H.HydrogenTables(atomic_numbers=(6, 7, 35))
    with pytest.raises(ValueError, match='outside the atomic numbers'):
        H.HydrogenTables(atomic_numbers=(6, 7), xh_length={6: 1.09, 7: 1.01, 8: 0.96})
    with pytest.raises(ValueError, match='outside the atomic numbers'):
        H.HydrogenTables(atomic_numbers=(6, 8), xh_length={6: 1.09, 8: 0.96}, planar=(7,))
    for bad in (0.0, -1.0, 4.5, float('nan')):
        with pytest.raises(ValueError, match=r'\(0, 4'):
            H.HydrogenTables(xh_length={**H.DEFAULT_XH_LENGTH, 6: bad})
    with pytest.raises(ValueError, match='elements'):
        H.HydrogenTables(atomic_numbers=range(33), xh_length={z: 1.0 for z in range(33)})
    with pytest.raises(ValueError, match='bond types'):
        H.HydrogenTables(num_bond_types=17)
    tb = H.HydrogenTables(planar=(7, 8))
    assert tb.planar == 0b110 and tb.xh_length.dtype == np.float64 and tb.xh_length.tolist() == [1.09, 1.01, 0.96, 0.92, 1.42, 1.34, 1.27]
    info, n_h, order = HC.named()['ethane']
    for kw in (dict(deg_tol=0.0), dict(deg_tol=1.0), dict(deg_tol=float('nan')), dict(clash_tol=-1.0), dict(clash_tol=2000.0)):
        with pytest.raises(ValueError, match='tol'):
            H.addh_ref(info, n_h, order, **kw)


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/hydrogens_host_check.cpp over csrc/mdx_hydrogens_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('hydrogens_host_check', tmp_path)
