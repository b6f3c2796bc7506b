"""Host tests of the stereo perception: ``stereo.stereo_ref`` alone (invariance, the fixtures, a brute force over all rank vectors),
the isomeric key, the isomeric SMILES of ``canon.smiles`` and the argument checks.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

from moldiff_amd import canon as C
from moldiff_amd import kekule as K
from moldiff_amd import stereo as S
from .canon_cases import mol
from .stereo_cases import fixtures, moved, random_3d, reflected
from .util import run_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = fixtures()
INVARIANT = S.STAT_KEYS + ('stereo_hash', 'mirror_hash', 'canon_tetra', 'mirror_tetra', 'canon_bond_stereo', 'mirror_bond_stereo')


def measure(m, **kw):
    c = C.canon_ref(m)
    return c, S.stereo_ref(m, c, **kw)


def same(a, b, keys=INVARIANT):
    return all(np.array_equal(a[k], b[k]) for k in keys)


RES = {name: measure(m) for name, m in FIX.items()}


def test_invariance_under_relabelling_and_rigid_motion_and_the_swap_under_reflection():
    cases = list(FIX.items()) + [('random%d' % s, random_3d(5000 + s)) for s in range(200)]
    chiral = 0
    for name, m in cases:
        if S.near_threshold(m, band=1e-4):           # float32 rounding of the rotated coordinates may cross a threshold there
            assert name.startswith('random'), name
            continue
        _, r = RES[name] if name in RES else measure(m)
        for k in range(20 if name in FIX else 3):
            other = moved(m, 100 * k + 7)
            assert same(r, measure(other)[1]), (name, k)
        _, q = measure(reflected(m))
        assert np.array_equal(q['canon_tetra'], r['mirror_tetra']) and np.array_equal(q['mirror_tetra'], r['canon_tetra']), name
        assert np.array_equal(q['canon_bond_stereo'], r['mirror_bond_stereo']) and q['stereo_hash'] == r['mirror_hash'], name
        assert [q[k] for k in S.STAT_KEYS] == [r[k] for k in S.STAT_KEYS], name
        if not r['chiral']:
            assert np.array_equal(q['canon_bond_stereo'], r['canon_bond_stereo']), name
        chiral += r['chiral']
    assert chiral >= 20


def test_random_graphs_twenty_motions_each():
    for s in range(200):
        m = random_3d(5000 + s)
        if S.near_threshold(m, band=1e-4):
            continue
        r = measure(m)[1]
        assert all(same(r, measure(moved(m, 31 * k + s))[1]) for k in range(3, 20)), s


def test_the_fixtures():
    st = lambda name: RES[name][1]
    a, b = st('chfclbr'), st('chfclbr_mirror')
    assert a['chiral'] == b['chiral'] == 1 and a['n_centres'] == 1 and a['n_stereogenic'] == 1
    assert np.array_equal(a['canon_tetra'], b['mirror_tetra']) and not np.array_equal(a['canon_tetra'], b['canon_tetra'])
    a, b = st('centre4'), st('centre4_mirror')
    assert a['chiral'] == 1 and np.array_equal(a['canon_tetra'], b['mirror_tetra']) and a['stereo_hash'] == b['mirror_hash'] != a['mirror_hash']
    n = st('neopentane')
    assert (n['n_aut'], n['n_centres'], n['n_stereogenic'], n['chiral']) == (24, 1, 0, 0) and RES['neopentane'][0]['n_aut'] == 24
    g, h = st('gem_dimethyl'), st('gem_dimethyl_swapped')
    assert (g['n_centre_candidates'], g['n_centres'], g['n_stereogenic'], g['chiral']) == (1, 1, 0, 0) and same(g, h)
    z, e = st('butene_z'), st('butene_e')
    assert z['canon_bond_stereo'].tolist().count(1) == 1 and e['canon_bond_stereo'].tolist().count(2) == 1 and z['chiral'] == e['chiral'] == 0
    assert st('difluoroethene_z')['n_stereo_bonds'] == 1 and st('difluoroethene_z')['stereo_hash'] != st('difluoroethene_e')['stereo_hash']
    c, t = st('dimethylcyclohexane_cis'), st('dimethylcyclohexane_trans')
    assert c['chiral'] == t['chiral'] == 0 and c['n_centres'] == t['n_centres'] == 2 and not np.array_equal(c['canon_tetra'], t['canon_tetra'])
    both = C.stack_ref([FIX['dimethylcyclohexane_cis'], FIX['dimethylcyclohexane_trans']])
    assert C.certificate(both, 0) == C.certificate(both, 1)
    pp, mm, meso = st('butane_pp'), st('butane_mm'), st('butane_meso')
    assert pp['chiral'] == mm['chiral'] == 1 and meso['chiral'] == 0 and meso['n_centres'] == 2 and pp['n_stereogenic'] == 2
    assert np.array_equal(pp['canon_tetra'], mm['mirror_tetra']) and np.array_equal(meso['canon_tetra'], meso['mirror_tetra'])
    assert not np.array_equal(pp['canon_tetra'], mm['canon_tetra']) and not np.array_equal(pp['canon_tetra'], meso['canon_tetra'])
    f = st('flat_centre')
    assert (f['n_centre_candidates'], f['n_flat'], f['n_centres'], f['chiral']) == (1, 1, 0, 0)
    assert (st('nan')['n_flat'], st('nan')['n_centres']) == (1, 0)
    assert (st('coincident')['n_bond_candidates'], st('coincident')['n_stereo_bonds']) == (1, 0)
    assert st('allene')['n_bond_candidates'] == 0 and st('allene')['status'] == 0
    assert all(RES[k][1]['n_aut'] == RES[k][0]['n_aut'] for k in RES)


def brute(m):
    """W and the number of optimal rank vectors by trying every permutation of the atoms as a rank vector"""
    c = C.canon_ref(m)
    geo = S.geometry_ref(m)
    n, nb = len(m['element']), m['bond_index'].shape[1] // 2
    bi, bt = m['bond_index'][:, :nb], m['bond_type'][:nb]
    words = lambda r: sorted((min(r[i], r[j]) << 20) | (max(r[i], r[j]) << 8) | int(t) for (i, j), t in zip(bi.T, bt))
    canonical = words(c['rank'])
    labels = [int(m['element'][a]) for a in np.argsort(c['rank'])]
    best, count = None, 0
    for r in itertools.permutations(range(n)):
        if [int(m['element'][a]) for a in np.argsort(r)] != labels or words(r) != canonical:
            continue
        count += 1
        w = [0] * (n + nb)
        for a, g in geo['g'].items():
            if g:
                ranks = [r[u] for u in geo['nbrs'][a]]
                even = sum(x > y for x, y in itertools.combinations(ranks, 2)) % 2 == 0
                w[r[a]] = 1 if (g > 0) == even else 2
        for e, (xs, ys, table) in geo['d'].items():
            i, j = int(bi[0, e]), int(bi[1, e])
            k = canonical.index((min(r[i], r[j]) << 20) | (max(r[i], r[j]) << 8) | int(bt[e]))
            w[n + k] = table[min(xs, key=lambda u: r[u]), min(ys, key=lambda u: r[u])]
        best = w if best is None or w < best else best
    return best, count


def test_brute_force_over_all_rank_vectors():
    small = [m for m in FIX.values() if len(m['element']) <= 7] + [random_3d(6000 + s, 3, 7) for s in range(25)]
    for k, m in enumerate(small):
        W, count = brute(m)
        c, r = measure(m)
        n = len(m['element'])
        assert count == c['n_aut'] == r['n_aut'], k
        assert r['canon_tetra'].tolist() + r['canon_bond_stereo'][:c['canon_n_bonds']].tolist() == W, k
        assert np.array_equal(r['atom_tetra'], r['canon_tetra'][r['stereo_rank']]) and sorted(r['stereo_rank'].tolist()) == list(range(n))
        assert r['stereo_hash'] == C.fnv1a64(W)


def test_the_isomeric_key_separates_what_the_certificate_merges():
    mols = [FIX['chfclbr'], FIX['chfclbr_mirror'], moved(FIX['chfclbr'], 3), FIX['butene_z'], FIX['butene_e'], FIX['butane_meso']]
    c = C.stack_ref(mols)
    s = S.stack_ref(mols, c)
    keys = [S.iso_certificate(c, s, m) for m in range(len(mols))]
    assert len({C.certificate(c, m) for m in range(3)}) == 1 and len(set(keys[:3])) == 2 and keys[0] == keys[2] != keys[1]
    assert keys[3] != keys[4] and C.certificate(c, 3) == C.certificate(c, 4)
    assert S.iso_certificate(c, s, 0, mirror=True) == keys[1] and S.iso_certificate(c, s, 5, mirror=True) == keys[5]
    u = S.summary(s, c)
    assert (u['n_measured'], u['n_distinct'], u['n_iso_distinct'], u['n_enantiomer_pairs'], u['n_chiral']) == (6, 3, 5, 1, 3)
    assert u['iso_uniqueness'] == 5 / 6 and u['uniqueness'] == 3 / 6 and u['share_chiral'] == 0.5 and u['share_flat_centres'] == 0.0
    three = S.stack_ref(mols[:3])
    assert S.summary(three, C.stack_ref(mols[:3]))['iso_uniqueness'] == 2 / 3 and C.summary(C.stack_ref(mols[:3]))['uniqueness'] == 1 / 3
    assert S.novelty(s, c, three, C.stack_ref(mols[:3])) == 3 / 6
    both = S.merged(c, s)
    assert S.compare(both, both)['novelty'] == [0.0, 0.0] and S.compare(both, both)['centres'] == 0
    again = S.concat([S.stack_ref(mols[:2]), S.stack_ref(mols[2:])])
    assert set(again) == set(s) and all(np.array_equal(again[k], s[k]) and again[k].dtype == s[k].dtype for k in s)
    e = S.empty()
    assert e['status'].shape == (0,) and e['stereo_hash'].dtype == np.int64 and np.isnan(S.summary(e, C.empty())['iso_uniqueness'])
    neo = [FIX['neopentane']]
    abandoned = S.stack_ref(neo, C.stack_ref(neo, max_nodes=1), max_nodes=1)
    assert abandoned['status'].tolist() == [1] and abandoned['stereo_rank'].tolist() == [-1] * 5 and S.iso_certificate(C.stack_ref(neo), abandoned, 0) is None
    assert S.stack_ref([FIX['neopentane']], C.stack_ref([FIX['neopentane']]), max_nodes=5)['status'].tolist() == [2]


# ``canon.smiles`` of the fixtures as the commit before the stereo argument wrote them
PLAIN = {'chfclbr': 'CC(F)Cl', 'chfclbr_mirror': 'CC(F)Cl', 'centre4': 'C(C)(O)(F)Cl', 'centre4_mirror': 'C(C)(O)(F)Cl', 'neopentane': 'C(C)(C)(C)C',
         'gem_dimethyl': 'CC(C)(F)Cl', 'gem_dimethyl_swapped': 'CC(C)(F)Cl', 'butene_z': 'CC=CC', 'butene_e': 'CC=CC', 'difluoroethene_z': 'C(=CF)F',
         'difluoroethene_e': 'C(=CF)F', 'dimethylcyclohexane_cis': 'C1CC(CCC1C)C', 'dimethylcyclohexane_trans': 'C1CC(CCC1C)C',
         'butane_pp': 'CC(C(C)F)F', 'butane_mm': 'CC(C(C)F)F', 'butane_meso': 'CC(C(C)F)F', 'flat_centre': 'C(C)(O)(F)Cl', 'nan': 'C(C)(O)(F)Cl',
         'coincident': 'CC=CC', 'allene': 'C(=CC)=CC'}


def text(m, stereo=True):
    c, r = measure(m)
    cm = C.canonical_mol(m, c)
    return C.smiles(cm, K.kekulize_ref(cm), r if stereo else None)


def test_isomeric_smiles():
    for name, want in PLAIN.items():                                   # without a stereo result: the strings of before
        assert text(FIX[name], stereo=False) == want == text(reflected(FIX[name]), stereo=False), name
    # hand-derived: in 'chfclbr' C sits at the origin with F, Cl, CH3 on tetrahedral directions 0, 1, 2 and H on 3; seen from the CH3
    # (-1, 1, -1) the others H (-1, -1, 1), F (1, 1, 1), Cl (1, -1, -1) run anticlockwise (det[H, F, Cl] = -4 < 0): '@'
    assert text(FIX['chfclbr']) == 'C[C@H](F)Cl' and text(FIX['chfclbr_mirror']) == 'C[C@@H](F)Cl'
    # the two methyls of (Z)-2-butene lie on the same side: 'C/C=C\\C' is cis in OpenSMILES, 'C\\C=C\\C' (= C/C=C/C) trans
    assert text(FIX['butene_z']) == 'C/C=C\\C' and text(FIX['butene_e']) == 'C\\C=C\\C'
    # 'centre4' adds O on direction 3 (-1, -1, 1): seen from the CH3, O, F, Cl run anticlockwise by the same determinant
    assert text(FIX['centre4']) == '[C@](C)(O)(F)Cl' and text(FIX['centre4_mirror']) == '[C@@](C)(O)(F)Cl'
    # a branch reads from its atom: C(\\F) and C\\F point the same way, so the two F are cis
    assert text(FIX['difluoroethene_z']) == 'C(=C\\F)\\F' and text(FIX['difluoroethene_e']) == 'C(=C/F)\\F'
    for name, m in FIX.items():
        want = text(m)
        assert all(text(moved(m, 11 * k + 5)) == want for k in range(5)), name
    a, b = text(FIX['centre4']), text(FIX['centre4_mirror'])
    assert a != b and a.replace('@@', '@') == b.replace('@@', '@') and a.count('@') + b.count('@') == 3
    pp, mm, meso = text(FIX['butane_pp']), text(FIX['butane_mm']), text(FIX['butane_meso'])
    assert len({pp, mm, meso}) == 3 and pp.replace('@@', '@') == mm.replace('@@', '@') == meso.replace('@@', '@')
    assert '@' not in text(FIX['flat_centre']) and '/' not in text(FIX['allene']) and '@' in text(FIX['neopentane'])
    z, e = text(FIX['butene_z']), text(FIX['butene_e'])
    assert sum(x != y for x, y in zip(z, e)) == 1 and len(z) == len(e)
    mols = [FIX['chfclbr'], FIX['butene_e']]
    c = C.stack_ref(mols)
    assert C.smiles_mols(mols, c, stereo=S.stack_ref(mols, c)) == ['C[C@H](F)Cl', 'C\\C=C\\C'] and C.smiles_mols(mols, c) == ['CC(F)Cl', 'CC=CC']


def test_argument_checks():
    m = FIX['chfclbr']
    c = C.canon_ref(m)
    for kw in ({'flat_tol': -0.1}, {'flat_tol': 1.0}, {'bond_tol': float('nan')}, {'max_nodes': 0}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            S.stereo_ref(m, c, **kw)
    with pytest.raises(ValueError, match='label'):
        S.stereo_ref(m, c, atom_label=[0, 1, 2])
    with pytest.raises(ValueError, match='different lists'):
        S.summary(S.stack_ref([m]), C.stack_ref([m, m]))
    assert S.class_mask(S.DEFAULT_CENTRE4) == 0b110011 and S.class_mask(S.DEFAULT_CENTRE3) == 1 and S.class_mask((8,), (6, 7)) == 0
    only_n = S.stereo_ref(m, c, centre3_mask=2)
    assert only_n['n_centre_candidates'] == 0 and only_n['status'] == 0
    assert S.stereo_ref(m, dict(c, rank=np.asarray([0, 1, 2, 9])))['status'] == 1
    assert S.stereo_ref(FIX['butene_z'], dict(C.canon_ref(FIX['butene_z']), rank=np.asarray([0, 2, 1, 3])))['status'] == 1   # no leaf attains it


def test_the_entry_point_is_declared_and_registered():
    from moldiff_amd import _lib
    with open(os.path.join(ROOT, 'include', 'moldiff_hip.h')) as f:
        hdr = f.read()
    proto = re.search(r'\bint mdx_mol_stereo\(([^;]*)\);', hdr).group(1)
    params = [p.strip() for p in proto.split(',')]
    assert len(params) == 31 and params[-1] == 'void* stream' and '#define MDX_STEREO_STATS 9' in hdr and len(S.STAT_KEYS) == 9
    assert 'NOT the CIP rules' in hdr and 'UNVERIFIED AGAINST RDKit' in hdr and 'mdx_mol_stereo' in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert hasattr(L, 'mdx_mol_stereo') and len(L.mdx_mol_stereo.argtypes) == 31


def test_command_line_and_files(tmp_path):
    import torch
    from moldiff_amd.molpack import load_npz
    mols = [FIX[k] for k in ('chfclbr', 'chfclbr_mirror', 'butene_z', 'neopentane')]
    torch.save({'finished': mols}, tmp_path / 'samples_all.pt')
    assert S.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'a.npz'), '--ref']) == 0
    c, s = S.split(load_npz(tmp_path / 'a.npz'))
    want = S.stack_ref(mols)
    assert all(np.array_equal(s[k], want[k]) for k in want) and S.summary(s, c)['n_enantiomer_pairs'] == 1
    assert S.main(['compare', str(tmp_path / 'a.npz'), str(tmp_path / 'a.npz')]) == 0


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/stereo_host_check.cpp over csrc/mdx_stereo_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('stereo_host_check', tmp_path)
