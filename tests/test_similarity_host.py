"""CPU tests of the set-level similarity's host half (moldiff_amd/similarity.py): the numpy restatements ``fingerprint_ref``,
``tanimoto_ref`` and ``summary_ref``, the spec, the fingerprint file, the command line with --ref, the sampling entry point's option
and the declaration / export / binding of the two device entries.  Every comparison is exact."""
import json
import os
import re

import numpy as np
import pytest

from moldiff_amd import _lib
from moldiff_amd import sample_drug3d
from moldiff_amd import similarity as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)


def mol(ele, bonds):
    """a decoded molecule dict: every bond once, then all of them flipped"""
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
            'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def random_mol(seed, n, extra=0.3):
    """a connected random molecule: a random spanning tree plus `extra` * n further bonds, every element and bond type drawn"""
    g = np.random.default_rng(seed)
    bonds = {(int(g.integers(0, k)), k) for k in range(1, n)}
    while len(bonds) < n - 1 + int(extra * n) and n > 2:
        i, j = sorted(int(x) for x in g.choice(n, 2, replace=False))
        bonds.add((i, j))
    return mol(g.choice(ELEMENTS, n), [(i, j, int(g.integers(1, 5))) for i, j in sorted(bonds)])


def relabelled(m, seed):
    """the same molecule with its atoms renumbered at random, its bonds reordered at random and some of them flipped"""
    g = np.random.default_rng(seed)
    n, nb = len(m['element']), m['bond_index'].shape[1] // 2
    new = g.permutation(n)                                             # old atom a becomes new[a]
    ele = np.empty(n, dtype=np.int64)
    ele[new] = m['element']
    order = g.permutation(nb)
    idx = new[m['bond_index'][:, :nb]][:, order]
    flip = g.random(nb) < 0.5
    idx = np.where(flip, idx[::-1], idx)
    bt = m['bond_type'][:nb][order]
    return {'element': ele, 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}


def same_fp(a, b):
    return np.array_equal(a['bits'], b['bits']) and a['n_on'] == b['n_on'] and a['key'] == b['key'] and a['n_atoms'] == b['n_atoms']


# ---- fingerprint_ref --------------------------------------------------------------------------------------------------------------------

def test_fingerprint_is_invariant_under_relabelling_and_changes_with_the_molecule():
    for spec in (S.FingerprintSpec(), S.FingerprintSpec(radius=0, nbits=32, key_rounds=3), S.FingerprintSpec(radius=3, nbits=96, key_rounds=3)):
        for seed, n in ((1, 2), (2, 7), (3, 23), (4, 60)):
            m = random_mol(seed, n)
            f = S.fingerprint_ref(m, spec)
            assert f['n_atoms'] == n and f['n_on'] == int(S.popcount(f['bits']).sum()) > 0
            for k in range(3):
                assert same_fp(f, S.fingerprint_ref(relabelled(m, 10 * seed + k), spec)), (seed, k)
            # one element changed, one bond type changed: the key always moves; the bits move when they are wide enough to show it
            e = dict(m, element=m['element'].copy())
            e['element'][n // 2] = 17 if e['element'][n // 2] != 17 else 6
            t = dict(m, bond_type=m['bond_type'].copy())
            nb = len(t['bond_type']) // 2
            t['bond_type'][[0, nb]] = t['bond_type'][0] % 4 + 1
            for other in (e, t):
                g = S.fingerprint_ref(other, spec)
                assert g['key'] != f['key']
                if spec.nbits == 2048:
                    assert not np.array_equal(g['bits'], f['bits'])
    # a bond type only enters from round 1 on: with radius 0 the bits stay and the key moves
    r0 = S.FingerprintSpec(radius=0, key_rounds=2)
    a, b = mol([6, 8], [(0, 1, 1)]), mol([6, 8], [(0, 1, 2)])
    assert np.array_equal(S.fingerprint_ref(a, r0)['bits'], S.fingerprint_ref(b, r0)['bits'])
    assert S.fingerprint_ref(a, r0)['key'] != S.fingerprint_ref(b, r0)['key']


def _mix(h):
    h &= 0xffffffff
    h ^= h >> 16
    h = h * 0x85ebca6b & 0xffffffff
    h ^= h >> 13
    h = h * 0xc2b2ae35 & 0xffffffff
    return h ^ h >> 16


def test_two_atom_molecule_by_hand():
    """C=O with radius 1, 64 bits, 2 key rounds: classes 0 and 2, one bond of type 2, both degrees 1.  The ids below were computed
    with Python integers from the header's text and are pinned as literals; the arithmetic is repeated here beside them."""
    G, P, M = 0x9e3779b9, 0x01000193, 0xffffffff
    ids = [[0x12bc8390, 0x2c85567e], [0x4aa0093c, 0xeafc20e0], [0x52a488b0, 0x707f2779]]
    assert ids[0] == [_mix(0 + 1 + G * 2), _mix(2 + 1 + G * 2)]
    for r in range(2):
        a, b = ids[r]
        assert ids[r + 1] == [_mix(a * P + (r + 1) + _mix(b + G * 2)), _mix(b * P + (r + 1) + _mix(a + G * 2))]
    spec = S.FingerprintSpec(radius=1, nbits=64, key_rounds=2)
    m = mol([6, 8], [(0, 1, 2)])
    assert S.atom_ids(m, spec).tolist() == ids
    f = S.fingerprint_ref(m, spec)
    assert sorted({x % 64 for row in ids[:2] for x in row}) == [16, 32, 60, 62]        # rounds 0 and 1 set bits, round 2 does not
    assert f['bits'].tolist() == [1 << 16, 1 << 0 | 1 << 28 | 1 << 30] and f['n_on'] == 4 and f['n_atoms'] == 2
    lo = sum(_mix(x + r) for r, row in enumerate(ids) for x in row) & M
    hi = sum(_mix(x ^ 0x5bd1e995) for row in ids for x in row) & M
    assert (lo, hi) == (0x16d24a6f, 0x49786add) and int(f['key']) == hi << 32 | lo == 5294098859777215087
    assert same_fp(f, S.fingerprint_ref(mol([8, 6], [(1, 0, 2)]), spec))


def test_invalid_bonds_are_ignored_and_tiny_molecules_give_the_stated_values():
    spec = S.FingerprintSpec()
    ring = mol([6, 6, 7, 6, 6, 8], [(k, (k + 1) % 6, 4) for k in range(6)])
    bad = mol([6, 6, 7, 6, 6, 8], [(0, 6, 1), (2, 2, 3)] + [(k, (k + 1) % 6, 4) for k in range(6)] + [(-1, 3, 2)])
    assert same_fp(S.fingerprint_ref(ring, spec), S.fingerprint_ref(bad, spec))
    empty = S.fingerprint_ref({'element': np.zeros(0, dtype=np.int64)}, spec)
    assert empty['n_on'] == 0 and empty['key'] == 0 and empty['n_atoms'] == 0 and not empty['bits'].any() and empty['bits'].shape == (64,)
    # one nitrogen (class 1, degree 0) with radius 0 and no further key round: id_0 = mix(1 + 1 + 0x9e3779b9) = 0xb4421bbb
    one = S.fingerprint_ref({'element': np.asarray([7])}, S.FingerprintSpec(radius=0, nbits=32, key_rounds=0))
    assert _mix(2 + 0x9e3779b9) == 0xb4421bbb and one['bits'].tolist() == [1 << (0xb4421bbb % 32)] and one['n_on'] == 1
    assert int(one['key']) == _mix(0xb4421bbb ^ 0x5bd1e995) << 32 | _mix(0xb4421bbb)
    lone = S.fingerprint_ref({'element': np.asarray([7]), 'bond_index': np.zeros((2, 0), dtype=np.int64), 'bond_type': np.zeros(0)}, spec)
    assert lone['n_atoms'] == 1 and 1 <= lone['n_on'] <= 3
    with pytest.raises(ValueError, match='not among'):
        S.fingerprint_ref({'element': np.asarray([5])}, spec)


# ---- tanimoto_ref -----------------------------------------------------------------------------------------------------------------------

def rows(*sets, words=2):
    out = np.zeros((len(sets), words), dtype=np.uint32)
    for r, s in enumerate(sets):
        for k in s:
            out[r, k // 32] |= np.uint32(1 << (k % 32))
    return out, S.popcount(out).sum(1).astype(np.int32)


def test_tanimoto_hand_cases():
    a, na = rows({0, 1, 40}, {5}, set(), {0, 1, 2, 3})
    b, nb = rows({0, 1, 40}, {7, 8}, set(), {0, 1}, {0, 1, 40})
    mx, am, sm = S.tanimoto_ref(a, na, b, nb)
    assert mx.dtype == np.float32 and am.dtype == np.int32 and sm.dtype == np.int64
    # row 0: identical to columns 0 and 4 (1.0, the tie goes to the smaller j), 2/3 with column 3, disjoint from 1 and 2
    assert mx[0] == 1.0 and am[0] == 0 and sm[0] == 2 * S.FIXED_ONE + int(np.float64(np.float32(2) / np.float32(3)) * S.FIXED_ONE)
    # row 1: disjoint from every column: all q are 0 and the smallest j is 0
    assert mx[1] == 0.0 and am[1] == 0 and sm[1] == 0
    # row 2 (empty): u = 0 against the empty column 2 gives q = 0, by this project's choice
    assert mx[2] == 0.0 and am[2] == 0 and sm[2] == 0
    assert mx[3] == np.float32(2) / np.float32(4) and am[3] == 3
    # no columns: no partner
    mx, am, sm = S.tanimoto_ref(a, na, b[:0], nb[:0])
    assert mx.tolist() == [0.0] * 4 and am.tolist() == [-1] * 4 and sm.tolist() == [0] * 4
    assert all(len(x) == 0 for x in S.tanimoto_ref(a[:0], na[:0], b, nb))


def test_tanimoto_self_mode_excludes_the_diagonal():
    a, na = rows({0, 1}, {0, 1}, {1, 2}, {9})
    mx, am, sm = S.tanimoto_ref(a, na, a, na, exclude_diagonal=True)
    third = np.float32(1) / np.float32(3)
    assert mx.tolist() == [1.0, 1.0, float(third), 0.0] and am.tolist() == [1, 0, 0, 0]
    assert sm[0] == S.FIXED_ONE + int(np.float64(third) * S.FIXED_ONE)
    full = S.tanimoto_ref(a, na, a, na)
    assert full[0].tolist() == [1.0] * 4 and full[1].tolist() == [0, 0, 2, 3] and (full[2] - sm).tolist() == [S.FIXED_ONE] * 4
    one = S.tanimoto_ref(a[:1], na[:1], a[:1], na[:1], exclude_diagonal=True)
    assert one[0].tolist() == [0.0] and one[1].tolist() == [-1] and one[2].tolist() == [0]
    with pytest.raises(ValueError):
        S.tanimoto_ref(a, na, a[:2], na[:2], exclude_diagonal=True)


def test_fixed_point_sum_equals_the_float64_sum_exactly():
    g = np.random.default_rng(5)
    for words, density in ((1, 0.5), (3, 0.2), (64, 0.05), (1024, 0.5)):
        a = (g.random((37, words * 32)) < density)
        b = (g.random((53, words * 32)) < density)
        pack = lambda x: np.packbits(x, axis=1, bitorder='little').view(np.uint32)
        wa, wb = pack(a), pack(b)
        na, nb = a.sum(1).astype(np.int32), b.sum(1).astype(np.int32)
        assert np.array_equal(S.popcount(wa).sum(1), na)
        mx, am, sm = S.tanimoto_ref(wa, na, wb, nb)
        c = (a[:, None, :] & b[None, :, :]).sum(-1)
        u = na[:, None] + nb[None, :] - c
        q = np.where(u > 0, c.astype(np.float32) / np.maximum(u, 1).astype(np.float32), np.float32(0)).astype(np.float32)
        exact = q.astype(np.float64).sum(1)               # at most 53 multiples of 2^-39 below 1: exact in float64
        assert np.array_equal(sm.astype(np.float64) / S.FIXED_ONE, exact) and np.array_equal(mx, q.max(1)) and np.array_equal(am, q.argmax(1))
        assert q[q > 0].min() >= 2.0 ** -16


# ---- summary_ref, the set and its file ---------------------------------------------------------------------------------------------------

def planted_sets():
    base = [random_mol(100 + k, 6 + k) for k in range(10)]
    own = base + [relabelled(base[0], 1), relabelled(base[0], 2), relabelled(base[3], 3)]      # 13 molecules, 10 distinct
    reference = [relabelled(base[1], 4), relabelled(base[4], 5), relabelled(base[4], 6)] + [random_mol(200 + k, 9) for k in range(4)]
    return own, reference


def test_summary_ref_on_planted_duplicates_and_reference_overlap():
    own, reference = planted_sets()
    spec = S.FingerprintSpec()
    a, r = S.FingerprintSet.from_ref(own, spec), S.FingerprintSet.from_ref(reference, spec)
    res = S.summary_ref(a, r)
    assert set(res) == {'n', 'uniqueness', 'diversity', 'novelty', 'sim_with_ref'}
    assert res['n'] == 13 and res['uniqueness'] == 10 / 13 and res['novelty'] == 11 / 13             # base[1] and base[4] are known
    mx, _, sm = S.tanimoto_ref(a.bits, a.n_on, a.bits, a.n_on, True)
    assert res['diversity'] == 1.0 - sum(sm.tolist()) / (S.FIXED_ONE * 13 * 12) and 0 < res['diversity'] < 1
    assert mx[0] == mx[10] == mx[11] == mx[3] == mx[12] == 1.0
    against = S.tanimoto_ref(a.bits, a.n_on, r.bits, r.n_on)[0]
    assert against[1] == against[4] == 1.0 and res['sim_with_ref'] == float(against.astype(np.float64).sum() / 13)
    alone = S.summary_ref(a)
    assert set(alone) == {'n', 'uniqueness', 'diversity'} and alone['diversity'] == res['diversity']
    # 256 copies of one molecule: valid one by one, and no diversity at all
    copies = S.FingerprintSet.from_ref([relabelled(own[5], k) for k in range(256)], spec)
    assert S.summary_ref(copies) == {'n': 256, 'uniqueness': 1 / 256, 'diversity': 0.0}
    few = S.summary_ref(S.FingerprintSet.from_ref(own[:1], spec), r)
    assert few['n'] == 1 and few['uniqueness'] == 1.0 and np.isnan(few['diversity']) and few['novelty'] == 1.0
    none = S.summary_ref(S.FingerprintSet.empty(spec), r)
    assert none['n'] == 0 and all(np.isnan(none[k]) for k in ('uniqueness', 'diversity', 'novelty', 'sim_with_ref'))


def test_set_file_round_trip_append_and_specs_that_differ(tmp_path):
    own, reference = planted_sets()
    spec = S.FingerprintSpec(radius=1, nbits=96, key_rounds=4)
    a = S.FingerprintSet.from_ref(own, spec)
    path = str(tmp_path / 'a.npz')
    a.save(path)
    b = S.FingerprintSet.load(path)
    assert b.spec == spec and b.bits.dtype == np.uint32 and b.bits.shape == (13, 3)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ('bits', 'n_on', 'key', 'n_atoms'))
    joined = S.FingerprintSet.from_ref(own[:4], spec).append(S.FingerprintSet.from_ref(own[4:], spec))
    assert all(np.array_equal(getattr(a, k), getattr(joined, k)) for k in ('bits', 'n_on', 'key', 'n_atoms'))
    other = S.FingerprintSet.from_ref(reference, S.FingerprintSpec(radius=2, nbits=96, key_rounds=4))
    with pytest.raises(ValueError, match='different specs'):
        S.summary_ref(a, other)
    with pytest.raises(ValueError, match='different specs'):
        a.append(other)
    with pytest.raises(ValueError):
        S.FingerprintSet(spec, a.bits[:, :2], a.n_on, a.key, a.n_atoms)


def test_spec_refuses_bad_values():
    d = S.FingerprintSpec()
    assert (d.radius, d.nbits, d.key_rounds, d.atomic_numbers, d.num_bond_types, d.words) == (2, 2048, 8, ELEMENTS, 4, 64)
    assert S.FingerprintSpec.from_dict(d.to_dict()) == d and d != S.FingerprintSpec(nbits=1024)
    for bad in (dict(nbits=100), dict(nbits=0), dict(nbits=32800), dict(nbits=65536), dict(radius=-1), dict(radius=3, key_rounds=2),
                dict(key_rounds=65), dict(radius=1.5), dict(nbits=True), dict(atomic_numbers=()), dict(atomic_numbers=(6, 6)),
                dict(atomic_numbers=(0, 6)), dict(num_bond_types=0)):
        with pytest.raises(ValueError):
            S.FingerprintSpec(**bad)
    assert S.FingerprintSpec(nbits=32).words == 1 and S.FingerprintSpec(nbits=32768, radius=0, key_rounds=0).words == 1024


# ---- wiring and command line ----------------------------------------------------------------------------------------------------------------

def test_similarity_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'moldiff_hip.h')).read()
    declared = set(re.findall(r'\b(mdx_[a-z_0-9]+)\s*\(', hdr))
    names = ('mdx_mol_fingerprint', 'mdx_mol_fingerprint_ws_bytes', 'mdx_fp_tanimoto', 'mdx_fp_tanimoto_ws_bytes')
    assert all(n in declared and n in _lib.EXPORTS for n in names)
    L = _lib.lib()
    assert len(L.mdx_mol_fingerprint.argtypes) == 20 and len(L.mdx_fp_tanimoto.argtypes) == 14
    assert L.mdx_mol_fingerprint_ws_bytes(0) == 8 and L.mdx_mol_fingerprint_ws_bytes(1000) == 8000
    assert L.mdx_fp_tanimoto_ws_bytes(0) == 8 and L.mdx_fp_tanimoto_ws_bytes(130) == 1040
    # argument checks that need no device
    ARG, UNSUPPORTED = 1, 4
    assert L.mdx_mol_fingerprint(1, *[None] * 5, 4, None, None, 4, None, 2, 8, 2048, None, None, None, None, 0, None) == ARG
    assert L.mdx_fp_tanimoto(None, None, 0, None, None, 0, 100, 0, None, None, None, None, 0, None) == ARG and b'nbits' in L.mdx_last_error()
    assert L.mdx_fp_tanimoto(None, None, 2, None, None, 3, 64, 1, None, None, None, None, 0, None) == ARG and b'Na == Nb' in L.mdx_last_error()
    assert L.mdx_fp_tanimoto(None, None, 0, None, None, (1 << 22) + 1, 64, 0, None, None, None, None, 0, None) == UNSUPPORTED


def test_command_line_round_trips_with_ref(tmp_path, capsys):
    import torch
    own, reference = planted_sets()
    torch.save({'finished': own, 'failed': reference[:2]}, tmp_path / 'samples_all.pt')
    torch.save(reference, tmp_path / 'train.pt')
    a, t = str(tmp_path / 'a.npz'), str(tmp_path / 'train.npz')
    assert S.main(['fingerprint', str(tmp_path / 'samples_all.pt'), '--out', a, '--ref']) == 0
    assert S.main(['fingerprint', str(tmp_path / 'train.pt'), '--out', t, '--ref', '--part', 'finished']) == 0
    fa = S.FingerprintSet.load(a)
    assert len(fa) == 13 and fa.spec == S.FingerprintSpec() and len(S.FingerprintSet.load(t)) == 7
    assert np.array_equal(fa.bits, S.FingerprintSet.from_ref(own, S.FingerprintSpec()).bits)
    capsys.readouterr()
    assert S.main(['summary', a, '--against', t, '--ref']) == 0
    res = json.loads(capsys.readouterr().out)
    assert res == S.summary_ref(fa, S.FingerprintSet.load(t)) and res['uniqueness'] == 10 / 13 and res['novelty'] == 11 / 13
    assert S.main(['fingerprint', str(tmp_path / 'samples_all.pt'), '--out', a, '--ref', '--part', 'failed', '--nbits', '96']) == 0
    assert len(S.FingerprintSet.load(a)) == 2 and S.FingerprintSet.load(a).spec.nbits == 96


def test_entry_point_option_the_flag_wins_and_absence_changes_nothing():
    base = ['--config', 'c.yml']
    ap = sample_drug3d.add_similarity_argument(sample_drug3d.build_parser())
    assert ap.parse_args(base).similarity is None
    assert ap.parse_args(base + ['--similarity']).similarity is True
    assert ap.parse_args(base + ['--similarity', 'train.npz']).similarity == 'train.npz'
    opt = sample_drug3d.similarity_option
    assert opt(None, {}) == (False, None) and opt(None, {'similarity': False}) == (False, None)
    assert opt(None, {'similarity': True}) == (True, None) and opt(None, {'similarity': 'cfg.npz'}) == (True, 'cfg.npz')
    assert opt(True, {'similarity': 'cfg.npz'}) == (True, None) and opt('flag.npz', {'similarity': 'cfg.npz'}) == (True, 'flag.npz')
    assert opt('flag.npz', {}) == (True, 'flag.npz')
    # every other argument keeps its name and default
    with_flag, without = vars(ap.parse_args(base + ['--similarity'])), vars(ap.parse_args(base))
    assert {k: v for k, v in with_flag.items() if k != 'similarity'} == {k: v for k, v in without.items() if k != 'similarity'}
    assert {k: v for k, v in without.items() if k != 'similarity'} == vars(sample_drug3d.build_parser().parse_args(base))
