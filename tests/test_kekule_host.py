"""Host tests of the Kekulé assignment (moldiff_amd/kekule.py): the plain Python restatement ``kekulize_ref`` against a brute-force
enumeration that knows nothing of the search, the named molecules of the specification, the budget, the tables, the mol block and the
command line.  No GPU."""
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

from moldiff_amd import kekule as K
from moldiff_amd import molpack
from .util import run_host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mol(ele, bonds, pos=False):
    ele = [6] * ele if isinstance(ele, int) else ele
    bonds = [tuple(b) + (1,) * (3 - len(b)) for b in bonds]
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    out = {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
           'bond_type': np.asarray(bt + bt, dtype=np.int64)}
    if pos:
        out['atom_pos'] = (np.arange(3 * len(ele), dtype=np.float32).reshape(-1, 3) * 0.25 - 1.5)
    return out


def ring(n, first=0, t=4):
    return [(first + k, first + (k + 1) % n, t) for k in range(n)]


def grid(X, Y):
    """the brick-wall grid: atom (x, y) at index x * Y + y, bonds (x, y)-(x + 1, y) always and (x, y)-(x, y + 1) when x + y is even"""
    bonds = []
    for x in range(X):
        for y in range(Y):
            if x + 1 < X:
                bonds.append((x * Y + y, (x + 1) * Y + y, 4))
            if y + 1 < Y and (x + y) % 2 == 0:
                bonds.append((x * Y + y, x * Y + y + 1, 4))
    return mol(X * Y, bonds)


# atoms in ring order with the heteroatom first
NAMED = {
    'benzene': mol(6, ring(6)),
    'pyridine': mol([7] + [6] * 5, ring(6)),
    'pyrrole': mol([7] + [6] * 4, ring(5)),
    'thiophene': mol([16] + [6] * 4, ring(5)),
    'imidazole': mol([7, 6, 7, 6, 6], ring(5)),
    'n_methylpyrrole': mol([7] + [6] * 5, ring(5) + [(0, 5, 1)]),
    'furan': mol([8] + [6] * 4, ring(5)),
    'pyridone': mol([7] + [6] * 5 + [8], ring(6) + [(1, 6, 2)]),
    'n_methylpyridinium': mol([7] + [6] * 6, ring(6) + [(0, 6, 1)]),
    'naphthalene': mol(10, ring(10) + [(0, 5, 4)]),
    'azulene': mol(10, ring(10) + [(0, 4, 4)]),
    'indole': mol([7] + [6] * 8, ring(9) + [(3, 8, 4)]),
    'ring5': mol(5, ring(5)),
    'ring7': mol(7, ring(7)),
    'ring4': mol(4, ring(4)),
}


def doubles(m, r):
    nb = m['bond_index'].shape[1] // 2
    return [(int(m['bond_index'][0, e]), int(m['bond_index'][1, e])) for e in range(nb) if m['bond_type'][e] == 4 and r['kek_order'][e] == 2]


def random_aromatic(seed, n_min=3, n_max=24):
    """a random graph of n_min .. n_max atoms: a chain with branches (atom k hangs on k - 1, one time in ten on any earlier atom) and a
    few ring closures over 4 or 5 bonds; a C-heavy mix of C, N, O, S, an aromatic-heavy mix of the types 4, 1, 2"""
    g = np.random.default_rng(seed)
    n = int(g.integers(n_min, n_max + 1))
    bonds = {(k - 1 if g.random() >= 0.1 else int(g.integers(0, k)), k) for k in range(1, n)}
    for _ in range(int(g.integers(0, n // 5 + 1))):
        i = int(g.integers(0, n))
        j = i + int(g.choice([4, 5]))
        if j < n:
            bonds.add((i, j))
    ele = g.choice([6, 7, 8, 16], n, p=[0.7, 0.15, 0.08, 0.07])
    bt = g.choice([4, 1, 2], len(bonds), p=[0.7, 0.2, 0.1])
    return mol(ele, [(i, j, int(t)) for (i, j), t in zip(sorted(bonds), bt)])


def brute_force_feasible(m, tables):
    """whether SOME set of aromatic bonds is a Kekulé structure of the whole molecule, by enumeration of all subsets: roles from the
    definition, no search order anywhere"""
    cls = [tables.atomic_numbers.index(int(z)) for z in m['element']]
    n, nb = len(cls), m['bond_index'].shape[1] // 2
    sigma, adeg, arom = [0] * n, [0] * n, []
    for e in range(nb):
        i, j, t = int(m['bond_index'][0, e]), int(m['bond_index'][1, e]), int(m['bond_type'][e])
        for a in (i, j):
            sigma[a] += 1 if t == 4 else t
            adeg[a] += t == 4
        if t == 4:
            arom.append((i, j))
    assert len(arom) <= 12
    V, Vc = [int(tables.normal_valence[c]) for c in cls], [int(tables.charged_valence[c]) for c in cls]
    flex = [bool(tables.flexible >> c & 1) for c in cls]
    NOT, MUST, MAY = 1, 2, 3
    role = {}
    for a in range(n):
        if adeg[a] == 0:
            continue
        if adeg[a] > 3:
            role[a] = NOT
        elif V[a] - sigma[a] >= 1:
            role[a] = MAY if flex[a] else MUST
        else:
            role[a] = MAY if Vc[a] - sigma[a] >= 1 else NOT
    must = {a for a, r in role.items() if r == MUST}
    for k in range(len(arom) + 1):
        for chosen in itertools.combinations(arom, k):
            ends = [a for b in chosen for a in b]
            if len(set(ends)) == len(ends) and all(role[a] != NOT for a in ends) and must <= set(ends):
                return True
    return False


def test_feasibility_equals_a_brute_force_enumeration_on_random_graphs():
    tables = K.KekuleTables()
    seen, feasible = 0, 0
    for seed in range(600):
        m = random_aromatic(seed, 3, 14)
        if int((m['bond_type'][:m['bond_index'].shape[1] // 2] == 4).sum()) > 12:
            continue
        r = K.kekulize_ref(m, tables)
        want = brute_force_feasible(m, tables)
        assert r['status'] == 0 and r['n_over_budget'] == 0
        assert bool(K.kekulizable(r)) == want, seed
        seen, feasible = seen + 1, feasible + want
    assert seen >= 300 and 0.2 * seen < feasible < 0.8 * seen, (seen, feasible)


def test_the_named_molecules_give_the_outcomes_of_the_specification():
    R = {k: K.kekulize_ref(m) for k, m in NAMED.items()}
    D = {k: doubles(NAMED[k], R[k]) for k in NAMED}
    role = lambda k, a: int(R[k]['atom_flag'][a]) & 3
    matched = lambda k, a: bool(R[k]['atom_flag'][a] & K.FLAG_MATCHED)
    assert all(K.kekulizable(R[k]) for k in NAMED if k not in ('ring5', 'ring7'))
    assert D['benzene'] == [(0, 1), (2, 3), (4, 5)] and R['benzene']['steps'] == 3 and R['benzene']['n_double'] == 3
    assert matched('pyridine', 0) and R['pyridine']['steps'] == 6 and R['pyridine']['n_charged'] == 0 and D['pyridine'] == [(0, 1), (2, 3), (4, 5)]
    for k in ('pyrrole', 'thiophene', 'imidazole', 'n_methylpyrrole'):
        assert D[k] == [(1, 2), (3, 4)] and R[k]['steps'] == 3 and R[k]['n_charged'] == 0, k
    assert R['pyrrole']['kek_h'][0] == 1 and R['n_methylpyrrole']['kek_h'][0] == 0 and R['n_methylpyrrole']['charge'][0] == 0
    assert R['thiophene']['kek_h'].tolist() == [0, 1, 1, 1, 1] and R['imidazole']['kek_h'].tolist() == [1, 1, 0, 1, 1]
    assert role('furan', 0) == K.ROLE_NOT and R['furan']['steps'] == 2 and D['furan'] == [(1, 2), (3, 4)]
    assert role('pyridone', 1) == K.ROLE_NOT and not matched('pyridone', 0) and R['pyridone']['kek_h'][0] == 1
    assert D['pyridone'] == [(2, 3), (4, 5)] and R['pyridone']['kek_order'].tolist() == [1, 1, 2, 1, 2, 1, 2]
    assert matched('n_methylpyridinium', 0) and R['n_methylpyridinium']['charge'].tolist() == [1, 0, 0, 0, 0, 0, 0]
    assert R['n_methylpyridinium']['n_charged'] == 1 and R['n_methylpyridinium']['val'][0] == 4 and R['n_methylpyridinium']['kek_h'][0] == 0
    for k in ('naphthalene', 'azulene', 'indole'):
        assert R[k]['steps'] == 5 and R[k]['n_failed'] == 0, k
    assert R['naphthalene']['n_double'] == 5 and R['indole']['n_double'] == 4 and R['indole']['kek_h'][0] == 1
    for k, steps in (('ring5', 4), ('ring7', 6)):
        r = R[k]
        assert (r['n_failed'], r['steps'], r['n_double'], r['n_hydrogens']) == (1, steps, 0, 0) and not K.kekulizable(r), k
        assert (r['kek_order'] == 0).all() and (r['atom_flag'] == (K.ROLE_MUST | K.FLAG_UNSOLVED)).all() and (r['val'] == 2).all()
    assert R['ring4']['steps'] == 2 and R['ring4']['n_failed'] == 0 and D['ring4'] == [(0, 1), (2, 3)]
    # benzene, every number
    r = R['benzene']
    assert {k: r[k] for k in K.STAT_KEYS} == {'status': 0, 'n_arom_atoms': 6, 'n_arom_bonds': 6, 'n_components': 1, 'n_failed': 0,
                                              'n_over_budget': 0, 'n_double': 3, 'n_charged': 0, 'n_hydrogens': 6, 'n_overvalent': 0, 'steps': 3}
    assert (r['val'] == 3).all() and (r['atom_flag'] == (K.ROLE_MUST | K.FLAG_MATCHED)).all()


def test_roles_ignored_bonds_and_unusual_types():
    # an atom with four aromatic bonds is NOT whatever its valence allows; the four arms are single atoms that must be matched and cannot
    star = mol(5, [(0, 1, 4), (0, 2, 4), (0, 3, 4), (0, 4, 4)])
    r = K.kekulize_ref(star)
    assert int(r['atom_flag'][0]) & 3 == K.ROLE_NOT and r['n_components'] == 1 and r['n_failed'] == 1 and r['steps'] == 0
    assert r['n_overvalent'] == 0 and r['val'].tolist() == [4, 1, 1, 1, 1]
    # ignored bonds (an index outside the molecule, i = j) change nothing but their own kek_order
    base = NAMED['pyridine']
    noisy = mol([7] + [6] * 5, [(0, 9, 4), (2, 2, 4)] + ring(6) + [(-1, 3, 2)])
    a, b = K.kekulize_ref(base), K.kekulize_ref(noisy)
    assert all(a[k] == b[k] for k in K.STAT_KEYS) and all(np.array_equal(a[k], b[k]) for k in K.ATOM_KEYS)
    assert b['kek_order'].tolist() == [0, 0] + a['kek_order'].tolist() + [0] and b['n_bonds'] == 9
    # a bond type outside 1 .. 4 stays in the graph, adds nothing and is not aromatic
    r = K.kekulize_ref(mol([6, 8], [(0, 1, 7)]))
    assert r['kek_order'].tolist() == [0] and r['val'].tolist() == [0, 0] and r['kek_h'].tolist() == [4, 2] and r['n_arom_bonds'] == 0
    # a non-aromatic four-valent nitrogen gets its charge; a five-valent one is over-valent
    r = K.kekulize_ref(mol([7, 6, 6, 6, 6], [(0, 1), (0, 2), (0, 3), (0, 4)]))
    assert r['charge'].tolist() == [1, 0, 0, 0, 0] and r['kek_h'].tolist() == [0, 3, 3, 3, 3] and r['n_components'] == 0 and K.kekulizable(r)
    r = K.kekulize_ref(mol([7, 6, 6, 6, 6], [(0, 1, 2), (0, 2), (0, 3), (0, 4)]))
    assert r['n_overvalent'] == 1 and int(r['atom_flag'][0]) == K.FLAG_OVERVALENT and r['charge'][0] == 0
    # three components, one of them without a structure: the others are assigned, the flag marks the failed ring alone
    three = mol(6 + 5 + 6, ring(6) + ring(5, 6) + ring(6, 11) + [(5, 6, 1), (10, 11, 1)])
    r = K.kekulize_ref(three)
    assert (r['n_components'], r['n_failed'], r['n_double'], r['steps']) == (3, 1, 6, 3 + 4 + 3) and not K.kekulizable(r)
    assert ((r['atom_flag'] & K.FLAG_UNSOLVED) != 0).tolist() == [False] * 6 + [True] * 5 + [False] * 6
    # sizes: 257 atoms, 513 bonds, an aromatic component of 65 atoms; 64 are measured
    for m, status in ((mol(257, [(k, k + 1) for k in range(256)]), 1), (mol(65, [(k, k + 1, 4) for k in range(64)]), 1),
                      (mol(64, [(k, k + 1, 4) for k in range(63)]), 0)):
        r = K.kekulize_ref(m)
        assert r['status'] == status
        if status:
            assert all(r[k] == 0 for k in K.STAT_KEYS[1:]) and not any(r[k].any() for k in K.ATOM_KEYS + K.BOND_KEYS)
    assert K.kekulize_ref(mol(64, [(k, k + 1, 4) for k in range(63)]))['n_double'] == 32
    with pytest.raises(ValueError, match='same pair'):
        K.kekulize_ref(mol(3, [(0, 1, 4), (1, 2, 4), (1, 0, 4)]))
    with pytest.raises(ValueError, match='element'):
        K.kekulize_ref(mol([6, 5], [(0, 1)]))


def test_table_validation():
    t = K.KekuleTables()
    assert t.normal_valence.tolist() == [4, 3, 2, 1, 3, 2, 1] and t.charged_valence.tolist() == [0, 4, 0, 0, 0, 3, 0] and t.flexible == 2
    from moldiff_amd import groups
    assert K.DEFAULT_NORMAL_VALENCE == groups.DEFAULT_NORMAL_VALENCE
    with pytest.raises(ValueError, match='no normal valence'):
        K.KekuleTables(normal_valence={6: 4})
    with pytest.raises(ValueError, match='0 .. 64'):
        K.KekuleTables(normal_valence={**K.DEFAULT_NORMAL_VALENCE, 6: 65})
    with pytest.raises(ValueError, match='0 .. 64'):
        K.KekuleTables(charged_valence={7: -1})
    with pytest.raises(ValueError, match='outside the atomic numbers'):
        K.KekuleTables(flexible=(5,))
    with pytest.raises(ValueError, match='elements'):
        K.KekuleTables(atomic_numbers=range(1, 34))
    with pytest.raises(ValueError, match='max_steps'):
        K.kekulize_ref(NAMED['benzene'], max_steps=0)
    with pytest.raises(ValueError, match='max_steps'):
        K.kekulize_ref(NAMED['benzene'], max_steps=(1 << 20) + 1)
    # other tables, other outcomes: without the flexible bit pyrrole's N must be matched and the ring has no structure; an oxygen
    # with a charged valence makes furan's O a MAY atom
    stiff = K.KekuleTables(flexible=())
    assert K.kekulize_ref(NAMED['pyrrole'], stiff)['n_failed'] == 1
    oxo = K.kekulize_ref(NAMED['furan'], K.KekuleTables(charged_valence={7: 4, 8: 3, 16: 3}))
    assert int(oxo['atom_flag'][0]) & 3 == K.ROLE_MAY and oxo['steps'] == 3


def test_budget_threshold_on_the_brick_wall_grids():
    g88, g79 = grid(8, 8), grid(7, 9)
    r = K.kekulize_ref(g88, max_steps=1 << 20)
    S = int(r['steps'])
    assert S == 28584 and r['n_failed'] == 0 and r['n_double'] == 32 and K.kekulizable(r)
    at = K.kekulize_ref(g88, max_steps=S)
    assert at['steps'] == S and at['n_over_budget'] == 0 and np.array_equal(at['kek_order'], r['kek_order'])
    below = K.kekulize_ref(g88, max_steps=S - 1)
    assert (below['n_over_budget'], below['n_failed'], below['steps'], below['n_double']) == (1, 0, 0, 0) and not K.kekulizable(below)
    assert (below['kek_order'] == 0).all() and ((below['atom_flag'] & K.FLAG_UNSOLVED) != 0).all()
    r = K.kekulize_ref(g79, max_steps=1 << 20)
    assert (r['n_failed'], r['steps'], r['n_over_budget']) == (1, 14501, 0)


def test_mol_block_round_trip_formula_and_weight():
    from moldiff_amd.sample_drug3d import mol_block, read_mol_block
    m = mol([7] + [6] * 6, ring(6) + [(0, 6, 1)], pos=True)                      # N-methylpyridinium
    r = K.kekulize_ref(m)
    text = K.kekule_mol_block(m, r)
    back = read_mol_block(text)
    assert np.array_equal(back['element'], m['element']) and np.array_equal(back['bond_index'], m['bond_index'])
    assert np.allclose(back['atom_pos'], m['atom_pos'], atol=1e-4)
    assert back['bond_type'].tolist() == r['kek_order'].tolist() * 2 and 4 not in back['bond_type'] and set(back['bond_type']) == {1, 2}
    assert 'M  CHG  1   1   1\n' in text and K.read_charges(text) == {0: 1} and text.endswith('M  END\n')
    assert read_mol_block(mol_block(m))['bond_type'].tolist() == m['bond_type'].tolist()      # the aromatic form is what it was
    # the block read back is a molecule without aromatic bonds with the same hydrogens and charges
    again = K.kekulize_ref(back)
    assert again['n_arom_bonds'] == 0 and np.array_equal(again['kek_h'], r['kek_h']) and np.array_equal(again['charge'], r['charge'])
    many = mol([7] * 9 + [6] * 36, [(k, 9 + 4 * k + q) for k in range(9) for q in range(4)], pos=True)   # nine ammonium centres
    text = K.kekule_mol_block(many, K.kekulize_ref(many))
    assert K.read_charges(text) == {k: 1 for k in range(9)} and len([ln for ln in text.splitlines() if ln.startswith('M  CHG')]) == 2
    with pytest.raises(ValueError, match='not kekulizable'):
        K.kekule_mol_block(mol(5, ring(5), pos=True), K.kekulize_ref(NAMED['ring5']))
    p = K.kekulize_ref(NAMED['pyridine'])
    assert K.formula(NAMED['pyridine']['element'], p['n_hydrogens']) == 'C5H5N'
    assert K.weight(NAMED['pyridine']['element'], p['n_hydrogens']) == pytest.approx(5 * 12.011 + 5 * 1.008 + 14.007, abs=1e-9)
    assert K.formula(m['element'], r['n_hydrogens'], r['n_charged']) == 'C6H8N+' and K.formula([8, 8], 2) == 'H2O2'
    assert K.formula([17, 6, 16], 3) == 'CH3ClS'
    with pytest.raises(ValueError, match='atomic weight'):
        K.weight([5], 0)


def test_stack_summary_compare_concat_and_the_command_line(tmp_path, capsys):
    mols = [NAMED['benzene'], NAMED['n_methylpyridinium'], NAMED['ring5'], mol(257, [(k, k + 1) for k in range(256)]), mol(0, [])]
    a = K.stack_ref(mols)
    assert a['status'].tolist() == [0, 0, 0, 1, 0] and a['atom_ptr'].tolist() == [0, 6, 13, 18, 275] and a['bond_ptr'].tolist() == [0, 6, 13, 18, 274]
    assert all(a[k].dtype == np.int32 for k in a) and K.kekulizable(a).tolist() == [True, True, False, False, True]
    assert {k: K.mol_result(a, 1)[k] for k in K.STAT_KEYS} == {k: K.kekulize_ref(mols[1])[k] for k in K.STAT_KEYS}
    s = K.summary(a)
    assert (s['n_molecules'], s['n_measured'], s['n_too_large'], s['n_kekulizable'], s['n_no_structure'], s['n_over_budget']) == (5, 4, 1, 3, 1, 0)
    assert s['fraction_kekulizable'] == 0.6 and s['fraction_charged'] == 1 / 3 and s['mean_hydrogens'] == 14 / 3 and s['charged_hist'] == [2, 1, 0, 0, 0]
    assert s['steps_hist'][:4] == [1, 0, 1, 2] and sum(s['steps_hist']) == 4 and len(s['steps_hist']) == K.STEP_BINS
    joined = K.concat([K.stack_ref(mols[:2]), K.stack_ref(mols[2:])])
    assert set(joined) == set(a) and all(np.array_equal(joined[k], a[k]) for k in a)
    e = K.empty()
    assert set(e) == set(a) and all(len(v) == 0 for v in e.values()) and K.summary(e)['n_molecules'] == 0
    c = K.compare(a, K.stack_ref(mols[:1]))
    assert 0 < c['steps'] <= 1 and c['fraction_kekulizable'] == [0.6, 1.0] and K.compare(a, a)['charged'] == 0.0
    pool = {'finished': [dict(m, atom_pos=np.zeros((len(m['element']), 3), dtype=np.float32)) for m in mols[:3]], 'failed': [mols[0]]}
    torch.save(pool, str(tmp_path / 'samples_all.pt'))
    assert K.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'a.npz'), '--sdf', str(tmp_path / 'a.sdf'), '--ref']) == 0
    printed = json.loads(capsys.readouterr().out)
    assert printed['n_kekulizable'] == 2 and printed['n_no_structure'] == 1
    saved, want = molpack.load_npz(str(tmp_path / 'a.npz')), K.stack_ref(pool['finished'])
    assert set(saved) == set(want) and all(np.array_equal(saved[k], want[k]) for k in want)
    from moldiff_amd.sample_drug3d import read_mol_block
    blocks = [b for b in open(tmp_path / 'a.sdf').read().split('$$$$\n') if b.strip()]
    assert len(blocks) == 2 and all(4 not in read_mol_block(b)['bond_type'] for b in blocks)
    assert K.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'b.npz'), '--ref', '--part', 'failed']) == 0
    capsys.readouterr()
    assert K.main(['compare', str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')]) == 0
    assert json.loads(capsys.readouterr().out)['fraction_kekulizable'] == [2 / 3, 1.0]


def test_header_exports_and_binding_agree():
    import ctypes
    from moldiff_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'moldiff_hip.h')).read()
    proto = re.search(r'\bint mdx_mol_kekulize\(([^;]*)\);', hdr).group(1)
    params = [p.strip() for p in proto.replace('\n', ' ').split(',')]
    assert len(params) == 24 and params[0] == 'int32_t B' and params[-1] == 'void* stream' and params[15] == 'uint32_t flexible'
    groups_proto = re.search(r'\bint mdx_mol_groups\(([^;]*)\);', hdr).group(1)
    assert params[:11] == [p.strip() for p in groups_proto.replace('\n', ' ').split(',')][:11]      # the leading operands through select
    assert 'mdx_mol_kekulize' in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, 'mdx_mol_kekulize') and len(L.mdx_mol_kekulize.argtypes) == 24
    width = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32}
    for p, t in zip(params, L.mdx_mol_kekulize.argtypes):
        assert t is (ctypes.c_void_p if '*' in p else width[p.split()[0]]), p
    assert re.search(rf'#define MDX_KEKULE_STATS {len(K.STAT_KEYS)}\b', hdr)
    for k, name in enumerate(K.STAT_KEYS):                        # the header lists the columns in the order of STAT_KEYS
        assert re.search(rf'\b{k} {name}\b', hdr), name
    with open(os.path.join(ROOT, 'moldiff_amd', 'csrc', 'Makefile')) as f:
        text = f.read()
    assert 'mdx_kekule.o' in text and 'mdx_kekule_args.h' in text


def test_kekulize_argument_and_the_acceptance_rule():
    from moldiff_amd import molcheck, sample_drug3d
    options = lambda ap: sorted(s for a in ap._actions for s in a.option_strings)
    before = options(sample_drug3d.build_parser())
    ap = sample_drug3d.add_kekulize_argument(sample_drug3d.build_parser())
    assert options(sample_drug3d.build_parser()) == before and '--kekulize' not in before
    assert sorted(set(options(ap)) - set(before)) == ['--kekulize']
    base = ['--config', 'c.yml']
    assert ap.parse_args(base).kekulize is None and ap.parse_args(base + ['--kekulize']).kekulize is True
    assert {k: v for k, v in vars(ap.parse_args(base)).items() if k != 'kekulize'} == vars(sample_drug3d.build_parser().parse_args(base))
    opt = sample_drug3d.kekulize_option
    assert not opt(None, {}) and opt(True, {}) and opt(None, {'kekulize': True}) and not opt(None, {'kekulize': False})
    assert molcheck.ACCEPT_RULES == ('connected', 'valence', 'kekule') and molcheck.accept_rule('kekule') == 'kekule'
    assert sample_drug3d.quality_options('kekule', None, {}) == ('kekule', None, True)
    rows = [dict(n_components=1, n_overvalent=0, min_dist=1.0, max_bond_len=1.5, salvaged=False, kekulizable=k) for k in (True, False, True)]
    plain, with_k = molcheck.quality_summary(rows, 2, 1), molcheck.quality_summary(rows, 2, 1, kekule=True)
    assert 'kekulizable' not in plain['counts'] and with_k['counts']['kekulizable'] == 2 and with_k['fractions']['kekulizable'] == 2 / 3
    assert {k: v for k, v in with_k['counts'].items() if k != 'kekulizable'} == plain['counts']
    assert 'there is no kekulisation' not in molcheck.__doc__ and 'mdx_mol_kekulize' in molcheck.__doc__


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/kekule_host_check.cpp over csrc/mdx_kekule_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('kekule_host_check', tmp_path)
