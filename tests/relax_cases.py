"""Molecules for the force-field relaxation tests (test_relax_host.py, test_gpu_relax.py): named molecules built on ``hydrogens_cases``, a
seeded random set and the size ladder.  A case is (molecule dict, order, h_count, h_pos, atom_flag): what ``relax_ref`` / ``mdx_mol_relax``
are given, the last three from ``hydrogens.addh_ref``.  References are computed once and shared."""
import functools
import math

import numpy as np

from moldiff_amd import hydrogens, relax
from . import hydrogens_cases as HC
from .hydrogens_cases import AROMATIC, C, CL, DOUBLE, F, N, O, S, SINGLE, TRIPLE, mol

RANDOM_SEED, RANDOM_COUNT = 20240917, 24
DEGENERATE = ('coincident',)
LADDER = (0, 1, 2, 3, 4, 64, 65, 255, 256)


def case(info, n_h=None, order=None, htables=None):
    """the hydrogens of the Kekulé assignment (or the caller's counts) placed by ``addh_ref`` -> (info, order, h_count, h_pos, atom_flag)"""
    h, o = HC.kekule_counts(info)
    n_h, order = (h if n_h is None else np.asarray(n_h, dtype=np.int32)), (o if order is None else np.asarray(order, dtype=np.int32))
    r = hydrogens.addh_ref(info, n_h, order, htables)
    return info, order, r['h_count'], r['h_pos'], r['atom_flag']


def bare(info):
    """the molecule without hydrogens: n_all equals the heavy count"""
    n = len(info['element'])
    _, o = HC.kekule_counts(info)
    return info, o, np.zeros(n, dtype=np.int32), np.zeros((n, 4, 3)), np.zeros(n, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def named():
    """{name: case}"""
    hn = HC.named()
    out = {k: case(*hn[k]) for k in ('ethane', 'propane', 'benzene', 'formamide', 'pyridinium')}
    out['nitrile'] = case(mol([C, C, N], [(-1.5, 0, 0), (0, 0, 0), (1.16, 0.02, 0)], [(0, 1, SINGLE), (1, 2, TRIPLE)]))
    q = 1.0
    out['sulfonamide'] = case(mol([S, C, O, O, N], [(0, 0, 0), (q, q, q), (0.85, -0.85, -0.85), (-0.85, 0.85, -0.85), (-q, -q, q)],
                                  [(0, 1, SINGLE), (0, 2, DOUBLE), (0, 3, DOUBLE), (0, 4, SINGLE)]))
    out['ethane_stretched'] = case(mol([C, C], [(0, 0, 0), (2.0, 0, 0)], [(0, 1, SINGLE)]))
    tb = relax.ForceFieldTables()
    t = lambda z, v=0: tb.type_of[tb.atomic_numbers.index(z), v][0]
    r_ff = tb.pair(t(F), t(F), 0)[0]
    out['f2_at_rest'] = case(mol([F, F], [(0, 0, 0), (np.float32(r_ff), 0, 0)], [(0, 1, SINGLE)]))
    r_ch = tb.pair(t(C), tb.h_type, 0)[0] if t(C) < tb.h_type else tb.pair(tb.h_type, t(C), 0)[0]
    out['methane_ideal'] = case(mol([C], [(0, 0, 0)]), htables=hydrogens.HydrogenTables(xh_length={**hydrogens.DEFAULT_XH_LENGTH, 6: r_ch}))
    out['coincident'] = case(*HC.named()['coincident'])
    return out


def named_lists():
    cases = named()
    names = list(cases)
    return names, [cases[k] for k in names]


def random_mol(rng):
    """a random tree of 4 .. 30 heavy atoms plus up to two ring closures, each atom 1.5 Angstrom from its parent in a direction that
    keeps it 1.3 Angstrom from every earlier atom when one is found, jittered by 0.05 Angstrom"""
    n = int(rng.integers(4, 31))
    while True:
        ele = [int(z) for z in rng.choice([C, C, C, C, N, N, O, O, S, F, CL], size=n)]
        ele[0] = C
        free = [HC.VALENCE[z] for z in ele]
        bonds, ok = [], True
        for j in range(1, n):
            parents = [i for i in range(j) if free[i] >= 1]
            if not parents:
                ok = False
                break
            i = int(rng.choice(parents))
            o = max(1, min(int(rng.choice([1, 1, 1, 1, 1, 1, 1, 2, 2, 3])), free[i], free[j]))
            bonds.append((i, j, o))
            free[i] -= o
            free[j] -= o
        if ok:
            break
    pos = [np.zeros(3)]
    for i, j, _ in bonds:
        for _ in range(60):
            d = rng.normal(size=3)
            p = pos[i] + 1.5 * d / np.linalg.norm(d)
            if all(np.linalg.norm(p - q) >= 1.3 for q in pos):
                break
        pos.append(p)
    have = {(i, j) for i, j, _ in bonds}
    for _ in range(2):
        i, j = sorted(int(x) for x in rng.choice(n, size=2, replace=False))
        if (i, j) not in have and free[i] >= 1 and free[j] >= 1 and np.linalg.norm(pos[i] - pos[j]) < 3.0:
            bonds.append((i, j, SINGLE))
            have.add((i, j))
            free[i] -= 1
            free[j] -= 1
    return mol(ele, np.asarray(pos) + rng.normal(0.0, 0.05, size=(n, 3)), bonds)


@functools.lru_cache(maxsize=None)
def random_set(seed=RANDOM_SEED, count=RANDOM_COUNT):
    rng = np.random.default_rng(seed)
    return [case(random_mol(rng)) for _ in range(count)]


def all_cases():
    """the named cases and then the random set, as one list"""
    return named_lists()[1] + random_set()


@functools.lru_cache(maxsize=None)
def refs(max_iters):
    """``relax_ref`` of every case of ``all_cases`` with its trace, computed once per max_iters -> [(result, trace)]"""
    out = []
    for c in all_cases():
        trace = []
        out.append((relax.relax_ref(*c, max_iters=max_iters, trace=trace), trace))
    return out


@functools.lru_cache(maxsize=None)
def evals():
    """``energy_ref`` of every case of ``all_cases`` at its starting point"""
    return [relax.energy_ref(*c) for c in all_cases()]


@functools.lru_cache(maxsize=None)
def ladder():
    """the size cases without hydrogens, then 254 heavy atoms + 3 hydrogens = 257 atoms"""
    out = [bare(HC.chain(n)) for n in LADDER]
    info, o, hc, hp, fl = bare(HC.chain(254))
    hc[0] = 3
    hp[0, :3] = [(-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0)]
    return out + [(info, o, hc, hp, fl)]


@functools.lru_cache(maxsize=None)
def ladder_refs(max_iters):
    return [relax.relax_ref(*c, max_iters=max_iters) for c in ladder()]


def ideal_methane():
    """(case, tables): methane whose C-H length is the table's rest length, with a table whose tetrahedral carbon angle is acos(-1/3)"""
    import yaml
    with open(relax.DEFAULT_TABLE) as f:
        table = yaml.safe_load(f)
    table['elements'][6]['variants']['tetrahedral']['theta0'] = math.degrees(math.acos(-1.0 / 3.0))
    tb = relax.ForceFieldTables(table=table)
    r_ch = tb.pair(tb.type_of[0, 0][0], tb.h_type, 0)[0]
    return case(mol([C], [(0, 0, 0)]), htables=hydrogens.HydrogenTables(xh_length={**hydrogens.DEFAULT_XH_LENGTH, 6: r_ch})), tb
