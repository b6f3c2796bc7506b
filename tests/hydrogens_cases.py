"""Molecules for the explicit-hydrogen tests (test_hydrogens_host.py, test_gpu_hydrogens.py): named molecules with exact coordinates, so
that the degenerate cases are exactly degenerate, and a seeded random set.  A case is (name, molecule dict, n_h, order): the hydrogen
count per atom and the order per bond that ``addh_ref`` / ``mdx_mol_hydrogens`` are given."""
import functools
import math

import numpy as np

from moldiff_amd import hydrogens, kekule

C, N, O, F, S, CL = 6, 7, 8, 9, 16, 17
SINGLE, DOUBLE, TRIPLE, AROMATIC = 1, 2, 3, 4
RANDOM_SEED, RANDOM_COUNT = 20240611, 256


def mol(elements, pos, bonds=()):
    """molecule dict from atomic numbers, (n, 3) coordinates and (i, j, type) bonds: every bond once and then flipped"""
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(elements, dtype=np.int64), 'atom_pos': np.asarray(pos, dtype=np.float32).reshape(len(elements), 3),
            'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def kekule_counts(info):
    """(n_h, order) of the Kekulé assignment with the default chemistry"""
    r = kekule.kekulize_ref(info)
    return r['kek_h'].copy(), r['kek_order'].copy()


def _ring(n, radius):
    return [(radius * math.cos(2.0 * math.pi * k / n), radius * math.sin(2.0 * math.pi * k / n), 0.0) for k in range(n)]


def _cycle(n, t):
    return [(k, (k + 1) % n, t) for k in range(n)]


@functools.lru_cache(maxsize=None)
def named():
    """{name: (molecule, n_h, order)}"""
    out = {}

    def add(name, info, n_h=None, order=None):
        h, o = kekule_counts(info)
        out[name] = (info, h if n_h is None else np.asarray(n_h, dtype=np.int32), o if order is None else np.asarray(order, dtype=np.int32))
    add('methane', mol([C], [(0, 0, 0)]))
    add('ammonia', mol([N], [(0.5, -0.25, 1.0)]))
    add('water', mol([O], [(0, 0, 0)]))
    add('ethane', mol([C, C], [(0, 0, 0), (1.5, 0, 0)], [(0, 1, SINGLE)]))
    add('ethene', mol([C, C], [(0, 0, 0), (0, 1.25, 0)], [(0, 1, DOUBLE)]))
    add('ethyne', mol([C, C], [(0, 0, 0), (0, 0, 1.25)], [(0, 1, TRIPLE)]))
    add('hcn', mol([C, N], [(0, 0, 0), (1.25, 0, 0)], [(0, 1, TRIPLE)]))
    add('methanol', mol([C, O], [(0, 0, 0), (1.5, 0, 0)], [(0, 1, SINGLE)]))
    add('methylamine', mol([C, N], [(0, 0, 0), (0, 1.5, 0)], [(0, 1, SINGLE)]))
    add('dimethylamine', mol([N, C, C], [(0, 0, 0), (1.25, 0.5, 0), (-1.25, 0.5, 0)], [(0, 1, SINGLE), (0, 2, SINGLE)]))
    add('formamide', mol([C, O, N], [(0, 0, 0), (0, 1.25, 0), (1.25, -0.5, 0)], [(0, 1, DOUBLE), (0, 2, SINGLE)]))
    add('benzene', mol([C] * 6, _ring(6, 1.5), _cycle(6, AROMATIC)))
    add('pyrrole', mol([N, C, C, C, C], _ring(5, 1.25), _cycle(5, AROMATIC)))
    pyridinium = mol([N, C, C, C, C, C], _ring(6, 1.5), _cycle(6, AROMATIC))
    h, _ = kekule_counts(pyridinium)
    h[0] = 1                                                       # the N-H of the cation: the caller's count, not the assignment's
    add('pyridinium', pyridinium, n_h=h)
    add('propane', mol([C, C, C], [(-1.25, -0.75, 0), (0, 0, 0), (1.25, -0.75, 0)], [(0, 1, SINGLE), (1, 2, SINGLE)]))
    add('isobutane', mol([C, C, C, C], [(0, 0, 0), (1, 1, 1), (1, -1, -1), (-1, 1, -1)], [(0, 1, SINGLE), (0, 2, SINGLE), (0, 3, SINGLE)]))
    y = 1.5 * math.sqrt(3.0) / 2.0
    add('flat_ch', mol([C, C, C, C], [(0, 0, 0), (1.5, 0, 0), (-0.75, y, 0), (-0.75, -y, 0)], [(0, 1, SINGLE), (0, 2, SINGLE), (0, 3, SINGLE)]))
    add('collinear_ch2', mol([C, C, C], [(0, 0, 0), (1.5, 0, 0), (-1.5, 0, 0)], [(0, 1, SINGLE), (0, 2, SINGLE)]))
    neo = mol([C] * 5, [(0, 0, 0), (1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], [(0, k, SINGLE) for k in range(1, 5)])
    add('no_room', neo, n_h=[1, 3, 3, 3, 3])
    add('clamped', mol([C], [(1, 2, 3)]), n_h=[7])
    add('coincident', mol([C, C], [(0.5, 0.5, 0.5), (0.5, 0.5, 0.5)], [(0, 1, SINGLE)]))
    add('bad_bond', mol([C, C], [(0, 0, 0), (0, 0, 1.5)], [(0, 1, SINGLE), (0, 5, SINGLE)]), n_h=[3, 3], order=[1, 1])
    return out


def named_lists():
    """the named cases as parallel lists: names, molecules, n_h arrays, order arrays"""
    cases = named()
    names = list(cases)
    return names, [cases[k][0] for k in names], [cases[k][1] for k in names], [cases[k][2] for k in names]


VALENCE = {C: 4, N: 3, O: 2, F: 1, S: 2, CL: 1}


def random_mol(rng):
    """a random tree of 2 .. 24 atoms plus up to two ring closures, the orders within the default valences, Gaussian coordinates"""
    n = int(rng.integers(2, 25))
    while True:
        ele = [int(z) for z in rng.choice([C, C, C, C, N, N, O, O, S, F, CL], size=n)]
        ele[0] = C
        free = [VALENCE[z] for z in ele]
        bonds, ok = [], True
        for j in range(1, n):
            parents = [i for i in range(j) if free[i] >= 1]
            if not parents:
                ok = False
                break
            i = int(rng.choice(parents))
            o = int(rng.choice([1, 1, 1, 1, 1, 1, 1, 2, 2, 3]))
            o = max(1, min(o, free[i], free[j]))
            bonds.append((i, j, o))
            free[i] -= o
            free[j] -= o
        if ok:
            break
    have = {(i, j) for i, j, _ in bonds}
    for _ in range(2):
        i, j = sorted(int(x) for x in rng.choice(n, size=2, replace=False)) if n > 2 else (0, 0)
        if i != j and (i, j) not in have and free[i] >= 1 and free[j] >= 1:
            bonds.append((i, j, SINGLE))
            have.add((i, j))
            free[i] -= 1
            free[j] -= 1
    return mol(ele, rng.normal(0.0, 1.5, size=(n, 3)), bonds)


@functools.lru_cache(maxsize=None)
def random_set(seed=RANDOM_SEED, count=RANDOM_COUNT):
    """(molecules, n_h arrays, order arrays) of the seeded random set"""
    rng = np.random.default_rng(seed)
    mols = [random_mol(rng) for _ in range(count)]
    counts = [kekule_counts(m) for m in mols]
    return mols, [c[0] for c in counts], [c[1] for c in counts]


@functools.lru_cache(maxsize=None)
def named_ref():
    """``stack_ref`` of the named cases, computed once"""
    _, mols, n_h, order = named_lists()
    return hydrogens.stack_ref(mols, n_h, order)


@functools.lru_cache(maxsize=None)
def random_ref():
    """``stack_ref`` of the random set, computed once"""
    mols, n_h, order = random_set()
    return hydrogens.stack_ref(mols, n_h, order)


def chain(n_atoms):
    """an unbranched carbon chain of `n_atoms` atoms on a zig-zag: the size cases"""
    pos = [(1.25 * k, 0.75 * (k & 1), 0.0) for k in range(n_atoms)]
    return mol([C] * n_atoms, pos, [(k, k + 1, SINGLE) for k in range(n_atoms - 1)])
