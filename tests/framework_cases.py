"""Cases for the tests of the frameworks and ring systems (test_framework_host.py, test_gpu_framework.py): named molecules whose
pieces are known by hand, the caps, and seeded random sparse graphs."""
import numpy as np

from .canon_cases import CUBE, chain, mol, permuted, ring


def _fused_chain(rings_, extra=0):
    """a linear chain of `rings_` fused six-rings (4 k + 2 atoms, 5 k + 1 bonds) with `extra` atoms in a side chain on atom 0"""
    n = 4 * rings_ + 2
    top, bottom = list(range(0, n, 2)), list(range(1, n, 2))
    bonds = [(top[k], top[k + 1]) for k in range(len(top) - 1)] + [(bottom[k], bottom[k + 1]) for k in range(len(bottom) - 1)]
    bonds += [(top[k], bottom[k]) for k in range(0, len(top), 2)]
    bonds += [(n + k - 1 if k else 0, n + k) for k in range(extra)]
    return mol(n + extra, bonds)


def _ladder(rungs):
    return mol(2 * rungs, [(2 * k, 2 * k + 1) for k in range(rungs)] + [(2 * k, 2 * k + 2) for k in range(rungs - 1)] +
               [(2 * k + 1, 2 * k + 3) for k in range(rungs - 1)])


BENZENE = ring(6, t=4)
TWO_PHENYLS = BENZENE + ring(6, 6, t=4)
CASES = {
    'propane': chain(3),
    'benzene': mol(6, BENZENE),
    'toluene': mol(7, BENZENE + [(0, 6)]),
    'ethylbenzene': mol(8, BENZENE + [(0, 6), (6, 7)]),
    'biphenyl': mol(12, TWO_PHENYLS + [(0, 6)]),
    'diphenylmethane': mol(13, TWO_PHENYLS + [(0, 12), (12, 6)]),
    'methyl_diphenylmethane': mol(14, TWO_PHENYLS + [(0, 12), (12, 6), (12, 13)]),
    'spiro_nonane': mol(9, ring(5) + [(0, 5), (5, 6), (6, 7), (7, 8), (8, 0)]),
    'naphthalene': mol(10, ring(10, t=4) + [(0, 5, 4)]),
    'cubane': mol(8, CUBE),
    'cyclohexanone': mol([6] * 6 + [8], ring(6) + [(0, 6, 2)]),
    'acetone': mol([6, 8, 6, 6], [(0, 1, 2), (0, 2), (0, 3)]),
    'pyridine': mol([7] + [6] * 5, BENZENE),
    'two_fragments': mol([6] * 6 + [6] * 5 + [8, 6], BENZENE + ring(5, 6) + [(6, 11, 2), (8, 12)]),
    'macrocycle': mol(12, ring(12)),
    'ignored_bonds': mol(8, [(0, 9), (3, 3, 2)] + ring(6) + [(-1, 2), (0, 6), (6, 7, 2)]),
    'fused_256': _fused_chain(63, extra=2),
    'chain_257': chain(257),
    'ladder_65_rings': _ladder(66),
}
# name -> (status, framework atoms, framework bonds, systems, linker, side, exo, fusion, largest system, most rings) without EXO
EXPECTED = {
    'propane': (0, 0, 0, 0, 0, 3, 0, 0, 0, 0),
    'benzene': (0, 6, 6, 1, 0, 0, 0, 0, 6, 1),
    'toluene': (0, 6, 6, 1, 0, 1, 0, 0, 6, 1),
    'ethylbenzene': (0, 6, 6, 1, 0, 2, 0, 0, 6, 1),
    'biphenyl': (0, 12, 13, 2, 0, 0, 0, 0, 6, 1),
    'diphenylmethane': (0, 13, 14, 2, 1, 0, 0, 0, 6, 1),
    'methyl_diphenylmethane': (0, 13, 14, 2, 1, 1, 0, 0, 6, 1),
    'spiro_nonane': (0, 9, 10, 1, 0, 0, 0, 1, 9, 2),
    'naphthalene': (0, 10, 11, 1, 0, 0, 0, 2, 10, 2),
    'cubane': (0, 8, 12, 1, 0, 0, 0, 8, 8, 5),
    'cyclohexanone': (0, 6, 6, 1, 0, 1, 0, 0, 6, 1),
    'acetone': (0, 0, 0, 0, 0, 4, 0, 0, 0, 0),
    'pyridine': (0, 6, 6, 1, 0, 0, 0, 0, 6, 1),
    'two_fragments': (0, 11, 11, 2, 0, 2, 0, 0, 6, 1),
    'macrocycle': (0, 12, 12, 1, 0, 0, 0, 0, 12, 1),
    'ignored_bonds': (0, 6, 6, 1, 0, 2, 0, 0, 6, 1),
    'fused_256': (0, 254, 316, 1, 0, 2, 0, 124, 254, 63),
    'chain_257': (1,) + (0,) * 9,
    'ladder_65_rings': (2,) + (0,) * 9,
}


def _assembled(g):
    """one to three ring systems (a ring of 3 .. 7, sometimes with a fused or a spiro ring) joined by linkers of 0 .. 2 atoms, with up
    to four side chains, some starting with a double bond: at most 40 atoms"""
    bonds, n, anchors = [], 0, []
    for _ in range(int(g.integers(1, 4))):
        size, base, t = int(g.integers(3, 8)), n, int(g.choice([1, 4]))
        bonds += ring(size, base, t)
        n += size
        kind = g.random()
        if kind < 0.6:                                                 # a path from `base` to its neighbour (fused) or to itself (spiro)
            extra = int(g.integers(1, 4)) if kind < 0.35 else int(g.integers(2, 4))
            path = [base] + list(range(n, n + extra)) + [base + 1 if kind < 0.35 else base]
            bonds += [(path[k], path[k + 1], 1) for k in range(len(path) - 1)]
            n += extra
        anchors.append(base + int(g.integers(0, size)))
    for a, b in zip(anchors, anchors[1:]):
        path = [a] + list(range(n, n + int(g.integers(0, 3)))) + [b]
        bonds += [(path[k], path[k + 1], int(g.choice([1, 2], p=[0.8, 0.2]))) for k in range(len(path) - 1)]
        n = max(n, max(path) + 1)
    for _ in range(int(g.integers(0, 5))):
        at, length = int(g.integers(0, n)), int(g.integers(1, 3))
        if n + length > 40:
            break
        path = [at] + list(range(n, n + length))
        bonds += [(path[k], path[k + 1], int(g.choice([1, 2])) if k == 0 else 1) for k in range(length)]
        n += length
    return mol(g.choice([6, 7, 8], n, p=[0.7, 0.15, 0.15]).tolist(), bonds)


def sparse_graph(seed):
    """a seeded random sparse graph of 3 .. 40 atoms as a molecule dict with positions.  Even seeds: about as many bonds as atoms
    between random pairs (trees, rings, fused rings and several fragments all occur), elements C / N / O, types 1 / 2 / 4.  Odd seeds:
    ring systems joined by linkers with side chains (``_assembled``), atoms and bonds renumbered at random."""
    g = np.random.default_rng(seed)
    if seed % 2:
        m = permuted(_assembled(g), seed)[0]
        m['atom_pos'] = g.normal(size=(len(m['element']), 3)).astype(np.float32)
        return m
    n = int(g.integers(3, 41))
    want = int(g.integers(n // 2, n + n // 4 + 2))
    pairs = set()
    for _ in range(want):
        i, j = (int(x) for x in g.integers(0, n, 2))
        if i != j and (min(i, j), max(i, j)) not in pairs and (g.random() < 0.3 or abs(i - j) < 6):
            pairs.add((min(i, j), max(i, j)))
    bonds = [((i, j) if g.random() < 0.5 else (j, i)) + (int(g.choice([1, 2, 4], p=[0.6, 0.25, 0.15])),) for i, j in sorted(pairs)]
    order = g.permutation(len(bonds))
    m = mol(g.choice([6, 7, 8], n, p=[0.7, 0.15, 0.15]).tolist(), [bonds[k] for k in order])
    m['atom_pos'] = g.normal(size=(n, 3)).astype(np.float32)
    return m
