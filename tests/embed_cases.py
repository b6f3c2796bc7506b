"""Molecules for the conformer-generation tests (test_embed_host.py, test_gpu_embed.py): the named molecules of ``relax_cases``, four
rings for the ring-angle rule, a few random molecules of at most 12 heavy atoms, a molecule whose bounds are inconsistent by
construction, and the size ladder.  A case is (molecule dict, order, h_count, h_pos, atom_flag) as in ``relax_cases``.  References are
computed once and shared."""
import functools
import math

import numpy as np

from moldiff_amd import embed, relax
from . import hydrogens_cases as HC
from . import relax_cases as RC
from .hydrogens_cases import AROMATIC, C, SINGLE, mol

K = 3                       # conformers per molecule
SEED = 20241021
RANDOM_SEED, RANDOM_COUNT, RANDOM_HEAVY = 20241021, 6, 12
RINGS = {'cyclopropane': 3, 'cyclobutane': 4, 'cyclopentane': 5}
ACYCLIC = ('ethane', 'propane', 'formamide', 'nitrile', 'sulfonamide', 'methane_ideal')


def ring(n, bond=SINGLE, length=1.5):
    r = length / (2.0 * math.sin(math.pi / n))
    pos = [(r * math.cos(2.0 * math.pi * k / n), r * math.sin(2.0 * math.pi * k / n), 0.0) for k in range(n)]
    return mol([C] * n, pos, [(k, (k + 1) % n, bond) for k in range(n)])


@functools.lru_cache(maxsize=None)
def named():
    """{name: case}: the named molecules of relax_cases, then the saturated rings"""
    out = dict(RC.named())
    out.update({name: RC.case(ring(n)) for name, n in RINGS.items()})
    return out


def named_lists():
    cases = named()
    return list(cases), [cases[k] for k in cases]


@functools.lru_cache(maxsize=None)
def random_set():
    rng = np.random.default_rng(RANDOM_SEED)
    out = []
    while len(out) < RANDOM_COUNT:
        m = RC.random_mol(rng)
        if len(m['element']) <= RANDOM_HEAVY:
            out.append(RC.case(m))
    return out


def all_cases():
    return named_lists()[1] + random_set()


def absurd_tables():
    """the default table with a tetrahedral carbon radius of 0.05 Angstrom: a chain's far ends must then be closer than they may be"""
    import yaml
    with open(relax.DEFAULT_TABLE) as f:
        table = yaml.safe_load(f)
    table['elements'][6]['variants']['tetrahedral']['r'] = 0.05
    return relax.ForceFieldTables(table=table)


def inconsistent():
    return RC.bare(HC.chain(6))


@functools.lru_cache(maxsize=None)
def bounds():
    """``bounds_ref`` of every case of ``all_cases``"""
    return [embed.bounds_ref(c[0], c[1], c[2], c[4]) for c in all_cases()]


@functools.lru_cache(maxsize=None)
def refs(max_iters):
    """``embed_ref`` of every case and conformer with its trace, once per max_iters -> [[(result, trace)] * K]"""
    out = []
    for m, b in enumerate(bounds()):
        row = []
        for c in range(K):
            trace = []
            row.append((embed.embed_ref(b, c, SEED, m, max_iters=max_iters, trace=trace), trace))
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def ladder_bounds():
    return [embed.bounds_ref(c[0], c[1], c[2], c[4]) for c in RC.ladder()]
