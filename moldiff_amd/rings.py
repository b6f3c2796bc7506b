"""Ring perception and composition counts of decoded molecules: ring sizes, ring atoms and bonds, rotatable bonds, element and bond
type histograms.

The device half is ``mdx_mol_rings`` (csrc/mdx_rings.hip), reached through ``rings_mols`` (a list of molecule dicts) and
``FeaturizeMol.rings_batch`` (the sampler's predictions).  ``rings_ref`` is the plain Python restatement for one molecule and needs no
GPU; the GPU tests compare every output exactly.

What it is: the reference's evaluation reports, from RDKit, the element / bond type / ring-size counts of ``frags_counts``
(utils/evaluation.py:52-83), ``n_atoms`` / ``n_bonds`` / ``n_rings`` / ``n_rotatable`` of ``count_prop`` (:24-37) and the ring atoms of
``ring_topo``.  RDKit is not available here, so every number is DEFINED by this project (include/moldiff_hip.h states them) such that
its value is unique -- no tie-break, atom order or traversal order enters:

  * ``n_rings`` is the cyclomatic number b - n + c of the molecule AS DECODED (valid bonds, atoms, fragments);
  * ``ring_hist`` counts the ring sizes of a MINIMUM CYCLE BASIS: the number of basis rings of size <= L is the GF(2) rank of all
    cycles of length <= L.  It is NOT RDKit's symmetrised SSSR (``GetSymmSSSR``): cubane has 5 four-rings here and 6 there;
  * a ring bond is a bond that is not a bridge, a ring atom an atom with a ring bond; ``bond_ring_min`` / ``atom_ring_min`` give the
    size of the smallest ring through a bond / an atom;
  * ``n_rotatable`` is this project's rule, not RDKit's SMARTS: a bond of type 1 that is no ring bond, both of whose atoms have at
    least two bonds and neither of whose atoms carries a bond of type 3.  There is NO amide exclusion.

The number of basis rings an atom lies in and ring SMILES are deliberately not offered: both depend on which basis is chosen.
With no trained checkpoint offline this is an instrument, not a measurement of quality.

    python -m moldiff_amd.rings stats samples_all.pt --out rings.npz [--ref] [--part finished]
    python -m moldiff_amd.rings compare a.npz b.npz
"""
import sys

import numpy as np

from . import molpack
from .molpack import DEFAULT_ATOMIC_NUMBERS, jsd_counts, mol_graph, to_host

MAX_ATOMS, MAX_BONDS, MAX_RINGS = 256, 512, 64      # include/moldiff_hip.h: beyond them a molecule gets a status, not a result
STATUS_OK, STATUS_TOO_LARGE, STATUS_TOO_MANY_RINGS = 0, 1, 2
MOL_KEYS = ('status', 'n_atoms', 'n_rings', 'ring_hist', 'n_ring_atoms', 'n_ring_bonds', 'n_rotatable', 'elem_count', 'bond_count')
SLOT_KEYS = ('bond_ring_min', 'atom_ring_min')
# the results table (molpack.Layout): bond_ptr but no n_bonds
LAYOUT = molpack.Layout(MOL_KEYS, atom=('atom_ring_min',), bond=('bond_ring_min',), wide=('ring_hist', 'elem_count', 'bond_count'))


def _widths(ring_bins, n_elements, num_bond_types):
    return {'ring_hist': ring_bins, 'elem_count': n_elements, 'bond_count': num_bond_types}


def _check_sizes(num_bond_types, n_elements, ring_bins):
    if not 1 <= int(ring_bins) <= 64:
        raise ValueError(f'ring_bins must lie in 1 .. 64, got {ring_bins}')
    if not 1 <= int(num_bond_types) <= 254 or not 1 <= n_elements <= 255:
        raise ValueError('at most 255 elements and 254 bond types')


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def _bfs(adj, root, skip=-1):
    """breadth-first search over adj[a] = [(neighbour, bond id)], without bond `skip` -> (depth per atom or -1, parent bond or -1);
    among an atom's neighbours of the previous level the one of smallest index becomes its parent, as on the device"""
    depth, pbond = [-1] * len(adj), [-1] * len(adj)
    depth[root], frontier = 0, [root]
    while frontier:
        reached = {}
        for p in frontier:
            for a, e in adj[p]:
                if e != skip and depth[a] < 0 and (a not in reached or (p, e) < reached[a]):
                    reached[a] = (p, e)
        for a, (p, e) in reached.items():
            depth[a], pbond[a] = depth[p] + 1, e
        frontier = sorted(reached)
    return depth, pbond


def rings_ref(info, num_bond_types=4, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, ring_bins=7):
    """Plain Python restatement of ``mdx_mol_rings`` for one molecule dict (element = atomic numbers, bond_index (2, 2b) with every bond
    once and then flipped, bond_type (2b)) -> dict: ``status`` (0 measured, 1 more than 256 atoms or 512 bonds, 2 more than 64
    rings), ``n_atoms``, ``n_rings``, ``ring_hist`` (ring_bins: sizes 3, 4, ... and the last bin every larger ring), ``n_ring_atoms``,
    ``n_ring_bonds``, ``n_rotatable``, ``elem_count``, ``bond_count`` (int32 arrays) and, per bond (the first b columns) and per atom,
    ``bond_ring_min`` / ``atom_ring_min``.  With a non-zero status everything but status and n_atoms is 0.  A bond whose index lies
    outside the molecule or with i = j is ignored; an element outside `atomic_numbers` and two bonds between the same pair of atoms
    raise ValueError."""
    atomic_numbers = tuple(int(z) for z in atomic_numbers)
    _check_sizes(num_bond_types, len(atomic_numbers), ring_bins)
    cls, bi, bt = mol_graph(info, atomic_numbers)
    n, nb = len(cls), bi.shape[1]
    bonds = [(e, int(bi[0, e]), int(bi[1, e])) for e in range(nb) if 0 <= bi[0, e] < n and 0 <= bi[1, e] < n and bi[0, e] != bi[1, e]]
    pairs = [(min(x, y), max(x, y)) for _, x, y in bonds]
    if len(set(pairs)) != len(pairs):
        raise ValueError('two bonds between the same pair of atoms')
    out = {'status': STATUS_OK, 'n_atoms': n, 'n_rings': 0, 'ring_hist': np.zeros(ring_bins, dtype=np.int32), 'n_ring_atoms': 0,
           'n_ring_bonds': 0, 'n_rotatable': 0, 'elem_count': np.zeros(len(atomic_numbers), dtype=np.int32),
           'bond_count': np.zeros(num_bond_types, dtype=np.int32), 'bond_ring_min': np.zeros(nb, dtype=np.int32),
           'atom_ring_min': np.zeros(n, dtype=np.int32)}
    if n > MAX_ATOMS or nb > MAX_BONDS:
        return dict(out, status=STATUS_TOO_LARGE)
    adj = [[] for _ in range(n)]
    for e, x, y in bonds:
        adj[x].append((y, e))
        adj[y].append((x, e))
    # the spanning forest: a breadth-first tree from the smallest atom of every fragment
    forest, seen, n_frag = set(), [False] * n, 0
    for r in range(n):
        if not seen[r]:
            n_frag += 1
            depth, pbond = _bfs(adj, r)
            for a in range(n):
                if depth[a] >= 0:
                    seen[a] = True
                    if pbond[a] >= 0:
                        forest.add(pbond[a])
    mu = len(bonds) - n + n_frag
    if mu > MAX_RINGS:
        return dict(out, status=STATUS_TOO_MANY_RINGS)
    # the smallest ring through a bond: 1 + the distance between its ends without it
    brm = out['bond_ring_min']
    for e, x, y in bonds:
        d = _bfs(adj, x, skip=e)[0][y]
        brm[e] = d + 1 if d >= 0 else 0
    for a in range(n):
        sizes = [int(brm[e]) for _, e in adj[a] if brm[e] > 0]
        out['atom_ring_min'][a] = min(sizes) if sizes else 0
    # a cycle is a set of the mu bonds outside the forest, held as the bits of a Python int
    bit = {e: 1 << k for k, e in enumerate(e for e, _, _ in bonds if e not in forest)}
    cand = []
    for v in range(n if mu else 0):
        depth, pbond = _bfs(adj, v)
        word = [0] * n
        for a in sorted(range(n), key=lambda a: depth[a]):
            if depth[a] > 0:
                e = pbond[a]
                x, y = int(bi[0, e]), int(bi[1, e])
                word[a] = word[x if y == a else y] ^ bit.get(e, 0)
        for e, x, y in bonds:
            if depth[x] >= 0:
                vec = word[x] ^ word[y] ^ bit.get(e, 0)
                if vec:
                    cand.append((depth[x] + depth[y] + 1, vec))
    basis, rank = {}, 0
    for length, vec in sorted(cand):
        if rank == mu:
            break
        while vec:
            hb = vec.bit_length() - 1
            if hb not in basis:
                basis[hb] = vec
                rank += 1
                out['ring_hist'][min(length - 3, ring_bins - 1)] += 1
                break
            vec ^= basis[hb]
    assert rank == mu, 'the candidate cycles do not span the cycle space'
    deg = [len(a) for a in adj]
    triple = [any(bt[e] == 3 for _, e in a) for a in adj]
    for e, x, y in bonds:
        if 1 <= bt[e] <= num_bond_types:
            out['bond_count'][bt[e] - 1] += 1
        if bt[e] == 1 and brm[e] == 0 and deg[x] >= 2 and deg[y] >= 2 and not triple[x] and not triple[y]:
            out['n_rotatable'] += 1
    np.add.at(out['elem_count'], cls, 1)
    out.update(n_rings=mu, n_ring_bonds=int((brm > 0).sum()), n_ring_atoms=int((out['atom_ring_min'] > 0).sum()))
    return out


def stack_ref(mols, num_bond_types=4, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, ring_bins=7):
    """``rings_ref`` of every molecule of a list as the results dict ``rings_mols`` returns (numpy): one entry per molecule of every
    key of MOL_KEYS, ``bond_ring_min`` / ``atom_ring_min`` over the bonds / atoms of the list in turn, ``atom_ptr`` / ``bond_ptr``"""
    out = molpack.stack([rings_ref(m, num_bond_types, atomic_numbers, ring_bins) for m in mols], LAYOUT,
                        _widths(ring_bins, len(tuple(atomic_numbers)), num_bond_types))
    return {k: out[k] for k in MOL_KEYS + SLOT_KEYS + ('atom_ptr', 'bond_ptr')}   # the key order of the stored files


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, num_element, num_bond_types, ring_bins=7, select=None):
    """``mdx_mol_rings`` on the device arrays `cm` (a ``CompactMols``) -> dict of int32 device tensors: the keys of MOL_KEYS but n_atoms, one
    entry (or row) per molecule, and ``bond_ring_min`` (Eh_stride) / ``atom_ring_min`` (N_cap) in the layout of the inputs, zero
    where no molecule has a slot; no sync"""
    from . import _lib
    _check_sizes(num_bond_types, num_element, ring_bins)
    out, _ = molpack.zeros_for(cm, LAYOUT, _widths(ring_bins, num_element, num_bond_types))
    if cm.B == 0:
        return out
    ops, at = cm.operands()
    _lib.check(_lib.lib().mdx_mol_rings(
        *ops, _lib.ptr(select), num_element, num_bond_types, ring_bins, at(out['n_rings']), at(out['ring_hist']), at(out['n_ring_atoms']),
        at(out['n_ring_bonds']), at(out['n_rotatable']), at(out['elem_count']), at(out['bond_count']), at(out['status']),
        at(out['bond_ring_min']), at(out['atom_ring_min']), _lib.stream()))
    return out


def rings_mols(mols, device, num_bond_types=4, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, ring_bins=7):
    """Ring and composition counts of a list of molecule dicts (finished molecules, or entries of ``samples_all.pt``) on the device: the
    list is packed densely, copied and handed to ``mdx_mol_rings``.  -> the results dict of ``stack_ref`` with device tensors.  Two
    bonds between the same pair of atoms and unknown elements raise ValueError."""
    atomic_numbers = tuple(int(z) for z in atomic_numbers)
    _check_sizes(num_bond_types, len(atomic_numbers), ring_bins)
    p, cm = molpack.packed(mols, atomic_numbers, device)
    return molpack.dense(launch(cm, len(atomic_numbers), num_bond_types, ring_bins), cm, p, LAYOUT)


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict"""
    return molpack.concat(parts, LAYOUT)


def empty(num_bond_types=4, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, ring_bins=7):
    return stack_ref([], num_bond_types, atomic_numbers, ring_bins)


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def _dist(counts):
    counts = [int(c) for c in counts]
    total = sum(counts)
    return {'counts': counts, 'fractions': [c / total if total else float('nan') for c in counts]}


def summary(results):
    """The numbers of a results dict (host or device arrays) -> dict, all from exact integer sums over the MEASURED molecules (status
    0): ``n_measured``; ``n_skipped`` by status (too_large, too_many_rings); ``mean_rings`` per molecule; ``ring_size`` (bin k = rings
    of size 3 + k, the last bin every larger one), ``element`` and ``bond_type``, each as counts and fractions;
    ``ring_atom_fraction`` = ring atoms over atoms; ``mean_rotatable`` per molecule.  NaN where nothing was measured."""
    r = to_host(results)
    ok = r['status'] == STATUS_OK
    n = int(ok.sum())
    total = lambda k: int(r[k][ok].astype(np.int64).sum())
    atoms = total('n_atoms')
    nan = float('nan')
    return {'n_measured': n,
            'n_skipped': {'too_large': int((r['status'] == STATUS_TOO_LARGE).sum()),
                          'too_many_rings': int((r['status'] == STATUS_TOO_MANY_RINGS).sum())},
            'mean_rings': total('n_rings') / n if n else nan,
            'ring_size': _dist(r['ring_hist'][ok].astype(np.int64).sum(0)),
            'element': _dist(r['elem_count'][ok].astype(np.int64).sum(0)),
            'bond_type': _dist(r['bond_count'][ok].astype(np.int64).sum(0)),
            'ring_atom_fraction': total('n_ring_atoms') / atoms if atoms else nan,
            'mean_rotatable': total('n_rotatable') / n if n else nan}


def compare(a, b):
    """Jensen-Shannon divergence (``molpack.jsd_counts``: base 2, in [0, 1], NaN when a side is empty) of the ring-size, element and
    bond-type distributions of two results dicts or two summaries -> {'ring_size': .., 'element': .., 'bond_type': ..}"""
    a, b = (x if 'ring_size' in x else summary(x) for x in (a, b))
    out = {}
    for k in ('ring_size', 'element', 'bond_type'):
        if len(a[k]['counts']) != len(b[k]['counts']):
            raise ValueError(f'{k}: the two sides have different bins')
        out[k] = jsd_counts(a[k]['counts'], b[k]['counts'])
    return out


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    return molpack.stats_main(
        argv, 'rings', __doc__, ('ring and composition counts of the molecules stored in a samples_all.pt',
                                 'Jensen-Shannon divergence of the ring-size, element and bond-type distributions of two files'),
        [('--ring_bins', dict(type=int, default=7))],
        lambda mols, a, dev: stack_ref(mols, ring_bins=a.ring_bins) if dev is None else rings_mols(mols, dev, ring_bins=a.ring_bins),
        summary, compare)


if __name__ == '__main__':
    sys.exit(main())
