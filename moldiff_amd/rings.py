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
import argparse
import json
import sys

import numpy as np

from .local3d import jsd_counts
from .molpack import check_simple, CompactMols, DEFAULT_ATOMIC_NUMBERS, load_mols, load_npz, mol_graph, pack_mols, save_npz, to_device, to_host

MAX_ATOMS, MAX_BONDS, MAX_RINGS = 256, 512, 64      # include/moldiff_hip.h: beyond them a molecule gets a status, not a result
STATUS_OK, STATUS_TOO_LARGE, STATUS_TOO_MANY_RINGS = 0, 1, 2
MOL_KEYS = ('status', 'n_atoms', 'n_rings', 'ring_hist', 'n_ring_atoms', 'n_ring_bonds', 'n_rotatable', 'elem_count', 'bond_count')
SLOT_KEYS = ('bond_ring_min', 'atom_ring_min')


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
    refs = [rings_ref(m, num_bond_types, atomic_numbers, ring_bins) for m in mols]
    width = {'ring_hist': ring_bins, 'elem_count': len(tuple(atomic_numbers)), 'bond_count': num_bond_types}
    out = {k: np.asarray([r[k] for r in refs], dtype=np.int32).reshape((len(refs), width[k]) if k in width else (len(refs),))
           for k in MOL_KEYS}
    for k in SLOT_KEYS:
        out[k] = np.concatenate([r[k] for r in refs] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    na, nb = out['n_atoms'].astype(np.int64), np.asarray([len(r['bond_ring_min']) for r in refs], dtype=np.int64)
    out['atom_ptr'], out['bond_ptr'] = (np.cumsum(na) - na).astype(np.int32), (np.cumsum(nb) - nb).astype(np.int32)
    return out


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, num_element, num_bond_types, ring_bins=7, select=None):
    """``mdx_mol_rings`` on the device arrays `cm` (a ``CompactMols``) -> dict of int32 device tensors: the keys of MOL_KEYS but n_atoms, one
    entry (or row) per molecule, and ``bond_ring_min`` (Eh_stride) / ``atom_ring_min`` (N_cap) in the layout of the inputs, zero
    where no molecule has a slot; no sync"""
    import torch
    from . import _lib
    _check_sizes(num_bond_types, num_element, ring_bins)
    B, dev = cm.B, cm.device
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    out = {'status': z(B), 'n_rings': z(B), 'ring_hist': z(B, ring_bins), 'n_ring_atoms': z(B), 'n_ring_bonds': z(B), 'n_rotatable': z(B),
           'elem_count': z(B, num_element), 'bond_count': z(B, num_bond_types), 'bond_ring_min': z(max(cm.Eh_stride, 1)),
           'atom_ring_min': z(max(cm.N_cap, 1))}
    if B == 0:
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
    import torch
    device = torch.device(device)
    atomic_numbers = tuple(int(z) for z in atomic_numbers)
    _check_sizes(num_bond_types, len(atomic_numbers), ring_bins)
    p = pack_mols(mols, atomic_numbers)
    check_simple(p)
    cm = CompactMols.from_packed(to_device(p, device))
    out = launch(cm, len(atomic_numbers), num_bond_types, ring_bins)
    out['bond_ring_min'], out['atom_ring_min'] = out['bond_ring_min'][:len(cm.bond_type)], out['atom_ring_min'][:cm.N_cap]
    out.update(n_atoms=cm.n_atoms, atom_ptr=cm.atom_ptr, bond_ptr=cm.bond_ptr)
    return out


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict"""
    parts = [to_host(p) for p in parts]
    out = {k: np.concatenate([p[k] for p in parts]) for k in MOL_KEYS + SLOT_KEYS}
    na = out['n_atoms'].astype(np.int64)
    nb = np.concatenate([np.diff(np.append(p['bond_ptr'].astype(np.int64), len(p['bond_ring_min']))) for p in parts])
    out['atom_ptr'], out['bond_ptr'] = (np.cumsum(na) - na).astype(np.int32), (np.cumsum(nb) - nb).astype(np.int32)
    return out


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
    """Jensen-Shannon divergence (``local3d.jsd_counts``: base 2, in [0, 1], NaN when a side is empty) of the ring-size, element and
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
    ap = argparse.ArgumentParser(prog='python -m moldiff_amd.rings', description=__doc__.split('\n\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    s = sub.add_parser('stats', help='ring and composition counts of the molecules stored in a samples_all.pt')
    s.add_argument('samples')
    s.add_argument('--out', required=True)
    s.add_argument('--part', default='finished')
    s.add_argument('--ring_bins', type=int, default=7)
    s.add_argument('--device', default='cuda:0')
    s.add_argument('--ref', action='store_true', help='the Python path instead of the device')
    c = sub.add_parser('compare', help='Jensen-Shannon divergence of the ring-size, element and bond-type distributions of two files')
    c.add_argument('a')
    c.add_argument('b')
    args = ap.parse_args(argv)
    if args.cmd == 'stats':
        mols = load_mols(args.samples, args.part)
        if args.ref:
            res = stack_ref(mols, ring_bins=args.ring_bins)
        else:
            import torch
            torch.cuda.set_device(torch.device(args.device))
            res = rings_mols(mols, args.device, ring_bins=args.ring_bins)
        save_npz(res, args.out)
        print(json.dumps(summary(res), indent=1))
    else:
        print(json.dumps(compare(load_npz(args.a), load_npz(args.b)), indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
