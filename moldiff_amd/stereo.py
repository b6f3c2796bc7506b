"""Stereo perception of decoded molecules from their 3D coordinates: tetrahedral parities, cis / trans codes of double bonds, and the
isomeric key (full certificate of ``canon``, canonical stereo word) that tells enantiomers, cis / trans rings and E / Z alkenes apart.

The device half is ``mdx_mol_stereo`` (csrc/mdx_stereo.hip), reached through ``stereo_mols`` (a list of molecule dicts; runs ``canon``
first), ``launch`` (a ``CompactMols`` and the results of ``canon.launch``) and ``FeaturizeMol.stereo_batch`` (the sampler's predictions).
``stereo_ref`` is the plain restatement for one molecule and needs no GPU; the GPU tests compare every output exactly.

What it is: the reference's uniqueness and novelty come from ``Chem.MolToSmiles`` of molecules read back from 3D mol blocks
(utils/scoring_func.py:170, utils/evaluation.py:360), where RDKit perceives stereo from the coordinates.  RDKit is not available here, so
this is THIS PROJECT'S OWN DEFINITION, stated exactly in include/moldiff_hip.h: NOT RDKit's stereo perception, NOT the CIP rules, and
UNVERIFIED AGAINST RDKit.  It is blind to allenes and cumulenes, atropisomers and nitrogen inversion, and every label depends on
``flat_tol`` and ``bond_tol`` (0.1 each: untuned choices).  With no trained checkpoint offline it is an instrument, not a measurement
of sample quality.

The definition in short.  Geometry, once, in float64: a tetrahedral candidate (4 bonds and a class of ``centre4``; or 3 single bonds
and a class of ``centre3``: one implicit H) gets g = the sign of a determinant of the unit vectors to its neighbours in ascending atom
index, 0 within the threshold; a double-bond candidate (type 2, 1 or 2 other bonds on each end, none of type 2 or 3) gets per pairing
of other neighbours d = 1 cis / 2 trans / 0.  An optimal leaf of canon's search tree (its certificate is the canonical one) has a word:
per rank p the atom's code (0; else 1 or 2 from g times the sign of the permutation that sorts its neighbours by leaf rank), then per
canonical bond word the bond's code d(x, y), x and y the other neighbours of smallest leaf rank.  W is the smallest word over all
optimal leaves, M the smallest mirror word (codes 1 and 2 of the atoms swapped); a reflection swaps W and M, and the molecule is chiral
iff W != M.  ``stereo_rank`` is the smallest rank vector among the leaves attaining W.

    python -m moldiff_amd.stereo stats samples_all.pt --out stereo.npz [--ref] [--flat_tol 0.1] [--bond_tol 0.1] [--part finished]
    python -m moldiff_amd.stereo compare a.npz b.npz
"""
import math
import sys

import numpy as np

from . import canon, molpack
from .molpack import DEFAULT_ATOMIC_NUMBERS, jsd_counts, mol_graph, to_host

MAX_ATOMS, MAX_BONDS = canon.MAX_ATOMS, canon.MAX_BONDS
DEFAULT_MAX_NODES = canon.DEFAULT_MAX_NODES
DEFAULT_FLAT_TOL, DEFAULT_BOND_TOL = 0.1, 0.1                     # this project's untuned choices
DEFAULT_CENTRE4, DEFAULT_CENTRE3 = (6, 7, 15, 16), (6,)           # atomic numbers that may be a centre with 4 / with 3 neighbours
STATUS_OK, STATUS_NO_CANON, STATUS_ABANDONED = 0, 1, 2
# the columns of the device's per-molecule table, in its order (include/moldiff_hip.h: MDX_STEREO_STATS)
STAT_KEYS = ('status', 'n_centre_candidates', 'n_centres', 'n_flat', 'n_bond_candidates', 'n_stereo_bonds', 'n_stereogenic', 'chiral', 'n_aut')
MOL_KEYS = STAT_KEYS + ('stereo_hash', 'mirror_hash', 'n_atoms', 'n_bonds')
ATOM_KEYS = ('canon_tetra', 'mirror_tetra', 'stereo_rank', 'atom_tetra')
BOND_KEYS = ('canon_bond_stereo', 'mirror_bond_stereo', 'bond_stereo')
LAYOUT = molpack.Layout(MOL_KEYS, atom=ATOM_KEYS, bond=BOND_KEYS, int64=('stereo_hash', 'mirror_hash'))          # the results table
CENTRE_BINS = 9                                                   # bin k: molecules with k centres, the last bin every larger count


def _check(flat_tol, bond_tol, max_nodes):
    for name, t in (('flat_tol', flat_tol), ('bond_tol', bond_tol)):
        if not 0.0 <= float(t) < 1.0:                             # NaN fails
            raise ValueError(f'{name} must lie in [0, 1), got {t}')
    return float(flat_tol), float(bond_tol), canon._check_nodes(max_nodes)


def class_mask(elements, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """the bit mask over the class indices of `atomic_numbers` for the atomic numbers `elements` (those not among them are skipped)"""
    z = [int(x) for x in atomic_numbers]
    mask = 0
    for e in elements:
        if int(e) in z and z.index(int(e)) < 32:
            mask |= 1 << z.index(int(e))
    return mask


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _det3(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0])


def _unit(d):
    dd = _dot(d, d)
    if not dd > 0.0:
        return None
    l = math.sqrt(dd)
    return (d[0] / l, d[1] / l, d[2] / l)


def _finite(*ps):
    return all(math.isfinite(x) for p in ps for x in p)


def _valid_bonds(bi, bt, n):
    nb = bi.shape[1]
    ok = (bi[0] >= 0) & (bi[0] < n) & (bi[1] >= 0) & (bi[1] < n) & (bi[0] != bi[1]) if nb else np.zeros(0, dtype=bool)
    return ok, (bt & 0xff)


def geometry_ref(info, flat_tol=DEFAULT_FLAT_TOL, bond_tol=DEFAULT_BOND_TOL, centre4_mask=None, centre3_mask=None,
                 atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """The geometry step of the definition for one molecule dict with ``atom_pos``, in Python floats (float64) with the operation order
    of the header -> dict: ``g`` {atom: +1 | -1 | 0} over the tetrahedral candidates, ``nbrs`` {atom: its neighbours ascending},
    ``d`` {bond slot: (xs, ys, {(x, y): 0 | 1 | 2})} over the double-bond candidates (xs / ys: the other neighbours of the bond's first
    / second atom, ascending), and what the tests' threshold band looks at: ``volumes`` [(v, threshold)] of the candidates with a
    volume and ``cosines`` [c] of the pairings with one."""
    cls, bi, bt = mol_graph(info, atomic_numbers)
    n = len(cls)
    c4 = class_mask(DEFAULT_CENTRE4, atomic_numbers) if centre4_mask is None else int(centre4_mask)
    c3 = class_mask(DEFAULT_CENTRE3, atomic_numbers) if centre3_mask is None else int(centre3_mask)
    pos = [tuple(float(x) for x in row) for row in np.asarray(info['atom_pos'], dtype=np.float32).reshape(n, 3)]
    ok, typ = _valid_bonds(bi, bt, n)
    adj = [[] for _ in range(n)]
    for e in np.flatnonzero(ok):
        i, j, t = int(bi[0, e]), int(bi[1, e]), int(typ[e])
        adj[i].append((j, t)), adj[j].append((i, t))
    out = {'g': {}, 'nbrs': {}, 'd': {}, 'volumes': [], 'cosines': []}
    for a in range(n):
        deg, c = len(adj[a]), int(cls[a])
        bit = lambda mask: c < 32 and (mask >> c) & 1
        if not ((deg == 4 and bit(c4)) or (deg == 3 and bit(c3) and all(t == 1 for _, t in adj[a]))):
            continue
        nbrs = sorted(u for u, _ in adj[a])
        out['nbrs'][a], out['g'][a] = nbrs, 0
        if not _finite(pos[a], *(pos[u] for u in nbrs)):
            continue
        us = [_unit(_sub(pos[u], pos[a])) for u in nbrs]
        if any(u is None for u in us):
            continue
        if deg == 4:
            v, thr = _det3(_sub(us[1], us[0]), _sub(us[2], us[0]), _sub(us[3], us[0])), 4.0 * flat_tol
        else:
            v, thr = _det3(us[0], us[1], us[2]), flat_tol
        out['volumes'].append((v, thr))
        out['g'][a] = 1 if v > thr else -1 if v < -thr else 0
    for e in np.flatnonzero(ok):
        a, b = int(bi[0, e]), int(bi[1, e])
        if int(typ[e]) != 2 or not (2 <= len(adj[a]) <= 3 and 2 <= len(adj[b]) <= 3):
            continue
        xs, ys = sorted(u for u, _ in adj[a] if u != b), sorted(u for u, _ in adj[b] if u != a)
        if any(t in (2, 3) for u, t in adj[a] if u != b) or any(t in (2, 3) for u, t in adj[b] if u != a) or not xs or not ys:
            continue
        table = {}
        for x in xs:
            for y in ys:
                table[x, y] = 0
                if not _finite(pos[a], pos[b], pos[x], pos[y]):
                    continue
                ev = _unit(_sub(pos[b], pos[a]))
                if ev is None:
                    continue
                dx, dy = _sub(pos[x], pos[a]), _sub(pos[y], pos[b])
                tx, ty = _dot(dx, ev), _dot(dy, ev)
                xp = (dx[0] - tx * ev[0], dx[1] - tx * ev[1], dx[2] - tx * ev[2])
                yp = (dy[0] - ty * ev[0], dy[1] - ty * ev[1], dy[2] - ty * ev[2])
                xx, yy = _dot(xp, xp), _dot(yp, yp)
                if not xx > 0.0 or not yy > 0.0:
                    continue
                c = _dot(xp, yp) / (math.sqrt(xx) * math.sqrt(yy))
                out['cosines'].append(c)
                table[x, y] = 1 if c > bond_tol else 2 if c < -bond_tol else 0
        out['d'][int(e)] = (xs, ys, table)
    return out


def near_threshold(info, flat_tol=DEFAULT_FLAT_TOL, bond_tol=DEFAULT_BOND_TOL, band=1e-6, **kw):
    """whether some volume of ``geometry_ref`` lies within `band` of its threshold or some cosine within `band` of +-bond_tol: the
    molecules a device comparison may leave out, because float64 contraction may differ"""
    geo = geometry_ref(info, flat_tol, bond_tol, **kw)
    return any(abs(abs(v) - thr) <= band for v, thr in geo['volumes']) or any(abs(abs(c) - bond_tol) <= band for c in geo['cosines'])


def _mirror(word, n):
    return [3 - c if p < n and c else c for p, c in enumerate(word)]


def stereo_ref(info, canon_result, atom_label=None, flat_tol=DEFAULT_FLAT_TOL, bond_tol=DEFAULT_BOND_TOL, centre4_mask=None,
               centre3_mask=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """Plain restatement of ``mdx_mol_stereo`` for one molecule dict with ``atom_pos`` and its canon result (``canon.canon_ref``'s dict
    or a ``canon.mol_result`` slice, made with the same `atom_label`) -> dict: the keys of STAT_KEYS, ``stereo_hash``, ``mirror_hash``,
    ``n_atoms``, ``n_bonds``; per atom ``canon_tetra`` / ``mirror_tetra`` (the atom codes of W / M by rank), ``stereo_rank`` and
    ``atom_tetra`` (W in input order); per bond slot ``canon_bond_stereo`` / ``mirror_bond_stereo`` (the bond codes of W / M in
    certificate order, zeros behind them) and ``bond_stereo`` (W's code of the bond in the slot).  With a non-zero status stereo_rank is
    -1 and every other output 0.  Two bonds between one pair of atoms are outside the definition (``molpack.check_simple``)."""
    flat_tol, bond_tol, max_nodes = _check(flat_tol, bond_tol, max_nodes)
    cls, bi, bt = mol_graph(info, atomic_numbers)
    n, nb = len(cls), bi.shape[1]
    label = cls.astype(np.int64) if atom_label is None else canon._check_label(atom_label, n)
    zi = lambda *k: np.zeros(k, dtype=np.int32)
    out = dict({k: 0 for k in STAT_KEYS}, stereo_hash=0, mirror_hash=0, n_atoms=n, n_bonds=nb)
    out.update({k: zi(n) for k in ATOM_KEYS}, stereo_rank=np.full(n, -1, dtype=np.int32))
    out.update({k: zi(nb) for k in BOND_KEYS})
    given = np.asarray(canon_result['rank'], dtype=np.int64).reshape(-1)
    if int(canon_result['status']) != 0 or n > MAX_ATOMS or nb > MAX_BONDS or len(given) != n or ((given < 0) | (given >= n)).any():
        return dict(out, status=STATUS_NO_CANON)
    ok, typ = _valid_bonds(bi, bt, n)
    slots = np.flatnonzero(ok)
    bx, by, btype = bi[0][ok], bi[1][ok], typ[ok].astype(np.int64)
    geo = geometry_ref(info, flat_tol, bond_tol, centre4_mask, centre3_mask, atomic_numbers)

    def words(c):
        lo, hi = np.minimum(c[bx], c[by]), np.maximum(c[bx], c[by])
        return (lo * (1 << 20) + hi * (1 << 8) + btype).tolist()
    canonical = sorted(words(given))
    place = {w: k for k, w in enumerate(canonical)}
    nbv = len(canonical)
    best = {'W': None, 'M': None, 'rank': None, 'table': None, 'n_aut': 0}

    def word_of(c):
        """the stereo word of the optimal leaf with ranks c, and the place of every valid bond in it"""
        w = [0] * (n + nbv)
        for a, g in geo['g'].items():
            if g:
                r = [int(c[u]) for u in geo['nbrs'][a]]
                inversions = sum(r[i] > r[j] for i in range(len(r)) for j in range(i + 1, len(r)))
                w[int(c[a])] = 1 if g * (-1 if inversions & 1 else 1) > 0 else 2
        where = [place[x] for x in words(c)]
        for k, e in enumerate(slots):
            if int(e) in geo['d']:
                xs, ys, table = geo['d'][int(e)]
                w[n + where[k]] = table[min(xs, key=lambda u: c[u]), min(ys, key=lambda u: c[u])]
        return w, where

    def leaf(c):
        if sorted(words(c)) != canonical:
            return
        best['n_aut'] += 1
        w, _ = word_of(c)
        mw = _mirror(w, n)
        if best['W'] is None or w < best['W']:
            best['W'], best['rank'] = w, c.copy()
        elif w == best['W'] and c.tolist() < best['rank'].tolist():
            best['rank'] = c.copy()
        if best['M'] is None or mw < best['M']:
            best['M'] = mw
        best['table'] = np.argsort(c) if best['table'] is None else np.minimum(best['table'], np.argsort(c))

    try:
        canon.search(label, bx, by, btype.astype(np.uint64), max_nodes, leaf)
    except canon.Abandoned:
        return dict(out, status=STATUS_ABANDONED)
    if best['n_aut'] == 0:                                             # the rank is not canon's for this molecule
        return dict(out, status=STATUS_NO_CANON)
    W, M, rank = best['W'], best['M'], best['rank']
    orbit = best['table'][given]
    _, where = word_of(rank)
    out['canon_tetra'][:], out['mirror_tetra'][:], out['stereo_rank'][:] = W[:n], M[:n], rank
    out['atom_tetra'][:] = np.asarray(W[:n], dtype=np.int32)[rank] if n else 0
    out['canon_bond_stereo'][:nbv], out['mirror_bond_stereo'][:nbv] = W[n:], M[n:]
    for k, e in enumerate(slots):
        out['bond_stereo'][e] = W[n + where[k]]
    centres = [a for a, g in geo['g'].items() if g]
    out.update(n_centre_candidates=len(geo['g']), n_centres=len(centres), n_flat=len(geo['g']) - len(centres), n_bond_candidates=len(geo['d']),
               n_stereo_bonds=int(sum(c != 0 for c in W[n:])), chiral=int(W != M), n_aut=best['n_aut'],
               n_stereogenic=sum(len({int(orbit[u]) for u in geo['nbrs'][a]}) == len(geo['nbrs'][a]) for a in centres),
               stereo_hash=canon.fnv1a64(W), mirror_hash=canon.fnv1a64(M))
    return out


def _labels(atom_label, k):
    return None if atom_label is None else atom_label[k]


def stack_ref(mols, canon_results=None, atom_label=None, flat_tol=DEFAULT_FLAT_TOL, bond_tol=DEFAULT_BOND_TOL, centre4_mask=None,
              centre3_mask=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """``stereo_ref`` of every molecule of a list as the results dict ``stereo_mols`` returns (numpy): one entry per molecule of every
    key of MOL_KEYS (int32, the hashes int64), the per-atom keys over the atoms and the per-bond keys over the bond slots of the list
    in turn, ``atom_ptr`` and ``bond_ptr``.  canon_results: the results dict of ``canon.stack_ref`` / ``canon.canon_mols`` for the
    same list (host arrays), made here with `max_nodes` when None.  atom_label: one array per molecule, or None."""
    if canon_results is None:
        canon_results = canon.stack_ref(mols, atom_label, max_nodes, atomic_numbers)
    refs = [stereo_ref(m, canon.mol_result(canon_results, k), _labels(atom_label, k), flat_tol, bond_tol, centre4_mask, centre3_mask,
                       max_nodes, atomic_numbers) for k, m in enumerate(mols)]
    return molpack.stack(refs, LAYOUT)


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, canon_results, flat_tol=DEFAULT_FLAT_TOL, bond_tol=DEFAULT_BOND_TOL, centre4_mask=None, centre3_mask=None,
           max_nodes=DEFAULT_MAX_NODES, select=None, atom_label=None, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """``mdx_mol_stereo`` on the device arrays `cm` (a ``CompactMols`` with positions) and the results of ``canon.launch`` on the same
    arrays with the same `atom_label` (its ``rank`` and ``status`` are read) -> dict of device tensors: the keys of STAT_KEYS (B) each
    (int32, columns of one (B, 9) table), ``stereo_hash`` / ``mirror_hash`` (B, int64), the keys of ATOM_KEYS (N_cap) and BOND_KEYS
    (Eh_stride) in the layout of the inputs, zero where no molecule has a slot.  The masks default to C, N, P, S and C among
    `atomic_numbers`.  No sync."""
    import torch
    from . import _lib
    flat_tol, bond_tol, max_nodes = _check(flat_tol, bond_tol, max_nodes)
    c4 = class_mask(DEFAULT_CENTRE4, atomic_numbers) if centre4_mask is None else int(centre4_mask)
    c3 = class_mask(DEFAULT_CENTRE3, atomic_numbers) if centre3_mask is None else int(centre3_mask)
    if not (0 <= c4 < 1 << 32 and 0 <= c3 < 1 << 32):
        raise ValueError('a centre mask is a 32-bit field over the atom classes')
    if atom_label is not None:
        if atom_label.dtype != torch.int32 or atom_label.numel() < cm.N_cap:
            raise ValueError('atom_label is an int32 tensor in the layout of atom_type')
        atom_label = atom_label.contiguous()
    out, stats = molpack.zeros_for(cm, LAYOUT, stat_keys=STAT_KEYS)
    if cm.B > 0:
        if cm.atom_pos is None:
            raise ValueError('stereo perception needs positions: a CompactMols with atom_pos')
        rank, cstat = canon_results['rank'], canon_results['status']
        if rank.dtype != torch.int32 or cstat.dtype != torch.int32 or rank.numel() < cm.N_cap or cstat.numel() < cm.B:
            raise ValueError('canon_results holds rank and status of canon.launch on the same arrays')
        rank, cstat = rank.contiguous(), cstat.contiguous()
        ops, at = cm.operands()
        g = lambda k: at(out[k])
        _lib.check(_lib.lib().mdx_mol_stereo(
            *ops, _lib.ptr(select), at(cm.atom_pos), None if atom_label is None else at(atom_label), at(rank), at(cstat), c4, c3, flat_tol,
            bond_tol, max_nodes, g('canon_tetra'), g('canon_bond_stereo'), g('mirror_tetra'), g('mirror_bond_stereo'), g('stereo_rank'),
            g('atom_tetra'), g('bond_stereo'), at(stats), g('stereo_hash'), g('mirror_hash'), _lib.stream()))
    return molpack.split_stats(out, stats, STAT_KEYS)


def stereo_mols(mols, device, atom_label=None, flat_tol=DEFAULT_FLAT_TOL, bond_tol=DEFAULT_BOND_TOL, centre4_mask=None, centre3_mask=None,
                max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, with_canon=False):
    """Stereo perception of a list of molecule dicts with ``atom_pos`` (finished molecules, or entries of ``samples_all.pt``) on the
    device: the list is packed densely, copied and handed to ``mdx_mol_canon`` and then ``mdx_mol_stereo``.  -> the results dict of
    ``stack_ref`` with device tensors; with `with_canon` -> (the results of ``canon.canon_mols``, that): what ``iso_certificate``,
    ``summary`` and ``canon.smiles_mols`` take.  Two bonds between the same pair of atoms, a molecule without positions and unknown
    elements raise ValueError."""
    import torch
    _check(flat_tol, bond_tol, max_nodes)
    if any('atom_pos' not in m for m in mols):
        raise ValueError('stereo perception needs atom_pos in every molecule')
    p, cm = molpack.packed(mols, atomic_numbers, device, positions=True)
    lab = None
    if atom_label is not None:
        if len(atom_label) != len(mols):
            raise ValueError('one label array per molecule')
        lab = np.concatenate([canon._check_label(a, int(n)) for a, n in zip(atom_label, p['n_atoms'])] + [np.zeros(0, dtype=np.int64)])
        lab = torch.from_numpy(lab.astype(np.int32)).to(cm.device)
    c = canon.launch(cm, max_nodes, atom_label=lab)
    s = launch(cm, c, flat_tol, bond_tol, centre4_mask, centre3_mask, max_nodes, atom_label=lab, atomic_numbers=atomic_numbers)
    s = molpack.dense(s, cm, p, LAYOUT)
    return (molpack.dense(c, cm, p, canon.LAYOUT), s) if with_canon else s


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict"""
    return molpack.concat(parts, LAYOUT)


def empty():
    return stack_ref([])


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def mol_result(results, m):
    """molecule `m` of a results dict with host arrays as the dict ``stereo_ref`` returns"""
    return molpack.mol_slice(results, m, LAYOUT)


def _word(r, k, mirror=False):
    pre = 'mirror_' if mirror else 'canon_'
    return np.concatenate([r[pre + 'tetra'], r[pre + 'bond_stereo'][:k]]).astype(np.int32).tobytes()


def iso_certificate(canon_results, stereo_results, m, mirror=False):
    """The isomeric key of molecule `m` as bytes: the full certificate of ``canon.certificate`` followed by the n + canon_n_bonds int32
    values of W (of M with `mirror`: the key of the mirror image).  Two measured molecules are the same labelled graph with the same
    perceived stereo iff these are equal.  None for a molecule either side did not measure.  Both dicts hold host arrays."""
    c = canon.certificate(canon_results, m)
    r = mol_result(stereo_results, m)
    if c is None or r['status'] != STATUS_OK:
        return None
    return c + _word(r, int(canon_results['canon_n_bonds'][m]), mirror)


def _keys(canon_results, stereo_results, mirror=False):
    c, s = to_host(canon_results), to_host(stereo_results)
    if len(c['status']) != len(s['status']):
        raise ValueError('the canon and the stereo results are of different lists')
    return [iso_certificate(c, s, m, mirror) for m in range(len(s['status']))]


def summary(stereo_results, canon_results):
    """The numbers of a stereo results dict and the canon results of the same list (host or device arrays) -> dict: ``n_molecules``,
    ``n_measured`` (status 0), ``n_no_canon``, ``n_abandoned``; over the measured molecules ``n_distinct`` and ``uniqueness`` (distinct
    full certificates: constitutional, as ``canon.summary``), ``n_iso_distinct`` and ``iso_uniqueness`` (distinct isomeric keys),
    ``n_chiral`` and ``share_chiral``, ``n_centre_candidates``, ``n_flat`` and ``share_flat_centres`` = n_flat / n_centre_candidates,
    ``mean_n_centres``, ``mean_n_stereogenic``, ``mean_n_stereo_bonds``, ``n_bond_candidates``, ``centres_hist`` (bin k: molecules with
    k centres, the last bin every larger count) and ``n_enantiomer_pairs``: the unordered pairs of distinct chiral keys that are each
    other's mirror image.  NaN where nothing was counted.  The stereo model is this project's own, unverified against RDKit."""
    s, c = to_host(stereo_results), to_host(canon_results)
    ok = s['status'] == STATUS_OK
    k, nan = int(ok.sum()), float('nan')
    keys = _keys(c, s)
    have = {key for key in keys if key is not None}
    mirrors = {key: mk for key, mk in zip(keys, _keys(c, s, mirror=True)) if key is not None}
    pairs = sum(mirrors[key] != key and mirrors[key] in have for key in have)
    certs = {canon.certificate(c, m) for m in np.flatnonzero(ok)}
    total = lambda key: int(s[key][ok].astype(np.int64).sum())
    cand, flat = total('n_centre_candidates'), total('n_flat')
    hist = np.bincount(np.minimum(s['n_centres'][ok].astype(np.int64), CENTRE_BINS - 1), minlength=CENTRE_BINS)
    return {'n_molecules': len(ok), 'n_measured': k, 'n_no_canon': int((s['status'] == STATUS_NO_CANON).sum()),
            'n_abandoned': int((s['status'] == STATUS_ABANDONED).sum()), 'n_distinct': len(certs), 'uniqueness': len(certs) / k if k else nan,
            'n_iso_distinct': len(have), 'iso_uniqueness': len(have) / k if k else nan, 'n_chiral': total('chiral'),
            'share_chiral': total('chiral') / k if k else nan, 'n_centre_candidates': cand, 'n_flat': flat,
            'share_flat_centres': flat / cand if cand else nan, 'mean_n_centres': total('n_centres') / k if k else nan,
            'mean_n_stereogenic': total('n_stereogenic') / k if k else nan, 'mean_n_stereo_bonds': total('n_stereo_bonds') / k if k else nan,
            'n_bond_candidates': total('n_bond_candidates'), 'centres_hist': hist.tolist(), 'n_enantiomer_pairs': pairs // 2}


def novelty(stereo_results, canon_results, ref_stereo, ref_canon):
    """the fraction of the measured molecules whose isomeric key occurs nowhere among the measured molecules of the reference pair (NaN
    when nothing was measured).  Both sides must have been labelled alike and measured with the same tolerances."""
    known = {key for key in _keys(ref_canon, ref_stereo) if key is not None}
    mine = [key for key in _keys(canon_results, stereo_results) if key is not None]
    return sum(key not in known for key in mine) / len(mine) if mine else float('nan')


def merged(canon_results, stereo_results):
    """both results dicts of one list as one dict (host arrays): what ``stats`` stores, ``split`` takes apart again"""
    c, s = to_host(canon_results), to_host(stereo_results)
    return dict({'canon/' + k: v for k, v in c.items()}, **s)


def split(results):
    """-> (canon results, stereo results) of a dict of ``merged``"""
    r = to_host(results)
    return {k[6:]: v for k, v in r.items() if k.startswith('canon/')}, {k: v for k, v in r.items() if not k.startswith('canon/')}


def _summary_of_merged(results):
    c, s = split(results)
    return summary(s, c)


def compare(a, b):
    """two dicts of ``merged`` -> dict: Jensen-Shannon divergence (``molpack.jsd_counts``) of ``centres_hist``, both sides'
    ``iso_uniqueness``, ``share_chiral`` and ``share_flat_centres``, and the novelty of each side against the other by isomeric key"""
    (ca, sa), (cb, sb) = split(a), split(b)
    ua, ub = summary(sa, ca), summary(sb, cb)
    return {'centres': jsd_counts(ua['centres_hist'], ub['centres_hist']), 'iso_uniqueness': [ua['iso_uniqueness'], ub['iso_uniqueness']],
            'share_chiral': [ua['share_chiral'], ub['share_chiral']], 'share_flat_centres': [ua['share_flat_centres'], ub['share_flat_centres']],
            'novelty': [novelty(sa, ca, sb, cb), novelty(sb, cb, sa, ca)]}


# ---- command line --------------------------------------------------------------------------------------------------------------------

def stats_mols(mols, device=None, flat_tol=DEFAULT_FLAT_TOL, bond_tol=DEFAULT_BOND_TOL, max_nodes=DEFAULT_MAX_NODES,
               atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """canon and stereo results of a list of molecule dicts in one host dict (``merged``): on `device`, or the Python path when None"""
    if device is None:
        c = canon.stack_ref(mols, max_nodes=max_nodes, atomic_numbers=atomic_numbers)
        return merged(c, stack_ref(mols, c, None, flat_tol, bond_tol, None, None, max_nodes, atomic_numbers))
    return merged(*stereo_mols(mols, device, None, flat_tol, bond_tol, None, None, max_nodes, atomic_numbers, with_canon=True))


def main(argv=None):
    return molpack.stats_main(
        argv, 'stereo', __doc__, ('stereo perception of the molecules stored in a samples_all.pt (canon and stereo results in one file)',
                                  'centre-count divergence, isomeric uniqueness and mutual novelty of two files'),
        [('--flat_tol', dict(type=float, default=DEFAULT_FLAT_TOL)), ('--bond_tol', dict(type=float, default=DEFAULT_BOND_TOL)),
         ('--max_nodes', dict(type=int, default=DEFAULT_MAX_NODES))],
        lambda mols, a, dev: stats_mols(mols, dev, a.flat_tol, a.bond_tol, a.max_nodes), _summary_of_merged, compare)


if __name__ == '__main__':
    sys.exit(main())
