"""Canonical labelling of decoded molecules: an exact molecule key (the full certificate), the order of the automorphism group, the
symmetry class (orbit) of every atom, the molecule in canonical atom order, and a SMILES string written from that order.

The device half is ``mdx_mol_canon`` (csrc/mdx_canon.hip), reached through ``canon_mols`` (a list of molecule dicts), ``launch`` (a
``CompactMols``) and ``FeaturizeMol.canon_batch`` (the sampler's predictions).  ``canon_ref`` is the plain restatement for one molecule
and needs no GPU; the GPU tests compare every output exactly.

What it is: the reference reports uniqueness and novelty from RDKit's canonical SMILES (utils/scoring_func.py:172-175) and writes a
SMILES per finished molecule (scripts/sample_drug3d.py:141-153).  RDKit is not available here, so this is THIS PROJECT'S OWN
DEFINITION, stated exactly in include/moldiff_hip.h: NOT RDKit's canonical ranking, and the strings of ``smiles`` are NOT RDKit's
canonical SMILES.  They are canonical among runs of this project, which is what uniqueness and novelty need.

The definition in short.  Atom labels L(v) (the class index, or the caller's ``atom_label``); a colouring gives every atom "how many
atoms have a strictly smaller key".  Initially the key is L(v); a refinement round takes key(v) = c(v) * 2^32 + h(v) with
h(v) = sum over the valid bonds {v, u} of mix(mix(c(u) + 1) + type) (wrapping 32-bit; mix = murmur3's fmix32; type = the low 8 bits of
the bond type), until the colouring stops changing.  The search tree: a node whose colours are all distinct is a leaf; otherwise one
child per atom v of the non-singleton cell of smallest colour k (the others of the cell move to k + 1, then refinement).  No pruning.
A leaf's certificate is the ascending list of lo * 2^20 + hi * 2^8 + type over the valid bonds (lo < hi the ranks of the ends); the
smallest over all leaves is canonical, ``n_aut`` is the number of leaves that attain it, ``rank`` is the lexicographically smallest
rank vector among those, and ``orbit[v]`` is the smallest atom found at rank[v] in any of them.

    python -m moldiff_amd.canon stats samples_all.pt --out canon.npz [--ref] [--part finished]
    python -m moldiff_amd.canon compare a.npz b.npz
"""
import sys

import numpy as np

from . import molpack, rings
from .molpack import DEFAULT_ATOMIC_NUMBERS, jsd_counts, mol_graph, to_host
from .similarity import mix

MAX_ATOMS, MAX_BONDS = rings.MAX_ATOMS, rings.MAX_BONDS           # include/moldiff_hip.h: the caps of mdx_mol_rings
MAX_DEPTH = 64
MAX_NODES_LIMIT, DEFAULT_MAX_NODES = 1 << 20, 1 << 16
MAX_LABEL = 1 << 16
STATUS_OK, STATUS_TOO_LARGE, STATUS_ABANDONED = 0, 1, 2
# the columns of the device's per-molecule table, in its order (include/moldiff_hip.h: MDX_CANON_STATS)
STAT_KEYS = ('status', 'n_nodes', 'n_leaves', 'n_aut', 'canon_n_bonds')
MOL_KEYS = STAT_KEYS + ('cert_hash', 'n_atoms', 'n_bonds')
ATOM_KEYS = ('rank', 'orbit', 'canon_atom_type')                  # + canon_atom_label, canon_pos when the inputs were given
BOND_KEYS = ('canon_bond_type',)                                  # + canon_bond_index (2, bonds)
LAYOUT = molpack.Layout(MOL_KEYS, atom=ATOM_KEYS, bond=BOND_KEYS, index=('canon_bond_index',), pos=('canon_pos',),
                        optional=('canon_atom_label',), int64=('cert_hash',))          # the results table
NODE_BINS = 22                                                    # bin k: molecules whose n_nodes have bit length k
FNV_OFFSET, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3
SYMBOL = molpack.ELEMENT_SYMBOL
SMILES_VALENCES = {6: (4,), 7: (3, 5), 8: (2,), 9: (1,), 15: (3, 5), 16: (2, 4, 6), 17: (1,)}   # what a SMILES reader assumes
_M = np.uint64(0xffffffff)


def _check_nodes(max_nodes):
    if not 1 <= int(max_nodes) <= MAX_NODES_LIMIT:
        raise ValueError(f'max_nodes must lie in 1 .. 2^20, got {max_nodes}')
    return int(max_nodes)


def _check_label(label, n):
    label = np.asarray(label, dtype=np.int64).reshape(-1)
    if len(label) != n:
        raise ValueError(f'atom_label holds {len(label)} values for {n} atoms')
    if ((label < 0) | (label >= MAX_LABEL)).any():
        raise ValueError('an atom label lies in 0 .. 65535')
    return label


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

class Abandoned(Exception):
    """the search tree has more than max_nodes nodes or a node deeper than 64"""


def _ranks(keys):
    """how many keys are strictly smaller, per key"""
    return np.searchsorted(np.sort(keys), keys, side='left').astype(np.int64)


def search(label, bx, by, btype, max_nodes, leaf):
    """The search tree of the definition over the labels (n) and the valid bonds bx - by of types `btype` (uint64): ``leaf(c)`` is called
    with the rank vector of every leaf, in the order of the walk (``canon_ref`` and ``stereo.stereo_ref`` are its two visitors) -> the
    number of nodes, the root counted.  Raises ``Abandoned`` at node max_nodes + 1 or at a node deeper than 64."""
    n = len(label)
    src, dst, typ = np.concatenate([bx, by]), np.concatenate([by, bx]), np.concatenate([btype, btype])
    nodes = [0]

    def refine(c):
        while True:
            h = np.zeros(n, dtype=np.uint64)
            np.add.at(h, src, mix(mix(c[dst].astype(np.uint64) + np.uint64(1)) + typ))
            new = _ranks((c.astype(np.uint64) << np.uint64(32)) | (h & _M))
            if np.array_equal(new, c):
                return c
            c = new

    def visit(c, depth):
        nodes[0] += 1
        if nodes[0] > max_nodes or depth > MAX_DEPTH:
            raise Abandoned
        cells = np.bincount(c, minlength=max(n, 1))
        big = np.flatnonzero(cells > 1)
        if len(big) == 0:
            leaf(c)
            return
        k = int(big[0])
        for v in np.flatnonzero(c == k):
            child = np.where((c == k) & (np.arange(n) != v), k + 1, c)
            visit(refine(child), depth + 1)

    visit(refine(_ranks(label)), 0)
    return nodes[0]


def fnv1a64(values):
    """FNV-1a-64 over int32 values taken as uint32, one step per value -> int (the int64 the device writes)"""
    h = FNV_OFFSET
    for w in values:
        h = ((h ^ (int(w) & 0xffffffff)) * FNV_PRIME) & 0xffffffffffffffff
    return h - (1 << 64) if h >= 1 << 63 else h


def canon_ref(info, atom_label=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """Plain restatement of ``mdx_mol_canon`` for one molecule dict (element = atomic numbers, bond_index (2, 2b) with every bond once
    and then flipped, bond_type (2b), optionally atom_pos) -> dict: ``status`` (0 measured, 1 more than 256 atoms or 512 bonds, 2 search
    abandoned: more than `max_nodes` nodes or a node deeper than 64), ``n_nodes``, ``n_leaves``, ``n_aut``, ``cert_hash``,
    ``canon_n_bonds`` (the valid bonds), ``n_atoms``, ``n_bonds``; per atom ``rank``, ``orbit``, ``canon_atom_type`` (and
    ``canon_atom_label`` with `atom_label`, ``canon_pos`` when the dict holds positions); per bond slot ``canon_bond_index`` (2, nb)
    and ``canon_bond_type``, the valid bonds in certificate order and zeros behind them.  With a non-zero status rank is -1 and every
    other output is 0.  A bond with an index outside the molecule or with i = j is ignored; several bonds between one pair of atoms
    are a multiset.  atom_label: int in [0, 65536) per atom, else ValueError; an element outside `atomic_numbers` raises ValueError."""
    max_nodes = _check_nodes(max_nodes)
    cls, bi, bt = mol_graph(info, atomic_numbers)
    n, nb = len(cls), bi.shape[1]
    label = cls.astype(np.int64) if atom_label is None else _check_label(atom_label, n)
    pos = np.asarray(info['atom_pos'], dtype=np.float32).reshape(n, 3) if 'atom_pos' in info else None
    zi = lambda *k: np.zeros(k, dtype=np.int32)
    out = dict({k: 0 for k in STAT_KEYS}, cert_hash=0, n_atoms=n, n_bonds=nb, rank=np.full(n, -1, dtype=np.int32), orbit=zi(n),
               canon_atom_type=zi(n), canon_bond_index=zi(2, nb), canon_bond_type=zi(nb))
    if atom_label is not None:
        out['canon_atom_label'] = zi(n)
    if pos is not None:
        out['canon_pos'] = np.zeros((n, 3), dtype=np.float32)
    if n > MAX_ATOMS or nb > MAX_BONDS:
        return dict(out, status=STATUS_TOO_LARGE)
    ok = (bi[0] >= 0) & (bi[0] < n) & (bi[1] >= 0) & (bi[1] < n) & (bi[0] != bi[1]) if nb else np.zeros(0, dtype=bool)
    bx, by, btype = bi[0][ok], bi[1][ok], (bt[ok] & 0xff).astype(np.uint64)
    best = {'cert': None, 'n_aut': 0, 'rank': None, 'table': None}
    count = {'leaves': 0}

    def leaf(c):
        count['leaves'] += 1
        lo, hi = np.minimum(c[bx], c[by]), np.maximum(c[bx], c[by])
        cert = sorted((lo * (1 << 20) + hi * (1 << 8) + btype.astype(np.int64)).tolist())
        if best['cert'] is None or cert < best['cert']:
            best.update(cert=cert, n_aut=1, rank=c.copy(), table=np.argsort(c))
        elif cert == best['cert']:
            best['n_aut'] += 1
            if c.tolist() < best['rank'].tolist():
                best['rank'] = c.copy()
            best['table'] = np.minimum(best['table'], np.argsort(c))

    try:
        count['nodes'] = search(label, bx, by, btype, max_nodes, leaf)
    except Abandoned:
        return dict(out, status=STATUS_ABANDONED)
    rank, words = best['rank'], best['cert']
    inv = np.argsort(rank)                                             # the atom of rank p
    out.update(n_nodes=count['nodes'], n_leaves=count['leaves'], n_aut=best['n_aut'], canon_n_bonds=len(words),
               rank=rank.astype(np.int32), orbit=best['table'][rank].astype(np.int32), canon_atom_type=cls[inv].astype(np.int32))
    if atom_label is not None:
        out['canon_atom_label'] = label[inv].astype(np.int32)
    if pos is not None:
        out['canon_pos'] = pos[inv]
    w = np.asarray(words, dtype=np.int64)
    out['canon_bond_index'][0, :len(w)], out['canon_bond_index'][1, :len(w)] = w >> 20, (w >> 8) & 0xfff
    out['canon_bond_type'][:len(w)] = w & 0xff
    out['cert_hash'] = fnv1a64([n] + label[inv].tolist() + [len(words)] + words)
    return out


def stack_ref(mols, atom_label=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """``canon_ref`` of every molecule of a list as the results dict ``canon_mols`` returns (numpy): one entry per molecule of every
    key of MOL_KEYS (int32, cert_hash int64), the per-atom keys over the atoms and the per-bond keys over the bond slots of the list
    in turn (canon_bond_index (2, bonds)), ``atom_ptr`` and ``bond_ptr``.  atom_label: one array per molecule, or None.  ``canon_pos``
    is present when every molecule holds positions."""
    refs = [canon_ref(m, None if atom_label is None else atom_label[k], max_nodes, atomic_numbers) for k, m in enumerate(mols)]
    return molpack.stack(refs, LAYOUT, optional=LAYOUT.optional if atom_label is not None else ())


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, max_nodes=DEFAULT_MAX_NODES, select=None, atom_label=None, positions=True):
    """``mdx_mol_canon`` on the device arrays `cm` (a ``CompactMols``) -> dict of device tensors: the keys of STAT_KEYS (B) each (int32,
    columns of one (B, 5) table), ``cert_hash`` (B, int64), ``rank`` / ``orbit`` / ``canon_atom_type`` (N_cap), ``canon_bond_index``
    (2, Eh_stride) and ``canon_bond_type`` (Eh_stride) in the layout of the inputs, zero where no molecule has a slot;
    ``canon_atom_label`` with `atom_label` (an int32 device tensor in the layout of atom_type, values in [0, 65536): the caller's
    word, not checked on the device) and ``canon_pos`` (N_cap, 3) when `cm` holds positions and `positions` is set.  No sync."""
    import torch
    from . import _lib
    max_nodes = _check_nodes(max_nodes)
    pos = cm.atom_pos if positions else None
    if atom_label is not None:
        if atom_label.dtype != torch.int32 or atom_label.numel() < cm.N_cap:
            raise ValueError('atom_label is an int32 tensor in the layout of atom_type')
        atom_label = atom_label.contiguous()
    out, stats = molpack.zeros_for(cm, LAYOUT, stat_keys=STAT_KEYS,
                                   held=(LAYOUT.optional if atom_label is not None else ()) + (LAYOUT.pos if pos is not None else ()))
    if cm.B > 0:
        ops, at = cm.operands()
        opt = lambda t: None if t is None else at(t)
        _lib.check(_lib.lib().mdx_mol_canon(
            *ops, _lib.ptr(select), opt(pos), opt(atom_label), max_nodes, at(out['rank']), at(out['orbit']), at(out['canon_atom_type']),
            opt(out.get('canon_atom_label')), opt(out.get('canon_pos')), at(out['canon_bond_index']), at(out['canon_bond_type']),
            at(stats), at(out['cert_hash']), _lib.stream()))
    return molpack.split_stats(out, stats, STAT_KEYS)


def canonical_compact(cm, results, select=None):
    """The canonical arrays of ``launch``'s results as a ``CompactMols`` in the layout of `cm` (same atom_ptr / bond_ptr, the bond
    counts ``canon_n_bonds``), and the `select` that leaves out every molecule without a canonical form (non-zero status) besides
    those `select` already leaves out -> (CompactMols, select): what ``kekule.launch``, ``groups.launch`` and ``rings.launch`` take."""
    import torch
    keep = (results['status'] == 0).to(torch.int32)
    if select is not None:
        keep = keep * (select != 0).to(torch.int32)
    canon = cm._replace(n_bonds=results['canon_n_bonds'].contiguous(), atom_type=results['canon_atom_type'], N_cap=cm.N_cap,
                        bond_type=results['canon_bond_type'], bond_index=results['canon_bond_index'],
                        Eh_stride=int(results['canon_bond_index'].shape[1]), atom_pos=results.get('canon_pos'))
    return canon, keep.contiguous()


def canon_mols(mols, device, atom_label=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """Canonical labelling of a list of molecule dicts (finished molecules, or entries of ``samples_all.pt``) on the device: the list
    is packed densely, copied and handed to ``mdx_mol_canon``.  -> the results dict of ``stack_ref`` with device tensors.  atom_label:
    one array per molecule (checked here: int in [0, 65536)), or None."""
    import torch
    _check_nodes(max_nodes)
    p, cm = molpack.packed(mols, atomic_numbers, device, positions=True, simple=False)
    lab = None
    if atom_label is not None:
        if len(atom_label) != len(mols):
            raise ValueError('one label array per molecule')
        lab = np.concatenate([_check_label(a, int(n)) for a, n in zip(atom_label, p['n_atoms'])] + [np.zeros(0, dtype=np.int64)])
        lab = torch.from_numpy(lab.astype(np.int32)).to(cm.device)
    return molpack.dense(launch(cm, max_nodes, atom_label=lab), cm, p, LAYOUT)


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict"""
    return molpack.concat(parts, LAYOUT)


def empty():
    return stack_ref([])


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def mol_result(results, m):
    """molecule `m` of a results dict with host arrays as the dict ``canon_ref`` returns"""
    return molpack.mol_slice(results, m, LAYOUT)


def certificate(results, m):
    """The full certificate of molecule `m` of a results dict with host arrays, as bytes: the int32 sequence n, the labels at ranks
    0 .. n - 1, the number of valid bonds, the words.  Two measured molecules are the same labelled graph iff these are equal.
    None for a molecule that was not measured (non-zero status)."""
    return certificate_of(mol_result(results, m))


def certificate_of(r):
    """the full certificate of one molecule's result (``canon_ref``'s dict or a ``mol_result`` slice): the one definition of the bytes"""
    if int(r['status']) != STATUS_OK:
        return None
    k = int(r['canon_n_bonds'])
    labels = r['canon_atom_label'] if 'canon_atom_label' in r else r['canon_atom_type']
    bi = np.asarray(r['canon_bond_index'])[:, :k].astype(np.int64)
    words = bi[0] * (1 << 20) + bi[1] * (1 << 8) + np.asarray(r['canon_bond_type'])[:k]
    return np.concatenate([[int(r['n_atoms'])], labels, [k], words]).astype(np.int32).tobytes()


def canonical_mol(info, result):
    """The molecule dict `info` in canonical atom order from its result (``canon_ref``'s dict or a ``mol_result`` slice): ``element``,
    ``bond_index`` (2, 2b) with the valid bonds in certificate order once and then flipped, ``bond_type`` (2b), ``atom_pos`` when
    `info` holds positions.  Isomorphic inputs give identical dicts apart from the positions.  None without a canonical form."""
    if int(result['status']) != STATUS_OK:
        return None
    inv = np.argsort(np.asarray(result['rank']))
    k = int(result['canon_n_bonds'])
    bi, bt = np.asarray(result['canon_bond_index'])[:, :k].astype(np.int64), np.asarray(result['canon_bond_type'])[:k].astype(np.int64)
    out = {'element': np.asarray(info['element'], dtype=np.int64).reshape(-1)[inv],
           'bond_index': np.concatenate([bi, bi[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}
    if 'atom_pos' in info:
        out['atom_pos'] = np.asarray(info['atom_pos'])[inv]
    return out


def _certificates(results):
    r = to_host(results)
    return [certificate(r, m) for m in range(len(r['status']))]


def summary(results):
    """The numbers of a results dict (host or device arrays) -> dict: ``n_molecules``, ``n_measured`` (status 0), ``n_too_large``,
    ``n_abandoned``; over the measured molecules ``n_distinct`` (distinct full certificates: EXACT, unlike the fingerprint key of
    ``similarity.summary``), ``uniqueness`` = n_distinct / n_measured, ``mean_n_aut``, ``max_n_aut`` and ``nodes_hist`` (bin k:
    n_nodes of bit length k, i.e. 1, 2-3, 4-7, ...).  NaN where nothing was counted.  The labelling is this project's own."""
    r = to_host(results)
    ok = r['status'] == STATUS_OK
    k = int(ok.sum())
    nan = float('nan')
    certs = {c for c in _certificates(r) if c is not None}
    bits = np.asarray([min(int(s).bit_length(), NODE_BINS - 1) for s in r['n_nodes'][ok]], dtype=np.int64)
    return {'n_molecules': len(ok), 'n_measured': k, 'n_too_large': int((r['status'] == STATUS_TOO_LARGE).sum()),
            'n_abandoned': int((r['status'] == STATUS_ABANDONED).sum()), 'n_distinct': len(certs),
            'uniqueness': len(certs) / k if k else nan, 'mean_n_aut': float(r['n_aut'][ok].astype(np.int64).sum()) / k if k else nan,
            'max_n_aut': int(r['n_aut'][ok].max()) if k else 0, 'nodes_hist': np.bincount(bits, minlength=NODE_BINS).tolist()}


def novelty(results, reference_results):
    """the fraction of the measured molecules of `results` whose full certificate occurs nowhere among the measured molecules of
    `reference_results` (NaN when nothing was measured).  Both sides must have been labelled alike (atom_label or not)."""
    known = {c for c in _certificates(reference_results) if c is not None}
    mine = [c for c in _certificates(results) if c is not None]
    return sum(c not in known for c in mine) / len(mine) if mine else float('nan')


def compare(a, b):
    """two results dicts -> dict: Jensen-Shannon divergence (``molpack.jsd_counts``) of ``nodes_hist``, both sides' ``uniqueness``
    and ``mean_n_aut``, and the novelty of each side against the other by full certificate"""
    sa, sb = summary(a), summary(b)
    return {'nodes': jsd_counts(sa['nodes_hist'], sb['nodes_hist']), 'uniqueness': [sa['uniqueness'], sb['uniqueness']],
            'mean_n_aut': [sa['mean_n_aut'], sb['mean_n_aut']], 'novelty': [novelty(a, b), novelty(b, a)]}


# ---- SMILES -------------------------------------------------------------------------------------------------------------------------

def assumed_hydrogens(z, bond_sum):
    """what a SMILES reader assumes on an unbracketed atom: the smallest of the element's SMILES valences that is at least the
    bond-order sum, minus that sum; 0 when the sum is above all of them"""
    if int(z) not in SMILES_VALENCES:
        raise ValueError(f'no SMILES valences for element {int(z)}')
    return next((v - bond_sum for v in SMILES_VALENCES[int(z)] if v >= bond_sum), 0)


def _stereo_marks(n, nbr, kek_h, stereo):
    """What ``smiles`` writes for a stereo result in the canonical frame -> (tetra, slash): tetra {atom: True when its neighbours in
    ascending index, an implicit H first, run anticlockwise seen from the first}; slash {(lo, hi): +1 | -1}, the direction of the
    single bond lo - hi written lo first ('/' for +1), for the reference bonds of the marked double bonds."""
    codes = np.asarray(stereo['canon_tetra'], dtype=np.int64).reshape(-1)
    bcodes = np.asarray(stereo['canon_bond_stereo'], dtype=np.int64).reshape(-1)
    tetra = {}
    for a in range(min(n, len(codes))):
        if codes[a] in (1, 2) and len(nbr[a]) + int(kek_h[a]) == 4 and int(kek_h[a]) <= 1:
            # code 1: the determinant of the definition is positive for the neighbours in ascending rank, which is CLOCKWISE seen from
            # the first of them (or from the implicit H); hand-derived, unchecked against RDKit
            tetra[a] = codes[a] == 2
    var, refs, rules = {}, [], []                                      # dir(lo -> hi); reference bonds; (p, q, r, t, sign): dir(p->q) dir(r->t) = sign
    key = lambda u, v: (min(u, v), max(u, v))
    get = lambda u, v: None if key(u, v) not in var else var[key(u, v)] * (1 if u < v else -1)

    def put(u, v, d):
        var[key(u, v)] = d if u < v else -d
    for a in range(n):
        for b, o, e in nbr[a]:
            if a < b and o == 2 and e < len(bcodes) and bcodes[e] in (1, 2):
                xs, ys = [u for u in nbr[a] if u[0] != b], [u for u in nbr[b] if u[0] != a]
                if not xs or not ys or any(u[1] != 1 for u in xs + ys):
                    continue
                refs += [key(a, xs[0][0]), key(b, ys[0][0])]
                rules.append((a, xs[0][0], b, ys[0][0], 1 if bcodes[e] == 1 else -1))      # cis: both bonds point the same way
                rules += [(c, us[0][0], c, us[1][0], -1) for c, us in ((a, xs), (b, ys)) if len(us) == 2]
    pending = True
    while pending:
        pending = False
        for p_, q, r, t, sign in rules:
            d1, d2 = get(p_, q), get(r, t)
            if d1 is not None and d2 is not None:
                if d1 * d2 != sign:
                    return tetra, {}                                   # contradictory codes around a ring: no slash is written
            elif d1 is not None:
                put(r, t, d1 * sign)
                pending = True
            elif d2 is not None:
                put(p_, q, d2 * sign)
                pending = True
        if not pending:
            seed = next((rule for rule in rules if get(rule[0], rule[1]) is None and key(rule[0], rule[1]) in refs), None)
            if seed is not None:
                put(seed[0], seed[1], -1)                              # the first reference bond reads '/' when its substituent is written first
                pending = True
    return tetra, {k: var[k] for k in refs if k in var}


def smiles(canon_mol, kekule_result, stereo=None):
    """A SMILES string of the CANONICAL molecule (``canonical_mol``) from the Kekulé result of THAT molecule (``kekule.kekulize_ref``
    of it, or a ``kekule.mol_result`` slice of ``kekule.launch`` on the canonical arrays): that is what makes the Kekulé structure,
    and so the string, independent of the sampler's atom order.  THIS PROJECT'S OWN STRING: its grammar is unchecked against RDKit
    offline, it is not RDKit's canonical SMILES and it is canonical only among this project's runs.

    Kekulé form only: upper-case atoms, bond orders 1 / 2 / 3 from ``kek_order`` ('', '=', '#').  Every fragment starts at its atom
    of lowest rank, fragments in rank order joined by '.'; depth-first, neighbours in ascending rank, all but the last in
    parentheses.  Ring-closure digits are allotted in order of opening (at one atom: by the rank of the closing atom) and are free
    again from the atom after the one that closes them; '%nn' from 10 on; at an atom the closing digits come first; the bond symbol
    of a ring closure goes at its opening.  An atom is bracketed iff its charge is non-zero or its ``kek_h`` differs from
    ``assumed_hydrogens``; a bracket atom writes H, H2, ... and +.  -> None when `canon_mol` is None, the molecule is not
    kekulizable or a bond has no order (a type outside the featuriser's).

    stereo: None, and the string is the constitutional one; or the stereo result of the molecule (``stereo.stereo_ref``'s dict or a
    ``stereo.mol_result`` slice), and the string is ISOMERIC.  The canonical arrays are the same under every optimal leaf, so
    `canon_mol` is also the molecule in the order of ``stereo_rank``, the frame in which ``canon_tetra`` and ``canon_bond_stereo`` (W)
    are stated: the string is a function of the isomeric key.  A centre with a non-zero code becomes a bracket atom with '@' or '@@'
    and its H (when its bonds and hydrogens make four neighbours, at most one of them H); the neighbour order of OpenSMILES is the
    preceding atom, the implicit H, the ring-closure digits as written, the branches.  A candidate double bond with a non-zero code
    gets '/' or '\\' on one single bond at each end (the other neighbour of smallest rank), ring closures at their opening; where
    the codes around a ring of conjugated candidates contradict each other no slash is written at all.  The handedness convention and
    the slash rule are HAND-DERIVED from the OpenSMILES text and UNCHECKED against RDKit."""
    from . import kekule
    if canon_mol is None:
        return None
    if not bool(kekule.kekulizable({k: np.asarray(kekule_result[k]) for k in ('status', 'n_failed', 'n_over_budget')})):
        return None
    ele = np.asarray(canon_mol['element'], dtype=np.int64).reshape(-1)
    n = len(ele)
    bi = np.asarray(canon_mol['bond_index'], dtype=np.int64).reshape(2, -1)
    nb = bi.shape[1] // 2
    order = np.asarray(kekule_result['kek_order'], dtype=np.int64)[:nb]
    if len(order) != nb or (order < 1).any() or (order > 3).any():
        return None
    charge, kek_h = np.asarray(kekule_result['charge'], dtype=np.int64), np.asarray(kekule_result['kek_h'], dtype=np.int64)
    nbr = [[] for _ in range(n)]
    for e in range(nb):
        x, y = int(bi[0, e]), int(bi[1, e])
        nbr[x].append((y, int(order[e]), e)), nbr[y].append((x, int(order[e]), e))
    for a in range(n):
        nbr[a].sort()
    # pass 1: the spanning forest and the ring closures (a closure opens at the atom visited first, an ancestor of the other)
    seen, used = [False] * n, [False] * nb
    children, opens, closes = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]
    roots = []
    for root in range(n):
        if seen[root]:
            continue
        roots.append(root)
        seen[root] = True
        stack = [(root, 0)]
        while stack:
            a, k = stack.pop()
            if k == len(nbr[a]):
                continue
            stack.append((a, k + 1))
            b, o, e = nbr[a][k]
            if used[e]:
                continue
            used[e] = True
            if seen[b]:
                opens[b].append((a, o)), closes[a].append(b)
            else:
                seen[b] = True
                children[a].append((b, o))
                stack.append((b, 0))
    tetra, slash = _stereo_marks(n, nbr, kek_h, stereo) if stereo is not None and int(stereo['status']) == 0 else ({}, {})
    sym = {1: '', 2: '=', 3: '#'}

    def bond_text(a, b, o):
        d = slash.get((min(a, b), max(a, b))) if o == 1 else None
        return sym[o] if d is None else '/' if d * (1 if a < b else -1) > 0 else '\\'
    digit = lambda d: str(d) if d < 10 else '%%%02d' % d
    free, taken = [], {}                                               # freed digits (kept sorted), (opener, closer) -> digit
    nxt = [1]

    def atom_text(a, parent):
        z, bond_sum = int(ele[a]), sum(o for _, o, _ in nbr[a])
        if z not in SYMBOL:
            raise ValueError(f'no symbol for element {z}')
        h, q = int(kek_h[a]), int(charge[a])
        mark = ''
        if a in tetra:
            listed = ([] if parent is None else [parent]) + [-1] * h + sorted(closes[a]) + [b for b, _ in sorted(opens[a])] + [b for b, _ in children[a]]
            odd = sum(listed[i] > listed[j] for i in range(4) for j in range(i + 1, 4)) & 1
            mark = '@' if tetra[a] != bool(odd) else '@@'
        if q == 0 and h == assumed_hydrogens(z, bond_sum) and not mark:
            return SYMBOL[z]
        return '[' + SYMBOL[z] + mark + ('H' + (str(h) if h > 1 else '') if h else '') + \
            (('+' if q > 0 else '-') + (str(abs(q)) if abs(q) > 1 else '') if q else '') + ']'

    def write(a, parent=None):
        text, freed = atom_text(a, parent), []
        for b in sorted(closes[a]):
            d = taken.pop((b, a))
            text += digit(d)
            freed.append(d)
        for b, o in sorted(opens[a]):
            if free:
                d = free.pop(0)
            else:
                d, nxt[0] = nxt[0], nxt[0] + 1
            taken[(a, b)] = d
            text += bond_text(a, b, o) + digit(d)
        free.extend(freed)
        free.sort()
        for k, (b, o) in enumerate(children[a]):
            sub = bond_text(a, b, o) + write(b, a)
            text += sub if k == len(children[a]) - 1 else '(' + sub + ')'
        return text
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * MAX_ATOMS + 100))
    try:
        return '.'.join(write(r) for r in roots)
    finally:
        sys.setrecursionlimit(limit)


def smiles_mols(mols, results, device=None, tables=None, stereo=None):
    """``smiles`` of every molecule of a list from its results dict (host arrays, one entry per molecule): the canonical molecules
    are kekulized together, on `device` (``kekule.kekulize_mols``) or with ``kekule.kekulize_ref`` when it is None -> a list of
    strings, None where a molecule has none.  stereo: the stereo results of the same list (``stereo.stack_ref`` / ``stereo_mols``,
    host arrays) for isomeric strings, or None"""
    from . import kekule
    from .stereo import mol_result as stereo_of
    canon = [canonical_mol(info, mol_result(results, m)) for m, info in enumerate(mols)]
    have = [m for m, c in enumerate(canon) if c is not None]
    out = [None] * len(mols)
    if not have:
        return out
    if device is None:
        kek = kekule.stack_ref([canon[m] for m in have], tables)
    else:
        kek = to_host(kekule.kekulize_mols([canon[m] for m in have], device, tables))
    for k, m in enumerate(have):
        out[m] = smiles(canon[m], kekule.mol_result(kek, k), None if stereo is None else stereo_of(stereo, m))
    return out


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    return molpack.stats_main(
        argv, 'canon', __doc__, ('canonical labelling of the molecules stored in a samples_all.pt',
                                 'node-count divergence, uniqueness and mutual novelty of two files'),
        [('--max_nodes', dict(type=int, default=DEFAULT_MAX_NODES))],
        lambda mols, a, dev: stack_ref(mols, max_nodes=a.max_nodes) if dev is None else canon_mols(mols, dev, max_nodes=a.max_nodes),
        summary, compare)


if __name__ == '__main__':
    sys.exit(main())
