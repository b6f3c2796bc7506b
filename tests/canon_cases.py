"""Cases and oracles for the tests of the canonical labelling (test_canon_host.py, test_gpu_canon.py): small labelled graphs, seeded
random ones, permuted copies, a brute force over all atom permutations that knows nothing of refinement or search, and a small SMILES
reader that covers exactly the grammar ``canon.smiles`` writes."""
import itertools
import re

import numpy as np

from moldiff_amd import canon as C

ELEMENTS = (6, 7, 8, 9, 15, 16, 17)


def mol(ele, bonds, pos=False):
    """a molecule dict: `ele` atomic numbers (an int n: n carbons), bonds (i, j[, type]) once each; bond type 1 by default"""
    ele = [6] * ele if isinstance(ele, int) else ele
    bonds = [tuple(b) + (1,) * (3 - len(b)) for b in bonds]
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    out = {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1),
           'bond_type': np.asarray(bt + bt, dtype=np.int64)}
    if pos:
        out['atom_pos'] = (np.arange(3 * len(ele), dtype=np.float32).reshape(-1, 3) * 0.25 - 1.5)
    return out


def ring(n, first=0, t=1):
    return [(first + k, first + (k + 1) % n, t) for k in range(n)]


def chain(n, t=1):
    return mol(n, [(k, k + 1, t) for k in range(n - 1)])


CUBE = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
# cuneane: 8 CH, 3-regular like cubane, with two three-rings, two four-rings and two five-rings
CUNEANE = [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (0, 6), (3, 6), (1, 7), (4, 7), (2, 5), (6, 7)]
NAMED = {
    'benzene': mol(6, ring(6, t=4)),
    'pyridine': mol([7] + [6] * 5, ring(6, t=4)),
    'cubane': mol(8, CUBE),
    'cuneane': mol(8, CUNEANE),
    'six_ring': mol(6, ring(6)),
    'two_three_rings': mol(6, ring(3) + ring(3, 3)),
    'two_equal_fragments': mol([6, 8, 6, 8], [(0, 1, 2), (2, 3, 2)]),
    'star': mol(5, [(0, 1), (0, 2), (0, 3), (0, 4)]),
    'mirror': mol(6, ring(5) + [(0, 5, 2)]),                                # a five-ring with =C on atom 0: one mirror
    'broken_symmetry': mol(6, [(0, 1), (1, 2, 2), (2, 3), (3, 4), (4, 0), (0, 5, 2)]),     # the ring bond 1-2 doubled breaks it
    'one_label_changed': mol([6, 6, 7, 6, 6, 6], [(0, 1), (1, 2, 2), (2, 3), (3, 4), (4, 0), (0, 5, 2)]),
}
K5 = mol(5, [(i, j) for i in range(5) for j in range(i + 1, 5)])


def random_mol(seed, n_min=3, n_max=8, elements=(6, 7), types=(1, 2, 4)):
    """a chain with ring closures: atom k hangs on k - 1 (one time in five on any earlier atom), a few closures over 2 .. 4 bonds;
    two elements and three bond types, carbon and single bonds heavy, so that symmetric cases are common"""
    g = np.random.default_rng(seed)
    n = int(g.integers(n_min, n_max + 1))
    bonds = {(k - 1 if g.random() >= 0.2 else int(g.integers(0, k)), k) for k in range(1, n)}
    for _ in range(int(g.integers(0, n // 3 + 1))):
        i = int(g.integers(0, n))
        j = i + int(g.choice([2, 3, 4]))
        if j < n:
            bonds.add((i, j))
    ele = g.choice(list(elements), n, p=[0.8, 0.2])
    bt = g.choice(list(types), len(bonds), p=[0.7, 0.15, 0.15])
    return mol(ele, [(i, j, int(t)) for (i, j), t in zip(sorted(bonds), bt)])


def decorated(m):
    """`m` with three carbons on its first atom and two on its last (single bonds): a tert-butyl-like and a gem-dimethyl-like group,
    so that the automorphism group has at least 12 elements and the unpruned tree more than 20 nodes"""
    n, nb = len(m['element']), m['bond_index'].shape[1] // 2
    bonds = [(int(i), int(j), int(t)) for (i, j), t in zip(m['bond_index'][:, :nb].T, m['bond_type'][:nb])]
    bonds += [(0, n + k, 1) for k in range(3)] + [(n - 1, n + 3 + k, 1) for k in range(2)]
    return mol(m['element'].tolist() + [6] * 5, bonds)


def permuted(m, seed, label=None):
    """the same molecule with its atoms renumbered, its bonds reordered and some bond directions flipped -> (molecule, new, label):
    new[a] is the new index of atom a"""
    g = np.random.default_rng(seed)
    n = len(m['element'])
    new = g.permutation(n)
    nb = m['bond_index'].shape[1] // 2
    order = g.permutation(nb)
    flip = g.random(nb) < 0.5
    bi = new[m['bond_index'][:, :nb]].reshape(2, nb)[:, order]
    bi = np.where(flip[None, :], bi[::-1], bi)
    bt = m['bond_type'][:nb][order]
    out = {'element': np.zeros(n, dtype=np.int64), 'bond_index': np.concatenate([bi, bi[::-1]], axis=1).astype(np.int64),
           'bond_type': np.concatenate([bt, bt])}
    out['element'][new] = m['element']
    if 'atom_pos' in m:
        out['atom_pos'] = np.zeros_like(m['atom_pos'])
        out['atom_pos'][new] = m['atom_pos']
    lab = None
    if label is not None:
        lab = np.zeros(n, dtype=np.int64)
        lab[new] = label
    return out, new, lab


def cert(m, label=None, **kw):
    """the full certificate of one molecule dict by ``canon_ref``"""
    return C.certificate(C.stack_ref([m], None if label is None else [label], **kw), 0)


# ---- brute force over all atom permutations ------------------------------------------------------------------------------------------

_PERMS = {}


def _perms(n):
    if n not in _PERMS:
        _PERMS[n] = np.asarray(list(itertools.permutations(range(n))), dtype=np.int64).reshape(-1, n)
    return _PERMS[n]


def brute_force(m, label=None):
    """-> (form, n_aut, orbit): `form` is the smallest (labels, bond matrix) over ALL arrangements of the atoms, as bytes: equal for two
    molecules iff some permutation maps one onto the other; n_aut the arrangements equal to the given one; orbit[v] the smallest atom
    an automorphism maps v to.  The bond matrix holds per pair the sum of 16^type over its bonds (a multiset)."""
    lab = np.asarray(m['element'] if label is None else label, dtype=np.int64)
    n = len(lab)
    assert n <= 8
    M = np.zeros((n, n), dtype=np.int64)
    nb = m['bond_index'].shape[1] // 2
    for e in range(nb):
        i, j, t = int(m['bond_index'][0, e]), int(m['bond_index'][1, e]), int(m['bond_type'][e])
        if 0 <= i < n and 0 <= j < n and i != j:
            M[i, j] += 16 ** t
            M[j, i] += 16 ** t
    p = _perms(n)
    rows = np.concatenate([lab[p], M[p[:, :, None], p[:, None, :]].reshape(len(p), n * n)], axis=1).astype('>i8')
    keys = [r.tobytes() for r in rows]
    same = np.asarray([k == keys[0] for k in keys])                      # row 0 is the identity
    orbit = p[same].min(axis=0) if n else np.zeros(0, dtype=np.int64)
    return bytes([n]) + min(keys), int(same.sum()), orbit


# ---- a SMILES reader for exactly the grammar canon.smiles writes --------------------------------------------------------------------

_VALENCES = {6: (4,), 7: (3, 5), 8: (2,), 9: (1,), 15: (3, 5), 16: (2, 4, 6), 17: (1,)}
_NUMBER = {'C': 6, 'N': 7, 'O': 8, 'F': 9, 'P': 15, 'S': 16, 'Cl': 17}
_TOKEN = re.compile(r'\[(Cl|[CNOFPS])(?:H(\d*))?(?:([+-])(\d*))?\]|(Cl|[CNOFPS])|([=#])|(%\d\d|\d)|([().])')


def read_smiles(text):
    """-> (molecule dict with bond orders as types, hydrogens per atom, charge per atom); an unbracketed atom gets the smallest of its
    element's valences that is at least its bond-order sum, minus that sum"""
    ele, hs, charge, bonds = [], [], [], []
    prev, stack, pending, open_rings, k = None, [], 1, {}, 0
    while k < len(text):
        t = _TOKEN.match(text, k)
        assert t, (text, k)
        k = t.end()
        bsym, bh, sign, mag, sym, bond, closure, other = t.groups()
        if bsym or sym:
            ele.append(_NUMBER[bsym or sym])
            hs.append((int(bh) if bh else 1) if bsym and bh is not None else (0 if bsym else None))
            charge.append((int(mag) if mag else 1) * (1 if sign == '+' else -1) if sign else 0)
            a = len(ele) - 1
            if prev is not None:
                bonds.append((prev, a, pending))
            prev, pending = a, 1
        elif bond:
            pending = {'=': 2, '#': 3}[bond]
        elif closure:
            d = int(closure.lstrip('%'))
            if d in open_rings:
                b, o = open_rings.pop(d)
                bonds.append((b, prev, o))
            else:
                open_rings[d] = (prev, pending)
            pending = 1
        elif other == '(':
            stack.append(prev)
        elif other == ')':
            prev = stack.pop()
        else:
            prev = None
    assert not open_rings and not stack
    total = [0] * len(ele)
    for i, j, o in bonds:
        total[i] += o
        total[j] += o
    for a, z in enumerate(ele):
        if hs[a] is None:
            hs[a] = next((v - total[a] for v in _VALENCES[z] if v >= total[a]), 0)
    return mol(ele, bonds), np.asarray(hs, dtype=np.int64), np.asarray(charge, dtype=np.int64)


def fold(m, hs, charge):
    """the label class + 8 h + 64 charge per atom"""
    cls = np.asarray([ELEMENTS.index(int(z)) for z in m['element']], dtype=np.int64)
    return cls + 8 * np.asarray(hs, dtype=np.int64) + 64 * np.asarray(charge, dtype=np.int64)
