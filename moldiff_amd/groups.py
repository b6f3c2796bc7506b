"""Substructure matching on decoded molecules: how often, and at which atoms, a small labelled subgraph (a functional group) occurs.

The device half is ``mdx_mol_groups`` (csrc/mdx_groups.hip), reached through ``groups_mols`` (a list of molecule dicts) and
``FeaturizeMol.groups_batch`` (the sampler's predictions).  ``groups_ref`` is the plain Python restatement for one molecule and needs
no GPU; the GPU tests compare every output exactly.

What it is: the reference's ``groups_counts`` (utils/evaluation.py:86-94), the donor / acceptor counts of ``count_prop`` (:27-28), its
PAINS filter and the SMARTS counts of ``Local3D.get_counts`` all ask RDKit "does this pattern occur, how often, where".  RDKit is not
available here, so the question is answered by a matcher and a PATTERN LANGUAGE OF THIS PROJECT'S OWN (include/moldiff_hip.h defines
both).  It is NOT SMARTS and the default set (configs/groups_default.yml) is NOT RDKit's ``Fragments``: there is no negation, no
recursion, no charge, and hydrogens are implicit and derived from a table of normal valences that is this project's choice
(``DEFAULT_NORMAL_VALENCE``: C 4, N 3, O 2, F 1, P 3, S 2, Cl 1), unverified against RDKit.

A pattern is a connected graph of 1 .. 8 atoms and 0 .. 12 bonds.  A pattern atom constrains the element, the number of bonds, the
implicit hydrogens, the smallest ring through the atom and whether the atom carries an aromatic bond (the last bond type); a pattern
bond constrains the bond type and the smallest ring through the bond.  An EMBEDDING is an injective map of pattern atoms to molecule
atoms that satisfies all of them; matching is non-induced.  Every output is defined so that its value is unique:

  * ``n_embed``  the number of embeddings; ``n_match = n_embed / |Aut(pattern)|`` on the host (``n_match``), an exact division.  That
    is RDKit's uniquified match count except where one atom set carries several inequivalent embeddings: a 3-atom path in a triangle
    gives 3 here and 1 there;
  * ``n_anchor`` / ``atom_hit``  the distinct atoms that are the image of pattern atom 0 (the ANCHOR: the first atom listed);
  * ``steps``  the candidates tested, by a formula in which no traversal order enters; ``max_steps`` bounds it per start atom, and a
    pattern whose search exceeds it in a molecule gets ``pat_status`` 3 and zeros there.  Untrained weights bond nearly every pair of
    atoms; without the budget a wildcard pattern of 8 atoms would never finish.

With no trained checkpoint offline this is an instrument, not a measurement of quality.

    python -m moldiff_amd.groups stats samples_all.pt --out groups.npz [--patterns P.yml] [--ref] [--part finished]
    python -m moldiff_amd.groups compare a.npz b.npz
"""
import os
import sys

import numpy as np

from . import molpack, rings
from .molpack import check_steps, DEFAULT_ATOMIC_NUMBERS, DEFAULT_NORMAL_VALENCE, jsd_counts, mol_graph, OverBudget, to_host

MAX_ATOMS, MAX_BONDS = rings.MAX_ATOMS, rings.MAX_BONDS           # include/moldiff_hip.h: the caps of mdx_mol_rings
PAT_ATOMS, PAT_BONDS, MAX_PATTERNS, RECORD = 8, 12, 32, 90        # include/moldiff_hip.h: MDX_GROUPS_*
MAX_STEPS_LIMIT, DEFAULT_MAX_STEPS = molpack.MAX_STEPS_LIMIT, 1 << 16
MAX_ELEMENTS, MAX_BOND_TYPES = 32, 16
ANY_RING = 0x7f
STATUS_OK, STATUS_TOO_LARGE, STATUS_NO_RINGS, PAT_OVER_BUDGET = 0, 1, 2, 3
MOL_KEYS = ('status', 'n_atoms', 'n_embed', 'n_anchor', 'steps', 'pat_status')
SLOT_KEYS = ('atom_hit',)
SET_KEYS = ('aut', 'names')
# the results table (molpack.Layout): neither n_bonds nor bond_ptr; every wide key has one column per pattern
LAYOUT = molpack.Layout(MOL_KEYS, atom=SLOT_KEYS, wide=('n_embed', 'n_anchor', 'steps', 'pat_status'))
DEFAULT_PATTERNS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'groups_default.yml')
SYMBOLS = molpack.ELEMENT_NUMBER


def ring_class(r):
    """the class of a ``bond_ring_min`` / ``atom_ring_min`` value: 0 no ring, 1 .. 5 smallest ring 3 .. 7, 6 a ring of 8 or more"""
    return 0 if r <= 0 else min(max(int(r), 3), 8) - 2


# ---- patterns -----------------------------------------------------------------------------------------------------------------------

def _bits(values, allowed, what, saturate=None):
    """a list of ints (or one int) as a bit mask; `saturate`: a value at or above it sets the top bit"""
    values = [values] if isinstance(values, (int, np.integer)) else list(values)
    mask = 0
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'{what}: {v!r} is not an integer')
        v = int(v)
        if saturate is not None and v >= saturate:
            v = saturate
        if v not in allowed:
            raise ValueError(f'{what}: {v} is not among {sorted(allowed)}')
        mask |= 1 << v
    if not mask:
        raise ValueError(f'{what}: an empty list matches nothing')
    return mask


def _ring_mask(spec, what):
    """'any' (or None) | 'ring' | 'none' | a list of 0 (no ring bond), 3 .. 7, 8 (8 or more) -> the 7-bit mask"""
    if spec is None or spec == 'any':
        return ANY_RING
    if spec == 'ring':
        return ANY_RING & ~1
    if spec == 'none':
        return 1
    spec = [spec] if isinstance(spec, (int, np.integer)) else list(spec)
    mask = 0
    for r in spec:
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not (r == 0 or r >= 3):
            raise ValueError(f'{what}: ring size {r!r} is neither 0 (no ring) nor at least 3')
        mask |= 1 << ring_class(int(r))
    if not mask:
        raise ValueError(f'{what}: an empty list matches nothing')
    return mask


class Pattern:
    """one validated pattern: ``atoms`` = [(elem_mask, deg_mask, h_mask, rsize_mask, arom)], ``bonds`` = [(i, j, type_mask, rsize_mask)]
    with i < j, ordered so that every atom k > 0 has a bond to an earlier atom"""

    def __init__(self, name, atoms, bonds):
        self.name, self.atoms, self.bonds = str(name), [tuple(int(v) for v in a) for a in atoms], [tuple(int(v) for v in b) for b in bonds]
        na = len(self.atoms)
        self.bond_of = {(i, j): (t, r) for i, j, t, r in self.bonds}
        # the earliest neighbour of every atom k > 0 (its PARENT), the bond to it, and the other bonds to earlier atoms
        self.parent, self.tree, self.closures = [-1] * na, [None] * na, [[] for _ in range(na)]
        for k in range(1, na):
            earlier = sorted(i for (i, j) in self.bond_of if j == k)
            self.parent[k], self.tree[k] = earlier[0], self.bond_of[(earlier[0], k)]
            self.closures[k] = [(i,) + self.bond_of[(i, k)] for i in earlier[1:]]

    @property
    def needs_rings(self):
        return any(a[3] != ANY_RING for a in self.atoms) or any(b[3] != ANY_RING for b in self.bonds)

    def automorphisms(self):
        """|Aut|: the permutations of the pattern's atoms that preserve bonds and every constraint field exactly"""
        na, perm, used = len(self.atoms), [], set()
        get = lambda i, j: self.bond_of.get((min(i, j), max(i, j)))

        def extend(k):
            if k == na:
                return 1
            total = 0
            for c in range(na):
                if c in used or self.atoms[c] != self.atoms[k] or any(get(k, j) != get(c, perm[j]) for j in range(k)):
                    continue
                used.add(c), perm.append(c)
                total += extend(k + 1)
                used.discard(c), perm.pop()
            return total
        return extend(0)


class PatternSet:
    """A set of 1 .. 32 named patterns for one featuriser.  Built from dicts (``from_dict``) or a YAML file (``from_yaml``):

        patterns:
          - name: amide
            atoms:                    # atom 0 is the ANCHOR: n_anchor / atom_hit report its images
              - {elem: [C]}           # elem: symbols or atomic numbers, '*' = any (the default)
              - {elem: [O], deg: [1]} # deg: allowed numbers of bonds, 7 = 7 or more;  h: allowed implicit hydrogens, 4 = 4 or more
              - {elem: [N]}           # ring: 'any' (default) | 'ring' | 'none' | sizes of the smallest ring: 0 none, 3 .. 7, 8 = 8 or more
            bonds:                    # arom: true = carries a bond of the last type, false = carries none (default: either)
              - [0, 1, [2]]           # i, j, allowed bond types ('*' = any) and optionally the ring spec of the bond
              - [0, 2, [1]]

    Validation refuses a pattern that is not connected, has more than 8 atoms or 12 bonds, names an element outside the featuriser's,
    repeats a bond or a name; more than 32 patterns are refused too.  Atoms are reordered (atom 0 stays) so that every later atom has
    a bond to an earlier one, which is the order the device entry demands."""

    def __init__(self, patterns, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
        self.atomic_numbers, self.num_bond_types = tuple(int(z) for z in atomic_numbers), int(num_bond_types)
        if not 1 <= len(self.atomic_numbers) <= MAX_ELEMENTS or not 1 <= self.num_bond_types <= MAX_BOND_TYPES:
            raise ValueError(f'at most {MAX_ELEMENTS} elements and {MAX_BOND_TYPES} bond types')
        patterns = list(patterns)
        if not 1 <= len(patterns) <= MAX_PATTERNS:
            raise ValueError(f'a pattern set holds 1 .. {MAX_PATTERNS} patterns, got {len(patterns)}')
        self.patterns = [p if isinstance(p, Pattern) else self._build(p, k) for k, p in enumerate(patterns)]
        self.names = [p.name for p in self.patterns]
        if len(set(self.names)) != len(self.names):
            raise ValueError('two patterns share a name')

    @classmethod
    def from_dict(cls, d, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
        return cls((d or {}).get('patterns') or [], atomic_numbers, num_bond_types)

    @classmethod
    def from_yaml(cls, path, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
        import yaml
        with open(path) as f:
            return cls.from_dict(yaml.safe_load(f) or {}, atomic_numbers, num_bond_types)

    @classmethod
    def default(cls, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
        return cls.from_yaml(DEFAULT_PATTERNS, atomic_numbers, num_bond_types)

    def _build(self, spec, k):
        name = str(spec.get('name', f'pattern{k}'))
        unknown = set(spec) - {'name', 'atoms', 'bonds'}
        if unknown:
            raise ValueError(f'{name}: unknown key(s) {sorted(unknown)}')
        raw_atoms, raw_bonds = list(spec.get('atoms') or []), list(spec.get('bonds') or [])
        if not 1 <= len(raw_atoms) <= PAT_ATOMS:
            raise ValueError(f'{name}: a pattern has 1 .. {PAT_ATOMS} atoms, got {len(raw_atoms)}')
        if len(raw_bonds) > PAT_BONDS:
            raise ValueError(f'{name}: a pattern has at most {PAT_BONDS} bonds, got {len(raw_bonds)}')
        cls_of = {z: c for c, z in enumerate(self.atomic_numbers)}
        atoms = []
        for a, at in enumerate(raw_atoms):
            at = dict(at or {})
            what = f'{name}: atom {a}'
            extra = set(at) - {'elem', 'deg', 'h', 'ring', 'arom'}
            if extra:
                raise ValueError(f'{what}: unknown key(s) {sorted(extra)}')
            elem = at.get('elem', '*')
            if isinstance(elem, str) and elem == '*':
                emask = (1 << len(self.atomic_numbers)) - 1
            else:
                emask = 0
                for z in ([elem] if isinstance(elem, (str, int, np.integer)) else list(elem)):
                    z = SYMBOLS.get(z, z) if isinstance(z, str) else int(z)
                    if z not in cls_of:
                        raise ValueError(f'{what}: element {z!r} is not among the featuriser\'s atomic numbers {self.atomic_numbers}')
                    emask |= 1 << cls_of[z]
                if not emask:
                    raise ValueError(f'{what}: an empty element list matches nothing')
            arom = at.get('arom')
            if arom not in (None, True, False):
                raise ValueError(f'{what}: arom is true, false or absent')
            atoms.append((emask, _bits(at.get('deg', range(8)), range(8), what + ' deg', 7),
                          _bits(at.get('h', range(5)), range(5), what + ' h', 4), _ring_mask(at.get('ring'), what),
                          0 if arom is None else 1 if arom else 2))
        bonds, seen = [], set()
        for b in raw_bonds:
            b = list(b)
            if len(b) not in (3, 4):
                raise ValueError(f'{name}: a bond is [i, j, types] or [i, j, types, ring], got {b!r}')
            i, j = int(b[0]), int(b[1])
            what = f'{name}: bond {i}-{j}'
            if not (0 <= i < len(atoms) and 0 <= j < len(atoms)) or i == j:
                raise ValueError(f'{what}: atom index outside the pattern, or a bond of an atom to itself')
            if (min(i, j), max(i, j)) in seen:
                raise ValueError(f'{what}: two bonds between the same pair of atoms')
            seen.add((min(i, j), max(i, j)))
            types_ = range(1, self.num_bond_types + 1) if isinstance(b[2], str) and b[2] == '*' else b[2]
            bonds.append((i, j, _bits(types_, range(1, self.num_bond_types + 1), what + ' types'),
                          _ring_mask(b[3] if len(b) == 4 else None, what)))
        # reorder: atom 0 stays; then, again and again, the smallest atom with a bond to one already placed
        order, nbrs = [0], {a: set() for a in range(len(atoms))}
        for i, j, _, _ in bonds:
            nbrs[i].add(j), nbrs[j].add(i)
        while len(order) < len(atoms):
            nxt = [a for a in range(len(atoms)) if a not in order and nbrs[a] & set(order)]
            if not nxt:
                raise ValueError(f'{name}: the pattern is not connected')
            order.append(nxt[0])
        new = {a: k for k, a in enumerate(order)}
        return Pattern(name, [atoms[a] for a in order],
                       sorted((min(new[i], new[j]), max(new[i], new[j]), t, r) for i, j, t, r in bonds))

    def __len__(self):
        return len(self.patterns)

    @property
    def needs_rings(self):
        return any(p.needs_rings for p in self.patterns)

    def pack(self):
        """the (P, 90) int32 table of ``mdx_mol_groups``: n_atoms, n_bonds, 8 x (elem_mask, deg_mask, h_mask, rsize_mask, arom),
        12 x (i, j, type_mask, rsize_mask); unused fields 0"""
        tab = np.zeros((len(self.patterns), RECORD), dtype=np.int64)
        for p, pat in zip(tab, self.patterns):
            p[0], p[1] = len(pat.atoms), len(pat.bonds)
            for k, a in enumerate(pat.atoms):
                p[2 + 5 * k:7 + 5 * k] = a
            for k, b in enumerate(pat.bonds):
                p[42 + 4 * k:46 + 4 * k] = b
        return np.ascontiguousarray(tab.astype(np.uint32).view(np.int32))

    def automorphisms(self):
        """|Aut| of every pattern (int32)"""
        return np.asarray([p.automorphisms() for p in self.patterns], dtype=np.int32)

    def valence_table(self, normal_valence=None):
        """``normal_valence`` (dict atomic number -> valence; None = DEFAULT_NORMAL_VALENCE) as one int32 per class"""
        table = DEFAULT_NORMAL_VALENCE if normal_valence is None else {int(z): int(v) for z, v in dict(normal_valence).items()}
        missing = [z for z in self.atomic_numbers if z not in table]
        if missing:
            raise ValueError(f'no normal valence for element(s) {missing}')
        if any(not 0 <= table[z] <= 64 for z in self.atomic_numbers):
            raise ValueError('a normal valence lies in 0 .. 64')
        return np.asarray([table[z] for z in self.atomic_numbers], dtype=np.int32)


def _patterns(patterns, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
    """a PatternSet, a path, a dict or None (= the default set) as a PatternSet"""
    if isinstance(patterns, PatternSet):
        return patterns
    if patterns is None:
        return PatternSet.default(atomic_numbers, num_bond_types)
    if isinstance(patterns, str):
        return PatternSet.from_yaml(patterns, atomic_numbers, num_bond_types)
    return PatternSet.from_dict(patterns, atomic_numbers, num_bond_types)


def _no_ring_data(pset):
    if pset.needs_rings:
        raise ValueError('a pattern carries a ring constraint and there is no ring data')


def _set_keys(out, pset):
    out['aut'], out['names'] = pset.automorphisms(), np.asarray(pset.names, dtype=str)
    return out


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def groups_ref(info, patterns, normal_valence=None, max_steps=DEFAULT_MAX_STEPS, ring_data=None):
    """Plain Python restatement of ``mdx_mol_groups`` for one molecule dict (element = atomic numbers, bond_index (2, 2b) with every
    bond once and then flipped, bond_type (2b)) and a PatternSet -> dict: ``status`` (0 measured, 1 more than 256 atoms or 512 bonds,
    2 the ring data are not measured), ``n_atoms``, and per pattern ``n_embed``, ``n_anchor``, ``steps``, ``pat_status`` (0, or 3
    budget exceeded) as int32 arrays, and per atom ``atom_hit`` (bit p: the atom is an anchor of pattern p).  With a non-zero status
    everything but status and n_atoms is 0.  The ring data come from ``rings.rings_ref`` when a pattern carries a ring constraint
    (or from ``ring_data``, a dict with its status / bond_ring_min / atom_ring_min; False = there are none, which a set with a ring
    constraint refuses); no ring data are read otherwise.  A bond whose
    index lies outside the molecule or with i = j is ignored; a bond type outside 1 .. num_bond_types adds no valence and matches no
    pattern bond; an element outside the set's atomic numbers and two bonds between the same pair of atoms raise ValueError."""
    pset = patterns
    max_steps = check_steps(max_steps)
    nv = pset.valence_table(normal_valence)
    nbt = pset.num_bond_types
    cls, bi, bt = mol_graph(info, pset.atomic_numbers)
    n, nb, P = len(cls), bi.shape[1], len(pset)
    bonds = [(e, int(bi[0, e]), int(bi[1, e])) for e in range(nb) if 0 <= bi[0, e] < n and 0 <= bi[1, e] < n and bi[0, e] != bi[1, e]]
    pairs = [(min(x, y), max(x, y)) for _, x, y in bonds]
    if len(set(pairs)) != len(pairs):
        raise ValueError('two bonds between the same pair of atoms')
    zp = lambda: np.zeros(P, dtype=np.int32)
    out = {'status': STATUS_OK, 'n_atoms': n, 'n_embed': zp(), 'n_anchor': zp(), 'steps': zp(), 'pat_status': zp(),
           'atom_hit': np.zeros(n, dtype=np.int32)}
    if n > MAX_ATOMS or nb > MAX_BONDS:
        return dict(out, status=STATUS_TOO_LARGE)
    arc, brc = [0] * n, [0] * nb
    if ring_data is False:
        _no_ring_data(pset)
    elif pset.needs_rings or ring_data is not None:
        r = ring_data if ring_data is not None else rings.rings_ref(info, nbt, pset.atomic_numbers)
        if int(r['status']) != 0:
            return dict(out, status=STATUS_NO_RINGS)
        arc, brc = [ring_class(v) for v in r['atom_ring_min']], [ring_class(v) for v in r['bond_ring_min']]
    adj, val2, arom = [[] for _ in range(n)], [0] * n, [False] * n
    for e, x, y in bonds:
        t = int(bt[e])
        t = t if 1 <= t <= nbt else 0
        adj[x].append((y, t, brc[e]))
        adj[y].append((x, t, brc[e]))
        w = 0 if t == 0 else 3 if t == nbt else 2 * t        # mdx_mol_check's valence2
        for a in (x, y):
            val2[a] += w
            arom[a] |= t == nbt
    deg = [len(a) for a in adj]
    hyd = [max(0, int(nv[cls[a]]) - (val2[a] + 1) // 2) for a in range(n)]

    def atom_ok(pa, a):
        emask, dmask, hmask, rmask, ar = pa
        return bool(emask >> int(cls[a]) & 1 and dmask >> min(deg[a], 7) & 1 and hmask >> min(hyd[a], 4) & 1 and rmask >> arc[a] & 1
                    and (ar == 0 or ar == (1 if arom[a] else 2)))

    bond_ok = lambda pb, t, rc: bool(t and pb[0] >> t & 1 and pb[1] >> rc & 1)
    hit = np.zeros(n, dtype=np.uint32)
    for p, pat in enumerate(pset.patterns):
        na = len(pat.atoms)
        embed_at, steps_at = [0] * n, [1] * n           # per start atom; the start candidate itself is one step
        try:
            for a in range(n):
                if not atom_ok(pat.atoms[0], a):
                    continue
                img = [a]

                def extend(k):
                    if k == na:
                        embed_at[a] += 1
                        return
                    steps_at[a] += deg[img[pat.parent[k]]]
                    if steps_at[a] > max_steps:
                        raise OverBudget
                    for v, t, rc in adj[img[pat.parent[k]]]:
                        if v in img or not bond_ok(pat.tree[k], t, rc) or not atom_ok(pat.atoms[k], v):
                            continue
                        if all(any(w == img[i] and bond_ok((tm, rm), t2, rc2) for w, t2, rc2 in adj[v]) for i, tm, rm in pat.closures[k]):
                            img.append(v)
                            extend(k + 1)
                            img.pop()
                extend(1)
        except OverBudget:
            out['pat_status'][p] = PAT_OVER_BUDGET
            continue
        out['n_embed'][p], out['steps'][p] = sum(embed_at), sum(steps_at)
        out['n_anchor'][p] = sum(1 for c in embed_at if c)
        hit |= np.asarray([np.uint32(1 << p) if c else np.uint32(0) for c in embed_at], dtype=np.uint32).reshape(n)
    out['atom_hit'] = hit.view(np.int32)
    return out


def stack_ref(mols, patterns=None, normal_valence=None, max_steps=DEFAULT_MAX_STEPS):
    """``groups_ref`` of every molecule of a list as the results dict ``groups_mols`` returns (numpy): one entry or row of P per
    molecule of every key of MOL_KEYS, ``atom_hit`` over the atoms of the list in turn, ``atom_ptr``, and the set's ``aut`` / ``names``"""
    pset = _patterns(patterns)
    refs = [groups_ref(m, pset, normal_valence, max_steps) for m in mols]
    return _set_keys(molpack.stack(refs, LAYOUT, dict.fromkeys(LAYOUT.wide, len(pset))), pset)


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, patterns, normal_valence=None, max_steps=DEFAULT_MAX_STEPS, select=None, ring_data=None):
    """``mdx_mol_groups`` on the device arrays `cm` (a ``CompactMols``) -> dict of int32 device tensors: status (B), n_embed / n_anchor / steps /
    pat_status (B, P) and ``atom_hit`` (N_cap) in the layout of the inputs, zero where no molecule has a slot; no sync.  ring_data: the
    dict ``rings.launch`` returned for the same arrays; when None and a pattern carries a ring constraint, ``rings.launch`` runs first;
    False = none, which a set with a ring constraint refuses."""
    import torch
    from . import _lib
    pset, max_steps = patterns, check_steps(max_steps)
    P, dev = len(pset), cm.device
    out, _ = molpack.zeros_for(cm, LAYOUT, dict.fromkeys(LAYOUT.wide, P))
    if cm.B == 0:
        return out
    if ring_data is False:
        _no_ring_data(pset)
        ring_data = None
    elif ring_data is None and pset.needs_rings:
        ring_data = rings.launch(cm, len(pset.atomic_numbers), pset.num_bond_types, select=select)
    table, nv = pset.pack(), pset.valence_table(normal_valence)
    L = _lib.lib()
    ws = torch.empty(L.mdx_mol_groups_ws_bytes(P), dtype=torch.uint8, device=dev)
    ops, at = cm.operands()
    rd = (lambda k: at(ring_data[k])) if ring_data is not None else (lambda k: None)
    _lib.check(L.mdx_mol_groups(
        *ops, _lib.ptr(select), len(pset.atomic_numbers), pset.num_bond_types, nv.ctypes.data, table.ctypes.data, P, max_steps,
        rd('atom_ring_min'), rd('bond_ring_min'), rd('status'), at(out['n_embed']), at(out['n_anchor']), at(out['steps']),
        at(out['pat_status']), at(out['status']), at(out['atom_hit']), _lib.ptr(ws), ws.numel(), _lib.stream()))
    return out


def groups_mols(mols, device, patterns=None, normal_valence=None, max_steps=DEFAULT_MAX_STEPS):
    """Pattern counts of a list of molecule dicts (finished molecules, or entries of ``samples_all.pt``) on the device: the list is
    packed densely, copied and handed to ``mdx_mol_groups`` (after ``mdx_mol_rings`` when a pattern carries a ring constraint).
    patterns: a PatternSet, a YAML path, a dict, or None for the default set.  -> the results dict of ``stack_ref`` with device tensors
    (``aut`` / ``names`` stay numpy).  Two bonds between the same pair of atoms and unknown elements raise ValueError."""
    pset = _patterns(patterns)
    check_steps(max_steps)
    p, cm = molpack.packed(mols, pset.atomic_numbers, device)
    return _set_keys(molpack.dense(launch(cm, pset, normal_valence, max_steps), cm, p, LAYOUT), pset)


def concat(parts):
    """the results of consecutive batches made with one pattern set (host or device arrays, not mixed) as one results dict"""
    parts = [to_host(p) for p in parts]
    if any(not np.array_equal(p['names'], parts[0]['names']) or not np.array_equal(p['aut'], parts[0]['aut']) for p in parts):
        raise ValueError('the parts were made with different pattern sets')
    return dict(molpack.concat(parts, LAYOUT), aut=parts[0]['aut'], names=parts[0]['names'])


def empty(patterns=None):
    return stack_ref([], patterns)


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def n_match(results):
    """(B, P) int64: n_embed / |Aut|.  Aut acts freely on the embeddings of a pattern, so the division is exact; asserted."""
    r = to_host(results)
    embed, aut = r['n_embed'].astype(np.int64), r['aut'].astype(np.int64)
    assert not (embed % aut[None, :]).any(), 'n_embed is not a multiple of |Aut|'
    return embed // aut[None, :]


def summary(results):
    """The numbers of a results dict (host or device arrays) -> dict: ``n_measured`` (molecules with status 0), ``n_skipped`` by status
    (too_large, no_ring_data), and ``patterns``: per pattern name ``mean_matches`` = the mean n_match and ``fraction_with_match`` =
    the share of molecules with at least one match, both over the molecules in which the pattern was measured (``n_measured`` of
    the pattern = status 0 and within the budget), ``n_over_budget``, and ``counts`` = how many of those molecules have 0, 1, ..., 7
    and 8 or more matches.  NaN where nothing was measured."""
    r = to_host(results)
    ok = r['status'] == STATUS_OK
    nm = n_match(r)
    nan = float('nan')
    pats = {}
    for p, name in enumerate(r['names'].tolist()):
        use = ok & (r['pat_status'][:, p] == 0)
        k, c = int(use.sum()), nm[use, p]
        pats[str(name)] = {'n_measured': k, 'n_over_budget': int((ok & (r['pat_status'][:, p] == PAT_OVER_BUDGET)).sum()),
                           'mean_matches': int(c.sum()) / k if k else nan, 'fraction_with_match': int((c > 0).sum()) / k if k else nan,
                           'counts': np.bincount(np.minimum(c, 8), minlength=9).tolist()}
    return {'n_measured': int(ok.sum()),
            'n_skipped': {'too_large': int((r['status'] == STATUS_TOO_LARGE).sum()),
                          'no_ring_data': int((r['status'] == STATUS_NO_RINGS).sum())},
            'patterns': pats}


def compare(a, b):
    """Jensen-Shannon divergence (``molpack.jsd_counts``: base 2, in [0, 1], NaN when a side is empty) of the per-molecule match count
    distributions (0, 1, ..., 7, 8 or more) of two results dicts or two summaries, per pattern name -> {name: jsd}"""
    a, b = (x if 'patterns' in x else summary(x) for x in (a, b))
    if list(a['patterns']) != list(b['patterns']):
        raise ValueError('the two sides were made with different pattern sets')
    return {k: jsd_counts(a['patterns'][k]['counts'], b['patterns'][k]['counts']) for k in a['patterns']}


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    def run(mols, a, dev):
        pset = _patterns(a.patterns)
        return stack_ref(mols, pset, max_steps=a.max_steps) if dev is None else groups_mols(mols, dev, pset, max_steps=a.max_steps)
    return molpack.stats_main(
        argv, 'groups', __doc__, ('pattern counts of the molecules stored in a samples_all.pt',
                                  'Jensen-Shannon divergence of the per-molecule match counts of two files, per pattern'),
        [('--patterns', dict(default=None, help='pattern file (YAML); default: configs/groups_default.yml')),
         ('--max_steps', dict(type=int, default=DEFAULT_MAX_STEPS))], run, summary, compare)


if __name__ == '__main__':
    sys.exit(main())
