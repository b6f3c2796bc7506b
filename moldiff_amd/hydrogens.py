"""Explicit hydrogens with 3D coordinates for decoded molecules: the hydrogens a Kekulé assignment counts are placed from the local
geometry of the heavy atoms, and the all-atom contacts of what was placed are measured.

The device half is ``mdx_mol_hydrogens`` (csrc/mdx_hydrogens.hip), reached through ``addh_mols`` (a list of molecule dicts; runs
``kekule`` first when no counts are given), ``launch`` (a ``CompactMols`` with positions and the device arrays ``n_h`` / ``order``) and
``FeaturizeMol.addh_batch`` (the sampler's predictions).  ``addh_ref`` is the plain restatement for one molecule and needs no GPU; the
GPU tests compare the integers exactly and the floats to 1e-8 Angstrom.

What it is: THIS PROJECT'S OWN IDEALISED PLACEMENT, stated exactly in include/moldiff_hip.h.  It is NOT RDKit's
``AddHs(addCoords=True)`` and it is UNVERIFIED AGAINST RDKit.  Torsions of rotors (methyl, hydroxyl, amine) are fixed by rule (the first
hydrogen anti to the lowest-index neighbour of the neighbour), not by an energy.  A pyramidal nitrogen takes the side set by the order of
its neighbours.  Lone atoms and two-atom molecules use fixed world axes (flag WORLD_FRAME), so their hydrogens are not
rotation-equivariant.  The X-H lengths (C 1.09, N 1.01, O 0.96, F 0.92, P 1.42, S 1.34, Cl 1.27 Angstrom: textbook values) and
``clash_tol`` (1.5 Angstrom) are conventions, untuned.  With no trained checkpoint offline it is an instrument, not a measurement of
sample quality.

The definition in short.  With ``order`` the Kekulé bond orders (0 counts as 1) and h = ``n_h`` clamped to 0 .. 4: an atom is LINEAR
(room 2) with a triple bond or two double bonds, else TRIGONAL (room 3) with a double or an aromatic bond, or when its class is in
``planar`` and a neighbour is trigonal or linear by those rules, else TETRAHEDRAL (room 4).  d neighbours + h hydrogens above the room:
NO_ROOM.  The directions come from the unit vectors to the neighbours in ascending index (the table in the header: d = 0 world
directions; d = 1 a frame from the neighbour's lowest-index other neighbour; d = 2 the bisector and the normal; d = 3 the negative
sum); a failing condition (``deg_tol``) or coinciding atoms make the atom DEGENERATE.  A contact is a pair (placed H, other atom or
placed H) without the H's parent, the parent's neighbours and the parent's other hydrogens.

    python -m moldiff_amd.hydrogens stats samples_all.pt --out hydrogens.npz [--sdf allatom.sdf] [--ref] [--clash_tol 1.5] [--part finished]
    python -m moldiff_amd.hydrogens compare a.npz b.npz
"""
import math
import sys

import numpy as np

from . import kekule, molpack
from .molpack import DEFAULT_ATOMIC_NUMBERS, host, jsd_counts, mol_graph, to_host

MAX_ATOMS, MAX_BONDS = kekule.MAX_ATOMS, kekule.MAX_BONDS          # include/moldiff_hip.h: the caps of mdx_mol_rings
MAX_ELEMENTS, MAX_BOND_TYPES, MAX_H, MAX_LENGTH = 32, 16, 4, 4.0
DEFAULT_DEG_TOL = 1e-3
DEFAULT_CLASH_TOL = 1.5                                            # Angstrom: a convention, untuned
# this project's choice of textbook values, unverified against RDKit
DEFAULT_XH_LENGTH = {6: 1.09, 7: 1.01, 8: 0.96, 9: 0.92, 15: 1.42, 16: 1.34, 17: 1.27}
DEFAULT_PLANAR = (7,)                                              # flattens next to a pi system
STATUS_OK, STATUS_TOO_LARGE = 0, 1
GEOM_TETRAHEDRAL, GEOM_TRIGONAL, GEOM_LINEAR = 0, 1, 2             # bits 0-1 of atom_flag
FLAG_NO_ROOM, FLAG_DEGENERATE, FLAG_WORLD_FRAME, FLAG_CLAMPED = 4, 8, 16, 32
# the columns of the device's per-molecule table, in its order (include/moldiff_hip.h: MDX_HYDROGENS_STATS)
STAT_KEYS = ('status', 'n_h_wanted', 'n_h_placed', 'n_no_room', 'n_degenerate', 'n_world_frame', 'n_clash')
MOL_KEYS = STAT_KEYS + ('n_atoms',)
ATOM_KEYS = ('h_count', 'atom_flag')
LAYOUT = molpack.Layout(MOL_KEYS, atom=ATOM_KEYS)                  # the int32 part of the results table
FLOAT_KEYS = ('h_pos', 'min_contact')                              # float64: (atoms, 4, 3) and one per molecule
CONTACT_BINS, CONTACT_MAX = 40, 4.0                                # the histogram of min_contact: 0.1 Angstrom bins, the last also more
# the constants of the definition, the same literals as csrc/mdx_hydrogens.hip
COS_TET, SIN_TET = -0.3333333333333333, 0.9428090415820635         # theta = acos(-1/3)
COS_TRI, SIN_TRI = -0.5, 0.8660254037844386                        # 120 degrees
COS_HALF, SIN_HALF = 0.5773502691896257, 0.816496580927726         # beta = theta / 2
INV_SQRT3 = 0.5773502691896258
_C = INV_SQRT3
WORLD_DIRS = {GEOM_TETRAHEDRAL: ((_C, _C, _C), (_C, -_C, -_C), (-_C, _C, -_C), (-_C, -_C, _C)),
              GEOM_TRIGONAL: ((1.0, 0.0, 0.0), (COS_TRI, SIN_TRI, 0.0), (COS_TRI, -SIN_TRI, 0.0)),
              GEOM_LINEAR: ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0))}
# (cos theta, sin theta) and the (cos phi, sin phi) of the hydrogens of an atom with one neighbour
POLAR = {GEOM_TETRAHEDRAL: (COS_TET, SIN_TET), GEOM_TRIGONAL: (COS_TRI, SIN_TRI)}
AZIMUTH = {GEOM_TETRAHEDRAL: ((-1.0, 0.0), (0.5, -SIN_TRI), (0.5, SIN_TRI)), GEOM_TRIGONAL: ((-1.0, 0.0), (1.0, 0.0))}


class HydrogenTables:
    """The conventions of one call, indexed by atom class: ``xh_length`` (float64, Angstrom) and ``planar``, a bit mask over classes.
    Built from a dict keyed by atomic number and a tuple of atomic numbers (None = the defaults above) and validated as the device
    entry validates them."""

    def __init__(self, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4, xh_length=None, planar=None):
        self.atomic_numbers, self.num_bond_types = tuple(int(z) for z in atomic_numbers), int(num_bond_types)
        if not 1 <= len(self.atomic_numbers) <= MAX_ELEMENTS or not 1 <= self.num_bond_types <= MAX_BOND_TYPES:
            raise ValueError(f'1 .. {MAX_ELEMENTS} elements and 1 .. {MAX_BOND_TYPES} bond types')
        xl = DEFAULT_XH_LENGTH if xh_length is None else {int(z): float(v) for z, v in dict(xh_length).items()}
        pl = DEFAULT_PLANAR if planar is None else tuple(int(z) for z in planar)
        missing = [z for z in self.atomic_numbers if z not in xl]
        if missing:
            raise ValueError(f'no X-H length for element(s) {missing}')
        if xh_length is not None or planar is not None:
            unknown = sorted((set(xl) | set(pl)) - set(self.atomic_numbers))
            if unknown:
                raise ValueError(f'xh_length / planar name element(s) {unknown} outside the atomic numbers {self.atomic_numbers}')
        self.xh_length = np.asarray([xl[z] for z in self.atomic_numbers], dtype=np.float64)
        if not all(0.0 < float(v) <= MAX_LENGTH for v in self.xh_length):   # NaN fails
            raise ValueError(f'an X-H length lies in (0, {MAX_LENGTH}] Angstrom')
        self.planar = sum(1 << c for c, z in enumerate(self.atomic_numbers) if z in pl)

    def key(self):
        return (self.atomic_numbers, self.num_bond_types, tuple(self.xh_length.tolist()), self.planar)


def _tables(tables):
    return HydrogenTables() if tables is None else tables


def _check(deg_tol, clash_tol):
    if not 0.0 < float(deg_tol) < 1.0:                             # NaN fails
        raise ValueError(f'deg_tol must lie in (0, 1), got {deg_tol}')
    if not 0.0 <= float(clash_tol) <= 1.0e3:
        raise ValueError(f'clash_tol must lie in [0, 1000] Angstrom, got {clash_tol}')
    return float(deg_tol), float(clash_tol)


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _norm(a):
    return math.sqrt(_dot(a, a))


def _comb(p, a, q, b):
    return (p * a[0] + q * b[0], p * a[1] + q * b[1], p * a[2] + q * b[2])


def _neg_over(a, l):
    return (-a[0] / l, -a[1] / l, -a[2] / l)


def _unit(d):
    dd = _dot(d, d)
    if not dd > 0.0:
        return None
    l = math.sqrt(dd)
    return (d[0] / l, d[1] / l, d[2] / l)


def _finite(p):
    return all(math.isfinite(x) for x in p)


def _positions(info, n):
    """float32 positions widened to Python floats, as the device sees them; float64 positions as they are (host only)"""
    pos = np.asarray(info['atom_pos'])
    pos = pos.astype(np.float64) if pos.dtype == np.float64 else pos.astype(np.float32).astype(np.float64)
    return [tuple(float(x) for x in row) for row in pos.reshape(n, 3)]


def _place(a, geom, nbrs, h, L, pos, fin, adj, deg_tol, trace):
    """the directions of the definition for atom `a` -> (the h positions or None when degenerate, world frame or not); every value
    compared with deg_tol goes into `trace`"""
    if not fin[a]:
        return None, False
    p, d, world = pos[a], len(nbrs), False
    us = []
    for b in nbrs:
        u = _unit(_sub(pos[b], p)) if fin[b] else None
        if u is None:
            return None, False
        us.append(u)
    if d == 0:
        world, dirs = True, list(WORLD_DIRS[geom])
    elif d == 1:
        e, n1 = us[0], nbrs[0]
        if geom == GEOM_LINEAR:
            dirs = [(-e[0], -e[1], -e[2])]
        else:
            w = None
            for r in adj[n1]:                                      # ascending
                if r == a or not fin[r]:
                    continue
                wv = _unit(_sub(pos[r], pos[n1]))
                if wv is None:
                    continue
                sine = _norm(_cross(e, wv))
                trace.append(('deg', sine))
                if sine >= deg_tol:
                    w = wv
                    break
            if w is None:
                ax, ay, az = abs(e[0]), abs(e[1]), abs(e[2])
                w = (1.0, 0.0, 0.0) if ax <= ay and ax <= az else (0.0, 1.0, 0.0) if ay <= az else (0.0, 0.0, 1.0)
                lo = sorted((ax, ay, az))
                trace.append(('axis', lo[1] - lo[0]))
                world = True
            t = _dot(w, e)
            f1 = _unit((w[0] - t * e[0], w[1] - t * e[1], w[2] - t * e[2]))
            if f1 is None:
                return None, False
            f2 = _cross(e, f1)
            ct, st = POLAR[geom]
            dirs = [_comb(ct, e, st, _comb(cp, f1, sp, f2)) for cp, sp in AZIMUTH[geom]]
    elif d == 2:
        sv = _add(us[0], us[1])
        ns = _norm(sv)
        if geom == GEOM_TRIGONAL:
            trace.append(('deg', ns))
            if not ns >= deg_tol:
                return None, False
            dirs = [_neg_over(sv, ns)]
        else:
            c = _cross(us[0], us[1])
            nc = _norm(c)
            trace.append(('deg', nc))
            if not nc >= deg_tol or not ns > 0.0:
                return None, False
            b, nh = _neg_over(sv, ns), (c[0] / nc, c[1] / nc, c[2] / nc)
            dirs = [_comb(COS_HALF, b, SIN_HALF, nh), _comb(COS_HALF, b, -SIN_HALF, nh)]
    else:
        sv = _add(_add(us[0], us[1]), us[2])
        ns = _norm(sv)
        trace.append(('deg', ns))
        if not ns >= deg_tol:
            return None, False
        dirs = [_neg_over(sv, ns)]
    return [(p[0] + L * q[0], p[1] + L * q[1], p[2] + L * q[2]) for q in dirs[:h]], world


def addh_ref(info, n_h, order, tables=None, deg_tol=DEFAULT_DEG_TOL, clash_tol=DEFAULT_CLASH_TOL, trace=None):
    """Plain Python-float restatement of ``mdx_mol_hydrogens`` for one molecule dict with ``atom_pos`` (float32 as the device gets it,
    or float64 for host-only use), the hydrogen count `n_h` per atom and the bond `order` per bond (each bond once: normally ``kek_h``
    and ``kek_order`` of ``kekule.kekulize_ref``) -> dict: the per-molecule numbers of STAT_KEYS, ``n_atoms``, ``min_contact`` (float),
    per atom ``h_count`` and ``atom_flag`` (int32) and ``h_pos`` (n, 4, 3) float64, zero where no hydrogen stands.  With status 1 (more
    than 256 atoms or 512 bonds) every other output is 0.  trace: a list that receives every number a decision compares with a
    threshold: ('deg', value), ('axis', gap between the two smallest |e . axis|), ('contact', length)."""
    tb = _tables(tables)
    deg_tol, clash_tol = _check(deg_tol, clash_tol)
    trace = [] if trace is None else trace
    nbt = tb.num_bond_types
    cls, bi, bt = mol_graph(info, tb.atomic_numbers)
    n, nb = len(cls), bi.shape[1]
    n_h = np.asarray(n_h, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    if len(n_h) != n or len(order) != nb:
        raise ValueError('n_h holds one count per atom and order one value per bond')
    out = dict({k: 0 for k in STAT_KEYS}, n_atoms=n, min_contact=0.0, h_count=np.zeros(n, dtype=np.int32), atom_flag=np.zeros(n, dtype=np.int32),
               h_pos=np.zeros((n, MAX_H, 3), dtype=np.float64))
    if n > MAX_ATOMS or nb > MAX_BONDS:
        return dict(out, status=STATUS_TOO_LARGE)
    pos = _positions(info, n)
    fin = [_finite(p) for p in pos]
    rows = [[] for _ in range(n)]                                      # (neighbour, order, aromatic)
    for e in range(nb):
        i, j = int(bi[0, e]), int(bi[1, e])
        if not (0 <= i < n and 0 <= j < n and i != j):
            continue
        o, arom = min(max(int(order[e]), 1), 3), int(bt[e]) == nbt
        rows[i].append((j, o, arom)), rows[j].append((i, o, arom))
    rows = [sorted(r) for r in rows]
    adj = [[u for u, _, _ in r] for r in rows]

    def first_rule(r):
        n2, n3 = sum(o == 2 for _, o, _ in r), sum(o == 3 for _, o, _ in r)
        return GEOM_LINEAR if n3 >= 1 or n2 >= 2 else GEOM_TRIGONAL if n2 >= 1 or any(ar for _, _, ar in r) else GEOM_TETRAHEDRAL
    g1 = [first_rule(r) for r in rows]
    placed = []                                                        # (atom, k, position)
    for a in range(n):
        c = int(cls[a])
        raw = int(n_h[a])
        h = min(max(raw, 0), MAX_H)
        geom = g1[a]
        if geom == GEOM_TETRAHEDRAL and (tb.planar >> c) & 1 and any(g1[u] != GEOM_TETRAHEDRAL for u in adj[a]):
            geom = GEOM_TRIGONAL
        flag = geom | (FLAG_CLAMPED if h != raw else 0)
        out['n_h_wanted'] += h
        if h >= 1:
            if len(adj[a]) + h > 4 - geom:
                flag |= FLAG_NO_ROOM
            else:
                where, world = _place(a, geom, adj[a], h, float(tb.xh_length[c]), pos, fin, adj, deg_tol, trace)
                if where is None:
                    flag |= FLAG_DEGENERATE
                else:
                    flag |= FLAG_WORLD_FRAME if world else 0
                    out['h_count'][a] = h
                    for k, q in enumerate(where):
                        out['h_pos'][a, k] = q
                        placed.append((a, k, q))
        out['atom_flag'][a] = flag
    shortest, clash = math.inf, 0
    for x, (a, _, q) in enumerate(placed):
        others = [pos[b] for b in range(n) if fin[b] and b != a and b not in adj[a]] + [q2 for a2, _, q2 in placed[x + 1:] if a2 != a]
        for o in others:
            dist = _norm(_sub(o, q))
            trace.append(('contact', dist))
            shortest = min(shortest, dist)
            clash += dist < clash_tol
    flags = out['atom_flag']
    out.update(n_h_placed=int(out['h_count'].sum()), n_no_room=int(((flags & FLAG_NO_ROOM) != 0).sum()),
               n_degenerate=int(((flags & FLAG_DEGENERATE) != 0).sum()), n_world_frame=int(((flags & FLAG_WORLD_FRAME) != 0).sum()),
               n_clash=clash, min_contact=shortest)
    return out


def near_threshold(info, n_h, order, tables=None, deg_tol=DEFAULT_DEG_TOL, clash_tol=DEFAULT_CLASH_TOL, band=1e-6):
    """whether some decision of ``addh_ref`` lies within `band` of its threshold: a value compared with ``deg_tol``, a contact at
    ``clash_tol``, or the choice between two world axes that are almost equally good (an exact tie is no decision: the first wins on
    both sides).  The molecules a device comparison may leave out, because float64 rounding may differ."""
    trace = []
    addh_ref(info, n_h, order, tables, deg_tol, clash_tol, trace)
    return any((kind == 'deg' and abs(v - deg_tol) <= band) or (kind == 'contact' and abs(v - clash_tol) <= band) or
               (kind == 'axis' and 0.0 < v <= band) for kind, v in trace)


def _counts(mols, tables, n_h, order):
    """per molecule (n_h, order): the caller's, or those of ``kekule.kekulize_ref`` with the default chemistry of the same featuriser"""
    if (n_h is None) != (order is None):
        raise ValueError('give both n_h and order, or neither')
    if n_h is not None:
        if len(n_h) != len(mols) or len(order) != len(mols):
            raise ValueError('one n_h array and one order array per molecule')
        return list(zip(n_h, order))
    kt = kekule.KekuleTables(tables.atomic_numbers, tables.num_bond_types)
    return [(r['kek_h'], r['kek_order']) for r in (kekule.kekulize_ref(m, kt) for m in mols)]


def _stack(refs):
    out = molpack.stack(refs, LAYOUT)
    out['h_pos'] = np.concatenate([r['h_pos'] for r in refs] + [np.zeros((0, MAX_H, 3))]).astype(np.float64)
    out['min_contact'] = np.asarray([r['min_contact'] for r in refs], dtype=np.float64)
    return out


def stack_ref(mols, n_h=None, order=None, tables=None, deg_tol=DEFAULT_DEG_TOL, clash_tol=DEFAULT_CLASH_TOL):
    """``addh_ref`` of every molecule of a list as the results dict ``addh_mols`` returns (numpy): one entry per molecule of every key
    of MOL_KEYS (int32) and ``min_contact`` (float64), ``h_count`` / ``atom_flag`` (int32) and ``h_pos`` (atoms, 4, 3; float64) over the
    atoms of the list in turn, ``atom_ptr``.  n_h, order: one array per molecule, or None for those of ``kekule.kekulize_ref``."""
    tb = _tables(tables)
    return _stack([addh_ref(m, h, o, tb, deg_tol, clash_tol) for m, (h, o) in zip(mols, _counts(mols, tb, n_h, order))])


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, n_h, order, tables=None, deg_tol=DEFAULT_DEG_TOL, clash_tol=DEFAULT_CLASH_TOL, select=None):
    """``mdx_mol_hydrogens`` on the device arrays `cm` (a ``CompactMols`` with positions), `n_h` (int32, N_cap) and `order` (int32,
    Eh_stride) in the layout of `cm` -- ``kek_h`` and ``kek_order`` of ``kekule.launch`` on the same arrays -> dict of device tensors:
    the keys of STAT_KEYS (B) each (int32, columns of one (B, 7) table), ``min_contact`` (B, float64), ``h_count`` / ``atom_flag``
    (N_cap, int32) and ``h_pos`` (N_cap, 4, 3; float64) in the layout of the inputs, zero where no molecule has a slot.  No sync."""
    import torch
    from . import _lib
    tb = _tables(tables)
    deg_tol, clash_tol = _check(deg_tol, clash_tol)
    out, stats = molpack.zeros_for(cm, LAYOUT, stat_keys=STAT_KEYS)
    out['h_pos'] = torch.zeros(max(cm.N_cap, 1), MAX_H, 3, dtype=torch.float64, device=cm.device)
    out['min_contact'] = torch.zeros(cm.B, dtype=torch.float64, device=cm.device)
    if cm.B > 0:
        if cm.atom_pos is None:
            raise ValueError('placing hydrogens needs positions: a CompactMols with atom_pos')
        if n_h.dtype != torch.int32 or order.dtype != torch.int32 or n_h.numel() < cm.N_cap or order.numel() < cm.Eh_stride:
            raise ValueError('n_h and order are int32 tensors in the layout of atom_type and bond_type')
        n_h, order = n_h.contiguous(), order.contiguous()
        ops, at = cm.operands()
        _lib.check(_lib.lib().mdx_mol_hydrogens(
            *ops, _lib.ptr(select), at(cm.atom_pos), at(n_h), at(order), len(tb.atomic_numbers), tb.num_bond_types, tb.xh_length.ctypes.data,
            tb.planar, deg_tol, clash_tol, at(out['h_pos']), at(out['h_count']), at(out['atom_flag']), at(stats), at(out['min_contact']),
            _lib.stream()))
    return molpack.split_stats(out, stats, STAT_KEYS)


def addh_mols(mols, device, n_h=None, order=None, tables=None, deg_tol=DEFAULT_DEG_TOL, clash_tol=DEFAULT_CLASH_TOL, with_kekule=False):
    """Hydrogens for a list of molecule dicts with ``atom_pos`` (finished molecules, or entries of ``samples_all.pt``) on the device:
    the list is packed densely, copied and handed to ``mdx_mol_kekulize`` (unless `n_h` and `order` are given: one array per
    molecule) and then to ``mdx_mol_hydrogens``.  -> the results dict of ``stack_ref`` with device tensors; with `with_kekule` -> (the
    results of ``kekule.kekulize_mols``, that).  Two bonds between the same pair of atoms, a molecule without positions and unknown
    elements raise ValueError."""
    import torch
    tb = _tables(tables)
    _check(deg_tol, clash_tol)
    if any('atom_pos' not in m for m in mols):
        raise ValueError('placing hydrogens needs atom_pos in every molecule')
    if (n_h is None) != (order is None):
        raise ValueError('give both n_h and order, or neither')
    if with_kekule and n_h is not None:
        raise ValueError('with_kekule returns the Kekulé assignment made here: give no n_h / order')
    p, cm = molpack.packed(mols, tb.atomic_numbers, device, positions=True)
    kek = None
    if n_h is None:
        kek = kekule.launch(cm, kekule.KekuleTables(tb.atomic_numbers, tb.num_bond_types))
        h_dev, o_dev = kek['kek_h'], kek['kek_order']
    else:
        if len(n_h) != len(mols) or len(order) != len(mols):
            raise ValueError('one n_h array and one order array per molecule')
        flat = lambda xs, counts, size: np.concatenate(
            [np.asarray(x, dtype=np.int32).reshape(int(c)) for x, c in zip(xs, counts)] + [np.zeros(0, dtype=np.int32)])
        h_host, o_host = flat(n_h, p['n_atoms'], 0), flat(order, p['n_bonds'], 0)
        o_full = np.zeros(max(cm.Eh_stride, 1), dtype=np.int32)
        o_full[:len(o_host)] = o_host
        h_full = np.zeros(max(cm.N_cap, 1), dtype=np.int32)
        h_full[:len(h_host)] = h_host
        h_dev, o_dev = torch.from_numpy(h_full).to(cm.device), torch.from_numpy(o_full).to(cm.device)
    out = launch(cm, h_dev, o_dev, tb, deg_tol, clash_tol)
    res = _dense(out, cm, p)
    return (molpack.dense(kek, cm, p, kekule.LAYOUT), res) if with_kekule else res


def _dense(out, cm, p):
    h_pos = out.pop('h_pos')[:cm.N_cap]
    min_contact = out.pop('min_contact')
    out = molpack.dense(out, cm, p, LAYOUT)
    out['h_pos'], out['min_contact'] = h_pos, min_contact
    return out


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict"""
    parts = [to_host(p) for p in parts]
    out = molpack.concat(parts, LAYOUT)
    out['h_pos'] = np.concatenate([p['h_pos'].reshape(-1, MAX_H, 3) for p in parts])
    out['min_contact'] = np.concatenate([p['min_contact'] for p in parts])
    return out


def empty():
    return stack_ref([])


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def mol_result(results, m):
    """molecule `m` of a results dict with host arrays as the dict ``addh_ref`` returns"""
    out = molpack.mol_slice(results, m, LAYOUT)
    lo = int(results['atom_ptr'][m])
    out['h_pos'] = np.asarray(results['h_pos'][lo:lo + out['n_atoms']]).reshape(-1, MAX_H, 3)
    out['min_contact'] = float(results['min_contact'][m])
    return out


def fully_hydrogenated(results):
    """bool per molecule: measured, and every hydrogen that was wanted is placed"""
    status, wanted, placed = (host(results[k]) for k in ('status', 'n_h_wanted', 'n_h_placed'))
    return (status == STATUS_OK) & (wanted == placed)


def summary(results, clash_tol=DEFAULT_CLASH_TOL):
    """The numbers of a results dict (host or device arrays) -> dict: ``n_molecules``, ``n_measured`` (status 0), ``n_too_large``; over
    the measured molecules ``fraction_fully_hydrogenated`` (every wanted hydrogen placed), ``mean_hydrogens`` (placed),
    ``mean_hydrogens_wanted``, ``fraction_no_room`` / ``fraction_degenerate`` / ``fraction_world_frame`` (atoms with the flag, of all
    their atoms), ``fraction_with_clash`` (at least one contact below clash_tol), ``n_with_contact`` (a finite min_contact),
    ``min_contact_mean`` / ``min_contact_median`` over those, and ``min_contact_hist`` (40 bins of 0.1 Angstrom from 0, the last also
    everything longer).  NaN where nothing was counted.  `clash_tol` is only recorded: the counts were made by the call that produced
    the results.  This project's idealised placement with conventional lengths and an untuned clash_tol, unverified against RDKit."""
    r = to_host(results)
    n = len(r['status'])
    ok = r['status'] == STATUS_OK
    k = int(ok.sum())
    atoms = int(r['n_atoms'][ok].astype(np.int64).sum())
    nan = float('nan')
    mean = lambda key: int(r[key][ok].astype(np.int64).sum()) / k if k else nan
    share = lambda key: int(r[key][ok].astype(np.int64).sum()) / atoms if atoms else nan
    mc = r['min_contact'][ok]
    mc = mc[np.isfinite(mc)]
    bins = np.minimum((mc / (CONTACT_MAX / CONTACT_BINS)).astype(np.int64), CONTACT_BINS - 1)
    return {'n_molecules': n, 'n_measured': k, 'n_too_large': int((r['status'] == STATUS_TOO_LARGE).sum()),
            'fraction_fully_hydrogenated': int(fully_hydrogenated(r).sum()) / k if k else nan,
            'mean_hydrogens': mean('n_h_placed'), 'mean_hydrogens_wanted': mean('n_h_wanted'),
            'fraction_no_room': share('n_no_room'), 'fraction_degenerate': share('n_degenerate'), 'fraction_world_frame': share('n_world_frame'),
            'fraction_with_clash': int((r['n_clash'][ok] > 0).sum()) / k if k else nan,
            'n_with_contact': int(len(mc)), 'min_contact_mean': float(mc.mean()) if len(mc) else nan,
            'min_contact_median': float(np.median(mc)) if len(mc) else nan,
            'min_contact_hist': np.bincount(bins, minlength=CONTACT_BINS).tolist(), 'clash_tol': float(clash_tol)}


def compare(a, b):
    """two results dicts or two summaries -> dict: Jensen-Shannon divergence (``molpack.jsd_counts``: base 2, in [0, 1], NaN when a
    side is empty) of ``min_contact_hist``, and both sides' ``fraction_fully_hydrogenated`` and ``fraction_with_clash``"""
    a, b = (x if 'min_contact_hist' in x else summary(x) for x in (a, b))
    return {'min_contact': jsd_counts(a['min_contact_hist'], b['min_contact_hist']),
            'fraction_fully_hydrogenated': [a['fraction_fully_hydrogenated'], b['fraction_fully_hydrogenated']],
            'fraction_with_clash': [a['fraction_with_clash'], b['fraction_with_clash']]}


def allatom_mol_block(info, kek_result, h_result, name='moldiff_amd'):
    """All-atom V2000 mol block of a kekulizable molecule: the heavy atoms in their order, then the placed hydrogens in (atom, k)
    order, the bonds with the Kekulé orders, one single bond from every hydrogen to its parent, and the charges as ``M  CHG`` lines.
    Hydrogens that were not placed (NO_ROOM, DEGENERATE) are simply absent.  A molecule that is not kekulizable, holds an ignored
    bond, or has more than 999 atoms or bonds in all raises ValueError."""
    heavy = kekule.kekule_mol_block(info, kek_result, name).splitlines()
    n, nb = len(np.asarray(info['element'])), np.asarray(info['bond_index']).shape[1] // 2
    count, h_pos = np.asarray(h_result['h_count']), np.asarray(h_result['h_pos']).reshape(-1, MAX_H, 3)
    hs = [(a, h_pos[a, k]) for a in range(n) for k in range(int(count[a]))]
    if n + len(hs) > 999 or nb + len(hs) > 999:
        raise ValueError('a V2000 block holds at most 999 atoms and 999 bonds')
    lines = heavy[:3] + ['%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (n + len(hs), nb + len(hs))] + heavy[4:4 + n]
    lines += ['%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0' % (q[0], q[1], q[2], 'H') for _, q in hs]
    lines += heavy[4 + n:4 + n + nb]
    lines += ['%3d%3d%3d  0' % (a + 1, n + 1 + x, 1) for x, (a, _) in enumerate(hs)]
    return '\n'.join(lines + heavy[4 + n + nb:]) + '\n'


def write_sdf(path, mols, kek_results, h_results):
    """the kekulizable molecules of `mols` as all-atom mol blocks (kek_results, h_results: host or device arrays, one entry per
    molecule) -> how many were written.  A molecule with unplaced hydrogens is still written; one that is not kekulizable, holds an
    ignored bond or does not fit a V2000 block is left out, as ``kekule.write_sdf`` leaves it out."""
    kr, hr, written = to_host(kek_results), to_host(h_results), 0
    keep = kekule.kekulizable(kr)
    with open(path, 'w') as f:
        for m, info in enumerate(mols):
            kres = kekule.mol_result(kr, m)
            if not keep[m] or not (kres['kek_order'] >= 1).all():
                continue
            try:
                block = allatom_mol_block(info, kres, mol_result(hr, m))
            except ValueError:
                continue
            f.write(block + '$$$$\n')
            written += 1
    return written


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    held = {}

    def run(mols, args, device):
        _check(DEFAULT_DEG_TOL, args.clash_tol)
        if device is None:
            kek = kekule.stack_ref(mols)
            n = len(mols)
            res = stack_ref(mols, [kekule.mol_result(kek, m)['kek_h'] for m in range(n)], [kekule.mol_result(kek, m)['kek_order'] for m in range(n)],
                            clash_tol=args.clash_tol)
        else:
            kek, res = addh_mols(mols, device, clash_tol=args.clash_tol, with_kekule=True)
        if args.sdf:
            write_sdf(args.sdf, mols, kek, res)
        held['clash_tol'] = args.clash_tol
        return res
    return molpack.stats_main(
        argv, 'hydrogens', __doc__, ('explicit hydrogens and their contacts for the molecules stored in a samples_all.pt',
                                     'Jensen-Shannon divergence of the shortest-contact distributions of two files'),
        [('--sdf', dict(default=None, help='also write the kekulizable molecules as all-atom mol blocks')),
         ('--clash_tol', dict(type=float, default=DEFAULT_CLASH_TOL, help='a contact below this many Angstrom is a clash (1.5: a convention, untuned)'))],
        run, lambda res: summary(res, held.get('clash_tol', DEFAULT_CLASH_TOL)), compare)


if __name__ == '__main__':
    sys.exit(main())
