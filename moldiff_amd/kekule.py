"""Kekulé assignment of the aromatic bonds of decoded molecules: which aromatic bonds become double bonds, which atoms take a charge or
a hydrogen, and whether the aromatic system has a Kekulé structure at all.

The device half is ``mdx_mol_kekulize`` (csrc/mdx_kekule.hip), reached through ``kekulize_mols`` (a list of molecule dicts),
``launch`` (a ``CompactMols``) and ``FeaturizeMol.kekulize_batch`` (the sampler's predictions).  ``kekulize_ref`` is the plain Python
restatement for one molecule and needs no GPU; the GPU tests compare every output exactly.

What it is: the reference hands its decoded bond graph to RDKit's sanitisation (utils/reconstruct.py:245-271) and counts a molecule as
generated only if that succeeds; "Can't kekulize mol" is one of the two ways it fails, and ``fix_valence`` / ``fix_aromatic``
(:295-387) retry with a hydrogen or a positive charge on ring N and S.  RDKit is not available here, so this is THIS PROJECT'S OWN
MODEL of that step, stated exactly in include/moldiff_hip.h, and UNVERIFIED AGAINST RDKit: the default tables below (normal valences
C 4, N 3, O 2, F 1, P 3, S 2, Cl 1; charged valences N+ 4, S+ 3; nitrogen may take a hydrogen instead of a double bond) are this
project's choice, and the structure reported is the FIRST ONE FOUND in a fixed search order, not a charge-minimal one.

The rule, per molecule: sigma of an atom = the sum of the orders of its valid non-aromatic bonds + the number of its aromatic bonds
(the last bond type); adeg = the number of its aromatic bonds.  An atom with adeg >= 1 has a role: NOT (adeg > 3, or no room for a
double bond), MUST (V - sigma >= 1 and the class is not flexible), MAY (V - sigma >= 1 and flexible: it takes a hydrogen instead; or
V - sigma < 1 and Vc - sigma >= 1: it takes a charge if matched).  Within every connected component of the aromatic bonds a Kekulé
structure is a matching on aromatic bonds between atoms that are not NOT which covers every MUST atom.  The canonical one is the first
found by a depth-first search over the component's atoms in ascending index: an atom that is NOT or already matched is skipped; the
others try "stay unmatched" (MAY only), then every aromatic neighbour of higher index that is not NOT and not yet matched, ascending.
``steps`` counts the options tried; a component that would need more than ``max_steps`` is over budget.

    python -m moldiff_amd.kekule stats samples_all.pt --out kekule.npz [--sdf kekule.sdf] [--ref] [--part finished]
    python -m moldiff_amd.kekule compare a.npz b.npz
"""
import argparse
import json
import sys

import numpy as np

from . import molpack, rings
from .molpack import check_steps, DEFAULT_ATOMIC_NUMBERS, DEFAULT_NORMAL_VALENCE, host, jsd_counts, load_mols, load_npz, mol_graph, OverBudget, save_npz, to_host

MAX_ATOMS, MAX_BONDS = rings.MAX_ATOMS, rings.MAX_BONDS           # include/moldiff_hip.h: the caps of mdx_mol_rings
MAX_COMPONENT = 64                                                # atoms of one aromatic component
MAX_STEPS_LIMIT, DEFAULT_MAX_STEPS = molpack.MAX_STEPS_LIMIT, 1 << 16
MAX_ELEMENTS, MAX_BOND_TYPES, MAX_VALENCE = 32, 16, 64
STATUS_OK, STATUS_TOO_LARGE = 0, 1
ROLE_NONE, ROLE_NOT, ROLE_MUST, ROLE_MAY = 0, 1, 2, 3             # bits 0-1 of atom_flag; NONE: the atom has no aromatic bond
FLAG_MATCHED, FLAG_OVERVALENT, FLAG_UNSOLVED = 4, 8, 16
# the columns of the device's per-molecule table, in its order (include/moldiff_hip.h: MDX_KEKULE_STATS)
STAT_KEYS = ('status', 'n_arom_atoms', 'n_arom_bonds', 'n_components', 'n_failed', 'n_over_budget', 'n_double', 'n_charged',
             'n_hydrogens', 'n_overvalent', 'steps')
MOL_KEYS = STAT_KEYS + ('n_atoms', 'n_bonds')
ATOM_KEYS = ('val', 'charge', 'kek_h', 'atom_flag')
BOND_KEYS = ('kek_order',)
LAYOUT = molpack.Layout(MOL_KEYS, atom=ATOM_KEYS, bond=BOND_KEYS)         # the results table
# this project's choice, unverified against RDKit (the normal valences are molpack.DEFAULT_NORMAL_VALENCE)
DEFAULT_CHARGED_VALENCE = {7: 4, 16: 3}                                   # the valence with one positive charge; absent = none
DEFAULT_FLEXIBLE = (7,)                                                   # takes a hydrogen instead of a double bond
SYMBOL = molpack.ELEMENT_SYMBOL
MASS = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998, 15: 30.974, 16: 32.06, 17: 35.45}   # standard atomic weights, abridged
STEP_BINS = 22                                                    # bin k: molecules whose steps have bit length k, the last bin also more


class KekuleTables:
    """The chemistry of one call, indexed by atom class: ``normal_valence`` V, ``charged_valence`` Vc (0 = none) as int32 arrays and
    ``flexible``, a bit mask over classes.  Built from dicts keyed by atomic number (None = the defaults above) and validated as the
    device entry validates them."""

    def __init__(self, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4, normal_valence=None, charged_valence=None, flexible=None):
        self.atomic_numbers, self.num_bond_types = tuple(int(z) for z in atomic_numbers), int(num_bond_types)
        if not 1 <= len(self.atomic_numbers) <= MAX_ELEMENTS or not 1 <= self.num_bond_types <= MAX_BOND_TYPES:
            raise ValueError(f'1 .. {MAX_ELEMENTS} elements and 1 .. {MAX_BOND_TYPES} bond types')
        nv = DEFAULT_NORMAL_VALENCE if normal_valence is None else {int(z): int(v) for z, v in dict(normal_valence).items()}
        cv = DEFAULT_CHARGED_VALENCE if charged_valence is None else {int(z): int(v) for z, v in dict(charged_valence).items()}
        fl = DEFAULT_FLEXIBLE if flexible is None else tuple(int(z) for z in flexible)
        missing = [z for z in self.atomic_numbers if z not in nv]
        if missing:
            raise ValueError(f'no normal valence for element(s) {missing}')
        if normal_valence is not None or charged_valence is not None or flexible is not None:
            unknown = sorted((set(cv) | set(fl)) - set(self.atomic_numbers))
            if unknown:
                raise ValueError(f'charged_valence / flexible name element(s) {unknown} outside the atomic numbers {self.atomic_numbers}')
        self.normal_valence = np.asarray([nv[z] for z in self.atomic_numbers], dtype=np.int32)
        self.charged_valence = np.asarray([cv.get(z, 0) for z in self.atomic_numbers], dtype=np.int32)
        if ((self.normal_valence < 0) | (self.normal_valence > MAX_VALENCE) | (self.charged_valence < 0) | (self.charged_valence > MAX_VALENCE)).any():
            raise ValueError(f'a valence lies in 0 .. {MAX_VALENCE}')
        self.flexible = sum(1 << c for c, z in enumerate(self.atomic_numbers) if z in fl)

    def key(self):
        return (self.atomic_numbers, self.num_bond_types, tuple(self.normal_valence.tolist()), tuple(self.charged_valence.tolist()), self.flexible)


def _tables(tables):
    return KekuleTables() if tables is None else tables


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def kekulize_ref(info, tables=None, max_steps=DEFAULT_MAX_STEPS):
    """Plain Python restatement of ``mdx_mol_kekulize`` for one molecule dict (element = atomic numbers, bond_index (2, 2b) with every
    bond once and then flipped, bond_type (2b)) -> dict: the per-molecule numbers of STAT_KEYS (status 0 measured, 1 too large: more
    than 256 atoms or 512 bonds, or an aromatic component of more than 64 atoms), ``n_atoms``, ``n_bonds``, per atom ``val``, ``charge``,
    ``kek_h``, ``atom_flag`` and per bond ``kek_order`` as int32 arrays.  With status 1 every other output is 0.  A bond whose index
    lies outside the molecule or with i = j is ignored (kek_order 0); a bond type outside 1 .. num_bond_types stays in the graph, adds
    nothing and is not aromatic (kek_order 0); an element outside the tables' atomic numbers and two bonds between the same pair of
    atoms raise ValueError.  A molecule is kekulizable iff status == 0 and n_failed == n_over_budget == 0 (``kekulizable``)."""
    tb = _tables(tables)
    max_steps = check_steps(max_steps)
    nbt = tb.num_bond_types
    cls, bi, bt = mol_graph(info, tb.atomic_numbers)
    n, nb = len(cls), bi.shape[1]
    valid = [0 <= bi[0, e] < n and 0 <= bi[1, e] < n and bi[0, e] != bi[1, e] for e in range(nb)]
    pairs = [(int(min(bi[:, e])), int(max(bi[:, e]))) for e in range(nb) if valid[e]]
    if len(set(pairs)) != len(pairs):
        raise ValueError('two bonds between the same pair of atoms')
    zi = lambda k: np.zeros(k, dtype=np.int32)
    out = dict({k: 0 for k in STAT_KEYS}, n_atoms=n, n_bonds=nb, val=zi(n), charge=zi(n), kek_h=zi(n), atom_flag=zi(n), kek_order=zi(nb))
    if n > MAX_ATOMS or nb > MAX_BONDS:
        return dict(out, status=STATUS_TOO_LARGE)
    V = [int(tb.normal_valence[c]) for c in cls]
    Vc = [int(tb.charged_valence[c]) for c in cls]
    flexible = [bool(tb.flexible >> int(c) & 1) for c in cls]
    sigma, arom = [0] * n, [[] for _ in range(n)]            # arom[a]: the aromatic neighbours of a
    for e in range(nb):
        t = int(bt[e])
        if not valid[e] or not 1 <= t <= nbt:
            continue
        x, y = int(bi[0, e]), int(bi[1, e])
        sigma[x] += 1 if t == nbt else t
        sigma[y] += 1 if t == nbt else t
        if t == nbt:
            arom[x].append(y), arom[y].append(x)
    role = [ROLE_NONE] * n
    for a in range(n):
        if not arom[a]:
            continue
        if len(arom[a]) > 3:
            role[a] = ROLE_NOT
        elif V[a] - sigma[a] >= 1:
            role[a] = ROLE_MAY if flexible[a] else ROLE_MUST
        else:
            role[a] = ROLE_MAY if Vc[a] - sigma[a] >= 1 else ROLE_NOT
    # the components of the aromatic bonds, each named by its smallest atom
    label = list(range(n))
    for a in range(n):
        if arom[a] and label[a] == a:
            todo = [a]
            while todo:
                x = todo.pop()
                for y in arom[x]:
                    if label[y] != a and y != a:
                        label[y] = a
                        todo.append(y)
    comps = {}
    for a in range(n):
        if arom[a]:
            comps.setdefault(label[a], []).append(a)           # ascending index
    if any(len(c) > MAX_COMPONENT for c in comps.values()):
        return dict(out, status=STATUS_TOO_LARGE)
    partner, unsolved = {}, set()
    for root, atoms in comps.items():
        count = [0]

        def search(k):
            while k < len(atoms) and (role[atoms[k]] == ROLE_NOT or atoms[k] in partner):
                k += 1
            if k == len(atoms):
                return True
            a = atoms[k]
            options = ([None] if role[a] == ROLE_MAY else []) + [b for b in sorted(arom[a]) if b > a and role[b] != ROLE_NOT and b not in partner]
            for b in options:
                if count[0] == max_steps:
                    raise OverBudget
                count[0] += 1
                if b is not None:
                    partner[a], partner[b] = b, a
                if search(k + 1):
                    return True
                if b is not None:
                    del partner[a], partner[b]
            return False
        try:
            if search(0):
                out['steps'] += count[0]
            else:
                out['n_failed'] += 1
                out['steps'] += count[0]
                unsolved.add(root)
        except OverBudget:
            for a in atoms:
                partner.pop(a, None)
            out['n_over_budget'] += 1
            unsolved.add(root)
    for a in range(n):
        bad = bool(arom[a]) and label[a] in unsolved
        matched = a in partner
        val = sigma[a] + (1 if matched else 0)
        charge = 0 if bad else int(V[a] < val <= Vc[a])
        out['val'][a], out['charge'][a] = val, charge
        out['kek_h'][a] = 0 if bad else max(0, (Vc[a] if charge else V[a]) - val)
        out['atom_flag'][a] = (role[a] | (FLAG_MATCHED if matched else 0) | (FLAG_OVERVALENT if val > max(V[a], Vc[a]) else 0) |
                               (FLAG_UNSOLVED if bad else 0))
    for e in range(nb):
        t = int(bt[e])
        if not valid[e] or not 1 <= t <= nbt:
            continue
        x, y = int(bi[0, e]), int(bi[1, e])
        if t < nbt:
            out['kek_order'][e] = t
        elif label[x] not in unsolved:
            out['kek_order'][e] = 2 if partner.get(x) == y else 1
    out.update(n_arom_atoms=sum(1 for a in range(n) if arom[a]), n_arom_bonds=sum(len(x) for x in arom) // 2, n_components=len(comps),
               n_double=len(partner) // 2, n_charged=int(out['charge'].sum()), n_hydrogens=int(out['kek_h'].sum()),
               n_overvalent=int(((out['atom_flag'] & FLAG_OVERVALENT) != 0).sum()))
    return out


def stack_ref(mols, tables=None, max_steps=DEFAULT_MAX_STEPS):
    """``kekulize_ref`` of every molecule of a list as the results dict ``kekulize_mols`` returns (numpy int32): one entry per molecule
    of every key of MOL_KEYS, the keys of ATOM_KEYS over the atoms and ``kek_order`` over the bonds of the list in turn, ``atom_ptr``
    and ``bond_ptr``"""
    tb = _tables(tables)
    return molpack.stack([kekulize_ref(m, tb, max_steps) for m in mols], LAYOUT)


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, tables=None, max_steps=DEFAULT_MAX_STEPS, select=None):
    """``mdx_mol_kekulize`` on the device arrays `cm` (a ``CompactMols``) -> dict of int32 device tensors: the keys of STAT_KEYS (B)
    each, columns of one (B, 11) table), ``val`` / ``charge`` / ``kek_h`` / ``atom_flag`` (N_cap) and ``kek_order`` (Eh_stride) in the
    layout of the inputs, zero where no molecule has a slot; no sync"""
    from . import _lib
    tb, max_steps = _tables(tables), check_steps(max_steps)
    out, stats = molpack.zeros_for(cm, LAYOUT, stat_keys=STAT_KEYS)
    if cm.B > 0:
        ops, at = cm.operands()
        _lib.check(_lib.lib().mdx_mol_kekulize(
            *ops, _lib.ptr(select), len(tb.atomic_numbers), tb.num_bond_types, tb.normal_valence.ctypes.data, tb.charged_valence.ctypes.data,
            tb.flexible, max_steps, at(out['kek_order']), at(out['val']), at(out['charge']), at(out['kek_h']), at(out['atom_flag']),
            at(stats), _lib.stream()))
    return molpack.split_stats(out, stats, STAT_KEYS)


def kekulize_mols(mols, device, tables=None, max_steps=DEFAULT_MAX_STEPS):
    """Kekulé assignment of a list of molecule dicts (finished molecules, or entries of ``samples_all.pt``) on the device: the list is
    packed densely, copied and handed to ``mdx_mol_kekulize``.  -> the results dict of ``stack_ref`` with device tensors.  Two bonds
    between the same pair of atoms and unknown elements raise ValueError."""
    tb = _tables(tables)
    check_steps(max_steps)
    p, cm = molpack.packed(mols, tb.atomic_numbers, device)
    return molpack.dense(launch(cm, tb, max_steps), cm, p, LAYOUT)


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict"""
    return molpack.concat(parts, LAYOUT)


def empty():
    return stack_ref([])


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def kekulizable(results):
    """bool per molecule: status == 0 and no aromatic component without a structure or over the budget"""
    status, failed, over = (host(results[k]) for k in ('status', 'n_failed', 'n_over_budget'))
    return (status == STATUS_OK) & (failed == 0) & (over == 0)


def mol_result(results, m):
    """molecule `m` of a results dict with host arrays as the dict ``kekulize_ref`` returns"""
    return molpack.mol_slice(results, m, LAYOUT)


def summary(results):
    """The numbers of a results dict (host or device arrays) -> dict: ``n_molecules``, ``n_measured`` (status 0), ``n_too_large``,
    ``n_kekulizable`` and ``fraction_kekulizable`` (of all molecules), ``n_no_structure`` / ``n_over_budget`` (measured molecules with
    such a component); over the kekulizable molecules ``fraction_charged`` (at least one charge), ``mean_charges``,
    ``mean_hydrogens``, ``mean_double``, and ``charged_hist`` (0, 1, 2, 3, 4 or more charges); over the measured molecules
    ``steps_hist`` (bin k: steps of bit length k, i.e. 0, 1, 2-3, 4-7, ...; the last bin also more).  NaN where nothing was counted.
    This project's model with its default tables, unverified against RDKit."""
    r = to_host(results)
    n = len(r['status'])
    ok = r['status'] == STATUS_OK
    kek = kekulizable(r)
    k = int(kek.sum())
    nan = float('nan')
    mean = lambda key: int(r[key][kek].astype(np.int64).sum()) / k if k else nan
    bits = np.asarray([min(int(s).bit_length(), STEP_BINS - 1) for s in r['steps'][ok]], dtype=np.int64)
    return {'n_molecules': n, 'n_measured': int(ok.sum()), 'n_too_large': int((r['status'] == STATUS_TOO_LARGE).sum()),
            'n_kekulizable': k, 'fraction_kekulizable': k / n if n else nan,
            'n_no_structure': int((ok & (r['n_failed'] > 0)).sum()), 'n_over_budget': int((ok & (r['n_over_budget'] > 0)).sum()),
            'fraction_charged': int((r['n_charged'][kek] > 0).sum()) / k if k else nan,
            'mean_charges': mean('n_charged'), 'mean_hydrogens': mean('n_hydrogens'), 'mean_double': mean('n_double'),
            'charged_hist': np.bincount(np.minimum(r['n_charged'][kek], 4), minlength=5).tolist(),
            'steps_hist': np.bincount(bits, minlength=STEP_BINS).tolist()}


def compare(a, b):
    """two results dicts or two summaries -> dict: Jensen-Shannon divergence (``molpack.jsd_counts``: base 2, in [0, 1], NaN when a
    side is empty) of ``steps_hist`` and ``charged_hist``, and both sides' ``fraction_kekulizable``"""
    a, b = (x if 'steps_hist' in x else summary(x) for x in (a, b))
    return {'steps': jsd_counts(a['steps_hist'], b['steps_hist']), 'charged': jsd_counts(a['charged_hist'], b['charged_hist']),
            'fraction_kekulizable': [a['fraction_kekulizable'], b['fraction_kekulizable']]}


def formula(element, n_hydrogens, charge=0):
    """Hill notation from the atomic numbers of the heavy atoms and the hydrogen count ``n_hydrogens`` of the Kekulé assignment: C, H,
    then the other symbols in alphabetical order; a net charge as a trailing '+', '2+', ..."""
    counts = {}
    for z in np.asarray(element, dtype=np.int64).reshape(-1):
        if int(z) not in SYMBOL:
            raise ValueError(f'no symbol for element {int(z)}')
        counts[SYMBOL[int(z)]] = counts.get(SYMBOL[int(z)], 0) + 1
    if int(n_hydrogens):
        counts['H'] = int(n_hydrogens)
    order = [s for s in ('C', 'H') if s in counts] if 'C' in counts else []
    order += sorted(s for s in counts if s not in order)
    text = ''.join(s + (str(counts[s]) if counts[s] > 1 else '') for s in order)
    charge = int(charge)
    return text + ('' if charge == 0 else ('+' if charge == 1 else f'{charge}+'))


def weight(element, n_hydrogens):
    """molecular weight from the heavy atoms and the hydrogen count, with the abridged standard atomic weights of ``MASS``"""
    ele = [int(z) for z in np.asarray(element, dtype=np.int64).reshape(-1)]
    missing = sorted({z for z in ele if z not in MASS})
    if missing:
        raise ValueError(f'no atomic weight for element(s) {missing}')
    return float(sum(MASS[z] for z in ele) + MASS[1] * int(n_hydrogens))


def kekule_mol_block(info, result, name='moldiff_amd'):
    """V2000 mol block of a kekulizable molecule: the bonds with the orders 1 / 2 / 3 of ``kek_order`` and the charges as ``M  CHG``
    lines (8 per line).  info: the molecule dict; result: its ``kekulize_ref`` dict or ``mol_result`` slice.  ``sample_drug3d.mol_block``
    writes the aromatic form and is unchanged; ``sample_drug3d.read_mol_block`` reads this block back (it does not read charges).
    Hydrogens stay implicit.  A molecule that is not kekulizable, or that holds an ignored bond, raises ValueError."""
    if not bool(kekulizable({k: np.asarray(result[k]) for k in ('status', 'n_failed', 'n_over_budget')})):
        raise ValueError('the molecule is not kekulizable: there is no Kekulé form to write')
    ele, pos = np.asarray(info['element']), np.asarray(info['atom_pos'])
    bi = np.asarray(info['bond_index'])
    nb = bi.shape[1] // 2
    order = np.asarray(result['kek_order'])
    if len(order) != nb or (order[:nb] < 1).any():
        raise ValueError('an ignored bond or a bond type outside the featuriser has no order to write')
    lines = [name, '  moldiff_amd', '', '%3d%3d  0  0  0  0  0  0  0  0999 V2000' % (len(ele), nb)]
    for e, p in zip(ele, pos):
        lines.append('%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0' % (p[0], p[1], p[2], SYMBOL.get(int(e), 'X')))
    for k in range(nb):
        lines.append('%3d%3d%3d  0' % (bi[0, k] + 1, bi[1, k] + 1, order[k]))
    charged = [(a + 1, int(c)) for a, c in enumerate(np.asarray(result['charge'])) if c]
    for k in range(0, len(charged), 8):
        part = charged[k:k + 8]
        lines.append('M  CHG%3d' % len(part) + ''.join(' %3d %3d' % ac for ac in part))
    lines.append('M  END')
    return '\n'.join(lines) + '\n'


def read_charges(text):
    """the ``M  CHG`` lines of a mol block -> {atom index (0-based): charge}"""
    out = {}
    for ln in text.splitlines():
        if ln.startswith('M  CHG'):
            for k in range(int(ln[6:9])):
                out[int(ln[9 + 8 * k:13 + 8 * k]) - 1] = int(ln[13 + 8 * k:17 + 8 * k])
    return out


def write_sdf(path, mols, results):
    """the kekulizable molecules of `mols` (results: host arrays, one entry per molecule) as Kekulé mol blocks -> how many were written.
    A kekulizable molecule that holds an ignored bond is left out."""
    r, written = to_host(results), 0
    keep = kekulizable(r)
    with open(path, 'w') as f:
        for m, info in enumerate(mols):
            res = mol_result(r, m)
            if keep[m] and (res['kek_order'] >= 1).all():
                f.write(kekule_mol_block(info, res) + '$$$$\n')
                written += 1
    return written


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m moldiff_amd.kekule', description=__doc__.split('\n\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    s = sub.add_parser('stats', help='Kekulé assignment of the molecules stored in a samples_all.pt')
    s.add_argument('samples')
    s.add_argument('--out', required=True)
    s.add_argument('--sdf', default=None, help='also write the kekulizable molecules as Kekulé mol blocks')
    s.add_argument('--part', default='finished')
    s.add_argument('--max_steps', type=int, default=DEFAULT_MAX_STEPS)
    s.add_argument('--device', default='cuda:0')
    s.add_argument('--ref', action='store_true', help='the Python path instead of the device')
    c = sub.add_parser('compare', help='Jensen-Shannon divergence of the steps and charge count distributions of two files')
    c.add_argument('a')
    c.add_argument('b')
    args = ap.parse_args(argv)
    if args.cmd == 'stats':
        mols = load_mols(args.samples, args.part)
        if args.ref:
            res = stack_ref(mols, max_steps=args.max_steps)
        else:
            import torch
            torch.cuda.set_device(torch.device(args.device))
            res = kekulize_mols(mols, args.device, max_steps=args.max_steps)
        save_npz(res, args.out)
        if args.sdf:
            write_sdf(args.sdf, mols, res)
        print(json.dumps(summary(res), indent=1))
    else:
        print(json.dumps(compare(load_npz(args.a), load_npz(args.b)), indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
