"""Frameworks and ring systems of decoded molecules: the skeleton of a molecule without its decoration (in the spirit of Bemis and
Murcko), its ring systems, linkers and side chains, each piece again a compact molecule, and exact keys for the pieces.

The device half is ``mdx_mol_framework`` (csrc/mdx_framework.hip), reached through ``framework_mols`` (a list of molecule dicts),
``launch`` (a ``CompactMols`` and the ring data of ``rings.launch``) and ``FeaturizeMol.framework_batch`` (the sampler's predictions).
``framework_ref`` is the plain restatement for one molecule and needs no GPU; the GPU tests compare every output exactly.  ``keys``
runs ``mdx_mol_canon`` on the framework and on the ring systems, which makes "the same framework" an exact statement.

What it is: the reference's ``ring_type`` metric (utils/evaluation.py: RingAnalyzer) reports which rings occur and how often, and
scaffold uniqueness and novelty are the usual second half of a generative model's report.  RDKit is not available here, so this is
THIS PROJECT'S OWN DEFINITION, stated exactly in include/moldiff_hip.h: it is NOT ``rdkit.Chem.Scaffolds.MurckoScaffold`` and agreement
with RDKit is UNMEASURED.  The word is *framework*: ``moldiff_amd/scaffold.py`` and ``--scaffold`` mean scaffold-constrained sampling.

The definition in short, on the graph of the valid bonds.  A ring bond is a bond that is no bridge (``bond_ring_min != 0``), a ring
atom an atom with one.  The core is the 2-core: delete atoms with at most one remaining bond until none is left; a core atom without a
ring bond is a linker atom.  With EXO (mode bit 0) an atom outside the core with exactly one bond, of type 2, to a core atom joins as an
exo atom.  The framework is the core plus the exo atoms.  A ring system is a connected component of the ring bonds; systems are
numbered by their smallest atom; one with a atoms and b bonds has b - a + 1 rings.  A fusion atom has at least three ring bonds.
GENERIC (mode bit 1) writes every atom of the pieces as class 0 and every bond as type 1.

    python -m moldiff_amd.framework stats samples_all.pt --out frameworks.npz [--ref] [--exo] [--generic] [--part finished]
    python -m moldiff_amd.framework compare a.npz b.npz
"""
import argparse
import json
import sys

import numpy as np

from . import canon, molpack, rings
from .molpack import CompactMols, DEFAULT_ATOMIC_NUMBERS, jsd_counts, load_mols, load_npz, mol_graph, save_npz, to_host

MAX_ATOMS, MAX_BONDS = rings.MAX_ATOMS, rings.MAX_BONDS           # include/moldiff_hip.h: the caps of mdx_mol_rings
MODE_EXO, MODE_GENERIC = 1, 2
MAX_BINS, DEFAULT_BINS = 16, 8
STATUS_OK, STATUS_TOO_LARGE, STATUS_NO_RINGS = 0, 1, 2
ROLE_SIDE, ROLE_LINKER, ROLE_RING, ROLE_EXO = 0, 1, 2, 3
# the columns of the device's per-molecule table, in its order (include/moldiff_hip.h: MDX_FW_STATS)
STAT_KEYS = ('status', 'n_fw_atoms', 'n_fw_bonds', 'n_systems', 'n_linker', 'n_side', 'n_exo', 'n_fusion', 'largest_system', 'most_rings')
MOL_KEYS = STAT_KEYS + ('sys_hist', 'n_atoms', 'n_bonds')
RECORD_KEYS = ('sys_atom_ptr', 'sys_bond_ptr', 'sys_n_atoms', 'sys_n_bonds')        # system k of molecule m at slot atom_ptr[m] + k
ATOM_KEYS = ('atom_role', 'atom_system', 'fw_atom_type', 'fw_atom_map', 'sys_atom_type', 'sys_atom_map') + RECORD_KEYS   # + fw_pos, sys_pos
BOND_KEYS = ('bond_role', 'fw_bond_type', 'sys_bond_type')                          # + fw_bond_index, sys_bond_index (2, bonds)
INDEX_KEYS = ('fw_bond_index', 'sys_bond_index')
POS_KEYS = ('fw_pos', 'sys_pos')
LAYOUT = molpack.Layout(MOL_KEYS, atom=ATOM_KEYS, bond=BOND_KEYS, index=INDEX_KEYS, pos=POS_KEYS, wide=('sys_hist',))   # the results table
KEY_OK, KEY_NONE, KEY_ABANDONED = 0, 1, 2          # a piece's key: there; the molecule was not measured; the canonical search gave up
KEY_ARRAYS = ('fw_key_status', 'fw_hash', 'fw_cert_ptr', 'fw_cert', 'sys_mol', 'sys_key_status', 'sys_hash', 'sys_cert_ptr', 'sys_cert')
STAT_BINS = 33                                     # the distributions of ``summary``: bin k = the value k, the last bin every larger one


def _check(mode, sys_bins):
    if not 0 <= int(mode) <= (MODE_EXO | MODE_GENERIC):
        raise ValueError(f'mode is a bit field of EXO = 1 and GENERIC = 2, got {mode}')
    if not 1 <= int(sys_bins) <= MAX_BINS:
        raise ValueError(f'sys_bins must lie in 1 .. 16, got {sys_bins}')
    return int(mode), int(sys_bins)


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def framework_ref(info, mode=0, sys_bins=DEFAULT_BINS, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
    """Plain restatement of ``mdx_mol_framework`` for one molecule dict (element = atomic numbers, bond_index (2, 2b) with every bond
    once and then flipped, bond_type (2b), optionally atom_pos); the ring bonds come from ``rings.rings_ref``.  -> dict: the keys of
    STAT_KEYS, ``sys_hist`` (sys_bins), ``n_atoms``, ``n_bonds``; per atom slot the keys of ATOM_KEYS (``sys_atom_ptr`` and
    ``sys_bond_ptr`` count from the molecule's own first atom / bond) and, when the dict holds positions, ``fw_pos`` / ``sys_pos``; per
    bond slot the keys of BOND_KEYS and ``fw_bond_index`` / ``sys_bond_index`` (2, nb).  With a non-zero status every count is 0,
    atom_system -1 and everything else 0.  Two bonds between one pair of atoms and unknown elements raise ValueError."""
    mode, sys_bins = _check(mode, sys_bins)
    cls, bi, bt = mol_graph(info, atomic_numbers)
    n, nb = len(cls), bi.shape[1]
    ring = rings.rings_ref(info, num_bond_types, atomic_numbers)
    pos = np.asarray(info['atom_pos'], dtype=np.float32).reshape(n, 3) if 'atom_pos' in info else None
    zi = lambda *k: np.zeros(k, dtype=np.int32)
    out = dict({k: 0 for k in STAT_KEYS}, sys_hist=zi(sys_bins), n_atoms=n, n_bonds=nb)
    out.update({k: zi(n) for k in ATOM_KEYS}, atom_system=np.full(n, -1, dtype=np.int32))
    out.update({k: zi(nb) for k in BOND_KEYS}, fw_bond_index=zi(2, nb), sys_bond_index=zi(2, nb))
    if pos is not None:
        out.update(fw_pos=np.zeros((n, 3), dtype=np.float32), sys_pos=np.zeros((n, 3), dtype=np.float32))
    if n > MAX_ATOMS or nb > MAX_BONDS:
        return dict(out, status=STATUS_TOO_LARGE)
    if ring['status'] != rings.STATUS_OK:
        return dict(out, status=STATUS_NO_RINGS)
    bonds = [(e, int(bi[0, e]), int(bi[1, e])) for e in range(nb) if 0 <= bi[0, e] < n and 0 <= bi[1, e] < n and bi[0, e] != bi[1, e]]
    is_ring = {e: bool(ring['bond_ring_min'][e] != 0) for e, _, _ in bonds}
    nbr = [[] for _ in range(n)]
    for e, x, y in bonds:
        nbr[x].append((y, e))
        nbr[y].append((x, e))
    # the core: delete, until nothing changes, every atom with at most one remaining bond
    core = set(range(n))
    changed = True
    while changed:
        changed = False
        for a in sorted(core):
            if sum(u in core for u, _ in nbr[a]) <= 1:
                core.discard(a)
                changed = True
    ring_atom = [any(is_ring[e] for _, e in nbr[a]) for a in range(n)]
    role = out['atom_role']
    for a in range(n):
        if a in core:
            role[a] = ROLE_RING if ring_atom[a] else ROLE_LINKER
        elif mode & MODE_EXO and len(nbr[a]) == 1 and bt[nbr[a][0][1]] == 2 and nbr[a][0][0] in core:
            role[a] = ROLE_EXO
    for e, x, y in bonds:
        if is_ring[e]:
            out['bond_role'][e] = 2
        elif x in core and y in core:
            out['bond_role'][e] = 1
        elif ROLE_EXO in (role[x], role[y]):
            out['bond_role'][e] = 3
    # ring systems: the components of the ring bonds, in the order of their smallest atoms
    system = out['atom_system']
    n_sys = 0
    for r in range(n):
        if ring_atom[r] and system[r] < 0:
            system[r], stack = n_sys, [r]
            while stack:
                a = stack.pop()
                for u, e in nbr[a]:
                    if is_ring[e] and system[u] < 0:
                        system[u] = n_sys
                        stack.append(u)
            n_sys += 1
    generic = bool(mode & MODE_GENERIC)
    atype = lambda a: 0 if generic else int(cls[a])
    btype = lambda e: 1 if generic else int(bt[e])
    # the framework as a compact molecule: atoms and bonds in their original order
    fw_atoms = [a for a in range(n) if role[a] != ROLE_SIDE]
    fw_bonds = [e for e in range(nb) if out['bond_role'][e] != 0]
    new = {a: p for p, a in enumerate(fw_atoms)}
    for p, a in enumerate(fw_atoms):
        out['fw_atom_type'][p], out['fw_atom_map'][p] = atype(a), a
        if pos is not None:
            out['fw_pos'][p] = pos[a]
    for p, e in enumerate(fw_bonds):
        out['fw_bond_index'][:, p], out['fw_bond_type'][p] = (new[int(bi[0, e])], new[int(bi[1, e])]), btype(e)
    # the ring systems as compact molecules, one behind the other
    a0 = b0 = most = largest = 0
    for k in range(n_sys):
        atoms = [a for a in range(n) if system[a] == k]
        sbonds = [e for e, x, _ in bonds if is_ring[e] and system[x] == k]
        local = {a: p for p, a in enumerate(atoms)}
        out['sys_atom_ptr'][k], out['sys_bond_ptr'][k], out['sys_n_atoms'][k], out['sys_n_bonds'][k] = a0, b0, len(atoms), len(sbonds)
        for p, a in enumerate(atoms):
            out['sys_atom_type'][a0 + p], out['sys_atom_map'][a0 + p] = atype(a), a
            if pos is not None:
                out['sys_pos'][a0 + p] = pos[a]
        for p, e in enumerate(sbonds):
            out['sys_bond_index'][:, b0 + p], out['sys_bond_type'][b0 + p] = (local[int(bi[0, e])], local[int(bi[1, e])]), btype(e)
        n_rings = len(sbonds) - len(atoms) + 1
        out['sys_hist'][min(n_rings - 1, sys_bins - 1)] += 1
        most, largest = max(most, n_rings), max(largest, len(atoms))
        a0, b0 = a0 + len(atoms), b0 + len(sbonds)
    out.update(n_fw_atoms=len(fw_atoms), n_fw_bonds=len(fw_bonds), n_systems=n_sys, n_linker=int((role == ROLE_LINKER).sum()),
               n_side=int((role == ROLE_SIDE).sum()), n_exo=int((role == ROLE_EXO).sum()),
               n_fusion=sum(sum(is_ring[e] for _, e in nbr[a]) >= 3 for a in range(n)), largest_system=largest, most_rings=most)
    return out


def stack_ref(mols, mode=0, sys_bins=DEFAULT_BINS, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
    """``framework_ref`` of every molecule of a list as the results dict ``framework_mols`` returns (numpy int32): one entry (or row, for
    ``sys_hist``) per molecule of every key of MOL_KEYS, the per-atom keys over the atoms and the per-bond keys over the bond slots of
    the list in turn (the two index arrays (2, bonds)), ``atom_ptr`` and ``bond_ptr``.  ``sys_atom_ptr`` / ``sys_bond_ptr`` count from
    the start of the list, as on the device.  ``fw_pos`` / ``sys_pos`` are present when every molecule holds positions."""
    mode, sys_bins = _check(mode, sys_bins)
    out = molpack.stack([framework_ref(m, mode, sys_bins, atomic_numbers, num_bond_types) for m in mols], LAYOUT, {'sys_hist': sys_bins})
    for a0, b0, k in zip(out['atom_ptr'], out['bond_ptr'], out['n_systems']):   # the records point into the list's arrays
        out['sys_atom_ptr'][a0:a0 + k] += a0
        out['sys_bond_ptr'][a0:a0 + k] += b0
    order = MOL_KEYS + ('atom_ptr', 'bond_ptr') + ATOM_KEYS + BOND_KEYS + INDEX_KEYS + POS_KEYS     # the key order of the stored files
    return {k: out[k] for k in order if k in out}


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, ring_data, mode=0, sys_bins=DEFAULT_BINS, select=None, positions=True):
    """``mdx_mol_framework`` on the device arrays `cm` (a ``CompactMols``) with the results of ``rings.launch`` on the same arrays (its
    ``bond_ring_min`` and ``status`` are read) -> dict of device tensors: the keys of STAT_KEYS (B) each (int32, columns of one
    (B, 10) table), ``sys_hist`` (B, sys_bins), the keys of ATOM_KEYS (N_cap) and BOND_KEYS (Eh_stride), ``fw_bond_index`` /
    ``sys_bond_index`` (2, Eh_stride) in the layout of the inputs, zero where no molecule has a slot; ``fw_pos`` / ``sys_pos``
    (N_cap, 3) when `cm` holds positions and `positions` is set.  No sync."""
    import torch
    from . import _lib
    mode, sys_bins = _check(mode, sys_bins)
    B, pos = cm.B, cm.atom_pos if positions else None
    out, stats = molpack.zeros_for(cm, LAYOUT, {'sys_hist': sys_bins}, STAT_KEYS, held=POS_KEYS if pos is not None else ())
    if B > 0:
        brm, rstat = ring_data['bond_ring_min'], ring_data['status']
        if brm.dtype != torch.int32 or rstat.dtype != torch.int32 or brm.numel() < cm.Eh_stride or rstat.numel() < B:
            raise ValueError('ring_data holds bond_ring_min and status of rings.launch on the same arrays')
        brm, rstat = brm.contiguous(), rstat.contiguous()
        ops, at = cm.operands()
        opt = lambda t: None if t is None else at(t)
        g = lambda k: at(out[k])
        _lib.check(_lib.lib().mdx_mol_framework(
            *ops, _lib.ptr(select), opt(pos), at(brm), at(rstat), mode, sys_bins, g('atom_role'), g('atom_system'), g('bond_role'), at(stats),
            g('sys_hist'), g('fw_atom_type'), g('fw_atom_map'), opt(out.get('fw_pos')), g('fw_bond_index'), g('fw_bond_type'),
            g('sys_atom_ptr'), g('sys_bond_ptr'), g('sys_n_atoms'), g('sys_n_bonds'), g('sys_atom_type'), g('sys_atom_map'),
            opt(out.get('sys_pos')), g('sys_bond_index'), g('sys_bond_type'), _lib.stream()))
    else:
        out['atom_system'] -= 1
    return molpack.split_stats(out, stats, STAT_KEYS)


def framework_mols(mols, device, mode=0, sys_bins=DEFAULT_BINS, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4, with_cm=False):
    """Frameworks and ring systems of a list of molecule dicts (finished molecules, or entries of ``samples_all.pt``) on the device: the
    list is packed densely, copied and handed to ``mdx_mol_rings`` and then ``mdx_mol_framework``.  -> the results dict of ``stack_ref``
    with device tensors; with `with_cm` -> (that, the ``CompactMols`` of the list, ``launch``'s own dict): what ``keys`` takes.  Two
    bonds between the same pair of atoms and unknown elements raise ValueError."""
    mode, sys_bins = _check(mode, sys_bins)
    atomic_numbers = tuple(int(z) for z in atomic_numbers)
    p, cm = molpack.packed(mols, atomic_numbers, device, positions=True)
    full = launch(cm, rings.launch(cm, len(atomic_numbers), num_bond_types), mode, sys_bins)
    out = molpack.dense(dict(full), cm, p, LAYOUT)
    return (out, cm, full) if with_cm else out


def framework_compact(cm, results):
    """The framework arrays of ``launch``'s results as a ``CompactMols`` in the layout of `cm` (same atom_ptr / bond_ptr, the counts
    ``n_fw_atoms`` / ``n_fw_bonds``): what ``canon.launch``, ``rings.launch`` and ``kekule.launch`` take.  A molecule that was not
    measured, or without rings, is an empty molecule there."""
    idx = results['fw_bond_index'].contiguous()
    return cm._replace(n_atoms=results['n_fw_atoms'].contiguous(), n_bonds=results['n_fw_bonds'].contiguous(),
                       atom_type=results['fw_atom_type'], bond_type=results['fw_bond_type'], bond_index=idx, Eh_stride=int(idx.shape[1]),
                       atom_pos=results.get('fw_pos'))


def systems_compact(cm, results):
    """The S ring systems of ``launch``'s results as a ``CompactMols`` of S molecules over the ``sys_*`` arrays, in the order of their
    molecules and ordinals -> (CompactMols, sys_mol): sys_mol (S, int64 on the device) is the molecule that owns each.  The records
    are gathered with torch on the device (the system counts give their slots); the call synchronises once, to learn S."""
    import torch
    dev = cm.device
    n_sys = results['n_systems'].to(torch.int64)
    sys_mol = torch.repeat_interleave(torch.arange(cm.B, device=dev), n_sys)
    ordinal = torch.arange(len(sys_mol), device=dev) - (torch.cumsum(n_sys, 0) - n_sys)[sys_mol]
    slot = cm.atom_ptr.to(torch.int64)[sys_mol] + ordinal
    rec = [results[k][slot].contiguous() for k in RECORD_KEYS]
    idx = results['sys_bond_index'].contiguous()
    return CompactMols(len(sys_mol), rec[0], rec[1], rec[2], rec[3], results['sys_atom_type'], cm.N_cap, results['sys_bond_type'], idx,
                       int(idx.shape[1]), results.get('sys_pos')), sys_mol


def _cert_arrays(canon_results, unmeasured):
    """the full certificates of a canon results dict (host arrays) as key status, flat int32 data and pointers"""
    status, data, ptr = [], [], [0]
    for m in range(len(canon_results['status'])):
        c = None if unmeasured[m] else canon.certificate(canon_results, m)
        status.append(KEY_NONE if unmeasured[m] else KEY_OK if c is not None else KEY_ABANDONED)
        if c is not None:
            data.append(np.frombuffer(c, dtype=np.int32))
        ptr.append(ptr[-1] + (len(data[-1]) if c is not None else 0))
    return (np.asarray(status, dtype=np.int32).reshape(-1), np.asarray(ptr, dtype=np.int64),
            np.concatenate(data + [np.zeros(0, dtype=np.int32)]).astype(np.int32))


def keys(cm, results, max_nodes=canon.DEFAULT_MAX_NODES, select=None):
    """Exact keys of the pieces: ``canon.launch`` on ``framework_compact`` and on ``systems_compact`` of ``launch``'s results -> dict of
    host arrays (KEY_ARRAYS): per molecule ``fw_key_status`` (0 a key; 1 none: the molecule was not measured or `select` leaves it out;
    2 the canonical search was abandoned), ``fw_hash`` (the certificate hash, 0 without a key) and the full certificate of
    ``canon.certificate`` as int32 values ``fw_cert[fw_cert_ptr[m] : fw_cert_ptr[m + 1]]``; per ring system the same under ``sys_*``
    and ``sys_mol``, the owning molecule.  An empty framework has the key of the empty molecule.  Two pieces are the same labelled
    graph iff their full certificates are equal."""
    import torch
    if select is not None:
        select = select.to(cm.device, torch.int32).contiguous()
    fw = framework_compact(cm, results)
    sy, sys_mol = systems_compact(cm, results)
    out = {}
    status = to_host({'s': results['status']})['s']
    sel = np.ones(len(status), dtype=bool) if select is None else to_host({'s': select})['s'] != 0
    for name, view, skip in (('fw', fw, (status != STATUS_OK) | ~sel), ('sys', sy, np.zeros(sy.B, dtype=bool))):
        r = canon.launch(view, max_nodes, select=select if name == 'fw' else None, positions=False)
        r.update(n_atoms=view.n_atoms, n_bonds=view.n_bonds, atom_ptr=view.atom_ptr, bond_ptr=view.bond_ptr)
        r = to_host(r)
        out[name + '_key_status'], out[name + '_cert_ptr'], out[name + '_cert'] = _cert_arrays(r, skip)
        out[name + '_hash'] = np.where(out[name + '_key_status'] == KEY_OK, r['cert_hash'], 0).astype(np.int64)
    out['sys_mol'] = sys_mol.cpu().numpy().astype(np.int64)
    return out


def keys_ref(mols, results, max_nodes=canon.DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """``keys`` on the host, from ``canon.canon_ref`` on the pieces of a results dict with host arrays"""
    r = to_host(results)
    fw_mols, sys_mols, sys_mol = [], [], []
    for m in range(len(r['status'])):
        fw_mols.append(piece_mol(r, m, None, atomic_numbers))
        for k in range(int(r['n_systems'][m])):
            sys_mols.append(piece_mol(r, m, k, atomic_numbers))
            sys_mol.append(m)
    out = {}
    for name, pieces, skip in (('fw', fw_mols, r['status'] != STATUS_OK), ('sys', sys_mols, np.zeros(len(sys_mols), dtype=bool))):
        c = canon.stack_ref(pieces, max_nodes=max_nodes, atomic_numbers=atomic_numbers)
        out[name + '_key_status'], out[name + '_cert_ptr'], out[name + '_cert'] = _cert_arrays(c, skip)
        out[name + '_hash'] = np.where(out[name + '_key_status'] == KEY_OK, c['cert_hash'], 0).astype(np.int64)
    out['sys_mol'] = np.asarray(sys_mol, dtype=np.int64).reshape(-1)
    return out


def piece_mol(results, m, system=None, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """The framework (system None) or ring system `system` of molecule `m` of a results dict with host arrays, as a molecule dict
    (``element``, ``bond_index`` (2, 2b) with every bond once and then flipped, ``bond_type``, ``atom_map``: the original local index
    of every atom, ``atom_pos`` when the results hold positions)"""
    if system is None:
        a0, b0, na, nb = (int(results[k][m]) for k in ('atom_ptr', 'bond_ptr', 'n_fw_atoms', 'n_fw_bonds'))
        pre = 'fw_'
    else:
        slot = int(results['atom_ptr'][m]) + int(system)
        a0, b0, na, nb = (int(results[k][slot]) for k in RECORD_KEYS)
        pre = 'sys_'
    z = np.asarray(atomic_numbers, dtype=np.int64)
    bi = results[pre + 'bond_index'][:, b0:b0 + nb].astype(np.int64)
    bt = results[pre + 'bond_type'][b0:b0 + nb].astype(np.int64)
    out = {'element': z[results[pre + 'atom_type'][a0:a0 + na]], 'bond_index': np.concatenate([bi, bi[::-1]], axis=1),
           'bond_type': np.concatenate([bt, bt]), 'atom_map': results[pre + 'atom_map'][a0:a0 + na].astype(np.int64)}
    if pre + 'pos' in results:
        out['atom_pos'] = results[pre + 'pos'][a0:a0 + na]
    return out


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed; with or without the arrays of ``keys`` merged in) as one
    results dict: the system records and ``sys_mol`` are moved to the joint numbering"""
    parts = [to_host(p) for p in parts]
    out = molpack.concat(parts, LAYOUT)
    a0 = b0 = 0
    for p in parts:   # the records of a part point into the part's own arrays
        rec = slice(a0, a0 + len(p['atom_role']))
        there = out['sys_n_atoms'][rec] > 0
        out['sys_atom_ptr'][rec][there] += a0
        out['sys_bond_ptr'][rec][there] += b0
        a0, b0 = a0 + len(p['atom_role']), b0 + len(p['bond_role'])
    if all('fw_cert' in p for p in parts):
        m0 = 0
        for pre in ('fw_', 'sys_'):
            for k in ('key_status', 'hash', 'cert'):
                out[pre + k] = np.concatenate([p[pre + k] for p in parts])
            lens = np.concatenate([np.diff(p[pre + 'cert_ptr']) for p in parts] + [np.zeros(0, dtype=np.int64)])
            out[pre + 'cert_ptr'] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        mol = []
        for p in parts:
            mol.append(p['sys_mol'] + m0)
            m0 += len(p['status'])
        out['sys_mol'] = np.concatenate(mol).astype(np.int64)
    return out


def empty(sys_bins=DEFAULT_BINS, with_keys=False):
    out = stack_ref([], 0, sys_bins)
    if with_keys:
        out.update(keys_ref([], out))
    return out


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def _certs(keys, pre):
    """the full certificates of the pieces as bytes, None without a key"""
    ptr, data, status = keys[pre + 'cert_ptr'], keys[pre + 'cert'], keys[pre + 'key_status']
    return [data[int(ptr[m]):int(ptr[m + 1])].astype(np.int32).tobytes() if status[m] == KEY_OK else None for m in range(len(status))]


def _framework_certs(results):
    """the certificates of the NON-EMPTY frameworks with a key, None for every other molecule"""
    r = results
    certs = _certs(r, 'fw_')
    return [c if c is not None and r['n_fw_atoms'][m] > 0 else None for m, c in enumerate(certs)]


def cert_mol(cert, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """a full certificate (bytes) back as a molecule dict in canonical atom order: the piece itself, up to isomorphism"""
    w = np.frombuffer(cert, dtype=np.int32).astype(np.int64)
    n = int(w[0])
    k = int(w[1 + n])
    words = w[2 + n:2 + n + k]
    bi = np.stack([words >> 20, (words >> 8) & 0xfff]).reshape(2, k)
    bt = words & 0xff
    return {'element': np.asarray(atomic_numbers, dtype=np.int64)[w[1:1 + n]], 'bond_index': np.concatenate([bi, bi[::-1]], axis=1),
            'bond_type': np.concatenate([bt, bt])}


def cert_smiles(certs, device=None, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, tables=None):
    """A Kekulé-form SMILES (``canon.smiles``: this project's own string, not RDKit's) per full certificate: the pieces are rebuilt in
    canonical order, kekulized together on `device` (``kekule.kekulize_mols``, i.e. ``kekule.launch``) or with ``kekule.stack_ref``
    when it is None, and written -> list of strings, None where the piece has no Kekulé structure or cannot be written.  A piece has
    lost its substituents, so the hydrogens are those of the piece."""
    from . import kekule
    mols = [cert_mol(c, atomic_numbers) for c in certs]
    if not mols:
        return []
    tables = kekule.KekuleTables(atomic_numbers) if tables is None else tables
    kek = kekule.stack_ref(mols, tables) if device is None else to_host(kekule.kekulize_mols(mols, device, tables))
    out = []
    for k, mol in enumerate(mols):
        try:
            out.append(canon.smiles(mol, kekule.mol_result(kek, k)))
        except ValueError:
            out.append(None)
    return out


def _top(certs, top_k, device, atomic_numbers):
    """the `top_k` most frequent certificates: count, fraction, size and SMILES; ties by certificate, so the table has one value"""
    count = {}
    for c in certs:
        count[c] = count.get(c, 0) + 1
    rows = sorted(count.items(), key=lambda kv: (-kv[1], kv[0]))[:top_k]
    text = cert_smiles([c for c, _ in rows], device, atomic_numbers)
    out = []
    for (c, k), s in zip(rows, text):
        w = np.frombuffer(c, dtype=np.int32)
        out.append({'count': k, 'fraction': k / len(certs), 'n_atoms': int(w[0]), 'n_bonds': int(w[1 + int(w[0])]),
                    'cert_hash': canon.fnv1a64(w.tolist()), 'smiles': s})
    return out


def summary(results, keys=None, top_k=10, device=None, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """The numbers of a results dict (host or device arrays) with the arrays of ``keys`` (given, or merged into `results`) -> dict:
    ``n_molecules``, ``n_measured`` (status 0), ``n_too_large``, ``n_no_ring_data``; over the measured molecules ``n_empty`` and
    ``empty_fraction`` (no framework: acyclic), ``n_keyed`` (non-empty frameworks with a key), ``n_abandoned`` (frameworks whose
    canonical search gave up: no key, counted nowhere else), ``n_distinct`` and ``uniqueness`` = n_distinct / n_keyed, decided on the
    FULL CERTIFICATE; ``n_systems``, ``n_systems_abandoned``, ``n_distinct_systems``; ``stats``: per key of STAT_KEYS[1:] its mean
    and histogram (bin k = value k, the last bin every larger one); ``system_rings`` (bin k = systems of 1 + k rings) as counts and
    fractions; ``top_frameworks`` and ``top_systems``: the `top_k` most frequent with count, fraction, size, certificate hash and a
    Kekulé-form SMILES (``cert_smiles``; None where that fails).  NaN where nothing was counted.  The definitions are this project's
    own, not RDKit's MurckoScaffold."""
    r = to_host(results)
    if keys is not None:
        r.update(to_host(keys))
    if 'fw_cert' not in r:
        raise ValueError('the results hold no keys: pass the dict of keys(), or merge it into the results')
    ok = r['status'] == STATUS_OK
    k, nan = int(ok.sum()), float('nan')
    fw = [c for c in _framework_certs(r) if c is not None]
    sy = [c for c in _certs(r, 'sys_') if c is not None]
    empty_fw = ok & (r['n_fw_atoms'] == 0)
    stats = {}
    for key in STAT_KEYS[1:]:
        v = r[key][ok].astype(np.int64)
        stats[key] = {'mean': float(v.sum()) / k if k else nan, 'hist': np.bincount(np.minimum(v, STAT_BINS - 1), minlength=STAT_BINS).tolist()}
    hist = r['sys_hist'][ok].astype(np.int64).sum(0)
    total = int(hist.sum())
    return {'n_molecules': len(ok), 'n_measured': k, 'n_too_large': int((r['status'] == STATUS_TOO_LARGE).sum()),
            'n_no_ring_data': int((r['status'] == STATUS_NO_RINGS).sum()), 'n_empty': int(empty_fw.sum()),
            'empty_fraction': int(empty_fw.sum()) / k if k else nan, 'n_keyed': len(fw),
            'n_abandoned': int((ok & (r['fw_key_status'] == KEY_ABANDONED)).sum()), 'n_distinct': len(set(fw)),
            'uniqueness': len(set(fw)) / len(fw) if fw else nan, 'n_systems': len(r['sys_key_status']),
            'n_systems_abandoned': int((r['sys_key_status'] == KEY_ABANDONED).sum()), 'n_distinct_systems': len(set(sy)),
            'stats': stats, 'system_rings': {'counts': hist.tolist(), 'fractions': [int(c) / total if total else nan for c in hist]},
            'top_frameworks': _top(fw, top_k, device, atomic_numbers), 'top_systems': _top(sy, top_k, device, atomic_numbers)}


def novelty(results, reference, what='framework'):
    """the fraction of the keyed non-empty frameworks (what = 'framework') or of the keyed ring systems ('system') of `results` whose
    full certificate occurs nowhere among those of `reference` (NaN when there is none).  Both are results dicts with the arrays of
    ``keys`` merged in, made with the same mode."""
    if what not in ('framework', 'system'):
        raise ValueError("what is 'framework' or 'system'")
    pick = (lambda r: _framework_certs(r)) if what == 'framework' else (lambda r: _certs(r, 'sys_'))
    known = {c for c in pick(to_host(reference)) if c is not None}
    mine = [c for c in pick(to_host(results)) if c is not None]
    return sum(c not in known for c in mine) / len(mine) if mine else float('nan')


def compare(a, b):
    """two results dicts with keys -> dict: Jensen-Shannon divergence (``molpack.jsd_counts``) of the system-ring distribution and of
    the framework-atom, linker-atom and system-count histograms, both sides' ``uniqueness`` and ``empty_fraction``, and the novelty of
    each side against the other for frameworks and for ring systems, by full certificate"""
    sa, sb = summary(a, top_k=0), summary(b, top_k=0)
    if len(sa['system_rings']['counts']) != len(sb['system_rings']['counts']):
        raise ValueError('system_rings: the two sides have different bins')
    out = {'system_rings': jsd_counts(sa['system_rings']['counts'], sb['system_rings']['counts'])}
    for key in ('n_fw_atoms', 'n_linker', 'n_systems'):
        out[key] = jsd_counts(sa['stats'][key]['hist'], sb['stats'][key]['hist'])
    out.update(uniqueness=[sa['uniqueness'], sb['uniqueness']], empty_fraction=[sa['empty_fraction'], sb['empty_fraction']],
               framework_novelty=[novelty(a, b), novelty(b, a)], system_novelty=[novelty(a, b, 'system'), novelty(b, a, 'system')])
    return out


def mol_result(results, m):
    """molecule `m` of a results dict with host arrays as the dict ``framework_ref`` returns (the records count from the molecule's
    own first atom / bond again)"""
    out = molpack.mol_slice(results, m, LAYOUT)
    for key, first in (('sys_atom_ptr', 'atom_ptr'), ('sys_bond_ptr', 'bond_ptr')):
        out[key] = out[key].copy()
        out[key][:out['n_systems']] -= results[first][m]
    return out


# ---- command line --------------------------------------------------------------------------------------------------------------------

def stats_mols(mols, device=None, mode=0, sys_bins=DEFAULT_BINS, max_nodes=canon.DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS,
               num_bond_types=4):
    """results and keys of a list of molecule dicts in one host dict: on `device`, or with the Python path when it is None"""
    if device is None:
        res = stack_ref(mols, mode, sys_bins, atomic_numbers, num_bond_types)
        return dict(res, **keys_ref(mols, res, max_nodes, atomic_numbers))
    res, cm, full = framework_mols(mols, device, mode, sys_bins, atomic_numbers, num_bond_types, with_cm=True)
    return dict(to_host(res), **keys(cm, full, max_nodes))


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m moldiff_amd.framework', description=__doc__.split('\n\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    s = sub.add_parser('stats', help='frameworks and ring systems of the molecules stored in a samples_all.pt')
    s.add_argument('samples')
    s.add_argument('--out', required=True)
    s.add_argument('--part', default='finished')
    s.add_argument('--exo', action='store_true', help='double-bonded atoms on the core join the framework')
    s.add_argument('--generic', action='store_true', help='every atom as carbon, every bond single')
    s.add_argument('--sys_bins', type=int, default=DEFAULT_BINS)
    s.add_argument('--max_nodes', type=int, default=canon.DEFAULT_MAX_NODES)
    s.add_argument('--device', default='cuda:0')
    s.add_argument('--ref', action='store_true', help='the Python path instead of the device')
    c = sub.add_parser('compare', help='divergences, uniqueness and mutual novelty of two files')
    c.add_argument('a')
    c.add_argument('b')
    args = ap.parse_args(argv)
    if args.cmd == 'stats':
        mols = load_mols(args.samples, args.part)
        mode = (MODE_EXO if args.exo else 0) | (MODE_GENERIC if args.generic else 0)
        device = None
        if not args.ref:
            import torch
            torch.cuda.set_device(torch.device(args.device))
            device = args.device
        res = stats_mols(mols, device, mode, args.sys_bins, args.max_nodes)
        save_npz(res, args.out)
        print(json.dumps(summary(res, device=device), indent=1))
    else:
        print(json.dumps(compare(load_npz(args.a), load_npz(args.b)), indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
