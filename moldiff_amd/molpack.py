"""The compact molecule arrays of the evaluation kernels (csrc/mdx_mol.h) on the Python side: a list of molecule dicts parsed and packed
into them, the packed arrays as the operands of a C entry point (``CompactMols``), the results table of the evaluation modules (``Layout``
and the functions over it) and the constants and small host helpers those modules (local3d, similarity, rings, groups, kekule, canon,
framework) share.  Nothing here needs torch at import.

A molecule dict holds ``element`` (atomic numbers), ``bond_index`` (2, 2b) with every bond once and then flipped, ``bond_type`` (2b) and,
for the geometry statistics, ``atom_pos`` (n, 3): what ``FeaturizeMol.decode_batch`` returns and ``samples_all.pt`` stores.
"""
import argparse
import ctypes
import functools
import json
from typing import Any, NamedTuple

import numpy as np

DEFAULT_ATOMIC_NUMBERS = (6, 7, 8, 9, 15, 16, 17)
ELEMENT_SYMBOL = {6: 'C', 7: 'N', 8: 'O', 9: 'F', 15: 'P', 16: 'S', 17: 'Cl'}   # the featuriser's atomic numbers
ELEMENT_NUMBER = {s: z for z, s in ELEMENT_SYMBOL.items()}
# this project's choice, unverified against RDKit: the valence from which implicit hydrogens are counted
DEFAULT_NORMAL_VALENCE = {6: 4, 7: 3, 8: 2, 9: 1, 15: 3, 16: 2, 17: 1}
MAX_STEPS_LIMIT = 1 << 20


class OverBudget(Exception):
    """a search of a ``*_ref`` function went over its step budget"""


def check_steps(max_steps):
    if not 1 <= int(max_steps) <= MAX_STEPS_LIMIT:
        raise ValueError(f'max_steps must lie in 1 .. 2^20, got {max_steps}')
    return int(max_steps)


# ---- host helpers --------------------------------------------------------------------------------------------------------------------

def host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def to_host(results):
    """a results dict with numpy arrays"""
    return {k: np.ascontiguousarray(host(v)) for k, v in results.items()}


def save_npz(results, path):
    with open(path, 'wb') as f:   # a file object: numpy appends no suffix
        np.savez(f, **to_host(results))


def load_npz(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def ptr(counts):
    """where each of consecutive runs of the given lengths starts (int32)"""
    c = np.asarray(counts, dtype=np.int64)
    return (np.cumsum(c) - c).astype(np.int32)


def jsd_counts(p, q):
    """Jensen-Shannon divergence of two count vectors over the same bins: base-2 logarithm, so in [0, 1]; each side is normalised by
    its own sum (scaling a side's counts changes nothing); NaN when either side is empty."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    if p.sum() <= 0 or q.sum() <= 0:
        return float('nan')
    p, q = p / p.sum(), q / q.sum()
    m = 0.5 * (p + q)
    kl = lambda a: float((a[a > 0] * np.log2(a[a > 0] / m[a > 0])).sum())
    return min(1.0, max(0.0, 0.5 * kl(p) + 0.5 * kl(q)))


def load_mols(path, part):
    """the molecule dicts of a ``samples_all.pt`` (its `part`), or of a file that holds a plain list"""
    import torch
    pool = torch.load(path, map_location='cpu', weights_only=False)
    return list(pool[part]) if isinstance(pool, dict) else list(pool)


# ---- parsing and packing -------------------------------------------------------------------------------------------------------------

def mol_graph(info, atomic_numbers=None):
    """One molecule dict -> class index per atom (int64; the atomic numbers themselves when `atomic_numbers` is None) and the bonds
    once each, the flipped half dropped: (2, b) int64 indices, (b) types.  An element outside `atomic_numbers` raises ValueError."""
    ele = np.asarray(info['element'], dtype=np.int64).reshape(-1)
    if 'bond_index' in info and np.asarray(info['bond_index']).size:
        bi = np.asarray(info['bond_index'], dtype=np.int64)
        nb = bi.shape[1] // 2
        bi, bt = bi[:, :nb], np.asarray(info['bond_type'], dtype=np.int64)[:nb]
    else:
        bi, bt = np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64)
    if atomic_numbers is None:
        return ele, bi, bt
    cls = {int(z): i for i, z in enumerate(atomic_numbers)}
    unknown = sorted({int(z) for z in ele if int(z) not in cls})
    if unknown:
        raise ValueError(f'element(s) {unknown} are not among the spec\'s atomic numbers')
    return np.asarray([cls[int(z)] for z in ele], dtype=np.int64), bi, bt


def pack_mols(mols, atomic_numbers, positions=False):
    """a list of molecule dicts as the dense compact arrays (numpy, int32): atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type (class
    index), bond_type, bond_index (2, max(total bonds, 1)) and, with `positions`, atom_pos (float32 (N, 3))"""
    graphs = [mol_graph(m, atomic_numbers) for m in mols]
    na = np.asarray([len(g[0]) for g in graphs], dtype=np.int64)
    nb = np.asarray([g[1].shape[1] for g in graphs], dtype=np.int64)
    cat = lambda xs, empty, axis=0: np.concatenate(xs + [np.zeros(empty, dtype=np.int64)], axis=axis).astype(np.int32)
    bidx = cat([g[1] for g in graphs], (2, 0), 1)
    if bidx.shape[1] == 0:
        bidx = np.zeros((2, 1), dtype=np.int32)
    p = {'atom_ptr': ptr(na), 'bond_ptr': ptr(nb), 'n_atoms': na.astype(np.int32), 'n_bonds': nb.astype(np.int32),
         'atom_type': cat([g[0] for g in graphs], 0)}
    if positions:
        pos = [np.asarray(m['atom_pos'], dtype=np.float32).reshape(n, 3) for m, n in zip(mols, na)]
        p['atom_pos'] = np.concatenate(pos + [np.zeros((0, 3), dtype=np.float32)])
    p.update(bond_type=cat([g[2] for g in graphs], 0), bond_index=np.ascontiguousarray(bidx))
    return p


def check_simple(p):
    """The precondition of rings and groups that the device cannot report: no two bonds between the same pair of atoms, in any molecule
    of the packed arrays `p`, else ValueError.  A bond with an index outside the molecule or with i = j is ignored, as on the device."""
    for m in range(len(p['n_atoms'])):
        b0, nb, n = int(p['bond_ptr'][m]), int(p['n_bonds'][m]), int(p['n_atoms'][m])
        i, j = p['bond_index'][:, b0:b0 + nb].astype(np.int64)
        ok = (i >= 0) & (i < n) & (j >= 0) & (j < n) & (i != j)
        key = np.minimum(i, j)[ok] * max(n, 1) + np.maximum(i, j)[ok]
        if len(np.unique(key)) != len(key):
            raise ValueError(f'molecule {m}: two bonds between the same pair of atoms')


def to_device(p, device):
    """packed arrays as torch tensors on `device`; the entry points index with int32, so 2^31 atoms or bonds raise ValueError"""
    import torch
    if int(p['n_atoms'].sum()) >= (1 << 31) or int(p['n_bonds'].sum()) >= (1 << 31):
        raise ValueError('2^31 atoms or bonds in one call: split the list')
    return {k: torch.from_numpy(v).to(device) for k, v in p.items()}


# ---- the operands of an entry point --------------------------------------------------------------------------------------------------

class CompactMols(NamedTuple):
    """The compact arrays as device tensors (int32, contiguous; atom_pos float32) in the order the C entry points take them.  N_cap and
    Eh_stride are the extents of the atom arrays and of a row of bond_index; molecule m lies at atom_ptr[m] / bond_ptr[m]."""
    B: int
    atom_ptr: Any
    bond_ptr: Any
    n_atoms: Any
    n_bonds: Any
    atom_type: Any
    N_cap: int
    bond_type: Any
    bond_index: Any
    Eh_stride: int
    atom_pos: Any = None

    @classmethod
    def from_packed(cls, d):
        """from ``to_device(pack_mols(...))``: dense, so N_cap is the number of atoms"""
        return cls(len(d['n_atoms']), d['atom_ptr'], d['bond_ptr'], d['n_atoms'], d['n_bonds'], d['atom_type'], int(d['atom_type'].shape[0]),
                   d['bond_type'], d['bond_index'], int(d['bond_index'].shape[1]), d.get('atom_pos'))

    @property
    def device(self):
        return self.n_atoms.device

    def operands(self, positions=False):
        """-> (the leading ctypes operands of an entry point: B .. Eh_stride, atom_pos after atom_type with `positions`; `at`, which
        gives the address of any further tensor).  An empty tensor has no address and a NULL operand is refused: an array nothing
        will be read from or written to is stood in for by 8 spare bytes."""
        import torch
        from . import _lib
        spare = torch.zeros(1, dtype=torch.int64, device=self.device)
        at = lambda t: _lib.ptr(t if t.numel() else spare)
        pos = (at(self.atom_pos),) if positions else ()
        return (self.B, at(self.atom_ptr), at(self.bond_ptr), at(self.n_atoms), at(self.n_bonds), at(self.atom_type)) + pos + (
            self.N_cap, at(self.bond_type), at(self.bond_index), self.Eh_stride), at

    @staticmethod
    def workspace(need, ws, dev):
        """`ws` = (pointer, bytes, ...) when it holds `need` bytes, else a fresh one that carries its buffer: keep it until the launch"""
        if ws is not None and ws[1].value >= need:
            return ws
        import torch
        buf = torch.empty(need, dtype=torch.uint8, device=dev)
        return ctypes.c_void_p(buf.data_ptr()), ctypes.c_size_t(need), buf


# ---- the results table of an evaluation module ----------------------------------------------------------------------------------------

class Layout(NamedTuple):
    """What the results dict of an evaluation module (rings, groups, kekule, canon, framework) holds, said once.  One entry per molecule
    of every key of `mol` (a row of ``widths[k]`` columns for a key of `wide`), int32 but for the keys of `int64`; the keys of `atom`
    over the atoms and of `bond` over the bond slots of the list in turn, molecule m at ``atom_ptr[m]`` / ``bond_ptr[m]``; the keys of
    `index` (2, bonds); the keys of `pos` (atoms, 3) float32, held when every molecule came with positions; the per-atom keys of
    `optional`, held only when their input was given.  `mol` names ``n_atoms``, and ``n_bonds`` unless the table carries none; a table
    with a per-bond key carries ``bond_ptr``.  The dicts are made in the order mol, atom, optional, bond, pos, index, atom_ptr, bond_ptr."""
    mol: tuple
    atom: tuple = ()
    bond: tuple = ()
    index: tuple = ()
    pos: tuple = ()
    optional: tuple = ()
    wide: tuple = ()
    int64: tuple = ()

    @property
    def has_n_bonds(self):
        return 'n_bonds' in self.mol

    @property
    def has_bond_ptr(self):
        return bool(self.bond)

    def columns(self, held=()):
        """the per-atom and per-bond arrays of a table that holds the optional and position keys in `held` (a dict will do) ->
        [(key, counted by 'atom' or 'bond', 'flat' (n) int32 | 'pos' (n, 3) float32 | 'index' (2, n) int32)]"""
        there = lambda keys: tuple(k for k in keys if k in held)
        return ([(k, 'atom', 'flat') for k in self.atom + there(self.optional)] + [(k, 'bond', 'flat') for k in self.bond] +
                [(k, 'atom', 'pos') for k in there(self.pos)] + [(k, 'bond', 'index') for k in self.index])

    def mol_shape(self, k, B, widths):
        return (B, widths[k]) if k in self.wide else (B,)


_SHAPE = {'flat': lambda n: (n,), 'pos': lambda n: (n, 3), 'index': lambda n: (2, n)}


def _cut(x, kind, lo, hi):
    return x[:, lo:hi] if kind == 'index' else x[lo:hi]


def _pointers(out, layout, n_bonds=None):
    out['atom_ptr'] = ptr(out['n_atoms'])
    if layout.has_bond_ptr:
        out['bond_ptr'] = ptr(out['n_bonds'] if layout.has_n_bonds else n_bonds)
    return out


def stack(refs, layout, widths=None, optional=()):
    """The dicts a ``*_ref`` function returned for the molecules of a list, as one host results dict (numpy).  widths: the column count of
    every key of ``layout.wide``; optional: the optional keys the refs hold.  A position key is held when every ref holds it."""
    out = {k: np.asarray([r[k] for r in refs], dtype=np.int64 if k in layout.int64 else np.int32).reshape(layout.mol_shape(k, len(refs), widths))
           for k in layout.mol}
    held = tuple(optional) + tuple(k for k in layout.pos if all(k in r for r in refs))
    for k, _, kind in layout.columns(held):
        dtype = np.float32 if kind == 'pos' else np.int32
        out[k] = np.concatenate([r[k] for r in refs] + [np.zeros(_SHAPE[kind](0), dtype=dtype)], axis=int(kind == 'index')).astype(dtype)
    return _pointers(out, layout, None if layout.has_n_bonds or not layout.has_bond_ptr else [len(r[layout.bond[0]]) for r in refs])


def concat(parts, layout):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict; the optional and position keys are
    those of the first part, and a later part without one raises KeyError"""
    parts = [to_host(p) for p in parts]
    out = {k: np.concatenate([p[k] for p in parts]) for k in layout.mol}
    out.update({k: np.concatenate([p[k] for p in parts], axis=int(kind == 'index')) for k, _, kind in layout.columns(parts[0])})
    if layout.has_n_bonds or not layout.has_bond_ptr:
        return _pointers(out, layout)
    # without n_bonds the bond counts are the steps of every part's bond_ptr, the last one up to the end of its arrays
    return _pointers(out, layout, np.concatenate([np.diff(np.append(p['bond_ptr'].astype(np.int64), len(p[layout.bond[0]]))) for p in parts]))


def mol_slice(results, m, layout):
    """molecule `m` of a results dict with host arrays as the dict the ``*_ref`` function returns: ints, the row of a wide key, and
    views of the per-atom and per-bond arrays"""
    out = {k: results[k][m] if k in layout.wide else int(results[k][m]) for k in layout.mol}
    lo = {'atom': int(results['atom_ptr'][m])}
    hi = {'atom': lo['atom'] + out['n_atoms']}
    if layout.has_bond_ptr:
        nxt = results['bond_ptr'][m + 1] if m + 1 < len(results['bond_ptr']) else len(results[layout.bond[0]])
        lo['bond'] = int(results['bond_ptr'][m])
        hi['bond'] = lo['bond'] + out['n_bonds'] if layout.has_n_bonds else int(nxt)
    out.update({k: _cut(results[k], kind, lo[per], hi[per]) for k, per, kind in layout.columns(results)})
    return out


def packed(mols, atomic_numbers, device, positions=None, simple=True):
    """The prologue of every ``<name>_mols``: a list of molecule dicts packed densely and copied to `device` -> (the packed numpy arrays,
    their ``CompactMols``).  With `positions` the positions travel too, if every molecule has them and the list is not empty; with
    `simple`, two bonds between one pair of atoms raise ValueError (``check_simple``)."""
    import torch
    device = torch.device(device)
    p = pack_mols(mols, atomic_numbers, positions=bool(positions) and len(mols) > 0 and all('atom_pos' in m for m in mols))
    if simple:
        check_simple(p)
    return p, CompactMols.from_packed(to_device(p, device))


@functools.lru_cache(maxsize=None)
def _outputs(layout, stat_keys, held):
    """what ``zeros_for`` allocates: ((key, which of its five shapes or None for a wide key, torch dtype)) -- worked out once per layout,
    because a ``launch`` takes tens of microseconds on the host and this runs in every one"""
    import torch
    shape = {('atom', 'flat'): 1, ('bond', 'flat'): 2, ('atom', 'pos'): 3, ('bond', 'index'): 4}
    mol = [(k, None if k in layout.wide else 0, torch.int64 if k in layout.int64 else torch.int32)
           for k in layout.mol if k not in stat_keys and k not in ('n_atoms', 'n_bonds')]
    return tuple(mol + [(k, shape[per, kind], torch.float32 if kind == 'pos' else torch.int32) for k, per, kind in layout.columns(held)])


def zeros_for(cm, layout, widths=None, stat_keys=(), held=()):
    """The output tensors of a ``launch`` on `cm`, zeroed -> (dict, stats).  The `stat_keys` are the columns of the one
    (B, len(stat_keys)) int32 table `stats` (None without them; ``split_stats``); every other key of ``layout.mol`` but n_atoms and
    n_bonds gets a tensor of its own, and so does every per-atom (max(N_cap, 1) long) and per-bond (max(Eh_stride, 1)) key, the
    optional and position keys when `held` (a tuple, like `stat_keys`) names them.  No tensor is empty unless B is 0."""
    import torch
    B, N, E, dev = cm.B, max(cm.N_cap, 1), max(cm.Eh_stride, 1), cm.device
    shapes = ((B,), (N,), (E,), (N, 3), (2, E))
    out = {k: torch.zeros(*((B, widths[k]) if s is None else shapes[s]), dtype=dtype, device=dev)
           for k, s, dtype in _outputs(layout, stat_keys, held)}
    return out, (torch.zeros(B, len(stat_keys), dtype=torch.int32, device=dev) if stat_keys else None)


def split_stats(out, stats, stat_keys):
    """the columns of the per-molecule table of a ``launch`` as the keys they are"""
    out.update({k: stats[:, c] for c, k in enumerate(stat_keys)})
    return out


def attach(out, cm, select, n_atoms, layout):
    """The epilogue of every ``FeaturizeMol.<name>_batch``: the counts and pointers of `cm` join the tensors of ``launch``.  n_atoms:
    the atom counts with 0 where `select` leaves a molecule out; n_bonds is zeroed there too."""
    import torch
    out['n_atoms'] = n_atoms
    if layout.has_n_bonds:
        n_bonds = cm.n_bonds[:cm.B]
        out['n_bonds'] = n_bonds if select is None else torch.where(select != 0, n_bonds, torch.zeros_like(n_bonds))
    out['atom_ptr'] = cm.atom_ptr
    if layout.has_bond_ptr:
        out['bond_ptr'] = cm.bond_ptr
    return out


def dense(out, cm, p, layout):
    """The epilogue of every ``<name>_mols``: the tensors of ``launch`` on the packed list `p` / `cm`, cut to the atoms and bonds there
    are, with the counts and pointers -> the results dict of ``stack`` with device tensors.  The empty list holds positions, as there."""
    import torch
    n = {'atom': cm.N_cap, 'bond': int(p['n_bonds'].sum())}
    out.update({k: _cut(out[k], kind, 0, n[per]) for k, per, kind in layout.columns(out)})
    if cm.B == 0:
        out.update({k: torch.zeros(0, 3, dtype=torch.float32, device=cm.device) for k in layout.pos})
    return attach(out, cm, None, cm.n_atoms, layout)


def on_device(host_results, device, keep=()):
    """a host results dict as tensors on `device`; the keys of `keep` stay numpy"""
    import torch
    return {k: v if k in keep else torch.from_numpy(v).to(device) for k, v in host_results.items()}


def stats_main(argv, name, doc, helps, options, run, summary, compare, extra=()):
    """The ``stats`` / ``compare`` command line of an evaluation module `name` with docstring `doc`.  helps: the help lines of the two
    commands; options: [(flag, add_argument keywords)] of ``stats`` beside samples, --out, --part, --device and --ref;
    run(mols, args, device) -> a results dict, device None for the Python path.  ``stats`` writes the results to --out and prints
    their summary; ``compare`` prints ``compare`` of two such files.  extra: further commands of the module as (name, help line,
    add_arguments(parser), run(args))."""
    ap = argparse.ArgumentParser(prog='python -m moldiff_amd.' + name, description=doc.split('\n\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    s = sub.add_parser('stats', help=helps[0])
    s.add_argument('samples')
    s.add_argument('--out', required=True)
    s.add_argument('--part', default='finished')
    for flag, kw in options:
        s.add_argument(flag, **kw)
    s.add_argument('--device', default='cuda:0')
    s.add_argument('--ref', action='store_true', help='the Python path instead of the device')
    c = sub.add_parser('compare', help=helps[1])
    c.add_argument('a')
    c.add_argument('b')
    for cmd, text, add, _ in extra:
        add(sub.add_parser(cmd, help=text))
    args = ap.parse_args(argv)
    for cmd, _, _, handler in extra:
        if args.cmd == cmd:
            handler(args)
            return 0
    if args.cmd == 'stats':
        mols = load_mols(args.samples, args.part)
        if not args.ref:
            import torch
            torch.cuda.set_device(torch.device(args.device))
        res = run(mols, args, None if args.ref else args.device)
        save_npz(res, args.out)
        print(json.dumps(summary(res), indent=1))
    else:
        print(json.dumps(compare(load_npz(args.a), load_npz(args.b)), indent=1))
    return 0
