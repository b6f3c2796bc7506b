"""The compact molecule arrays of the evaluation kernels (csrc/mdx_mol.h) on the Python side: a list of molecule dicts parsed and packed
into them, the packed arrays as the operands of a C entry point (``CompactMols``), and the small host helpers the evaluation modules
(local3d, similarity, rings, groups, kekule) share.  Nothing here needs torch at import.

A molecule dict holds ``element`` (atomic numbers), ``bond_index`` (2, 2b) with every bond once and then flipped, ``bond_type`` (2b) and,
for the geometry statistics, ``atom_pos`` (n, 3): what ``FeaturizeMol.decode_batch`` returns and ``samples_all.pt`` stores.
"""
import ctypes
from typing import Any, NamedTuple

import numpy as np

DEFAULT_ATOMIC_NUMBERS = (6, 7, 8, 9, 15, 16, 17)


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
    ptr = lambda c: (np.cumsum(c) - c).astype(np.int32)
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
