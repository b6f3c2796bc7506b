"""Scaffold-constrained sampling: the known part of a molecule that the reverse chain holds fixed.

An addition beyond the reference (it has no conditional sampling): replacement conditioning as in RePaint / DiffSBDD, without
their resampling loop.  After every reverse step the fixed rows of the state are overwritten with a draw from q(x_k | x_0) of the
known molecule (``mdx_scaffold_merge``, one launch); the free rows are generated around them.  ``Scaffold`` only carries and
validates the known values; the sampler (``model._Sampler``) owns the chain.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch


@dataclass
class Scaffold:
    """Known atoms / bonds of a packed batch; every field lives on the batch's device.

    node_mask      (N) bool      atoms held fixed
    node_type      (N) int64     class ids
    node_pos       (N,3) float32 coordinates
    halfedge_type  (Eh) int64    class ids of the known half-edges (0 = "no bond")
    halfedge_mask  (Eh) bool     optional; default: a half-edge is fixed exactly when both its atoms are

    Values on free rows are ignored unless the chain is started part-way (``start_step``): then the scaffold carries the whole
    start molecule and the masks say which rows stay fixed afterwards."""
    node_mask: torch.Tensor
    node_type: torch.Tensor
    node_pos: torch.Tensor
    halfedge_type: torch.Tensor
    halfedge_mask: Optional[torch.Tensor] = None

    def resolve(self, n_nodes, halfedge_index, num_node_types, num_edge_types, every_row=False):
        """Validate against a packed batch and return contiguous (node_mask, node_type, node_pos, halfedge_type, halfedge_mask).
        Shapes, dtypes and device raise TypeError / ValueError without touching the data; the value checks -- every fixed class id
        (every id when `every_row`) in [0, K), no fixed half-edge with a free end point -- cost ONE host read."""
        N, Eh, dev = int(n_nodes), int(halfedge_index.shape[1]), halfedge_index.device
        hm = self.halfedge_mask
        want = (('node_mask', self.node_mask, (N,), torch.bool), ('node_type', self.node_type, (N,), torch.int64),
                ('node_pos', self.node_pos, (N, 3), torch.float32), ('halfedge_type', self.halfedge_type, (Eh,), torch.int64),
                ('halfedge_mask', hm, (Eh,), torch.bool))
        for name, t, shape, dtype in want:
            if t is None and name == 'halfedge_mask':
                continue
            if not isinstance(t, torch.Tensor):
                raise TypeError(f'scaffold.{name} must be a tensor')
            if tuple(t.shape) != shape:
                raise ValueError(f'scaffold.{name} has shape {tuple(t.shape)}, the batch needs {shape}')
            if t.dtype != dtype:
                raise TypeError(f'scaffold.{name} must be {dtype} (got {t.dtype})')
            if t.device != dev:
                raise ValueError(f'scaffold.{name} is on {t.device}, the batch on {dev}')
        nm = self.node_mask.contiguous()
        both = nm[halfedge_index[0]] & nm[halfedge_index[1]]
        hm = both if hm is None else hm.contiguous()
        nt, ht = self.node_type.contiguous(), self.halfedge_type.contiguous()
        bad_n = (nt < 0) | (nt >= num_node_types)
        bad_h = (ht < 0) | (ht >= num_edge_types)
        if not every_row:
            bad_n, bad_h = bad_n & nm, bad_h & hm
        flags = torch.stack([bad_n.any(), bad_h.any(), (hm & ~both).any()]).tolist()   # the one host read
        if flags[0]:
            raise ValueError(f'scaffold.node_type: class id outside [0, {num_node_types}) on a fixed atom')
        if flags[1]:
            raise ValueError(f'scaffold.halfedge_type: class id outside [0, {num_edge_types}) on a fixed half-edge')
        if flags[2]:
            raise ValueError('scaffold.halfedge_mask fixes a half-edge that has a free end point')
        return nm, nt, self.node_pos.contiguous(), ht, hm


def scaffold_for_sizes(info, sizes, featurizer, device=None):
    """The same scaffold at the front of every molecule of a packed batch (``harness.placeholder_from_sizes`` layout).

    info: dict(element, atom_pos, bond_index, bond_type) as ``sample_drug3d.read_mol_block`` returns it; sizes: atoms per molecule,
    each >= the scaffold's K atoms.  Molecule m's first K atoms are the scaffold; the bonds among them are fixed, "no bond"
    included; the remaining atoms and every half-edge that touches them are free.  Elements map to classes through the
    featurizer's atomic-number list (an element it does not know raises), bond orders 1..num_bond_types to their class ids.

    Coordinates are shifted so that the SCAFFOLD's centroid is at the origin.  Training molecules are centred on their full
    centroid, which for a grown molecule is not known in advance: this is an approximation, good when the scaffold is most of the
    molecule or the growth is roughly symmetric around it."""
    ele = np.asarray(info['element']).astype(np.int64)
    K = int(ele.shape[0])
    sizes = np.asarray(sizes, dtype=np.int64)
    if K == 0 or (sizes < K).any():
        raise ValueError(f'every molecule needs at least the scaffold\'s {K} atoms (and the scaffold at least one)')
    unknown = sorted({int(e) for e in ele if int(e) not in featurizer.ele_to_nodetype})
    if unknown:
        raise ValueError(f'scaffold elements {unknown} are not in the featurizer\'s list {featurizer.atomic_numbers.tolist()}')
    cls = np.array([featurizer.ele_to_nodetype[int(e)] for e in ele], dtype=np.int64)
    pos = np.asarray(info['atom_pos'], dtype=np.float64).reshape(K, 3)
    pos = (pos - pos.mean(axis=0, keepdims=True)).astype(np.float32)
    nb = np.asarray(info['bond_index']).shape[1] // 2
    bi, bt = np.asarray(info['bond_index'])[:, :nb].astype(np.int64), np.asarray(info['bond_type'])[:nb].astype(np.int64)
    if nb and (bi.min() < 0 or bi.max() >= K or (bi[0] == bi[1]).any()):
        raise ValueError('scaffold bond refers to an atom outside the scaffold')
    if nb and (bt.min() < 1 or bt.max() > featurizer.num_bond_types):
        raise ValueError(f'scaffold bond order outside 1..{featurizer.num_bond_types}')
    lo, hi = np.minimum(bi[0], bi[1]), np.maximum(bi[0], bi[1])
    node_off = np.concatenate([[0], np.cumsum(sizes)])
    half_off = np.concatenate([[0], np.cumsum(sizes * (sizes - 1) // 2)])
    N, Eh = int(node_off[-1]), int(half_off[-1])
    node_mask, node_type, node_pos = np.zeros(N, dtype=bool), np.zeros(N, dtype=np.int64), np.zeros((N, 3), dtype=np.float32)
    half_type = np.zeros(Eh, dtype=np.int64)
    for m, n in enumerate(sizes):
        a = int(node_off[m])
        node_mask[a:a + K], node_type[a:a + K], node_pos[a:a + K] = True, cls, pos
        # half-edge (i, j), i < j, of an n-atom molecule sits at i n - i (i + 1) / 2 + (j - i - 1) of its row-major upper triangle
        half_type[half_off[m] + lo * n - lo * (lo + 1) // 2 + (hi - lo - 1)] = bt
    t = lambda x: torch.from_numpy(x) if device is None else torch.from_numpy(x).to(device)
    return Scaffold(t(node_mask), t(node_type), t(node_pos), t(half_type))
