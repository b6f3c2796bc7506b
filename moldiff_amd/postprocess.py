"""Harness consumers of the sampling path's outputs.

* ``FeaturizeMol`` -- constructor + ``decode_output`` with the reference's signature (utils/transforms.py:13-31,
  :65-122).  The reference runs this per molecule on the host in numpy after a full D2H copy; the same host form
  is kept for drop-in use, and ``decode_batch`` is the accelerated path: one pair of HIP kernels
  (``mdx_decode_output``) arg-maxes, drops mask-type atoms, re-indexes and compacts atoms/bonds for the whole
  packed batch on the device, so only the compact arrays travel.
* ``seperate_outputs`` / ``seperate_outputs_no_traj`` -- utils/sample.py:4-55 (same spelling as the reference).
``FeaturizeMol.__call__`` (training-side featurisation of a processed record) lives in ``moldiff_amd/data.py``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .molcheck import fragment_fraction, valence_table
from .molpack import attach, CompactMols, on_device


def _softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


class FeaturizeMol(object):
    def __init__(self, atomic_numbers, mol_bond_types, use_mask_node, use_mask_edge):
        self.atomic_numbers = torch.LongTensor(atomic_numbers)
        self.mol_bond_types = torch.LongTensor(mol_bond_types)
        self.num_element = self.atomic_numbers.size(0)
        self.num_bond_types = self.mol_bond_types.size(0)
        self.num_node_types = self.num_element + int(use_mask_node)
        self.num_edge_types = self.num_bond_types + 1 + int(use_mask_edge)  # +1: the non-bonded class
        self.use_mask_node, self.use_mask_edge = use_mask_node, use_mask_edge
        self.ele_to_nodetype = {ele: i for i, ele in enumerate(atomic_numbers)}
        self.nodetype_to_ele = {i: ele for i, ele in enumerate(atomic_numbers)}

    follow_batch = ['node_type', 'halfedge_type']

    def __call__(self, data):
        """Training-side featurisation of one processed record (utils/transforms.py:35-62): see ``moldiff_amd.data.featurize``."""
        from .data import featurize
        return featurize(data, self)

    def decode_output(self, pred_node, pred_pos, pred_halfedge, halfedge_index):
        """One molecule, numpy arrays in, dict out (element, atom_pos, bond_type, bond_index, atom_prob, bond_prob)."""
        pa = _softmax(pred_node)
        atom_type, atom_prob = np.argmax(pa, axis=-1), np.max(pa, axis=-1)
        keep = atom_type < self.num_element
        renum = -np.ones(len(keep), dtype=np.int64)
        renum[keep] = np.arange(keep.sum())
        out = {'element': np.array([self.nodetype_to_ele[i] for i in atom_type[keep]]),
               'atom_pos': pred_pos[keep], 'atom_prob': atom_prob[keep]}
        if self.num_edge_types == 1:
            return out
        ph = _softmax(pred_halfedge)
        edge_type, edge_prob = np.argmax(ph, axis=-1), np.max(ph, axis=-1)
        is_bond = (edge_type > 0) & (edge_type <= self.num_bond_types)
        bond_type, bond_prob, bond_index = edge_type[is_bond], edge_prob[is_bond], halfedge_index[:, is_bond]
        if not keep.all():
            bond_index = renum[bond_index]
            ok = ~(bond_index < 0).any(axis=0)
            bond_index, bond_type, bond_prob = bond_index[:, ok], bond_type[ok], bond_prob[ok]
        out.update(bond_type=np.concatenate([bond_type, bond_type]), bond_prob=np.concatenate([bond_prob, bond_prob]),
                   bond_index=np.concatenate([bond_index, bond_index[::-1]], axis=1))
        return out

    def _decode_device(self, pred, batch_node, halfedge_index, n_graphs, graph):
        """Launch ``mdx_decode_output`` -> (graph, dict of the compact device tensors); no copy, no sync."""
        pn, pp, ph = (_lib.f32c(t) for t in pred)
        _lib._need_gpu(pn, pp, ph, batch_node, halfedge_index)
        dev = pn.device
        if graph is None:
            graph = _lib.graph_for_halfedges(halfedge_index, batch_node, n_graphs)
        N, Eh, B = graph.N, graph.Eh, graph.B
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        atom_type, atom_prob, atom_pos = torch.empty(N, **i32), torch.empty(N, **f32), torch.empty(N, 3, **f32)
        bond_type, bond_prob, bond_index = torch.empty(Eh, **i32), torch.empty(Eh, **f32), torch.empty(2, max(Eh, 1), **i32)
        n_atoms, n_bonds = torch.empty(max(B, 1), **i32), torch.empty(max(B, 1), **i32)
        ws, nb = graph.workspace(dev)
        _lib.check(_lib.lib().mdx_decode_output(
            graph.h, _lib.ptr(pn), pn.shape[1], _lib.ptr(pp), _lib.ptr(ph), ph.shape[1], self.num_element,
            self.num_bond_types, _lib.ptr(atom_type), _lib.ptr(atom_prob), _lib.ptr(atom_pos), _lib.ptr(n_atoms),
            _lib.ptr(bond_type), _lib.ptr(bond_prob), _lib.ptr(bond_index), _lib.ptr(n_bonds), ws, nb, _lib.stream()))
        return graph, dict(atom_type=atom_type, atom_prob=atom_prob, atom_pos=atom_pos, n_atoms=n_atoms, bond_type=bond_type,
                           bond_prob=bond_prob, bond_index=bond_index, n_bonds=n_bonds)

    def _slice_mols(self, d, batch_node, batch_halfedge, B):
        """Copy the compact arrays to the host and slice them per molecule -> (list of dicts, node_ptr, n_atoms)."""
        at, ap, apos = d['atom_type'].cpu().numpy(), d['atom_prob'].cpu().numpy(), d['atom_pos'].cpu().numpy()
        bt, bp, bi = d['bond_type'].cpu().numpy(), d['bond_prob'].cpu().numpy(), d['bond_index'].cpu().numpy()
        na, nbd = d['n_atoms'].cpu().numpy(), d['n_bonds'].cpu().numpy()
        node_ptr = np.concatenate([[0], np.cumsum(np.bincount(batch_node.cpu().numpy(), minlength=B))])
        he_ptr = np.concatenate([[0], np.cumsum(np.bincount(batch_halfedge.cpu().numpy(), minlength=B))])
        ele = np.asarray(self.atomic_numbers.numpy())
        out = []
        for m in range(B):
            a0, a1 = node_ptr[m], node_ptr[m] + na[m]
            b0, b1 = he_ptr[m], he_ptr[m] + nbd[m]
            idx = bi[:, b0:b1].astype(np.int64)
            out.append({'element': ele[at[a0:a1]], 'atom_pos': apos[a0:a1], 'atom_prob': ap[a0:a1],
                        'bond_type': np.concatenate([bt[b0:b1], bt[b0:b1]]).astype(np.int64),
                        'bond_prob': np.concatenate([bp[b0:b1], bp[b0:b1]]),
                        'bond_index': np.concatenate([idx, idx[::-1]], axis=1)})
        return out, node_ptr, na

    def decode_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph=None):
        """Whole packed batch on the device -> list of per-molecule dicts identical to
        [decode_output(*seperate_outputs(...)[i]) for i in range(n_graphs)].
        pred = [pred_node (N,Kn), pred_pos (N,3), pred_halfedge (Eh,Ke)] device tensors (model.sample()['pred'])."""
        graph, d = self._decode_device(pred, batch_node, halfedge_index, n_graphs, graph)
        return self._slice_mols(d, batch_node, batch_halfedge, graph.B)[0]

    def _check_device(self, graph, d, max_valence=None, largest_fragment=None):
        """The device part of ``check_batch`` on the compact tensors `d` of ``_decode_device``: ``mdx_mol_check``, and with
        `largest_fragment` the selection (device integer arithmetic, no host sync) + ``mdx_mol_keep_component``, which rewrites `d`
        in place.  -> (ri (6,B) int32: n_components, largest_size, largest_label, n_overvalent, n_atoms as decoded,
        salvaged; rf (2,B) float32: min_dist, max_bond_len; pa (2,N) int32: component, valence2)."""
        dev = d['atom_type'].device
        N, B = graph.N, graph.B
        key = (str(dev), tuple(valence_table(self.atomic_numbers.tolist(), max_valence)))
        if getattr(self, '_mv_key', None) != key:
            self._mv, self._mv_key = torch.tensor(key[1], dtype=torch.int32, device=dev), key
        ri = torch.zeros(6, max(B, 1), dtype=torch.int32, device=dev)
        rf = torch.empty(2, max(B, 1), dtype=torch.float32, device=dev)
        pa = torch.empty(2, max(N, 1), dtype=torch.int32, device=dev)
        ws, nb = graph.workspace(dev)
        _lib.check(_lib.lib().mdx_mol_check(
            graph.h, _lib.ptr(d['atom_type']), _lib.ptr(d['atom_pos']), _lib.ptr(d['n_atoms']), _lib.ptr(d['bond_type']),
            _lib.ptr(d['bond_index']), _lib.ptr(d['n_bonds']), self.num_element, self.num_bond_types, _lib.ptr(self._mv),
            _lib.ptr(pa[0]), _lib.ptr(pa[1]), _lib.ptr(ri[0]), _lib.ptr(ri[1]), _lib.ptr(ri[2]), _lib.ptr(ri[3]), _lib.ptr(rf[0]),
            _lib.ptr(rf[1]), ws, nb, _lib.stream()))
        ri[4].copy_(d['n_atoms'])
        if largest_fragment is not None:
            p, q = fragment_fraction(largest_fragment)
            # more than one fragment, and largest_size / n_atoms >= p / q in int64
            ri[5] = ((ri[0] > 1) & (ri[1].long() * q >= ri[4].long() * p)).to(torch.int32)
            _lib.check(_lib.lib().mdx_mol_keep_component(
                graph.h, _lib.ptr(ri[5]), _lib.ptr(ri[2]), _lib.ptr(pa[0]), _lib.ptr(d['atom_type']), _lib.ptr(d['atom_prob']),
                _lib.ptr(d['atom_pos']), _lib.ptr(d['n_atoms']), _lib.ptr(d['bond_type']), _lib.ptr(d['bond_prob']),
                _lib.ptr(d['bond_index']), _lib.ptr(d['n_bonds']), ws, nb, _lib.stream()))
        return ri, rf, pa

    def check_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph=None, *, max_valence=None,
                    largest_fragment=None):
        """``decode_batch`` + the quality check of every molecule on the device (``mdx_mol_check``) -> (mols, report).
        mols: as from decode_batch, plus per atom ``component`` (index of the smallest atom of the atom's fragment) and ``valence``
        (float, bond-order sum; aromatic bonds count 1.5).  report: numpy arrays of length n_graphs -- n_components, largest_size,
        largest_label, n_overvalent, min_dist, max_bond_len, n_atoms, salvaged -- that always describe the molecule AS DECODED.
        max_valence: dict atomic number -> largest permitted valence (None = molcheck.DEFAULT_MAX_VALENCE, unchecked against RDKit).
        largest_fragment = f in (0, 1]: a molecule with more than one fragment whose largest fragment holds at least f * n_atoms
        atoms is restricted to that fragment on the device (``mdx_mol_keep_component``): mols[m] is then the fragment (its atoms'
        valences are those they had in the whole molecule) and report['salvaged'][m] is True.
        The valence rule is a necessary condition of the reference's RDKit sanitisation only: see moldiff_amd/molcheck.py."""
        graph, d = self._decode_device(pred, batch_node, halfedge_index, n_graphs, graph)
        ri, rf, pa = self._check_device(graph, d, max_valence, largest_fragment)
        B = graph.B
        mols, node_ptr, na = self._slice_mols(d, batch_node, batch_halfedge, B)
        ri, rf, pa = ri.cpu().numpy(), rf.cpu().numpy(), pa.cpu().numpy()
        report = {'n_components': ri[0, :B], 'largest_size': ri[1, :B], 'largest_label': ri[2, :B], 'n_overvalent': ri[3, :B],
                  'min_dist': rf[0, :B], 'max_bond_len': rf[1, :B], 'n_atoms': ri[4, :B], 'salvaged': ri[5, :B] != 0}
        for m in range(B):
            a0 = node_ptr[m]
            comp, val = pa[0, a0:a0 + ri[4, m]].astype(np.int64), pa[1, a0:a0 + ri[4, m]] / 2.0
            if ri[5, m]:   # the fragment's atoms in their new numbering: its smallest atom is atom 0
                keep = comp == ri[2, m]
                comp, val = np.zeros(int(keep.sum()), dtype=np.int64), val[keep]
            mols[m]['component'], mols[m]['valence'] = comp, val
        return mols, report

    def local3d_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, spec, graph=None, *, select=None, out=None):
        """``decode_batch``'s device part + the local 3D geometry statistics of every decoded molecule (``mdx_mol_local3d``): bond
        lengths, bond angles and dihedral angles histogrammed per pattern of `spec` (a ``local3d.Local3DSpec``).  Nothing is copied
        to the host and nothing synchronises.  select: (n_graphs) device tensor, molecules with 0 are left out; out: a
        ``Local3DStats`` with device arrays (``local3d.device_stats``) to add into.  -> Local3DStats with device arrays.
        These are the molecules AS DECODED, not RDKit's reconstruction of them: see moldiff_amd/local3d.py.  Like ``decode_batch``,
        it needs a batch with at least one half-edge (``mdx_decode_output`` refuses an empty prediction array)."""
        from . import local3d
        self._same_featuriser(spec, 'the spec was')
        cm, graph, select, _ = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        if out is None:
            out = local3d.device_stats(spec, cm.device)
        elif out.spec != spec:
            raise ValueError('`out` was made for another spec')
        if cm.B == 0:
            return out
        return local3d.launch(cm, spec, out, select=select, ws=graph.workspace(cm.device))

    def _same_featuriser(self, made, what):
        """`made` (anything with atomic_numbers and num_bond_types: a spec, a pattern set, tables) was made for this featuriser"""
        if tuple(made.atomic_numbers) != tuple(self.atomic_numbers.tolist()) or made.num_bond_types != self.num_bond_types:
            raise ValueError(f'{what} made for another featuriser (atomic_numbers / num_bond_types differ)')

    def _compact_mols(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select):
        """The prologue of the ``*_batch`` methods below: ``mdx_decode_output``, then its compact tensors as the operands of an
        evaluation entry point -> (cm: a ``molpack.CompactMols``; the graph; `select` as int32 on the device, or None; n_atoms (B) with
        0 for a molecule `select` leaves out)."""
        graph, d = self._decode_device(pred, batch_node, halfedge_index, n_graphs, graph)
        dev = d['atom_type'].device
        ptrs = self._mol_ptrs(graph, batch_node, batch_halfedge, dev)
        n_atoms = d['n_atoms'][:graph.B]
        if select is not None:
            select = select.to(dev, torch.int32).contiguous()
            n_atoms = torch.where(select != 0, n_atoms, torch.zeros_like(n_atoms))
        cm = CompactMols(graph.B, ptrs[0], ptrs[1], d['n_atoms'], d['n_bonds'], d['atom_type'], max(graph.N, 1), d['bond_type'],
                         d['bond_index'], int(d['bond_index'].shape[1]), d['atom_pos'])
        return cm, graph, select, n_atoms

    @staticmethod
    def _mol_ptrs(graph, batch_node, batch_halfedge, dev):
        """(2, B) int32 on the device, kept with the graph: the first atom / first half-edge of every molecule, formed on the device"""
        ptrs = getattr(graph, '_mol_ptr', None)
        if ptrs is None or ptrs.device != dev:
            cnt = torch.zeros(2, graph.B, dtype=torch.int64, device=dev)
            cnt[0].scatter_add_(0, batch_node.to(dev, torch.int64), torch.ones(graph.N, dtype=torch.int64, device=dev))
            cnt[1].scatter_add_(0, batch_halfedge.to(dev, torch.int64), torch.ones(graph.Eh, dtype=torch.int64, device=dev))
            ptrs = graph._mol_ptr = (cnt.cumsum(1) - cnt).to(torch.int32).contiguous()
        return ptrs

    def fingerprint_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, spec, graph=None, *, select=None):
        """``decode_batch``'s device part + the fingerprint and key of every decoded molecule (``mdx_mol_fingerprint``) for the
        set-level numbers of ``moldiff_amd/similarity.py``; `spec` is a ``similarity.FingerprintSpec``.  Nothing is copied to the host
        and nothing synchronises.  select: (n_graphs) device tensor; a molecule with 0 keeps its place with a zero row, key 0 and
        n_atoms 0.  -> FingerprintSet with device tensors, one entry per molecule of the batch.
        These are the molecules AS DECODED; the fingerprint is this project's, not RDKit's.  Like ``decode_batch``, it needs a batch
        with at least one half-edge."""
        from . import similarity
        self._same_featuriser(spec, 'the spec was')
        cm, graph, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        if cm.B == 0:
            return similarity.FingerprintSet.empty(spec).to(cm.device)
        bits, n_on, key = similarity.launch(cm, spec, select=select, ws=graph.workspace(cm.device))
        return similarity.FingerprintSet(spec, bits, n_on, key, n_atoms)

    def rings_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph=None, *, ring_bins=7, select=None):
        """``decode_batch``'s device part + the ring and composition counts of every decoded molecule (``mdx_mol_rings``; see
        ``moldiff_amd/rings.py``).  Nothing is copied to the host and nothing synchronises.  select: (n_graphs) device tensor; a
        molecule with 0 keeps its place with status 0, n_atoms 0 and every count 0.  -> results dict of int32 device tensors, one entry
        (or row) per molecule of the batch: status, n_atoms, n_rings, ring_hist, n_ring_atoms, n_ring_bonds, n_rotatable, elem_count,
        bond_count; bond_ring_min / atom_ring_min in the decode's own layout, molecule m at bond_ptr[m] / atom_ptr[m].
        These are the molecules AS DECODED; the ring sizes are those of a minimum cycle basis, not RDKit's SSSR.  Like
        ``decode_batch``, it needs a batch with at least one half-edge."""
        from . import rings
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        if cm.B == 0:
            return on_device(rings.empty(self.num_bond_types, self.atomic_numbers.tolist(), ring_bins), cm.device)
        return attach(rings.launch(cm, self.num_element, self.num_bond_types, ring_bins, select=select), cm, select, n_atoms, rings.LAYOUT)

    def groups_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, patterns, graph=None, *, select=None,
                     max_steps=None, normal_valence=None):
        """``decode_batch``'s device part + the pattern counts of every decoded molecule (``mdx_mol_groups``, after ``mdx_mol_rings``
        when a pattern carries a ring constraint; see ``moldiff_amd/groups.py``).  patterns: a ``groups.PatternSet`` made for this
        featuriser.  Nothing is copied to the host and nothing synchronises.  select: (n_graphs) device tensor; a molecule with 0
        keeps its place with status 0, n_atoms 0 and every count 0.  -> results dict: int32 device tensors status, n_atoms (B),
        n_embed, n_anchor, steps, pat_status (B, P), atom_hit in the decode's own layout, molecule m at atom_ptr[m]; the set's
        ``aut`` / ``names`` as numpy.  These are the molecules AS DECODED; the pattern language is this project's, not SMARTS.  Like
        ``decode_batch``, it needs a batch with at least one half-edge."""
        from . import groups
        self._same_featuriser(patterns, 'the pattern set was')
        max_steps = groups.DEFAULT_MAX_STEPS if max_steps is None else max_steps
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        if cm.B == 0:
            return on_device(groups.empty(patterns), cm.device, keep=groups.SET_KEYS)
        out = attach(groups.launch(cm, patterns, normal_valence, max_steps, select=select), cm, select, n_atoms, groups.LAYOUT)
        out.update(aut=patterns.automorphisms(), names=np.asarray(patterns.names, dtype=str))
        return out

    def kekulize_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, tables=None, graph=None, *, select=None,
                       max_steps=None):
        """``decode_batch``'s device part + the Kekulé assignment of every decoded molecule (``mdx_mol_kekulize``; see
        ``moldiff_amd/kekule.py``).  tables: a ``kekule.KekuleTables`` made for this featuriser (None = the defaults).  Nothing is
        copied to the host and nothing synchronises.  select: (n_graphs) device tensor; a molecule with 0 keeps its place with status
        0, n_atoms 0 and every output 0.  -> results dict of int32 device tensors: the per-molecule numbers of ``kekule.STAT_KEYS`` and
        n_atoms, n_bonds (B); val, charge, kek_h, atom_flag and kek_order in the decode's own layout, molecule m at atom_ptr[m] /
        bond_ptr[m].  These are the molecules AS DECODED; the rule is this project's model with default tables unverified against
        RDKit, and the structure is the first found in search order, not a charge-minimal one.  Like ``decode_batch``, it needs a
        batch with at least one half-edge."""
        from . import kekule
        tables = kekule.KekuleTables(self.atomic_numbers.tolist(), self.num_bond_types) if tables is None else tables
        self._same_featuriser(tables, 'the tables were')
        max_steps = kekule.DEFAULT_MAX_STEPS if max_steps is None else max_steps
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        if cm.B == 0:
            return on_device(kekule.empty(), cm.device)
        return attach(kekule.launch(cm, tables, max_steps, select=select), cm, select, n_atoms, kekule.LAYOUT)

    def addh_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, tables=None, graph=None, *, select=None,
                   deg_tol=None, clash_tol=None):
        """``decode_batch``'s device part + the Kekulé assignment and the explicit hydrogens of every decoded molecule
        (``mdx_mol_kekulize`` with the default chemistry, then ``mdx_mol_hydrogens``; see ``moldiff_amd/hydrogens.py``).  tables: a
        ``hydrogens.HydrogenTables`` made for this featuriser (None = the defaults).  Nothing is copied to the host and nothing
        synchronises.  select: (n_graphs) device tensor; a molecule with 0 keeps its place with status 0, n_atoms 0 and every output
        0.  -> (kekule results, hydrogen results): the dict of ``kekulize_batch`` and the results dict of device tensors of
        ``hydrogens.launch`` (the per-molecule numbers of ``hydrogens.STAT_KEYS`` and n_atoms (B, int32), min_contact (B, float64);
        h_count, atom_flag and h_pos (4 x 3 float64 per atom) in the decode's own layout, molecule m at atom_ptr[m]).  These are the
        molecules AS DECODED; the placement is this project's idealised rule, not RDKit's AddHs and unverified against it, and
        clash_tol (1.5 Angstrom) is a convention.  Like ``decode_batch``, it needs a batch with at least one half-edge."""
        from . import hydrogens, kekule
        tables = hydrogens.HydrogenTables(self.atomic_numbers.tolist(), self.num_bond_types) if tables is None else tables
        self._same_featuriser(tables, 'the tables were')
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        if cm.B == 0:
            return on_device(kekule.empty(), cm.device), on_device(hydrogens.empty(), cm.device)
        kek = kekule.launch(cm, kekule.KekuleTables(tables.atomic_numbers, tables.num_bond_types), select=select)
        out = hydrogens.launch(cm, kek['kek_h'], kek['kek_order'], tables, hydrogens.DEFAULT_DEG_TOL if deg_tol is None else deg_tol,
                               hydrogens.DEFAULT_CLASH_TOL if clash_tol is None else clash_tol, select=select)
        return attach(kek, cm, select, n_atoms, kekule.LAYOUT), attach(out, cm, select, n_atoms, hydrogens.LAYOUT)

    def relax_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, tables=None, graph=None, *, select=None,
                    max_iters=None, gtol=None):
        """``addh_batch`` + the force-field relaxation of every decoded all-atom molecule (``mdx_mol_kekulize``, ``mdx_mol_hydrogens``
        with the default chemistry, then ``mdx_mol_relax``; see ``moldiff_amd/relax.py``).  tables: a ``relax.ForceFieldTables`` made
        for this featuriser (None = the defaults).  Nothing is copied to the host and nothing synchronises.  select: (n_graphs) device
        tensor; a molecule with 0 keeps its place with status 0, n_atoms 0 and every output 0.  -> (kekule results, hydrogen results,
        relax results): the dicts of ``addh_batch`` and the results dict of device tensors of ``relax.launch`` with n_atoms, in the
        decode's own layout, molecule m at atom_ptr[m].  These are the molecules AS DECODED; the force field is this project's own
        UFF-form model over an unverified table, not RDKit's UFFOptimizeMolecule.  Like ``decode_batch``, it needs a batch with at
        least one half-edge."""
        from . import hydrogens, kekule, relax
        tables = relax.ForceFieldTables(self.atomic_numbers.tolist(), self.num_bond_types) if tables is None else tables
        self._same_featuriser(tables, 'the tables were')
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        if cm.B == 0:
            return on_device(kekule.empty(), cm.device), on_device(hydrogens.empty(), cm.device), on_device(relax.empty(), cm.device)
        kek = kekule.launch(cm, kekule.KekuleTables(tables.atomic_numbers, tables.num_bond_types), select=select)
        hyd = hydrogens.launch(cm, kek['kek_h'], kek['kek_order'], hydrogens.HydrogenTables(tables.atomic_numbers, tables.num_bond_types), select=select)
        out = relax.launch(cm, kek['kek_order'], hyd['h_pos'], hyd['h_count'], hyd['atom_flag'], tables,
                           relax.DEFAULT_MAX_ITERS if max_iters is None else max_iters, relax.DEFAULT_GTOL if gtol is None else gtol, select=select)
        return attach(kek, cm, select, n_atoms, kekule.LAYOUT), attach(hyd, cm, select, n_atoms, hydrogens.LAYOUT), attach(out, cm, select, n_atoms, relax.LAYOUT)

    def embed_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, tables=None, graph=None, *, select=None, n_confs=None,
                    seed=0, mol_ids=None, **kw):
        """``addh_batch`` + conformers of every decoded all-atom molecule (``mdx_mol_kekulize``, ``mdx_mol_hydrogens`` with the default
        chemistry, then ``mdx_mol_bounds`` and ``mdx_mol_embed``; see ``moldiff_amd/embed.py``).  tables: a ``relax.ForceFieldTables`` made
        for this featuriser (None = the defaults); mol_ids: int64 device tensor of the ids that key the random numbers (None: the index
        in the batch); kw: the settings of ``embed.launch``.  Nothing is copied to the host and nothing synchronises; the bounds take the
        full stride of 256 atoms unless `na_cap` is given.  select: a molecule with 0 keeps its place with every output 0.
        -> (kekule results, hydrogen results, the dict of device tensors of ``embed.launch`` with n_atoms and atom_ptr) in the decode's
        own layout.  This project's own distance geometry, not ETKDG, unverified against RDKit; stereocentres are not constrained."""
        from . import embed, hydrogens, kekule, relax
        tables = relax.ForceFieldTables(self.atomic_numbers.tolist(), self.num_bond_types) if tables is None else tables
        self._same_featuriser(tables, 'the tables were')
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        kek = kekule.launch(cm, kekule.KekuleTables(tables.atomic_numbers, tables.num_bond_types), select=select)
        hyd = hydrogens.launch(cm, kek['kek_h'], kek['kek_order'], hydrogens.HydrogenTables(tables.atomic_numbers, tables.num_bond_types), select=select)
        out = embed.launch(cm, kek['kek_order'], hyd['h_count'], hyd['atom_flag'], embed.DEFAULT_N_CONFS if n_confs is None else n_confs, seed, tables,
                           mol_ids, select, **kw)
        out['n_atoms'], out['atom_ptr'] = n_atoms, cm.atom_ptr
        return attach(kek, cm, select, n_atoms, kekule.LAYOUT), attach(hyd, cm, select, n_atoms, hydrogens.LAYOUT), out

    def canon_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph=None, *, select=None, max_nodes=None,
                    atom_label=None):
        """``decode_batch``'s device part + the canonical labelling of every decoded molecule (``mdx_mol_canon``; see
        ``moldiff_amd/canon.py``).  Nothing is copied to the host and nothing synchronises.  select: (n_graphs) device tensor; a
        molecule with 0 keeps its place with status 0, n_atoms 0, rank -1 and every other output 0.  atom_label: int32 device tensor
        in the decode's atom layout, values in [0, 65536), instead of the atom class.  -> (results, canonical, keep): the results dict
        of device tensors (the per-molecule numbers of ``canon.STAT_KEYS``, cert_hash, n_atoms, n_bonds (B); rank, orbit and the
        canonical arrays in the decode's own layout, molecule m at atom_ptr[m] / bond_ptr[m]); a ``CompactMols`` over the canonical
        arrays (same pointers, the bond counts canon_n_bonds) and the `select` that leaves out the molecules without a canonical
        form, for ``kekule.launch``, ``groups.launch`` and ``rings.launch``.  These are the molecules AS DECODED; the labelling is
        this project's own, not RDKit's canonical ranking.  Like ``decode_batch``, it needs a batch with at least one half-edge."""
        from . import canon
        max_nodes = canon.DEFAULT_MAX_NODES if max_nodes is None else max_nodes
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        out = canon.launch(cm, max_nodes, select=select, atom_label=atom_label)
        canonical, keep = canon.canonical_compact(cm, out, select)
        return attach(out, cm, select, n_atoms, canon.LAYOUT), canonical, keep

    def stereo_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph=None, *, select=None, max_nodes=None,
                     atom_label=None, flat_tol=None, bond_tol=None):
        """``decode_batch``'s device part + the canonical labelling and the stereo perception of every decoded molecule
        (``mdx_mol_canon``, then ``mdx_mol_stereo``; see ``moldiff_amd/stereo.py``).  Nothing is copied to the host and nothing
        synchronises.  select, max_nodes, atom_label: as for ``canon_batch``.  -> (canon results, stereo results): the dict of
        ``canon_batch`` and the results dict of device tensors of ``stereo.launch`` (the per-molecule numbers of ``stereo.STAT_KEYS``,
        the two hashes, n_atoms, n_bonds (B); the words, stereo_rank, atom_tetra and bond_stereo in the decode's own layout, molecule
        m at atom_ptr[m] / bond_ptr[m]).  A masked molecule keeps its place with status 0, n_atoms 0, stereo_rank -1 and every other
        output 0.  These are the molecules AS DECODED; the stereo model is this project's own, not RDKit's and not CIP.  Two bonds
        between one pair of atoms cannot come out of the decode.  Like ``decode_batch``, it needs a batch with at least one half-edge."""
        from . import canon, stereo
        max_nodes = canon.DEFAULT_MAX_NODES if max_nodes is None else max_nodes
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        c = canon.launch(cm, max_nodes, select=select, atom_label=atom_label)
        s = stereo.launch(cm, c, stereo.DEFAULT_FLAT_TOL if flat_tol is None else flat_tol, stereo.DEFAULT_BOND_TOL if bond_tol is None else bond_tol,
                          max_nodes=max_nodes, select=select, atom_label=atom_label, atomic_numbers=self.atomic_numbers.tolist())
        return attach(c, cm, select, n_atoms, canon.LAYOUT), attach(s, cm, select, n_atoms, stereo.LAYOUT)

    def conformer_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph=None, *, select=None, max_nodes=None,
                        tol=None, max_group=None):
        """``decode_batch``'s device part + the conformer statistics of the decoded batch (``mdx_mol_canon``, then ``mdx_mol_bestrms``
        over all pairs inside every group of equal full certificate; see ``moldiff_amd/rmsd.py``) -> the summary dict of
        ``rmsd.summary``.  The coordinates and the canonical positions stay on the device; the grouping is exact, so canon's integer
        arrays are copied to the host, and so are the per-pair result columns the summary is made of: unlike the other ``*_batch``
        methods this call synchronises, and more than the summary crosses to the host.  tol: the RMSD in
        Angstrom up to which two conformers are one (0.5: a convention, not tuned).  These are the molecules AS DECODED.  Like
        ``decode_batch``, it needs a batch with at least one half-edge."""
        from . import canon, rmsd
        max_nodes = canon.DEFAULT_MAX_NODES if max_nodes is None else max_nodes
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        c = attach(canon.launch(cm, max_nodes, select=select), cm, select, n_atoms, canon.LAYOUT)
        return rmsd.conformers(cm, c, rmsd.DEFAULT_TOL if tol is None else tol, rmsd.DEFAULT_MAX_GROUP if max_group is None else max_group,
                               max_nodes=max_nodes, select=select)

    def framework_batch(self, pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph=None, *, mode=0, sys_bins=None, select=None):
        """``decode_batch``'s device part + the framework and the ring systems of every decoded molecule (``mdx_mol_rings``, then
        ``mdx_mol_framework``; see ``moldiff_amd/framework.py``).  mode: bit 0 EXO, bit 1 GENERIC.  Nothing is copied to the host and
        nothing synchronises.  select: (n_graphs) device tensor; a molecule with 0 keeps its place with status 0, n_atoms 0, every
        count 0 and atom_system -1.  -> (results, cm): the results dict of device tensors (the per-molecule numbers of
        ``framework.STAT_KEYS``, sys_hist, n_atoms, n_bonds (B); roles, the framework and the ring systems in the decode's own layout,
        molecule m at atom_ptr[m] / bond_ptr[m]) and the ``CompactMols`` of the decoded molecules, which is what
        ``framework.framework_compact``, ``framework.systems_compact`` and ``framework.keys`` take with the results.  These are the
        molecules AS DECODED; the definitions are this project's own, not RDKit's MurckoScaffold.  Like ``decode_batch``, it needs a
        batch with at least one half-edge."""
        from . import framework, rings
        sys_bins = framework.DEFAULT_BINS if sys_bins is None else sys_bins
        cm, _, select, n_atoms = self._compact_mols(pred, batch_node, halfedge_index, batch_halfedge, n_graphs, graph, select)
        ring_data = rings.launch(cm, self.num_element, self.num_bond_types, select=select)
        return attach(framework.launch(cm, ring_data, mode, sys_bins, select=select), cm, select, n_atoms, framework.LAYOUT), cm


def seperate_outputs(outputs, n_graphs, batch_node, halfedge_index, batch_halfedge):
    """Split packed numpy outputs {'pred': [...], 'traj': [...]} per molecule (host, numpy -- like the reference)."""
    pred, traj = outputs['pred'], outputs['traj']
    res = []
    for i in range(n_graphs):
        mn, mh = (batch_node == i), (batch_halfedge == i)
        assert mn.sum() * (mn.sum() - 1) == mh.sum() * 2
        he = halfedge_index[:, mh]
        first = mn.nonzero()[0].min()
        assert first == he.min()
        res.append({'pred': [pred[0][mn], pred[1][mn], pred[2][mh]],
                    'traj': [traj[0][:, mn], traj[1][:, mn], traj[2][:, mh]],
                    'halfedge_index': he - first})
    return res


def seperate_outputs_no_traj(outputs, n_graphs, batch_node, halfedge_index, batch_halfedge):
    res = []
    for i in range(n_graphs):
        mn, mh = (batch_node == i), (batch_halfedge == i)
        assert mn.sum() * (mn.sum() - 1) == mh.sum() * 2
        he = halfedge_index[:, mh]
        first = mn.nonzero()[0].min()
        assert first == he.min()
        res.append({'node': outputs[0][mn], 'pos': outputs[1][mn], 'halfedge': outputs[2][mh],
                    'halfedge_index': he - first})
    return res
