"""Symmetry-aware best RMSD between conformers of one constitution: the mean squared deviation after optimal rigid superposition,
minimised over every atom map that the symmetry of the labelled graph allows; the same against the mirror image; conformer statistics
of a batch and the reference's ``global_3d`` numbers against conformers made elsewhere.

The device half is ``mdx_mol_bestrms`` (csrc/mdx_bestrms.hip), reached through ``pairs_mols`` (lists of molecule dicts; runs ``canon``
on both sides), ``launch`` (a ``CompactMols``, the results of ``canon.launch`` and the targets), ``conformers`` / ``global_3d`` and
``FeaturizeMol.conformer_batch`` (the sampler's predictions).  ``best_rms_ref`` is the plain restatement for one pair (numpy's SVD) and
needs no GPU; the GPU tests compare with it in the unit (Ga + Gb) / n of the pair, to a tolerance derived from float64 alone
(profiles/bestrms_accuracy.txt).

What it is: the reference's ``global_3d`` metric is ``get_rdkit_rmsd`` (utils/scoring_func.py:56-74): ``rdMolAlign.GetBestRMS(mol,
mol3d)`` against conformers from ETKDG + UFF; it reports max / min / median.  This is the alignment half, defined in
include/moldiff_hip.h.  What it is NOT: there is no conformer generation (hand the conformers in, e.g. as an SDF from RDKit); the atoms
are the heavy atoms only; the symmetry group is that of this project's labelled graph (``canon``: aromatic bonds are a type of their
own), which can be smaller than RDKit's substructure match on a kekulised input; agreement with RDKit's ``GetBestRMS`` beyond the shared
definition is unmeasured; and with no trained checkpoint offline it is an instrument, not a measurement of sample quality.

The quantity in short.  Probe A and target B of equal full certificate.  Every optimal leaf of A's search tree has a rank vector c: the
atom map a -> B's canonical atom c[a]; over all optimal leaves these are the n_aut graph-preserving maps.  Per map, in float64, both
sides centred: Ga = sum |p|^2, Gb = sum |q|^2, H = sum p_a q_c[a]^T with singular values s1 >= s2 >= s3; msd = max(0, Ga + Gb -
2 (s1 + s2 + sign(det H) s3)) / n and msd_mirror with - sign(det H).  Per pair the minima over the maps, and msd_first: the value of the
map of A's own canonical rank.  RMSD = sqrt(msd), taken here on the host.

    python -m moldiff_amd.rmsd stats samples_all.pt --out conformers.npz [--tol 0.5] [--ref] [--part finished]
    python -m moldiff_amd.rmsd compare a.npz b.npz
    python -m moldiff_amd.rmsd against samples_all.pt --sdf conformers.sdf --out global3d.npz [--ref]
    python -m moldiff_amd.rmsd between a.pt b.pt [--ref]
"""
import json
import sys

import numpy as np

from . import canon, molpack
from .molpack import DEFAULT_ATOMIC_NUMBERS, jsd_counts, mol_graph, to_host

MAX_ATOMS, MAX_BONDS = canon.MAX_ATOMS, canon.MAX_BONDS
DEFAULT_MAX_NODES = canon.DEFAULT_MAX_NODES
DEFAULT_TOL = 0.5                                                 # Angstrom; a convention for "the same conformer", not tuned
DEFAULT_MAX_GROUP = 64
STATUS_OK, STATUS_NO_CANON, STATUS_ABANDONED, STATUS_NOT_THIS = 0, 1, 2, 3
# the columns of the device's per-probe table, in its order (include/moldiff_hip.h: MDX_BESTRMS_STATS)
STAT_KEYS = ('status', 'n_nodes', 'n_aut')
LAYOUT = molpack.Layout(STAT_KEYS + ('n_atoms',))                  # the per-probe part of the results table
FLOAT_KEYS = ('msd', 'msd_mirror', 'msd_first')                   # per pair, float64
PAIR_KEYS = FLOAT_KEYS + ('n_maps', 'pair_status', 'pair_target')  # + pair_ptr (B + 1): probe m owns the rows pair_ptr[m] .. pair_ptr[m + 1]
# a mirror value counts as smaller only by more than this many A^2: two honest float64 evaluations of one value differ by some 1e-15 of
# the pair's unit (Ga + Gb) / n, which stays below 1e4 A^2 for 256 atoms within 100 A of each other, so rounding alone gives 1e-11 at the
# most; an RMSD of 3e-5 A is far below anything a conformer comparison means
MIRROR_MARGIN = 1e-9
RMSD_BINS, RMSD_BIN_WIDTH = 21, 0.25                              # bin k: RMSD in [k / 4, (k + 1) / 4), the last bin everything above


def _check_tol(tol):
    if not float(tol) >= 0.0:                                      # NaN fails
        raise ValueError(f'tol must be a distance >= 0, got {tol}')
    return float(tol)


# ---- one probe on the host -----------------------------------------------------------------------------------------------------------

def kabsch_msd(p, q, c):
    """msd and its mirror value of the (n, 3) float64 point sets p and q under the atom map a -> c[a] (n >= 1), by numpy's SVD ->
    (msd, msd_mirror, unit): unit = (Ga + Gb) / n, in which an honest float64 evaluation is exact to a few ulp"""
    n = len(p)
    p, q = p - p.mean(axis=0), q[c] - q.mean(axis=0)
    G = float((p * p).sum() + (q * q).sum())
    H = p.T @ q
    s = np.linalg.svd(H, compute_uv=False)
    sign = 1.0 if np.linalg.det(H) >= 0.0 else -1.0
    return max(0.0, G - 2.0 * (s[0] + s[1] + sign * s[2])) / n, max(0.0, G - 2.0 * (s[0] + s[1] - sign * s[2])) / n, G / n


def _canon_pos(result):
    return np.asarray(result['canon_pos'], dtype=np.float64).reshape(-1, 3)


def probe_ref(info, canon_result, targets, atom_label=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS,
              evaluate=None):
    """Plain restatement of what ``mdx_mol_bestrms`` does for one probe: a molecule dict with ``atom_pos``, its canon result
    (``canon.canon_ref``'s dict or a ``canon.mol_result`` slice) and the targets, each an (n_t, 3) array of positions IN CANONICAL ATOM
    ORDER -> dict: ``status``, ``n_nodes``, ``n_aut``, ``n_atoms`` and one entry per target of ``msd``, ``msd_mirror``, ``msd_first``
    (float64), ``n_maps``, ``pair_status`` (3 where the atom count differs) and ``unit`` = (Ga + Gb) / n.  That a target has the probe's
    constitution is the caller's word, as on the device.  evaluate: ``kabsch_msd`` or a function like it (tools/bestrms_accuracy.py
    passes the device's own sums and solver)."""
    evaluate = evaluate or kabsch_msd
    max_nodes = canon._check_nodes(max_nodes)
    cls, bi, bt = mol_graph(info, atomic_numbers)
    n, nb, k = len(cls), bi.shape[1], len(targets)
    label = cls.astype(np.int64) if atom_label is None else canon._check_label(atom_label, n)
    out = dict(status=0, n_nodes=0, n_aut=0, n_atoms=n, n_maps=np.zeros(k, dtype=np.int32), pair_status=np.zeros(k, dtype=np.int32),
               unit=np.zeros(k), **{key: np.zeros(k) for key in FLOAT_KEYS})

    def failed(status):
        out['pair_status'][:] = status
        return dict(out, status=status)
    given = np.asarray(canon_result['rank'], dtype=np.int64).reshape(-1)
    if int(canon_result['status']) != 0 or n > MAX_ATOMS or nb > MAX_BONDS or len(given) != n or ((given < 0) | (given >= n)).any():
        return failed(STATUS_NO_CANON)
    ok = (bi[0] >= 0) & (bi[0] < n) & (bi[1] >= 0) & (bi[1] < n) & (bi[0] != bi[1]) if nb else np.zeros(0, dtype=bool)
    bx, by, btype = bi[0][ok], bi[1][ok], (bt[ok] & 0xff).astype(np.int64)
    pos = np.asarray(info['atom_pos'], dtype=np.float32).reshape(n, 3).astype(np.float64)
    tgt = [np.asarray(t, dtype=np.float32).reshape(-1, 3).astype(np.float64) for t in targets]
    fits = [len(t) == n for t in tgt]

    def words(c):
        lo, hi = np.minimum(c[bx], c[by]), np.maximum(c[bx], c[by])
        return sorted((lo * (1 << 20) + hi * (1 << 8) + btype).tolist())
    canonical = words(given)
    best = {'n_aut': 0}
    cur = [[np.inf, np.inf] for _ in tgt]

    def leaf(c):
        if words(c) != canonical:
            return
        best['n_aut'] += 1
        for j, t in enumerate(tgt):
            if fits[j] and n:
                a, b, _ = evaluate(pos, t, c)
                cur[j] = [min(cur[j][0], a), min(cur[j][1], b)]
    try:
        nodes = canon.search(label, bx, by, btype.astype(np.uint64), max_nodes, leaf)
    except canon.Abandoned:
        return failed(STATUS_ABANDONED)
    if best['n_aut'] == 0:                                             # the rank is not canon's for this molecule
        return failed(STATUS_NO_CANON)
    out.update(n_nodes=nodes, n_aut=best['n_aut'])
    for j, t in enumerate(tgt):
        if not fits[j]:
            out['pair_status'][j] = STATUS_NOT_THIS
            continue
        out['n_maps'][j] = best['n_aut']
        if n:
            out['msd'][j], out['msd_mirror'][j] = cur[j]
            out['msd_first'][j], _, out['unit'][j] = evaluate(pos, t, given)
    return out


def best_rms_ref(probe, target, canon_probe=None, canon_target=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """The plain restatement for one pair of molecule dicts with ``atom_pos`` (numpy's SVD in float64 at every optimal leaf of
    ``canon.search``) -> dict: ``msd``, ``msd_mirror``, ``msd_first``, ``unit`` (floats), ``n_maps``, ``status``, ``n_nodes``.  The canon
    results (``canon.canon_ref``) are made here when None.  Raises ValueError when the full certificates differ; a probe without a
    canonical form gives status 1 or 2 and zeros."""
    cp = canon.canon_ref(probe, None, max_nodes, atomic_numbers) if canon_probe is None else canon_probe
    ct = canon.canon_ref(target, None, max_nodes, atomic_numbers) if canon_target is None else canon_target
    for m, c in ((probe, cp), (target, ct)):
        if 'atom_pos' not in m or 'canon_pos' not in c:
            raise ValueError('best RMSD needs atom_pos in both molecules')
    if int(cp['status']) == 0 and canon.certificate_of(cp) != canon.certificate_of(ct):
        raise ValueError('probe and target differ in their full certificates: not the same constitution')
    r = probe_ref(probe, cp, [_canon_pos(ct)], None, max_nodes, atomic_numbers)
    return dict({k: float(r[k][0]) for k in FLOAT_KEYS + ('unit',)}, n_maps=int(r['n_maps'][0]), status=int(r['pair_status'][0]),
                n_nodes=r['n_nodes'])


def _csr(pairs, n_probes, n_targets):
    """[(probe, target)] -> (pair_ptr (B + 1), pair_target, order): the rows sorted by probe, stably; ``order[r]`` is the place of row
    r in `pairs`.  An index out of range raises ValueError."""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pr) and (pr.min() < 0 or pr[:, 0].max() >= n_probes or pr[:, 1].max() >= n_targets):
        raise ValueError('a pair index is out of range')
    order = np.argsort(pr[:, 0], kind='stable')
    ptr = np.zeros(n_probes + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(np.bincount(pr[:, 0], minlength=n_probes))
    return ptr, pr[order, 1].astype(np.int32), order


def _check_certs(cp, ct, pair_ptr, pair_target):
    """exact, on full certificates: every pair of a probe that has a canonical form joins it with a target of the same certificate"""
    certs_p, certs_t = canon._certificates(cp), canon._certificates(ct)
    for m, c in enumerate(certs_p):
        for j in pair_target[pair_ptr[m]:pair_ptr[m + 1]]:
            if c is not None and certs_t[int(j)] != c:
                raise ValueError(f'probe {m} and target {int(j)} differ in their full certificates: not the same constitution')


def stack_ref(probes, targets, pairs, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, canon_probes=None,
              canon_targets=None, check=True, evaluate=None):
    """``probe_ref`` of every probe of a list with its targets as the results dict ``pairs_mols`` returns (numpy).  pairs: [(probe index,
    target index)].  -> one entry per probe of ``status``, ``n_nodes``, ``n_aut``, ``n_atoms`` (int32) and ``atom_ptr``; one row per pair,
    sorted by probe (stably), of ``msd``, ``msd_mirror``, ``msd_first`` (float64), ``n_maps``, ``pair_status``, ``pair_target`` (int32),
    and ``unit`` (float64: (Ga + Gb) / n, host only); ``pair_ptr`` (B + 1).  The canon results of both lists (``canon.stack_ref``) are made
    here when None.  Differing certificates raise ValueError unless `check` is off."""
    cp = canon.stack_ref(probes, None, max_nodes, atomic_numbers) if canon_probes is None else to_host(canon_probes)
    ct = canon.stack_ref(targets, None, max_nodes, atomic_numbers) if canon_targets is None else to_host(canon_targets)
    ptr, tgt, _ = _csr(pairs, len(probes), len(targets))
    if len(tgt) and 'canon_pos' not in ct:
        raise ValueError('best RMSD needs atom_pos in every molecule')
    if check:
        _check_certs(cp, ct, ptr, tgt)
    tpos = [_canon_pos(canon.mol_result(ct, int(j))) for j in range(len(targets))] if len(tgt) else []
    if any('atom_pos' not in m for m in probes):
        raise ValueError('best RMSD needs atom_pos in every molecule')
    refs = [probe_ref(m, canon.mol_result(cp, k), [tpos[int(j)] for j in tgt[ptr[k]:ptr[k + 1]]], None, max_nodes, atomic_numbers, evaluate)
            for k, m in enumerate(probes)]
    out = molpack.stack(refs, LAYOUT)
    cat = lambda key, dtype: np.concatenate([r[key] for r in refs] + [np.zeros(0)]).astype(dtype)
    out.update({k: cat(k, np.float64) for k in FLOAT_KEYS + ('unit',)}, n_maps=cat('n_maps', np.int32), pair_status=cat('pair_status', np.int32),
               pair_target=tgt, pair_ptr=ptr)
    return out


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, canon_results, targets, pair_ptr, pair_target, select=None, max_nodes=DEFAULT_MAX_NODES, atom_label=None):
    """``mdx_mol_bestrms`` on the device arrays `cm` (a ``CompactMols`` with positions: the probes), the results of ``canon.launch`` on
    the same arrays (``rank`` and ``status`` are read), the targets (a dict of device tensors ``atom_ptr`` (T), ``n_atoms`` (T) and
    ``canon_pos`` (atoms, 3) float32 in canonical atom order: the results of ``canon.launch`` / ``canon_mols`` on the targets will do)
    and the pairs as CSR (int32 device tensors: pair_ptr (B + 1), pair_target (P)) -> dict of device tensors: ``status``, ``n_nodes``,
    ``n_aut`` (B; int32, columns of one (B, 3) table), ``msd``, ``msd_mirror``, ``msd_first`` (P, float64), ``n_maps`` and
    ``pair_status`` (P; columns of one (P, 2) table), and the ``pair_ptr`` and ``pair_target`` given.  That every target has its probe's
    constitution is the caller's word (``pairs_mols`` checks it).  No sync."""
    import torch
    from . import _lib
    max_nodes = canon._check_nodes(max_nodes)
    dev = cm.device
    i32 = lambda t, what: _int32(t, what, torch)
    pair_ptr, pair_target = i32(pair_ptr, 'pair_ptr'), i32(pair_target, 'pair_target')
    if pair_ptr.numel() != cm.B + 1:
        raise ValueError('pair_ptr holds one value per probe and one more')
    P = int(pair_target.numel())
    f64 = lambda: torch.zeros(max(P, 1), dtype=torch.float64, device=dev)
    out = {k: f64() for k in FLOAT_KEYS}
    pstats = torch.zeros(max(P, 1), 2, dtype=torch.int32, device=dev)
    stats = torch.zeros(cm.B, len(STAT_KEYS), dtype=torch.int32, device=dev)
    if cm.B > 0:
        if cm.atom_pos is None:
            raise ValueError('best RMSD needs positions: a CompactMols with atom_pos')
        rank, cstat = canon_results['rank'], canon_results['status']
        if rank.dtype != torch.int32 or cstat.dtype != torch.int32 or rank.numel() < cm.N_cap or cstat.numel() < cm.B:
            raise ValueError('canon_results holds rank and status of canon.launch on the same arrays')
        tptr, tn, tpos = i32(targets['atom_ptr'], 'the targets\' atom_ptr'), i32(targets['n_atoms'], 'the targets\' n_atoms'), targets['canon_pos']
        if tpos.dtype != torch.float32 or tpos.dim() != 2 or tpos.shape[1] != 3 or tptr.numel() < tn.numel():
            raise ValueError('the targets hold atom_ptr, n_atoms and canon_pos (atoms, 3) float32')
        if atom_label is not None:
            if atom_label.dtype != torch.int32 or atom_label.numel() < cm.N_cap:
                raise ValueError('atom_label is an int32 tensor in the layout of atom_type')
            atom_label = atom_label.contiguous()
        ops, at = cm.operands()
        _lib.check(_lib.lib().mdx_mol_bestrms(
            *ops, _lib.ptr(select), at(cm.atom_pos), None if atom_label is None else at(atom_label), at(rank.contiguous()),
            at(cstat.contiguous()), at(pair_ptr), at(pair_target), P, int(tn.numel()), at(tptr), at(tn), at(tpos.contiguous()),
            int(tpos.shape[0]), max_nodes, at(out['msd']), at(out['msd_mirror']), at(out['msd_first']), at(pstats), at(stats), _lib.stream()))
    out = {k: v[:P] for k, v in out.items()}
    out.update(n_maps=pstats[:P, 0], pair_status=pstats[:P, 1], pair_target=pair_target, pair_ptr=pair_ptr)
    return molpack.split_stats(out, stats, STAT_KEYS)


def _int32(t, what, torch):
    if t.dtype != torch.int32:
        raise ValueError(f'{what} is an int32 device tensor')
    return t.contiguous()


def _canon_both(probes, targets, device, max_nodes, atomic_numbers):
    """both lists packed, copied and labelled -> (cm of the probes, their canon results in cm's layout, the dense canon results of both)"""
    for m in list(probes) + list(targets):
        if 'atom_pos' not in m:
            raise ValueError('best RMSD needs atom_pos in every molecule')
    pp, cm = molpack.packed(probes, atomic_numbers, device, positions=True, simple=False)
    c = canon.launch(cm, max_nodes)
    same = targets is probes
    if same:
        pt, cmt, t = pp, cm, c
    else:
        pt, cmt = molpack.packed(targets, atomic_numbers, device, positions=True, simple=False)
        t = canon.launch(cmt, max_nodes)
    dense_p = molpack.dense(dict(c), cm, pp, canon.LAYOUT)
    dense_t = dense_p if same else molpack.dense(dict(t), cmt, pt, canon.LAYOUT)
    return cm, c, dense_p, dense_t


def pairs_mols(probes, targets, pairs, device, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, check=True):
    """Best RMSD of pairs of molecule dicts with ``atom_pos`` on the device: both lists are packed, copied and handed to ``mdx_mol_canon``;
    the certificates of every pair are compared exactly on the host (differing ones raise ValueError unless `check` is off); then
    ``mdx_mol_bestrms``.  pairs: [(probe index, target index)]; an index out of range raises ValueError.  -> the results dict of
    ``stack_ref`` with device tensors (without ``unit``)."""
    import torch
    canon._check_nodes(max_nodes)
    ptr, tgt, _ = _csr(pairs, len(probes), len(targets))
    cm, c, dense_p, dense_t = _canon_both(probes, targets, device, max_nodes, atomic_numbers)
    if check and len(tgt):
        _check_certs(to_host(dense_p), to_host(dense_t), ptr, tgt)
    dev = cm.device
    tdict = dense_t if len(targets) else {'atom_ptr': torch.zeros(0, dtype=torch.int32, device=dev), 'n_atoms': torch.zeros(0, dtype=torch.int32, device=dev),
                                          'canon_pos': torch.zeros(0, 3, dtype=torch.float32, device=dev)}
    out = launch(cm, c, tdict, torch.from_numpy(ptr).to(dev), torch.from_numpy(tgt).to(dev), None, max_nodes)
    return molpack.attach(out, cm, None, cm.n_atoms, LAYOUT)


# ---- conformers of a batch -----------------------------------------------------------------------------------------------------------

def group_pairs(canon_results, max_group=DEFAULT_MAX_GROUP):
    """The molecules of a canon results dict (host arrays) grouped by full certificate -> (group (B; the group's number by first member,
    -1 for a molecule without a canonical form, without atoms (a masked one) or left out by the cap), pairs [(i, j)] with i < j inside every group, n_left_out).
    A group keeps its first `max_group` members."""
    if int(max_group) < 1:
        raise ValueError('max_group must be at least 1')
    certs = canon._certificates(canon_results)
    first, members = {}, []
    group = np.full(len(certs), -1, dtype=np.int32)
    left = 0
    for m, c in enumerate(certs):
        if c is None or int(canon_results['n_atoms'][m]) == 0:
            continue
        g = first.setdefault(c, len(members))
        if g == len(members):
            members.append([])
        if len(members[g]) >= max_group:
            left += 1
            continue
        members[g].append(m)
        group[m] = g
    pairs = [(i, j) for ms in members for a, i in enumerate(ms) for j in ms[a + 1:]]
    return group, pairs, left


def conformer_results(mols, canon_results=None, tol=DEFAULT_TOL, max_group=DEFAULT_MAX_GROUP, device=None, max_nodes=DEFAULT_MAX_NODES,
                      atomic_numbers=DEFAULT_ATOMIC_NUMBERS, select=None):
    """All pairs inside every group of equal full certificate, measured -> the host results dict ``summary`` takes: per molecule
    ``group`` and ``canon_status``; per pair ``pair_probe``, ``pair_target`` (i < j), the float columns, ``n_maps``, ``pair_status``;
    ``tol``, ``max_group``, ``n_left_out``.  mols: a list of molecule dicts (on `device`, or the Python path when it is None), or a
    ``CompactMols`` with `canon_results` = the results of ``canon.launch`` on it joined with its counts and pointers (what
    ``FeaturizeMol.canon_batch`` returns): then the pairs are measured on its device; the grouping reads the canon results on the host,
    because it is exact, and the coordinates never leave the device."""
    tol = _check_tol(tol)
    on_cm = isinstance(mols, molpack.CompactMols)
    if on_cm:
        import torch
        cm, c_dev = mols, canon_results
        if c_dev is None:
            raise ValueError('a CompactMols comes with its canon results')
        c_host = to_host({k: v for k, v in c_dev.items() if k != 'canon_pos'})
    elif device is None:
        c_host = canon.stack_ref(mols, None, max_nodes, atomic_numbers) if canon_results is None else to_host(canon_results)
    else:
        import torch
        cm, c_dev, dense_p, _ = _canon_both(mols, mols, device, max_nodes, atomic_numbers)
        c_host = to_host(dense_p)
    group, pairs, left = group_pairs(c_host, max_group)
    B = len(group)
    if on_cm or device is not None:
        ptr, tgt, _ = _csr(pairs, B, B)
        dev = cm.device
        tdict = {'atom_ptr': cm.atom_ptr, 'n_atoms': cm.n_atoms, 'canon_pos': c_dev['canon_pos']}
        r = to_host(launch(cm, c_dev, tdict, torch.from_numpy(ptr).to(dev), torch.from_numpy(tgt).to(dev), select, max_nodes)) if B else None
    else:
        r = stack_ref(mols, mols, pairs, max_nodes, atomic_numbers, c_host, c_host, check=False) if B else None
    if r is None:
        r = dict({k: np.zeros(0) for k in FLOAT_KEYS}, n_maps=np.zeros(0, dtype=np.int32), pair_status=np.zeros(0, dtype=np.int32),
                 pair_target=np.zeros(0, dtype=np.int32), pair_ptr=np.zeros(1, dtype=np.int32))
    probe = np.repeat(np.arange(B, dtype=np.int32), np.diff(r['pair_ptr'].astype(np.int64)))
    out = {'group': group, 'canon_status': np.asarray(c_host['status'], dtype=np.int32), 'pair_probe': probe,
           'pair_target': np.asarray(r['pair_target'], dtype=np.int32), 'n_maps': np.asarray(r['n_maps'], dtype=np.int32),
           'pair_status': np.asarray(r['pair_status'], dtype=np.int32), 'tol': np.asarray(tol), 'max_group': np.asarray(int(max_group)),
           'n_left_out': np.asarray(int(left))}
    out.update({k: np.asarray(r[k], dtype=np.float64) for k in FLOAT_KEYS})
    return out


def summary(results):
    """The numbers of a ``conformer_results`` dict -> dict: ``n_molecules``, ``n_grouped`` (molecules with a canonical form, inside the
    cap), ``n_left_out`` (by the cap), ``n_groups`` (groups with at least 2 members), ``n_pairs`` and ``n_pairs_measured`` (status 0),
    ``conformers_per_group`` (per such group, in order of first member: the leaders of a leader clustering in batch order at
    sqrt(msd) <= tol; a group with an unmeasured pair treats it as far apart), ``n_duplicates`` (members of those groups beyond the
    first), ``share_geometric_duplicates`` (of these, the share that joined an earlier leader), ``mean_pairwise_rmsd``,
    ``rmsd_hist`` (bins of 0.25 A, the last everything from 5 A on), ``n_mirror_pairs`` (msd_mirror < msd at sqrt(msd_mirror) <= tol:
    mirror-image conformers; "smaller" means by more than MIRROR_MARGIN = 1e-9 A^2, which keeps two copies of one achiral conformer, whose
    two values differ by rounding alone, out), ``mean_first_minus_best`` (msd_first - msd, in A^2: what the symmetry search bought) and ``tol``.  NaN where
    nothing was counted.  The default tol of 0.5 A is a convention, not tuned."""
    r = to_host(results)
    tol, nan = float(np.reshape(r['tol'], -1)[0]), float('nan')
    group = r['group']
    ok = r['pair_status'] == STATUS_OK
    rmsd = np.sqrt(np.maximum(r['msd'], 0.0))
    near = {(int(i), int(j)) for i, j, good, d in zip(r['pair_probe'], r['pair_target'], ok, rmsd) if good and d <= tol}
    per_group, dup, joined = [], 0, 0
    for g in range(int(group.max()) + 1 if len(group) else 0):
        ms = np.flatnonzero(group == g)
        if len(ms) < 2:
            continue
        leaders = []
        for j in ms:
            if not any((int(l), int(j)) in near for l in leaders):
                leaders.append(j)
        per_group.append(len(leaders))
        dup += len(ms) - 1
        joined += len(ms) - len(leaders)
    k = int(ok.sum())
    mirror = ok & (r['msd'] - r['msd_mirror'] > MIRROR_MARGIN) & (np.sqrt(np.maximum(r['msd_mirror'], 0.0)) <= tol)
    hist = np.bincount(np.minimum((rmsd[ok] / RMSD_BIN_WIDTH).astype(np.int64), RMSD_BINS - 1), minlength=RMSD_BINS)
    return {'n_molecules': len(group), 'n_grouped': int((group >= 0).sum()), 'n_left_out': int(np.reshape(r['n_left_out'], -1)[0]), 'n_groups': len(per_group),
            'n_pairs': len(ok), 'n_pairs_measured': k, 'conformers_per_group': per_group, 'n_duplicates': dup,
            'share_geometric_duplicates': joined / dup if dup else nan, 'mean_pairwise_rmsd': float(rmsd[ok].mean()) if k else nan,
            'rmsd_hist': hist.tolist(), 'n_mirror_pairs': int(mirror.sum()),
            'mean_first_minus_best': float((r['msd_first'][ok] - r['msd'][ok]).mean()) if k else nan, 'tol': tol}


def conformers(mols, canon_results=None, tol=DEFAULT_TOL, max_group=DEFAULT_MAX_GROUP, device=None, max_nodes=DEFAULT_MAX_NODES,
               atomic_numbers=DEFAULT_ATOMIC_NUMBERS, select=None):
    """``summary`` of ``conformer_results``: the conformer statistics of a batch (a list of molecule dicts or a ``CompactMols``)"""
    return summary(conformer_results(mols, canon_results, tol, max_group, device, max_nodes, atomic_numbers, select))


def compare(a, b):
    """two ``conformer_results`` dicts -> dict: Jensen-Shannon divergence of ``rmsd_hist``, and both sides' ``n_groups``,
    ``share_geometric_duplicates``, ``mean_pairwise_rmsd`` and ``n_mirror_pairs``"""
    sa, sb = summary(a), summary(b)
    return dict({'rmsd': jsd_counts(sa['rmsd_hist'], sb['rmsd_hist'])},
                **{k: [sa[k], sb[k]] for k in ('n_groups', 'share_geometric_duplicates', 'mean_pairwise_rmsd', 'n_mirror_pairs')})


# ---- the reference's global_3d --------------------------------------------------------------------------------------------------------

def matching_pairs(canon_probes, canon_targets):
    """[(probe, target)] of every probe with every target of equal full certificate (host arrays), and the share of probes matched"""
    where = {}
    for j, c in enumerate(canon._certificates(canon_targets)):
        if c is not None:
            where.setdefault(c, []).append(j)
    return [(m, j) for m, c in enumerate(canon._certificates(canon_probes)) if c is not None for j in where.get(c, [])]


def _spread(results, n_probes):
    rmsd = np.sqrt(np.maximum(results['msd'], 0.0))
    out = {'rmsd_max': np.full(n_probes, np.nan), 'rmsd_min': np.full(n_probes, np.nan), 'rmsd_median': np.full(n_probes, np.nan),
           'n_matched': np.zeros(n_probes, dtype=np.int32)}
    ptr = results['pair_ptr'].astype(np.int64)
    for m in range(n_probes):
        d = rmsd[ptr[m]:ptr[m + 1]][results['pair_status'][ptr[m]:ptr[m + 1]] == STATUS_OK]
        out['n_matched'][m] = len(d)
        if len(d):
            out['rmsd_max'][m], out['rmsd_min'][m], out['rmsd_median'][m] = d.max(), d.min(), np.median(d)
    return out


def global_3d(probes, targets, device=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """The reference's ``global_3d`` columns: every probe against every target of equal full certificate (conformers made elsewhere)
    -> dict of (len(probes)) arrays: ``rmsd_max``, ``rmsd_min``, ``rmsd_median`` (NaN without a target) and ``n_matched``.  On
    `device`, or the Python path when it is None.  Equal certificate means equal bond types too: a target whose aromatic bonds were
    kekulised to types 1 and 2 does not match a probe that holds them as type 4."""
    if device is None:
        cp, ct = canon.stack_ref(probes, None, max_nodes, atomic_numbers), canon.stack_ref(targets, None, max_nodes, atomic_numbers)
        r = stack_ref(probes, targets, matching_pairs(cp, ct), max_nodes, atomic_numbers, cp, ct, check=False)
    else:
        import torch
        cm, c, dense_p, dense_t = _canon_both(probes, targets, device, max_nodes, atomic_numbers)
        ptr, tgt, _ = _csr(matching_pairs(to_host(dense_p), to_host(dense_t)), len(probes), len(targets))
        if len(tgt) == 0:
            return _spread(dict(msd=np.zeros(0), pair_status=np.zeros(0, dtype=np.int32), pair_ptr=ptr), len(probes))
        r = to_host(launch(cm, c, dense_t, torch.from_numpy(ptr).to(cm.device), torch.from_numpy(tgt).to(cm.device), None, max_nodes))
    return _spread(r, len(probes))


def strip_hydrogens(block):
    """a V2000 mol block without its hydrogen atoms and their bonds: the reference's probe is the heavy-atom molecule.  Only the
    counts line, the atom block and the bond block are kept: every property line behind them (``M  CHG``, ``M  ISO``, ...) is dropped,
    as ``read_mol_block`` reads none of them"""
    lines = block.splitlines()
    at = next((k for k, ln in enumerate(lines) if ln.rstrip().endswith('V2000')), None)
    if at is None:
        raise ValueError('not a V2000 mol block (no counts line)')
    na, nb = int(lines[at][0:3]), int(lines[at][3:6])
    atoms, bonds = lines[at + 1:at + 1 + na], lines[at + 1 + na:at + 1 + na + nb]
    keep = [ln[31:34].strip() not in ('H', 'D') for ln in atoms]
    new = np.cumsum(keep)
    bonds = [ln for ln in bonds if keep[int(ln[0:3]) - 1] and keep[int(ln[3:6]) - 1]]
    bonds = ['%3d%3d%s' % (new[int(ln[0:3]) - 1], new[int(ln[3:6]) - 1], ln[6:]) for ln in bonds]
    atoms = [ln for ln, k in zip(atoms, keep) if k]
    return '\n'.join(lines[:at] + ['%3d%3d%s' % (len(atoms), len(bonds), lines[at][6:])] + atoms + bonds + ['M  END']) + '\n'


def read_sdf(path):
    """the mol blocks of an SDF as heavy-atom molecule dicts (``sample_drug3d.read_mol_block`` of ``strip_hydrogens``)"""
    from .sample_drug3d import read_mol_block
    with open(path) as f:
        blocks = [b[1:] if b.startswith('\n') else b for b in f.read().split('$$$$') if 'V2000' in b]
    return [read_mol_block(strip_hydrogens(b)) for b in blocks]


def between(a, b, device=None, max_nodes=DEFAULT_MAX_NODES, atomic_numbers=DEFAULT_ATOMIC_NUMBERS):
    """molecule m of list `a` against molecule m of list `b` where their certificates agree -> dict: ``n_compared`` (the shorter
    length), ``share_same_constitution``, and over the agreeing pairs ``mean_rmsd``, ``median_rmsd``, ``max_rmsd`` and ``rmsd_hist``"""
    k = min(len(a), len(b))
    a, b = list(a[:k]), list(b[:k])
    if device is None:
        ca, cb = canon.stack_ref(a, None, max_nodes, atomic_numbers), canon.stack_ref(b, None, max_nodes, atomic_numbers)
    else:
        ca, cb = to_host(canon.canon_mols(a, device, None, max_nodes, atomic_numbers)), to_host(canon.canon_mols(b, device, None, max_nodes, atomic_numbers))
    certs_a, certs_b = canon._certificates(ca), canon._certificates(cb)
    pairs = [(m, m) for m in range(k) if certs_a[m] is not None and certs_a[m] == certs_b[m]]
    r = stack_ref(a, b, pairs, max_nodes, atomic_numbers, ca, cb, check=False) if device is None else to_host(pairs_mols(a, b, pairs, device, max_nodes, atomic_numbers, check=False))
    d = np.sqrt(np.maximum(r['msd'], 0.0))[r['pair_status'] == STATUS_OK]
    nan = float('nan')
    hist = np.bincount(np.minimum((d / RMSD_BIN_WIDTH).astype(np.int64), RMSD_BINS - 1), minlength=RMSD_BINS)
    return {'n_compared': k, 'share_same_constitution': len(pairs) / k if k else nan, 'mean_rmsd': float(d.mean()) if len(d) else nan,
            'median_rmsd': float(np.median(d)) if len(d) else nan, 'max_rmsd': float(d.max()) if len(d) else nan, 'rmsd_hist': hist.tolist()}


# ---- command line --------------------------------------------------------------------------------------------------------------------

def _against(args):
    probes, targets = molpack.load_mols(args.samples, args.part), read_sdf(args.sdf)
    res = global_3d(probes, targets, _device(args), args.max_nodes)
    molpack.save_npz(res, args.out)
    have = res['n_matched'] > 0
    mean = lambda k: float(res[k][have].mean()) if have.any() else float('nan')
    print(json.dumps({'n_probes': len(probes), 'n_targets': len(targets), 'n_probes_matched': int(have.sum()),
                      'mean_rmsd_max': mean('rmsd_max'), 'mean_rmsd_min': mean('rmsd_min'), 'mean_rmsd_median': mean('rmsd_median')}, indent=1))


def _between(args):
    print(json.dumps(between(molpack.load_mols(args.a, args.part), molpack.load_mols(args.b, args.part), _device(args), args.max_nodes), indent=1))


def _device(args):
    if args.ref:
        return None
    import torch
    torch.cuda.set_device(torch.device(args.device))
    return args.device


def _common(p):
    p.add_argument('--part', default='finished')
    p.add_argument('--max_nodes', type=int, default=DEFAULT_MAX_NODES)
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--ref', action='store_true', help='the Python path instead of the device')


def _add_against(p):
    p.add_argument('samples')
    p.add_argument('--sdf', required=True, help='conformers made elsewhere, as V2000 mol blocks; hydrogens are dropped.  A block matches a sample only when its bond '
                        'types are the sample\'s: aromatic bonds written as type 4, not kekulised (RDKit: MolToMolBlock(mol, kekulize=False))')
    p.add_argument('--out', required=True)
    _common(p)


def _add_between(p):
    p.add_argument('a')
    p.add_argument('b')
    _common(p)


def main(argv=None):
    return molpack.stats_main(
        argv, 'rmsd', __doc__, ('conformer statistics of the molecules stored in a samples_all.pt: best RMSD inside groups of equal certificate',
                                'RMSD-histogram divergence and both sides\' conformer numbers of two files'),
        [('--tol', dict(type=float, default=DEFAULT_TOL, help='two conformers are the same up to this RMSD in Angstrom (0.5: a convention, not tuned)')),
         ('--max_group', dict(type=int, default=DEFAULT_MAX_GROUP)), ('--max_nodes', dict(type=int, default=DEFAULT_MAX_NODES))],
        lambda mols, a, dev: conformer_results(mols, None, a.tol, a.max_group, dev, a.max_nodes), summary, compare,
        extra=[('against', 'the reference\'s global_3d columns against the conformers of an SDF', _add_against, _against),
               ('between', 'molecule by molecule RMSD of two runs where the constitutions agree', _add_between, _between)])


if __name__ == '__main__':
    sys.exit(main())
