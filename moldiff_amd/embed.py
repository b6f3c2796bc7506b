"""Conformer generation: distance bounds of the all-atom molecule (heavy atoms plus the hydrogens of ``hydrogens.addh_mols``), triangle
smoothed, and 3D coordinates embedded from them; with ``relax`` and ``rmsd`` behind it, the reference's ``global_3d`` metric
(``get_rdkit_rmsd``: AddHs, EmbedMultipleConfs, UFF, GetBestRMS -> max / min / median) without another program.

The device half is ``mdx_mol_bounds`` (csrc/mdx_bounds.hip) and ``mdx_mol_embed`` (csrc/mdx_embed.hip), reached through ``embed_mols`` (a
list of molecule dicts; runs ``kekule`` and ``hydrogens`` first), ``launch`` (a ``CompactMols`` and the device arrays of
``hydrogens.launch``), ``global3d_mols`` (the whole chain) and ``FeaturizeMol.embed_batch``.  ``bounds_ref`` and ``embed_ref`` are the
restatement for one molecule in float64, in the device's own order of operations and reduction tree (numpy's element-wise float64
operations over the atoms, sequential over the partner atom as the device's loop is), and need no GPU.

What it is: THIS PROJECT'S OWN MODEL, stated exactly in include/moldiff_hip.h: distance geometry with random starting coordinates,
in the spirit of RDKit's ``useRandomCoords`` embedding.  It is NOT ETKDG (no torsion preferences, no planarity preference for 1-4 pairs,
no chiral-volume constraints: an embedded conformer MAY BE THE MIRROR IMAGE at a stereocentre) and it is UNVERIFIED AGAINST RDKit; its
rest lengths and angles come from the UNVERIFIED rows of ``relax.ForceFieldTables``.  The tolerances (0.01 / 0.04 / 0.06 Angstrom),
``vdw_scale`` 0.6, ``viol_tol`` 0.1, ``gtol`` 1e-3 and the iteration caps are conventions.  With no trained checkpoint offline it is
an instrument, not a measurement of sample quality.

    python -m moldiff_amd.embed stats samples_all.pt --out global3d.npz [--sdf conformers.sdf] [--confs 10] [--seed 0] [--part finished]
    python -m moldiff_amd.embed compare a.npz b.npz
"""
import math
import sys

import numpy as np

from . import hydrogens, kekule, molpack, relax
from .hydrogens import MAX_H
from .molpack import jsd_counts, to_host
from .relax import P_C0, P_X, block_max, block_sum

MAX_ATOMS = relax.MAX_ATOMS
DEFAULT_TOL12, DEFAULT_TOL13, DEFAULT_TOL14 = 0.01, 0.04, 0.06     # Angstrom: conventions
DEFAULT_VDW_SCALE = 0.6                                            # of the mean of the two rows' x: a convention
DEFAULT_VIOL_TOL = 0.1                                             # largest relative violation of an accepted conformer: a convention
DEFAULT_MAX_ITERS = 400                                            # per stage
DEFAULT_MAX_ATTEMPTS = 4
DEFAULT_GTOL = 1e-3                                                # rms gradient of the error function
DEFAULT_MAX_STEP = 1.0                                             # Angstrom
DEFAULT_N_CONFS = 10
FAR, BOX, W4_A, W4_B = 1000.0, 2.0, 0.1, 1.0
HIST_PER_ATOM = 2 * relax.HISTORY * 4
STATUS_OK, STATUS_TOO_LARGE, STATUS_NONFINITE, STATUS_INCONSISTENT, STATUS_FAILED = 0, 1, 2, 3, 4
OTHER, P12, P13, P14 = 0, 1, 2, 3
BOUNDS_KEYS = ('status', 'n_all', 'n_12', 'n_13', 'n_14', 'n_ring_angles', 'n_tightened')
CONF_KEYS = ('status', 'attempts', 'iterations_a', 'iterations_b', 'n_evals')
VALUE_KEYS = ('error_a', 'error_b', 'max_violation')
RING_C0 = tuple(math.cos(d * (math.pi / 180.0)) for d in (60.0, 90.0, 108.0))
RMSD_BINS, RMSD_MAX = 40, 4.0


def _check_bounds(tol12, tol13, tol14, vdw_scale, na_cap):
    for t in (tol12, tol13, tol14):
        if not 0.0 <= float(t) <= 1.0:                             # NaN fails
            raise ValueError(f'tol12, tol13 and tol14 must lie in [0, 1], got {t}')
    if not 0.0 < float(vdw_scale) <= 2.0:
        raise ValueError(f'vdw_scale must lie in (0, 2], got {vdw_scale}')
    if not 1 <= int(na_cap) <= MAX_ATOMS:
        raise ValueError(f'na_cap must lie in 1 .. {MAX_ATOMS}, got {na_cap}')
    return float(tol12), float(tol13), float(tol14), float(vdw_scale), int(na_cap)


def _check_embed(n_confs, max_iters, max_attempts, gtol, max_step, viol_tol):
    if not 1 <= int(n_confs) <= 65535:
        raise ValueError(f'n_confs must lie in 1 .. 65535, got {n_confs}')
    if not 0 <= int(max_iters) <= relax.MAX_ITERS_LIMIT:
        raise ValueError(f'max_iters must lie in 0 .. {relax.MAX_ITERS_LIMIT}, got {max_iters}')
    if not 1 <= int(max_attempts) <= 64:
        raise ValueError(f'max_attempts must lie in 1 .. 64, got {max_attempts}')
    if not 0.0 < float(gtol) <= 1e6:
        raise ValueError(f'gtol must lie in (0, 1e6], got {gtol}')
    if not 0.0 < float(max_step) <= 10.0:
        raise ValueError(f'max_step must lie in (0, 10] Angstrom, got {max_step}')
    if not 0.0 < float(viol_tol) <= 10.0:
        raise ValueError(f'viol_tol must lie in (0, 10], got {viol_tol}')
    return int(n_confs), int(max_iters), int(max_attempts), float(gtol), float(max_step), float(viol_tol)


# ---- Philox4x32-10: the arithmetic of tests/philox_ref.py and csrc/mdx_philox.h on Python integers ------------------------------------

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(c, k0, k1):
    """one counter (four 32-bit words) and a key (two words) -> four 32-bit words"""
    c0, c1, c2, c3 = (int(x) & _MASK for x in c)
    k0, k1 = int(k0) & _MASK, int(k1) & _MASK
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def u53(p, q):
    """two words -> a double in [0, 1), exactly: ((p >> 5) 2^26 + (q >> 6)) 2^-53"""
    return (float(p >> 5) * 67108864.0 + float(q >> 6)) * 2.0 ** -53


def start_coords(n_all, box, seed, mol_id, conf, attempt):
    """the 4D starting coordinates of one attempt -> (n_all, 4) float64"""
    k0, k1 = int(seed) & _MASK, (int(seed) >> 32) & _MASK
    mol_id = int(mol_id) & 0xFFFFFFFFFFFFFFFF
    hi = (((mol_id >> 32) << 8) & _MASK) | int(attempt)
    out = np.zeros((n_all, 4))
    for a in range(n_all):
        ra = philox4x32_10((2 * a, conf, mol_id & _MASK, hi), k0, k1)
        rb = philox4x32_10((2 * a + 1, conf, mol_id & _MASK, hi), k0, k1)
        out[a] = [(u53(ra[0], ra[1]) - 0.5) * box, (u53(ra[2], ra[3]) - 0.5) * box, (u53(rb[0], rb[1]) - 0.5) * box, (u53(rb[2], rb[3]) - 0.5) * box]
    return out


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------

def _b13(r1, r2, c):
    return math.sqrt((r1 * r1 + r2 * r2) - ((2.0 * r1) * r2) * c)


def _b14(r1, r2, r3, c1, c2):
    s1, s2 = math.sqrt(1.0 - c1 * c1), math.sqrt(1.0 - c2 * c2)
    dx = (r2 - r3 * c2) - r1 * c1
    yc, yt = r3 * s2 - r1 * s1, r3 * s2 + r1 * s1
    return math.sqrt(dx * dx + yc * yc), math.sqrt(dx * dx + yt * yt)


def bounds_ref(info, order, h_count, atom_flag, tables=None, tol12=DEFAULT_TOL12, tol13=DEFAULT_TOL13, tol14=DEFAULT_TOL14,
               vdw_scale=DEFAULT_VDW_SCALE, na_cap=MAX_ATOMS):
    """Restatement of ``mdx_mol_bounds`` for one molecule (order, h_count, atom_flag as for ``relax.relax_ref``) -> dict: the numbers
    of BOUNDS_KEYS, ``n_atoms``, ``h`` (hydrogens per heavy atom), and for status OK or INCONSISTENT ``lower`` / ``upper`` (n_all, n_all)
    float64, ``cls`` (uint8: 0 other, 1 1-2, 2 1-3, 3 1-4) and ``lower0`` / ``upper0``, the bounds before smoothing."""
    tb = relax._tables(tables)
    tol12, tol13, tol14, vdw_scale, na_cap = _check_bounds(tol12, tol13, tol14, vdw_scale, na_cap)
    n = len(np.asarray(info['element']).reshape(-1))
    m = relax._stage(info, order, h_count, np.zeros((n, MAX_H, 3)), atom_flag, tb)
    zero = dict({k: 0 for k in BOUNDS_KEYS}, n_atoms=n, h=[min(max(int(x), 0), MAX_H) for x in np.asarray(h_count).reshape(-1)])
    if m is None or m.n_all > na_cap:
        return dict(zero, status=STATUS_TOO_LARGE)
    na = m.n_all
    nbrs = [[b for b, _ in r] for r in m.rows]
    bond = {(a, b): e for a in range(na) for b, e in m.rows[a]}
    r = lambda a, b: m.bond_par[bond[a, b]][0]

    def ring_size(a, b, c):
        if (a, c) in bond:
            return 3
        if any(x != b and (x, c) in bond for x in nbrs[a]):
            return 4
        if any(x != b and y != b and (x, y) in bond for x in nbrs[a] for y in nbrs[c]):
            return 5
        return 0

    def c0(a, b, c):
        rs = ring_size(a, b, c)
        return RING_C0[rs - 3] if rs else m.par[b][P_C0]
    x = np.asarray([p[P_X] for p in m.par] + [0.0] * 0, dtype=np.float64).reshape(na)
    L = vdw_scale * (0.5 * (x[:, None] + x[None, :]))
    U = np.full((na, na), FAR)
    np.fill_diagonal(L, 0.0), np.fill_diagonal(U, 0.0)
    cls = np.zeros((na, na), dtype=np.uint8)

    def widen(a, d, lo, hi, c):
        lo = 0.0 if lo < 0.0 else lo
        if cls[a, d] != c:
            cls[a, d] = cls[d, a] = c
            L[a, d] = L[d, a] = lo
            U[a, d] = U[d, a] = hi
        else:
            L[a, d] = L[d, a] = min(L[a, d], lo)
            U[a, d] = U[d, a] = max(U[a, d], hi)
    for b in range(na):                                                # 1-3
        for a in nbrs[b]:
            for d in nbrs[b]:
                if a < d and (a, d) not in bond:
                    l = _b13(r(a, b), r(b, d), c0(a, b, d))
                    widen(a, d, l - tol13, l + tol13, P13)
    for b in range(na):                                                # 1-4: every path once, from its lower end
        for c in nbrs[b]:
            for a in nbrs[b]:
                if a == c:
                    continue
                for d in nbrs[c]:
                    if d == b or d == a or not a < d or (a, d) in bond or cls[a, d] == P13:
                        continue
                    cis, trans = _b14(r(a, b), r(b, c), r(c, d), c0(a, b, c), c0(b, c, d))
                    widen(a, d, cis - tol14, trans + tol14, P14)
    for (a, b), e in bond.items():                                     # 1-2
        lo = m.bond_par[e][0] - tol12
        L[a, b], U[a, b], cls[a, b] = (0.0 if lo < 0.0 else lo), m.bond_par[e][0] + tol12, P12
    ring = sum(ring_size(nbrs[b][q1], b, nbrs[b][q2]) != 0 for b in range(na) for q1 in range(len(nbrs[b])) for q2 in range(q1 + 1, len(nbrs[b])))
    L0, U0 = L.copy(), U.copy()
    for k in range(na):
        row = U[k].copy()
        U = np.minimum(U, row[:, None] + row[None, :])
    for k in range(na):
        lr, ur = L[k].copy(), U[k]
        L = np.maximum(np.maximum(L, lr[:, None] - ur[None, :]), lr[None, :] - ur[:, None])
    upper_tri = np.triu(np.ones((na, na), dtype=bool), 1)
    count = lambda c: int(((cls == c) & upper_tri).sum())
    return dict(zero, status=STATUS_INCONSISTENT if bool(((L > U) & upper_tri).any()) else STATUS_OK, n_all=na, n_12=count(P12), n_13=count(P13),
                n_14=count(P14), n_ring_angles=int(ring), n_tightened=int((((L != L0) | (U != U0)) & upper_tri).sum()), lower=L, upper=U, cls=cls,
                lower0=L0, upper0=U0)


# ---- the error function and its minimisation ------------------------------------------------------------------------------------------

def error_ref(X, L, U, w4):
    """the distance-violation error at the 4D point X (n_all, 4) and its gradient, as the device accumulates them -> (total, gradient
    (n_all, 4), per-atom partial energies)"""
    na = len(X)
    g, e, idx = np.zeros((na, 4)), np.zeros(na), np.arange(na)
    with np.errstate(all='ignore'):
        for b in range(na):
            d = X - X[b]
            d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3]
            lb, ub = L[b], U[b]
            ub2, lb2 = ub * ub, lb * lb
            over = d2 > ub2
            under = ~over & (d2 < lb2)
            v1 = d2 / ub2 - 1.0
            q = lb2 + d2
            v2 = (2.0 * lb2) / q - 1.0
            en = np.where(over, v1 * v1, np.where(under, v2 * v2, 0.0))
            pre = np.where(over, (4.0 * v1) / ub2, np.where(under, -(((8.0 * lb2) * v2) / (q * q)), 0.0))
            g = g + pre[:, None] * d
            e = e + np.where(idx < b, en, 0.0)
    if na:
        e = e + w4 * (X[:, 3] * X[:, 3])
        g[:, 3] = g[:, 3] + (2.0 * w4) * X[:, 3]
    return block_sum(e.tolist()), g, e


def violation_ref(pos, bounds):
    """the largest relative violation in 3D of the 1-2 and 1-3 bounds and of the other pairs' lower bounds; pos: (n_all, 3)"""
    L, U, cls = bounds['lower'], bounds['upper'], bounds['cls']
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    worst = 0.0
    for a in range(len(pos)):
        d3 = pos[a] - pos
        d = np.sqrt((d3[:, 0] * d3[:, 0] + d3[:, 1] * d3[:, 1]) + d3[:, 2] * d3[:, 2])
        for b in range(len(pos)):
            if b == a or cls[b, a] == P14:
                continue
            if d[b] < L[b, a]:
                worst = max(worst, (L[b, a] - d[b]) / L[b, a])
            elif cls[b, a] != OTHER and d[b] > U[b, a]:
                worst = max(worst, (d[b] - U[b, a]) / U[b, a])
    return float(worst)


def allatom(pos, h_pos, h):
    """the inverse of the output layout: (n, 3) and (n, 4, 3) -> (n_all, 3), heavy atoms, then the hydrogens in (atom, k) order"""
    h_pos = np.asarray(h_pos).reshape(-1, MAX_H, 3)
    return np.concatenate([np.asarray(pos, dtype=np.float64).reshape(-1, 3)] + [h_pos[a, :h[a]].reshape(-1, 3) for a in range(len(h))])


def embed_ref(bounds, conf=0, seed=0, mol_id=0, max_iters=DEFAULT_MAX_ITERS, max_attempts=DEFAULT_MAX_ATTEMPTS, gtol=DEFAULT_GTOL,
              max_step=DEFAULT_MAX_STEP, viol_tol=DEFAULT_VIOL_TOL, trace=None):
    """Restatement of ``mdx_mol_embed`` for one (molecule, conformer); bounds: what ``bounds_ref`` returned -> dict: the numbers of
    CONF_KEYS and VALUE_KEYS, ``pos`` (n, 3), ``h_pos`` (n, 4, 3) float64 and ``errors``, the accepted error after every iteration of the
    last attempt (stage A, then stage B).  trace: receives every number a decision compares with a threshold as (kind, value,
    threshold): 'rms', 'descent', 'cap', 'armijo', 'curvature', 'violation'."""
    _, max_iters, max_attempts, gtol, max_step, viol_tol = _check_embed(1, max_iters, max_attempts, gtol, max_step, viol_tol)
    trace = [] if trace is None else trace
    n, h = bounds['n_atoms'], bounds['h']
    zero = dict({k: 0 for k in CONF_KEYS}, **{k: 0.0 for k in VALUE_KEYS}, pos=np.zeros((n, 3)), h_pos=np.zeros((n, MAX_H, 3)), errors=[])
    if bounds['status'] != STATUS_OK:
        return dict(zero, status=bounds['status'])
    na, L, U, cls = bounds['n_all'], bounds['lower'], bounds['upper'], bounds['cls']
    box = BOX * block_max(float(U[a][cls[a] != OTHER].max(initial=0.0)) for a in range(na))
    status, n_evals = STATUS_FAILED, 0
    for attempt in range(max_attempts):
        x = start_coords(na, box, seed, mol_id, conf, attempt)
        errors, iters, err = [], [0, 0], [0.0, 0.0]
        for stage, w4 in enumerate((W4_A, W4_B)):
            r = relax.lbfgs_ref(x, lambda p: error_ref(p, L, U, w4), max_iters, gtol, max_step, trace)
            if r is None:
                return dict(zero, status=STATUS_NONFINITE)
            x, err[stage], iters[stage] = r['x'], r['energy'], r['iterations']
            n_evals += r['n_evals']
            errors += r['energies']
        viol = violation_ref(x[:, :3], bounds)
        trace.append(('violation', viol, viol_tol))
        if viol <= viol_tol:
            status = STATUS_OK
            break
    heavy, hs = relax._split(n, h, x[:, :3])
    return dict(status=status, attempts=attempt + 1, iterations_a=iters[0], iterations_b=iters[1], n_evals=n_evals, error_a=err[0], error_b=err[1],
                max_violation=viol, pos=heavy, h_pos=hs, errors=errors)


def near_threshold(bounds, conf=0, seed=0, mol_id=0, max_iters=DEFAULT_MAX_ITERS, max_attempts=DEFAULT_MAX_ATTEMPTS, gtol=DEFAULT_GTOL,
                   max_step=DEFAULT_MAX_STEP, viol_tol=DEFAULT_VIOL_TOL, band=1e-9, trace=None):
    """whether some decision of ``embed_ref`` is ``relax.near`` its threshold: the conformers a device comparison may leave out.
    trace: the decision trace to judge instead of running ``embed_ref``."""
    if trace is None:
        trace = []
        embed_ref(bounds, conf, seed, mol_id, max_iters, max_attempts, gtol, max_step, viol_tol, trace)
    return relax.near(trace, band)


def stack_ref(mols, n_confs=DEFAULT_N_CONFS, seed=0, inputs=None, tables=None, mol_ids=None, max_iters=DEFAULT_MAX_ITERS,
              max_attempts=DEFAULT_MAX_ATTEMPTS, gtol=DEFAULT_GTOL, max_step=DEFAULT_MAX_STEP, viol_tol=DEFAULT_VIOL_TOL, **bounds_kw):
    """``bounds_ref`` and ``embed_ref`` of every molecule of a list as the results dict ``embed_mols`` returns (numpy)"""
    tb = relax._tables(tables)
    inputs = relax._inputs(mols, tb) if inputs is None else inputs
    K = _check_embed(n_confs, max_iters, max_attempts, gtol, max_step, viol_tol)[0]
    bs = [bounds_ref(info, i[0], i[1], i[3], tb, **bounds_kw) for info, i in zip(mols, inputs)]
    ids = range(len(mols)) if mol_ids is None else mol_ids
    refs = [[embed_ref(b, c, seed, mid, max_iters, max_attempts, gtol, max_step, viol_tol) for c in range(K)] for b, mid in zip(bs, ids)]
    out = {'bounds_' + k: np.asarray([b[k] for b in bs], dtype=np.int32).reshape(len(mols)) for k in BOUNDS_KEYS}
    out.update({k: np.asarray([[r[k] for r in rs] for rs in refs], dtype=np.int32).reshape(len(mols), K) for k in CONF_KEYS})
    out.update({k: np.asarray([[r[k] for r in rs] for rs in refs], dtype=np.float64).reshape(len(mols), K) for k in VALUE_KEYS})
    out['n_atoms'] = np.asarray([b['n_atoms'] for b in bs], dtype=np.int32).reshape(len(mols))
    out['atom_ptr'] = np.concatenate([[0], np.cumsum(out['n_atoms'])])[:len(mols)].astype(np.int32)
    N = int(out['n_atoms'].sum())
    out['pos'] = np.stack([np.concatenate([rs[c]['pos'] for rs in refs] + [np.zeros((0, 3))]) for c in range(K)]).reshape(K, N, 3)
    out['h_pos'] = np.stack([np.concatenate([rs[c]['h_pos'] for rs in refs] + [np.zeros((0, MAX_H, 3))]) for c in range(K)]).reshape(K, N, MAX_H, 3)
    return out


# ---- the device path ------------------------------------------------------------------------------------------------------------------

def launch(cm, order, h_count, atom_flag, n_confs=DEFAULT_N_CONFS, seed=0, tables=None, mol_ids=None, select=None, na_cap=None,
           max_iters=DEFAULT_MAX_ITERS, max_attempts=DEFAULT_MAX_ATTEMPTS, gtol=DEFAULT_GTOL, max_step=DEFAULT_MAX_STEP, viol_tol=DEFAULT_VIOL_TOL,
           tol12=DEFAULT_TOL12, tol13=DEFAULT_TOL13, tol14=DEFAULT_TOL14, vdw_scale=DEFAULT_VDW_SCALE, keep_bounds=False):
    """``mdx_mol_bounds`` and ``mdx_mol_embed`` on the device arrays `cm` (a ``CompactMols``), `order` (int32, Eh_stride) and `h_count`,
    `atom_flag` (int32, N_cap) of ``kekule.launch`` / ``hydrogens.launch`` -> dict of device tensors: ``bounds_<key>`` (B) for BOUNDS_KEYS,
    the keys of CONF_KEYS (B, K; int32) and of VALUE_KEYS (B, K; float64), ``pos`` (K, N_cap, 3) and ``h_pos`` (K, N_cap, 4, 3) float64: slice
    c is what ``relax.launch`` takes as `h_pos` and, ROUNDED ONCE to float32 by the caller (``global3d_mols`` does it), as ``atom_pos``.
    na_cap: the stride of the bounds (None: 256; a smaller one saves memory, a molecule above it is TOO_LARGE).  keep_bounds: also
    ``lower`` / ``upper`` (B, na_cap, na_cap) float64 and ``cls`` (uint8).  mol_ids: int64 (B) ids that key the random numbers (None: the
    index in the batch).  No sync."""
    import torch
    from . import _lib
    tb = relax._tables(tables)
    K, max_iters, max_attempts, gtol, max_step, viol_tol = _check_embed(n_confs, max_iters, max_attempts, gtol, max_step, viol_tol)
    tol12, tol13, tol14, vdw_scale, cap = _check_bounds(tol12, tol13, tol14, vdw_scale, MAX_ATOMS if na_cap is None else na_cap)
    B, N, dev = cm.B, max(cm.N_cap, 1), cm.device
    bstats = torch.zeros(B, len(BOUNDS_KEYS), dtype=torch.int32, device=dev)
    cstats = torch.zeros(B, K, len(CONF_KEYS), dtype=torch.int32, device=dev)
    values = torch.zeros(B, K, len(VALUE_KEYS), dtype=torch.float64, device=dev)
    out = {'pos': torch.zeros(K, N, 3, dtype=torch.float64, device=dev), 'h_pos': torch.zeros(K, N, MAX_H, 3, dtype=torch.float64, device=dev)}
    ws = torch.zeros(max(17 * B * cap * cap, 8), dtype=torch.uint8, device=dev)
    if B > 0:
        if (order.dtype != torch.int32 or h_count.dtype != torch.int32 or atom_flag.dtype != torch.int32 or order.numel() < cm.Eh_stride or
                h_count.numel() < cm.N_cap or atom_flag.numel() < cm.N_cap):
            raise ValueError('order, h_count and atom_flag are int32 tensors in the layout of the compact arrays')
        if mol_ids is not None and (mol_ids.dtype != torch.int64 or mol_ids.numel() < B):
            raise ValueError('mol_ids is an int64 tensor with one id per molecule')
        order, h_count, atom_flag = order.contiguous(), h_count.contiguous(), atom_flag.contiguous()
        hist = torch.empty(B * K * HIST_PER_ATOM * cap, dtype=torch.float64, device=dev)
        ops, at = cm.operands()
        L = _lib.lib()
        _lib.check(L.mdx_mol_bounds(*ops, _lib.ptr(select), at(order), at(h_count), at(atom_flag), len(tb.atomic_numbers), tb.num_bond_types,
                                    tb.rows.ctypes.data, len(tb.rows), tol12, tol13, tol14, vdw_scale, cap, at(ws), ws.numel(), at(bstats), _lib.stream()))
        _lib.check(L.mdx_mol_embed(*ops, _lib.ptr(select), at(h_count), _lib.ptr(mol_ids), at(ws), ws.numel(), cap, at(bstats), K, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                   max_iters, max_attempts, gtol, max_step, viol_tol, at(out['pos']), at(out['h_pos']), at(cstats), at(values), at(hist),
                                   hist.numel() * 8, _lib.stream()))
    out.update({'bounds_' + k: bstats[:, q] for q, k in enumerate(BOUNDS_KEYS)})
    out.update({k: cstats[:, :, q] for q, k in enumerate(CONF_KEYS)})
    out.update({k: values[:, :, q] for q, k in enumerate(VALUE_KEYS)})
    if keep_bounds:
        planes = ws[:16 * B * cap * cap].view(torch.float64).reshape(B, 2, cap, cap)
        out.update(lower=planes[:, 0], upper=planes[:, 1], cls=ws[16 * B * cap * cap:17 * B * cap * cap].reshape(B, cap, cap))
    return out


def _cap(n_all_most):
    return min(MAX_ATOMS, max(8, -(-int(n_all_most) // 8) * 8))


def embed_mols(mols, device, n_confs=DEFAULT_N_CONFS, seed=0, tables=None, inputs=None, mol_ids=None, with_inputs=False, **kw):
    """Conformers of a list of molecule dicts on the device: the list is packed densely and handed to ``mdx_mol_kekulize``,
    ``mdx_mol_hydrogens`` (default chemistry; they need ``atom_pos``, which the embedding itself never reads), ``mdx_mol_bounds`` and
    ``mdx_mol_embed``.  inputs: per molecule (order, h_count, h_pos, atom_flag) to embed the caller's hydrogens instead (h_pos is not
    read).  -> the results dict of ``launch`` with ``n_atoms`` and ``atom_ptr`` and the per-atom arrays cut to the atoms of the list;
    with `with_inputs` -> (packed host arrays, the ``CompactMols``, (order, h_pos, h_count, atom_flag) device tensors, that)."""
    import torch
    tb = relax._tables(tables)
    p, cm = molpack.packed(mols, tb.atomic_numbers, device, positions=inputs is None)
    if inputs is None:
        kek = kekule.launch(cm, kekule.KekuleTables(tb.atomic_numbers, tb.num_bond_types))
        hyd = hydrogens.launch(cm, kek['kek_h'], kek['kek_order'], hydrogens.HydrogenTables(tb.atomic_numbers, tb.num_bond_types))
        ops = (kek['kek_order'], hyd['h_pos'], hyd['h_count'], hyd['atom_flag'])
    else:
        if len(inputs) != len(mols):
            raise ValueError('one (order, h_count, h_pos, atom_flag) per molecule')
        N, E = max(cm.N_cap, 1), max(cm.Eh_stride, 1)
        full = {'order': np.zeros(E, dtype=np.int32), 'h_count': np.zeros(N, dtype=np.int32), 'atom_flag': np.zeros(N, dtype=np.int32),
                'h_pos': np.zeros((N, MAX_H, 3), dtype=np.float64)}
        for m, (o, hc, hp, fl) in enumerate(inputs):
            a0, na, b0, nb = int(p['atom_ptr'][m]), int(p['n_atoms'][m]), int(p['bond_ptr'][m]), int(p['n_bonds'][m])
            full['order'][b0:b0 + nb] = np.asarray(o, dtype=np.int32).reshape(nb)
            full['h_count'][a0:a0 + na], full['atom_flag'][a0:a0 + na] = np.asarray(hc).reshape(na), np.asarray(fl).reshape(na)
        d = {k: torch.from_numpy(v).to(cm.device) for k, v in full.items()}
        ops = (d['order'], d['h_pos'], d['h_count'], d['atom_flag'])
    if kw.get('na_cap') is None and cm.B:                              # the smallest stride (a multiple of 8) that holds every molecule
        hc = np.clip(molpack.host(ops[2]).reshape(-1), 0, MAX_H)
        n_all = [int(n) + int(hc[int(a0):int(a0) + int(n)].sum()) for a0, n in zip(p['atom_ptr'], p['n_atoms'])]
        kw['na_cap'] = _cap(min(max(n_all), MAX_ATOMS))
    if mol_ids is not None and (len(mol_ids) != len(mols) or any(not 0 <= int(i) < 1 << 56 for i in mol_ids)):
        raise ValueError('mol_ids holds one id per molecule, each in 0 .. 2^56 - 1 (only those bits key the random numbers)')
    ids = None if mol_ids is None else torch.as_tensor(np.asarray(mol_ids, dtype=np.int64)).to(cm.device)
    res = launch(cm, ops[0], ops[2], ops[3], n_confs, seed, tb, ids, **kw)
    res['pos'], res['h_pos'] = res['pos'][:, :cm.N_cap], res['h_pos'][:, :cm.N_cap]
    res['n_atoms'], res['atom_ptr'] = cm.n_atoms, cm.atom_ptr
    if with_inputs:
        return p, cm, ops, res
    return res


# ---- the numbers ---------------------------------------------------------------------------------------------------------------------

def spread(msd, ok):
    """the reference's three numbers over the conformers of every molecule: msd (B, K) mean square deviations, ok (B, K) which
    conformers count -> dict of (B) arrays ``rmsd_max`` / ``rmsd_min`` / ``rmsd_median`` (NaN without a conformer) and ``n_matched``: what
    ``rmsd.global_3d`` computes over its matched targets"""
    msd, ok = np.asarray(msd, dtype=np.float64), np.asarray(ok, dtype=bool)
    pairs = dict(msd=msd.reshape(-1), pair_status=np.where(ok.reshape(-1), 0, 1).astype(np.int32),
                 pair_ptr=np.arange(msd.shape[0] + 1, dtype=np.int64) * (msd.shape[1] if msd.ndim == 2 else 0))
    from . import rmsd
    return rmsd._spread(pairs, msd.shape[0])


MOL_KEYS_G3D = ('rmsd_max', 'rmsd_min', 'rmsd_median', 'n_matched', 'mirror_rmsd_max', 'mirror_rmsd_min', 'mirror_rmsd_median', 'msd', 'msd_mirror', 'ok',
                'relax_status', 'pair_status', 'n_atoms') + tuple('bounds_' + k for k in BOUNDS_KEYS) + CONF_KEYS + VALUE_KEYS
ATOM_KEYS_G3D = {'pos': (3,), 'h_pos': (MAX_H, 3), 'embed_pos': (3,), 'embed_h_pos': (MAX_H, 3)}    # (K, atoms) + these: the atom axis is axis 1


def global3d_mols(mols, device, n_confs=DEFAULT_N_CONFS, seed=0, tables=None, relax_iters=relax.DEFAULT_MAX_ITERS, relax_gtol=relax.DEFAULT_GTOL, **kw):
    """The reference's ``global_3d`` of every molecule of a list (dicts with ``atom_pos``) on the device: kekulize -> hydrogens -> bounds
    -> embed -> relax (every conformer its own batch entry; the embedded heavy-atom positions are ROUNDED ONCE to float32 here, because
    ``mdx_mol_relax`` takes float32) -> canon -> bestrms of the heavy atoms of every relaxed conformer against the generated molecule.
    kw: the settings of ``embed_mols`` (``mol_ids`` among them).  -> one flat dict of host arrays (what ``molpack.save_npz`` stores):
    ``rmsd_max`` / ``rmsd_min`` / ``rmsd_median`` (B; over the conformers with embed status OK, relax status OK and pair status OK; NaN
    without one), ``n_matched``, the same over the mirror-image deviations as ``mirror_rmsd_max`` / ``_min`` / ``_median``; ``msd`` /
    ``msd_mirror`` / ``ok`` / ``relax_status`` / ``pair_status`` (B, K); the embed results (``bounds_<key>`` (B), the keys of CONF_KEYS and
    VALUE_KEYS (B, K), ``embed_pos`` (K, N, 3), ``embed_h_pos`` (K, N, 4, 3)); the relaxed ``pos`` (K, N, 3) and ``h_pos`` (K, N, 4, 3);
    ``n_atoms`` and ``atom_ptr`` (B).  STEREOCENTRES ARE NOT CONSTRAINED: an embedded conformer may be the mirror image of the generated
    molecule, in which case ``msd`` is large and ``msd_mirror`` small; both are reported and neither is chosen.  The conformers are
    relaxed and aligned one conformer index at a time (K launches of each kernel, one copy to the host at the end); a conformer that
    was not embedded is relaxed from zeros and masked out by ``ok``.  Memory: the embedding's history takes B x K x 64 x na_cap doubles
    (na_cap: the largest n_all of the list rounded up to 8).  This project's own model, not ETKDG + UFF."""
    import torch
    from . import canon, rmsd
    tb = relax._tables(tables)
    K = _check_embed(n_confs, 0, 1, 1.0, 1.0, 1.0)[0]
    p, cm, ops, emb = embed_mols(mols, device, K, seed, tb, with_inputs=True, **kw)
    order, _, h_count, flag = ops
    B, N = len(mols), cm.N_cap
    held = []
    if B:
        c0 = canon.launch(cm)
        ptr = torch.arange(B + 1, dtype=torch.int32, device=cm.device)
        tgt = torch.arange(B, dtype=torch.int32, device=cm.device)
        for c in range(K):
            moved = cm._replace(atom_pos=emb['pos'][c].to(torch.float32).contiguous())     # the one rounding
            rel = relax.launch(moved, order, emb['h_pos'][c].contiguous(), h_count, flag, tb, relax_iters, relax_gtol)
            target = cm._replace(atom_pos=rel['pos'][:max(N, 1)].to(torch.float32).contiguous())
            ct = canon.launch(target)
            pr = rmsd.launch(cm, c0, {'atom_ptr': cm.atom_ptr, 'n_atoms': cm.n_atoms, 'canon_pos': ct['canon_pos']}, ptr, tgt)
            held.append({'msd': pr['msd'], 'msd_mirror': pr['msd_mirror'], 'pair_status': pr['pair_status'], 'relax_status': rel['status'],
                         'pos': rel['pos'][:N], 'h_pos': rel['h_pos'][:N]})
    e = to_host(dict(emb))
    held = [to_host(h) for h in held]
    col = lambda k, dt: np.stack([h[k] for h in held], axis=1).astype(dt) if B else np.zeros((0, K), dtype=dt)
    msd, mir, pstat, rstat = col('msd', np.float64), col('msd_mirror', np.float64), col('pair_status', np.int32), col('relax_status', np.int32)
    ok = (e['status'].reshape(B, K) == STATUS_OK) & (rstat == relax.STATUS_OK) & (pstat == rmsd.STATUS_OK)
    out = spread(msd, ok)
    out.update({'mirror_' + k: v for k, v in spread(mir, ok).items() if k != 'n_matched'})
    out.update(msd=msd, msd_mirror=mir, ok=ok, relax_status=rstat, pair_status=pstat)
    out.update({k: e[k] for k in tuple('bounds_' + b for b in BOUNDS_KEYS) + CONF_KEYS + VALUE_KEYS})
    out['n_atoms'], out['atom_ptr'] = e['n_atoms'].astype(np.int32), e['atom_ptr'].astype(np.int32)
    out['embed_pos'], out['embed_h_pos'] = e['pos'].reshape(K, N, 3), e['h_pos'].reshape(K, N, MAX_H, 3)
    out['pos'] = np.stack([h['pos'] for h in held]).reshape(K, N, 3) if B else np.zeros((K, 0, 3))
    out['h_pos'] = np.stack([h['h_pos'] for h in held]).reshape(K, N, MAX_H, 3) if B else np.zeros((K, 0, MAX_H, 3))
    return out


def empty(n_confs=DEFAULT_N_CONFS):
    """the ``global3d_mols`` result of no molecule"""
    K = _check_embed(n_confs, 0, 1, 1.0, 1.0, 1.0)[0]
    out = spread(np.zeros((0, K)), np.zeros((0, K), dtype=bool))
    out.update({'mirror_' + k: v for k, v in spread(np.zeros((0, K)), np.zeros((0, K), dtype=bool)).items() if k != 'n_matched'})
    out.update(msd=np.zeros((0, K)), msd_mirror=np.zeros((0, K)), ok=np.zeros((0, K), dtype=bool), relax_status=np.zeros((0, K), dtype=np.int32),
               pair_status=np.zeros((0, K), dtype=np.int32), n_atoms=np.zeros(0, dtype=np.int32), atom_ptr=np.zeros(0, dtype=np.int32))
    out.update({'bounds_' + k: np.zeros(0, dtype=np.int32) for k in BOUNDS_KEYS})
    out.update({k: np.zeros((0, K), dtype=np.int32) for k in CONF_KEYS})
    out.update({k: np.zeros((0, K), dtype=np.float64) for k in VALUE_KEYS})
    out.update({k: np.zeros((K, 0) + s, dtype=np.float64) for k, s in ATOM_KEYS_G3D.items()})
    return out


def concat(parts):
    """the ``global3d_mols`` results of consecutive batches (the same number of conformers in each) as one"""
    parts = [to_host(p) for p in parts]
    out = {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in MOL_KEYS_G3D}
    out.update({k: np.concatenate([np.asarray(p[k]) for p in parts], axis=1) for k in ATOM_KEYS_G3D})
    out['atom_ptr'] = (np.cumsum(out['n_atoms'].astype(np.int64)) - out['n_atoms']).astype(np.int32)
    return out


def write_sdf(path, mols, kek_results, h_results, results):
    """every conformer that counts (``ok``) of the kekulizable molecules of `mols` as an all-atom mol block at its relaxed coordinates,
    molecule by molecule (kek_results, h_results: the results of ``kekule`` and ``hydrogens`` on the same list, host or device arrays;
    results: those of ``global3d_mols``) -> how many were written"""
    kr, hr, written = to_host(kek_results), to_host(h_results), 0
    keep = kekule.kekulizable(kr)
    with open(path, 'w') as f:
        for m, info in enumerate(mols):
            kres, hres = kekule.mol_result(kr, m), hydrogens.mol_result(hr, m)
            a0, n = int(results['atom_ptr'][m]), int(results['n_atoms'][m])
            if not keep[m] or not (kres['kek_order'] >= 1).all():
                continue
            for c in np.flatnonzero(np.asarray(results['ok'][m])):
                moved = dict(info, atom_pos=np.asarray(results['pos'][c, a0:a0 + n]))
                try:
                    block = hydrogens.allatom_mol_block(moved, kres, dict(hres, h_pos=np.asarray(results['h_pos'][c, a0:a0 + n])))
                except ValueError:
                    continue
                f.write(block + '$$$$\n')
                written += 1
    return written


def summary(results):
    """the numbers of a ``global3d_mols`` result -> dict: ``n_molecules``, ``n_conformers`` (per molecule), ``n_measured`` (at least one
    conformer), the share of embed statuses over all (molecule, conformer) slots, ``mean_attempts``, the mean / median of ``rmsd_median``
    and ``rmsd_min`` and of their mirror counterparts, and ``rmsd_median_hist`` (40 bins of 0.1 Angstrom).  Stereocentres are not
    constrained, so a conformer may be the mirror image: compare the plain and the mirror numbers.  This project's own model, not
    ETKDG + UFF."""
    r = results
    st = np.asarray(r['status']).reshape(-1)
    nan = float('nan')
    share = lambda s: float((st == s).sum()) / len(st) if len(st) else nan
    fin = lambda v: np.asarray(v, dtype=np.float64)[np.isfinite(np.asarray(v, dtype=np.float64))]
    stat = lambda v, f: float(f(fin(v))) if len(fin(v)) else nan
    return {'n_molecules': int(len(r['rmsd_max'])), 'n_conformers': int(np.asarray(r['msd']).shape[1]), 'n_measured': int((np.asarray(r['n_matched']) > 0).sum()),
            'fraction_ok': share(STATUS_OK), 'fraction_failed': share(STATUS_FAILED), 'fraction_inconsistent': share(STATUS_INCONSISTENT),
            'fraction_too_large': share(STATUS_TOO_LARGE), 'mean_attempts': stat(np.asarray(r['attempts'], dtype=np.float64).reshape(-1), np.mean),
            'rmsd_median_mean': stat(r['rmsd_median'], np.mean), 'rmsd_median_median': stat(r['rmsd_median'], np.median),
            'rmsd_min_mean': stat(r['rmsd_min'], np.mean), 'mirror_rmsd_median_mean': stat(r['mirror_rmsd_median'], np.mean),
            'mirror_rmsd_min_mean': stat(r['mirror_rmsd_min'], np.mean), 'rmsd_median_hist': relax._hist(fin(r['rmsd_median']), RMSD_MAX, RMSD_BINS)}


def compare(a, b):
    """two ``global3d_mols`` results or two summaries -> Jensen-Shannon divergence (base 2, ``molpack.jsd_counts``) of ``rmsd_median_hist``
    and both sides' ``fraction_ok`` and ``rmsd_median_median``"""
    a, b = (x if 'rmsd_median_hist' in x else summary(x) for x in (a, b))
    return {'rmsd_median': jsd_counts(a['rmsd_median_hist'], b['rmsd_median_hist']), 'fraction_ok': [a['fraction_ok'], b['fraction_ok']],
            'rmsd_median_median': [a['rmsd_median_median'], b['rmsd_median_median']]}


def main(argv=None):
    def run(mols, args, device):
        if device is None:
            raise SystemExit('the global_3d chain runs on the device only; embed_ref is the restatement of its embedding stage')
        ids = [int(m.get('mol_id', i)) for i, m in enumerate(mols)]
        if not mols:
            return empty(args.confs)
        res = global3d_mols(mols, device, args.confs, args.seed, mol_ids=ids)
        if args.sdf:
            kek, hyd = kekule.kekulize_mols(mols, device), hydrogens.addh_mols(mols, device)
            write_sdf(args.sdf, mols, kek, hyd, res)
        return res
    return molpack.stats_main(
        argv, 'embed', __doc__, ('global_3d (max / min / median best RMSD against generated conformers) of the molecules stored in a samples_all.pt',
                                 'Jensen-Shannon divergence of the median-RMSD distributions of two files'),
        [('--confs', dict(type=int, default=DEFAULT_N_CONFS, help='conformers per molecule')),
         ('--seed', dict(type=int, default=0, help='seed of the starting coordinates')),
         ('--sdf', dict(default=None, help='also write the relaxed conformers that count as all-atom mol blocks'))],
        run, summary, compare)


if __name__ == '__main__':
    sys.exit(main())
