"""GPU tests of the local 3D geometry statistics (mdx_mol_local3d through local3d.local3d_mols, FeaturizeMol.local3d_batch and the
sampling entry point's --local3d).  The oracle is ``local3d.local3d_ref``: numpy, float64, from the same fp32 coordinates.

Exact comparison against a float64 oracle needs inputs whose values keep clear of the bin edges.  The fp32 error model of the device
forms, eps = 2^-24: a coordinate difference is exact or off by eps * |coordinate| (below 16 here) on a bond of at least 0.5, at most
32 eps relative per component; a cross product adds about 3 eps |u| |v|, which is 3 eps / sin(angle) relative to its own length; the
atan2f forms return the angle between such vectors, whose error is the sum of their direction errors plus atan2f's own few ulp.  With
every bond >= 0.5 long and every bond angle's sine >= 0.1 that is below about 100 eps = 6e-6 rad = 3.4e-4 degrees for a dihedral in the
worst case and about 30 eps = 1e-4 degrees for typical items, and a few eps relative for a length.  The margins
used are DELTA_LEN = 1e-4 relative for lengths and DELTA_DEG = 1e-3 degrees for angles: 3 times the worst case and about
30 times the typical one, and a thousandth of a 1-degree bin.  Coordinates are drawn atom by atom: an atom is redrawn on the host until
every item it completes meets the conditions, so NO item is left out; the fixture asserts that on the finished batch before anything
goes to the GPU.  Under these conditions hist, outside and n_items must equal the oracle exactly.
"""
import os

import numpy as np
import pytest
import torch

from moldiff_amd import _lib, molpack
from moldiff_amd import local3d as L3
from moldiff_amd.harness import placeholder_from_sizes
from moldiff_amd.postprocess import FeaturizeMol

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = (6, 7, 8, 9, 15, 16, 17)
FEAT = FeaturizeMol(list(ELEMENTS), [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
DELTA_LEN, DELTA_DEG = 1e-4, 1e-3
# the coarse bins (1 degree, 0.01 A) and the fine ones (twice as many): every coarse edge is a fine edge
COARSE = dict(length_bins=(1.0, 2.2, 120), angle_bins=(0, 180, 180), dihedral_bins=(-180, 180, 360))
FINE = dict(length_bins=(1.0, 2.2, 240), angle_bins=(0, 180, 360), dihedral_bins=(-180, 180, 720))


def mol(ele, bonds, pos):
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'atom_pos': np.asarray(pos, dtype=np.float32).reshape(len(ele), 3),
            'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def edge_distance(spec, kind, v):
    """distance of float64 values to the nearest bin edge of `kind` (lo and hi included), in the value's unit"""
    lo, hi, n = spec.bins[kind]
    w = (hi - lo) / n
    k = np.clip(np.round((v - lo) / w), 0, n)
    return np.abs(v - (lo + k * w))


def well_conditioned(spec, kind, pos, atoms):
    """the conditions of the module docstring for items of one kind (float64) -> bool per item"""
    v = L3.item_values(pos, kind, atoms)
    if kind == 'lengths':
        return (v >= 0.5) & (edge_distance(spec, kind, v) >= DELTA_LEN * v)
    ok = edge_distance(spec, kind, v) >= DELTA_DEG
    if kind == 'angles':
        ok &= np.sin(np.radians(v)) >= 0.1
    return ok


def conditioned_mol(seed, n, n_bonds, spec, sigma=2.0, even=False):
    """random molecule: all 7 elements, `n_bonds` distinct random bonds of types 1-4, coordinates drawn atom by atom so that every
    item meets the conditions (an item is complete once its highest-numbered atom is placed).  even: the bonds join atom p[i] to
    p[i + s] for a random numbering p and n_bonds // n random strides s, the rest are drawn freely -- every atom then has about the
    same number of bonds.  (With freely drawn bonds at 8 per atom a few atoms have 14 and complete some 5,000 dihedrals each: no
    position keeps all of those a thousandth of a bin from every edge.)"""
    g = np.random.default_rng(seed)
    ele = g.choice(ELEMENTS, n, p=[.4, .2, .15, .05, .05, .1, .05])
    iu, ju = np.triu_indices(n, 1)
    code = iu * n + ju
    if even:
        p = g.permutation(n)
        strides = g.choice(np.arange(1, n // 2), n_bonds // n, replace=False)
        a, b = np.repeat(p[None], len(strides), 0), np.stack([np.roll(p, -int(s)) for s in strides])
        fixed = np.unique(np.minimum(a, b).ravel() * n + np.maximum(a, b).ravel())
        assert len(fixed) == n * len(strides)
        free = np.setdiff1d(code, fixed)
        pick = np.searchsorted(code, np.concatenate([fixed, g.choice(free, n_bonds - len(fixed), replace=False)]))
        pick = g.permutation(pick)
    else:
        pick = g.choice(iu.shape[0], min(n_bonds, iu.shape[0]), replace=False)
    bonds = [(int(iu[k]), int(ju[k]), int(g.choice([1, 2, 3, 4], p=[.45, .15, .05, .35]))) for k in pick]
    m = mol(ele, bonds, np.zeros((n, 3)))
    items = {k: a for k, (a, _) in L3.enumerate_items(m).items()}
    last = {k: (a.max(1) if len(a) else np.zeros(0, dtype=np.int64)) for k, a in items.items()}
    pos = np.zeros((n, 3), dtype=np.float32)
    for i in range(n):
        mine = {k: items[k][last[k] == i] for k in L3.KINDS}
        for _ in range(20000):
            pos[i] = (sigma * g.standard_normal(3)).astype(np.float32)
            if all(well_conditioned(spec, k, pos, a).all() for k, a in mine.items() if len(a)):
                break
        else:
            raise AssertionError(f'no well-conditioned position for atom {i} of seed {seed}')
    m['atom_pos'] = pos
    return m


def all_conditions_hold(mols, spec):
    for m in mols:
        for kind, (atoms, _) in L3.enumerate_items(m).items():
            if len(atoms) and not well_conditioned(spec, kind, m['atom_pos'], atoms).all():
                return False
    return True


def spec_from(mols, top, bins, extra=True):
    """patterns from frequent_patterns on the batch itself, plus one per kind that never occurs (F#F...)"""
    pats = {k: [p for p, _ in L3.frequent_patterns(mols, k, t)] for k, t in zip(L3.KINDS, top)}
    if extra:
        for k, w in zip(L3.KINDS, (3, 5, 7)):
            never = tuple(9 if i % 2 == 0 else 3 for i in range(w))
            assert never not in pats[k]
            pats[k].append(never)
    return L3.Local3DSpec(pats['lengths'], pats['angles'], pats['dihedrals'], **bins)


def oracle(mols, spec):
    refs = [L3.local3d_ref(m, spec) for m in mols]
    return refs, L3.Local3DStats(spec, sum((r['hist'] for r in refs), np.zeros(spec.hist_size, dtype=np.int64)),
                                 sum((r['outside'] for r in refs), np.zeros(spec.kind_ptr[3], dtype=np.int64)),
                                 sum((r['n_items'] for r in refs), np.zeros(3, dtype=np.int64)))


def same(got, want, what=''):
    g = got.cpu()
    assert np.array_equal(g.n_items, want.n_items), (what, g.n_items, want.n_items)
    assert np.array_equal(g.outside, want.outside), (what, np.flatnonzero(g.outside != want.outside))
    bad = np.flatnonzero(g.hist != want.hist)
    assert bad.size == 0, (what, bad[:10], g.hist[bad[:10]], want.hist[bad[:10]])


# ---- 1. designed molecules, exact bins ----------------------------------------------------------------------------------------------

CHAIN_POS = [[1, 0, 0], [0, 0, 0], [0, 0, 1], [0, 1, 1]]
DESIGNED = [mol([6, 6, 7, 8], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], CHAIN_POS),                               # dihedral +90
            mol([8, 7, 6, 6], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], CHAIN_POS[::-1]),                         # the same, renumbered
            mol([6, 6, 7, 8], [(0, 1, 1), (1, 2, 2), (2, 3, 1)], np.asarray(CHAIN_POS) * [1, -1, 1]),      # its mirror image: -90
            mol([6, 6, 6], [(0, 1, 1), (1, 2, 1), (0, 2, 1)], [[0, 0, 0], [1, 0, 0], [0, 1, 0]]),           # triangle: no dihedral
            mol([6, 6, 6, 6], [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)], [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]),
            mol([6, 7, 8], [], [[0, 0, 0], [1, 0, 0], [0, 1, 0]]),                                          # no bond
            mol([6], [], [[0, 0, 0]]),                                                                      # one atom
            mol([6, 6], [(0, 1, 1)], [[0, 0, 0], [0, 0, 1]])]                                               # two atoms


def test_designed_molecules_exact_bins():
    # every value sits at a bin centre: lengths 1 and sqrt 2 with bins of sqrt 2 - 1 (centres 1 - w, 1, 1 + w, 1 + 2 w), angles 45 and 90
    # with bins of 15 degrees from -7.5 (centres 0, 15, ..., 180), dihedrals 0 and +-90 with bins of 10 degrees from -185
    w = np.sqrt(2.0) - 1.0
    spec = L3.Local3DSpec(lengths=['C-C', 'C=N', 'N-O', 'C:C'], angles=['C-C=N', 'C=N-O', 'C-C-C', 'C:C:C'],
                          dihedrals=['C-C=N-O', 'C:C:C:C'], length_bins=(1 - 1.5 * w, 1 + 2.5 * w, 4), angle_bins=(-7.5, 187.5, 13),
                          dihedral_bins=(-185, 185, 37))
    for kind in L3.KINDS:                                              # asserted on the oracle's float64 values: centres within 1e-6 bins
        lo, hi, n = spec.bins[kind]
        for m in DESIGNED:
            for v in L3.local3d_ref(m, spec)['values'][kind]:
                assert np.all(np.abs(((v - lo) / ((hi - lo) / n)) % 1.0 - 0.5) < 1e-6), (kind, v)
    refs, want = oracle(DESIGNED, spec)
    assert [r['n_items'].tolist() for r in refs] == [[3, 2, 1], [3, 2, 1], [3, 2, 1], [3, 3, 0], [4, 4, 4], [0, 0, 0], [0, 0, 0], [1, 0, 0]]
    got = L3.local3d_mols(DESIGNED, spec, DEV)
    same(got, want)
    per = got.last_n_items.cpu().numpy().T
    assert per.tolist() == [r['n_items'].tolist() for r in refs]
    assert got.counts('dihedrals', 'C-C=N-O').nonzero()[0].tolist() == [9, 27] and got.counts('dihedrals', 'O-N=C-C')[27] == 2
    assert got.counts('dihedrals', 'C:C:C:C')[18] == 4 and got.counts('angles', 'C:C:C')[6] == 4
    assert got.counts('angles', 'C-C-C').nonzero()[0].tolist() == [3, 6] and got.counts('angles', 'C-C-C')[3] == 2     # 45, 45, 90
    assert got.counts('lengths', 'C-C').nonzero()[0].tolist() == [1, 2] and got.counts('lengths', 'C:C')[1] == 4
    assert got.cpu().outside.sum() == 0


# ---- 2. random molecules against the oracle -------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def batch():
    """sizes {1, 2, 3, 4, 17, 64, 65}, one molecule of 513 atoms and one of 512 atoms with 2,050 bonds (each beyond one of the two LDS
    limits); conditioned against the FINE edges, which include the coarse ones"""
    probe = L3.Local3DSpec(**FINE)
    mols = [conditioned_mol(100 + n, n, int(1.3 * n), probe) for n in (1, 2, 3, 4, 17, 64, 65)]
    mols.append(conditioned_mol(513, 513, 700, probe, sigma=2.5))
    mols.append(conditioned_mol(512, 512, 2050, probe, sigma=2.5, even=True))
    assert all_conditions_hold(mols, probe) and all_conditions_hold(mols, L3.Local3DSpec(**COARSE))   # asserted, never skipped on
    assert [len(m['element']) for m in mols[-2:]] == [513, 512] and mols[-1]['bond_index'].shape[1] // 2 == 2050 > 2048
    assert np.abs(np.concatenate([m['atom_pos'] for m in mols])).max() < 16
    spec = spec_from(mols, (8, 6, 6), COARSE)
    assert spec.hist_size <= 8192                                     # counted in LDS
    refs, want = oracle(mols, spec)
    return mols, spec, refs, want


def test_random_molecules_equal_the_oracle(batch):
    mols, spec, refs, want = batch
    assert want.hist.sum() > 1000 and want.outside.sum() > 100 and (want.n_items > want.hist.sum() // 3).all()
    for k in L3.KINDS:                                                 # the added pattern never occurs
        assert want.counts(k, spec.patterns[k][-1]).sum() == 0
    got = L3.local3d_mols(mols, spec, DEV)
    same(got, want)
    assert got.last_n_items.cpu().numpy().T.tolist() == [r['n_items'].tolist() for r in refs]


# ---- 3. conservation on ill-conditioned input ------------------------------------------------------------------------------------------

def test_conservation_on_collinear_and_coincident_atoms():
    line = mol([6] * 5, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1)], [[0, 0, k] for k in range(5)])              # exactly collinear
    twin = mol([6] * 5, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (3, 4, 1), (1, 3, 1)], [[0, 0, 0], [1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 0]])
    spec = L3.Local3DSpec(lengths=['C-C'], angles=['C-C-C'], dihedrals=['C-C-C-C'], length_bins=(0, 4, 8))
    mols = [line, twin]
    refs, want = oracle(mols, spec)
    got = L3.local3d_mols(mols, spec, DEV).cpu()
    assert np.array_equal(got.n_items, want.n_items) and want.n_items.tolist() == [4 + 5, 3 + 7, 2 + 5]
    for k, kind in enumerate(L3.KINDS):
        items = sum(len(r['values'][kind][0]) for r in refs)
        assert got.counts(kind, spec.patterns[kind][0]).sum() + got.outside[k] == items == want.n_items[k]


# ---- 4. outside and NaN ----------------------------------------------------------------------------------------------------------------

def test_a_cutting_range_and_a_nan_coordinate_land_in_outside(batch):
    mols = batch[0][4:7]                                               # 17, 64, 65 atoms
    spec = spec_from(mols, (4, 3, 3), dict(length_bins=(1.3, 1.9, 60), angle_bins=(60, 120, 60), dihedral_bins=(-90, 90, 180)), extra=False)
    assert all_conditions_hold(mols, spec)                             # these edges are among the fine ones
    _, want = oracle(mols, spec)
    assert (want.outside > 0).all() and want.hist.sum() > 0
    same(L3.local3d_mols(mols, spec, DEV), want)
    _, clean = oracle([mols[0]], spec)
    for atom in range(len(mols[0]['element'])):       # the first atom whose items include binned ones (chosen by the oracle alone)
        poisoned = dict(mols[0], atom_pos=mols[0]['atom_pos'].copy())
        poisoned['atom_pos'][atom, 1] = np.nan       # ONE NaN coordinate
        _, want_nan = oracle([poisoned], spec)
        if want_nan.hist.sum() < clean.hist.sum():
            break
    assert want_nan.outside.sum() > clean.outside.sum() and want_nan.hist.sum() < clean.hist.sum()
    assert want_nan.hist.sum() + want_nan.outside.sum() == clean.hist.sum() + clean.outside.sum()
    same(L3.local3d_mols([poisoned], spec, DEV), want_nan)


# ---- 5. select, accumulation, placement ---------------------------------------------------------------------------------------------------

def _launch(spec, p, out, select=None, pad=0):
    """mdx_mol_local3d on packed numpy arrays `p` (molpack.pack_mols); pad > 0 moves every molecule to an offset of its own with a gap
    after it, like mdx_decode_output's layout (atoms / bonds at the molecule's original offsets, fewer of them than the slots)"""
    if pad:
        na, nb = p['n_atoms'].astype(np.int64), p['n_bonds'].astype(np.int64)
        aptr, bptr = np.concatenate([[0], np.cumsum(na + pad)]), np.concatenate([[0], np.cumsum(nb + 2 * pad)])
        at, ap = np.full(aptr[-1], 99, dtype=np.int32), np.full((aptr[-1], 3), np.nan, dtype=np.float32)
        bt, bi = np.full(bptr[-1], 77, dtype=np.int32), np.full((2, bptr[-1]), -5, dtype=np.int32)
        for m in range(len(na)):
            a0, b0 = int(p['atom_ptr'][m]), int(p['bond_ptr'][m])
            at[aptr[m]:aptr[m] + na[m]], ap[aptr[m]:aptr[m] + na[m]] = p['atom_type'][a0:a0 + na[m]], p['atom_pos'][a0:a0 + na[m]]
            bt[bptr[m]:bptr[m] + nb[m]] = p['bond_type'][b0:b0 + nb[m]]
            bi[:, bptr[m]:bptr[m] + nb[m]] = p['bond_index'][:, b0:b0 + nb[m]]
        p = dict(p, atom_ptr=aptr[:-1].astype(np.int32), bond_ptr=bptr[:-1].astype(np.int32), atom_type=at, atom_pos=ap, bond_type=bt, bond_index=bi)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in p.items()}
    sel = None if select is None else torch.as_tensor(select, dtype=torch.int32, device=DEV)
    return L3.launch(molpack.CompactMols.from_packed(d), spec, out, select=sel)


def test_select_accumulation_and_placement(batch):
    mols, spec, refs, want = batch
    p = molpack.pack_mols(mols, spec.atomic_numbers, positions=True)
    # a masked call equals the oracle over the selected molecules; their n_items are 0
    select = np.array([1, 0, 1, 1, 0, 1, 0, 1, 0], dtype=np.int32)
    got = _launch(spec, p, L3.device_stats(spec, DEV), select)
    same(got, L3.Local3DStats.from_ref([m for m, s in zip(mols, select) if s], spec), 'select')
    per = got.last_n_items.cpu().numpy().T
    assert all((per[m] == (refs[m]['n_items'] if select[m] else 0)).all() for m in range(len(mols)))
    # two calls into one `out` equal the sum
    out = L3.local3d_mols(mols[:5], spec, DEV)
    assert L3.local3d_mols(mols[5:], spec, DEV, out=out) is out
    same(out, want, 'two calls')
    # the batch in permuted molecule order gives bit-identical totals
    whole = L3.local3d_mols(mols, spec, DEV).cpu()
    perm = [mols[k] for k in (8, 2, 5, 0, 7, 3, 6, 1, 4)]
    again = L3.local3d_mols(perm, spec, DEV).cpu()
    assert whole.hist.tobytes() == again.hist.tobytes() and whole.outside.tobytes() == again.outside.tobytes()
    assert whole.n_items.tobytes() == again.n_items.tobytes()
    # int32 pointers of the decode layout (gaps after each molecule, filled with rubbish) and of the dense layout agree
    gaps = _launch(spec, p, L3.device_stats(spec, DEV), pad=7).cpu()
    assert gaps.hist.tobytes() == whole.hist.tobytes() and gaps.outside.tobytes() == whole.outside.tobytes()
    assert gaps.n_items.tobytes() == whole.n_items.tobytes()


# ---- 6. both histogram paths ----------------------------------------------------------------------------------------------------------

def test_lds_and_global_histograms_agree_after_rebinning(batch):
    mols, spec, _, want = batch
    fine = L3.Local3DSpec(spec.patterns['lengths'], spec.patterns['angles'], spec.patterns['dihedrals'], **FINE)
    assert spec.hist_size <= 8192 < fine.hist_size                     # the coarse tables are counted in LDS, the fine ones in global memory
    _, want_fine = oracle(mols, fine)
    got, got_fine = L3.local3d_mols(mols, spec, DEV).cpu(), L3.local3d_mols(mols, fine, DEV).cpu()
    same(got, want, 'lds')
    same(got_fine, want_fine, 'global')
    for kind in L3.KINDS:
        rows = len(spec.patterns[kind])
        merged = got_fine.hist[fine.hist_slice(kind)].reshape(rows, spec.bins[kind][2], 2).sum(-1)
        assert np.array_equal(merged, got.hist[spec.hist_slice(kind)].reshape(rows, -1)), kind
    assert np.array_equal(got.outside, got_fine.outside) and np.array_equal(got.n_items, got_fine.n_items)


# ---- 7. through the public method -----------------------------------------------------------------------------------------------------

def test_local3d_batch_equals_the_oracle_over_decode_batch(batch):
    mols = batch[0][2:6]                                               # 3, 4, 17 and 64 atoms
    mols = [dict(m) for m in mols] + [batch[0][1]]
    spec = spec_from(mols, (6, 5, 5), COARSE)
    cls = {z: i for i, z in enumerate(ELEMENTS)}
    pn, pp, ph = [], [], []
    for k, m in enumerate(mols):
        n = len(m['element'])
        ids = np.asarray([cls[int(z)] for z in m['element']])
        pos = m['atom_pos']
        if k == 2:      # a mask-type atom in front of the 17-atom molecule: the decode drops it and re-indexes the rest
            ids, pos, n = np.concatenate([[7], ids]), np.concatenate([np.zeros((1, 3), dtype=np.float32), pos]), n + 1
        T = np.zeros((n, n), dtype=np.int64)
        shift = 1 if k == 2 else 0
        nb = m['bond_index'].shape[1] // 2
        for (i, j), t in zip(m['bond_index'][:, :nb].T, m['bond_type'][:nb]):
            T[min(i, j) + shift, max(i, j) + shift] = t
        iu, ju = np.triu_indices(n, 1)
        pn.append((10.0 * np.eye(8)[ids]).astype(np.float32)), pp.append(pos.astype(np.float32))
        ph.append((10.0 * np.eye(6)[T[iu, ju]]).astype(np.float32).reshape(-1, 6))
    sizes = [len(x) for x in pn]
    ph_ = placeholder_from_sizes(sizes, DEV)
    pred = [torch.from_numpy(np.concatenate(x)).to(DEV) for x in (pn, pp, ph)]
    args = (pred, ph_['batch_node'], ph_['halfedge_index'], ph_['batch_halfedge'], len(mols))
    decoded = FEAT.decode_batch(*args)
    assert [len(d['element']) for d in decoded] == [len(m['element']) for m in mols]
    assert all_conditions_hold(decoded, spec)                          # the same atoms and bonds, bonds in another order
    want = L3.Local3DStats.from_ref(decoded, spec)
    assert want.hist.sum() > 50
    got = FEAT.local3d_batch(*args, spec)
    same(got, want, 'local3d_batch')
    same(L3.local3d_mols(decoded, spec, DEV), want, 'local3d_mols')
    sel = torch.tensor([1, 1, 0, 1, 1], device=DEV)
    out = FEAT.local3d_batch(*args, spec, select=sel)
    assert FEAT.local3d_batch(*args, spec, select=1 - sel, out=out) is out
    same(out, want, 'select + out')


def test_molecules_without_bonds_and_a_spec_without_patterns():
    """one-atom molecules only (every bond array is empty), no molecule with an atom (the atom arrays are empty too) and a spec
    without a pattern (empty histograms): all are served, and n_items still counts"""
    spec = L3.Local3DSpec(lengths=['C-C'], angles=['C-C-C'])
    for mols in ([DESIGNED[6]] * 3, [mol([], [], np.zeros((0, 3)))] * 2):
        got = L3.local3d_mols(mols, spec, DEV)
        assert got.last_n_items.cpu().tolist() == [[0] * len(mols)] * 3
        got = got.cpu()
        assert got.n_items.tolist() == [0, 0, 0] and got.hist.sum() == 0 and got.outside.sum() == 0
    none = L3.Local3DSpec()
    assert none.hist_size == 0 and none.kind_ptr == [0, 0, 0, 0]
    got = L3.local3d_mols(DESIGNED, none, DEV).cpu()
    assert got.hist.size == 0 and got.outside.size == 0 and got.n_items.tolist() == [17, 13, 7]
    assert np.array_equal(got.n_items, L3.Local3DStats.from_ref(DESIGNED, none).n_items)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    spec = L3.Local3DSpec(lengths=['C-C'], angles=['C-C-C'], dihedrals=['C-C-C-C'])
    p = molpack.pack_mols([DESIGNED[3], DESIGNED[4]], spec.atomic_numbers, positions=True)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
    hist = torch.full((spec.hist_size,), 7, dtype=torch.int64, device=DEV)
    outside, n_items = torch.full((3,), 7, dtype=torch.int64, device=DEV), torch.full((3, 2), 7, dtype=torch.int64, device=DEV)
    need = L.mdx_mol_local3d_ws_bytes(7, 7)
    assert need == 4 * (7 + 2 * 7) and L.mdx_mol_local3d_ws_bytes(0, 0) == 12
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rows, kptr, brange, bcount = (x.copy() for x in spec.table())

    def call(rows=rows, kptr=kptr, brange=brange, bcount=bcount, ws_bytes=need, B=2, **null):
        ptr = lambda name, t: None if null.get(name) else _lib.ptr(t)
        host = lambda name, a: None if null.get(name) else a.ctypes.data
        return L.mdx_mol_local3d(B, ptr('atom_ptr', d['atom_ptr']), ptr('bond_ptr', d['bond_ptr']), ptr('n_atoms', d['n_atoms']),
                                 ptr('n_bonds', d['n_bonds']), ptr('atom_type', d['atom_type']), ptr('atom_pos', d['atom_pos']), 7,
                                 ptr('bond_type', d['bond_type']), ptr('bond_index', d['bond_index']), 7, 7, 4, None,
                                 host('patterns', rows), host('kind_ptr', kptr), host('bin_range', brange), host('bin_count', bcount),
                                 ptr('hist', hist), ptr('outside', outside), ptr('n_items', n_items), _lib.ptr(ws), ws_bytes, _lib.stream())

    ARG, UNSUPPORTED = 1, 4
    for name in ('atom_ptr', 'bond_ptr', 'n_atoms', 'n_bonds', 'atom_type', 'atom_pos', 'bond_type', 'bond_index', 'patterns', 'kind_ptr',
                 'bin_range', 'bin_count', 'hist', 'outside', 'n_items'):
        assert call(**{name: True}) == ARG, name
    assert call(ws_bytes=need - 1) == ARG and b'workspace too small' in L.mdx_last_error()
    assert call(B=-1) == ARG
    many = np.zeros((65, 7), dtype=np.int32)
    many[:, 0], many[:, 1], many[:, 2] = np.arange(65) % 7, 1 + (np.arange(65) // 7) % 4, (np.arange(65) // 28) % 7
    assert call(rows=many, kptr=np.array([0, 65, 65, 65], dtype=np.int32)) == UNSUPPORTED and b'64' in L.mdx_last_error()
    for bad in ([[1.0, 1.0], [0, 180], [-180, 180]], [[1.0, 2.2], [180, 0], [-180, 180]], [[1.0, 2.2], [0, 180], [np.nan, 180]]):
        assert call(brange=np.asarray(bad, dtype=np.float32)) == ARG
    assert call(bcount=np.array([120, 0, 180], dtype=np.int32)) == ARG
    for f, v in ((0, 7), (0, -1), (1, 0), (1, 5), (2, 7)):
        r = rows.copy()
        r[0, f] = v
        assert call(rows=r) == ARG and b'out of range' in L.mdx_last_error(), (f, v)
    twice = np.array([[0, 1, 1, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0]], dtype=np.int32)     # C-N and N-C: one pattern
    assert call(rows=twice, kptr=np.array([0, 2, 2, 2], dtype=np.int32)) == ARG and b'duplicate' in L.mdx_last_error()
    torch.cuda.synchronize()
    assert (hist == 7).all() and (outside == 7).all() and (n_items == 7).all()
    assert call() == 0                                                 # and the same operands, unbroken, are accepted
    torch.cuda.synchronize()
    assert n_items.cpu().tolist() == [[3, 4], [3, 4], [0, 4]] and int(hist.sum()) > 7 * spec.hist_size


# ---- 9. the sampling entry point (recipe weights are synthetic: this tests plumbing, not chemistry) -------------------------------------

def _sample(tmp_path, name, extra):
    from moldiff_amd import sample_drug3d
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log_dir = sample_drug3d.main(['--config', os.path.join(root, 'configs', 'sample_MolDiff_simple.yml'), '--outdir', str(tmp_path / name),
                                  '--device', DEV, '--recipe-weights', '--num_steps', '2', '--num_mols', '6', '--batch_size', '8'] + extra)
    return log_dir, torch.load(os.path.join(log_dir, 'samples_all.pt'), weights_only=False)


def test_entry_point_writes_local3d_npz_of_the_finished_molecules(tmp_path):
    # the seed is sample.seed + sum(ord(outdir)): the two directory names are permutations of each other, so both runs sample the same
    # molecules, and the first run's finished molecules say which patterns the second one will meet
    d0, pool0 = _sample(tmp_path, 'ab', ['--largest_fragment', '0.2'])
    pats = {k: [L3.pattern_text(p) for p, _ in L3.frequent_patterns(pool0['finished'], k, top)] for k, top in zip(L3.KINDS, (6, 4, 3))}
    assert all(pats.values())
    pats['lengths'].append(next(t for t in ('Cl=Cl', 'P=P', 'S#S') if t not in pats['lengths']))   # and one that is rare at best
    pat = tmp_path / 'patterns.yml'
    pat.write_text('lengths: %r\nangles: %r\ndihedrals: %r\ndihedral_bins: [-180, 180, 360]\n' % (pats['lengths'], pats['angles'], pats['dihedrals']))
    d1, pool = _sample(tmp_path, 'ba', ['--largest_fragment', '0.2', '--local3d', str(pat)])
    assert [m['mol_id'] for m in pool['finished']] == [m['mol_id'] for m in pool0['finished']] and len(pool['finished']) > 0
    assert not os.path.exists(os.path.join(d0, 'local3d.npz'))
    assert sorted(os.listdir(d0)) == sorted(f for f in os.listdir(d1) if f != 'local3d.npz')
    got = L3.Local3DStats.load(os.path.join(d1, 'local3d.npz'))
    spec = got.spec
    assert spec == L3.Local3DSpec.from_yaml(str(pat)) and spec.bins['lengths'] == (1.0, 2.2, 120) and spec.bins['dihedrals'][2] == 360
    refs = [L3.local3d_ref(m, spec) for m in pool['finished']]
    want = L3.Local3DStats.from_ref(pool['finished'], spec)
    print('finished', len(pool['finished']), 'items', want.n_items.tolist(), 'binned', int(want.hist.sum()), 'outside', int(want.outside.sum()))
    assert np.array_equal(got.n_items, want.n_items) and want.hist.sum() > 100
    # free-running coordinates: a value the float64 oracle places within delta of an edge may sit in the neighbouring bin (or, at lo /
    # hi, in `outside`); nothing else may move, and such values are at most 1 % of the matched values
    near_total, matched_total = 0, 0
    for k, kind in enumerate(L3.KINDS):
        for r, p in enumerate(spec.patterns[kind]):
            v = np.concatenate([x['values'][kind][r] for x in refs]) if refs else np.zeros(0)
            dist = edge_distance(spec, kind, v)
            near = int((dist < (DELTA_LEN * np.abs(v) if kind == 'lengths' else DELTA_DEG)).sum()) + int(np.isnan(v).sum())
            near_total += near
            matched_total += len(v)
            row = spec.kind_ptr[k] + r
            g, w = got.counts(kind, p), want.counts(kind, p)
            moved = np.abs(g - w).sum() + abs(int(got.outside[row]) - int(want.outside[row]))
            print(f'{kind} {L3.pattern_text(p)}: {len(v)} items, {near} within delta of an edge, {moved // 2} in another bin than the oracle\'s')
            assert g.sum() + got.outside[row] == w.sum() + want.outside[row] == len(v), (kind, p)
            assert moved <= 2 * near, (kind, p, moved, near)
    assert near_total <= 0.01 * matched_total, (near_total, matched_total)      # of the values matched to a pattern
