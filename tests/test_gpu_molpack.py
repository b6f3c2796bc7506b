"""GPU test of what the four evaluation kernels share (csrc/mdx_mol.h, moldiff_amd/molpack.py): ONE designed list of molecule dicts goes
through ``local3d_mols``, ``fingerprint_mols``, ``rings_mols`` and ``groups_mols`` and every output equals the Python restatement of its
module exactly.  The sizes 64, 65 and 256 are the wave and workgroup boundaries of the shared scan of the degrees; a list without any bond
exercises the shared stand-in for empty tensors.  The last test is about what rings, groups, kekule, canon and framework share on the
output side: the one results table of ``molpack.Layout``.

The geometry histograms are compared exactly too, which the device's fp32 allows because the bins are few and wide: the test asserts, in
float64 on the host, that no matched item lies within 1e-3 (degrees, or length units) of a bin edge -- far more than fp32 rounding of
values of this size moves it."""
import numpy as np
import pytest

from moldiff_amd import canon as C
from moldiff_amd import framework as F
from moldiff_amd import groups as G
from moldiff_amd import kekule as K
from moldiff_amd import local3d as L3
from moldiff_amd import molpack
from moldiff_amd import rings as R
from moldiff_amd import similarity as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = molpack.DEFAULT_ATOMIC_NUMBERS
BINS = dict(length_bins=(0.0, 64.0, 4), angle_bins=(-1, 181, 2), dihedral_bins=(-181, 181, 2))
EDGE_MARGIN = 1e-3


def mol(ele, bonds, seed=0):
    g = np.random.default_rng(seed)
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).reshape(-1, 2).T
    bt = [t for _, _, t in bonds]
    return {'element': np.asarray(ele, dtype=np.int64), 'atom_pos': (2.0 * g.standard_normal((len(ele), 3))).astype(np.float32),
            'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.asarray(bt + bt, dtype=np.int64)}


def connected(seed, n, extra):
    """a random spanning tree plus `extra` further bonds (so `extra` independent rings), random elements and bond types"""
    g = np.random.default_rng(seed)
    bonds = {(int(g.integers(0, k)), k) for k in range(1, n)}
    while len(bonds) < n - 1 + extra:
        i, j = sorted(int(x) for x in g.choice(n, 2, replace=False))
        bonds.add((i, j))
    ele = g.choice(ELEMENTS, n, p=[.7, .1, .1, .02, .02, .04, .02])
    return mol(ele, [(i, j, int(g.choice([1, 2, 3, 4], p=[.6, .1, .05, .25]))) for i, j in sorted(bonds)], seed)


DESIGNED = [mol([7], []),                                                                       # one atom
            mol([6, 8], [(0, 1, 2)]),                                                           # two atoms, one bond
            connected(1, 64, 6), connected(2, 65, 7), connected(3, 256, 20),                    # one wave, one wave + 1, the whole workgroup
            mol([6, 6, 7, 6, 8], [(0, 1, 1), (1, 9, 1), (2, 2, 3), (1, 2, 4), (2, 3, 4), (3, 1, 4), (-1, 0, 2), (3, 4, 1)], 5)]   # ignored bonds
BONDLESS = [mol([6], []), mol([7, 8, 6], [], 1), mol(list(ELEMENTS) * 10, [], 2)]


@pytest.fixture(scope='module')
def l3_spec():
    pats = {k: [p for p, _ in L3.frequent_patterns(DESIGNED, k, 12)] for k in L3.KINDS}
    return L3.Local3DSpec(pats['lengths'], pats['angles'], pats['dihedrals'], **BINS)


def same_results(got, ref, what):
    got = molpack.to_host(got)
    assert set(got) == set(ref), what
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k)


def check_all_four(mols, l3_spec, what):
    # local 3D geometry
    ref = L3.Local3DStats.from_ref(mols, l3_spec)
    for m in mols:
        values = L3.local3d_ref(m, l3_spec)['values']
        for kind in L3.KINDS:
            for v in values[kind]:
                assert np.isfinite(v).all() and (np.abs(v[:, None] - l3_spec.edges(kind)[None, :]) >= EDGE_MARGIN).all(), (what, kind)
    got = L3.local3d_mols(mols, l3_spec, DEV).cpu()
    assert np.array_equal(got.n_items, ref.n_items) and np.array_equal(got.outside, ref.outside) and np.array_equal(got.hist, ref.hist), what
    # fingerprints and keys
    fspec = S.FingerprintSpec(nbits=256)
    got, ref = S.fingerprint_mols(mols, fspec, DEV).cpu(), S.FingerprintSet.from_ref(mols, fspec)
    for k in ('bits', 'n_on', 'key', 'n_atoms'):
        assert np.array_equal(getattr(got, k), getattr(ref, k)), (what, k)
    # rings and composition
    same_results(R.rings_mols(mols, DEV), R.stack_ref(mols), what)
    # functional groups, the default set: it carries ring constraints, so mdx_mol_rings runs first on the same arrays
    pset = G.PatternSet.default()
    assert pset.needs_rings
    same_results(G.groups_mols(mols, DEV, pset), G.stack_ref(mols, pset), what)


def test_one_designed_list_through_all_four_entry_points(l3_spec):
    ref = R.stack_ref(DESIGNED)
    assert ref['n_atoms'].tolist() == [1, 2, 64, 65, 256, 5] and ref['n_rings'].tolist() == [0, 0, 6, 7, 20, 1] and not ref['status'].any()
    assert L3.Local3DStats.from_ref(DESIGNED, l3_spec).hist.sum() > 500
    check_all_four(DESIGNED, l3_spec, 'designed')


def test_a_list_without_any_bond_through_all_four_entry_points(l3_spec):
    p = molpack.pack_mols(BONDLESS, ELEMENTS, positions=True)
    assert p['bond_index'].shape == (2, 1) and p['bond_type'].size == 0
    check_all_four(BONDLESS, l3_spec, 'bondless')


def test_the_five_results_tables_match_stack_ref_and_two_batches_concat_to_the_single_run():
    """what rings, groups, kekule, canon and framework share on the output side (molpack.Layout): ``<name>_mols`` of a benzene, a
    two-atom molecule and a single atom without bonds has exactly the keys, dtypes and shapes (and values) of ``stack_ref``, and
    ``concat`` of the list run as two batches (2 + 1) equals the single run"""
    mols = [mol([6] * 6, [(k, (k + 1) % 6, 4) for k in range(6)], 1), mol([6, 8], [(0, 1, 2)], 2), mol([7], [], 3)]
    pset = G.PatternSet.default()
    for mod, run in ((R, lambda ms: R.rings_mols(ms, DEV)), (G, lambda ms: G.groups_mols(ms, DEV, pset)), (K, lambda ms: K.kekulize_mols(ms, DEV)),
                     (C, lambda ms: C.canon_mols(ms, DEV)), (F, lambda ms: F.framework_mols(ms, DEV))):
        whole = molpack.to_host(run(mols))
        same_results(whole, mod.stack_ref(mols), mod.__name__)
        same_results(mod.concat([run(mols[:2]), run(mols[2:])]), whole, mod.__name__ + ' in two batches')
