"""GPU test of the staging that the per-molecule evaluation kernels share (csrc/mdx_mol.h: the guard, the bond word, the adjacency as
CSR in LDS), through rings.launch, groups.launch, framework.launch, canon.launch, kekule.launch and hydrogens.launch on ONE batch:
a molecule at the atom limit whose 512 bond slots, valid and ignored ones mixed, fill both strides of the bond loops (e and e + 256),
behind a small molecule (so that its pointers are not 0), before a molecule above the limit (status 1, zeros) and a masked copy of
itself (status 0, zeros).  The oracles are the plain restatements of the six modules; every integer is compared exactly, ``h_pos`` and
``min_contact`` to the bound of tests/test_gpu_hydrogens.py."""
import numpy as np
import pytest
import torch

from moldiff_amd import canon as C
from moldiff_amd import framework as F
from moldiff_amd import groups as G
from moldiff_amd import hydrogens as H
from moldiff_amd import kekule as K
from moldiff_amd import molpack
from moldiff_amd import rings as R
from . import hydrogens_cases as HC
from .test_gpu_hydrogens import TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ELEMENTS = molpack.DEFAULT_ATOMIC_NUMBERS
IGNORED = [(-1, 3), (5, 5), (0, 256), (263, 2)]   # an index below 0, i = j, an index at n, an index past a byte
BIG, MASKED = 1, 3


def big():
    """256 atoms on a path with 40 chords, 295 single bonds in all, and 217 ignored bonds, over the 512 slots in a random order"""
    g = np.random.default_rng(7)
    ele = g.choice([6, 6, 6, 7, 8], 256)
    bonds = [(a, a + 1) for a in range(255)]
    while len(bonds) < 295:
        i, j = sorted(int(x) for x in g.integers(0, 256, 2))
        if j - i >= 3 and (i, j) not in bonds:
            bonds.append((i, j))
    slots = bonds + [IGNORED[k % 4] for k in range(512 - len(bonds))]
    slots = [slots[k] + (1,) for k in g.permutation(512)]
    return HC.mol(ele, g.normal(0, 6, (256, 3)), slots)


@pytest.fixture(scope='module')
def batch():
    mols = [HC.chain(5), big(), HC.chain(257), big()]
    i, j = mols[BIG]['bond_index'][:, :512]
    ignored = ~((i >= 0) & (i < 256) & (j >= 0) & (j < 256) & (i != j))
    assert (int(ignored[:256].sum()), int(ignored[256:].sum())) == (107, 110)
    p = molpack.pack_mols(mols, ELEMENTS, positions=True)
    assert p['atom_ptr'][BIG] == 5 and p['bond_ptr'][BIG] == 4 and p['n_bonds'].tolist() == [4, 512, 256, 512]
    cm = molpack.CompactMols.from_packed(molpack.to_device(p, DEV))
    select = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=DEV)
    return {'mols': mols, 'p': p, 'cm': cm, 'select': select, 'rings': R.launch(cm, len(ELEMENTS), 4, select=select)}


def expected(ref, layout, p, minus_one=()):
    """`ref` (a stack_ref of the batch) with the masked molecule as the kernels leave it: 0 in every per-molecule key but the counts and
    in its atom and bond slots, -1 in the per-atom keys of `minus_one`"""
    ref = {k: v.copy() for k, v in ref.items()}
    lo = {'atom': int(p['atom_ptr'][MASKED]), 'bond': int(p['bond_ptr'][MASKED])}
    hi = {'atom': lo['atom'] + int(p['n_atoms'][MASKED]), 'bond': lo['bond'] + int(p['n_bonds'][MASKED])}
    for k in layout.mol:
        if k not in ('n_atoms', 'n_bonds'):
            ref[k][MASKED] = 0
    for k, per, kind in layout.columns(ref):
        if kind == 'index':
            ref[k][:, lo[per]:hi[per]] = 0
        else:
            ref[k][lo[per]:hi[per]] = -1 if k in minus_one else 0
    return ref


def same(got, want, what, floats=()):
    got = molpack.to_host(got)
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        if k in floats:
            inf = np.isinf(want[k])
            assert np.array_equal(np.isinf(got[k]), inf), (what, k)
            diff = float(np.abs(got[k][~inf] - want[k][~inf]).max(initial=0.0))
            print(what, k, 'max abs diff', diff)
            assert diff <= TOL, (what, k, diff)
        else:
            bad = np.flatnonzero((got[k] != want[k]).reshape(-1))
            assert len(bad) == 0, (what, k, bad[:8], got[k].reshape(-1)[bad[:8]], want[k].reshape(-1)[bad[:8]])


def test_rings(batch):
    ref = R.stack_ref(batch['mols'])
    assert ref['status'].tolist() == [0, 0, 1, 0] and ref['n_rings'].tolist() == [0, 40, 0, 40]
    same(molpack.dense(dict(batch['rings']), batch['cm'], batch['p'], R.LAYOUT), expected(ref, R.LAYOUT, batch['p']), 'rings')


def test_groups(batch):
    pset = G.PatternSet.default()
    ref = G.stack_ref(batch['mols'], pset)
    assert ref['status'].tolist() == [0, 0, 1, 0] and not ref['pat_status'].any() and ref['n_embed'][BIG].any()
    want = expected({k: v for k, v in ref.items() if k not in ('aut', 'names')}, G.LAYOUT, batch['p'])   # the set's own: no device output
    out = G.launch(batch['cm'], pset, select=batch['select'], ring_data=batch['rings'])
    same(molpack.dense(out, batch['cm'], batch['p'], G.LAYOUT), want, 'groups')


def test_framework(batch):
    ref = F.stack_ref(batch['mols'])
    assert ref['status'].tolist() == [0, 0, 1, 0] and ref['n_systems'][BIG] >= 1
    out = F.launch(batch['cm'], batch['rings'], select=batch['select'])
    same(molpack.dense(out, batch['cm'], batch['p'], F.LAYOUT), expected(ref, F.LAYOUT, batch['p'], minus_one=('atom_system',)), 'framework')


def test_canon(batch):
    ref = C.stack_ref(batch['mols'])
    assert ref['status'].tolist() == [0, 0, 1, 0] and ref['n_nodes'][BIG] == 1 and ref['canon_n_bonds'][BIG] == 295
    out = C.launch(batch['cm'], select=batch['select'])
    same(molpack.dense(out, batch['cm'], batch['p'], C.LAYOUT), expected(ref, C.LAYOUT, batch['p'], minus_one=('rank',)), 'canon')


def test_kekule_and_hydrogens(batch):
    mols, p, cm = batch['mols'], batch['p'], batch['cm']
    ref = K.stack_ref(mols)
    assert ref['status'].tolist() == [0, 0, 1, 0]
    kek = K.launch(cm, select=batch['select'])
    same(molpack.dense(dict(kek), cm, p, K.LAYOUT), expected(ref, K.LAYOUT, p), 'kekule')
    # the hydrogens of that assignment
    r = K.kekulize_ref(mols[BIG])
    assert not H.near_threshold(mols[BIG], r['kek_h'], r['kek_order']) and not H.near_threshold(mols[0], *HC.kekule_counts(mols[0]))
    ref = H.stack_ref(mols)
    assert ref['status'].tolist() == [0, 0, 1, 0] and ref['n_h_wanted'][BIG] == 288 and ref['n_h_placed'][BIG] == 288
    want = expected(ref, H.LAYOUT, p)
    a0, na = int(p['atom_ptr'][MASKED]), int(p['n_atoms'][MASKED])
    want['h_pos'][a0:a0 + na] = 0
    want['min_contact'][MASKED] = 0
    out = H.launch(cm, kek['kek_h'], kek['kek_order'], select=batch['select'])
    h_pos, min_contact = out.pop('h_pos')[:cm.N_cap], out.pop('min_contact')
    same(dict(molpack.dense(out, cm, p, H.LAYOUT), h_pos=h_pos, min_contact=min_contact), want, 'hydrogens', floats=H.FLOAT_KEYS)
