"""Host tests of the frameworks and ring systems (moldiff_amd/framework.py): ``framework_ref`` against networkx and against the pieces
known by hand, the count identities, invariance under renumbering, the maps back to the molecule, and the set-level numbers."""
import os
import re

import networkx as nx
import numpy as np
import pytest

from moldiff_amd import canon as C
from moldiff_amd import framework as F
from .canon_cases import ELEMENTS, mol, permuted, ring
from .framework_cases import CASES, EXPECTED, sparse_graph
from .util import run_host_check

MEASURED = [k for k, v in EXPECTED.items() if v[0] == 0]
SMALL = [k for k in MEASURED if k != 'fused_256']
_REF = {}


def ref(name, mode=0):
    """framework_ref of a case, computed once"""
    if (name, mode) not in _REF:
        _REF[name, mode] = F.framework_ref(CASES[name], mode)
    return _REF[name, mode]


def graph_of(m):
    n, nb = len(m['element']), m['bond_index'].shape[1] // 2
    G = nx.Graph()
    G.add_nodes_from(range(n))
    for e in range(nb):
        i, j = int(m['bond_index'][0, e]), int(m['bond_index'][1, e])
        if 0 <= i < n and 0 <= j < n and i != j:
            G.add_edge(i, j, e=e, t=int(m['bond_type'][e]))
    return G


def against_networkx(m, what):
    G = graph_of(m)
    n, nb = len(m['element']), m['bond_index'].shape[1] // 2
    core = set(nx.k_core(G, 2).nodes)
    bridges = {frozenset(b) for b in nx.bridges(G)}
    R = nx.Graph([(i, j) for i, j in G.edges if frozenset((i, j)) not in bridges])
    systems = sorted((sorted(c) for c in nx.connected_components(R)), key=lambda c: c[0])
    for mode in range(4):
        r = F.framework_ref(m, mode)
        assert r['status'] == 0, what
        exo = {a for a in G if mode & 1 and a not in core and G.degree(a) == 1 and
               all(G[a][u]['t'] == 2 and u in core for u in G[a])}
        assert {a for a in range(n) if r['atom_role'][a] in (1, 2)} == core, (what, mode)
        assert {a for a in range(n) if r['atom_role'][a] == 2} == set(R.nodes), (what, mode)
        assert {a for a in range(n) if r['atom_role'][a] == 3} == exo, (what, mode)
        want = np.zeros(nb, dtype=np.int64)
        for i, j, d in G.edges(data=True):
            want[d['e']] = 2 if R.has_edge(i, j) else 1 if i in core and j in core else 3 if i in exo or j in exo else 0
        assert r['bond_role'].tolist() == want.tolist(), (what, mode)
        assert r['n_systems'] == len(systems), (what, mode)
        for k, c in enumerate(systems):
            assert np.flatnonzero(r['atom_system'] == k).tolist() == c, (what, mode, k)
            assert (r['sys_n_atoms'][k], r['sys_n_bonds'][k]) == (len(c), R.subgraph(c).number_of_edges())
        assert r['n_fw_atoms'] == len(core) + len(exo) and r['n_fw_bonds'] == G.subgraph(core).number_of_edges() + len(exo)
        assert r['n_fusion'] == sum(R.degree(a) >= 3 for a in R)
        identities(r, what)


def identities(r, what):
    role, n = r['atom_role'], r['n_atoms']
    assert [int((role == k).sum()) for k in range(4)] == [r['n_side'], r['n_linker'], int((r['atom_system'] >= 0).sum()), r['n_exo']], what
    assert r['n_side'] + r['n_fw_atoms'] == n and r['sys_hist'].sum() == r['n_systems'], what
    k = r['n_systems']
    assert r['sys_n_atoms'][:k].sum() == (role == 2).sum() and r['sys_n_bonds'][:k].sum() == (r['bond_role'] == 2).sum(), what
    assert not r['sys_n_atoms'][k:].any() and not r['sys_atom_ptr'][k:].any() and not r['sys_bond_ptr'][k:].any(), what
    assert r['sys_atom_ptr'][:k].tolist() == (np.cumsum(r['sys_n_atoms'][:k]) - r['sys_n_atoms'][:k]).tolist(), what
    rings_ = r['sys_n_bonds'][:k] - r['sys_n_atoms'][:k] + 1
    assert r['most_rings'] == (rings_.max() if k else 0) and r['largest_system'] == (r['sys_n_atoms'][:k].max() if k else 0), what
    assert r['sys_hist'].tolist() == np.bincount(np.minimum(rings_ - 1, len(r['sys_hist']) - 1), minlength=len(r['sys_hist'])).tolist(), what
    assert r['n_fw_bonds'] == (r['bond_role'] != 0).sum() and not r['fw_bond_type'][r['n_fw_bonds']:].any(), what


def test_the_named_cases_have_the_pieces_known_by_hand():
    for name, want in EXPECTED.items():
        r = ref(name)
        assert tuple(int(r[k]) for k in F.STAT_KEYS) == want, name
        if want[0]:
            assert (r['atom_system'] == -1).all() and not r['atom_role'].any() and not r['sys_hist'].any() and not r['fw_bond_index'].any()
    assert ref('cyclohexanone', 1)['atom_role'].tolist() == [2] * 6 + [3] and ref('cyclohexanone', 1)['bond_role'].tolist() == [2] * 6 + [3]
    assert ref('cyclohexanone', 1)['n_exo'] == 1 and ref('acetone', 1)['n_fw_atoms'] == 0 and ref('two_fragments', 1)['n_exo'] == 1
    assert ref('ignored_bonds', 1)['n_exo'] == 0                           # =C on a side chain: no core atom next to it
    assert ref('biphenyl')['bond_role'].tolist().count(1) == 1 and ref('diphenylmethane')['atom_role'][12] == 1
    assert ref('spiro_nonane')['sys_hist'].tolist() == [0, 1] + [0] * 6 and ref('cubane')['sys_hist'][4] == 1
    assert F.framework_ref(CASES['cubane'], 0, 3)['sys_hist'].tolist() == [0, 0, 1]     # the last bin takes every larger system
    with pytest.raises(ValueError, match='mode'):
        F.framework_ref(CASES['benzene'], 4)
    with pytest.raises(ValueError, match='sys_bins'):
        F.framework_ref(CASES['benzene'], 0, 17)
    with pytest.raises(ValueError, match='same pair'):
        F.framework_ref(mol(3, ring(3) + [(1, 0)]))


def test_against_networkx_on_the_cases_and_300_random_sparse_graphs():
    for name in SMALL:
        against_networkx(CASES[name], name)
    seen = np.zeros(4, dtype=np.int64)
    for s in range(300):
        m = sparse_graph(9000 + s)
        against_networkx(m, s)
        r = F.framework_ref(m, 1)
        seen += [r['n_systems'] > 1, r['n_linker'] > 0, r['n_exo'] > 0, r['n_fusion'] > 0]
    assert (seen >= 10).all(), seen                                         # the random graphs do exercise every kind of piece


def key_of(m, result, system=None):
    """the full certificate of a piece by canon_ref on the host sub-molecule"""
    res = {k: np.asarray([v]) if np.ndim(v) == 0 else v for k, v in result.items()}
    res.update(atom_ptr=np.zeros(1, dtype=np.int32), bond_ptr=np.zeros(1, dtype=np.int32))
    return C.certificate(C.stack_ref([F.piece_mol(res, 0, system, ELEMENTS)]), 0)


def test_renumbering_atoms_and_bonds_changes_nothing_but_the_numbering():
    for name in SMALL:
        if name == 'ignored_bonds':                                        # its bad indices cannot be renumbered
            continue
        m, r = CASES[name], ref(name, 1)
        key = key_of(m, r)
        for s in range(20):
            p, new, _ = permuted(m, 700 + s)
            q = F.framework_ref(p, 1)
            assert all(q[k] == r[k] for k in F.STAT_KEYS) and q['sys_hist'].tolist() == r['sys_hist'].tolist(), (name, s)
            assert q['atom_role'][new].tolist() == r['atom_role'].tolist(), (name, s)
            assert (q['atom_system'][new] >= 0).tolist() == (r['atom_system'] >= 0).tolist(), (name, s)
            assert sorted(q['bond_role'].tolist()) == sorted(r['bond_role'].tolist()), (name, s)
            assert key_of(p, q) == key, (name, s)


def test_the_maps_reproduce_the_types_and_the_bonds_of_the_molecule():
    cls = {z: i for i, z in enumerate(ELEMENTS)}
    mols = [CASES[k] for k in MEASURED] + [sparse_graph(9500 + s) for s in range(40)]
    for what, m in enumerate(mols):
        G = graph_of(m)
        for mode in (0, 1, 3):
            r = F.framework_ref(m, mode)
            pieces = [(r['fw_atom_map'], r['fw_atom_type'], r['fw_bond_index'], r['fw_bond_type'], 0, 0, r['n_fw_atoms'], r['n_fw_bonds'],
                       r.get('fw_pos'))]
            for k in range(r['n_systems']):
                pieces.append((r['sys_atom_map'], r['sys_atom_type'], r['sys_bond_index'], r['sys_bond_type'], r['sys_atom_ptr'][k],
                               r['sys_bond_ptr'][k], r['sys_n_atoms'][k], r['sys_n_bonds'][k], r.get('sys_pos')))
            for amap, atype, bidx, btype, a0, b0, na, nb, pos in pieces:
                atoms = amap[a0:a0 + na]
                assert (np.diff(atoms) > 0).all(), what                     # the original relative order
                want = [0 if mode & 2 else cls[int(m['element'][a])] for a in atoms]
                assert atype[a0:a0 + na].tolist() == want, what
                if pos is not None:
                    assert np.array_equal(pos[a0:a0 + na], m['atom_pos'][atoms]), what
                last = -1
                for e in range(b0, b0 + nb):
                    i, j = int(atoms[bidx[0, e]]), int(atoms[bidx[1, e]])
                    d = G[i][j]
                    assert d['e'] > last and (int(m['bond_index'][0, d['e']]), int(m['bond_index'][1, d['e']])) == (i, j), what
                    assert btype[e] == (1 if mode & 2 else d['t']), what
                    last = d['e']
                assert nb == G.subgraph(atoms.tolist()).number_of_edges(), what   # every bond between atoms of a piece belongs to it


def test_key_relations_of_the_named_cases():
    fw = lambda name, mode=0: key_of(CASES[name], ref(name, mode))
    assert fw('toluene') == fw('ethylbenzene') == fw('benzene')
    assert fw('pyridine') != fw('benzene') and fw('pyridine', 2) == fw('benzene', 2)
    assert fw('diphenylmethane') == fw('methyl_diphenylmethane') != fw('biphenyl')
    assert fw('cyclohexanone', 1) != fw('cyclohexanone', 0)
    r = ref('biphenyl')
    assert key_of(CASES['biphenyl'], r, 0) == key_of(CASES['biphenyl'], r, 1) == fw('benzene')


def hand_made():
    a = F.stats_mols([CASES[k] for k in ('propane', 'benzene', 'toluene', 'ethylbenzene', 'biphenyl', 'pyridine', 'chain_257', 'naphthalene')])
    b = F.stats_mols([CASES[k] for k in ('benzene', 'diphenylmethane', 'acetone', 'spiro_nonane')])
    return a, b


def test_summary_novelty_and_compare_on_hand_made_results():
    a, b = hand_made()
    s = F.summary(a, top_k=2)
    assert (s['n_molecules'], s['n_measured'], s['n_too_large'], s['n_empty'], s['n_keyed'], s['n_distinct']) == (8, 7, 1, 1, 6, 4)
    assert s['empty_fraction'] == 1 / 7 and s['uniqueness'] == 4 / 6 and s['n_abandoned'] == 0
    assert (s['n_systems'], s['n_distinct_systems']) == (7, 3) and s['system_rings']['counts'] == [6, 1] + [0] * 6
    assert s['stats']['n_systems']['hist'][:3] == [1, 5, 1] and s['stats']['n_fw_atoms']['mean'] == (6 * 4 + 12 + 10) / 7
    top = s['top_frameworks']
    assert [t['count'] for t in top] == [3, 1] and top[0]['smiles'] == 'C1=CC=CC=C1' and top[0]['fraction'] == 0.5
    assert s['top_systems'][0]['count'] == 5 and s['top_systems'][0]['n_atoms'] == 6
    assert F.summary({k: v for k, v in a.items() if k not in F.KEY_ARRAYS}, {k: a[k] for k in F.KEY_ARRAYS}, top_k=2) == s
    # an abandoned search leaves the key empty and is counted
    tight = F.stats_mols([CASES['benzene'], CASES['cubane']], max_nodes=30)
    st = F.summary(tight)
    assert tight['fw_key_status'].tolist() == [0, 2] and tight['fw_hash'][1] == 0 and tight['fw_cert_ptr'][2] == tight['fw_cert_ptr'][1]
    assert (st['n_keyed'], st['n_abandoned'], st['n_systems_abandoned'], st['n_distinct']) == (1, 1, 1, 1)
    assert F.novelty(a, b) == 3 / 6 and F.novelty(b, a) == 2 / 3 and F.novelty(a, b, 'system') == 2 / 7 and np.isnan(F.novelty(F.empty(with_keys=True), a))
    c = F.compare(a, b)
    assert c['framework_novelty'] == [3 / 6, 2 / 3] and c['uniqueness'] == [4 / 6, 1.0] and 0 < c['system_rings'] < 1
    assert F.compare(a, a)['n_fw_atoms'] == 0 and F.compare(a, a)['framework_novelty'] == [0.0, 0.0]
    both = F.concat([a, b])
    whole = F.stats_mols([CASES[k] for k in ('propane', 'benzene', 'toluene', 'ethylbenzene', 'biphenyl', 'pyridine', 'chain_257', 'naphthalene',
                                             'benzene', 'diphenylmethane', 'acetone', 'spiro_nonane')])
    assert set(both) == set(whole) and all(np.array_equal(both[k], whole[k]) and both[k].dtype == whole[k].dtype for k in whole)


def test_command_line_and_files(tmp_path):
    import torch
    a, b = hand_made()
    torch.save({'finished': [CASES[k] for k in ('propane', 'benzene', 'toluene', 'ethylbenzene', 'biphenyl', 'pyridine', 'chain_257', 'naphthalene')]},
               tmp_path / 'samples_all.pt')
    assert F.main(['stats', str(tmp_path / 'samples_all.pt'), '--out', str(tmp_path / 'a.npz'), '--ref']) == 0
    from moldiff_amd.molpack import load_npz, save_npz
    saved = load_npz(tmp_path / 'a.npz')
    assert set(saved) == set(a) and all(np.array_equal(saved[k], a[k]) for k in a)
    save_npz(b, tmp_path / 'b.npz')
    assert F.main(['compare', str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')]) == 0


def test_the_entry_point_is_declared_and_registered():
    from moldiff_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'moldiff_hip.h')) as f:
        hdr = f.read()
    proto = re.search(r'\bint mdx_mol_framework\(([^;]*)\);', hdr).group(1)
    params = [p.strip() for p in proto.split(',')]
    assert len(params) == 36 and params[-1] == 'void* stream' and '#define MDX_FW_STATS 10' in hdr and len(F.STAT_KEYS) == 10
    assert 'MurckoScaffold' in hdr and 'mdx_mol_framework' in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        assert hasattr(L, 'mdx_mol_framework') and len(L.mdx_mol_framework.argtypes) == 36


def test_host_validation_under_the_host_sanitizers(tmp_path):
    """tools/framework_host_check.cpp over csrc/mdx_framework_args.h, a stand-alone program built with AddressSanitizer and UBSan"""
    run_host_check('framework_host_check', tmp_path)
