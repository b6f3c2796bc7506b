"""Centred against un-centred weight packs of the MolDiff denoiser's edge kernels, on ONE handle (csrc/mdx_pack.cpp Layer::centred,
csrc/mdx_row.h row_layernorm_centred; the bound on what centring leaves is stated and asserted in
tests/test_ln_centred_pack.py).

Centring a Linear that feeds a LayerNorm is exact in real arithmetic and moves the fp32 rounding in the last bits, like any legal
summation order.  So both conventions are held to the SAME bound against a float64 evaluation of the oracle, the one the un-centred
path has always been held to (tests/test_gpu_fullsize.py):  |HIP - fp64| <= max(contract, f |oracle_fp32 - fp64|)  with f =
tests/util.py's factor for forward quantities; contracts 2e-5 for pre-softmax network outputs and block outputs, 1e-4 for positions --
as they stand for mdx_moldiff_forward on the recipe weights, and relative to max(1, max|fp64 value|) where the quantity is not O(1):
the stress weights (as tests/test_gpu_fullsize.py's rel_scale) and the raw block outputs on random activations.  With it go that
file's two population checks: the rms error within 2x the fp32 oracle's own (or 0.02 of the contract), and the rows outside the plain
contract no more than 1.1x the fp32 oracle's + 1.  The ratio of the two conventions' errors is printed, not asserted.
The two population checks are asserted on the recipe-weight cases (64 atoms, 1,800 half-edge rows) and only PRINTED on the stress
fixtures: at 12 atoms (66 half-edge rows) the rms of ONE fp32 oracle evaluation is no yardstick -- measured on the exact path,
pred_halfedge: rms |HIP - fp64| 4.212e-6 for the centred AND for the un-centred packs (the arithmetic every earlier test accepted)
against 2 x 1.800e-6 = 3.656e-6; pred_node 5.52e-6 / 3.98e-6 against 5.885e-6; every other stress figure is inside.  tests/util.py
explains why a single evaluation under-samples such statistics; the suite itself applies them at 256 molecules only.

The batch: molecules of 2, 3, 9, 17 and 33 atoms -- one- to three-run tiles of 16 edges, a partial last tile, and a molecule whose
rows span more than one tile -- uncapped and with the launchers capped to 1 and 2 compute units (`_lib.cu_cap`), so that the work
queue, the static plan and the section-cut tail of the persistent kernels are all walked.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moldiff_amd import _lib
from oracle import moldiff_oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [2, 3, 9, 17, 33]
CAPS = (0, 1, 2)
_cache = {}


def _positions(r, sizes):
    """atoms of a molecule on a jittered lattice, no pair closer than 1: the 1 / d / (d + 1) force of a near pair would set the error of
    pred_pos, not the LayerNorms this file is about"""
    pos = []
    for n in sizes:
        side = int(np.ceil(max(n, 1) ** (1 / 3))) + 1
        cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing='ij'), -1).reshape(-1, 3)
        pick = cells[r.permutation(len(cells))[:n]]
        pos.append(pick * 1.7 + r.uniform(-0.35, 0.35, (n, 3)))
    return U.t32(np.concatenate(pos))


def _f64(P):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}


def _inputs(sizes, seed):
    key = (tuple(sizes), seed)
    if key not in _cache:
        bn, hei, bh, ei, be = U.graph_from_sizes(sizes)
        N, Eh, E = len(bn), len(bh), ei.shape[1]
        r = U.rng(seed)
        d = dict(bn=bn, hei=hei, bh=bh, ei=ei, be=be, N=N, Eh=Eh, E=E)
        d['xn'] = F.one_hot(torch.from_numpy(r.integers(0, 8, N)), 8).float()
        xh = F.one_hot(torch.from_numpy(r.integers(0, 6, Eh)), 6).float()
        d['he'] = torch.cat([xh, xh])
        d['pos'] = _positions(r, sizes)
        d['t'] = torch.from_numpy(r.integers(0, 1000, len(sizes)))
        # block-level inputs: activations of the size the blocks see (O(1) features), times in [0, 1]
        d['x'] = U.t32(r.standard_normal((N, 256)))
        d['ea'] = U.t32(r.standard_normal((E, 64)))
        d['tn'] = U.t32(r.random((N, 1)))
        d['te'] = U.t32(r.random((E, 1)))
        d['rel'] = d['pos'][ei[0]] - d['pos'][ei[1]]
        d['dist'] = d['rel'].norm(dim=-1)
        d['dev'] = {k: v.to(DEV) for k, v in d.items() if torch.is_tensor(v)}
        _cache[key] = d
    return _cache[key]


def _bound(name, hip, r32, r64, tol, rel_scale, population=True):
    """(error, bound) of tests/test_gpu_fullsize.py's _check_against_oracle, with its rms and rows-outside-the-contract checks"""
    if rel_scale:
        tol = tol * max(1.0, float(r64.abs().max()))
    e_hip, e_ref = U.maxdiff(hip, r64), U.maxdiff(r32, r64)
    rms_hip, rms_ref = U.rmsdiff(hip, r64), U.rmsdiff(r32, r64)
    print(f'[ln_centred rms] {name}: rms |HIP-fp64| {rms_hip:.3e}  rms |oracle32-fp64| {rms_ref:.3e}  bound {max(0.02 * tol, 2.0 * rms_ref):.3e}')
    bad = [] if rms_hip <= max(0.02 * tol, 2.0 * rms_ref) or not population else [f'{name}: rms {rms_hip:.3e} > {max(0.02 * tol, 2.0 * rms_ref):.3e}']

    def rows_out(x):
        d = (torch.as_tensor(x).detach().cpu().double() - r64.double()).abs()
        return int((d.reshape(d.shape[0], -1).max(dim=1).values > tol).sum())
    n_hip, n_ref = rows_out(hip), rows_out(r32)
    if n_hip > 1.1 * n_ref + 1 and population:
        bad.append(f'{name}: {n_hip} rows outside the {tol} contract, the fp32 oracle has {n_ref}')
    bound = max(tol, U.tail('factor') * e_ref)
    if e_hip > bound:
        bad.append(f'{name}: |HIP-fp64| {e_hip:.3e} > {bound:.3e}')
    return e_hip, bound, e_ref, bad


def _both(model, run):
    """run() with centred packs (the handle's default) and with the weights as stored, on the same handle"""
    eng = model._engine()
    cen = run()
    torch.cuda.synchronize()
    with _lib.ln_centred(eng, False):
        unc = run()
        torch.cuda.synchronize()
    again = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(cen, again)), 'the handle does not come back to the centred packs bit for bit'
    return cen, unc


def _compare(tag, names, cen, unc, r32, r64, tols, rel_scale, population=True):
    bad = []   # every figure is printed before anything is asserted
    for n, c, u, a, b, tol in zip(names, cen, unc, r32, r64, tols):
        e_c, bound, e_ref, bad_c = _bound(f'{tag} {n} centred', c, a, b, tol, rel_scale, population)
        e_u, _, _, bad_u = _bound(f'{tag} {n} un-centred', u, a, b, tol, rel_scale, population)
        bad += bad_c + bad_u
        print(f'[ln_centred] {tag} {n}: |centred-fp64| {e_c:.3e}  |uncentred-fp64| {e_u:.3e}  ratio {e_c / max(e_u, 1e-300):.2f}  '
              f'|oracle32-fp64| {e_ref:.3e}  bound {bound:.3e}  |centred-uncentred| {U.maxdiff(c, u):.3e}')
    assert not bad, bad


def _forward_refs(d, P, cfg=U.CFG):
    out = []
    for Q in (P, _f64(P)):
        dt = torch.float64 if Q is not P else torch.float32
        with torch.no_grad():
            o = O.moldiff_forward(Q, cfg, d['xn'].to(dt), d['pos'].to(dt), d['bn'], d['he'].to(dt), d['ei'], d['be'], d['t'])
        out.append([o[k] for k in ('pred_node', 'pred_halfedge', 'pred_pos')])
    return out


@U.both_paths
@pytest.mark.parametrize('cap', CAPS)
def test_moldiff_forward_centred_and_uncentred_match_fp64(cap):
    d = _inputs(SIZES, 11)
    v = d['dev']
    m = U.moldiff('MolDiff', DEV)
    if 'fwd' not in d:
        d['fwd'] = _forward_refs(d, U.params(U.moldiff('MolDiff')))
    r32, r64 = d['fwd']

    def run():
        out = m(v['xn'], v['pos'], v['bn'], v['he'], v['ei'], v['be'], v['t'])
        return [out[k].clone() for k in ('pred_node', 'pred_halfedge', 'pred_pos')]

    with _lib.cu_cap(cap):
        cen, unc = _both(m, run)
    assert any(not torch.equal(a, b) for a, b in zip(cen, unc)), 'the test aid changed nothing'
    _compare(f'moldiff_forward cap {cap} {U.current_matrix_path()}', ('pred_node', 'pred_halfedge', 'pred_pos'), cen, unc, r32, r64,
             (2e-5, 2e-5, 1e-4), rel_scale=False)


def _raw_blocks(m, d, i):
    """mdx_node_block, mdx_edge_block and mdx_pos_update of block i on the MolDiff handle itself (the raw entry points)"""
    v, L, eng = d['dev'], _lib.lib(), m._engine()
    g = _lib.Graph(d['ei'], d['bn'], len(SIZES))
    ws, nb = g.workspace(torch.device(DEV))
    dn = torch.empty(d['N'], 256, device=DEV)
    de = torch.empty(d['E'], 64, device=DEV)
    dp = torch.empty(d['N'], 3, device=DEV)
    tn, te, dist = v['tn'].view(-1).contiguous(), v['te'].view(-1).contiguous(), v['dist'].contiguous()
    rel = v['rel'].contiguous()
    s = _lib.stream()
    _lib.check(L.mdx_node_block(eng.h, g.h, i, _lib.ptr(v['x']), _lib.ptr(v['ea']), _lib.ptr(tn), _lib.ptr(dn), ws, nb, s))
    _lib.check(L.mdx_edge_block(eng.h, g.h, i, _lib.ptr(v['ea']), _lib.ptr(v['x']), _lib.ptr(te), _lib.ptr(de), ws, nb, s))
    _lib.check(L.mdx_pos_update(eng.h, g.h, i, _lib.ptr(v['x']), _lib.ptr(v['ea']), _lib.ptr(rel), _lib.ptr(dist), _lib.ptr(te),
                                _lib.ptr(dp), ws, nb, s))
    torch.cuda.synchronize()   # `g` and its workspace die with this frame
    return [dn, de, dp]


def _block_refs(d, P, i):
    out = []
    for Q, dt in ((P, torch.float32), (_f64(P), torch.float64)):
        c = lambda k: d[k].to(dt)
        with torch.no_grad():
            out.append([O.node_block(Q, f'denoiser.node_blocks_with_edge.{i}', c('x'), d['ei'], c('ea'), c('tn')),
                        O.edge_block(Q, f'denoiser.edge_blocks.{i}', c('ea'), d['ei'], c('x'), c('te')),
                        O.pos_update(Q, f'denoiser.pos_blocks.{i}', c('x'), c('ea'), d['ei'], c('rel'), c('dist'), c('te'))])
    return out


@U.both_paths
@pytest.mark.parametrize('cap', CAPS)
def test_raw_block_entry_points_centred_and_uncentred_match_fp64(cap):
    d = _inputs(SIZES, 11)
    m = U.moldiff('MolDiff', DEV)
    i = 2
    if 'blk' not in d:
        d['blk'] = _block_refs(d, U.params(U.moldiff('MolDiff')), i)
    r32, r64 = d['blk']
    with _lib.cu_cap(cap):
        cen, unc = _both(m, lambda: _raw_blocks(m, d, i))
    # each of the three reaches centred LayerNorms: kernel A's NodeBlock path, both BondFFNs (edge_block), kernel B's PosUpdate
    assert all(not torch.equal(c, u) for c, u in zip(cen, unc)), 'the test aid changed nothing'
    _compare(f'raw blocks cap {cap} {U.current_matrix_path()}', ('node_block', 'edge_block', 'pos_update'), cen, unc, r32, r64,
             (2e-5, 2e-5, 1e-4), rel_scale=True)


@U.both_paths
@pytest.mark.parametrize('natoms', [12, 101])
def test_stress_weights_centred_and_uncentred(natoms):
    """Heavy-tailed stress weights (LayerNorm gains up to 30): the forward against fp64 for both conventions, and the class ids of one
    sampling step identical between them."""
    d = _inputs([natoms], 300 + natoms)
    v = d['dev']
    m = U.moldiff_stress(DEV, 'MolDiff_simple')
    if 'fwd' not in d:
        d['fwd'] = _forward_refs(d, U.params(U.moldiff_stress('cpu', 'MolDiff_simple')))
    r32, r64 = d['fwd']

    def run():
        out = m(v['xn'], v['pos'], v['bn'], v['he'], v['ei'], v['be'], v['t'])
        res = [out[k].clone() for k in ('pred_node', 'pred_halfedge', 'pred_pos')]
        sm = m.sampler(1, v['bn'], v['hei'], v['bh'], seed=7)
        sm.init()
        sm.step(0)
        st = sm.state()
        return res + [st['h_node'].argmax(-1).clone(), st['h_halfedge'].argmax(-1).clone()]

    cen, unc = _both(m, run)
    _compare(f'stress {natoms} atoms {U.current_matrix_path()}', ('pred_node', 'pred_halfedge', 'pred_pos'), cen[:3], unc[:3], r32, r64,
             (2e-5, 2e-5, 1e-4), rel_scale=True, population=False)
    assert torch.equal(cen[3], unc[3]), 'atom classes of one sampling step differ between the conventions'
    assert torch.equal(cen[4], unc[4]), 'bond classes of one sampling step differ between the conventions'
