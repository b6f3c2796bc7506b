"""GPU: every work-plan regime of the persistent row-owner kernels at small sizes, against the oracle at the tight tolerances.

Edge kernels A and B, the guidance backward and linear_rows size their grid as min(ceil(units / 4), #CUs x waves per SIMD); on the
whole device a wave gets a second unit only beyond ~32,768 directed edges, so the oracle tests at small shapes run the persistent loop
body once.  Here the compute-unit count the launchers see is capped (`_lib.cu_cap`, a test aid) so that batches of 60 .. 1,800 directed
edges loop: the one-unit-ahead prologue, the re-primed weight ring, the reused parking area and the repeated look-ahead of the last item
are compared with the oracle, in every regime of the static plan (csrc/mdx_plan.h make_plan) and of the per-pair work queue.

Which regime a (sizes, cap) pair is in comes from the library's own plan (`_lib.launch_units`, `_lib.work_plan`: the host exports of
the real make_plan and launch arithmetic), and `test_the_cases_cover_every_regime` asserts the set below is complete.  Caps 1, 2, 3 give
8 / 16 / 24 slots to the exact build and 4 / 8 / 12 to the split build; split 2 with m = 4 needs ceil(rem / (slots - rem)) = 4, which
no remainder of 4, 8 or 12 slots gives (rem = 3 -> 3, 6 -> 3, 7 -> none, 9 -> 3, 10 -> 5), so one batch also runs under cap 5 (20
slots, rem = 16).

The static plan is selected the way tests/test_gpu_round3.py does: a graph owns four work-queue counter sets, one per launching stream,
and the launches of a fifth stream use the static plan.  (The split forward kernels always take it.)  For the queue a pair's range is
compared with its section-cut tail, (waves of the pair) x 10 / 8 units: shorter (every unit of the pair is cut), longer with one
workgroup in the pair, longer with two (grid > #CUs).

Tolerances are the existing contracts: pred_node / pred_halfedge < 2e-5, pred_pos < 1e-4 (tests/test_gpu_edgecases.py), bond logits
< 2e-5 and the gradient within 1e-3 of its own maximum (tests/test_gpu_bondpred.py), the Linear bounds of
tests/test_gpu_train_ops.py::test_linear_on_many_rows_takes_the_row_owner_kernel.  Which wave computes a unit enters no result, so
every capped run is also byte-equal to the uncapped run of the same inputs.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from moldiff_amd import _lib
from oracle import moldiff_oracle as O
from tests import util as U

DEV = 'cuda:0'
gpu = pytest.mark.gpu

# ragged size lists, 62 .. 1,788 directed edges (the first three are the suite's usual ones)
SIZES = {
    'two': [5, 7],
    'degenerate': [1, 7, 2, 1, 0, 5],
    'three': [24, 31, 18],
    'six': [33, 2, 12, 2, 0, 24],
    'ragged': [2, 9, 17, 3, 5, 7],
    'five': [21, 12, 2, 2, 9],
    'four': [21, 12, 2, 5],
    'small': [2, 5, 12],
}
CAPS = (1, 2, 3)
CASES = [(name, cap) for name in SIZES for cap in CAPS] + [('six', 5)]
STATIC = ('even', 'nosplit', 'split1_m1', 'split1_m2', 'split2_m3', 'split2_m4', 'split2_m5')
QUEUE = ('short', 'long1', 'long2')
WANTED = {(build, r) for build in ('exact', 'split') for r in STATIC} | {('queue', r) for r in QUEUE}


def regimes(sizes, cap):
    """{(build, regime of the static plan)} and {('queue', regime)} that edge kernel A's launches of this batch are in under the cap"""
    bn, hei, bh, ei, be = U.graph_from_sizes(sizes)
    lu = _lib.launch_units(ei, bn, len(sizes), cap)
    out = set()
    for build in ('exact', 'split'):
        a = lu['edge_a_' + build]
        p = _lib.work_plan(a['nunits'], 4 * a['grid'], True)
        if p['nf'] >= 2 and p['rem'] == 0:
            out.add((build, 'even'))                                   # every wave loops, no partial round
        elif p['nf'] >= 1 and p['split'] == 0 and 6 * p['rem'] > 5 * p['nslots']:
            out.add((build, 'nosplit'))                                # rem > 5/6 of the slots: the last round is cut by rows
        elif p['nf'] >= 1 and p['split']:
            out.add((build, f"split{p['split']}_m{p['m']}"))
    out |= {('queue', r) for r in QUEUE if lu['edge_a_exact'][r]}
    return out


def test_the_cases_cover_every_regime():
    """No GPU needed: the plan exports are host code."""
    got = set()
    for name, cap in CASES:
        got |= regimes(SIZES[name], cap)
    assert got >= WANTED, sorted(WANTED - got)
    # caps 1, 2, 3 alone reach everything but the split build's split 2 with m = 4 (module docstring)
    small = set()
    for name, cap in CASES:
        if cap <= 3:
            small |= regimes(SIZES[name], cap)
    assert WANTED - small == {('split', 'split2_m4')}, sorted(WANTED - small)
    # and every batch loops under every cap of its largest units: the exact kernel B and the backward run more units than waves
    for name in ('three', 'six', 'ragged', 'five', 'four'):
        bn, hei, bh, ei, be = U.graph_from_sizes(SIZES[name])
        for cap in CAPS:
            lu = _lib.launch_units(ei, bn, len(SIZES[name]), cap)
            assert all(lu[k]['nunits'] > 4 * lu[k]['grid'] for k in _lib.LAUNCHES), (name, cap, lu)


# ---- inputs and references, computed once per size list ---------------------------------------------------------------------------

def _positions(r, sizes):
    """atoms of a molecule on a jittered lattice: no pair closer than 1 (the 1 / d / (d + 1) force of a near pair would set the error of
    pred_pos, tests/test_gpu_edgecases.py keeps atoms apart for the same reason)"""
    pos = []
    for n in sizes:
        side = int(np.ceil(max(n, 1) ** (1 / 3))) + 1
        cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing='ij'), -1).reshape(-1, 3)
        pick = cells[r.permutation(len(cells))[:n]]
        pos.append(pick * 1.7 + r.uniform(-0.35, 0.35, (n, 3)))
    return U.t32(np.concatenate(pos) if pos else np.zeros((0, 3)))


_cache = {}
_streams = []


def _inputs(name):
    if name not in _cache:
        sizes = SIZES[name]
        bn, hei, bh, ei, be = U.graph_from_sizes(sizes)
        N, Eh = len(bn), len(bh)
        r = U.rng(1000 + len(_cache))
        d = dict(bn=bn, ei=ei, be=be, N=N, Eh=Eh)
        d['xn'] = F.one_hot(torch.from_numpy(r.integers(0, 8, N)), 8).float()
        d['xh'] = F.one_hot(torch.from_numpy(r.integers(0, 6, Eh)), 6).float()
        d['he'] = torch.cat([d['xh'], d['xh']])
        d['pos'] = _positions(r, sizes)
        dist = (d['pos'][ei[0]] - d['pos'][ei[1]]).norm(dim=-1)
        assert float(dist.min()) > 1.0
        d['t'] = torch.from_numpy(r.integers(0, 1000, len(sizes)))
        d['cot'] = U.t32(r.standard_normal((Eh, 5), dtype=np.float32))
        d['dev'] = {k: d[k].to(DEV) for k in ('bn', 'ei', 'be', 'xn', 'he', 'pos', 't', 'cot')}   # the same tensors every time: one cached graph
        _cache[name] = d
    return _cache[name]


def _moldiff_ref(name):
    d = _inputs(name)
    if 'moldiff' not in d:
        with torch.no_grad():
            d['moldiff'] = O.moldiff_forward(U.params(U.moldiff('MolDiff', DEV)), U.CFG, d['xn'], d['pos'], d['bn'], d['he'], d['ei'], d['be'], d['t'])
    return d['moldiff']


def _bondpred_ref(name):
    d = _inputs(name)
    if 'bondpred' not in d:
        p = d['pos'].clone().requires_grad_(True)
        logits = O.bondpred_forward(U.params(U.bondpred(DEV)), U.CFGB, d['xn'], p, d['bn'], d['ei'], d['be'], d['t'])
        grad, = torch.autograd.grad((logits * d['cot']).sum(), p)
        d['bondpred'] = (logits.detach(), grad)
    return d['bondpred']


def _runs(run, cap):
    """run() uncapped on the current stream, then under the cap on the current stream (work queues) and on four further streams -- the
    graph's counter sets go to the first four streams that launch on it, so the last one takes the static plan -- then uncapped again on
    the first stream: the counters a capped launch left behind are all zero."""
    if not _streams:
        _streams.extend(torch.cuda.Stream() for _ in range(4))
    base = run()
    torch.cuda.synchronize()
    capped = []
    with _lib.cu_cap(cap):
        capped.append(run())
        torch.cuda.synchronize()
        for s in _streams:
            with torch.cuda.stream(s):
                capped.append(run())
            s.synchronize()
    after = run()
    torch.cuda.synchronize()
    return base, capped, after


def _same_bytes(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@gpu
@U.both_paths
@pytest.mark.parametrize('name,cap', CASES)
def test_moldiff_forward_under_a_cu_cap_matches_oracle(name, cap):
    d, ref = _inputs(name), _moldiff_ref(name)
    v = d['dev']
    m = U.moldiff('MolDiff', DEV)
    keys = ('pred_node', 'pred_halfedge', 'pred_pos')

    def run():
        out = m(v['xn'], v['pos'], v['bn'], v['he'], v['ei'], v['be'], v['t'])
        return [out[k].clone() for k in keys]

    base, capped, after = _runs(run, cap)
    for i, got in enumerate(capped):
        err = [U.maxdiff(g, ref[k]) for g, k in zip(got, keys)]
        print(f'{name} cap {cap} run {i}: max |HIP - oracle| node {err[0]:.2e} halfedge {err[1]:.2e} pos {err[2]:.2e}')
        assert err[0] < 2e-5 and err[1] < 2e-5 and err[2] < 1e-4, (i, err)
        assert _same_bytes(got, base), f'capped run {i} differs from the uncapped run'
    assert _same_bytes(after, base)


@gpu
@U.both_paths
@pytest.mark.parametrize('name,cap', CASES)
def test_bond_predictor_and_its_gradient_under_a_cu_cap_match_oracle(name, cap):
    d = _inputs(name)
    ref_logits, ref_grad = _bondpred_ref(name)
    v = d['dev']
    m = U.bondpred(DEV)

    def run():
        pos = v['pos'].detach().clone().requires_grad_(True)
        logits = m(v['xn'], pos, v['bn'], v['ei'], v['be'], v['t'])
        grad, = torch.autograd.grad((logits * v['cot']).sum(), pos)
        return [logits.detach().clone(), grad.clone()]

    base, capped, after = _runs(run, cap)
    scale = float(ref_grad.abs().max())
    for i, (logits, grad) in enumerate(capped):
        el, eg = U.maxdiff(logits, ref_logits), U.maxdiff(grad, ref_grad)
        print(f'{name} cap {cap} run {i}: max |HIP - oracle| logits {el:.2e}, gradient {eg:.2e} of {scale:.2e}')
        assert el < 2e-5, (i, el)
        assert eg <= 1e-3 * scale, (i, eg, scale)
        assert _same_bytes((logits, grad), base), f'capped run {i} differs from the uncapped run'
    assert _same_bytes(after, base)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


@gpu
@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('K,N,with_addend', [(256, 256, False), (80, 64, True), (64, 20, False)])
def test_linear_on_many_rows_under_a_cu_cap(K, N, with_addend, cap):
    """linear_rows' waves take ceil(units / slots) consecutive 16-row units each: 1,032 units on 8, 16 and 24 slots (129, 65 and 43 per
    wave, the last wave short).  Forward and all gradients against float64, and the bytes of the uncapped run."""
    from moldiff_amd import train_ops as T
    M = T.ROWS_MIN + 123
    g = U.rng(K * 1000 + N + cap)
    leaf = lambda *shape, scale=1.0: (U.t32(g.standard_normal(shape)) * scale).to(DEV).requires_grad_(True)
    wide, w, b = leaf(M, K + 16), leaf(N, K, scale=K ** -0.5), leaf(N)
    add = leaf(M, N) if with_addend else None
    gy = U.t32(g.standard_normal((M, N))).to(DEV)

    def run():
        for t in (wide, w, b, add):
            if t is not None:
                t.grad = None
        x = wide[:, 8:8 + K]
        assert T.linear_rows_ok(T._rows(x), N, K, add)
        y = T.linear(x, w, b, add)
        y.backward(gy)
        return [y.detach().clone(), wide.grad.clone(), w.grad.clone(), b.grad.clone()] + ([add.grad.clone()] if with_addend else [])

    base = run()
    with _lib.cu_cap(cap):
        got = run()
    after = run()
    torch.cuda.synchronize()
    w2, b2, wide2 = (t.detach().clone().requires_grad_(True) for t in (w, b, wide))
    y2 = F.linear(wide2[:, 8:8 + K].double(), w2.double(), b2.double())
    if with_addend:
        a2 = add.detach().clone().requires_grad_(True)
        y2 = y2 + a2.double()
    y2.backward(gy.double())
    assert _rel(got[0], y2) < 2e-6
    assert _rel(got[1], wide2.grad) < 2e-6 and _rel(got[2], w2.grad) < 5e-6 and _rel(got[3], b2.grad) < 5e-6
    if with_addend:
        assert _rel(got[4], a2.grad) < 1e-6
    # the row-owner kernel's outputs (forward and grad_input): every unit owns its rows
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    assert torch.equal(after[0], base[0]) and torch.equal(after[1], base[1])


@gpu
def test_the_cap_is_restored_and_only_lowers_the_count():
    L = _lib.lib()
    with _lib.cu_cap(2):
        with _lib.cu_cap(1):
            assert _lib._cu_cap == 1
        assert _lib._cu_cap == 2
    assert _lib._cu_cap == 0
    bn, hei, bh, ei, be = U.graph_from_sizes(SIZES['three'])
    own = torch.cuda.get_device_properties(0).multi_processor_count
    assert _lib.launch_units(ei, bn, 3) == _lib.launch_units(ei, bn, 3, own)
    with _lib.cu_cap(2):
        assert _lib.launch_units(ei, bn, 3) == _lib.launch_units(ei, bn, 3, 2) != _lib.launch_units(ei, bn, 3, own)
    with _lib.cu_cap(own + 7):
        assert _lib.launch_units(ei, bn, 3) == _lib.launch_units(ei, bn, 3, own)
    # a cap beyond the device's count is the device's count: the same bytes as without one
    d = _inputs('two')
    v = d['dev']
    m = U.moldiff('MolDiff', DEV)
    a = m(v['xn'], v['pos'], v['bn'], v['he'], v['ei'], v['be'], v['t'])['pred_pos'].clone()
    with _lib.cu_cap(1 << 20):
        b = m(v['xn'], v['pos'], v['bn'], v['he'], v['ei'], v['be'], v['t'])['pred_pos'].clone()
    assert torch.equal(a, b) and L.mdx_debug_set_num_cus(0) == 0
