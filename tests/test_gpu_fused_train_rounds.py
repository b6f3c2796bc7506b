"""GPU: every round regime of the eight fused float16 training kernels (csrc/mdx_train_fused.hip: bondffn, edge_tail, posffn, nodemsg,
forward and backward) at under 2,000 rows, against the uncapped run, the per-operator composition and float64.

The kernels are persistent row owners: a wave owns 16-row tiles and walks them with a stride of nw = grid x waves.  On the whole device
(256 CUs x 8 waves) a wave takes a second tile only beyond 32,768 rows, so tests/test_gpu_fused_train.py runs every loop body once.
Here the compute-unit count the launchers see is capped (`_lib.cu_cap`, a test aid) and batches of 62 .. 1,788 directed edges loop:
the second trip of each loop, bondffn_fwd's look-ahead load of tile + nw, the `iters` loop of nodemsg (waves past the last tile keep
taking part in the workgroup's weight copies, compute on the clamped last row and store nothing), the reuse of the wave-private LDS
transposition areas, the per-workgroup LayerNorm-parameter partial rows of a workgroup that adds several tiles, and a ragged last tile
in a later round.

Regimes, per kernel, from the launchers' own arithmetic (`_lib.fused_grid`, the host export of csrc/mdx_train_plan.h fused_grid):
  a  one round (what the uncapped device gives at these sizes)
  b  two or more rounds, all full
  c  a short last round that ends inside a workgroup: some of its waves work, the others are past the end
  d  a short last round that leaves a whole workgroup idle
each with a ragged last tile (E % 16 != 0; in b, c, d it lies in a round >= 2) and with E % 16 == 0.  `test_the_cases_cover_every_regime`
(no GPU) asserts that CASES reaches every (kernel, regime, tile case).  The size lists are the suite's ragged ones
(tests/test_gpu_work_plan.py) plus [22, 7, 3, 2]: 512 edges = 32 full tiles, the one regime (b with E % 16 == 0) none of the others has.

Every tile owns its rows and the callers' segment sums are CSR-ordered, so outputs and input gradients under a cap are BYTE-equal to the
uncapped run.  Parameter gradients are not: the number of partial rows (one per workgroup of a backward = per compute unit) and, for some
contractions, the weight-gradient plan depend on the count; they agree to rounding.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from moldiff_amd import _lib
from moldiff_amd import train_ops as T
from tests import fused_train_cases as C
from tests import util as U

gpu = pytest.mark.gpu

SIZES = {
    'two': [5, 7],                        # 62 edges, 4 tiles
    'degenerate': [1, 7, 2, 1, 0, 5],     # 64 edges, 4 full tiles
    'three': [24, 31, 18],                # 1,788 edges, 112 tiles, 12 rows in the last
    'six': [33, 2, 12, 2, 0, 24],         # 1,744 edges, 109 full tiles
    'ragged': [2, 9, 17, 3, 5, 7],        # 414 edges, 26 tiles, 14 rows in the last
    'full': [22, 7, 3, 2],                # 512 edges, 32 full tiles
}
CASES = [('two', 3), ('degenerate', 2), ('three', 1), ('three', 2), ('three', 3), ('ragged', 1), ('ragged', 2), ('six', 1), ('six', 3),
         ('full', 1)]
KERNELS = {'bond_ffn': ('bondffn_fwd', 'bondffn_bwd'),
           'edge_block': ('bondffn_fwd', 'bondffn_bwd', 'edge_tail_fwd', 'edge_tail_bwd'),
           'pos_update': ('posffn_fwd', 'posffn_bwd'),
           'node_block': ('nodemsg_fwd', 'nodemsg_bwd')}
OPS = tuple(KERNELS)
DEVICE_CUS = 256      # an MI355X; the coverage test also takes the count of the device it runs on, where there is one
WANTED = {(k, r, t) for k in _lib.FUSED_KERNELS for r in 'abcd' for t in ('ragged', 'even')}


def n_edges(name):
    return sum(n * (n - 1) for n in SIZES[name])


def regimes(kernel, E, n_cus):
    """{(regime, tile case)} of one fused kernel for E rows on n_cus compute units"""
    p = _lib.fused_grid(kernel, E, n_cus)
    nw, tile = p['grid'] * p['waves'], 'even' if E % 16 == 0 else 'ragged'
    assert p['tiles'] == (E + 15) // 16 and p['last_rows'] == E - 16 * (p['tiles'] - 1)
    assert (p['rounds'] - 1) * nw + p['last_tiles'] == p['tiles'] and 0 < p['last_tiles'] <= nw
    if p['rounds'] == 1:
        return {('a', tile)}
    if p['last_tiles'] == nw:
        return {('b', tile)}
    busy = -(-p['last_tiles'] // p['waves'])      # workgroups with a tile in the last round
    return ({('c', tile)} if p['last_tiles'] % p['waves'] else set()) | ({('d', tile)} if busy < p['grid'] else set())


def test_the_cases_cover_every_regime():
    """No GPU needed: the grid export is host code."""
    for name in SIZES:
        bn, hei, bh, ei, be = U.graph_from_sizes(SIZES[name])
        assert ei.shape[1] == n_edges(name) <= 2000
    got = {(k, r, t) for name, cap in CASES for k in _lib.FUSED_KERNELS for r, t in regimes(k, n_edges(name), cap)}
    assert got == WANTED, sorted(WANTED - got)
    # worked by hand: [24, 31, 18] is 112 tiles with 12 rows in the last, 14 full rounds under cap 1 and 4 full rounds + 16
    # tiles (workgroup 2 idle) under cap 3; [2, 9, 17, 3, 5, 7] is 26 tiles, 3 rounds + 2 under cap 1 and 1 round + 10 under cap 2
    keys = ('grid', 'waves', 'tiles', 'rounds', 'last_tiles', 'last_rows')
    for kernel in ('bondffn_fwd', 'bondffn_bwd', 'edge_tail_bwd', 'posffn_fwd', 'posffn_bwd', 'nodemsg_bwd'):
        assert _lib.fused_grid(kernel, 1788, 1) == dict(zip(keys, (1, 8, 112, 14, 8, 12)))
        assert _lib.fused_grid(kernel, 1788, 3) == dict(zip(keys, (3, 8, 112, 5, 16, 12)))
        assert _lib.fused_grid(kernel, 414, 1) == dict(zip(keys, (1, 8, 26, 4, 2, 14)))
        assert _lib.fused_grid(kernel, 414, 2) == dict(zip(keys, (2, 8, 26, 2, 10, 14)))
    assert _lib.fused_grid('edge_tail_fwd', 1788, 3)['grid'] == 6          # two workgroups per CU
    # a backward always launches one workgroup per CU, a forward no more than it has tiles for
    assert _lib.fused_grid('bondffn_bwd', 62, 3)['grid'] == 3 and _lib.fused_grid('bondffn_fwd', 62, 3)['grid'] == 1
    assert _lib.fused_grid('nodemsg_bwd', 0, 3) == dict(zip(keys, (3, 8, 0, 0, 0, 0)))
    with pytest.raises(ValueError):
        _lib.fused_grid('bondffn', 16, 1)
    assert _lib.lib().mdx_debug_fused_grid_host(8, 16, 1, (ctypes.c_int32 * 6)()) != 0       # no ninth kernel
    # without a cap these sizes reach regime a only: nothing above is covered by the uncapped tests
    counts = {DEVICE_CUS}
    if torch.cuda.is_available():
        counts.add(torch.cuda.get_device_properties(0).multi_processor_count)
    for n_cus in counts:
        for name in SIZES:
            for k in _lib.FUSED_KERNELS:
                assert {r for r, t in regimes(k, n_edges(name), n_cus)} == {'a'}, (name, k, n_cus)
    # the launchers read the cap: what they do "right now" is what they do on a device of that many compute units
    with _lib.cu_cap(2):
        assert all(_lib.fused_grid(k, 1788) == _lib.fused_grid(k, 1788, 2) for k in _lib.FUSED_KERNELS)


# ---- operators, inputs and references: one per (operator, size list), made once ------------------------------------------------------

_cache = {}


def _case(op, name):
    """the operator on the batch, its uncapped fused run (never modified: the byte reference) and its per-operator run"""
    key = (op, name)
    if key not in _cache:
        c = C.CASES[op](SIZES[name], 41) if op == 'bond_ffn' else C.CASES[op](SIZES[name])
        _cache[key] = dict(case=c, base=c.run(True), perop=c.run(False))
    return _cache[key]


def _fp64(op, name):
    d = _case(op, name)
    if 'fp64' not in d:
        d['fp64'] = d['case'].run64()
    return d['fp64']


def _same_bytes(a, b):
    """outputs and input gradients of two runs, bit for bit"""
    return torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in b[1])


def _check_against_per_operator(op, got, ref):
    """the bounds tests/test_gpu_fused_train.py holds the fused path to against the per-operator composition"""
    o1, gl1, gp1 = got
    o0, gl0, gp0 = ref
    assert set(gp1) == set(gp0)
    if op == 'bond_ffn':
        assert C.rel(o1, o0) < 2e-3, C.rel(o1, o0)
        for k in gl0:
            assert C.rel(gl1[k], gl0[k]) < 4e-3, (k, C.rel(gl1[k], gl0[k]))
        for k in gp0:
            assert torch.isfinite(gp1[k]).all(), k
            assert C.rel(gp1[k], gp0[k]) < 6e-3, (k, C.rel(gp1[k], gp0[k]))
        return
    assert C.rel(o1, o0) < 3e-3, C.rel(o1, o0)
    for k in gl0:
        assert C.rel2(gl1[k], gl0[k]) < 1e-2, (k, C.rel2(gl1[k], gl0[k]))
    for k in gp0:
        assert torch.isfinite(gp1[k]).all(), k
        assert C.rel2(gp1[k], gp0[k]) < 1e-2, (k, C.rel2(gp1[k], gp0[k]))


@gpu
@pytest.mark.parametrize('name,cap', CASES)
@pytest.mark.parametrize('op', OPS)
def test_fused_operator_under_a_cu_cap(op, name, cap):
    """Forward + backward uncapped, under the cap (forward, backward and the reduction of the parameter gradients inside it), uncapped
    again.  Output, dL/dX, dL/dh (and dL/dpos of PosUpdate) under the cap are the uncapped bytes, and so is the third run (nothing is
    left behind); parameter gradients are finite and within 2e-3 of the uncapped fused run's (the bound of the sink-vs-autograd tests);
    the capped run keeps the fused-vs-per-operator bounds."""
    d = _case(op, name)
    case, base = d['case'], d['base']
    with _lib.cu_cap(cap):
        got = case.run(True)
        torch.cuda.synchronize()
    after = case.run(True)
    torch.cuda.synchronize()
    worst = max(C.rel(got[2][k], base[2][k]) for k in base[2])
    print(f'\n[{op} {name} E={case.E} cap {cap}] ' + ' '.join(
        f"{k}: {sorted(r + t[0] for r, t in regimes(k, case.E, cap))}" for k in KERNELS[op]) + f' | parameter gradients vs uncapped: {worst:.2e}')
    assert _same_bytes(got, base), 'the capped run differs from the uncapped run'
    assert _same_bytes(after, base), 'the run after the cap differs from the run before it'
    for k in base[2]:
        assert torch.isfinite(got[2][k]).all(), k
        assert C.rel(got[2][k], base[2][k]) < 2e-3, (k, C.rel(got[2][k], base[2][k]))
        assert C.rel(after[2][k], base[2][k]) < 2e-3, (k, C.rel(after[2][k], base[2][k]))
    _check_against_per_operator(op, got, d['perop'])


@gpu
@pytest.mark.parametrize('op', OPS)
def test_a_backward_workgroup_without_a_tile_leaves_a_zero_partial_row(op, monkeypatch):
    """[5, 7] is four tiles: under cap 3 every fused backward launches three workgroups, the first takes all tiles, and the partial rows
    of LayerNorm-parameter gradients of the other two -- which the reduction adds like any other -- must be zero."""
    case = _case(op, 'two')['case']
    seen = []
    real = T._fused_param_grads

    def spy(ps, need, contractions, lnp, slices):
        seen.append(lnp.detach().clone())
        return real(ps, need, contractions, lnp, slices)

    monkeypatch.setattr(T, '_fused_param_grads', spy)
    with _lib.cu_cap(3):
        assert all(_lib.fused_grid(k, case.E)['grid'] == 3 and _lib.fused_grid(k, case.E)['tiles'] <= 8 for k in KERNELS[op] if k.endswith('bwd'))
        case.run(True)
        torch.cuda.synchronize()
    assert len(seen) == {'bond_ffn': 1, 'edge_block': 3, 'pos_update': 1, 'node_block': 1}[op]
    for lnp in seen:
        assert lnp.shape[0] == 3 and torch.isfinite(lnp).all()
        assert float(lnp[0].abs().max()) > 0 and float(lnp[1:].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize('cap', [1, 3])
@pytest.mark.parametrize('op', OPS)
def test_fused_operator_with_the_gradient_sink_under_a_cu_cap(op, cap):
    """Inside a gradient sink the deferred reduction reads `cap` partial rows per fused backward: the flat gradient buffer against the
    no-sink run under the same cap, within 2e-3 (tests/test_gpu_fused_train.py, ..._with_the_gradient_sink_equals_autograd_accumulation).
    A module of its own: the flat buffers take over the parameters' storage."""
    from moldiff_amd.trainer import FlatParams
    case = C.CASES[op](SIZES['three'], 43) if op == 'bond_ffn' else C.CASES[op](SIZES['three'])
    with _lib.cu_cap(cap):
        ref = case.run(True)
        flat = FlatParams(case.m)
        got = case.run(True, sink=flat)
        torch.cuda.synchronize()
    for k in ref[2]:
        assert torch.isfinite(got[2][k]).all(), k
        assert C.rel(got[2][k], ref[2][k]) < 2e-3, (k, C.rel(got[2][k], ref[2][k]))


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------

def _e0_table(doc):
    """{operator: {tensor: measured e0}} from the table in the float64 test's docstring"""
    out = {}
    for op, name, e0, cap in re.findall(r'^ +(edge_block|pos_update|node_block) +(\S+) +(\S+) +(\S+)$', doc, re.M):
        assert abs(float(cap) - 1.5 * float(e0)) <= 1e-3 * float(cap), (op, name)
        out.setdefault(op, {})[name] = float(e0)
    return out


@gpu
@pytest.mark.parametrize('cap', [0, 3])
@pytest.mark.parametrize('op', ['edge_block', 'pos_update', 'node_block'])
def test_fused_operator_against_fp64_autograd_of_the_reference_formula(op, cap):
    """The fused path, uncapped and under cap 3 (regime d, the ragged tile in round 5), vs torch autograd in float64 on the reference's
    formula (models/graph.py:268-294 and :360, :384-396, :29-55; restated in tests/fused_train_cases.py).  The inputs are float16 values,
    exact in float64.  Forward within 3e-3 of the output scale.  Gradients: the yardstick is e0, the per-operator path's relative L2
    distance to float64 on the same inputs -- float16 arithmetic lands some LayerNorm -> ReLU pre-activations on the other side of zero
    than float64 (tests/test_gpu_fused_train.py, the BondFFN's float64 test), so e0 is percents for any float16 evaluation.  The fused
    path is held to e1 <= 1.02 e0 + 1e-4 on every tensor (none needed the wider triangle bound e0 + 1e-2: the largest measured excess
    is 0.5 % of e0, on bond_ffn_left.gate.net.0.bias and right_lin_edge.net.0.bias) and to an absolute cap of 1.5 x the e0 measured on an
    MI355X for these seeds; the factor covers kink flips, which differ from input to input.  Measured on [24, 31, 18] (the fused
    path's e1 equals e0 to three digits on every row, uncapped and under cap 3 alike):

        operator   tensor                                   e0         cap = 1.5 e0
        edge_block dx                                       3.638e-03  5.457e-03
        edge_block dh                                       1.887e-02  2.831e-02
        edge_block bond_ffn_left.bond_linear.weight         2.343e-02  3.514e-02
        edge_block bond_ffn_left.node_linear.weight         2.398e-02  3.597e-02
        edge_block bond_ffn_left.inter_module.net.0.weight  2.323e-02  3.485e-02
        edge_block bond_ffn_left.inter_module.net.0.bias    1.049e-02  1.573e-02
        edge_block bond_ffn_left.inter_module.net.1.weight  7.636e-03  1.145e-02
        edge_block bond_ffn_left.inter_module.net.1.bias    9.057e-03  1.359e-02
        edge_block bond_ffn_left.inter_module.net.3.weight  7.908e-03  1.186e-02
        edge_block bond_ffn_left.inter_module.net.3.bias    7.626e-03  1.144e-02
        edge_block bond_ffn_left.gate.net.0.weight          9.635e-03  1.445e-02
        edge_block bond_ffn_left.gate.net.0.bias            4.899e-03  7.348e-03
        edge_block bond_ffn_left.gate.net.1.weight          3.887e-03  5.830e-03
        edge_block bond_ffn_left.gate.net.1.bias            4.339e-03  6.509e-03
        edge_block bond_ffn_left.gate.net.3.weight          3.965e-03  5.947e-03
        edge_block bond_ffn_left.gate.net.3.bias            3.349e-03  5.024e-03
        edge_block bond_ffn_right.bond_linear.weight        1.676e-02  2.514e-02
        edge_block bond_ffn_right.node_linear.weight        1.784e-02  2.676e-02
        edge_block bond_ffn_right.inter_module.net.0.weight 1.719e-02  2.579e-02
        edge_block bond_ffn_right.inter_module.net.0.bias   5.614e-03  8.421e-03
        edge_block bond_ffn_right.inter_module.net.1.weight 4.467e-03  6.700e-03
        edge_block bond_ffn_right.inter_module.net.1.bias   5.344e-03  8.016e-03
        edge_block bond_ffn_right.inter_module.net.3.weight 4.921e-03  7.382e-03
        edge_block bond_ffn_right.inter_module.net.3.bias   4.825e-03  7.238e-03
        edge_block bond_ffn_right.gate.net.0.weight         9.127e-03  1.369e-02
        edge_block bond_ffn_right.gate.net.0.bias           3.585e-03  5.378e-03
        edge_block bond_ffn_right.gate.net.1.weight         4.097e-03  6.145e-03
        edge_block bond_ffn_right.gate.net.1.bias           3.980e-03  5.970e-03
        edge_block bond_ffn_right.gate.net.3.weight         3.916e-03  5.874e-03
        edge_block bond_ffn_right.gate.net.3.bias           3.237e-03  4.855e-03
        edge_block node_ffn_left.weight                     1.153e-02  1.730e-02
        edge_block node_ffn_left.bias                       9.169e-03  1.375e-02
        edge_block node_ffn_right.weight                    1.204e-02  1.806e-02
        edge_block node_ffn_right.bias                      9.191e-03  1.379e-02
        edge_block self_ffn.weight                          1.309e-02  1.963e-02
        edge_block self_ffn.bias                            9.151e-03  1.373e-02
        edge_block layer_norm.weight                        1.336e-03  2.004e-03
        edge_block layer_norm.bias                          6.284e-03  9.426e-03
        edge_block out_transform.weight                     4.791e-04  7.186e-04
        edge_block out_transform.bias                       2.043e-04  3.064e-04
        pos_update dx                                       2.096e-02  3.144e-02
        pos_update dh                                       1.956e-02  2.934e-02
        pos_update dpos                                     1.083e-03  1.625e-03
        pos_update left_lin_edge.net.0.weight               1.878e-02  2.817e-02
        pos_update left_lin_edge.net.0.bias                 1.820e-02  2.730e-02
        pos_update left_lin_edge.net.1.weight               2.096e-02  3.144e-02
        pos_update left_lin_edge.net.1.bias                 1.739e-02  2.608e-02
        pos_update left_lin_edge.net.3.weight               2.163e-02  3.245e-02
        pos_update left_lin_edge.net.3.bias                 2.315e-02  3.472e-02
        pos_update right_lin_edge.net.0.weight              2.083e-02  3.125e-02
        pos_update right_lin_edge.net.0.bias                2.124e-02  3.186e-02
        pos_update right_lin_edge.net.1.weight              1.785e-02  2.678e-02
        pos_update right_lin_edge.net.1.bias                1.875e-02  2.812e-02
        pos_update right_lin_edge.net.3.weight              2.266e-02  3.399e-02
        pos_update right_lin_edge.net.3.bias                2.405e-02  3.607e-02
        pos_update edge_lin.bond_linear.weight              2.246e-02  3.369e-02
        pos_update edge_lin.node_linear.weight              2.135e-02  3.202e-02
        pos_update edge_lin.inter_module.net.0.weight       1.991e-02  2.987e-02
        pos_update edge_lin.inter_module.net.0.bias         1.358e-02  2.037e-02
        pos_update edge_lin.inter_module.net.1.weight       2.559e-03  3.838e-03
        pos_update edge_lin.inter_module.net.1.bias         1.234e-02  1.851e-02
        pos_update edge_lin.inter_module.net.3.weight       7.734e-04  1.160e-03
        pos_update edge_lin.inter_module.net.3.bias         6.099e-04  9.149e-04
        pos_update edge_lin.gate.net.0.weight               2.561e-03  3.841e-03
        pos_update edge_lin.gate.net.0.bias                 1.821e-03  2.731e-03
        pos_update edge_lin.gate.net.1.weight               8.174e-04  1.226e-03
        pos_update edge_lin.gate.net.1.bias                 3.081e-03  4.621e-03
        pos_update edge_lin.gate.net.3.weight               1.099e-03  1.648e-03
        pos_update edge_lin.gate.net.3.bias                 1.246e-03  1.869e-03
        node_block dx                                       2.621e-02  3.932e-02
        node_block dh                                       2.156e-02  3.234e-02
        node_block node_net.net.0.weight                    2.306e-02  3.459e-02
        node_block node_net.net.0.bias                      2.363e-02  3.545e-02
        node_block node_net.net.1.weight                    2.198e-02  3.297e-02
        node_block node_net.net.1.bias                      2.308e-02  3.462e-02
        node_block node_net.net.3.weight                    2.113e-02  3.170e-02
        node_block node_net.net.3.bias                      2.150e-02  3.225e-02
        node_block edge_net.net.0.weight                    2.463e-02  3.694e-02
        node_block edge_net.net.0.bias                      2.268e-02  3.402e-02
        node_block edge_net.net.1.weight                    2.193e-02  3.290e-02
        node_block edge_net.net.1.bias                      2.176e-02  3.264e-02
        node_block edge_net.net.3.weight                    2.135e-02  3.202e-02
        node_block edge_net.net.3.bias                      2.128e-02  3.192e-02
        node_block msg_net.weight                           2.459e-02  3.689e-02
        node_block msg_net.bias                             2.579e-02  3.868e-02
        node_block gate.net.0.weight                        2.125e-02  3.188e-02
        node_block gate.net.0.bias                          8.882e-03  1.332e-02
        node_block gate.net.1.weight                        8.142e-03  1.221e-02
        node_block gate.net.1.bias                          8.134e-03  1.220e-02
        node_block gate.net.3.weight                        8.778e-03  1.317e-02
        node_block gate.net.3.bias                          4.738e-03  7.107e-03
        node_block centroid_lin.weight                      1.673e-02  2.509e-02
        node_block centroid_lin.bias                        1.610e-02  2.415e-02
        node_block layer_norm.weight                        9.590e-03  1.438e-02
        node_block layer_norm.bias                          2.099e-02  3.148e-02
        node_block out_transform.weight                     4.820e-04  7.230e-04
        node_block out_transform.bias                       2.105e-04  3.158e-04
    """
    E0 = _e0_table(test_fused_operator_against_fp64_autograd_of_the_reference_formula.__doc__)
    d = _case(op, 'three')
    ref = _fp64(op, 'three')
    with _lib.cu_cap(cap):
        got = d['case'].run(True)
        torch.cuda.synchronize()
    base = d['perop']
    assert C.rel(got[0], ref[0]) < 3e-3, C.rel(got[0], ref[0])
    rows = [('d' + k, got[1][k], base[1][k], ref[1][k]) for k in ref[1]] + [(k, got[2][k], base[2][k], ref[2][k]) for k in ref[2]]
    errs = [(n, C.rel2(g, r), C.rel2(b, r), C.rel(g, r), C.rel(b, r)) for n, g, b, r in rows]
    print(f'\n[fused {op} vs fp64, cap {cap}]  tensor: relative L2 fused, per-operator | max-norm fused, per-operator')
    for n, e1, e0, m1, m0 in errs:
        print(f'    {n:44s} {e1:.3e}  {e0:.3e} | {m1:.3e}  {m0:.3e}')
    assert {n for n, *_ in errs} == set(E0[op]), sorted({n for n, *_ in errs} ^ set(E0[op]))
    for n, e1, e0, m1, m0 in errs:
        assert np.isfinite(e1) and e1 <= 1.5 * E0[op][n], (n, e1, E0[op][n])
        assert e1 <= 1.02 * e0 + 1e-4, (n, e1, e0)
