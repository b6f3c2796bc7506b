"""Fused row-owner training operators (round 6, csrc/mdx_train_fused.hip): the EdgeBlock's BondFFN + scatter_sum as one forward and
one backward launch, against (a) the per-operator composition of the same module in the same float16 autocast arithmetic (same
rounding points: agreement to a few float16 ulp) and (b) the fp64 evaluation of the reference formula (models/graph.py:133-141,
:272-279 through torch autograd)."""
import numpy as np
import pytest
import torch

from moldiff_amd import graph as G
from moldiff_amd import train_graph as TG
from moldiff_amd import train_ops as T
from tests import fused_train_cases as C
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _setup(sizes, seed, scale=1.0):
    c = C.bond_ffn_case(sizes, seed, scale)
    return c.m, c.leaves['x'], c.leaves['h'], c.consts['te'], c.g_out, c.tg


def _run(m, x, h, te, gS, tg, fused):
    m.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    h = h.clone().requires_grad_(True)
    with C.fused_path(fused), T.precision('fp16'):
        out = TG.bond_ffn_scatter(m, x, te, h, tg.left, tg.right)
        out.backward(gS)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    return out.detach(), x.grad.detach(), h.grad.detach(), grads


_rel, _rel2 = C.rel, C.rel2


def _both_paths(case):
    """(out, *input gradients, parameter gradients) of the fused and of the per-operator path"""
    return [(o, *gl.values(), gp) for o, gl, gp in (case.run(True), case.run(False))]


@pytest.mark.parametrize('sizes', [[5, 7, 4], [24, 31, 18, 27, 22, 25, 30, 19, 26, 23], [2, 2, 3]])
def test_fused_bondffn_equals_the_per_operator_composition(sizes):
    """Same arithmetic, same rounding points, another summation order inside the LayerNorm statistics and the MFMA chains: outputs and
    every gradient within 2e-3 of the per-operator path relative to the tensor's largest entry (a float16 ulp is 1e-3)."""
    args = _setup(sizes, 11)
    o1, gx1, gh1, gr1 = _run(*args, fused=True)
    o0, gx0, gh0, gr0 = _run(*args, fused=False)
    assert o1.dtype == o0.dtype and gx1.dtype == gx0.dtype and gh1.dtype == gh0.dtype
    assert _rel(o1, o0) < 2e-3, _rel(o1, o0)
    assert _rel(gx1, gx0) < 4e-3, _rel(gx1, gx0)
    assert _rel(gh1, gh0) < 4e-3, _rel(gh1, gh0)
    assert set(gr1) == set(gr0)
    for k in gr0:
        assert torch.isfinite(gr1[k]).all(), k
        assert _rel(gr1[k], gr0[k]) < 6e-3, (k, _rel(gr1[k], gr0[k]))


def test_fused_bondffn_against_fp64_autograd_of_the_reference_formula():
    """The fused path vs torch autograd in float64 on the reference's formula: forward within 3e-3 of the output scale.  Gradients: in
    float16 arithmetic ~1e-3 of the 800 k LayerNorm->ReLU pre-activations of this batch land on the other side of zero than in float64,
    and each such kink event changes its row's gradient discretely -- the MAXIMUM over rows is therefore O(10 %) for ANY float16
    evaluation (measured 18 % on dL/dX for both paths, to four digits the same number: the fused kernels take the per-operator path's
    rounding points, so they flip the same units).  Asserted: relative L2 distance to float64 below 6 % and equal to the per-operator
    path's within 2 % of it, i.e. the fused node is as far from exact arithmetic as autocast's own arithmetic, not further."""
    m, x, h, te, gS, tg = _setup([24, 31, 18, 27, 22, 25, 30, 19], 13)
    o1, gx1, gh1, gr1 = _run(m, x, h, te, gS, tg, fused=True)
    o0, gx0, gh0, gr0 = _run(m, x, h, te, gS, tg, fused=False)
    P = {k: p.detach().double().clone().requires_grad_(True) for k, p in m.named_parameters()}
    xd, hd = x.double().clone().requires_grad_(True), h.double().clone().requires_grad_(True)
    li, ri = tg.left.index, tg.right.index
    F = torch.nn.functional

    def mlp(pre, v):
        v = F.linear(v, P[pre + '.net.0.weight'], P[pre + '.net.0.bias'])
        v = torch.relu(F.layer_norm(v, (v.shape[1],), P[pre + '.net.1.weight'], P[pre + '.net.1.bias'], 1e-5))
        return F.linear(v, P[pre + '.net.3.weight'], P[pre + '.net.3.bias'])
    node = hd[li]
    inter = mlp('inter_module', F.linear(xd, P['bond_linear.weight']) * F.linear(node, P['node_linear.weight']))
    gate = mlp('gate', torch.cat([xd, node, te.double()], -1))
    out = torch.zeros(hd.shape[0], 64, dtype=torch.float64, device=DEV).index_add_(0, ri, inter * torch.sigmoid(gate))
    out.backward(gS.double())
    assert _rel(o1, out.detach()) < 3e-3
    rows = [('dX', gx1, gx0, xd.grad), ('dh', gh1, gh0, hd.grad)] + [(k, gr1[k], gr0[k], P[k].grad) for k in gr1]
    errs = [(name, _rel2(got, ref), _rel2(base, ref), _rel(got, ref), _rel(base, ref)) for name, got, base, ref in rows]
    print('\n[fused BondFFN vs fp64]  tensor: relative L2 fused, per-operator | max-norm fused, per-operator')
    for name, e1, e0, m1, m0 in errs:
        print(f'    {name:28s} {e1:.3e}  {e0:.3e} | {m1:.3e}  {m0:.3e}')
    for name, e1, e0, m1, m0 in errs:
        assert e1 < 6e-2, (name, e1)
        assert e1 <= 1.02 * e0 + 1e-4, (name, e1, e0)


def test_fused_bondffn_with_the_gradient_sink_equals_autograd_accumulation():
    """Inside Trainer.step the weight gradients bypass autograd (train_ops.grad_sink): the fused node's six weight-gradient contractions
    and its LayerNorm-parameter partial rows must land in the flat gradient buffer exactly as the returned tensors would."""
    from moldiff_amd.trainer import FlatParams
    m, x, h, te, gS, tg = _setup([24, 31, 18, 27, 22, 25, 30, 19], 17)
    _, _, _, ref = _run(m, x, h, te, gS, tg, fused=True)
    flat = FlatParams(m)
    flat.grad.zero_()
    old, old_rows = T._FUSED, T.FUSED_MIN_ROWS
    T._FUSED, T.FUSED_MIN_ROWS = True, 1
    try:
        with T.grad_sink(flat), T.precision('fp16'):
            out = TG.bond_ffn_scatter(m, x.clone().requires_grad_(True), te, h.clone().requires_grad_(True), tg.left, tg.right)
            out.backward(gS)
    finally:
        T._FUSED, T.FUSED_MIN_ROWS = old, old_rows
    for k, p in m.named_parameters():
        got = p.grad if p.grad is not None else None
        assert got is not None, k
        assert _rel(got, ref[k]) < 2e-3, (k, _rel(got, ref[k]))


def test_fused_bondffn_with_a_sink_that_holds_some_of_its_parameters():
    """A sink over the inter module alone: Wi1, bi1, g1, be1, Wi2 and bi2 are deferred into the flat gradient buffer, the other eight
    parameters of the same fused node return through autograd.  Every parameter's gradient must be what the no-sink fused run gives."""
    from moldiff_amd.trainer import FlatParams
    m, x, h, te, gS, tg = _setup([5, 7, 4], 19)
    _, _, _, ref = _run(m, x, h, te, gS, tg, fused=True)
    m.zero_grad(set_to_none=True)
    flat = FlatParams(m.inter_module)
    inside = {id(p) for p in flat.params}
    assert len(inside) == 6 and any(id(p) not in inside for p in m.parameters())
    old, old_rows = T._FUSED, T.FUSED_MIN_ROWS
    T._FUSED, T.FUSED_MIN_ROWS = True, 1
    try:
        with T.grad_sink(flat), T.precision('fp16'):
            out = TG.bond_ffn_scatter(m, x.clone().requires_grad_(True), te, h.clone().requires_grad_(True), tg.left, tg.right)
            out.backward(gS)
    finally:
        T._FUSED, T.FUSED_MIN_ROWS = old, old_rows
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert _rel(p.grad, ref[k]) < 2e-3, (k, _rel(p.grad, ref[k]))


# ---------------------------------------------------------------------------------------------------------------------------
# EdgeBlock (two fused BondFFNs + the fused tail with the residual) against the per-operator composition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [[5, 7, 4], [24, 31, 18, 27, 22, 25, 30, 19, 26, 23]])
def test_fused_edge_block_with_residual_equals_the_per_operator_composition(sizes):
    """h + EdgeBlock(h) (models/graph.py:268-294, :360) with both BondFFNs and the tail fused vs the per-operator path in the same float16
    arithmetic: output within 2 float16 ulp of its scale; gradients within 1 % in L2 (individual rows may sit on different sides of a ReLU kink once the
    two paths' LayerNorm statistics differ in the last bit)."""
    (o1, gx1, gh1, gr1), (o0, gx0, gh0, gr0) = _both_paths(C.edge_block_case(sizes))
    assert o1.dtype == o0.dtype == torch.float16 and gx1.dtype == gx0.dtype
    print(f'\n[fused EdgeBlock vs per-operator] out max {_rel(o1, o0):.2e}  dX L2 {_rel2(gx1, gx0):.2e}  dh L2 {_rel2(gh1, gh0):.2e}')
    for k in gr0:
        print(f'    {k:40s} L2 {_rel2(gr1[k], gr0[k]):.2e}')
    assert _rel(o1, o0) < 3e-3, _rel(o1, o0)
    assert _rel2(gx1, gx0) < 1e-2 and _rel2(gh1, gh0) < 1e-2, (_rel2(gx1, gx0), _rel2(gh1, gh0))
    for k in gr0:
        assert torch.isfinite(gr1[k]).all(), k
        assert _rel2(gr1[k], gr0[k]) < 1e-2, (k, _rel2(gr1[k], gr0[k]))


# ---------------------------------------------------------------------------------------------------------------------------
# PosUpdate with the fused front of its BondFFN against the per-operator composition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [[5, 7, 4], [24, 31, 18, 27, 22, 25, 30, 19, 26, 23]])
def test_fused_pos_update_equals_the_per_operator_composition(sizes):
    """PosUpdate.forward (models/graph.py:384-396) with gather / product / bond_linear / node_linear / gate MLP fused into one launch each
    way: the position increment and every gradient against the per-operator path in the same float16 arithmetic."""
    (o1, gx1, gh1, gp1, gr1), (o0, gx0, gh0, gp0, gr0) = _both_paths(C.pos_update_case(sizes))
    print(f'\n[fused PosUpdate vs per-operator] out max {_rel(o1, o0):.2e}  dX L2 {_rel2(gx1, gx0):.2e}  dh L2 {_rel2(gh1, gh0):.2e}  dpos L2 {_rel2(gp1, gp0):.2e}')
    for k in gr0:
        print(f'    {k:40s} L2 {_rel2(gr1[k], gr0[k]):.2e}')
    assert _rel(o1, o0) < 3e-3, _rel(o1, o0)
    assert _rel2(gx1, gx0) < 1e-2 and _rel2(gh1, gh0) < 1e-2 and _rel2(gp1, gp0) < 1e-2
    for k in gr0:
        assert torch.isfinite(gr1[k]).all(), k
        assert _rel2(gr1[k], gr0[k]) < 1e-2, (k, _rel2(gr1[k], gr0[k]))


# ---------------------------------------------------------------------------------------------------------------------------
# NodeBlock with the fused message path (streamed weights) against the per-operator composition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [[5, 7, 4], [24, 31, 18, 27, 22, 25, 30, 19, 26, 23]])
def test_fused_node_block_equals_the_per_operator_composition(sizes):
    """NodeBlock.forward (models/graph.py:29-55) with edge_net, the product with node_net(x)[col], msg_net, the gate MLP and the sigmoid
    product in one launch each way (weights streamed as float16 A-operand packs): output and every gradient against the per-operator
    path in the same float16 arithmetic."""
    (o1, gx1, gh1, gr1), (o0, gx0, gh0, gr0) = _both_paths(C.node_block_case(sizes))
    print(f'\n[fused NodeBlock vs per-operator] out max {_rel(o1, o0):.2e}  dX L2 {_rel2(gx1, gx0):.2e}  dh L2 {_rel2(gh1, gh0):.2e}')
    for k in gr0:
        print(f'    {k:40s} L2 {_rel2(gr1[k], gr0[k]):.2e}')
    assert _rel(o1, o0) < 3e-3, _rel(o1, o0)
    assert _rel2(gx1, gx0) < 1e-2 and _rel2(gh1, gh0) < 1e-2
    for k in gr0:
        assert torch.isfinite(gr1[k]).all(), k
        assert _rel2(gr1[k], gr0[k]) < 1e-2, (k, _rel2(gr1[k], gr0[k]))


@pytest.mark.parametrize('sink', [True, False])
def test_posffn_front_outputs_are_freed_without_backward(sink):
    """The fused PosUpdate front keeps its outputs prod (E,256) and gate (E,1) for the backward.  Held on the autograd context they
    formed a cycle (output -> grad_fn -> ctx -> output): a forward that is never back-propagated kept them until the cyclic collector
    ran.  Saved through save_for_backward they are freed as soon as the caller drops them -- inside a float16 sink and without one
    (one autograd class serves both)."""
    import gc
    import weakref
    from moldiff_amd.trainer import FlatParams
    g = U.rng(37)
    bn, hei, bh, ei, be = U.graph_from_sizes([24, 31, 18, 27])
    N, E = len(bn), ei.shape[1]
    m = G.PosUpdate(256, 64, 64, True).to(DEV)
    flat = FlatParams(m)
    ff = m.edge_lin
    g0, gt = ff.gate.net[0], ff.gate.net
    params = dict(Wb=ff.bond_linear.weight, Wn=ff.node_linear.weight, Wg1x=g0.weight[:, :64], Wg1a=g0.weight[:, 64:128],
                  Wt=g0.weight[:, 128:], bg1=g0.bias, gg=gt[1].weight, gbe=gt[1].bias, Wg2=gt[3].weight, bg2=gt[3].bias)
    he = torch.from_numpy(g.standard_normal((E, 64)).astype(np.float32)).to(DEV).half().requires_grad_(True)
    lf, rf = (torch.from_numpy(g.standard_normal((N, 64)).astype(np.float32)).to(DEV).half() for _ in range(2))
    te = torch.from_numpy(g.random((E, 1)).astype(np.float32)).to(DEV)
    tg = TG.TrainGraph(ei.to(DEV), N)
    old_rows, was_enabled = T.FUSED_MIN_ROWS, gc.isenabled()
    T.FUSED_MIN_ROWS = 1
    gc.disable()
    try:
        with T.grad_sink(flat) if sink else torch.enable_grad(), T.precision('fp16'):
            assert T.posffn_fused_ok(he, lf, rf, (64, 64, 256, 32, 1))
            prod, gate = T.posffn_front(he, lf, rf, te, tg.left, tg.right, params)
            name = type(prod.grad_fn).__name__
            refs = weakref.ref(prod), weakref.ref(gate)
            del prod, gate
        torch.cuda.synchronize()
        assert name == '_PosFfnFrontBackward', name
        assert refs[0]() is None and refs[1]() is None
    finally:
        T.FUSED_MIN_ROWS = old_rows
        if was_enabled:
            gc.enable()
