"""Shared set-up of the fused float16 training-operator tests (tests/test_gpu_fused_train.py, tests/test_gpu_fused_train_rounds.py): the
four operators' modules with their weight recipes, their inputs on a ragged batch, one forward + backward of either path (fused kernels
or the per-operator composition), the two error measures, and the float64 restatement of each operator's reference formula."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from moldiff_amd import graph as G
from moldiff_amd import train_graph as TG
from moldiff_amd import train_ops as T
from tests import util as U

DEV = 'cuda:0'


def rel2(a, b):
    """relative L2 distance"""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


def rel(a, b):
    """largest difference over the reference's largest entry"""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


@contextlib.contextmanager
def fused_path(fused):
    """the fused kernels (or the per-operator composition) at every row count"""
    old, old_rows = T._FUSED, T.FUSED_MIN_ROWS
    T._FUSED, T.FUSED_MIN_ROWS = fused, 1
    try:
        yield
    finally:
        T._FUSED, T.FUSED_MIN_ROWS = old, old_rows


def fill(m, g, weight, gain, other):
    """the tests' weight recipe: matrices N(0, weight^2 / fan_in), LayerNorm gains 1 + gain N(0, 1), every other vector other N(0, 1)"""
    with torch.no_grad():
        for k, p in sorted(m.named_parameters()):
            if p.dim() == 2:
                p.copy_(torch.from_numpy((g.standard_normal(tuple(p.shape)) * (weight / np.sqrt(p.shape[1]))).astype(np.float32)))
            elif ('net.1.' in k or 'layer_norm' in k) and k.endswith('weight'):
                p.copy_(torch.from_numpy((1.0 + gain * g.standard_normal(tuple(p.shape))).astype(np.float32)))
            else:
                p.copy_(torch.from_numpy((other * g.standard_normal(tuple(p.shape))).astype(np.float32)))


def _normal(g, shape, scale=1.0):
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32)).to(DEV)


def _uniform(g, shape):
    return torch.from_numpy(g.random(shape).astype(np.float32)).to(DEV)


class Case:
    """One operator on one batch: module `m`, differentiated inputs `leaves` (name -> tensor, in the order of run()'s gradients),
    constants `consts`, the cotangent `g_out` and the graph `tg`."""

    def __init__(self, m, leaves, consts, g_out, tg, forward, forward64):
        self.m, self.leaves, self.consts, self.g_out, self.tg = m, leaves, consts, g_out, tg
        self._forward, self._forward64 = forward, forward64
        self.E = int(tg.left.index.numel())

    def run(self, fused, sink=None):
        """forward + backward in float16 autocast arithmetic -> (out, {leaf: gradient}, {parameter: gradient}).  With `sink` (a
        trainer.FlatParams of the module) the parameter gradients bypass autograd into the flat buffer, as inside Trainer.step."""
        if sink is None:
            self.m.zero_grad(set_to_none=True)
        else:
            sink.zero_grad()
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.leaves.items()}
        with fused_path(fused):
            with (T.grad_sink(sink) if sink is not None else contextlib.nullcontext()), T.precision('fp16'):
                out = self._forward(self.m, self.tg, **leaves, **self.consts)
                out.backward(self.g_out)
        return (out.detach(), {k: v.grad.detach() for k, v in leaves.items()},
                {k: p.grad.detach().clone() for k, p in self.m.named_parameters()})

    def run64(self):
        """the reference formula in float64 through torch autograd, on the same (float16-valued) inputs -> like run()"""
        P = {k: p.detach().double().clone().requires_grad_(True) for k, p in self.m.named_parameters()}
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in self.leaves.items()}
        consts = {k: v.double() for k, v in self.consts.items()}
        out = self._forward64(P, self.tg.left.index, self.tg.right.index, **leaves, **consts)
        out.backward(self.g_out.double())
        return out.detach(), {k: v.grad for k, v in leaves.items()}, {k: p.grad for k, p in P.items()}


# ---- float64 restatements of the reference formulas (models/common.py MLP: Linear -> LayerNorm -> ReLU -> Linear) ----------------------

def mlp64(P, pre, v):
    v = F.linear(v, P[pre + '.net.0.weight'], P[pre + '.net.0.bias'])
    v = torch.relu(F.layer_norm(v, (v.shape[1],), P[pre + '.net.1.weight'], P[pre + '.net.1.bias'], 1e-5))
    return F.linear(v, P[pre + '.net.3.weight'], P[pre + '.net.3.bias'])


def bond_ffn64(P, pre, bond, node, time):
    """BondFFN.forward, models/graph.py:133-141"""
    inter = mlp64(P, pre + 'inter_module', F.linear(bond, P[pre + 'bond_linear.weight']) * F.linear(node, P[pre + 'node_linear.weight']))
    return inter * torch.sigmoid(mlp64(P, pre + 'gate', torch.cat([bond, node, time], -1)))


def scatter64(src, index, n):
    return torch.zeros(n, src.shape[1], dtype=src.dtype, device=src.device).index_add_(0, index, src)


def bond_ffn_scatter64(P, li, ri, x, h, te):
    """models/graph.py:278-279: the left BondFFN of an EdgeBlock, summed over the right node's edges"""
    return scatter64(bond_ffn64(P, '', x, h[li], te), ri, h.shape[0])


def edge_block64(P, li, ri, x, h, te):
    """h_bond + EdgeBlock(h_bond), models/graph.py:268-294 and :360"""
    n = h.shape[0]
    left = scatter64(bond_ffn64(P, 'bond_ffn_left.', x, h[li], te), ri, n)[li]
    right = scatter64(bond_ffn64(P, 'bond_ffn_right.', x, h[ri], te), li, n)[ri]
    v = (left + right + F.linear(h[li], P['node_ffn_left.weight'], P['node_ffn_left.bias'])
         + F.linear(h[ri], P['node_ffn_right.weight'], P['node_ffn_right.bias']) + F.linear(x, P['self_ffn.weight'], P['self_ffn.bias']))
    v = F.layer_norm(v, (v.shape[1],), P['layer_norm.weight'], P['layer_norm.bias'], 1e-5)
    return x + F.linear(torch.relu(v), P['out_transform.weight'], P['out_transform.bias'])


def pos_update64(P, li, ri, x, h, pos, te):
    """PosUpdate.forward, models/graph.py:384-396, on rel = pos[left] - pos[right] and its norm (:371-372)"""
    w = bond_ffn64(P, 'edge_lin.', x, mlp64(P, 'left_lin_edge', h[li]) * mlp64(P, 'right_lin_edge', h[ri]), te)
    r = pos[li] - pos[ri]
    d = r.norm(dim=-1, keepdim=True)
    return scatter64(w * r / d / (d + 1.0), li, h.shape[0])


def node_block64(P, li, ri, x, h, tn):
    """NodeBlock.forward, models/graph.py:29-55 (row = left, col = right)"""
    msg = F.linear(mlp64(P, 'edge_net', x) * mlp64(P, 'node_net', h)[ri], P['msg_net.weight'], P['msg_net.bias'])
    msg = msg * torch.sigmoid(mlp64(P, 'gate', torch.cat([x, h[ri], tn[ri]], -1)))
    v = F.linear(h, P['centroid_lin.weight'], P['centroid_lin.bias']) + scatter64(msg, li, h.shape[0])
    v = F.layer_norm(v, (v.shape[1],), P['layer_norm.weight'], P['layer_norm.bias'], 1e-5)
    return F.linear(torch.relu(v), P['out_transform.weight'], P['out_transform.bias'])


# ---- the four operators ---------------------------------------------------------------------------------------------------------------

def _graph(sizes):
    bn, hei, bh, ei, be = U.graph_from_sizes(sizes)
    return len(bn), ei.shape[1], ei


def bond_ffn_case(sizes, seed, scale=1.0):
    """the EdgeBlock's BondFFN + scatter_sum (train_graph.bond_ffn_scatter)"""
    g = U.rng(seed)
    N, E, ei = _graph(sizes)
    m = G.BondFFN(64, 256, 128, True).to(DEV)
    fill(m, g, 1.2, 0.4, 0.3)
    x = _normal(g, (E, 64), scale).half()
    h = _normal(g, (N, 256)).half()
    te = _uniform(g, (E, 1))
    gS = _normal(g, (N, 64))
    tg = TG.TrainGraph(ei.to(DEV), N)
    return Case(m, dict(x=x, h=h), dict(te=te), gS, tg,
                lambda m, tg, x, h, te: TG.bond_ffn_scatter(m, x, te, h, tg.left, tg.right), bond_ffn_scatter64)


def edge_block_case(sizes, seed=23):
    """h + EdgeBlock(h): two fused BondFFNs and the fused tail with the residual"""
    g = U.rng(seed)
    N, E, ei = _graph(sizes)
    m = G.EdgeBlock(64, 256).to(DEV)
    fill(m, g, 1.0, 0.3, 0.2)
    x = _normal(g, (E, 64)).half()
    h = _normal(g, (N, 256)).half()
    te = _uniform(g, (E, 1))
    g_out = _normal(g, (E, 64)).half()
    tg = TG.TrainGraph(ei.to(DEV), N)
    return Case(m, dict(x=x, h=h), dict(te=te), g_out, tg,
                lambda m, tg, x, h, te: TG.edge_block(m, x, tg, h, te, residual=True), edge_block64)


def _pos_update(m, tg, x, h, pos, te):
    r, dist = T.edge_geom(pos, tg.left, tg.right)
    return TG.pos_update(m, h, x, tg, r, dist, te)


def pos_update_case(sizes, seed=29):
    """PosUpdate with the fused front of its BondFFN, from the positions on (train_ops.edge_geom)"""
    g = U.rng(seed)
    N, E, ei = _graph(sizes)
    m = G.PosUpdate(256, 64, 64, True).to(DEV)
    fill(m, g, 1.0, 0.3, 0.2)
    he = _normal(g, (E, 64)).half()
    hn = _normal(g, (N, 256)).half()
    pos = _normal(g, (N, 3), 2.0)
    te = _uniform(g, (E, 1))
    g_out = _normal(g, (N, 3))
    tg = TG.TrainGraph(ei.to(DEV), N)
    return Case(m, dict(x=he, h=hn, pos=pos), dict(te=te), g_out, tg, _pos_update, pos_update64)


def node_block_case(sizes, seed=31):
    """NodeBlock with the fused message path (streamed weights)"""
    g = U.rng(seed)
    N, E, ei = _graph(sizes)
    m = G.NodeBlock(256, 64, 256, True).to(DEV)
    fill(m, g, 1.0, 0.3, 0.2)
    he = _normal(g, (E, 64)).half()
    hn = _normal(g, (N, 256)).half()
    tn = _uniform(g, (N, 1))
    g_out = _normal(g, (N, 256)).half()
    tg = TG.TrainGraph(ei.to(DEV), N)
    return Case(m, dict(x=he, h=hn), dict(te=tn), g_out, tg,
                lambda m, tg, x, h, te: TG.node_block(m, h, tg, x, te), lambda P, li, ri, x, h, te: node_block64(P, li, ri, x, h, te))


CASES = dict(bond_ffn=bond_ffn_case, edge_block=edge_block_case, pos_update=pos_update_case, node_block=node_block_case)
