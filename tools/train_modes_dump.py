"""One-off behaviour check for changes to the host side of the training operators (development tool, GPU box): dumps what a training step
computes in every precision mode, so that a build before and a build after such a change can be compared bit for bit.

  python tools/train_modes_dump.py OUT.pt            two Trainer.steps per mode of train_ops.KINDS (plus 'fp16' with the fused row-owner
                                                     operators forced on) and one get_loss forward + backward WITHOUT a gradient sink in
                                                     'f32' and 'fp16': loss, gradient norm, flat.grad after each step, flat.data
  python tools/train_modes_dump.py --compare A B     every dumped tensor under torch.equal; exit status 1 on any difference

Model, batch and noise are those of tests/test_gpu_trainer.py::test_cpp_nodes_are_bit_identical_to_the_python_bodies."""
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda:0'


def _fresh(base):
    m = copy.deepcopy(base)
    for mod in m.modules():
        if hasattr(mod, '_eng'):
            mod._eng, mod._eng_sig = None, None
    return m


def dump(path):
    from tests import util as U
    from moldiff_amd import train_ops
    from moldiff_amd.trainer import Trainer
    base = U.moldiff('MolDiff', DEV)
    g = U.rng(41)
    sizes = (9, 14, 7, 12, 10, 6)
    bn, hei, bh, _, _ = U.graph_from_sizes(list(sizes), DEV)
    N, Eh = len(bn), len(bh)
    pos = U.t32(g.standard_normal((N, 3)) * 1.5).to(DEV)
    batch = (torch.from_numpy(g.integers(0, 7, N)).to(DEV), pos, bn, torch.from_numpy((g.random(Eh) < 0.3) * g.integers(1, 5, Eh)).to(DEV),
             hei, bh, len(sizes))
    t = torch.tensor([0, 100, 300, 500, 700, 999], device=DEV)
    g = U.rng(42)
    noise = dict(eps_pos=U.t32(g.standard_normal((N, 3))).to(DEV), u_node=U.t32(g.random((N, 8))).to(DEV),
                 u_halfedge=U.t32(g.random((Eh, 6))).to(DEV))
    out = {}
    old_rows = train_ops.FUSED_MIN_ROWS
    for name, kind, fused_rows in [(k, k, old_rows) for k in train_ops.KINDS] + [('fp16_fused', 'fp16', 1)]:
        train_ops.FUSED_MIN_ROWS = fused_rows
        try:
            scaled = train_ops.KINDS[kind] is not None and train_ops.KINDS[kind][0] == 2 and train_ops.KINDS[kind][1]
            tr = Trainer(_fresh(base), lr=1e-4, max_grad_norm=50.0, precision=kind, init_scale=256.0 if scaled else None)
            for step in (1, 2):
                o = tr.step(*batch, time_step=t, noise=noise)
                out[f'{name}/step{step}/loss'] = o['loss'].detach().float().cpu()
                out[f'{name}/step{step}/grad_norm'] = o['grad_norm'].detach().float().cpu()
                out[f'{name}/step{step}/flat.grad'] = tr.flat.grad.detach().cpu().clone()
            out[f'{name}/flat.data'] = tr.flat.data.detach().cpu().clone()
        finally:
            train_ops.FUSED_MIN_ROWS = old_rows
        print(name, float(out[f'{name}/step1/loss']), float(out[f'{name}/step2/loss']), float(out[f'{name}/step2/grad_norm']), flush=True)
    for kind, scale in (('f32', 1.0), ('fp16', 256.0)):      # no sink, no transposed parameters: every gradient through autograd
        m = _fresh(base)
        with train_ops.precision(kind):
            o = m.get_loss(*batch, time_step=t, noise=noise)
        (o['loss'] * scale).backward()
        out[f'nosink_{kind}/loss'] = o['loss'].detach().float().cpu()
        out[f'nosink_{kind}/grads'] = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().float().reshape(-1).cpu()
                                                 for p in m.parameters()])
        print('nosink', kind, float(o['loss'].detach()), float(out[f'nosink_{kind}/grads'].abs().max()), flush=True)
    torch.cuda.synchronize()
    torch.save(out, path)
    print('wrote', path, len(out), 'tensors')


def compare(a, b):
    A, B = torch.load(a), torch.load(b)
    bad = sorted(set(A) ^ set(B))
    for k in sorted(set(A) & set(B)):
        # (bit patterns: torch.equal of the values, except that a NaN equals the same NaN)
        same = A[k].shape == B[k].shape and torch.equal(A[k].reshape(-1).view(torch.int32), B[k].reshape(-1).view(torch.int32))
        nz = float(A[k].abs().max())
        print(f'{k:32s} {"equal" if same else "DIFFERENT"}   numel {A[k].numel():9d}   max |a| {nz:.6g}')
        if not same:
            bad.append(k)
    print('ALL EQUAL' if not bad else f'DIFFERENT OR MISSING: {bad}')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
