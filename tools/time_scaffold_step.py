"""Step time of the sampler with and without a scaffold, on the benchmark's config #2 batch (256 molecules, MolDiff_simple, exact
fp32 matrix path): does the merge of scaffold-constrained sampling (mdx_scaffold_merge) cost anything a user would see?

    python tools/time_scaffold_step.py [--steps 200] [--warmup 20] [--repeats 3] [--out profiles/scaffold_step.txt]
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- python tools/time_scaffold_step.py --mode plain|scaffold --steps 20 --repeats 1

Both samplers are built in ONE process on the same library; each timed window is `steps` consecutive sampler.step() calls between
two device events after `warmup` untimed steps, and the two samplers alternate (`repeats` windows each) so that drift of the machine
hits both.  The scaffold fixes the first 8 atoms of every molecule and the bonds among them.  `--mode plain|scaffold` runs one of the
two only (for a kernel trace: the difference of the two traces' launch counts, divided by the number of steps, is the number of
launches a conditioned step adds).  Not part of bench.py: the headline measures the unconditioned chain, which this leaves alone.
"""
import numpy as np
import torch

import evalbench as EB


def main():
    ap = EB.parser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--fixed', type=int, default=8, help='atoms held fixed at the front of every molecule')
    ap.add_argument('--mode', choices=('both', 'plain', 'scaffold'), default='both')
    args = EB.parse(ap)
    import bench
    from moldiff_amd import Scaffold
    dev = torch.device(args.device)
    model, ph, sizes = bench.build_workload(args.batch, 0, dev)
    model = model.to(dev)
    bn, hei, bh = ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge']
    N, Eh = int(bn.numel()), int(bh.numel())
    g = np.random.Generator(np.random.PCG64(1))
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    mask = np.zeros(N, dtype=bool)
    for o, n in zip(off, sizes):
        mask[o:o + min(args.fixed, int(n))] = True
    sc = Scaffold(torch.from_numpy(mask).to(dev), torch.from_numpy(g.integers(0, 7, N)).to(dev),
                  torch.from_numpy(g.standard_normal((N, 3)).astype(np.float32)).to(dev), torch.from_numpy(g.integers(0, 5, Eh)).to(dev))
    samplers = {}
    if args.mode in ('both', 'plain'):
        samplers['plain'] = model.sampler(args.batch, bn, hei, bh, seed=1, return_traj=False)
    if args.mode in ('both', 'scaffold'):
        samplers['scaffold'] = model.sampler(args.batch, bn, hei, bh, seed=1, return_traj=False, scaffold=sc)
    nxt = {}
    for name, sm in samplers.items():
        sm.init()
        for i in range(args.warmup):
            sm.step(i)
        nxt[name] = args.warmup
    torch.cuda.synchronize()
    ms = {name: [] for name in samplers}
    for _ in range(args.repeats):
        for name, sm in samplers.items():
            steps = iter(range(nxt[name], nxt[name] + args.steps))
            ms[name].append(EB.timed(lambda: sm.step(next(steps)), args.steps, warmup=0)[0])
            nxt[name] += args.steps
    lines = [f'# tools/time_scaffold_step.py --steps {args.steps} --warmup {args.warmup} --repeats {args.repeats} --batch {args.batch} '
             f'--fixed {args.fixed}',
             f'# {torch.cuda.get_device_name(0)}; {args.batch} molecules, {N} atoms, {Eh} half-edges; {int(mask.sum())} atoms and '
             f'{int((mask[hei[0].cpu().numpy()] & mask[hei[1].cpu().numpy()]).sum())} half-edges fixed; exact fp32 matrix path',
             '# ms per step: device events around each window of consecutive sampler.step() calls, windows alternate']
    for name, v in ms.items():
        lines.append(f'{name:9s} windows {" ".join("%.4f" % x for x in v)}   median {np.median(v):.4f}   min {min(v):.4f}   max {max(v):.4f}')
    if len(ms) == 2:
        lines.append(f'ratio scaffold / plain (medians) {np.median(ms["scaffold"]) / np.median(ms["plain"]):.4f}')
    EB.report(lines, args.out)


if __name__ == '__main__':
    main()
