"""Per-launch time of the up-move of resampling (mdx_forward_jump) next to the scaffold merge (mdx_scaffold_merge), on the benchmark's
config #2 batch (256 molecules, MolDiff_simple): is the forward jump anything next to a sampling step?

    python tools/time_forward_jump.py [--calls 200] [--warmup 20] [--repeats 3] [--out profiles/forward_jump.txt]

One sampler with a scaffold and the path num_steps = 100, jump_length = 10, resample = 2.  Each timed window is `calls` consecutive
library calls between two device events after `warmup` untimed ones; the windows of the two kernels alternate.  Both are timed with
the noise already in its buffers (draw < 0: the one launch named) and with the library's Philox launch in front (draw >= 0: two
launches).  A window of `steps` whole down-moves gives the step time they are compared with.  Not part of bench.py.
"""
import ctypes

import numpy as np
import torch

import evalbench as EB


def main():
    ap = EB.parser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    args = EB.parse(ap)
    import bench
    from moldiff_amd import Scaffold, _lib
    dev = torch.device(args.device)
    model, ph, sizes = bench.build_workload(args.batch, 0, dev)
    model = model.to(dev)
    bn, hei, bh = ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge']
    N, Eh = int(bn.numel()), int(bh.numel())
    g = np.random.Generator(np.random.PCG64(1))
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    mask = np.zeros(N, dtype=bool)
    for o, n in zip(off, sizes):
        mask[o:o + min(8, int(n))] = True
    sc = Scaffold(torch.from_numpy(mask).to(dev), torch.from_numpy(g.integers(0, 7, N)).to(dev),
                  torch.from_numpy(g.standard_normal((N, 3)).astype(np.float32)).to(dev), torch.from_numpy(g.integers(0, 5, Eh)).to(dev))
    sm = model.sampler(args.batch, bn, hei, bh, seed=1, return_traj=False, scaffold=sc, num_steps=100, jump_length=10, resample=2)
    sm.init()
    P, L = _lib.ptr, _lib.lib()
    nxt = sm._state(1, 1, 1)

    def jump(draw):
        nz = sm._step_noise(draw)
        _lib.check(L.mdx_forward_jump(sm.g.h, ctypes.byref(sm.fwd), 0, P(sm.node_ids[0]), P(sm.half_ids[0]), P(sm.pos_traj[0]),
                                      ctypes.byref(nz), ctypes.byref(nxt), _lib.log_eps32(), P(sm.node_ids[1]), P(sm.half_ids[1]),
                                      _lib.stream()))

    def merge(draw):
        nz = sm._step_noise(draw)
        _lib.check(L.mdx_scaffold_merge(sm.g.h, ctypes.byref(sm.sc_tabs), 500, ctypes.byref(sm.sc), ctypes.byref(nz), ctypes.byref(nxt),
                                        _lib.log_eps32(), P(sm.node_ids[1]), P(sm.half_ids[1]), None, None, None, _lib.stream()))

    state = {'k': 0}

    def down(_):
        sm.move(state['k'])                  # the first walk of the first block: down-moves only
        state['k'] = (state['k'] + 1) % 10

    jobs = {'forward_jump (1 launch)': (jump, -1, args.calls), 'scaffold_merge (1 launch)': (merge, -1, args.calls),
            'forward_jump + philox': (jump, 7, args.calls), 'scaffold_merge + philox': (merge, 7, args.calls),
            'down-move (whole step + merge)': (down, 0, args.steps)}
    for fn, draw, n in jobs.values():
        for _ in range(min(args.warmup, n)):
            fn(draw)
    torch.cuda.synchronize()
    us = {name: [] for name in jobs}
    for _ in range(args.repeats):
        for name, (fn, draw, n) in jobs.items():
            us[name].append(1e3 * EB.timed(lambda: fn(draw), n, warmup=0)[0])
    lines = [f'# tools/time_forward_jump.py --calls {args.calls} --steps {args.steps} --warmup {args.warmup} --repeats {args.repeats} --batch {args.batch}',
             f'# {torch.cuda.get_device_name(0)}; {args.batch} molecules, {N} atoms, {Eh} half-edges; exact fp32 matrix path',
             '# microseconds per call: device events around each window of consecutive calls (back-to-back launches from Python, so a',
             '# short kernel is bounded below by the host\'s launch rate), windows alternate']
    for name, v in us.items():
        lines.append(f'{name:32s} windows {" ".join("%.2f" % x for x in v)}   median {np.median(v):.2f}')
    step = np.median(us['down-move (whole step + merge)'])
    lines.append(f'forward_jump + philox / down-move (medians) {np.median(us["forward_jump + philox"]) / step:.5f}')
    EB.report(lines, args.out)


if __name__ == '__main__':
    main()
