"""Wall time of strided sampling on the benchmark's config #2 batch (256 molecules, MolDiff_simple, exact fp32 matrix path): whole
runs of MolDiff.sample at 1000 (the full chain, no keyword) / 250 / 100 / 50 steps, the per-iteration time of a jump iteration against
an ordinary one, and the number of kernel launches of each.

    python tools/time_strided_sampling.py [--out FILE] [--window 200] [--repeats 3] [--no-launch-count]
    python tools/time_strided_sampling.py --mode plain|jump --iters 20      (one sampler, `iters` iterations: what the launch count traces)

Whole runs: MolDiff.sample(..., return_traj=False) between two host clock reads with a device synchronisation before each, after one
untimed 50-step run.  Per iteration: two samplers in ONE process on the same library, an ordinary one and one on the 250-level schedule
(every move a jump of 4 levels); each timed window is `window` consecutive step() calls between two device events after 20 untimed
ones, and the two alternate (`repeats` windows each) so that drift of the machine hits both.  Launch count: this script run four times
as a child under `rocprofv3 --kernel-trace` (plain / jump, 10 and 20 iterations) before the parent touches the GPU; the difference of
the traces' row counts divided by 10 is the number of launches of one iteration, whatever the set-up launches.
Says nothing about sample QUALITY at reduced step counts: no trained checkpoint is available.  Not part of bench.py.
"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

import evalbench as EB
JUMP_LEVELS = 250


def _workload(batch, device):
    import bench
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    model, ph, _ = bench.build_workload(batch, 0, dev)
    return model.to(dev), (ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge'])


def _child(args):
    model, g = _workload(args.batch, args.device)
    sm = model.sampler(args.batch, *g, seed=1, return_traj=False, **({} if args.mode == 'plain' else {'num_steps': JUMP_LEVELS}))
    sm.init()
    for i in range(args.iters):
        sm.step(i)
    torch.cuda.synchronize()


def _launches_per_iteration(mode, batch):
    rows = {}
    for iters in (10, 20):
        with tempfile.TemporaryDirectory() as d:
            # `timeout` ends the profiler AND the Python child that holds the GPU; stderr is kept for the error message
            r = subprocess.run(['timeout', '-k', '10', '240', 'rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', d, '-o', 'p',
                                '--', sys.executable, os.path.abspath(__file__), '--mode', mode, '--iters', str(iters), '--batch', str(batch)],
                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                raise RuntimeError(f'kernel trace of mode {mode}, {iters} iterations: exit status {r.returncode}\n{r.stderr[-2000:]}')
            files = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)
            if not files:
                raise RuntimeError('rocprofv3 wrote no kernel trace')
            rows[iters] = sum(sum(1 for _ in csv.reader(open(f))) - 1 for f in files)
    return (rows[20] - rows[10]) / 10.0


def main():
    ap = EB.parser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, nargs='+', default=[1000, 250, 100, 50])
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--mode', choices=('all', 'plain', 'jump'), default='all')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--note', type=str, action='append', default=[], help='line appended to the output (e.g. a figure measured on '
                                                                          'another build in the same session)')
    args = ap.parse_args()   # not EB.parse: the parent must not open the GPU before its traced children have run
    if args.mode != 'all':
        return _child(args)
    launches = None
    if not args.no_launch_count:   # children first: the parent has not opened the GPU yet
        launches = {mode: _launches_per_iteration(mode, args.batch) for mode in ('plain', 'jump')}
    model, g = _workload(args.batch, args.device)
    T = model.num_timesteps
    N, Eh = int(g[0].numel()), int(g[2].numel())
    model.sample(args.batch, *g, seed=1, return_traj=False, num_steps=50)   # warm-up
    runs = []
    for m in args.steps:
        kw = {} if m == T else {'num_steps': m}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.sample(args.batch, *g, seed=1, return_traj=False, **kw)
        torch.cuda.synchronize()
        runs.append((m, time.perf_counter() - t0))
    samplers = {'plain': model.sampler(args.batch, *g, seed=1, return_traj=False),
                'jump': model.sampler(args.batch, *g, seed=1, return_traj=False, num_steps=JUMP_LEVELS)}
    nxt = {}
    for name, sm in samplers.items():
        sm.init()
        for i in range(20):
            sm.step(i)
        nxt[name] = 20
    torch.cuda.synchronize()
    ms = {name: [] for name in samplers}
    for _ in range(args.repeats):
        for name, sm in samplers.items():
            if nxt[name] + args.window > (T if name == 'plain' else JUMP_LEVELS) - 1:   # start the chain again, untimed
                sm.init()
                nxt[name] = 0
            steps = iter(range(nxt[name], nxt[name] + args.window))
            ms[name].append(EB.timed(lambda: sm.step(next(steps)), args.window, warmup=0)[0])
            nxt[name] += args.window
    lines = [f'# tools/time_strided_sampling.py --batch {args.batch} --window {args.window} --repeats {args.repeats}',
             f'# {torch.cuda.get_device_name(0)}; {args.batch} molecules, {N} atoms, {Eh} half-edges; MolDiff_simple, exact fp32 matrix path, '
             f'T = {T}',
             '# sample quality at reduced step counts is NOT measured here (no trained checkpoint); guidance is not rescaled',
             '# whole runs of MolDiff.sample(return_traj=False), host clock around a synchronised run, after a warm-up run']
    full = dict(runs).get(T)
    for m, sec in runs:
        lines.append(f'steps {m:5d}   wall {sec:8.3f} s   {1e3 * sec / m:7.3f} ms per iteration' +
                     (f'   {full / sec:6.2f} x faster than {T} steps' if full and m != T else ''))
    lines.append(f'# ms per iteration: device events around windows of {args.window} consecutive step() calls, windows alternate; '
                 f'jump = the {JUMP_LEVELS}-level schedule')
    for name, v in ms.items():
        lines.append(f'{name:6s} windows {" ".join("%.4f" % x for x in v)}   median {np.median(v):.4f}   min {min(v):.4f}   max {max(v):.4f}')
    lines.append(f'ratio jump / plain (medians) {np.median(ms["jump"]) / np.median(ms["plain"]):.4f}')
    if launches is not None:
        lines.append(f'kernel launches per iteration (kernel trace, (20 iterations - 10 iterations) / 10): plain {launches["plain"]:.1f}   '
                     f'jump {launches["jump"]:.1f}')
    lines += args.note
    EB.report(lines, args.out)


if __name__ == '__main__':
    main()
