"""Device time of the molecule quality check next to the decode it follows: the device part of FeaturizeMol.decode_batch
(mdx_decode_output) and of FeaturizeMol.check_batch (decode + mdx_mol_check, and with largest_fragment the selection +
mdx_mol_keep_component), at 256 and 2,048 molecules of the placeholder sizes (GEOM-Drugs atom-count statistics).

    python tools/time_mol_check.py [--calls 200] [--warmup 20] [--repeats 3] [--out profiles/mol_check_timing.txt]

Predictions are random logits (about one atom in eight decodes to the mask type, about one half-edge in three to a bond: far more
fragments and sweeps than a trained model's output, so the check's share is if anything overstated).  Each timed window is `calls`
consecutive calls between two device events after `warmup` untimed ones; the windows of the variants alternate, `repeats` times.
The host part (copies and per-molecule slicing) is the same with and without the check but for three more copies, and is not timed
here.  To set the numbers against decode_batch on another commit, run this file's 'decode' row there.  Not part of bench.py.
"""
import numpy as np
import torch

import evalbench as EB


def main():
    ap = EB.parser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 2048])
    args = EB.parse(ap)
    from moldiff_amd import _lib
    from moldiff_amd.harness import make_data_placeholder
    from moldiff_amd.postprocess import FeaturizeMol
    dev = torch.device(args.device)
    feat = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    lines = []
    for B in args.batches:
        np.random.seed(2023)
        ph = make_data_placeholder(B, dev)
        bn, hei, bh = ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge']
        N, Eh = int(bn.numel()), int(bh.numel())
        g = torch.Generator(device='cpu').manual_seed(B)
        pred = [(3 * torch.randn(N, 8, generator=g)).to(dev), torch.randn(N, 3, generator=g).to(dev),
                (3 * torch.randn(Eh, 6, generator=g) + torch.tensor([2.5, 0, 0, 0, 0, 0])).to(dev)]
        graph = _lib.graph_for_halfedges(hei, bn, B)

        def decode():
            return feat._decode_device(pred, bn, hei, B, graph)[1]

        jobs = {'decode (mdx_decode_output)': decode,
                'decode + check': lambda: feat._check_device(graph, decode()),
                'decode + check + largest_fragment 0.5': lambda: feat._check_device(graph, decode(), None, 0.5)}
        for fn in jobs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        us = {name: [] for name in jobs}
        for _ in range(args.repeats):
            for name, fn in jobs.items():
                us[name].append(1000.0 * EB.timed(fn, args.calls, warmup=0)[0])
        ri = feat._check_device(graph, decode())[0].cpu().numpy()
        lines.append(f'{B} molecules, {N} atoms, {Eh} half-edges; decoded: {int(ri[4].sum())} atoms, {int((ri[0] == 1).sum())} connected, '
                     f'{float(ri[0].mean()):.1f} fragments per molecule')
        for name, v in us.items():
            lines.append(f'  {name:40s} median {np.median(v):8.1f} us per call   (windows of {args.calls}: ' +
                         ', '.join(f'{x:.1f}' for x in v) + ')')
    EB.report(lines, args.out, 'tools/time_mol_check.py: device time per call, hipEvents around windows of consecutive calls (allocations of the '
              'output tensors included)')


if __name__ == '__main__':
    main()
