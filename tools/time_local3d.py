"""Device time of the local 3D geometry statistics next to the decode they follow: the device part of FeaturizeMol.decode_batch
(mdx_decode_output) and of FeaturizeMol.local3d_batch (decode + mdx_mol_local3d), at 256 and 2,048 molecules of the placeholder sizes
(GEOM-Drugs atom-count statistics), in the manner of tools/time_mol_check.py.

    python tools/time_local3d.py [--calls 200] [--warmup 20] [--repeats 3] [--out profiles/local3d_timing.txt]

Predictions are random logits, about one atom in eight decoding to the mask type, at two bond densities set by the bias of the no-bond
logit (--bond_bias): 8.0 gives about one bond per atom, the density of a drug-like molecule, and so the number of angles and dihedrals a
user's batch has; 2.5, the input of tools/time_mol_check.py, gives about five bonds per atom and some 200 times as many dihedrals per
molecule, a regime no sampled molecule is in, kept to show how the cost follows the item count.  The patterns are the 20 / 13 / 15 most frequent lengths / angles / dihedrals of the same
batch (local3d.frequent_patterns on the decoded molecules), with the default bins: 7,440 bins, counted per workgroup in LDS; a second
row doubles the bin counts, which puts the tables over the LDS budget and every item's add into global memory.  Each timed window is
`calls` consecutive calls between two device events after `warmup` untimed ones; the windows of the variants alternate, `repeats` times;
every call adds into the same statistics object, as the sampling entry point does.  Not part of bench.py.
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
    ap.add_argument('--bond_bias', type=float, nargs='+', default=[8.0, 2.5])
    args = EB.parse(ap)
    from moldiff_amd import _lib
    from moldiff_amd import local3d as L3
    from moldiff_amd.harness import make_data_placeholder
    from moldiff_amd.postprocess import FeaturizeMol
    dev = torch.device(args.device)
    feat = FeaturizeMol([6, 7, 8, 9, 15, 16, 17], [1, 2, 3, 4], use_mask_node=True, use_mask_edge=True)
    lines = []
    for bias in args.bond_bias:
        for B in args.batches:
            np.random.seed(2023)
            ph = make_data_placeholder(B, dev)
            bn, hei, bh = ph['batch_node'], ph['halfedge_index'], ph['batch_halfedge']
            N, Eh = int(bn.numel()), int(bh.numel())
            g = torch.Generator(device='cpu').manual_seed(B)
            pred = [(3 * torch.randn(N, 8, generator=g)).to(dev), torch.randn(N, 3, generator=g).to(dev),
                    (3 * torch.randn(Eh, 6, generator=g) + torch.tensor([bias, 0, 0, 0, 0, 0])).to(dev)]
            graph = _lib.graph_for_halfedges(hei, bn, B)
            some = feat.decode_batch(pred, bn, hei, bh, B, graph)[:64]       # patterns from a part of the same batch
            pats = [[p for p, _ in L3.frequent_patterns(some, k, top)] for k, top in zip(L3.KINDS, (20, 13, 15))]
            spec = L3.Local3DSpec(*pats)
            wide = L3.Local3DSpec(*pats, length_bins=(1.0, 2.2, 240), angle_bins=(0, 180, 360), dihedral_bins=(-180, 180, 360))
            outs = {s: L3.device_stats(s, dev) for s in (spec, wide)}

            def decode():
                return feat._decode_device(pred, bn, hei, B, graph)[1]

            def stats(s):
                return feat.local3d_batch(pred, bn, hei, bh, B, s, graph, out=outs[s])

            jobs = {'decode (mdx_decode_output)': decode,
                    f'decode + local3d, {spec.hist_size} bins (LDS)': lambda: stats(spec),
                    f'decode + local3d, {wide.hist_size} bins (global)': lambda: stats(wide)}
            for fn in jobs.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            us = {name: [] for name in jobs}
            for _ in range(args.repeats):
                for name, fn in jobs.items():
                    us[name].append(1000.0 * EB.timed(fn, args.calls, warmup=0)[0])
            one = feat.local3d_batch(pred, bn, hei, bh, B, spec, graph).cpu()
            lines.append(f'no-bond bias {bias}: {B} molecules, {N} atoms, {Eh} half-edges, {int(one.n_items[0]) / max(N, 1):.1f} bonds per atom; per call {one.n_items.tolist()} lengths / angles / dihedrals, '
                         f'{int(one.hist.sum())} binned, {int(one.outside.sum())} outside, patterns {[len(p) for p in pats]}')
            for name, v in us.items():
                lines.append(f'  {name:44s} median {np.median(v):8.1f} us per call   (windows of {args.calls}: ' +
                             ', '.join(f'{x:.1f}' for x in v) + ')')
    EB.report(lines, args.out, 'tools/time_local3d.py: device time per call, hipEvents around windows of consecutive calls (allocations of the '
              'output tensors included)')


if __name__ == '__main__':
    main()
