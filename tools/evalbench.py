"""What the timing scripts under tools/ share, once each: the synthetic molecule generators, the batch builder, the event-timed window,
the common command-line options, the output tail and the choice of an alternative library build.  The scripts import this module and
``moldiff_amd`` and never each other.  Importing it puts the repository root on ``sys.path``.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ELEMENTS = (6, 7, 8, 9, 15, 16, 17)


def drug_like(g, atoms):
    """two to four rings of 5 or 6 atoms, each fused to the previous one along a bond, then chains grown from random atoms"""
    size = int(g.choice([5, 6]))
    bonds = [(k, (k + 1) % size) for k in range(size)]
    n, last = size, (0, 1)
    for _ in range(int(g.integers(1, 4))):
        size = int(g.choice([5, 6]))
        new = list(range(n, n + size - 2))
        path = [last[0]] + new + [last[1]]
        bonds += [(path[k], path[k + 1]) for k in range(len(path) - 1)]
        last, n = (new[0], new[1]), n + size - 2
    while n < atoms:
        bonds.append((int(g.integers(0, n)), n))
        n += 1
    ele = g.choice(ELEMENTS, n, p=[0.7, 0.1, 0.12, 0.02, 0.01, 0.03, 0.02])
    idx = np.asarray(bonds, dtype=np.int64).T
    bt = g.choice([1, 2, 4], len(bonds), p=[0.6, 0.1, 0.3])
    return {'element': ele.astype(np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}


def extended(g, atoms):
    """``drug_like`` + a para-substituted aromatic ring on a random atom carrying a CF3, and a tert-butyl on another"""
    m = drug_like(g, atoms)
    n = len(m['element'])
    nb = m['bond_index'].shape[1] // 2
    bonds = [(int(i), int(j), int(t)) for (i, j), t in zip(m['bond_index'][:, :nb].T, m['bond_type'][:nb])]
    ele = m['element'].tolist()
    a, b = (int(x) for x in g.choice(n, 2, replace=False))
    r = n                                                              # the ring r .. r + 5, attached at r, the CF3 at r + 3
    bonds += [(a, r, 1)] + [(r + k, r + (k + 1) % 6, 4) for k in range(6)] + [(r + 3, r + 6, 1)] + [(r + 6, r + 7 + k, 1) for k in range(3)]
    ele += [6] * 7 + [9] * 3
    t = r + 10                                                         # the tert-butyl: t and its three methyls
    bonds += [(b, t, 1)] + [(t, t + 1 + k, 1) for k in range(3)]
    ele += [6] * 4
    idx = np.asarray([(i, j) for i, j, _ in bonds], dtype=np.int64).T
    bt = np.asarray([t for _, _, t in bonds], dtype=np.int64)
    return {'element': np.asarray(ele, dtype=np.int64), 'bond_index': np.concatenate([idx, idx[::-1]], axis=1), 'bond_type': np.concatenate([bt, bt])}


def batch(n, atoms, device, gen=drug_like, pos_sigma=None, mols=None, elements=ELEMENTS):
    """The batch every script times: `n` molecules of about `atoms` atoms from ``gen`` under seed 0 (or the list `mols`), with Gaussian
    coordinates of width `pos_sigma` if given, packed and moved to `device`.  Returns (mols, packed, CompactMols, the generator)."""
    from moldiff_amd import molpack
    g = np.random.default_rng(0)
    if mols is None:
        mols = [gen(g, max(12, int(g.normal(atoms, 5)))) for _ in range(n)]
    if pos_sigma is not None:
        for m in mols:
            m['atom_pos'] = g.normal(0.0, pos_sigma, size=(len(m['element']), 3)).astype(np.float32)
    p = molpack.pack_mols(mols, elements, positions='atom_pos' in mols[0])
    return mols, p, molpack.CompactMols.from_packed(molpack.to_device(p, device)), g


def timed(fn, reps, warmup=5):
    """(ms per call, the last result) of `reps` calls between two device events, after `warmup` untimed calls"""
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps, out


def parser(reps=None, atoms=None, out=''):
    """the options the scripts share: --reps and --atoms where the script has them, --device and --out"""
    ap = argparse.ArgumentParser()
    if atoms is not None:
        ap.add_argument('--atoms', type=int, default=atoms)
    if reps is not None:
        ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--out', type=str, default=out, help='file the printed lines are also written to' + ('' if out else ' (default: none)'))
    return ap


def parse(ap, argv=None):
    """parse, and make the chosen device the current one"""
    args = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(args.device))
    return args


def profile_path(name):
    return os.path.join(ROOT, 'profiles', name)


def report(lines, out, header=None):
    """the tail: print the lines (a dict becomes one JSON line); if `out` names a file, write the header and the lines there"""
    text = '\n'.join(x if isinstance(x, str) else json.dumps(x) for x in lines) + '\n'
    print(text, end='')
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write((header + '\n' if header else '') + text)


def use_lib_from_env():
    """MDX_LIB, if set, names an alternative build of the library (tools/build_variant.sh); call this before anything loads the library"""
    import moldiff_amd._lib as _lib
    if os.environ.get('MDX_LIB'):
        _lib.LIB_PATH = os.path.abspath(os.environ['MDX_LIB'])
    return _lib.LIB_PATH
