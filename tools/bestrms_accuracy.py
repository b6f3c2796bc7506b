"""How far an honest float64 evaluation of the best RMSD may stand from numpy's SVD: the tolerance of tests/test_gpu_rmsd.py.

A second float64 evaluation of every pair of the tests' fixtures and random batch that restates, operation by operation, what
mdx_mol_bestrms does on the device (csrc/mdx_bestrms.hip, csrc/mdx_bestrms_args.h): lane l of a wave adds its atoms l, l + 64, ... in
turn, a butterfly adds the 64 lanes, Horn's 4 x 4 quaternion matrix is solved by cyclic Jacobi in the kernel's order with its
threshold.  The largest difference from ``rmsd.best_rms_ref``'s numbers, in the unit (Ga + Gb) / n of the pair, goes to
profiles/bestrms_accuracy.txt; the GPU tests allow 16 times that.  No GPU.

    python tools/bestrms_accuracy.py [--out profiles/bestrms_accuracy.txt]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moldiff_amd import rmsd  # noqa: E402
from tests import rmsd_cases  # noqa: E402

SWEEPS, OFF = 16, 1e-36          # BR_SWEEPS, BR_OFF
LANES = np.arange(64)


def wave_sum(rows):
    """rows (n, k): lane l adds its rows l, l + 64, ... in turn; then v += v[lane ^ o] for o = 32 .. 1 -> (k), the same in every lane"""
    lanes = np.zeros((64, rows.shape[1]))
    for a in range(len(rows)):
        lanes[a & 63] += rows[a]
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[LANES ^ o]
    return lanes[0]


def frame(pos):
    c = wave_sum(pos) / float(len(pos))
    d = pos - c
    return d, wave_sum(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None])[0]


def solve(h):
    """bestrms_solve, in Python floats"""
    xx, xy, xz, yx, yy, yz, zx, zy, zz = (float(v) for v in h)
    a = [[(xx + yy) + zz, yz - zy, zx - xz, xy - yx], [0.0, (xx - yy) - zz, xy + yx, zx + xz], [0.0, 0.0, (yy - xx) - zz, yz + zy],
         [0.0, 0.0, 0.0, (zz - xx) - yy]]
    sq = lambda i, j: a[i][j] * a[i][j]
    off_now = lambda: ((sq(0, 1) + sq(0, 2)) + (sq(0, 3) + sq(1, 2))) + (sq(1, 3) + sq(2, 3))
    bound = OFF * (((sq(0, 0) + sq(1, 1)) + (sq(2, 2) + sq(3, 3))) + 2.0 * off_now())
    for _ in range(SWEEPS):
        if not off_now() > bound:
            break
        for p, q, rs in ((0, 1, (2, 3)), (0, 2, (1, 3)), (0, 3, (1, 2)), (1, 2, (0, 3)), (1, 3, (0, 2)), (2, 3, (0, 1))):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t2 = theta * theta
            t = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + math.sqrt(t2 + 1.0)) if math.isfinite(t2) else 0.0
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            tau = s / (1.0 + c)
            a[p][p], a[q][q], a[p][q] = a[p][p] - t * apq, a[q][q] + t * apq, 0.0
            for r in rs:
                gi, hi = (min(p, r), max(p, r)), (min(q, r), max(q, r))
                g0, h0 = a[gi[0]][gi[1]], a[hi[0]][hi[1]]
                a[gi[0]][gi[1]] = g0 - s * (h0 + tau * g0)
                a[hi[0]][hi[1]] = h0 + s * (g0 - tau * h0)
    diag = [a[i][i] for i in range(4)]
    return max(diag), min(diag)


def device_msd(p, q, c):
    """the signature of ``rmsd.kabsch_msd``, the device's arithmetic"""
    n = len(p)
    pc, Ga = frame(p)
    qc, Gb = frame(q)
    x = qc[c]
    rows = np.stack([pc[:, i] * x[:, j] for i in range(3) for j in range(3)], axis=1)
    lmax, lmin = solve(wave_sum(rows))
    G = Ga + Gb
    return max(0.0, G - 2.0 * lmax) / n, max(0.0, G + 2.0 * lmin) / n, G / n


def measure():
    """-> [(name of the set, pairs, the largest difference in the pair's unit, the key and row where it stands)]"""
    rows = []
    for name, table in (('fixtures', rmsd_cases.cases()), ('random batch', rmsd_cases.random_batch())):
        probes, targets, pairs, _ = rmsd_cases.flat(table)
        want = rmsd.stack_ref(probes, targets, pairs)
        got = rmsd.stack_ref(probes, targets, pairs, evaluate=device_msd)
        assert all(np.array_equal(want[k], got[k]) for k in ('n_maps', 'pair_status', 'status', 'n_nodes', 'n_aut'))
        ok = want['pair_status'] == 0
        unit = np.where(want['unit'] > 0, want['unit'], 1.0)
        worst = (0.0, '', -1)
        for k in rmsd.FLOAT_KEYS:
            d = np.where(ok, np.abs(want[k] - got[k]) / unit, 0.0)
            if len(d) and d.max() >= worst[0]:
                worst = (float(d.max()), k, int(d.argmax()))
        rows.append((name, int(ok.sum()), worst))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bestrms_accuracy.txt'))
    args = ap.parse_args(argv)
    rows = measure()
    figure = max(w[0] for _, _, w in rows)
    lines = ['best RMSD: numpy SVD (rmsd.best_rms_ref) against a float64 restatement of the device\'s sums and Jacobi solve, on the CPU',
             'unit: (Ga + Gb) / n of the pair; columns msd, msd_mirror, msd_first; made by tools/bestrms_accuracy.py', '']
    lines += ['%-13s %4d measured pairs   largest difference %.3e  (%s, row %d)' % (name, k, w[0], w[1], w[2]) for name, k, w in rows]
    lines += ['', 'max_abs_difference_in_unit %.3e' % figure, 'test_tolerance_16x %.3e' % (16 * figure), '']
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines))
    print('\n'.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
