"""Cases for the tests of the best RMSD (test_rmsd_host.py, test_gpu_rmsd.py): probes with their targets on top of ``canon_cases`` and
``stereo_cases`` -- degenerate geometry, zero-distance pairs, mirror pairs, symmetric molecules, sizes that cross waves and the cap, one
probe with nine targets -- a brute force over all atom permutations with a Kabsch of its own, and the random batch of the GPU test."""
import itertools

import numpy as np

from .canon_cases import mol, permuted, ring
from .stereo_cases import T, butane23, centre_h, dimethylcyclohexane, gem_dimethyl, moved, random_3d, reflected, rotation, with_pos


def noisy(m, seed, sigma=0.05):
    g = np.random.default_rng(seed)
    return dict(m, atom_pos=(np.asarray(m['atom_pos'], dtype=np.float64) + g.normal(size=np.shape(m['atom_pos'])) * sigma).astype(np.float32))


def relabelled(m, new):
    """the molecule with atom a renamed new[a] (bonds in their order)"""
    new = np.asarray(new, dtype=np.int64)
    out = dict(m, element=np.zeros_like(m['element']), bond_index=new[m['bond_index']], atom_pos=np.zeros_like(m['atom_pos']))
    out['element'][new], out['atom_pos'][new] = m['element'], m['atom_pos']
    return out


def neopentane():
    return with_pos(mol(5, [(0, 1), (0, 2), (0, 3), (0, 4)]), np.vstack([[0, 0, 0], 1.5 * T]))


def chair():
    pos = [[1.45 * np.cos(k * np.pi / 3), 1.45 * np.sin(k * np.pi / 3), 0.25 * (-1) ** k] for k in range(6)]
    return noisy(with_pos(mol(6, ring(6)), pos), 5, 0.1)      # no two atoms alike in space: the 12 maps give different values


def branched(n, seed):
    """a tree of n atoms with random elements (so that few atoms are equivalent) along a random walk in space"""
    g = np.random.default_rng(seed)
    bonds = [(k - 1 if g.random() < 0.8 else int(g.integers(max(0, k - 10), k)), k) for k in range(1, n)]
    pos = np.cumsum(g.normal(size=(n, 3)), axis=0) * 0.9
    return with_pos(mol(g.choice([6, 7, 8], n).tolist(), bonds), pos)


def cases():
    """{name: (probe, [targets])}; every target has the probe's constitution"""
    two = with_pos(mol([6, 8], [(0, 1)]), [[0, 0, 0], [1.2, 0, 0]])
    line = with_pos(mol([6, 6, 8], [(0, 1), (1, 2, 2)]), [[-1.3, 0, 0], [0, 0, 0], [1.2, 0, 0]])
    hexagon = with_pos(mol(6, ring(6, t=4)), [[1.39 * np.cos(k * np.pi / 3), 1.39 * np.sin(k * np.pi / 3), 0] for k in range(6)])
    toluene = with_pos(mol(7, ring(6, t=4) + [(0, 6)]), [[1.39 * np.cos(k * np.pi / 3), 1.39 * np.sin(k * np.pi / 3), 0] for k in range(6)] + [[2.9, 0, 0]])
    chf, neo, six = centre_h(), neopentane(), chair()
    shuffled = relabelled(noisy(neo, 3, 0.08), [0, 3, 1, 4, 2])       # the points of the plain noisy copy, the methyls renamed
    big = {n: branched(n, 40 + n) for n in (70, 200, 256, 257)}
    return {
        'two_atoms': (two, [moved(noisy(two, 1), 2)]),
        'collinear': (line, [moved(noisy(line, 3, 0.0), 4), noisy(line, 5)]),
        'planar': (toluene, [moved(toluene, 6), reflected(toluene)]),
        'planar_symmetric': (hexagon, [noisy(hexagon, 8)]),
        'identical': (chf, [dict(chf)]),
        'moved_copy': (dimethylcyclohexane(True), [moved(dimethylcyclohexane(True), 9)]),
        'chfclbr_mirror': (chf, [centre_h(flip=True)]),
        'butane_pp_mm': (butane23(1, 1), [butane23(-1, -1)]),
        'neopentane': (neo, [shuffled, noisy(neo, 3, 0.08)]),
        'six_ring_turned': (six, [noisy(relabelled(six, [(k + 2) % 6 for k in range(6)]), 10, 0.03)]),
        'gem_dimethyl': (gem_dimethyl(), [gem_dimethyl(swap=True)]),
        'chain70': (big[70], [moved(noisy(big[70], 11), 12)]),
        'chain200': (big[200], [moved(noisy(big[200], 13), 14)]),
        'cap256': (big[256], [moved(noisy(big[256], 15), 16)]),
        'over257': (big[257], [noisy(big[257], 17)]),
        'nine_targets': (neo, [moved(noisy(neo, 20 + k, 0.1), 30 + k) for k in range(9)]),
    }


def flat(table):
    """{name: (probe, [targets])} -> (probes, targets, pairs, names): one probe per case, its targets in turn"""
    probes, targets, pairs = [], [], []
    for probe, tgts in table.values():
        for t in tgts:
            pairs.append((len(probes), len(targets)))
            targets.append(t)
        probes.append(probe)
    return probes, targets, pairs, list(table)


def random_batch(count=64):
    """`count` probes ``random_3d(9000 + s)``, each with two targets: a relabelled and rotated copy with Gaussian noise of 0.05 A, and
    the reflected copy"""
    table = {}
    for s in range(count):
        m = random_3d(9000 + s)
        table['random%d' % s] = (m, [moved(noisy(m, 500 + s, 0.05), 700 + s), reflected(m)])
    return table


# ---- brute force over all atom permutations, with its own Kabsch -----------------------------------------------------------------------

def kabsch_3x3(p, q, mirror=False):
    """mean squared deviation of (n, 3) point sets paired row by row after the best proper rotation (of q's mirror image with `mirror`):
    the rotation itself from the SVD of the 3 x 3 covariance, then the residual is measured -- no eigenvalue formula"""
    p, q = p - p.mean(axis=0), q - q.mean(axis=0)
    if mirror:
        q = q * np.asarray([1.0, 1.0, -1.0])
    u, _, vt = np.linalg.svd(p.T @ q)
    d = np.diag([1.0, 1.0, 1.0 if np.linalg.det(u @ vt) >= 0 else -1.0])
    rot = u @ d @ vt                                                  # q_k ~ rot^T p_k
    return float((((p @ rot) - q) ** 2).sum() / len(p))


def brute_force(probe, target):
    """-> (msd, msd_mirror, n_maps) over ALL n! atom maps that keep elements and bonds; n <= 7"""
    n = len(probe['element'])
    assert n <= 7 and len(target['element']) == n

    def matrix(m):
        M = np.zeros((n, n), dtype=np.int64)
        nb = m['bond_index'].shape[1] // 2
        for (i, j), t in zip(m['bond_index'][:, :nb].T, m['bond_type'][:nb]):
            M[i, j] = M[j, i] = t
        return M
    Mp, Mt = matrix(probe), matrix(target)
    p, q = np.asarray(probe['atom_pos'], dtype=np.float64), np.asarray(target['atom_pos'], dtype=np.float64)
    best, best_m, count = np.inf, np.inf, 0
    for perm in itertools.permutations(range(n)):
        f = np.asarray(perm)                                           # probe atom a -> target atom f[a]
        if (probe['element'] != target['element'][f]).any() or (Mp != Mt[np.ix_(f, f)]).any():
            continue
        count += 1
        best, best_m = min(best, kabsch_3x3(p, q[f])), min(best_m, kabsch_3x3(p, q[f], mirror=True))
    return best, best_m, count
