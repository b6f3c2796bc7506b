"""Cases for the tests of the stereo perception (test_stereo_host.py, test_gpu_stereo.py): hand-built 3D fixtures with ideal tetrahedral
or planar coordinates on top of ``canon_cases``, a rigid motion with relabelling, a reflection, and seeded random graphs with random
coordinates."""
import numpy as np

from .canon_cases import mol, permuted, random_mol

S3 = 1.0 / np.sqrt(3.0)
# the four directions of a tetrahedron; T[0], T[1], T[2] seen from T[3] run clockwise
T = np.asarray([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) * S3


def with_pos(m, pos):
    return dict(m, atom_pos=np.asarray(pos, dtype=np.float32).reshape(len(m['element']), 3))


def centre_h(elements=(9, 17, 6), flip=False):
    """C with three different neighbours on tetrahedral directions 0 .. 2 and the implicit H on the fourth"""
    pos = np.vstack([[0, 0, 0], 1.5 * T[:3]])
    return with_pos(mol([6] + list(elements), [(0, 1), (0, 2), (0, 3)]), pos * ([1, 1, -1] if flip else [1, 1, 1]))


def centre4(elements=(9, 17, 6, 8), flip=False):
    pos = np.vstack([[0, 0, 0], 1.5 * T])
    return with_pos(mol([6] + list(elements), [(0, 1), (0, 2), (0, 3), (0, 4)]), pos * ([1, 1, -1] if flip else [1, 1, 1]))


def gem_dimethyl(swap=False):
    """C(CH3)2(F)(Cl): a candidate with two equivalent neighbours; `swap` puts the methyls on each other's direction"""
    order = [0, 1, 3, 2] if swap else [0, 1, 2, 3]
    return with_pos(mol([6, 9, 17, 6, 6], [(0, 1), (0, 2), (0, 3), (0, 4)]), np.vstack([[0, 0, 0], 1.5 * T[order]]))


def butene(cis, ends=(6, 6)):
    """X-CH=CH-Y in the plane, the two substituents on the same side (cis) or not"""
    pos = [[-0.65, 0, 0], [0.65, 0, 0], [-1.4, 1.25, 0], [1.4, 1.25 if cis else -1.25, 0]]
    return with_pos(mol([6, 6] + list(ends), [(0, 1, 2), (0, 2), (1, 3)]), pos)


def dimethylcyclohexane(cis):
    """1,4-dimethylcyclohexane, heavy atoms only: a chair, the methyl on C0 up, the one on C3 up (cis: one axial, one equatorial side
    of the mean plane alike) or down"""
    ring = [[1.45 * np.cos(k * np.pi / 3), 1.45 * np.sin(k * np.pi / 3), 0.25 * (-1) ** k] for k in range(6)]
    up = lambda k, s: [ring[k][0] * 1.35, ring[k][1] * 1.35, ring[k][2] + 1.2 * s]
    pos = ring + [up(0, 1), up(3, 1 if cis else -1)]
    return with_pos(mol(8, [(k, (k + 1) % 6) for k in range(6)] + [(0, 6), (3, 7)]), pos)


def butane23(first, second):
    """CH3-CH(F)-CH(F)-CH3, heavy atoms: centres 1 and 2, each with the handedness asked for (+1 / -1 as built here); (+1, +1) and
    (-1, -1) are mirror images, (+1, -1) is meso"""
    def centre(at, axis, hand):
        # three directions around the axis pointing away from the other centre, in the order (other centre, F, CH3)
        a = np.asarray(axis, dtype=np.float64)
        u, v = np.asarray([0, 1.0, 0]), np.cross(a, [0, 1.0, 0])
        f = -a / 3 + np.sqrt(8) / 3 * u
        c = -a / 3 + np.sqrt(8) / 3 * (-0.5 * u + hand * np.sqrt(3) / 2 * v)
        return at + 1.4 * f, at + 1.5 * c
    c1, c2 = np.asarray([-0.77, 0, 0]), np.asarray([0.77, 0, 0])
    f1, m1 = centre(c1, [1.0, 0, 0], first)
    f2, m2 = centre(c2, [-1.0, 0, 0], second)
    return with_pos(mol([6, 6, 6, 6, 9, 9], [(0, 1), (1, 2), (2, 3), (1, 4), (2, 5)]), [m1, c1, c2, m2, f1, f2])


def fixtures():
    flat = with_pos(mol([6, 9, 17, 6, 8], [(0, 1), (0, 2), (0, 3), (0, 4)]), [[0, 0, 0], [1.4, 0, 0], [0, 1.4, 0], [-1.4, 0, 0], [0, -1.4, 0]])
    nan = centre4()
    nan['atom_pos'] = nan['atom_pos'].copy()
    nan['atom_pos'][2, 1] = np.nan
    coincident = butene(True)
    coincident['atom_pos'] = coincident['atom_pos'].copy()
    coincident['atom_pos'][1] = coincident['atom_pos'][0]
    allene = with_pos(mol(5, [(0, 1, 2), (1, 2, 2), (0, 3), (2, 4)]), [[-1.3, 0, 0], [0, 0, 0], [1.3, 0, 0], [-2, 1, 0], [2, 0, 1]])
    return {
        'chfclbr': centre_h(), 'chfclbr_mirror': centre_h(flip=True),
        'centre4': centre4(), 'centre4_mirror': centre4(flip=True),
        'neopentane': with_pos(mol(5, [(0, 1), (0, 2), (0, 3), (0, 4)]), np.vstack([[0, 0, 0], 1.5 * T])),
        'gem_dimethyl': gem_dimethyl(), 'gem_dimethyl_swapped': gem_dimethyl(swap=True),
        'butene_z': butene(True), 'butene_e': butene(False),
        'difluoroethene_z': butene(True, (9, 9)), 'difluoroethene_e': butene(False, (9, 9)),
        'dimethylcyclohexane_cis': dimethylcyclohexane(True), 'dimethylcyclohexane_trans': dimethylcyclohexane(False),
        'butane_pp': butane23(1, 1), 'butane_mm': butane23(-1, -1), 'butane_meso': butane23(1, -1),
        'flat_centre': flat, 'nan': nan, 'coincident': coincident, 'allene': allene,
    }


def rotation(g):
    """a proper rotation drawn from the generator `g` (QR of a normal matrix, the determinant made +1)"""
    q, r = np.linalg.qr(g.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def moved(m, seed):
    """the same molecule rotated, translated and relabelled (``canon_cases.permuted``) -> the molecule"""
    g = np.random.default_rng(seed)
    pos = np.asarray(m['atom_pos'], dtype=np.float64) @ rotation(g).T + g.normal(size=3) * 3
    return permuted(dict(m, atom_pos=pos.astype(np.float32)), seed + 1)[0]


def reflected(m):
    return dict(m, atom_pos=(np.asarray(m['atom_pos']) * np.asarray([1, 1, -1], dtype=np.float32)).astype(np.float32))


def random_3d(seed, n_min=3, n_max=12):
    """a ``random_mol`` graph (elements C / N, types 1 / 2 / 4) with normal coordinates"""
    m = random_mol(seed, n_min, n_max)
    return with_pos(m, np.random.default_rng(seed + 77).normal(size=(len(m['element']), 3)) * 1.5)
