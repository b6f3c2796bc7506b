"""Force-field relaxation of all-atom molecules: every molecule with its placed hydrogens (``hydrogens.addh_mols``) is relaxed in a
UFF-form force field by L-BFGS, and the energy it loses (the strain) and the distance its heavy atoms move are reported.

The device half is ``mdx_mol_relax`` (csrc/mdx_relax.hip), reached through ``relax_mols`` (a list of molecule dicts; runs ``kekule`` and
``hydrogens`` first), ``launch`` (a ``CompactMols`` with positions and the device arrays of ``hydrogens.launch``) and
``FeaturizeMol.relax_batch`` (the sampler's predictions).  ``energy_ref`` and ``relax_ref`` are the plain restatement for one molecule
in float64 (the terms in Python floats, the minimiser ``lbfgs_ref``, which ``embed.embed_ref`` shares, in element-wise numpy rows), in
the device's own order of operations and reduction tree, and need no GPU.

What it is: THIS PROJECT'S OWN MODEL, stated exactly in include/moldiff_hip.h: UFF's functional forms (harmonic bonds, cosine angle
terms, cosine torsions, inversions, 12-6 van der Waals without cutoff, no electrostatics) over a small parameter table
(configs/forcefield_default.yml) that is a TRANSCRIPTION FROM MEMORY of Rappe et al. 1992 and UNVERIFIED.  It is NOT RDKit's
``UFFOptimizeMolecule`` and it is UNVERIFIED AGAINST RDKit: the atom typing is (element, variant) from the geometry flag of
``mdx_mol_hydrogens`` (an atom with an aromatic bond is RESONANT), hypervalent P and S use their tetrahedral row, a missing
(element, variant) row falls back to the element's tetrahedral row, and the torsion and inversion rules are simplified.  ``gtol``
(1e-2 kcal/mol/Angstrom) is a convention; ``max_iters`` 200 is RDKit's default.  With no trained checkpoint offline it is an
instrument, not a measurement of sample quality.

    python -m moldiff_amd.relax stats samples_all.pt --out relax.npz [--sdf relaxed.sdf] [--ref] [--iters 200] [--gtol 0.01] [--part finished]
    python -m moldiff_amd.relax compare a.npz b.npz
"""
import math
import os
import sys

import numpy as np

from . import hydrogens, kekule, molpack
from .hydrogens import MAX_H, _cross, _dot, _positions, _sub
from .molpack import DEFAULT_ATOMIC_NUMBERS, jsd_counts, mol_graph, to_host

MAX_ATOMS, MAX_BONDS = hydrogens.MAX_ATOMS, hydrogens.MAX_BONDS
MAX_ELEMENTS, MAX_BOND_TYPES, MAX_TYPES, HISTORY, MAX_ITERS_LIMIT = 32, 16, 32, 8, 100000
WS_DOUBLES = 2 * HISTORY * 768                                     # the device's history per molecule
DEFAULT_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'forcefield_default.yml')
DEFAULT_MAX_ITERS = 200                                            # RDKit's default
DEFAULT_GTOL = 1e-2                                                # kcal/mol/Angstrom, rms: a convention
DEFAULT_MAX_STEP = 0.3                                             # Angstrom
DEFAULT_DEG_TOL = 1e-3
ARMIJO, CURVATURE = 1e-4, 1e-10
MAX_TRIALS = 20
STATUS_OK, STATUS_TOO_LARGE, STATUS_NONFINITE = 0, 1, 2
STOP_CONVERGED, STOP_MAXITER, STOP_LINESEARCH = 0, 1, 2
TETRAHEDRAL, TRIGONAL, LINEAR, RESONANT, HYDROGEN = 0, 1, 2, 3, 4
VARIANT_NAMES = {'tetrahedral': TETRAHEDRAL, 'trigonal': TRIGONAL, 'linear': LINEAR, 'resonant': RESONANT}
# the columns of the device's two per-molecule tables, in their order (include/moldiff_hip.h: MDX_RELAX_STATS, MDX_RELAX_ENERGIES)
STAT_KEYS = ('status', 'stop_reason', 'iterations', 'n_evals', 'n_all', 'n_ff_bonds', 'n_angles', 'n_torsions', 'n_inversions', 'n_pairs',
             'n_fallback')
COMPONENTS = ('bond', 'angle', 'torsion', 'inversion', 'vdw')
ENERGY_KEYS = tuple('e_%s0' % c for c in COMPONENTS) + ('e_total0',) + tuple('e_' + c for c in COMPONENTS) + ('e_total', 'rms_grad', 'rmsd_heavy')
MOL_KEYS = STAT_KEYS + ('n_atoms',)
LAYOUT = molpack.Layout(MOL_KEYS)                                  # the int32 part of the results table
ATOM_FLOAT_KEYS = {'pos': (3,), 'h_pos': (MAX_H, 3), 'grad': (3,), 'h_grad': (MAX_H, 3)}   # float64 per atom slot
FLOAT_KEYS = ('energy',) + tuple(ATOM_FLOAT_KEYS)
STRAIN_BINS, STRAIN_MAX = 40, 200.0                                # kcal/mol: 5 per bin, the last also more
RMSD_BINS, RMSD_MAX = 40, 2.0                                      # Angstrom: 0.05 per bin, the last also more
# a packed row of the table, as csrc/mdx_relax_args.h packs it
P_R, P_C0, P_X, P_SQRT_D, P_Z, P_CHI, P_SQRT_CHI, P_V, P_U, P_KINV = range(10)
ROW_FIELDS = 11                                                    # class, variant, r, theta0, x, D, Z, chi, V, U, K_inv


class ForceFieldTables:
    """The parameter rows of one call: from a YAML file or dict in the form of configs/forcefield_default.yml (None = that file),
    validated as the device entry validates them.  ``rows``: float64 (n, 11) of class (-1 hydrogen), variant, r, theta0 (degrees), x,
    D, Z, chi, V, U, K_inv -- what ``mdx_mol_relax`` takes; ``par``: the derived rows (cos theta0, the square roots) the energy uses."""

    def __init__(self, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4, table=None):
        self.atomic_numbers, self.num_bond_types = tuple(int(z) for z in atomic_numbers), int(num_bond_types)
        if not 1 <= len(self.atomic_numbers) <= MAX_ELEMENTS or not 1 <= self.num_bond_types <= MAX_BOND_TYPES:
            raise ValueError(f'1 .. {MAX_ELEMENTS} elements and 1 .. {MAX_BOND_TYPES} bond types')
        if table is None or isinstance(table, str):
            import yaml
            with open(DEFAULT_TABLE if table is None else table) as f:
                table = yaml.safe_load(f) or {}
        elements = {int(z): dict(v) for z, v in dict(table.get('elements') or {}).items()}
        if 1 not in elements:
            raise ValueError('no hydrogen row')
        missing = [z for z in self.atomic_numbers if z not in elements]
        if missing:
            raise ValueError(f'no force-field row for element(s) {missing}')
        cls = {z: c for c, z in enumerate(self.atomic_numbers)}
        rows = []
        for z in [1] + list(self.atomic_numbers):
            e = elements[z]
            variants = dict(e.get('variants') or {})
            unknown = sorted(set(variants) - set(VARIANT_NAMES))
            if unknown:
                raise ValueError(f'element {z}: unknown variant(s) {unknown}')
            if 'tetrahedral' not in variants or (z == 1 and len(variants) != 1):
                raise ValueError(f'element {z}: every element needs its tetrahedral row, hydrogen only that')
            for name, v in variants.items():
                rows.append([-1 if z == 1 else cls[z], VARIANT_NAMES[name], float(v['r']), float(v['theta0']), float(e['x']), float(e['D']),
                             float(e['Z']), float(e['chi']), float(e.get('V', 0.0)), float(e.get('U', 0.0)), float(e.get('K_inv', 0.0))])
        self.rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, ROW_FIELDS))
        if len(self.rows) > MAX_TYPES:
            raise ValueError(f'the force field holds 1 .. {MAX_TYPES} rows')
        limits = ((2, 'r', 0.0, 4.0, False), (3, 'theta0', 0.0, 180.0, False), (4, 'x', 0.0, 10.0, False), (5, 'D', 0.0, 10.0, True),
                  (6, 'Z', 0.0, 100.0, False), (7, 'chi', 0.0, 100.0, False), (8, 'V', 0.0, 1e3, True), (9, 'U', 0.0, 1e3, True), (10, 'K_inv', 0.0, 1e3, True))
        for col, name, lo, hi, closed in limits:
            for v in self.rows[:, col]:
                if not ((lo <= v if closed else lo < v) and v <= hi):   # NaN fails
                    raise ValueError(f'{name} must lie in {"[" if closed else "("}{lo:g}, {hi:g}], got {v}')
        # the derived rows, with the host functions the C side uses
        self.par, self.type_of, self.h_type = [], {}, None
        for q, row in enumerate(self.rows.tolist()):
            c, v, r, th, x, D, Z, chi, V, U, kinv = row
            self.par.append((r, -1.0 if th == 180.0 else math.cos(th * (math.pi / 180.0)), x, math.sqrt(D), Z, chi, math.sqrt(chi), V, U, kinv))
            if c < 0:
                self.h_type = q
            else:
                self.type_of[int(c), int(v)] = (q, False)
        for c in range(len(self.atomic_numbers)):
            for v in range(4):
                self.type_of.setdefault((c, v), (self.type_of[c, 0][0], True))
        self.ln_order = (0.0, math.log(1.5), math.log(2.0), math.log(3.0))

    def key(self):
        return (self.atomic_numbers, self.num_bond_types, self.rows.tobytes())

    def pair(self, ta, tb, o):
        """rest length and force constant of a bond of order index `o` between rows `ta` and `tb` (csrc/mdx_relax_args.h: relax_pair)"""
        a, b = self.par[ta], self.par[tb]
        total = a[P_R] + b[P_R]
        ds = a[P_SQRT_CHI] - b[P_SQRT_CHI]
        en = ((a[P_R] * b[P_R]) * (ds * ds)) / (a[P_CHI] * a[P_R] + b[P_CHI] * b[P_R])
        r = (total - (0.1332 * total) * self.ln_order[o]) - en
        return r, ((664.12 * a[P_Z]) * b[P_Z]) / ((r * r) * r)


def _tables(tables):
    return ForceFieldTables() if tables is None else tables


def _check(max_iters, gtol, max_step=DEFAULT_MAX_STEP, deg_tol=DEFAULT_DEG_TOL):
    if not 0 <= int(max_iters) <= MAX_ITERS_LIMIT:
        raise ValueError(f'max_iters must lie in 0 .. {MAX_ITERS_LIMIT}, got {max_iters}')
    if not 0.0 < float(gtol) <= 1e6:                               # NaN fails
        raise ValueError(f'gtol must lie in (0, 1e6], got {gtol}')
    if not 0.0 < float(max_step) <= 10.0:
        raise ValueError(f'max_step must lie in (0, 10] Angstrom, got {max_step}')
    if not 0.0 < float(deg_tol) < 1.0:
        raise ValueError(f'deg_tol must lie in (0, 1), got {deg_tol}')
    return int(max_iters), float(gtol), float(max_step), float(deg_tol)


# ---- the terms: one function each, the same operations in the same order as csrc/mdx_relax.hip ----------------------------------------

def _bond_term(pa, pb, r0, k):
    d = _sub(pa, pb)
    r = math.sqrt(_dot(d, d))
    dr = r - r0
    f = _div(k * dr, r)
    return (0.5 * k) * (dr * dr), (f * d[0], f * d[1], f * d[2])


def _div(a, b):
    """IEEE division: x / 0 is an infinity or NaN, as on the device"""
    try:
        return a / b
    except ZeroDivisionError:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else math.nan


def _angle_k(zi, zk, rij, rjk, c0):
    rik2 = (rij * rij + rjk * rjk) - ((2.0 * rij) * rjk) * c0
    rik = math.sqrt(rik2)
    return (((664.12 * zi) * zk) / ((rik2 * rik2) * rik)) * (((3.0 * rij) * rjk) * (1.0 - c0 * c0) - rik2 * c0)


ANGLE_LINEAR, ANGLE_TRIGONAL, ANGLE_GENERAL = 0, 1, 2


def _angle_term(pi, pj, pk, K, kind, c0):
    u, v = _sub(pi, pj), _sub(pk, pj)
    uu, vv = _dot(u, u), _dot(v, v)
    luv = math.sqrt(uu) * math.sqrt(vv)
    c = _div(_dot(u, v), luv)
    if kind == ANGLE_LINEAR:
        e, de = K * (1.0 + c), K
    elif kind == ANGLE_TRIGONAL:
        k9, c2 = K / 9.0, c * c
        e, de = k9 * (1.0 - ((4.0 * c2) * c - 3.0 * c)), -(k9 * (12.0 * c2 - 3.0))
    else:
        c2 = 1.0 / (4.0 * (1.0 - c0 * c0))
        c1 = (-4.0 * c2) * c0
        e, de = K * ((c2 * ((2.0 * c0) * c0 + 1.0) + c1 * c) + c2 * ((2.0 * c) * c - 1.0)), K * (c1 + (4.0 * c2) * c)
    fu, fv = _div(c, uu), _div(c, vv)
    gi = tuple(de * (_div(v[x], luv) - fu * u[x]) for x in range(3))
    gk = tuple(de * (_div(u[x], luv) - fv * v[x]) for x in range(3))
    return e, gi, gk


TORSION_TT, TORSION_PP, TORSION_MIXED = 0, 1, 2


def _torsion_term(p0, p1, p2, p3, kind, vq, deg_tol, trace):
    """-> None for a collinear triple, or (energy, gradient on p0, gradient on p1)"""
    F, G, H = _sub(p0, p1), _sub(p1, p2), _sub(p3, p2)
    A, B = _cross(F, G), _cross(H, G)
    aa, bb = _dot(A, A), _dot(B, B)
    la, lb = _sqrt(aa), _sqrt(bb)
    trace.append(('deg', la)), trace.append(('deg', lb))
    if not la >= deg_tol or not lb >= deg_tol:
        return None
    lab = la * lb
    c = _dot(A, B) / lab
    c2, hv = c * c, 0.5 * vq
    if kind == TORSION_TT:
        e, de = hv * (1.0 + ((4.0 * c2) * c - 3.0 * c)), hv * (12.0 * c2 - 3.0)
    elif kind == TORSION_PP:
        e, de = hv * (1.0 - (2.0 * c2 - 1.0)), hv * (-4.0 * c)
    else:
        c4 = c2 * c2
        e, de = hv * (1.0 - ((((32.0 * c4) * c2 - 48.0 * c4) + 18.0 * c2) - 1.0)), -(hv * (((192.0 * c4) * c - (192.0 * c2) * c) + 36.0 * c))
    fa, fb = c / aa, c / bb
    tA = tuple(B[x] / lab - fa * A[x] for x in range(3))
    tB = tuple(A[x] / lab - fb * B[x] for x in range(3))
    GA, AF, BH = _cross(G, tA), _cross(tA, F), _cross(tB, H)
    return e, tuple(de * GA[x] for x in range(3)), tuple(de * ((AF[x] - GA[x]) + BH[x]) for x in range(3))


def _inversion_term(pj, pi, pk, pl, k3, deg_tol, trace):
    """-> None for a collinear plane or an apex on the centre, or (energy, gradients on i, k and the apex l)"""
    u, v, w = _sub(pi, pj), _sub(pk, pj), _sub(pl, pj)
    n = _cross(u, v)
    nn, ww = _dot(n, n), _dot(w, w)
    ln, lw = _sqrt(nn), _sqrt(ww)
    trace.append(('deg', ln))
    if not ln >= deg_tol or not lw > 0.0:
        return None
    lnw = ln * lw
    y = _dot(n, w) / lnw
    sq = _sqrt(1.0 - y * y)
    e, de = k3 * (1.0 - sq), _div(k3 * y, sq)
    fn, fw = y / nn, y / ww
    tn = tuple(w[x] / lnw - fn * n[x] for x in range(3))
    tw = tuple(n[x] / lnw - fw * w[x] for x in range(3))
    vi, vk = _cross(v, tn), _cross(tn, u)
    return e, tuple(de * vi[x] for x in range(3)), tuple(de * vk[x] for x in range(3)), tuple(de * tw[x] for x in range(3))


def _vdw_term(pa, pb, x2, dij):
    d = _sub(pa, pb)
    r2 = _dot(d, d)
    q2 = _div(x2, r2)
    q6 = (q2 * q2) * q2
    q12 = q6 * q6
    f = _div((12.0 * dij) * (q6 - q12), r2)
    return dij * (q12 - 2.0 * q6), (f * d[0], f * d[1], f * d[2])


# ---- the device's sums ---------------------------------------------------------------------------------------------------------------

def _fmax(a, b):
    """fmax: a NaN operand is dropped, as on the device"""
    return b if a != a else a if b != b else max(a, b)


def block_max(vals):
    """the largest of one value per thread (missing threads hold 0.0) as the device takes it, with fmax"""
    out = 0.0
    for v in vals:
        out = _fmax(out, v)
    return out


def _wave_sum(v):
    """what every lane of a 64-wide xor butterfly (32, 16, .. 1) ends with"""
    for o in (32, 16, 8, 4, 2, 1):
        v = [v[i] + v[i + o] for i in range(o)]
    return v[0]


def block_sum(vals):
    """the sum of one value per thread (missing threads hold 0.0) as the device takes it: a butterfly in each of the four waves, then
    ((w0 + w1) + w2) + w3"""
    vals = list(vals) + [0.0] * (256 - len(vals))
    w = [_wave_sum(vals[64 * k:64 * k + 64]) if any(vals[64 * k:64 * k + 64]) else 0.0 for k in range(4)]   # a wave of zeros sums to zero
    return ((w[0] + w[1]) + w[2]) + w[3]


def _rowdot(a, b):
    """one value per thread of two (atoms, D) arrays: (x x' + y y') + z z', then + w w' -> list"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not len(a):
        return []
    p = a[:, 0] * b[:, 0]
    for c in range(1, a.shape[1]):
        p = p + a[:, c] * b[:, c]
    return p.tolist()


def _vdot(a, b):
    """the dot product of two (atoms, D) arrays: ``_rowdot`` per thread, then block_sum"""
    return block_sum(_rowdot(a, b))


# ---- the minimiser of relax_ref and embed.embed_ref: csrc/mdx_lbfgs.h -----------------------------------------------------------------

@np.errstate(all='ignore')
def lbfgs_ref(x, evaluate, max_iters, gtol, max_step, trace):
    """The L-BFGS of csrc/mdx_lbfgs.h from the point x, (atoms, D) float64, in element-wise float64 operations over the atoms (the
    device's thread per atom) and the device's block sums.  evaluate(x) -> (energy, gradient (atoms, D), whatever else the caller wants
    of that point).  trace receives every number a decision compares with a threshold as (kind, value, threshold): 'rms', 'descent',
    'cap', 'armijo' (value = trial energy, threshold = the bound), 'curvature'.  -> None when the energy or gradient at x is not finite,
    else dict: ``x``, ``energy``, ``grad``, ``extra`` at the last accepted point, ``first`` (the extra at x), ``rms``, ``iterations``,
    ``n_evals``, ``stop_reason`` and ``energies``, the accepted energy after every iteration."""
    x = np.asarray(x, dtype=np.float64)
    na, D = x.shape
    E, g, extra = evaluate(x)
    first, n_evals = extra, 1
    if not math.isfinite(E) or not math.isfinite(_vdot(g, g)):
        return None
    hist, iters, energies = [], 0, []                                  # hist: (s, y, s.y, y.y), oldest first
    while True:
        gg = _vdot(g, g)
        rms = math.sqrt(gg / (float(D) * na)) if na else 0.0
        trace.append(('rms', rms, gtol))
        if rms <= gtol:
            reason = STOP_CONVERGED
            break
        if iters >= max_iters:
            reason = STOP_MAXITER
            break
        if hist:
            q, alphas = g, []
            for s, y, sy, _ in reversed(hist):
                al = _vdot(s, q) / sy
                alphas.append(al)
                q = q - al * y
            gamma = hist[-1][2] / hist[-1][3]
            r = gamma * q
            for (s, y, sy, _), al in zip(hist, reversed(alphas)):
                co = al - _vdot(y, r) / sy
                r = r + co * s
            d = -r
            gd = _vdot(g, d)
            trace.append(('descent', gd, 0.0))
            if not gd < 0.0:
                hist = []
        if not hist:
            d = -g
        accepted = None
        while True:
            big = _sqrt(block_max(_rowdot(d, d)))
            trace.append(('cap', big, max_step))
            if big > max_step:
                d = (max_step / big) * d
            gd = _vdot(g, d)
            t = 1.0
            for _ in range(MAX_TRIALS):
                xt = x + t * d
                new = evaluate(xt)
                n_evals += 1
                bound = E + (ARMIJO * t) * gd
                if math.isfinite(new[0]):
                    trace.append(('armijo', new[0], bound))
                if math.isfinite(new[0]) and new[0] <= bound:
                    accepted = new
                    break
                t = t * 0.5
            if accepted is not None or not hist:
                break
            hist = []
            d = -g
        if accepted is None:
            reason = STOP_LINESEARCH
            break
        s, y = xt - x, accepted[1] - g
        sy, ss, yy = _vdot(s, y), _vdot(s, s), _vdot(y, y)
        lim = CURVATURE * _sqrt(ss * yy)
        trace.append(('curvature', sy, lim))
        if sy > lim:
            hist = (hist + [(s, y, sy, yy)])[-HISTORY:]
        x, (E, g, extra) = xt, accepted
        iters += 1
        energies.append(E)
    return dict(x=x, energy=E, grad=g, extra=extra, first=first, rms=rms, iterations=iters, n_evals=n_evals, stop_reason=reason, energies=energies)


def near(trace, band=1e-9):
    """whether some decision of a trace lies within `band` (relative to the larger of the two magnitudes, or absolute against a
    threshold of 0) of its threshold: what a device comparison may leave out, because float64 rounding may differ"""
    return any(math.isfinite(v) and abs(v - th) <= band * max(abs(v), abs(th), 1e-300 if th else 1.0) for _, v, th in trace)


def _split(n, h, vecs):
    """(n_all, 3) of the all-atom molecule -> (n, 3) heavy and (n, 4, 3) hydrogen arrays"""
    heavy = np.asarray(vecs[:n], dtype=np.float64).reshape(n, 3)
    hs = np.zeros((n, MAX_H, 3), dtype=np.float64)
    at = n
    for a in range(n):
        for k in range(h[a]):
            hs[a, k] = vecs[at]
            at += 1
    return heavy, hs


# ---- the all-atom molecule -------------------------------------------------------------------------------------------------------------

class _Mol:
    """the staged all-atom molecule of one evaluation: what csrc/mdx_relax.hip keeps in LDS"""


def _stage(info, order, h_count, h_pos, atom_flag, tb):
    """-> a _Mol, or None when it is too large"""
    nbt = tb.num_bond_types
    cls, bi, bt = mol_graph(info, tb.atomic_numbers)
    n, nb = len(cls), bi.shape[1]
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    h_count = np.asarray(h_count, dtype=np.int64).reshape(-1)
    atom_flag = np.asarray(atom_flag, dtype=np.int64).reshape(-1)
    h_pos = np.asarray(h_pos, dtype=np.float64).reshape(-1, MAX_H, 3)
    if len(order) != nb or len(h_count) != n or len(atom_flag) != n or len(h_pos) != n:
        raise ValueError('order holds one value per bond; h_count, atom_flag and h_pos one entry per atom')
    m = _Mol()
    m.n, m.h = n, [min(max(int(x), 0), MAX_H) for x in h_count]
    m.n_all = n + sum(m.h)
    if n > MAX_ATOMS or nb > MAX_BONDS or m.n_all > MAX_ATOMS:
        return None
    m.pos = _positions(info, n) + [tuple(float(x) for x in h_pos[a, k]) for a in range(n) for k in range(m.h[a])]
    m.parent = [a for a in range(n) for _ in range(m.h[a])]
    rows = [[] for _ in range(m.n_all)]                                # (neighbour, bond)
    m.bond_order = []
    arom = [False] * n
    for e in range(nb):
        i, j = int(bi[0, e]), int(bi[1, e])
        m.bond_order.append(None)
        if not (0 <= i < n and 0 <= j < n and i != j):
            continue
        ar = int(bt[e]) == nbt
        m.bond_order[e] = 1 if ar else (0, 2, 3)[min(max(int(order[e]), 1), 3) - 1]
        arom[i], arom[j] = arom[i] or ar, arom[j] or ar
        rows[i].append((j, e)), rows[j].append((i, e))
    for x, a in enumerate(m.parent):
        rows[a].append((n + x, nb + x)), rows[n + x].append((a, nb + x))
        m.bond_order.append(0)
    m.rows = [sorted(r) for r in rows]
    m.var, m.typ, m.n_fallback = [], [], 0
    for a in range(n):
        v = int(atom_flag[a]) & 3
        v = RESONANT if arom[a] else TETRAHEDRAL if v == 3 else v
        t, fell = tb.type_of[int(cls[a]), v]
        m.var.append(v), m.typ.append(t)
        m.n_fallback += fell
    m.var += [HYDROGEN] * len(m.parent)
    m.typ += [tb.h_type] * len(m.parent)
    m.par = [tb.par[t] for t in m.typ]
    m.bond_par = [None] * len(m.bond_order)
    for a in range(m.n_all):
        for b, e in m.rows[a]:
            if a < b:
                m.bond_par[e] = tb.pair(m.typ[a], m.typ[b], m.bond_order[e])
    m.excl = []
    for a in range(m.n_all):
        s = {a}
        for b, _ in m.rows[a]:
            s.add(b)
            s.update(c for c, _ in m.rows[b])
        m.excl.append(s)
    m.ln_order = tb.ln_order
    return m


def _angle_kind(m, j):
    return ANGLE_LINEAR if m.var[j] == LINEAR or m.par[j][P_C0] == -1.0 else ANGLE_TRIGONAL if m.var[j] in (TRIGONAL, RESONANT) else ANGLE_GENERAL


def _angle(m, pos, i, j, k, ei, ek):
    pj = m.par[j]
    K = _angle_k(m.par[i][P_Z], m.par[k][P_Z], m.bond_par[ei][0], m.bond_par[ek][0], pj[P_C0])
    return _angle_term(pos[i], pos[j], pos[k], K, _angle_kind(m, j), pj[P_C0])


def _torsion_bond(m, j, k, e):
    """-> None when the bond j-k carries no torsion, or (kind, V per quadruple)"""
    dj, dk = len(m.rows[j]), len(m.rows[k])
    if dj < 2 or dk < 2 or m.var[j] == LINEAR or m.var[k] == LINEAR:
        return None
    nq = float((dj - 1) * (dk - 1))
    pj, pk = m.var[j] in (TRIGONAL, RESONANT), m.var[k] in (TRIGONAL, RESONANT)
    if not pj and not pk:
        return TORSION_TT, math.sqrt(m.par[j][P_V] * m.par[k][P_V]) / nq
    if pj and pk:
        return TORSION_PP, ((5.0 * math.sqrt(m.par[j][P_U] * m.par[k][P_U])) * (1.0 + 4.18 * m.ln_order[m.bond_order[e]])) / nq
    return TORSION_MIXED, 1.0 / nq


def _inverts(m, j):
    return m.var[j] in (TRIGONAL, RESONANT) and len(m.rows[j]) == 3 and m.par[j][P_KINV] > 0.0


def _evaluate(m, pos, deg_tol, trace):
    """-> dict: per-thread energy partials reduced as on the device (``components``, ``total``), ``grad`` per atom, the term counts,
    and the sums of absolute values (``abs_components``, ``abs_grad`` per atom) the tolerances of the tests rest on"""
    na = m.n_all
    part = [[0.0] * na for _ in range(5)]
    apart = [[0.0] * na for _ in range(5)]
    grad, agrad = [], []
    counts = [0, 0, 0, 0, 0]
    tors, invs = {}, {}

    def torsion(p0, p1, p2, p3, kv):
        key = (p0, p1, p2, p3)
        if key not in tors:
            tors[key] = _torsion_term(pos[p0], pos[p1], pos[p2], pos[p3], kv[0], kv[1], deg_tol, trace)
        return tors[key]

    def inversion(j, t):
        if (j, t) not in invs:
            r = [b for b, _ in m.rows[j]]
            i, k = [x for q, x in enumerate(r) if q != t]
            invs[j, t] = (i, k, r[t]), _inversion_term(pos[j], pos[i], pos[k], pos[r[t]], m.par[j][P_KINV] / 3.0, deg_tol, trace)
        return invs[j, t]

    for a in range(na):
        g, ag = [0.0, 0.0, 0.0], 0.0
        row = m.rows[a]

        def add(c, sign=1.0):
            nonlocal ag
            for x in range(3):
                g[x] = g[x] + c[x] if sign > 0 else g[x] - c[x]
            ag += abs(c[0]) + abs(c[1]) + abs(c[2])

        def own(which, e):
            part[which][a] = part[which][a] + e
            apart[which][a] += abs(e)
            counts[which] += 1
        for b, e in row:                                               # bonds
            r0, k = m.bond_par[e]
            en, ga = _bond_term(pos[a], pos[b], r0, k)
            add(ga)
            if a < b:
                own(0, en)
        for q1 in range(len(row)):                                     # angles centred here
            for q2 in range(q1 + 1, len(row)):
                (i, ei), (k, ek) = row[q1], row[q2]
                en, gi, gk = _angle(m, pos, i, a, k, ei, ek)
                add((gi[0] + gk[0], gi[1] + gk[1], gi[2] + gk[2]), -1.0)
                own(1, en)
        for j, ej in row:                                              # angles that end here
            for k, ek in m.rows[j]:
                if k != a:
                    add(_angle(m, pos, a, j, k, ej, ek)[1])
        for k, e in row:                                               # torsions about a bond of this atom
            kv = _torsion_bond(m, a, k, e)
            if kv is None:
                continue
            for i, _ in row:
                if i == k:
                    continue
                for l, _ in m.rows[k]:
                    if l == a or l == i:
                        continue
                    t = torsion(i, a, k, l, kv)
                    if t is not None:
                        add(t[2])
                        if a < k:
                            own(2, t[0])
        for j, _ in row:                                               # torsions that end here
            for k, e in m.rows[j]:
                if k == a:
                    continue
                kv = _torsion_bond(m, j, k, e)
                if kv is None:
                    continue
                for l, _ in m.rows[k]:
                    if l == j or l == a:
                        continue
                    t = torsion(a, j, k, l, kv)
                    if t is not None:
                        add(t[1])
        if _inverts(m, a):                                             # inversions centred here
            for t in range(3):
                _, r = inversion(a, t)
                if r is not None:
                    add(((r[1][0] + r[2][0]) + r[3][0], (r[1][1] + r[2][1]) + r[3][1], (r[1][2] + r[2][2]) + r[3][2]), -1.0)
                    own(3, r[0])
        for j, _ in row:                                               # inversions of a neighbour
            if _inverts(m, j):
                for t in range(3):
                    who, r = inversion(j, t)
                    if r is not None:
                        add(r[1 + who.index(a)])
        pa, ex = m.par[a], m.excl[a]
        for b in range(na):                                            # van der Waals
            if b in ex:
                continue
            pb = m.par[b]
            en, ga = _vdw_term(pos[a], pos[b], pa[P_X] * pb[P_X], pa[P_SQRT_D] * pb[P_SQRT_D])
            add(ga)
            if a < b:
                own(4, en)
        grad.append(tuple(g)), agrad.append(ag)
    comp = [block_sum(p) for p in part]
    total = (((comp[0] + comp[1]) + comp[2]) + comp[3]) + comp[4]
    return {'components': comp, 'total': total, 'grad': grad, 'counts': counts, 'abs_components': [sum(p) for p in apart], 'abs_grad': agrad}


def energy_ref(info, order, h_count, h_pos, atom_flag, tables=None, deg_tol=DEFAULT_DEG_TOL, positions=None, trace=None):
    """The energy and gradient of the all-atom molecule in plain Python floats, in the device's order of operations and reduction
    tree.  info: a molecule dict with ``atom_pos``; order: the Kekulé order per bond; h_count, h_pos, atom_flag: what
    ``hydrogens.addh_ref`` returned.  positions: (n_all, 3) to evaluate there instead (heavy atoms, then the hydrogens in (atom, k)
    order).  -> None when the molecule is too large, else dict: ``components`` (bond, angle, torsion, inversion, vdw), ``total``,
    ``grad`` (n_all tuples), ``counts`` (the terms of each component), ``n_all``, ``n_fallback``, and the sums of absolute term energies
    (``abs_components``) and of absolute gradient contributions per atom (``abs_grad``)."""
    tb = _tables(tables)
    m = _stage(info, order, h_count, h_pos, atom_flag, tb)
    if m is None:
        return None
    pos = m.pos if positions is None else [tuple(float(x) for x in p) for p in np.asarray(positions, dtype=np.float64).reshape(m.n_all, 3)]
    out = _evaluate(m, pos, float(deg_tol), [] if trace is None else trace)
    out.update(n_all=m.n_all, n_fallback=m.n_fallback)
    return out


def relax_ref(info, order, h_count, h_pos, atom_flag, tables=None, max_iters=DEFAULT_MAX_ITERS, gtol=DEFAULT_GTOL, max_step=DEFAULT_MAX_STEP,
              deg_tol=DEFAULT_DEG_TOL, trace=None):
    """Plain float64 restatement of ``mdx_mol_relax`` for one molecule (the arguments of ``energy_ref``) -> dict: the numbers of
    STAT_KEYS, ``n_atoms``, ``energy`` (14 float64: ENERGY_KEYS), ``pos`` / ``grad`` (n, 3) and ``h_pos`` / ``h_grad`` (n, 4, 3) float64,
    and ``energies``, the accepted total energy after every iteration.  With status 1 (TOO_LARGE) or 2 (NONFINITE) every other output is
    0.  trace: a list that receives every number a decision compares with a threshold, as (kind, value, threshold): 'deg', 'rms',
    'descent', 'cap', 'armijo' (value = trial energy, threshold = the bound), 'curvature'."""
    tb = _tables(tables)
    max_iters, gtol, max_step, deg_tol = _check(max_iters, gtol, max_step, deg_tol)
    trace = [] if trace is None else trace
    n = len(np.asarray(info['element']).reshape(-1))
    zero = dict({k: 0 for k in STAT_KEYS}, n_atoms=n, energy=np.zeros(len(ENERGY_KEYS)), energies=[],
                **{k: np.zeros((n,) + s, dtype=np.float64) for k, s in ATOM_FLOAT_KEYS.items()})
    m = _stage(info, order, h_count, h_pos, atom_flag, tb)
    if m is None:
        return dict(zero, status=STATUS_TOO_LARGE)
    na = m.n_all

    def evaluate(x):
        degs = []
        ev = _evaluate(m, [tuple(p) for p in x.tolist()], deg_tol, degs)
        trace.extend((k, v, deg_tol) for k, v in degs)
        return ev['total'], np.asarray(ev['grad'], dtype=np.float64).reshape(na, 3), ev
    start = np.asarray(m.pos, dtype=np.float64).reshape(na, 3)
    r = lbfgs_ref(start, evaluate, max_iters, gtol, max_step, trace)
    if r is None:
        return dict(zero, status=STATUS_NONFINITE)
    first, cur, x = r['first'], r['extra'], r['x']
    heavy, hs = _split(m.n, m.h, x)
    gh, ghs = _split(m.n, m.h, r['grad'])
    moved = _vdot(x[:m.n] - start[:m.n], x[:m.n] - start[:m.n])
    c = first['counts']
    energy = first['components'] + [first['total']] + cur['components'] + [cur['total'], r['rms'], math.sqrt(moved / m.n) if m.n else 0.0]
    return dict(zero, status=STATUS_OK, stop_reason=r['stop_reason'], iterations=r['iterations'], n_evals=r['n_evals'], n_all=na, n_ff_bonds=c[0],
                n_angles=c[1], n_torsions=c[2], n_inversions=c[3], n_pairs=c[4], n_fallback=m.n_fallback, energy=np.asarray(energy, dtype=np.float64),
                pos=heavy, h_pos=hs, grad=gh, h_grad=ghs, energies=r['energies'])


def near_threshold(info, order, h_count, h_pos, atom_flag, tables=None, max_iters=DEFAULT_MAX_ITERS, gtol=DEFAULT_GTOL, max_step=DEFAULT_MAX_STEP,
                   deg_tol=DEFAULT_DEG_TOL, band=1e-9):
    """whether some decision of ``relax_ref`` is ``near`` its threshold: the molecules a device comparison may leave out"""
    trace = []
    relax_ref(info, order, h_count, h_pos, atom_flag, tables, max_iters, gtol, max_step, deg_tol, trace)
    return near(trace, band)


def _inputs(mols, tb, kek=None, hyd=None):
    """per molecule (order, h_count, h_pos, atom_flag) from ``kekule.kekulize_ref`` and ``hydrogens.addh_ref`` with the default chemistry"""
    kt, ht = kekule.KekuleTables(tb.atomic_numbers, tb.num_bond_types), hydrogens.HydrogenTables(tb.atomic_numbers, tb.num_bond_types)
    out = []
    for info in mols:
        k = kekule.kekulize_ref(info, kt)
        h = hydrogens.addh_ref(info, k['kek_h'], k['kek_order'], ht)
        out.append((k['kek_order'], h['h_count'], h['h_pos'], h['atom_flag']))
    return out


def _stack(refs):
    out = molpack.stack(refs, LAYOUT)
    out['energy'] = np.asarray([r['energy'] for r in refs], dtype=np.float64).reshape(len(refs), len(ENERGY_KEYS))
    for k, s in ATOM_FLOAT_KEYS.items():
        out[k] = np.concatenate([np.asarray(r[k], dtype=np.float64).reshape((-1,) + s) for r in refs] + [np.zeros((0,) + s)]).astype(np.float64)
    return out


def stack_ref(mols, inputs=None, tables=None, max_iters=DEFAULT_MAX_ITERS, gtol=DEFAULT_GTOL, max_step=DEFAULT_MAX_STEP, deg_tol=DEFAULT_DEG_TOL):
    """``relax_ref`` of every molecule of a list as the results dict ``relax_mols`` returns (numpy): one entry per molecule of every
    key of MOL_KEYS (int32), ``energy`` (molecules, 14; float64: ENERGY_KEYS), and ``pos`` / ``grad`` (atoms, 3), ``h_pos`` / ``h_grad``
    (atoms, 4, 3) float64 over the atoms of the list in turn, ``atom_ptr``.  inputs: per molecule (order, h_count, h_pos, atom_flag), or
    None for those of ``kekule.kekulize_ref`` and ``hydrogens.addh_ref``."""
    tb = _tables(tables)
    inputs = _inputs(mols, tb) if inputs is None else inputs
    if len(inputs) != len(mols):
        raise ValueError('one (order, h_count, h_pos, atom_flag) per molecule')
    return _stack([relax_ref(m, *i, tb, max_iters, gtol, max_step, deg_tol) for m, i in zip(mols, inputs)])


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, order, h_pos, h_count, atom_flag, tables=None, max_iters=DEFAULT_MAX_ITERS, gtol=DEFAULT_GTOL, max_step=DEFAULT_MAX_STEP,
           deg_tol=DEFAULT_DEG_TOL, select=None):
    """``mdx_mol_relax`` on the device arrays `cm` (a ``CompactMols`` with positions), `order` (int32, Eh_stride: ``kek_order`` of
    ``kekule.launch``) and `h_pos` (float64, (N_cap, 4, 3)), `h_count`, `atom_flag` (int32, N_cap) of ``hydrogens.launch`` on the same
    arrays -> dict of device tensors: the keys of STAT_KEYS (B) each (int32, columns of one (B, 11) table), ``energy`` (B, 14; float64)
    and ``pos`` / ``grad`` (N_cap, 3), ``h_pos`` / ``h_grad`` (N_cap, 4, 3) float64 in the layout of the inputs, zero where no molecule
    has a slot.  No sync."""
    import torch
    from . import _lib
    tb = _tables(tables)
    max_iters, gtol, max_step, deg_tol = _check(max_iters, gtol, max_step, deg_tol)
    out, stats = molpack.zeros_for(cm, LAYOUT, stat_keys=STAT_KEYS)
    N = max(cm.N_cap, 1)
    out['energy'] = torch.zeros(cm.B, len(ENERGY_KEYS), dtype=torch.float64, device=cm.device)
    for k, s in ATOM_FLOAT_KEYS.items():
        out[k] = torch.zeros((N,) + s, dtype=torch.float64, device=cm.device)
    if cm.B > 0:
        if cm.atom_pos is None:
            raise ValueError('relaxing needs positions: a CompactMols with atom_pos')
        if (order.dtype != torch.int32 or h_count.dtype != torch.int32 or atom_flag.dtype != torch.int32 or h_pos.dtype != torch.float64 or
                order.numel() < cm.Eh_stride or h_count.numel() < cm.N_cap or atom_flag.numel() < cm.N_cap or h_pos.numel() < 12 * cm.N_cap):
            raise ValueError('order, h_count and atom_flag are int32 tensors and h_pos a float64 tensor in the layout of the compact arrays')
        order, h_pos, h_count, atom_flag = order.contiguous(), h_pos.contiguous(), h_count.contiguous(), atom_flag.contiguous()
        ws = torch.empty(cm.B * WS_DOUBLES, dtype=torch.float64, device=cm.device)
        ops, at = cm.operands()
        _lib.check(_lib.lib().mdx_mol_relax(
            *ops, _lib.ptr(select), at(cm.atom_pos), at(order), at(h_pos), at(h_count), at(atom_flag), len(tb.atomic_numbers), tb.num_bond_types,
            tb.rows.ctypes.data, len(tb.rows), deg_tol, gtol, max_step, max_iters, at(out['pos']), at(out['h_pos']), at(out['grad']), at(out['h_grad']),
            at(stats), at(out['energy']), at(ws), ws.numel() * 8, _lib.stream()))
    return molpack.split_stats(out, stats, STAT_KEYS)


def relax_mols(mols, device, tables=None, max_iters=DEFAULT_MAX_ITERS, gtol=DEFAULT_GTOL, max_step=DEFAULT_MAX_STEP, deg_tol=DEFAULT_DEG_TOL,
               inputs=None, with_inputs=False):
    """Relaxation of a list of molecule dicts with ``atom_pos`` on the device: the list is packed densely, copied and handed to
    ``mdx_mol_kekulize``, ``mdx_mol_hydrogens`` (default chemistry) and ``mdx_mol_relax``.  inputs: per molecule (order, h_count,
    h_pos, atom_flag) to relax the caller's hydrogens instead.  -> the results dict of ``stack_ref`` with device tensors; with
    `with_inputs` -> (the results of ``kekule.kekulize_mols``, of ``hydrogens.addh_mols``, that).  Two bonds between the same pair of
    atoms, a molecule without positions and unknown elements raise ValueError."""
    import torch
    tb = _tables(tables)
    _check(max_iters, gtol, max_step, deg_tol)
    if any('atom_pos' not in m for m in mols):
        raise ValueError('relaxing needs atom_pos in every molecule')
    if with_inputs and inputs is not None:
        raise ValueError('with_inputs returns the assignments made here: give no inputs')
    p, cm = molpack.packed(mols, tb.atomic_numbers, device, positions=True)
    kek = hyd = None
    if inputs is None:
        kek = kekule.launch(cm, kekule.KekuleTables(tb.atomic_numbers, tb.num_bond_types))
        hyd = hydrogens.launch(cm, kek['kek_h'], kek['kek_order'], hydrogens.HydrogenTables(tb.atomic_numbers, tb.num_bond_types))
        ops = (kek['kek_order'], hyd['h_pos'], hyd['h_count'], hyd['atom_flag'])
    else:
        if len(inputs) != len(mols):
            raise ValueError('one (order, h_count, h_pos, atom_flag) per molecule')
        N, E = max(cm.N_cap, 1), max(cm.Eh_stride, 1)
        full = {'order': np.zeros(E, dtype=np.int32), 'h_count': np.zeros(N, dtype=np.int32), 'atom_flag': np.zeros(N, dtype=np.int32),
                'h_pos': np.zeros((N, MAX_H, 3), dtype=np.float64)}
        for m, (o, hc, hp, fl) in enumerate(inputs):
            a0, na, b0, nb = int(p['atom_ptr'][m]), int(p['n_atoms'][m]), int(p['bond_ptr'][m]), int(p['n_bonds'][m])
            full['order'][b0:b0 + nb] = np.asarray(o, dtype=np.int32).reshape(nb)
            full['h_count'][a0:a0 + na], full['atom_flag'][a0:a0 + na] = np.asarray(hc).reshape(na), np.asarray(fl).reshape(na)
            full['h_pos'][a0:a0 + na] = np.asarray(hp, dtype=np.float64).reshape(na, MAX_H, 3)
        d = {k: torch.from_numpy(v).to(cm.device) for k, v in full.items()}
        ops = (d['order'], d['h_pos'], d['h_count'], d['atom_flag'])
    res = _dense(launch(cm, *ops, tb, max_iters, gtol, max_step, deg_tol), cm, p)
    if with_inputs:
        return molpack.dense(kek, cm, p, kekule.LAYOUT), hydrogens._dense(hyd, cm, p), res
    return res


def _dense(out, cm, p):
    floats = {k: out.pop(k) for k in FLOAT_KEYS}
    out = molpack.dense(out, cm, p, LAYOUT)
    out.update({k: v if k == 'energy' else v[:cm.N_cap] for k, v in floats.items()})
    return out


def concat(parts):
    """the results of consecutive batches (host or device arrays, not mixed) as one results dict"""
    parts = [to_host(p) for p in parts]
    out = molpack.concat(parts, LAYOUT)
    out['energy'] = np.concatenate([p['energy'].reshape(-1, len(ENERGY_KEYS)) for p in parts])
    out.update({k: np.concatenate([p[k].reshape((-1,) + s) for p in parts]) for k, s in ATOM_FLOAT_KEYS.items()})
    return out


def empty():
    return stack_ref([])


# ---- the numbers -------------------------------------------------------------------------------------------------------------------

def mol_result(results, m):
    """molecule `m` of a results dict with host arrays as the dict ``relax_ref`` returns (without ``energies``)"""
    out = molpack.mol_slice(results, m, LAYOUT)
    lo = int(results['atom_ptr'][m])
    out['energy'] = np.asarray(results['energy'][m])
    out.update({k: np.asarray(results[k][lo:lo + out['n_atoms']]).reshape((-1,) + s) for k, s in ATOM_FLOAT_KEYS.items()})
    return out


def _hist(values, top, bins):
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    idx = np.clip((np.maximum(v, 0.0) / (top / bins)).astype(np.int64), 0, bins - 1)
    return np.bincount(idx, minlength=bins).tolist()


def summary(results):
    """The numbers of a results dict (host or device arrays) -> dict: ``n_molecules``, ``n_measured`` (status 0), ``n_too_large``,
    ``fraction_nonfinite`` (of all that fit); over the measured molecules ``fraction_converged`` / ``fraction_maxiter`` /
    ``fraction_linesearch``, ``mean_iterations``, the strain (initial - final total energy, kcal/mol) as ``strain_mean`` /
    ``strain_median`` and per heavy atom ``strain_per_atom_mean`` / ``strain_per_atom_median``, ``components_initial`` /
    ``components_final`` (the mean of each component), ``rmsd_heavy_mean`` / ``rmsd_heavy_median``, ``n_fallback`` (atoms typed by a
    fall-back row), ``strain_hist`` (40 bins of 5 kcal/mol from 0, the last also more) and ``rmsd_heavy_hist`` (40 bins of 0.05
    Angstrom).  NaN where nothing was counted.  This project's own UFF-form model over an unverified table, not RDKit's."""
    r = to_host(results)
    n = len(r['status'])
    ok = r['status'] == STATUS_OK
    k = int(ok.sum())
    fit = int((r['status'] != STATUS_TOO_LARGE).sum())
    nan = float('nan')
    en = r['energy'].reshape(-1, len(ENERGY_KEYS))[ok]
    strain = en[:, 5] - en[:, 11]
    heavy = np.maximum(r['n_atoms'][ok].astype(np.float64), 1.0)
    rmsd = en[:, 13]
    share = lambda reason: int((r['stop_reason'][ok] == reason).sum()) / k if k else nan
    stat = lambda v, f: float(f(v)) if len(v) else nan
    return {'n_molecules': n, 'n_measured': k, 'n_too_large': int((r['status'] == STATUS_TOO_LARGE).sum()),
            'fraction_nonfinite': int((r['status'] == STATUS_NONFINITE).sum()) / fit if fit else nan,
            'fraction_converged': share(STOP_CONVERGED), 'fraction_maxiter': share(STOP_MAXITER), 'fraction_linesearch': share(STOP_LINESEARCH),
            'mean_iterations': stat(r['iterations'][ok], np.mean),
            'strain_mean': stat(strain, np.mean), 'strain_median': stat(strain, np.median),
            'strain_per_atom_mean': stat(strain / heavy, np.mean), 'strain_per_atom_median': stat(strain / heavy, np.median),
            'components_initial': {c: stat(en[:, q], np.mean) for q, c in enumerate(COMPONENTS)},
            'components_final': {c: stat(en[:, 6 + q], np.mean) for q, c in enumerate(COMPONENTS)},
            'rmsd_heavy_mean': stat(rmsd, np.mean), 'rmsd_heavy_median': stat(rmsd, np.median),
            'n_fallback': int(r['n_fallback'][ok].astype(np.int64).sum()),
            'strain_hist': _hist(strain, STRAIN_MAX, STRAIN_BINS), 'rmsd_heavy_hist': _hist(rmsd, RMSD_MAX, RMSD_BINS)}


def compare(a, b):
    """two results dicts or two summaries -> dict: Jensen-Shannon divergence (``molpack.jsd_counts``: base 2, in [0, 1], NaN when a
    side is empty) of ``strain_hist`` and of ``rmsd_heavy_hist``, and both sides' ``fraction_converged`` and ``strain_median``"""
    a, b = (x if 'strain_hist' in x else summary(x) for x in (a, b))
    return {'strain': jsd_counts(a['strain_hist'], b['strain_hist']), 'rmsd_heavy': jsd_counts(a['rmsd_heavy_hist'], b['rmsd_heavy_hist']),
            'fraction_converged': [a['fraction_converged'], b['fraction_converged']], 'strain_median': [a['strain_median'], b['strain_median']]}


def write_sdf(path, mols, kek_results, h_results, results):
    """the kekulizable, relaxed (status 0) molecules of `mols` as all-atom mol blocks at their relaxed coordinates (kek_results,
    h_results, results: host or device arrays, one entry per molecule) -> how many were written; ``hydrogens.write_sdf`` otherwise."""
    kr, hr, rr, written = to_host(kek_results), to_host(h_results), to_host(results), 0
    keep = kekule.kekulizable(kr)
    with open(path, 'w') as f:
        for m, info in enumerate(mols):
            kres, res = kekule.mol_result(kr, m), mol_result(rr, m)
            if not keep[m] or res['status'] != STATUS_OK or not (kres['kek_order'] >= 1).all():
                continue
            moved = dict(info, atom_pos=res['pos'])
            try:
                block = hydrogens.allatom_mol_block(moved, kres, dict(hydrogens.mol_result(hr, m), h_pos=res['h_pos']))
            except ValueError:
                continue
            f.write(block + '$$$$\n')
            written += 1
    return written


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    def run(mols, args, device):
        _check(args.iters, args.gtol)
        if device is None:
            kek = kekule.stack_ref(mols)
            hyd = hydrogens.stack_ref(mols)
            inputs = [(kekule.mol_result(kek, m)['kek_order'],) + tuple(hydrogens.mol_result(hyd, m)[k] for k in ('h_count', 'h_pos', 'atom_flag'))
                      for m in range(len(mols))]
            res = stack_ref(mols, inputs, max_iters=args.iters, gtol=args.gtol)
        else:
            kek, hyd, res = relax_mols(mols, device, max_iters=args.iters, gtol=args.gtol, with_inputs=True)
        if args.sdf:
            write_sdf(args.sdf, mols, kek, hyd, res)
        return res
    return molpack.stats_main(
        argv, 'relax', __doc__, ('strain energy and heavy-atom displacement of the relaxed molecules stored in a samples_all.pt',
                                 'Jensen-Shannon divergence of the strain and displacement distributions of two files'),
        [('--sdf', dict(default=None, help='also write the relaxed all-atom mol blocks')),
         ('--iters', dict(type=int, default=DEFAULT_MAX_ITERS, help='L-BFGS iterations at most (200: RDKit\'s default)')),
         ('--gtol', dict(type=float, default=DEFAULT_GTOL, help='rms gradient in kcal/mol/Angstrom at which a molecule has converged (1e-2: a convention)'))],
        run, summary, compare)


if __name__ == '__main__':
    sys.exit(main())
