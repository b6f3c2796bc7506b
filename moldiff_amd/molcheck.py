"""Quality check of decoded molecules: fragments, valences, shortest contact, longest bond -- the host half.

The device half is ``mdx_mol_check`` / ``mdx_mol_keep_component`` (csrc/mdx_molcheck.hip), reached through
``FeaturizeMol.check_batch``; ``check_ref`` below is the plain numpy restatement of the same rules for ONE decoded molecule
dict (an entry of ``samples_all.pt``, or what ``decode_output`` / ``decode_batch`` return).  The GPU tests compare the two.

What the check is: the reference finishes a molecule when RDKit sanitises it and its SMILES has no '.'
(scripts/sample_drug3d.py:141-153, utils/reconstruct.py:245-271).  "One fragment" is the second condition exactly.  "No atom
above its largest permitted valence" is a NECESSARY condition of the first, not a restatement of it: there is no aromaticity
perception, no formal charge and no hydrogen in this check, so a molecule the reference would refuse on kekulisation passes it.
The kekulisation test is a separate instrument, ``mdx_mol_kekulize`` (moldiff_amd/kekule.py): the rule 'kekule' is 'valence' and
"every aromatic system has a Kekulé structure" by THIS PROJECT'S MODEL of that step -- default tables unverified against RDKit, the
first structure in search order rather than a charge-minimal one -- so it too models the reference's test and does not restate it.
The two distances are descriptive; no rule is built on them.

``DEFAULT_MAX_VALENCE`` maps an atomic number to the largest explicit valence the reference's pipeline can let through for that
element -- written down from memory of RDKit's element table (nitrogen is 4 because ``fix_valence`` charges a four-valent N).
RDKit is not available where this was written, so THE TABLE IS UNCHECKED AGAINST RDKit.  It is only a default: every entry point
takes ``max_valence=``.
"""
from fractions import Fraction

import numpy as np

DEFAULT_MAX_VALENCE = {6: 4, 7: 4, 8: 2, 9: 1, 15: 7, 16: 6, 17: 1}
ACCEPT_RULES = ('connected', 'valence', 'kekule')


def valence_table(atomic_numbers, max_valence=None):
    """``max_valence`` (dict atomic number -> largest valence; None = the default) as a list in the order of `atomic_numbers`.
    An element without an entry is refused: a missing limit must not read as 'anything goes'."""
    table = DEFAULT_MAX_VALENCE if max_valence is None else max_valence
    missing = [int(z) for z in atomic_numbers if int(z) not in table]
    if missing:
        raise ValueError(f'max_valence has no entry for element(s) {missing}')
    return [int(table[int(z)]) for z in atomic_numbers]


def fragment_fraction(f):
    """The --largest_fragment threshold as a rational (p, q): 0 < f <= 1, anything else is refused (there is no default)."""
    try:
        f = float(f)
    except (TypeError, ValueError):
        raise ValueError(f'largest_fragment must be a number in (0, 1], got {f!r}')
    if not (0.0 < f <= 1.0):
        raise ValueError(f'largest_fragment must be in (0, 1], got {f!r}')
    r = Fraction(f).limit_denominator(1 << 20)   # exact for every short decimal or binary fraction; products stay far inside int64
    return r.numerator, r.denominator


def accept_rule(name):
    if name not in ACCEPT_RULES:
        raise ValueError(f'unknown acceptance rule {name!r} (one of {list(ACCEPT_RULES)})')
    return name


def bond_weight2(bond_type, num_bond_types):
    """Twice the bond order: types 1, 2, 3 -> 2, 4, 6; the last type `num_bond_types` (aromatic in the shipped featuriser) -> 3."""
    t = np.asarray(bond_type, dtype=np.int64)
    return np.where(t == num_bond_types, 3, 2 * t)


def check_ref(info, max_valence=None, num_bond_types=4):
    """Numpy restatement of ``mdx_mol_check`` for one decoded molecule dict (element = atomic numbers, atom_pos, bond_index
    (2, 2b) with every bond once and then flipped, bond_type (2b)).  Returns a dict: per atom ``component`` (index of the smallest
    atom of the atom's fragment), ``valence2`` (twice the bond-order sum) and ``valence`` (= valence2 / 2, float); per molecule
    ``n_atoms``, ``n_components`` (0 without atoms), ``largest_size``, ``largest_label`` (ties to the smaller label, -1 without
    atoms), ``n_overvalent`` (atoms with valence2 // 2 above max_valence[element]: half bonds round down), ``min_dist`` (shortest
    distance over all pairs of distinct atoms, inf below two atoms) and ``max_bond_len`` (0 without bonds), both in float64 from
    the stored coordinates.  max_valence: dict atomic number -> largest valence (None = DEFAULT_MAX_VALENCE, which is unchecked
    against RDKit -- see the module docstring)."""
    ele = np.asarray(info['element'], dtype=np.int64).reshape(-1)
    n = int(ele.shape[0])
    table = DEFAULT_MAX_VALENCE if max_valence is None else max_valence
    missing = sorted({int(z) for z in ele if int(z) not in table})
    if missing:
        raise ValueError(f'max_valence has no entry for element(s) {missing}')
    pos = np.asarray(info['atom_pos'], dtype=np.float64).reshape(n, 3)
    if 'bond_index' in info and np.asarray(info['bond_index']).size:
        bi = np.asarray(info['bond_index'], dtype=np.int64)
        nb = bi.shape[1] // 2
        bi, bt = bi[:, :nb], np.asarray(info['bond_type'], dtype=np.int64)[:nb]
    else:
        bi, bt = np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64)
    # fragments: repeated minimum over the bonds until nothing changes
    comp = np.arange(n, dtype=np.int64)
    while True:
        low = np.minimum(comp[bi[0]], comp[bi[1]])
        new = comp.copy()
        np.minimum.at(new, bi[0], low)
        np.minimum.at(new, bi[1], low)
        if (new == comp).all():
            break
        comp = new
    labels, sizes = np.unique(comp, return_counts=True)
    if n:
        k = int(np.argmax(sizes))          # first maximum of ascending labels = ties to the smaller label
        largest_size, largest_label = int(sizes[k]), int(labels[k])
    else:
        largest_size, largest_label = 0, -1
    v2 = np.zeros(n, dtype=np.int64)
    w = bond_weight2(bt, num_bond_types)
    np.add.at(v2, bi[0], w)
    np.add.at(v2, bi[1], w)
    limit = np.array([table[int(z)] for z in ele], dtype=np.int64)
    if n >= 2:
        d = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1))
        min_dist = float(d[np.triu_indices(n, 1)].min())
    else:
        min_dist = float('inf')
    blen = np.sqrt(((pos[bi[0]] - pos[bi[1]]) ** 2).sum(-1))
    return {'component': comp, 'valence2': v2, 'valence': v2 / 2.0, 'n_atoms': n, 'n_components': int(labels.shape[0]),
            'largest_size': largest_size, 'largest_label': largest_label, 'n_overvalent': int((v2 // 2 > limit).sum()),
            'min_dist': min_dist, 'max_bond_len': float(blen.max()) if blen.size else 0.0}


def restrict_ref(info, component, label):
    """Numpy restatement of ``mdx_mol_keep_component`` for one molecule dict: the atoms with component == label, order kept, bonds
    re-indexed (and mirrored like the input).  Keys other than the six decoded arrays are carried over unchanged."""
    keep = np.asarray(component) == label
    renum = -np.ones(keep.shape[0], dtype=np.int64)
    renum[keep] = np.arange(int(keep.sum()))
    bi = np.asarray(info['bond_index'], dtype=np.int64)
    ok = keep[bi[0]] & keep[bi[1]] if bi.size else np.zeros(0, dtype=bool)
    out = dict(info)
    out.update(element=np.asarray(info['element'])[keep], atom_pos=np.asarray(info['atom_pos'])[keep],
               bond_index=renum[bi[:, ok]] if bi.size else bi, bond_type=np.asarray(info['bond_type'])[ok])
    if 'atom_prob' in info:
        out['atom_prob'] = np.asarray(info['atom_prob'])[keep]
    if 'bond_prob' in info:
        out['bond_prob'] = np.asarray(info['bond_prob'])[ok]
    return out


def judge(info, report, m, rule, max_valence=None, annotate=False):
    """The sampling entry point's verdict on molecule `m` of a ``check_batch`` result (info = mols[m]) -> (finished, n_components,
    n_overvalent) of the molecule AS IT STANDS: 'connected' = one fragment, 'valence' = that and no over-valent atom; 'kekule' is
    judged here as 'valence', and the caller adds "kekulizable" from ``kekule.kekulizable``.  A salvaged
    molecule is one fragment by construction and its atoms keep the valences they had, so its count comes from info['valence'];
    every other molecule's figures are the report's.  annotate: write the report's figures (of the molecule as decoded) and
    ``salvaged`` into `info` as plain Python numbers."""
    ncomp, nover, salvaged = int(report['n_components'][m]), int(report['n_overvalent'][m]), bool(report['salvaged'][m])
    if annotate:
        info.update(n_components=ncomp, n_overvalent=nover, min_dist=float(report['min_dist'][m]),
                    max_bond_len=float(report['max_bond_len'][m]), salvaged=salvaged)
    if salvaged:
        table = DEFAULT_MAX_VALENCE if max_valence is None else max_valence
        limit = np.array([table[int(z)] for z in info['element']], dtype=np.int64)
        ncomp, nover = 1, int((np.floor(info['valence']).astype(np.int64) > limit).sum())
    return ncomp == 1 and (rule == 'connected' or nover == 0), ncomp, nover


def quality_summary(rows, n_finished, n_failed, kekule=False):
    """The entry point's quality report from one dict per SAMPLED molecule (n_components, n_overvalent, min_dist, max_bond_len,
    salvaged -- all of the molecule as decoded): counts, their fractions of sampled, and medians of the two distances.  kekule: the
    rows carry ``kekulizable`` (of the molecule as it stands), and the counts gain it."""
    n = len(rows)
    counts = {'sampled': n,
              'connected': sum(1 for r in rows if r['n_components'] == 1),
              'valence_clean': sum(1 for r in rows if r['n_components'] >= 1 and r['n_overvalent'] == 0),
              'finished': int(n_finished), 'salvaged': sum(1 for r in rows if r['salvaged']), 'failed': int(n_failed)}
    if kekule:
        counts['kekulizable'] = sum(1 for r in rows if r['kekulizable'])
    md = [r['min_dist'] for r in rows if np.isfinite(r['min_dist'])]
    return {'counts': counts, 'fractions': {k: (v / n if n else 0.0) for k, v in counts.items() if k != 'sampled'},
            'median_min_dist': float(np.median(md)) if md else None,
            'median_max_bond_len': float(np.median([r['max_bond_len'] for r in rows])) if rows else None}
