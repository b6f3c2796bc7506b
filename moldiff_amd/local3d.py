"""Local 3D geometry statistics of decoded molecules: bond lengths, bond angles and dihedral angles, histogrammed per bond pattern.

The device half is ``mdx_mol_local3d`` (csrc/mdx_local3d.hip), reached through ``local3d_mols`` (a list of molecule dicts) and
``FeaturizeMol.local3d_batch`` (the sampler's predictions); ``local3d_ref`` is the numpy / float64 restatement for ONE molecule dict
and needs no GPU.  The GPU tests compare the two.

What it is: the reference compares sample sets by the distributions its ``Local3D`` collects per SMARTS (utils/evaluation.py:156-329,
scripts/evaluate_all.py:143-155).  A linear SMARTS of that kind is a chain (element, bond, element, ...), which is all a pattern is
here: ``'C:C-N'`` -> ``(6, 4, 6, 1, 7)`` over atomic numbers and the bond ids 1 '-', 2 '=', 3 '#', 4 ':' (aromatic).  Two differences
stand: the reference measures the molecule after RDKit's reconstruction and aromaticity fixes, this measures the molecule AS DECODED;
and no pattern list ships with this module -- derive one from your own data with ``frequent_patterns``.

Items: a length is a bond; an angle is a centre with two bonded neighbours; a dihedral is a path a-b-c-d along three bonds with four
distinct atoms.  A path and its reverse are one item; a pattern and its reverse are one pattern, kept as the lexicographically smaller
tuple.  The default bins (lengths 1.0-2.2 A in 120 bins, angles 0-180 and dihedrals -180-180 degrees in 180 bins) are this project's
choice, not the reference's.  Bin k holds lo + k w <= v < lo + (k + 1) w and the last bin includes hi (``numpy.histogram``); a value
outside [lo, hi], NaN included, is counted in ``outside``.  The device computes in fp32: which side a value within fp32 rounding of a
bin edge falls on is not specified.

The Jensen-Shannon divergence is defined once, in ``molpack.jsd_counts``: base-2 logarithm (range [0, 1]) over the normalised in-range counts,
NaN when either side is empty.

No trained checkpoint is available offline, so this is an instrument: nothing here is a measurement of sample quality.

    python -m moldiff_amd.local3d stats samples_all.pt --patterns patterns.yml --out a.npz [--ref] [--part finished]
    python -m moldiff_amd.local3d compare a.npz b.npz
    python -m moldiff_amd.local3d frequent samples_all.pt [--top 20]        # writes a patterns.yml to stdout
"""
import argparse
import json
import sys
from collections import Counter

import numpy as np

from .molpack import CompactMols, DEFAULT_ATOMIC_NUMBERS, ELEMENT_SYMBOL, host, jsd_counts, load_mols, mol_graph, pack_mols, to_device  # noqa: F401

KINDS = ('lengths', 'angles', 'dihedrals')
BOND_SYMBOL = {1: '-', 2: '=', 3: '#', 4: ':'}
MAX_PATTERNS = 64          # per kind: the device keeps the table in LDS
_FIELDS = {'lengths': 3, 'angles': 5, 'dihedrals': 7}


def parse_pattern(text):
    """'C:C-N' -> (6, 4, 6, 1, 7): element symbols (C N O F P S Cl) joined by the bond symbols - = # :.  A tuple is passed through
    after the same checks.  2, 3 or 4 atoms; anything else raises ValueError."""
    if not isinstance(text, str):
        pat = tuple(int(x) for x in text)
    else:
        number = {s: z for z, s in ELEMENT_SYMBOL.items()}
        bond = {s: b for b, s in BOND_SYMBOL.items()}
        pat, i, s = [], 0, text.strip()
        while i < len(s):
            if len(pat) % 2 == 0:
                sym = s[i:i + 2] if s[i:i + 2] in number else s[i:i + 1]
                if sym not in number:
                    raise ValueError(f'unknown element at {s[i:]!r} in pattern {text!r} (known: {sorted(number)})')
                pat.append(number[sym])
                i += len(sym)
            else:
                if s[i] not in bond:
                    raise ValueError(f'unknown bond symbol {s[i]!r} in pattern {text!r} (known: - = # :)')
                pat.append(bond[s[i]])
                i += 1
        pat = tuple(pat)
    if len(pat) not in (3, 5, 7):
        raise ValueError(f'pattern {text!r} must name 2, 3 or 4 atoms joined by bonds')
    return pat


def canonical(pat):
    """the lexicographically smaller of a pattern and its reverse"""
    pat = tuple(int(x) for x in pat)
    return min(pat, pat[::-1])


def pattern_text(pat):
    return ''.join((ELEMENT_SYMBOL.get(v, f'[#{v}]') if k % 2 == 0 else BOND_SYMBOL.get(v, f'<{v}>')) for k, v in enumerate(pat))


class Local3DSpec:
    """What to collect: the patterns of each kind (strings or tuples; canonicalised; a duplicate, also after reversal, raises
    ValueError, as do a pattern of the wrong length, an element outside `atomic_numbers`, a bond id outside 1 .. num_bond_types and
    more than 64 patterns of a kind) and the bins of each kind as (lo, hi, n).  The default bins are this project's choice."""

    def __init__(self, lengths=(), angles=(), dihedrals=(), length_bins=(1.0, 2.2, 120), angle_bins=(0, 180, 180),
                 dihedral_bins=(-180, 180, 180), atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
        self.atomic_numbers = tuple(int(z) for z in atomic_numbers)
        self.num_bond_types = int(num_bond_types)
        self.patterns, self.bins = {}, {}
        for kind, pats, bins in zip(KINDS, (lengths, angles, dihedrals), (length_bins, angle_bins, dihedral_bins)):
            rows = []
            for p in pats:
                c = canonical(parse_pattern(p))
                if len(c) != _FIELDS[kind]:
                    raise ValueError(f'{p!r} is no pattern of {kind} (needs {(_FIELDS[kind] + 1) // 2} atoms)')
                if any(z not in self.atomic_numbers for z in c[0::2]) or any(not 1 <= b <= self.num_bond_types for b in c[1::2]):
                    raise ValueError(f'{p!r}: element or bond type outside the featuriser\'s')
                if c in rows:
                    raise ValueError(f'duplicate pattern {p!r} in {kind} (a pattern and its reverse are the same)')
                rows.append(c)
            if len(rows) > MAX_PATTERNS:
                raise ValueError(f'more than {MAX_PATTERNS} patterns of {kind}')
            lo, hi, n = float(bins[0]), float(bins[1]), int(bins[2])
            if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo and n > 0 and n == bins[2]):
                raise ValueError(f'{kind}: bins must be (lo, hi, n) with lo < hi and n > 0, got {tuple(bins)!r}')
            self.patterns[kind], self.bins[kind] = tuple(rows), (lo, hi, n)
        self._table = None

    # ---- layout of the flat tables --------------------------------------------------------------------------------------------------
    @property
    def kind_ptr(self):
        c = np.cumsum([0] + [len(self.patterns[k]) for k in KINDS])
        return [int(x) for x in c]

    @property
    def hist_size(self):
        return sum(len(self.patterns[k]) * self.bins[k][2] for k in KINDS)

    def hist_slice(self, kind, row=None):
        """where kind's (rows, bins) block -- or one of its rows -- sits in the flat histogram"""
        off = 0
        for k in KINDS:
            n = self.bins[k][2]
            if k == kind:
                return slice(off, off + len(self.patterns[k]) * n) if row is None else slice(off + row * n, off + (row + 1) * n)
            off += len(self.patterns[k]) * n
        raise KeyError(kind)

    def row_of(self, kind, pattern):
        return self.patterns[kind].index(canonical(parse_pattern(pattern)))

    def edges(self, kind):
        lo, hi, n = self.bins[kind]
        return np.linspace(lo, hi, n + 1)

    def table(self):
        """the host tables ``mdx_mol_local3d`` takes -- (P,7) int32 rows of class indices and bond ids, kind_ptr, bin ranges and
        counts -- built once and kept (the library validates them and hands them to the kernel as launch arguments)"""
        if self._table is None:
            cls = {z: i for i, z in enumerate(self.atomic_numbers)}
            rows = np.zeros((max(self.kind_ptr[3], 1), 7), dtype=np.int32)
            r = 0
            for k in KINDS:
                for p in self.patterns[k]:
                    rows[r, :len(p)] = [cls[v] if i % 2 == 0 else v for i, v in enumerate(p)]
                    r += 1
            self._table = (rows, np.asarray(self.kind_ptr, dtype=np.int32),
                           np.asarray([[self.bins[k][0], self.bins[k][1]] for k in KINDS], dtype=np.float32),
                           np.asarray([self.bins[k][2] for k in KINDS], dtype=np.int32))
        return self._table

    # ---- identity and storage -----------------------------------------------------------------------------------------------------
    def to_dict(self):
        return {'lengths': [list(p) for p in self.patterns['lengths']], 'angles': [list(p) for p in self.patterns['angles']],
                'dihedrals': [list(p) for p in self.patterns['dihedrals']], 'length_bins': list(self.bins['lengths']),
                'angle_bins': list(self.bins['angles']), 'dihedral_bins': list(self.bins['dihedrals']),
                'atomic_numbers': list(self.atomic_numbers), 'num_bond_types': self.num_bond_types}

    @classmethod
    def from_dict(cls, d):
        """from ``to_dict``'s form or a patterns file's content: lengths / angles / dihedrals as strings or lists, bins optional"""
        d = dict(d)
        known = {'lengths', 'angles', 'dihedrals', 'length_bins', 'angle_bins', 'dihedral_bins', 'atomic_numbers', 'num_bond_types'}
        if set(d) - known:
            raise ValueError(f'unknown key(s) {sorted(set(d) - known)} in a pattern file (known: {sorted(known)})')
        return cls(**{k: v for k, v in d.items() if v is not None})

    @classmethod
    def from_yaml(cls, path):
        import yaml
        with open(path) as f:
            return cls.from_dict(yaml.safe_load(f) or {})

    def __eq__(self, other):
        return isinstance(other, Local3DSpec) and self.to_dict() == other.to_dict()

    def __hash__(self):
        return hash(json.dumps(self.to_dict()))


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def enumerate_items(info):
    """Every item of one molecule dict -> {kind: (atoms (k, 2|3|4) int64, chains (k, 3|5|7) int64 over atomic numbers and bond ids)}.
    Bonds with an index outside the molecule or with i = j are ignored.  Angles: centre b, neighbours a < c.  Dihedrals: each bond
    once as the central bond b-c, a over b's other neighbours, d over c's neighbours other than b and a."""
    ele, bi, bt = mol_graph(info)
    n = len(ele)
    ok = (bi[0] >= 0) & (bi[0] < n) & (bi[1] >= 0) & (bi[1] < n) & (bi[0] != bi[1])
    bi, bt = bi[:, ok], bt[ok]
    nbr = [[] for _ in range(n)]
    for (i, j), t in zip(bi.T.tolist(), bt.tolist()):
        nbr[i].append((j, t))
        nbr[j].append((i, t))
    nbr = [np.asarray(x, dtype=np.int64).reshape(-1, 2) for x in nbr]
    ang_atoms, ang_chain, dih_atoms, dih_chain = [], [], [], []
    for b in range(n):
        if len(nbr[b]) < 2:
            continue
        s1, s2 = np.triu_indices(len(nbr[b]), 1)
        a, ta, c, tc = nbr[b][s1, 0], nbr[b][s1, 1], nbr[b][s2, 0], nbr[b][s2, 1]
        swap = a > c
        a, c, ta, tc = np.where(swap, c, a), np.where(swap, a, c), np.where(swap, tc, ta), np.where(swap, ta, tc)
        keep = a != c
        bb = np.full_like(a, b)
        ang_atoms.append(np.stack([a, bb, c], 1)[keep])
        ang_chain.append(np.stack([ele[a], ta, ele[bb], tc, ele[c]], 1)[keep])
    for (b, c), t in zip(bi.T.tolist(), bt.tolist()):
        if not len(nbr[b]) or not len(nbr[c]):
            continue
        ia, id_ = np.meshgrid(np.arange(len(nbr[b])), np.arange(len(nbr[c])), indexing='ij')
        a, t1, d, t3 = nbr[b][ia.ravel(), 0], nbr[b][ia.ravel(), 1], nbr[c][id_.ravel(), 0], nbr[c][id_.ravel(), 1]
        keep = (a != c) & (d != b) & (d != a)
        a, t1, d, t3 = a[keep], t1[keep], d[keep], t3[keep]
        bb, cc, tt = np.full_like(a, b), np.full_like(a, c), np.full_like(a, t)
        dih_atoms.append(np.stack([a, bb, cc, d], 1))
        dih_chain.append(np.stack([ele[a], t1, ele[bb], tt, ele[cc], t3, ele[d]], 1))
    cat = lambda xs, w: np.concatenate(xs) if xs else np.zeros((0, w), dtype=np.int64)
    return {'lengths': (bi.T.copy(), np.stack([ele[bi[0]], bt, ele[bi[1]]], 1) if bi.shape[1] else np.zeros((0, 3), dtype=np.int64)),
            'angles': (cat(ang_atoms, 3), cat(ang_chain, 5)), 'dihedrals': (cat(dih_atoms, 4), cat(dih_chain, 7))}


def item_values(pos, kind, atoms):
    """float64 values of items: lengths in the coordinates' unit, angles in [0, 180] and dihedrals in [-180, 180] degrees (IUPAC sign:
    a = (1,0,0), b = (0,0,0), c = (0,0,1), d = (0,1,1) gives +90), by the atan2 forms the device uses"""
    pos = np.asarray(pos, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        if kind == 'lengths':
            return np.sqrt(((pos[atoms[:, 0]] - pos[atoms[:, 1]]) ** 2).sum(-1))
        if kind == 'angles':
            u, v = pos[atoms[:, 0]] - pos[atoms[:, 1]], pos[atoms[:, 2]] - pos[atoms[:, 1]]
            return np.degrees(np.arctan2(np.sqrt((np.cross(u, v) ** 2).sum(-1)), (u * v).sum(-1)))
        b1, b2, b3 = pos[atoms[:, 1]] - pos[atoms[:, 0]], pos[atoms[:, 2]] - pos[atoms[:, 1]], pos[atoms[:, 3]] - pos[atoms[:, 2]]
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        return np.degrees(np.arctan2((np.cross(n1, n2) * b2).sum(-1) / np.sqrt((b2 * b2).sum(-1)), (n1 * n2).sum(-1)))


def _canonical_rows(chains):
    """rows of an integer matrix, each replaced by the lexicographically smaller of itself and its reverse"""
    if not len(chains):
        return chains
    rev = chains[:, ::-1]
    diff = chains != rev
    first = np.argmax(diff, axis=1)
    r = np.arange(len(chains))
    use_rev = diff.any(1) & (rev[r, first] < chains[r, first])
    return np.where(use_rev[:, None], rev, chains)


def local3d_ref(info, spec):
    """Numpy / float64 restatement of ``mdx_mol_local3d`` for one molecule dict (element = atomic numbers, atom_pos, bond_index
    (2, 2b) with every bond once and then flipped, bond_type (2b)).  -> dict: ``values`` {kind: one float64 array per pattern},
    ``hist`` (flat int64, ``spec.hist_slice``'s layout, via ``numpy.histogram``), ``outside`` (one per pattern, all kinds in turn)
    and ``n_items`` (3: every enumerated item of the kind, matched or not)."""
    pos = np.asarray(info['atom_pos'], dtype=np.float64).reshape(np.asarray(info['element']).size, 3)
    items = enumerate_items(info)
    hist = np.zeros(spec.hist_size, dtype=np.int64)
    outside = np.zeros(spec.kind_ptr[3], dtype=np.int64)
    values, n_items = {}, np.zeros(3, dtype=np.int64)
    for k, kind in enumerate(KINDS):
        atoms, chains = items[kind]
        n_items[k] = len(atoms)
        chains = _canonical_rows(chains)
        val = item_values(pos, kind, atoms) if len(atoms) else np.zeros(0)
        lo, hi, n = spec.bins[kind]
        values[kind] = []
        for r, p in enumerate(spec.patterns[kind]):
            v = val[(chains == np.asarray(p)).all(1)] if len(atoms) else val
            inside = (v >= lo) & (v <= hi)
            hist[spec.hist_slice(kind, r)] = np.histogram(v[inside], bins=n, range=(lo, hi))[0]
            outside[spec.kind_ptr[k] + r] = int((~inside).sum())
            values[kind].append(v)
    return {'values': values, 'hist': hist, 'outside': outside, 'n_items': n_items}


def frequent_patterns(mols, kind, top=20):
    """The `top` most frequent patterns of `kind` among the items of a list of decoded molecule dicts -> list of (canonical pattern
    tuple, count), most frequent first (ties: the smaller tuple first).  This is how a pattern list is derived from one's own data."""
    counts = Counter()
    for info in mols:
        chains = _canonical_rows(enumerate_items(info)[kind][1])
        if len(chains):
            rows, c = np.unique(chains, axis=0, return_counts=True)
            for row, k in zip(rows.tolist(), c.tolist()):
                counts[tuple(row)] += k
    return sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))[:top]


# ---- statistics ---------------------------------------------------------------------------------------------------------------------

class Local3DStats:
    """Accumulated statistics: ``hist`` (flat int64, ``spec.hist_slice``'s layout), ``outside`` (one int64 per pattern), ``n_items``
    (3 int64: all enumerated items per kind, matched or not) and the ``spec``.  The arrays are numpy or, straight from the device
    entry points, torch tensors on the device (no copy is made until a host method needs one)."""

    def __init__(self, spec, hist=None, outside=None, n_items=None):
        self.spec = spec
        self.hist = np.zeros(spec.hist_size, dtype=np.int64) if hist is None else hist
        self.outside = np.zeros(spec.kind_ptr[3], dtype=np.int64) if outside is None else outside
        self.n_items = np.zeros(3, dtype=np.int64) if n_items is None else n_items

    @classmethod
    def from_ref(cls, mols, spec):
        """the numpy path: ``local3d_ref`` summed over a list of molecule dicts"""
        out = cls(spec)
        for info in mols:
            r = local3d_ref(info, spec)
            out.hist, out.outside, out.n_items = out.hist + r['hist'], out.outside + r['outside'], out.n_items + r['n_items']
        return out

    def cpu(self):
        return Local3DStats(self.spec, host(self.hist).astype(np.int64), host(self.outside).astype(np.int64),
                            host(self.n_items).astype(np.int64))

    def __add__(self, other):
        if not isinstance(other, Local3DStats) or other.spec != self.spec:
            raise ValueError('statistics of different specs cannot be added')
        a, b = self.cpu(), other.cpu()
        return Local3DStats(self.spec, a.hist + b.hist, a.outside + b.outside, a.n_items + b.n_items)

    def counts(self, kind, pattern):
        """the histogram row of one pattern (string or tuple, either direction) as a numpy array"""
        return host(self.hist)[self.spec.hist_slice(kind, self.spec.row_of(kind, pattern))].astype(np.int64)

    def outside_of(self, kind, pattern):
        return int(host(self.outside)[self.spec.kind_ptr[KINDS.index(kind)] + self.spec.row_of(kind, pattern)])

    def save(self, path):
        c = self.cpu()
        with open(path, 'wb') as f:   # a file object: numpy appends no suffix
            np.savez(f, hist=c.hist, outside=c.outside, n_items=c.n_items, spec=np.asarray(json.dumps(self.spec.to_dict())))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            spec = Local3DSpec.from_dict(json.loads(str(z['spec'])))
            return cls(spec, z['hist'].astype(np.int64), z['outside'].astype(np.int64), z['n_items'].astype(np.int64))

    def jsd(self, other):
        """-> {kind: {'patterns': {pattern text: JSD}, 'mean': mean over the non-NaN patterns (NaN without one)}}; see jsd_counts"""
        if not isinstance(other, Local3DStats) or other.spec != self.spec:
            raise ValueError('statistics of different specs cannot be compared')
        out = {}
        for kind in KINDS:
            per = {pattern_text(p): jsd_counts(self.counts(kind, p), other.counts(kind, p)) for p in self.spec.patterns[kind]}
            ok = [v for v in per.values() if not np.isnan(v)]
            out[kind] = {'patterns': per, 'mean': float(np.mean(ok)) if ok else float('nan')}
        return out


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def device_stats(spec, device):
    """an empty Local3DStats whose arrays are int64 tensors on `device`: what the device entry points add into"""
    import torch
    z = lambda n: torch.zeros(n, dtype=torch.int64, device=device)
    return Local3DStats(spec, z(spec.hist_size), z(spec.kind_ptr[3]), z(3))


def launch(cm, spec, out, select=None, ws=None):
    """``mdx_mol_local3d`` on the device arrays `cm` (a ``CompactMols`` with atom_pos), adding into the device Local3DStats
    `out`; no sync.  ws: (pointer, bytes) of a workspace, or None to allocate one."""
    import torch
    from . import _lib
    L = _lib.lib()
    B, dev = cm.B, cm.atom_pos.device
    if not all(torch.is_tensor(x) and x.device == dev and x.dtype == torch.int64 for x in (out.hist, out.outside, out.n_items)):
        raise ValueError('`out` must hold int64 tensors on the molecules\' device (local3d.device_stats)')
    if B == 0:
        return out
    rows, kptr, brange, bcount = spec.table()
    ws = cm.workspace(L.mdx_mol_local3d_ws_bytes(cm.N_cap, cm.Eh_stride), ws, dev)
    n_items = torch.empty(3, B, dtype=torch.int64, device=dev)
    ops, at = cm.operands(positions=True)   # `at`: a spec without patterns has empty tables too
    _lib.check(L.mdx_mol_local3d(
        *ops, len(spec.atomic_numbers), spec.num_bond_types, _lib.ptr(select), rows.ctypes.data, kptr.ctypes.data, brange.ctypes.data,
        bcount.ctypes.data, at(out.hist), at(out.outside), _lib.ptr(n_items), ws[0], ws[1], _lib.stream()))
    out.n_items += n_items.sum(1)
    out.last_n_items = n_items     # per molecule, for callers that want it
    return out


def local3d_mols(mols, spec, device, out=None):
    """Statistics of a list of molecule dicts (finished molecules, or entries of ``samples_all.pt``) on the device: the list is
    packed densely, copied and handed to ``mdx_mol_local3d``.  -> Local3DStats with device arrays; `out`: add into this one."""
    import torch
    device = torch.device(device)
    if out is None:
        out = device_stats(spec, device)
    elif out.spec != spec:
        raise ValueError('`out` was made for another spec')
    if not len(mols):
        return out
    p = pack_mols(mols, spec.atomic_numbers, positions=True)
    if int(p['n_atoms'].sum()) > (1 << 24):
        raise ValueError('more than 2^24 atoms in one call: split the list')
    return launch(CompactMols.from_packed(to_device(p, device)), spec, out)


# ---- command line --------------------------------------------------------------------------------------------------------------------

def compare_table(a, b):
    res = a.jsd(b)
    lines = ['%-10s %-24s %10s %10s %8s' % ('kind', 'pattern', 'count a', 'count b', 'JSD')]
    for kind in KINDS:
        for p in a.spec.patterns[kind]:
            t = pattern_text(p)
            lines.append('%-10s %-24s %10d %10d %8.4f' % (kind, t, a.counts(kind, p).sum(), b.counts(kind, p).sum(), res[kind]['patterns'][t]))
        lines.append('%-10s %-24s %10s %10s %8.4f' % (kind, 'mean over non-empty', '', '', res[kind]['mean']))
    return '\n'.join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m moldiff_amd.local3d', description=__doc__.split('\n\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    s = sub.add_parser('stats', help='statistics of the molecules stored in a samples_all.pt')
    s.add_argument('samples')
    s.add_argument('--patterns', required=True, help='YAML: lengths / angles / dihedrals lists, optional *_bins')
    s.add_argument('--out', required=True)
    s.add_argument('--part', default='finished')
    s.add_argument('--device', default='cuda:0')
    s.add_argument('--ref', action='store_true', help='the numpy / float64 path instead of the device')
    c = sub.add_parser('compare', help='Jensen-Shannon divergence per pattern between two statistics files')
    c.add_argument('a')
    c.add_argument('b')
    f = sub.add_parser('frequent', help='the most frequent patterns of stored molecules, as a patterns file')
    f.add_argument('samples')
    f.add_argument('--part', default='finished')
    f.add_argument('--top', type=int, default=20)
    args = ap.parse_args(argv)
    if args.cmd == 'compare':
        print(compare_table(Local3DStats.load(args.a), Local3DStats.load(args.b)))
    elif args.cmd == 'frequent':
        mols = load_mols(args.samples, args.part)
        for kind in KINDS:
            print(f'{kind}:')
            for p, k in frequent_patterns(mols, kind, args.top):
                print(f"  - '{pattern_text(p)}'   # {k}")
    else:
        spec = Local3DSpec.from_yaml(args.patterns)
        mols = load_mols(args.samples, args.part)
        if args.ref:
            stats = Local3DStats.from_ref(mols, spec)
        else:
            import torch
            torch.cuda.set_device(torch.device(args.device))
            stats = local3d_mols(mols, spec, args.device)
        stats.save(args.out)
        print(f'{len(mols)} molecules -> {args.out}: items {host(stats.n_items).tolist()} (lengths, angles, dihedrals)')
    return 0


if __name__ == '__main__':
    sys.exit(main())
