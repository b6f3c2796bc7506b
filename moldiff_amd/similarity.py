"""Set-level similarity of decoded molecules: uniqueness, diversity, and similarity to / novelty against a reference set.

The device half is ``mdx_mol_fingerprint`` and ``mdx_fp_tanimoto`` (csrc/mdx_similarity.hip), reached through ``fingerprint_mols`` (a
list of molecule dicts), ``FeaturizeMol.fingerprint_batch`` (the sampler's predictions), ``tanimoto`` and ``summary``.
``fingerprint_ref``, ``tanimoto_ref`` and ``summary_ref`` are the numpy restatements and need no GPU; the GPU tests compare bit for bit.

What it is: the reference reports three set-level numbers under ``similarity`` (scripts/evaluate_all.py:164-174,
utils/scoring_func.py:102-223) from RDKit fingerprints and canonical SMILES.  RDKit is not available here, so the fingerprint and the
identity of a molecule are DEFINED by this project (include/moldiff_hip.h states them; ``fingerprint_ref`` restates them):

  * the fingerprint is a hashed circular fingerprint over (element class, degree) refined `radius` times over the bonds.  It is NOT
    ``Chem.RDKFingerprint`` (a path fingerprint) and there is no ECFP duplicate-substructure removal;
  * the key is a 64-bit isomorphism INVARIANT from `key_rounds` rounds of the same refinement.  It is NOT a canonical SMILES: relabelled
    copies of a molecule always agree, two different molecules can agree (colour refinement cannot separate them, or a hash collision),
    so the number of distinct (key, atom count) pairs is a lower bound of the number of distinct molecules;
  * the molecule is the one AS DECODED, not RDKit's reconstruction of it.

The defaults (radius 2, 2048 bits, 8 key rounds) are this project's choice.  The numbers therefore compare runs of this project with
each other, not with the paper's table; and with no trained checkpoint offline this is an instrument, not a measurement of quality.

    python -m moldiff_amd.similarity fingerprint samples_all.pt --out a.npz [--ref] [--part finished]
    python -m moldiff_amd.similarity summary a.npz [--against train.npz] [--ref]
"""
import argparse
import json
import sys

import numpy as np

from .molpack import CompactMols, DEFAULT_ATOMIC_NUMBERS, host, load_mols, mol_graph, pack_mols, to_device

MAX_COLUMNS = 1 << 22      # mdx_fp_tanimoto: more columns could take row_sum out of int64
FIXED_ONE = 1 << 40        # row_sum's unit: q * 2^40 is an exact integer (include/moldiff_hip.h)
_M = np.uint64(0xffffffff)
_GOLD, _PRIME, _HI = np.uint64(0x9e3779b9), np.uint64(0x01000193), np.uint64(0x5bd1e995)


class FingerprintSpec:
    """What a fingerprint is made with: `radius` rounds set bits, `key_rounds` >= radius rounds feed the key, `nbits` (a multiple of
    32 in 32 .. 32768), and the featuriser's `atomic_numbers` / `num_bond_types` (an element's class index is what is hashed).
    Anything else raises ValueError.  The defaults are this project's choice, not the reference's."""

    def __init__(self, radius=2, nbits=2048, key_rounds=8, atomic_numbers=DEFAULT_ATOMIC_NUMBERS, num_bond_types=4):
        ints = (radius, nbits, key_rounds, num_bond_types)
        if any(isinstance(v, bool) or int(v) != v for v in ints):
            raise ValueError(f'radius, nbits, key_rounds and num_bond_types must be integers, got {ints!r}')
        self.radius, self.nbits, self.key_rounds, self.num_bond_types = (int(v) for v in ints)
        self.atomic_numbers = tuple(int(z) for z in atomic_numbers)
        if not 0 <= self.radius <= self.key_rounds <= 64:
            raise ValueError(f'rounds must satisfy 0 <= radius <= key_rounds <= 64, got {self.radius}, {self.key_rounds}')
        if self.nbits % 32 or not 32 <= self.nbits <= 32768:
            raise ValueError(f'nbits must be a multiple of 32 in 32 .. 32768, got {self.nbits}')
        if not self.atomic_numbers or len(set(self.atomic_numbers)) != len(self.atomic_numbers) or min(self.atomic_numbers) < 1:
            raise ValueError(f'atomic_numbers must be distinct positive numbers, got {self.atomic_numbers!r}')
        if self.num_bond_types < 1:
            raise ValueError(f'num_bond_types must be positive, got {self.num_bond_types}')

    @property
    def words(self):
        return self.nbits // 32

    def to_dict(self):
        return {'radius': self.radius, 'nbits': self.nbits, 'key_rounds': self.key_rounds, 'atomic_numbers': list(self.atomic_numbers),
                'num_bond_types': self.num_bond_types}

    @classmethod
    def from_dict(cls, d):
        return cls(**dict(d))

    def __eq__(self, other):
        return isinstance(other, FingerprintSpec) and self.to_dict() == other.to_dict()

    def __hash__(self):
        return hash(json.dumps(self.to_dict()))


# ---- one molecule on the host --------------------------------------------------------------------------------------------------------

def mix(h):
    """murmur3's fmix32 on an array of 32-bit values held in uint64"""
    h = np.asarray(h, dtype=np.uint64) & _M
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & _M
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & _M
    return h ^ (h >> np.uint64(16))


def atom_ids(info, spec):
    """id_r[a] for r = 0 .. key_rounds -> (key_rounds + 1, n) uint64 array of 32-bit values: the refinement include/moldiff_hip.h
    defines.  Bonds with an index outside the molecule or with i = j are ignored."""
    cls, bi, bt = mol_graph(info, spec.atomic_numbers)
    n = len(cls)
    ok = (bi[0] >= 0) & (bi[0] < n) & (bi[1] >= 0) & (bi[1] < n) & (bi[0] != bi[1])
    i, j, t = bi[0, ok], bi[1, ok], (bt[ok].astype(np.uint64) & _M)
    deg = (np.bincount(i, minlength=n) + np.bincount(j, minlength=n)).astype(np.uint64)
    ids = np.zeros((spec.key_rounds + 1, n), dtype=np.uint64)
    ids[0] = mix(cls.astype(np.uint64) + np.uint64(1) + ((_GOLD * (deg + np.uint64(1))) & _M))
    gt = (_GOLD * t) & _M
    for r in range(spec.key_rounds):
        acc = np.zeros(n, dtype=np.uint64)
        np.add.at(acc, i, mix(ids[r][j] + gt))
        np.add.at(acc, j, mix(ids[r][i] + gt))
        ids[r + 1] = mix(((ids[r] * _PRIME) & _M) + np.uint64(r + 1) + (acc & _M))
    return ids


def fingerprint_ref(info, spec):
    """Numpy restatement of ``mdx_mol_fingerprint`` for one molecule dict (element = atomic numbers, bond_index (2, 2b) with every bond
    once and then flipped, bond_type (2b); the keys ``local3d_ref`` reads, positions not needed) -> dict: ``bits`` (nbits / 32 uint32
    words, bit k = bit k % 32 of word k // 32), ``n_on``, ``key`` (int64: key_hi << 32 | key_lo) and ``n_atoms``.  A molecule without
    atoms has no bit set and key 0."""
    ids = atom_ids(info, spec)
    bits = np.zeros(spec.words, dtype=np.uint32)
    k = (ids[:spec.radius + 1].ravel() % np.uint64(spec.nbits)).astype(np.int64)
    np.bitwise_or.at(bits, k >> 5, (np.uint32(1) << (k & 31).astype(np.uint32)))
    r = np.arange(spec.key_rounds + 1, dtype=np.uint64)[:, None]
    lo, hi = int(mix(ids + r).sum() & _M), int(mix(ids ^ _HI).sum() & _M)
    key = np.asarray([hi << 32 | lo], dtype=np.uint64).view(np.int64)[0]
    return {'bits': bits, 'n_on': int(popcount(bits).sum()), 'key': key, 'n_atoms': int(ids.shape[1])}


def popcount(words):
    """set bits per element of a uint32 array"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (4,)), axis=-1).sum(-1, dtype=np.int64)


def _as_words(bits):
    b = np.ascontiguousarray(host(bits))
    if b.dtype == np.int32:
        b = b.view(np.uint32)
    if b.dtype != np.uint32 or b.ndim != 2:
        raise ValueError('bits must be a (rows, words) array of 32-bit words')
    return b


def tanimoto_ref(bits_a, n_on_a, bits_b, n_on_b, exclude_diagonal=False):
    """Numpy restatement of ``mdx_fp_tanimoto`` -> (row_max float32, row_argmax int32, row_sum int64).  For a pair c = popcount(a & b),
    u = n_on_a + n_on_b - c and q = float32(c) / float32(u) (one correctly rounded division; 0 where u <= 0, this project's choice);
    row_max is the largest q over the row's partners, row_argmax the smallest j attaining it (-1 and 0.0 without a partner) and
    row_sum the sum of q * 2^40, an exact integer per pair.  exclude_diagonal (legal for equally many rows only) leaves i == j out."""
    a, b = _as_words(bits_a), _as_words(bits_b)
    na, nb = np.asarray(host(n_on_a), dtype=np.int64).reshape(-1), np.asarray(host(n_on_b), dtype=np.int64).reshape(-1)
    if a.shape[1] != b.shape[1] or len(na) != len(a) or len(nb) != len(b):
        raise ValueError('the two sets differ in row width, or n_on does not fit its rows')
    if exclude_diagonal and len(a) != len(b):
        raise ValueError('exclude_diagonal needs equally many rows')
    Na, Nb = len(a), len(b)
    row_max, row_argmax, row_sum = np.zeros(Na, dtype=np.float32), np.full(Na, -1, dtype=np.int32), np.zeros(Na, dtype=np.int64)
    if Na == 0 or Nb == 0:
        return row_max, row_argmax, row_sum
    # popcount(a & b) as a product of 0 / 1 matrices: at most 32768 terms of 1, exact in float32
    unpack = lambda w: np.unpackbits(w.view(np.uint8), axis=1).astype(np.float32)
    fb = unpack(b).T.copy()
    for r0 in range(0, Na, 1024):
        r1 = min(r0 + 1024, Na)
        c = np.rint(unpack(a[r0:r1]) @ fb).astype(np.int64)
        u = na[r0:r1, None] + nb[None, :] - c
        q = np.zeros(c.shape, dtype=np.float32)
        np.divide(c.astype(np.float32), u.astype(np.float32), out=q, where=u > 0)
        allowed = np.ones(c.shape, dtype=bool)
        if exclude_diagonal:
            allowed[np.arange(r1 - r0), np.arange(r0, r1)] = False
        row_sum[r0:r1] = np.where(allowed, (q.astype(np.float64) * FIXED_ONE).astype(np.int64), 0).sum(1)
        masked = np.where(allowed, q, np.float32(-1))
        j = masked.argmax(1)                                    # the first, hence the smallest, j attaining the maximum
        has = allowed.any(1)
        row_argmax[r0:r1] = np.where(has, j, -1)
        row_max[r0:r1] = np.where(has, masked[np.arange(r1 - r0), j], np.float32(0))
    return row_max, row_argmax, row_sum


# ---- a set of fingerprints -------------------------------------------------------------------------------------------------------------

class FingerprintSet:
    """Fingerprints of n molecules: ``bits`` (n, nbits / 32) 32-bit words, ``n_on`` (n) int32, ``key`` (n) int64, ``n_atoms`` (n) int32
    and the ``spec``.  The arrays are numpy (``from_ref``, ``load``) or, straight from the device entry points, torch tensors on the
    device (bits as int32: the same words)."""

    def __init__(self, spec, bits, n_on, key, n_atoms):
        self.spec, self.bits, self.n_on, self.key, self.n_atoms = spec, bits, n_on, key, n_atoms
        if not (len(bits) == len(n_on) == len(key) == len(n_atoms)) or tuple(bits.shape) != (len(key), spec.words):
            raise ValueError('arrays of a FingerprintSet must describe the same molecules with nbits / 32 words each')

    def __len__(self):
        return len(self.key)

    @classmethod
    def empty(cls, spec):
        return cls(spec, np.zeros((0, spec.words), dtype=np.uint32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64),
                   np.zeros(0, dtype=np.int32))

    @classmethod
    def from_ref(cls, mols, spec):
        """the numpy path: ``fingerprint_ref`` of every molecule dict of a list"""
        fps = [fingerprint_ref(m, spec) for m in mols]
        if not fps:
            return cls.empty(spec)
        return cls(spec, np.stack([f['bits'] for f in fps]), np.asarray([f['n_on'] for f in fps], dtype=np.int32),
                   np.asarray([f['key'] for f in fps], dtype=np.int64), np.asarray([f['n_atoms'] for f in fps], dtype=np.int32))

    def cpu(self):
        return FingerprintSet(self.spec, _as_words(self.bits), host(self.n_on).astype(np.int32), host(self.key).astype(np.int64),
                              host(self.n_atoms).astype(np.int32))

    def to(self, device):
        """the same set as torch tensors on `device`"""
        import torch
        c = self.cpu()
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
        return FingerprintSet(self.spec, t(c.bits.view(np.int32)), t(c.n_on), t(c.key), t(c.n_atoms))

    def append(self, other):
        """this set followed by `other` (same spec, same kind of arrays) -> a new set"""
        if not isinstance(other, FingerprintSet) or other.spec != self.spec:
            raise ValueError('fingerprints of different specs cannot be joined or compared')
        if hasattr(self.key, 'detach') != hasattr(other.key, 'detach'):
            raise ValueError('one set is on the host and one on the device: use .cpu() or .to(device)')
        if hasattr(self.key, 'detach'):
            import torch
            cat = torch.cat
        else:
            cat = np.concatenate
        return FingerprintSet(self.spec, *(cat([getattr(self, k), getattr(other, k)]) for k in ('bits', 'n_on', 'key', 'n_atoms')))

    def save(self, path):
        c = self.cpu()
        with open(path, 'wb') as f:   # a file object: numpy appends no suffix
            np.savez(f, bits=c.bits, n_on=c.n_on, key=c.key, n_atoms=c.n_atoms, spec=np.asarray(json.dumps(self.spec.to_dict())))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            spec = FingerprintSpec.from_dict(json.loads(str(z['spec'])))
            return cls(spec, z['bits'].astype(np.uint32), z['n_on'].astype(np.int32), z['key'].astype(np.int64), z['n_atoms'].astype(np.int32))


def _comparable(a, b):
    if not isinstance(a, FingerprintSet) or not isinstance(b, FingerprintSet) or a.spec != b.spec:
        raise ValueError('fingerprints of different specs cannot be joined or compared')


# ---- the device path ----------------------------------------------------------------------------------------------------------------

def launch(cm, spec, select=None, ws=None):
    """``mdx_mol_fingerprint`` on the device arrays `cm` (a ``CompactMols``) -> (bits (B, words) int32, n_on (B) int32, key (B)
    int64) on the same device; no sync.  ws: (pointer, bytes) of a workspace, or None to allocate one."""
    import torch
    from . import _lib
    L = _lib.lib()
    B, dev = cm.B, cm.device
    bits = torch.empty(B, spec.words, dtype=torch.int32, device=dev)
    n_on, key = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    if B == 0:
        return bits, n_on, key
    ws = cm.workspace(L.mdx_mol_fingerprint_ws_bytes(cm.N_cap), ws, dev)
    ops, _ = cm.operands()
    _lib.check(L.mdx_mol_fingerprint(*ops, _lib.ptr(select), spec.radius, spec.key_rounds, spec.nbits, _lib.ptr(bits), _lib.ptr(n_on),
                                     _lib.ptr(key), ws[0], ws[1], _lib.stream()))
    return bits, n_on, key


def fingerprint_mols(mols, spec, device):
    """Fingerprints of a list of molecule dicts (finished molecules, or entries of ``samples_all.pt``) on the device: the list is packed
    densely, copied and handed to ``mdx_mol_fingerprint``.  -> FingerprintSet with device tensors."""
    import torch
    device = torch.device(device)
    cm = CompactMols.from_packed(to_device(pack_mols(mols, spec.atomic_numbers), device))
    bits, n_on, key = launch(cm, spec)
    return FingerprintSet(spec, bits, n_on, key, cm.n_atoms)


def tanimoto(a, b, exclude_diagonal=False):
    """``mdx_fp_tanimoto`` of two FingerprintSets with device tensors -> (row_max float32, row_argmax int32, row_sum int64), device
    tensors with one entry per molecule of `a`; no sync.  Sets of different specs raise ValueError."""
    import torch
    from . import _lib
    _comparable(a, b)
    if not (torch.is_tensor(a.bits) and torch.is_tensor(b.bits) and a.bits.is_cuda and a.bits.device == b.bits.device):
        raise ValueError('both sets must hold tensors on one device (FingerprintSet.to)')
    if len(b) > MAX_COLUMNS:
        raise ValueError('more than 2^22 molecules to compare against: split the set')
    L = _lib.lib()
    dev, Na, Nb = a.bits.device, len(a), len(b)
    ba, bb = a.bits.to(torch.int32).contiguous(), b.bits.to(torch.int32).contiguous()
    na, nb = a.n_on.to(torch.int32).contiguous(), b.n_on.to(torch.int32).contiguous()
    row_max, row_argmax = torch.empty(Na, dtype=torch.float32, device=dev), torch.empty(Na, dtype=torch.int32, device=dev)
    row_sum = torch.empty(Na, dtype=torch.int64, device=dev)
    ws = torch.empty(L.mdx_fp_tanimoto_ws_bytes(Na) // 8, dtype=torch.int64, device=dev)
    at = lambda t: _lib.ptr(t) if t.numel() else None
    _lib.check(L.mdx_fp_tanimoto(at(ba), at(na), Na, at(bb), at(nb), Nb, a.spec.nbits, int(bool(exclude_diagonal)), at(row_max),
                                 at(row_argmax), at(row_sum), _lib.ptr(ws), ws.numel() * 8, _lib.stream()))
    return row_max, row_argmax, row_sum


# ---- the set-level numbers ------------------------------------------------------------------------------------------------------------

def _numbers(n, n_distinct, self_sum, n_novel=None, ref_max_sum=None):
    """the summary dict from exact integers: distinct (key, n_atoms) pairs, the total of the self-similarity row_sum, the molecules
    whose pair is absent from the reference and the total of row_max * 2^40 against it -- one place, so both paths round alike"""
    nan = float('nan')
    out = {'n': n, 'uniqueness': n_distinct / n if n else nan,
           'diversity': 1.0 - self_sum / (FIXED_ONE * n * (n - 1)) if n >= 2 else nan}
    if n_novel is not None:
        out.update(novelty=n_novel / n if n else nan, sim_with_ref=ref_max_sum / (FIXED_ONE * n) if n else nan)
    return out


def summary(fset, reference=None):
    """The set-level numbers of a FingerprintSet with device tensors -> dict:
      n             molecules;
      uniqueness    distinct (key, n_atoms) pairs over n -- a lower bound of the share of distinct molecules (the reference: distinct
                    canonical SMILES);
      diversity     1 - the mean Tanimoto similarity over the ordered pairs i != j (NaN below two molecules);
      with `reference` (a FingerprintSet of the same spec on the same device):
      novelty       the share of molecules whose (key, n_atoms) pair is absent from the reference;
      sim_with_ref  the mean over the molecules of the largest similarity to a reference molecule (the reference's sim_with_val).
    The pair matrix is ``mdx_fp_tanimoto``; the sums are exact integers, so the result equals ``summary_ref`` to the last bit."""
    import torch
    n = len(fset)
    if not torch.is_tensor(fset.key):
        raise ValueError('summary needs a set with device tensors (FingerprintSet.to); summary_ref serves host arrays')
    pairs = torch.stack([fset.key.to(torch.int64), fset.n_atoms.to(torch.int64)], 1)
    n_distinct = int(torch.unique(pairs, dim=0).shape[0]) if n else 0
    self_sum = sum(tanimoto(fset, fset, exclude_diagonal=True)[2].tolist()) if n >= 2 else 0      # Python integers: no overflow
    if reference is None:
        return _numbers(n, n_distinct, self_sum)
    _comparable(fset, reference)
    ref_pairs = torch.stack([reference.key.to(torch.int64), reference.n_atoms.to(torch.int64)], 1)
    _, inv = torch.unique(torch.cat([ref_pairs, pairs]), dim=0, return_inverse=True)
    known = torch.zeros(int(inv.max()) + 1 if inv.numel() else 0, dtype=torch.bool, device=inv.device)
    known[inv[:len(reference)]] = True
    n_novel = int((~known[inv[len(reference):]]).sum()) if n else 0
    row_max = tanimoto(fset, reference)[0]
    ref_max_sum = sum((row_max.double() * FIXED_ONE).to(torch.int64).tolist())
    return _numbers(n, n_distinct, self_sum, n_novel, ref_max_sum)


def summary_ref(fset, reference=None):
    """``summary`` from the numpy restatements (``tanimoto_ref``, sets of pairs), for a FingerprintSet with host or device arrays"""
    c = fset.cpu()
    n = len(c)
    pairs = list(zip(c.key.tolist(), c.n_atoms.tolist()))
    self_sum = sum(tanimoto_ref(c.bits, c.n_on, c.bits, c.n_on, True)[2].tolist()) if n >= 2 else 0
    if reference is None:
        return _numbers(n, len(set(pairs)), self_sum)
    _comparable(fset, reference)
    r = reference.cpu()
    known = set(zip(r.key.tolist(), r.n_atoms.tolist()))
    row_max = tanimoto_ref(c.bits, c.n_on, r.bits, r.n_on)[0]
    ref_max_sum = sum((row_max.astype(np.float64) * FIXED_ONE).astype(np.int64).tolist())
    return _numbers(n, len(set(pairs)), self_sum, sum(p not in known for p in pairs), ref_max_sum)


# ---- command line --------------------------------------------------------------------------------------------------------------------

def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m moldiff_amd.similarity', description=__doc__.split('\n\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    f = sub.add_parser('fingerprint', help='fingerprints of the molecules stored in a samples_all.pt')
    f.add_argument('samples')
    f.add_argument('--out', required=True)
    f.add_argument('--part', default='finished')
    f.add_argument('--radius', type=int, default=2)
    f.add_argument('--nbits', type=int, default=2048)
    f.add_argument('--key_rounds', type=int, default=8)
    s = sub.add_parser('summary', help='uniqueness and diversity of a fingerprint file; novelty and similarity against another')
    s.add_argument('set')
    s.add_argument('--against', default=None, help='fingerprint file of the reference set (train / validation molecules)')
    for p in (f, s):
        p.add_argument('--device', default='cuda:0')
        p.add_argument('--ref', action='store_true', help='the numpy path instead of the device')
    args = ap.parse_args(argv)
    if not args.ref:
        import torch
        torch.cuda.set_device(torch.device(args.device))
    if args.cmd == 'fingerprint':
        spec = FingerprintSpec(args.radius, args.nbits, args.key_rounds)
        mols = load_mols(args.samples, args.part)
        fset = FingerprintSet.from_ref(mols, spec) if args.ref else fingerprint_mols(mols, spec, args.device)
        fset.save(args.out)
        print(f'{len(mols)} molecules -> {args.out}: {spec.nbits} bits, radius {spec.radius}, {spec.key_rounds} key rounds')
    else:
        fset = FingerprintSet.load(args.set)
        against = FingerprintSet.load(args.against) if args.against else None
        if args.ref:
            res = summary_ref(fset, against)
        else:
            res = summary(fset.to(args.device), against.to(args.device) if against is not None else None)
        print(json.dumps(res, indent=1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
