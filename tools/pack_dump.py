"""One-off behaviour check for changes to the weight packer (csrc/mdx_pack.cpp; development tool): dumps what finalize would upload for
the three handle kinds of tests/test_ln_centred_pack.py (`moldiff`, `bondpred`, `net`), each with centred packs off and on, so that a
tree before and a tree after such a change can be compared slot by slot.  It uses only _lib.pack_host.  No GPU.

  python tools/pack_dump.py OUTDIR         six files OUTDIR/<kind>_<0|1>.txt: one line per slot,
                                           "kind F K col0 transposed centred key floats sha256(bytes of the slot)", then "arena <floats>"
  python tools/pack_dump.py --compare A B  the six dumps as multisets of lines (offsets are not in a line): arena sizes, the lines on
                                           one side only, and whether A - B holds dense ('d') slots alone and B - A is empty; exit
                                           status 1 if not
"""
import collections
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ('moldiff', 'bondpred', 'net')


def dump(outdir):
    from moldiff_amd import _lib
    from tests.test_ln_centred_pack import _engine_params
    for kind in KINDS:
        eng, _ = _engine_params(kind)
        for on in (0, 1):
            arena, slots = _lib.pack_host(eng, on)
            with open(os.path.join(outdir, f'{kind}_{on}.txt'), 'w') as f:
                for sl in slots:
                    h = hashlib.sha256(arena[sl['off']:sl['off'] + sl['n']].tobytes()).hexdigest()
                    f.write(f"{sl['kind']} {sl['F']} {sl['K']} {sl['col0']} {int(sl['transposed'])} {int(sl['centred'])} "
                            f"{sl['key'] or '-'} {sl['n']} {h}\n")
                f.write(f'arena {arena.size}\n')
            print(kind, on, len(slots), 'slots', arena.size, 'floats', flush=True)


def read(path):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[-1].startswith('arena ')
    return collections.Counter(lines[:-1]), int(lines[-1].split()[1])


def compare(a, b):
    bad = False
    for kind in KINDS:
        for on in (0, 1):
            name = f'{kind}_{on}.txt'
            (A, na), (B, nb) = read(os.path.join(a, name)), read(os.path.join(b, name))
            only_a, only_b = sorted((A - B).elements()), sorted((B - A).elements())
            print(f'== {kind}, centred packs {"on" if on else "off"}: arena {na} floats ({na * 4 / 2 ** 20:.2f} MiB) -> {nb} floats '
                  f'({nb * 4 / 2 ** 20:.2f} MiB); {sum(A.values())} -> {sum(B.values())} slots')
            print(f'   only in A: {len(only_a)} lines ({sum(int(x.split()[7]) for x in only_a)} floats), only in B: {len(only_b)} lines')
            for x in only_a:
                print('   - ' + ' '.join(x.split()[:8]))
            for x in only_b:
                print('   + ' + ' '.join(x.split()[:8]))
            ok = all(x.startswith('d ') for x in only_a) and not only_b
            print('   ' + ('every other slot identical, bit for bit' if ok else 'DIFFERENT beyond removed dense slots'))
            bad |= not ok
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    os.makedirs(sys.argv[1], exist_ok=True)
    dump(sys.argv[1])
