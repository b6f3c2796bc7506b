"""Times the self-similarity (mdx_fp_tanimoto with the diagonal excluded) of N random fingerprints on the device with device events
after a warm-up, and the numpy restatement ``tanimoto_ref`` on M rows of the same set on this host (wall clock), extrapolated
quadratically to N.  One measurement, no threshold: the numbers go into INTEGRATION.md's section "Set-level similarity".

    python tools/time_similarity.py [--n 10000] [--nbits 2048] [--density 0.05] [--host-rows 2000] [--reps 20] [--out FILE]
"""
import sys
import time

import numpy as np

import evalbench as EB
from moldiff_amd import similarity as S


def main(argv=None):
    ap = EB.parser(reps=20)
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--nbits', type=int, default=2048)
    ap.add_argument('--density', type=float, default=0.05)
    ap.add_argument('--host-rows', type=int, default=2000)
    args = EB.parse(ap, argv)
    g = np.random.default_rng(0)
    bits = np.packbits(g.random((args.n, args.nbits)) < args.density, axis=1, bitorder='little').view(np.uint32).reshape(args.n, -1).copy()
    n_on = S.popcount(bits).sum(1).astype(np.int32)
    zeros = np.zeros(args.n, dtype=np.int64)
    fset = S.FingerprintSet(S.FingerprintSpec(nbits=args.nbits), bits, n_on, zeros, zeros.astype(np.int32)).to(args.device)
    device_ms, out = EB.timed(lambda: S.tanimoto(fset, fset, True), args.reps, warmup=3)
    m = min(args.host_rows, args.n)
    t0 = time.perf_counter()
    want = S.tanimoto_ref(bits[:m], n_on[:m], bits[:m], n_on[:m], True)
    host_s = time.perf_counter() - t0
    sub = S.FingerprintSet(fset.spec, bits[:m], n_on[:m], zeros[:m], zeros[:m].astype(np.int32)).to(args.device)
    got = [x.cpu().numpy() for x in S.tanimoto(sub, sub, True)]
    same = all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(got, want))
    pairs = args.n * (args.n - 1)
    row = {'n': args.n, 'nbits': args.nbits, 'density': args.density, 'device_ms_per_call': round(device_ms, 3),
           'pairs_per_s': round(pairs / (device_ms * 1e-3)), 'host_rows': m, 'host_s': round(host_s, 3),
           'host_s_extrapolated_to_n': round(host_s * (args.n / m) ** 2, 2), 'device_equals_host_on_host_rows': bool(same),
           'diversity': 1.0 - sum(out[2].tolist()) / (S.FIXED_ONE * pairs)}
    EB.report([row], args.out, 'tools/time_similarity.py: one measurement, not gated')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
