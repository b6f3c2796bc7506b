"""The two launches that produce every weight gradient of a float16 training step, through the C ABI with raw device pointers:
`mdx_op_wgrad_grouped` (wgrad_grouped_kernel<KIND>, eight tile classes over a device record table) and `mdx_op_reduce_deferred`
(reduce_deferred_kernel), one contraction at a time against float64 at the smallest shapes that reach each class, its tiling, the
record look-up and the dealing of a record's blocks.  Tables are built as csrc/mdx_fast.cpp builds them (tests/wgrad_cases.py, itself
checked on the host by tests/test_wgrad_queue_host.py).

Bounds.  Inputs are float16-representable, so a product is exact in fp32 and only the accumulation rounds:
  * an fp32 accumulation allows  ACC * sum |terms|,  ACC = 2e-6  (the convention of tests/test_gpu_typed_ops.py), element by element;
  * adding a sum s to a destination d is one more fp32 addition: |d| is one more term of that sum;
  * rounding the sum into float16 (rkind 2) allows  2^-11 |s| + 2^-25,  into bfloat16 (rkind 1)  2^-8 |s| + 2^-134  (half an ulp; the
    second term covers subnormals), where |s| <= |ref| + the accumulation bound.
Every partial buffer starts as a NaN sentinel with guard zones between the records: each float a record owns must be written and every
other float must keep the sentinel.  For classes 0..4 the partials must be byte-equal to mdx_op_xgemm_tn_t(dW = NULL) over the same row
ranges; classes 5..7 exist only in the grouped kernel and have the float64 bound alone.  Each comparison prints
`PARITY <case> <quantity> <largest error / bound>`; the table of one run is kept in profiles/wgrad_queue_parity.txt."""
import collections
import zlib

import numpy as np
import pytest
import torch

from tests import util as U
from tests import wgrad_cases as W
from moldiff_amd._lib import stream

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

H_EPS, H_TINY = 2.0 ** -11, 2.0 ** -25
B_EPS, B_TINY = 2.0 ** -8, 2.0 ** -134     # bfloat16: 8 significant bits (float16: 11), subnormals 2^-133 apart
ACC = 2e-6
SENT = 0x7fc5a5a5          # a quiet NaN no kernel produces
GUARD = 64                 # sentinel floats between two records' areas
BIG = 10 ** 6              # `splits` that gives the smallest row range, mper = 64


def _sentinel(n):
    return torch.full((n,), SENT, dtype=torch.int32, device=DEV)


def _check(case, name, got, ref, bound):
    """every element of |got - ref| <= bound (float64; a zero bound demands equality); prints the largest ratio"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (case, name, got.shape, ref.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert np.isfinite(got).all(), (case, name, 'not finite')
    err = np.abs(got - ref)
    zero = bound == 0
    assert not (err[zero] > 0).any(), (case, name, 'differs where the model is exact')
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print(f'PARITY {case} {name} {ratio:.3f}')
    assert ratio <= 1.0, (case, name, ratio)


def _same_bytes(case, name, a, b):
    ok = np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))
    print(f'PARITY {case} {name} {"exact" if ok else "DIFFERS"}')
    assert ok, (case, name)


def _container(rkind, s_abs):
    return {0: 0.0 * s_abs, 1: B_EPS * s_abs + B_TINY, 2: H_EPS * s_abs + H_TINY}[rkind]


def _table(flat):
    return torch.tensor(flat, dtype=torch.int64, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) every tile class, every partial
# ---------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'kind N K M splits dt layout bias twin')
TILE = {0: (128, 128), 1: (128, 64), 2: (64, 128), 3: (64, 64), 4: (64, 64), 5: (32, 64), 6: (64, 32)}   # (n, k) tile of a class
MS = (1, 63, 64, 65, 129, 512, 513, 645, 903, 1025)   # with 64-row ranges: S = 1, 1, 1, 2, 3, 8, 9, 11, 15, 17
FEW = (1, 65, 513, 645)


def _name(c):
    return f'k{c.kind}-{c.N}x{c.K}-M{c.M}-{"plan" if c.splits == 1 else "m64"}-dt{c.dt}-{c.layout}-{"b" if c.bias else "nb"}'


def _cases():
    out = []

    def add(kind, N, K, Ms, dt=3, layouts=('tight', 'slice'), twin=True):
        for i, M in enumerate(Ms):
            out.append(Case(kind, N, K, M, BIG, dt, layouts[i % len(layouts)], i % 3 != 2, twin))
    add(0, 128, 128, FEW), add(0, 256, 128, MS)                       # gy = 2
    add(1, 128, 64, FEW), add(1, 128, 192, MS)                        # gx = 3
    add(2, 64, 128, MS)
    add(3, 64, 64, FEW), add(3, 192, 64, MS)                          # gy = 3
    add(4, 54, 6, FEW, dt=1, layouts=('tight', 'slice', 'off1'))      # fp32 X; one case starts one element in
    add(4, 64, 16, FEW, dt=0)
    add(4, 256, 256, MS, layouts=('off1',))                           # float16 on a base that is off 16 bytes: gx = gy = 4
    add(4, 64, 64, FEW, layouts=('ld4',))                             # float16 rows that are no multiple of 16 bytes
    add(5, 32, 64, MS, twin=False)
    add(6, 64, 32, MS, twin=False)
    for dt in range(4):
        for j, (N, K) in enumerate([(1, 4), (1, 12), (1, 32), (1, 256), (4, 1), (32, 1), (256, 1)]):
            add(7, N, K, (MS[(j + dt) % 10], MS[(j + dt + 5) % 10]), dt=dt, twin=False)
    # the plan's own rows per block (splits = 1): M = mper and mper + 1.  The per-call operator has no `splits` that cuts 1,025 rows
    # into ranges of 1,024 (or 513 into 512), so those cases have no twin; the test asserts that there is none.
    out += [Case(0, 128, 128, 1025, 1, 3, 'slice', True, True), Case(1, 128, 64, 1024, 1, 3, 'tight', False, True),
            Case(2, 64, 128, 1024, 1, 3, 'tight', True, True), Case(2, 64, 128, 1025, 1, 3, 'slice', True, False),
            Case(3, 64, 64, 1024, 1, 3, 'slice', False, True), Case(3, 64, 64, 1025, 1, 3, 'tight', True, False),
            Case(4, 54, 6, 512, 1, 1, 'slice', True, True), Case(4, 64, 16, 513, 1, 0, 'tight', True, False),
            Case(5, 32, 64, 1024, 1, 3, 'slice', True, False), Case(5, 32, 64, 1025, 1, 3, 'tight', False, False),
            Case(6, 64, 32, 1024, 1, 3, 'tight', True, False), Case(6, 64, 32, 1025, 1, 3, 'slice', True, False),
            Case(7, 1, 256, 256, 1, 3, 'slice', True, False), Case(7, 1, 256, 257, 1, 3, 'tight', True, False),
            Case(7, 32, 1, 256, 1, 1, 'tight', True, False), Case(7, 32, 1, 257, 1, 2, 'slice', False, False)]
    return out


CASES = _cases()


def _tiles(c):
    return 1 if c.kind == 7 else W.ceil_div(c.K, TILE[c.kind][1]) * W.ceil_div(c.N, TILE[c.kind][0])


def _group(kind):
    """up to five 64-row-range cases of one class with different block counts, a multi-tile record with a short last dealing chunk
    (S % 8 in {3, 7}) first in line where the class has one, and not in order of size"""
    pool = [c for c in CASES if c.kind == kind and c.splits == BIG]
    if kind == 7:
        pool = pool[::5] + pool          # shapes and containers of both forms (N == 1, K == 1) in one table
    pool.sort(key=lambda c: not (_tiles(c) > 1 and W.ceil_div(c.M, 64) % 8 in (3, 7)))
    picked, seen = [], set()
    for c in pool:
        b = _tiles(c) * W.ceil_div(c.M, 64)
        if b not in seen and len(picked) < 5:
            seen.add(b), picked.append(c)
    return picked[1::2] + picked[0::2]


def _operand(g, M, C, half, layout):
    """(M, C) float16-representable values as a column slice of a wider random matrix -> (storage, address, ld, float64 values)"""
    pad, col0 = {'tight': (0, 0), 'slice': (16, 8), 'off1': (8, 1), 'ld4': (4, 0)}[layout]
    wide = torch.from_numpy(g.standard_normal((M, C + pad)).astype(np.float32)).to(DEV).half()
    if not half:
        wide = wide.float()
    view = wide[:, col0:col0 + C]
    return wide, view.data_ptr(), wide.stride(0), view.double().cpu().numpy()


def _jobs(kind, cases):
    jobs, off = [], GUARD
    for c in cases:
        g = U.rng(zlib.crc32(_name(c).encode()))
        gs, gp, ldg, g64 = _operand(g, c.M, c.N, c.dt & 1, c.layout)
        xs, xp, ldx, x64 = _operand(g, c.M, c.K, (c.dt >> 1) & 1, c.layout)
        p = W.plan(c.M, c.N, c.K, c.splits, c.dt, ldg, ldx, gp % 16 == 0 and xp % 16 == 0)
        assert p['kind'] == kind, (_name(c), p)
        assert p['blocks'] == _tiles(c) * p['S'] and (c.splits == 1 or p['mper'] == 64), (_name(c), p)
        jobs.append(dict(case=c, G=gp, X=xp, ldg=ldg, ldx=ldx, M=c.M, N=c.N, K=c.K, dt=c.dt, plan=p, bias=c.bias, off=off, g64=g64, x64=x64,
                         keep=(gs, xs)))
        off += (p['psize'] + 3) // 4 * 4 + GUARD
    return jobs, off


def _twin(j, tag, got_p, got_b):
    """the per-call operator over the same row ranges leaves the same bytes (classes 0..4)"""
    c, p = j['case'], j['plan']
    S, N, K = p['S'], c.N, c.K
    want = (p['S'], p['mper'], p['boff'])
    if not c.twin:
        assert all(W.per_call_layout(c.M, N, K, s) != want for s in range(1, c.M + 1)), (tag, 'a per-call twin exists')
        return
    assert W.per_call_layout(c.M, N, K, c.splits) == want, (tag, want)
    part = _sentinel((p['psize'] + 3) // 4 * 4)
    db = torch.zeros(N, dtype=torch.float32, device=DEV) if c.bias else None
    rc = W.lib().mdx_op_xgemm_tn_t(j['G'], j['ldg'], j['X'], j['ldx'], None, K, db.data_ptr() if c.bias else None, c.M, N, K, c.splits,
                                   part.data_ptr(), 2, 0, c.dt, stream())
    assert rc == 0, W.lib().mdx_last_error()
    torch.cuda.synchronize()
    tb = part.cpu().numpy()
    _same_bytes(tag, 'P==per-call', got_p, tb[:S * N * K])
    if c.bias:
        _same_bytes(tag, 'Pb==per-call', got_b, tb[p['boff']:p['boff'] + S * N])
    else:
        assert (tb[S * N * K:] == SENT).all(), (tag, 'the per-call twin wrote bias partials nobody asked for')


def _run_grouped(kind, cases, where):
    jobs, size = _jobs(kind, cases)
    area = _sentinel(size)
    for j in jobs:
        j['P'] = area.data_ptr() + 4 * j['off']
    flat, total = W.grouped_table(jobs)
    desc = _table(flat)
    rc = W.lib().mdx_op_wgrad_grouped(desc.data_ptr(), len(jobs), total, kind, stream())
    assert rc == 0, W.lib().mdx_last_error()
    torch.cuda.synchronize()
    bits = area.cpu().numpy()
    owner = np.full(size, -1)
    for i, j in enumerate(jobs):
        p, c = j['plan'], j['case']
        owner[j['off']:j['off'] + p['S'] * c.N * c.K] = i
        if c.bias:
            owner[j['off'] + p['boff']:j['off'] + p['boff'] + p['S'] * c.N] = i
    stray = np.flatnonzero((owner < 0) & (bits != SENT))
    assert stray.size == 0, (where, 'written outside every record: first float offsets', stray[:8].tolist(), [j['off'] for j in jobs])
    for i, j in enumerate(jobs):
        p, c = j['plan'], j['case']
        tag = f'{where}:{_name(c)}'
        S, N, K = p['S'], c.N, c.K
        missed = np.flatnonzero((owner == i) & (bits == SENT))
        assert missed.size == 0, (tag, 'never written: float offsets in the record', (missed[:8] - j['off']).tolist())
        got_p = bits[j['off']:j['off'] + S * N * K]
        got_b = bits[j['off'] + p['boff']:j['off'] + p['boff'] + S * N]
        prod, aprod, col, acol = W.partials_ref(j['g64'], j['x64'], c.M, p['mper'], S)
        _check(tag, 'P', got_p.view(np.float32).reshape(S, N, K), prod, ACC * aprod)
        if c.bias:
            _check(tag, 'Pb', got_b.view(np.float32).reshape(S, N), col, ACC * acol)      # [S][N]: one value per range where N == 1
        if kind <= 4:
            _twin(j, tag, got_p, got_b)
    return jobs, area


@pytest.mark.parametrize('case', CASES, ids=_name)
def test_one_record_alone(case):
    _run_grouped(case.kind, [case], 'alone')


@pytest.mark.parametrize('kind', range(8))
def test_records_of_one_class_in_one_launch(kind):
    cases = _group(kind)
    assert 3 <= len(cases) <= 5 and len({_tiles(c) * W.ceil_div(c.M, 64) for c in cases}) == len(cases)
    if any(_tiles(c) > 1 for c in CASES if c.kind == kind):
        assert any(_tiles(c) > 1 and W.ceil_div(c.M, 64) % 8 in (3, 7) for c in cases)        # a short dealing chunk with gx gy > 1
    _run_grouped(kind, cases, f'group{kind}')


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the deferred reduction alone, on synthetic partials
# ---------------------------------------------------------------------------------------------------------------------------------
RED_SHAPES = ((1, 1), (1, 3), (5, 7), (2, 64), (3, 128), (64, 64))      # blocks 1, 1, 1, 1, 3, 32
RED_S = (1, 7, 8, 9, 255, 256)


def _pstride(total, form):
    if form == 'odd':                                                    # planes that are no multiple of 16 bytes apart
        return total + 1 if (total + 1) % 4 else total + 2
    return (total + 3) // 4 * 4 + 4


def _planes(recs, form):
    """the records' partial planes in one buffer: [S + extra][pstride] each, NaN between a plane's last element and the next plane (a
    load past `rows * cols` poisons the sum), sentinel planes behind the partials of a chunked record -> (buffer, offsets)"""
    lead = 5 if form == 'off4' else 4                                    # 'off4': every record's base is 4 bytes off a 16-byte boundary
    off, offs = lead, []
    for r in recs:
        offs.append(off)
        off += ((r['S'] + r['extra']) * r['pstride'] + 3) // 4 * 4 + GUARD
    buf = _sentinel(off)
    host = buf.cpu().numpy()
    for r, o in zip(recs, offs):
        total = r['rows'] * r['cols']
        v = host[o:o + r['S'] * r['pstride']].view(np.float32).reshape(r['S'], r['pstride'])
        v[:, :total] = r['planes']
    buf.copy_(torch.from_numpy(host))
    return buf, offs


def _dst(recs):
    """destinations in one sentinel buffer: an adding record finds its `init` values, a storing one the sentinel"""
    off, offs = GUARD, []
    for r in recs:
        offs.append(off)
        off += r['rows'] * r['ld'] + GUARD
    host = np.full(off, SENT, dtype=np.int32)
    for r, o in zip(recs, offs):
        if not r['store']:
            v = host[o:o + r['rows'] * r['ld']].view(np.float32).reshape(r['rows'], r['ld'])
            v[:, :r['cols']] = r['init']
    return torch.from_numpy(host).to(DEV), offs


def _reduce(recs, form):
    """both tables of sink_record for `recs` -> (destination bits, their offsets, partial buffer, its offsets)"""
    for r in recs:
        r['pstride'] = _pstride(r['rows'] * r['cols'], form)
    pbuf, poffs = _planes(recs, form)
    dbuf, doffs = _dst(recs)
    for r, po, do in zip(recs, poffs, doffs):
        r['P'], r['dst'] = pbuf.data_ptr() + 4 * po, dbuf.data_ptr() + 4 * do
        assert (r['P'] % 16 == 0) == (form != 'off4')
    (t1, b1), (t2, b2) = W.red_tables(recs)
    d1 = _table(t1)
    assert W.lib().mdx_op_reduce_deferred(d1.data_ptr(), len(t1) // 8, b1, stream()) == 0, W.lib().mdx_last_error()
    torch.cuda.synchronize()
    return dbuf, doffs, pbuf, poffs, (t2, b2)


def _red_expect(case, r, got_bits, off):
    """one record's destination against the float64 sum; the columns beyond `cols` keep the sentinel"""
    rows, cols, ld = r['rows'], r['cols'], r['ld']
    got = got_bits[off:off + rows * ld].reshape(rows, ld)
    assert (got[:, cols:] == SENT).all(), (case, 'wrote beyond its columns')
    p64 = r['planes'].astype(np.float64)
    s, sabs = p64.sum(0).reshape(rows, cols), np.abs(p64).sum(0).reshape(rows, cols)
    init = np.zeros((rows, cols)) if r['store'] else r['init'].astype(np.float64)
    acc = ACC * (sabs + np.abs(init))
    _check(case, f'sum[rkind{r["rkind"]}{"=" if r["store"] else "+="}]', np.ascontiguousarray(got[:, :cols]).view(np.float32), init + s,
           acc + _container(r['rkind'], np.abs(s) + acc))


def _red_records(rot):
    g = U.rng(9100 + rot)
    recs = []
    for i, (rows, cols) in enumerate(RED_SHAPES):
        S, k = RED_S[(i + rot) % 6], (i + rot) % 4
        recs.append(dict(rows=rows, cols=cols, S=S, ld=cols + (3 if k & 1 else 0), store=bool(k & 2), rkind=(i + 2 * rot) % 3, extra=0,
                         planes=g.standard_normal((S, rows * cols)).astype(np.float32),
                         init=g.standard_normal((rows, cols)).astype(np.float32)))
    return recs


@pytest.mark.parametrize('rot', range(6))
def test_reduction_table_of_six_records_on_the_vector_and_the_scalar_path(rot):
    """one launch over six records (1, 1, 1, 1, 3 and 32 blocks; S, ld, add / store and rkind rotate over them with `rot`), three
    times: planes 16-byte aligned (the vector loads), planes an odd number of floats apart, and a base 4 bytes off -- the same sums in
    the same order, so the same bytes"""
    bits = {}
    for form in ('vec', 'odd', 'off4'):
        recs = _red_records(rot)
        dbuf, doffs, pbuf, poffs, (t2, b2) = _reduce(recs, form)
        assert not t2 and b2 == 0
        bits[form] = dbuf.cpu().numpy()
        owned = np.zeros(bits[form].size, dtype=bool)
        for r, o in zip(recs, doffs):
            case = f'red[rot{rot}-{form}-{r["rows"]}x{r["cols"]}-S{r["S"]}-ld{r["ld"]}]'
            _red_expect(case, r, bits[form], o)
            owned[o:o + r['rows'] * r['ld']] = True
        assert (bits[form][~owned] == SENT).all(), (rot, form, 'wrote outside every destination')
    _same_bytes(f'red[rot{rot}]', 'odd-stride==vector', bits['odd'], bits['vec'])
    _same_bytes(f'red[rot{rot}]', 'offset-base==vector', bits['off4'], bits['vec'])


@pytest.mark.parametrize('form', ['vec', 'odd', 'off4'])
@pytest.mark.parametrize('S,rows,cols', [(257, 5, 3), (513, 5, 3), (600, 5, 3), (257, 64, 64), (513, 64, 64), (600, 64, 64)])
def test_chunked_record_takes_two_stages(S, rows, cols, form):
    """S > 256: the first table (a small plain record in front, so the chunked one does not start at block 0) leaves chunk c's sum in
    plane S + c of the partial area and touches nothing else; the second table sums those planes into the destination"""
    g = U.rng(9300 + S + cols)
    nc, total = W.ceil_div(S, W.RED_CHUNK), rows * cols
    front = dict(rows=1, cols=3, S=2, ld=3, store=False, rkind=0, extra=0, planes=g.standard_normal((2, 3)).astype(np.float32),
                 init=g.standard_normal((1, 3)).astype(np.float32))
    rec = dict(rows=rows, cols=cols, S=S, ld=cols + 3, store=False, rkind=2, extra=nc + 1,      # one plane more than the stage needs
               planes=g.standard_normal((S, total)).astype(np.float32), init=g.standard_normal((rows, cols)).astype(np.float32))
    recs = [front, rec]
    dbuf, doffs, pbuf, poffs, (t2, b2) = _reduce(recs, form)
    case = f'chunked[S{S}-{rows}x{cols}-{form}]'
    ps, po = rec['pstride'], poffs[1]
    pb = pbuf.cpu().numpy()
    inp = pb[po:po + S * ps].view(np.float32).reshape(S, ps)[:, :total]
    _same_bytes(case, 'partials-untouched', np.ascontiguousarray(inp), rec['planes'])
    p64 = rec['planes'].astype(np.float64)
    for c in range(nc):
        plane = pb[po + W.chunk_plane(S, c) * ps:po + W.chunk_plane(S, c) * ps + ps]
        assert (plane[total:] == SENT).all(), (case, c, 'chunk sum wrote past rows * cols')
        ch = p64[c * 256:(c + 1) * 256]
        _check(case, f'plane{S}+{c}', plane[:total].view(np.float32), ch.sum(0), ACC * np.abs(ch).sum(0))
    assert (pb[po + (S + nc) * ps:po + (S + nc + 1) * ps + GUARD] == SENT).all(), (case, 'wrote beyond plane S + nc - 1')
    d1 = dbuf.cpu().numpy()
    dr = d1[doffs[1]:doffs[1] + rows * rec['ld']].view(np.float32).reshape(rows, rec['ld'])[:, :cols]
    _same_bytes(case, 'dst-untouched-by-stage-1', np.ascontiguousarray(dr), rec['init'])
    _red_expect(case, front, d1, doffs[0])
    # second stage
    assert len(t2) == 8 and t2[2] == nc and t2[0] == rec['P'] + 4 * S * ps and b2 == W.red_blocks(total)
    dt2 = _table(t2)
    assert W.lib().mdx_op_reduce_deferred(dt2.data_ptr(), 1, b2, stream()) == 0, W.lib().mdx_last_error()
    torch.cuda.synchronize()
    d2 = dbuf.cpu().numpy()
    _red_expect(case, rec, d2, doffs[1])
    owned = np.zeros(d2.size, dtype=bool)
    owned[doffs[1]:doffs[1] + rows * rec['ld']] = True
    assert np.array_equal(d2[~owned], d1[~owned]), (case, 'the second stage wrote outside its destination')


@pytest.mark.parametrize('M,N,K,dt,bias', [(1, 128, 128, 3, False), (645, 64, 64, 3, True), (200, 54, 6, 1, True), (64 * 255 + 1, 8, 4, 0, True),
                                           (64 * 300 - 7, 8, 4, 0, True), (64 * 513, 4, 1, 0, True)])
def test_deferred_sum_is_the_per_call_reduction_bit_for_bit(M, N, K, dt, bias):
    """include/moldiff_hip.h: `Same fixed summation order as the per-layer reduction kernels`.  mdx_op_xgemm_tn_t with a dW reduces
    its partials itself (one stage up to 256 of them, two beyond); the deferred reduction of a copy of those partials, stored with
    rkind 0, must give the same bytes."""
    g = U.rng(9500 + M + N)
    gs, gp, ldg, _ = _operand(g, M, N, dt & 1, 'tight')
    xs, xp, ldx, _ = _operand(g, M, K, (dt >> 1) & 1, 'tight')
    p = W.plan(M, N, K, BIG, dt, ldg, ldx, 1)
    S = p['S']
    assert W.per_call_layout(M, N, K, BIG) == (S, p['mper'], p['boff'])
    part = _sentinel((p['psize'] + 3) // 4 * 4)
    dw, db = _sentinel(N * K), _sentinel(N)
    rc = W.lib().mdx_op_xgemm_tn_t(gp, ldg, xp, ldx, dw.data_ptr(), K, db.data_ptr() if bias else None, M, N, K, BIG, part.data_ptr(), 2, 0, dt,
                                   stream())
    assert rc == 0, W.lib().mdx_last_error()
    torch.cuda.synchronize()
    host = part.cpu().numpy()
    copy = _sentinel(host.size)
    copy[:S * N * K] = part[:S * N * K]
    copy[p['boff']:p['boff'] + S * N] = part[p['boff']:p['boff'] + S * N]
    out_w, out_b = _sentinel(N * K), _sentinel(N)
    recs = [dict(P=copy.data_ptr(), dst=out_w.data_ptr(), S=S, rows=N, cols=K, ld=K, pstride=N * K, rkind=0, store=True)]
    if bias:
        recs.append(dict(P=copy.data_ptr() + 4 * p['boff'], dst=out_b.data_ptr(), S=S, rows=1, cols=N, ld=N, pstride=N, rkind=0, store=True))
    (t1, b1), (t2, b2) = W.red_tables(recs)
    assert bool(t2) == (S > W.RED_CHUNK)
    for t, b in ((t1, b1), (t2, b2)):
        if t:
            d = _table(t)
            assert W.lib().mdx_op_reduce_deferred(d.data_ptr(), len(t) // 8, b, stream()) == 0, W.lib().mdx_last_error()
            torch.cuda.synchronize()
    case = f'order[{M}x{N}x{K}-S{S}]'
    assert (dw.cpu().numpy() != SENT).all()
    _same_bytes(case, 'dW==per-call', out_w.cpu().numpy(), dw.cpu().numpy())
    if bias:
        _same_bytes(case, 'db==per-call', out_b.cpu().numpy(), db.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) grouped launch -> deferred reduction -> a float16-valued slot that already holds a value
# ---------------------------------------------------------------------------------------------------------------------------------
E2E = [Case(0, 256, 128, 645, BIG, 3, 'slice', True, True), Case(1, 128, 192, 903, BIG, 3, 'tight', True, True),
       Case(2, 64, 128, 645, BIG, 3, 'slice', True, True), Case(3, 192, 64, 645, BIG, 3, 'tight', True, True),
       Case(4, 54, 6, 645, BIG, 1, 'off1', True, True), Case(5, 32, 64, 645, BIG, 3, 'slice', True, False),
       Case(6, 64, 32, 903, BIG, 3, 'tight', True, False), Case(7, 1, 256, 645, BIG, 3, 'slice', True, False),
       Case(7, 32, 1, 645, BIG, 1, 'tight', True, False)]


@pytest.mark.parametrize('case', E2E, ids=_name)
def test_queue_to_gradient_slot(case):
    """what flush_wgrads drives, one contraction at a time: the partials of a grouped launch summed, rounded to float16 and ADDED to
    a weight's slot (a column slice of a wider parameter: ld > K) and a bias's slot"""
    c = case
    jobs, area = _run_grouped(c.kind, [c], 'e2e')
    j = jobs[0]
    p, N, K = j['plan'], c.N, c.K
    g = U.rng(9700 + c.kind + N)
    recs = [dict(rows=N, cols=K, S=p['S'], ld=K + 5, store=False, rkind=2, init=g.standard_normal((N, K)).astype(np.float32)),
            dict(rows=1, cols=N, S=p['S'], ld=N, store=False, rkind=2, init=g.standard_normal((1, N)).astype(np.float32))]
    dbuf, doffs = _dst(recs)
    recs[0].update(P=j['P'], pstride=N * K, dst=dbuf.data_ptr() + 4 * doffs[0])
    recs[1].update(P=j['P'] + 4 * p['boff'], pstride=N, dst=dbuf.data_ptr() + 4 * doffs[1])
    (t1, b1), (t2, b2) = W.red_tables(recs)
    assert not t2 and b1 == W.red_blocks(N * K) + W.red_blocks(N)
    d = _table(t1)
    assert W.lib().mdx_op_reduce_deferred(d.data_ptr(), 2, b1, stream()) == 0, W.lib().mdx_last_error()
    torch.cuda.synchronize()
    bits = dbuf.cpu().numpy()
    prod, aprod, col, acol = W.partials_ref(j['g64'], j['x64'], c.M, p['mper'], p['S'])
    tag = f'e2e:{_name(c)}'
    for r, o, s, sabs, name in ((recs[0], doffs[0], prod.sum(0), aprod.sum(0), 'dW'), (recs[1], doffs[1], col.sum(0)[None], acol.sum(0)[None], 'db')):
        got = bits[o:o + r['rows'] * r['ld']].reshape(r['rows'], r['ld'])
        assert (got[:, r['cols']:] == SENT).all(), (tag, name, 'wrote beyond its columns')
        init = r['init'].astype(np.float64)
        acc = ACC * (sabs + np.abs(init))
        _check(tag, name, np.ascontiguousarray(got[:, :r['cols']]).view(np.float32), init + s, acc + _container(2, np.abs(s) + acc))
    owned = np.zeros(bits.size, dtype=bool)
    for r, o in zip(recs, doffs):
        owned[o:o + r['rows'] * r['ld']] = True
    assert (bits[~owned] == SENT).all(), (tag, 'wrote outside both slots')


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) refusals and empties
# ---------------------------------------------------------------------------------------------------------------------------------
def test_empty_tables_launch_nothing_and_bad_ones_are_refused():
    L = W.lib()
    c = Case(3, 64, 64, 65, BIG, 3, 'tight', True, True)
    jobs, size = _jobs(3, [c])
    area = _sentinel(size)
    jobs[0]['P'] = area.data_ptr() + 4 * jobs[0]['off']
    flat, total = W.grouped_table(jobs)
    desc = _table(flat)
    dst = _sentinel(64 * 64 + GUARD)
    rec, nb = W.red_record(jobs[0]['P'], dst.data_ptr(), 2, 64, 64, 64, 64 * 64, 0, 0, store=True)
    rdesc = _table(rec)

    def untouched():
        torch.cuda.synchronize()
        return bool((area == SENT).all()) and bool((dst == SENT).all())
    assert L.mdx_op_wgrad_grouped(desc.data_ptr(), 0, total, 3, stream()) == 0 and untouched()
    assert L.mdx_op_wgrad_grouped(desc.data_ptr(), 1, 0, 3, stream()) == 0 and untouched()
    assert L.mdx_op_reduce_deferred(rdesc.data_ptr(), 0, nb, stream()) == 0 and untouched()
    assert L.mdx_op_reduce_deferred(rdesc.data_ptr(), 1, 0, stream()) == 0 and untouched()
    assert L.mdx_op_wgrad_grouped(None, 1, total, 3, stream()) == 1 and b'wgrad_grouped: null record table' in L.mdx_last_error()
    assert L.mdx_op_reduce_deferred(None, 1, nb, stream()) == 1 and b'reduce_deferred: null record table' in L.mdx_last_error()
    assert untouched()
    for kind in (8, -1):
        assert L.mdx_op_wgrad_grouped(desc.data_ptr(), 1, total, kind, stream()) == 1 and b'wgrad_grouped: kind must be 0..7' in L.mdx_last_error()
    assert untouched()
