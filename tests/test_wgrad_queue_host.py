"""The host side of the weight-gradient queue's tests (tests/wgrad_cases.py), checked without a GPU so that what
tests/test_gpu_wgrad_queue.py expects of the kernels is itself right: the block -> (row range, tile) map is a bijection, the record
builders agree with mdx_op_wgrad_plan, and a chunked record's chunk-sum planes lie inside the partial area the plan reserves."""
import os

import numpy as np
import pytest

from tests import wgrad_cases as W


@pytest.fixture(scope='module', autouse=True)
def _built():
    if not os.path.exists(W.LIB):
        pytest.skip('libmoldiff_hip.so not built (python -c "import __graft_entry__ as g; g.build()")')


@pytest.mark.parametrize('gx,gy', [(gx, gy) for gx in (1, 2, 3, 4) for gy in (1, 2)])
def test_dealing_is_a_bijection_and_keeps_a_row_range_on_one_xcd(gx, gy):
    """For S = 1..40: every (row range, tile) gets exactly one block.  Workgroup ids go round-robin over 8 XCDs, so the tiles of one
    row range should sit on ids that are equal mod 8.  A full chunk of 8 row ranges does that (a record starts at a multiple of 8 T
    plus its first_block; the property is about ids relative to the chunk's start, which is what the kernel comment claims).  The last
    chunk of w < 8 row ranges has w T consecutive ids for w T pairs, so with T > 1 no numbering can give a row range T ids of one
    residue mod 8 (a residue has at most ceil(w T / 8) < T of them): there the kernel deals `over what is left`, ids equal mod w."""
    T = gx * gy
    for S in range(1, 41):
        seen = {}
        for rel in range(T * S):
            bz, bx, by = W.deal(rel, gx, gy, S)
            assert 0 <= bz < S and 0 <= bx < gx and 0 <= by < gy, (S, rel)
            assert (bz, bx, by) not in seen, (S, rel, seen[(bz, bx, by)])
            seen[(bz, bx, by)] = rel
        assert len(seen) == T * S
        for bz in range(S):
            chunk = bz // 8
            w = min(8, S - 8 * chunk)
            ids = [seen[(bz, bx, by)] - chunk * 8 * T for bx in range(gx) for by in range(gy)]
            assert all(0 <= i < w * T for i in ids), (S, bz)                       # a row range's blocks stay inside their chunk
            assert len({i % w for i in ids}) == 1, (S, bz, ids)
            if w == 8:
                assert len({seen[(bz, bx, by)] % 8 for bx in range(gx) for by in range(gy)}) == 1, (S, bz)
            assert sorted(ids) == [bz - 8 * chunk + w * t for t in range(T)]      # close in dispatch order: w ids apart


SHAPES = [(1, 128, 128, 3), (645, 256, 128, 3), (903, 128, 192, 3), (513, 64, 128, 3), (1025, 192, 64, 3), (1024, 64, 64, 3), (65, 54, 6, 1),
          (513, 64, 16, 0), (1025, 256, 256, 3), (645, 32, 64, 3), (129, 64, 32, 3), (257, 1, 256, 3), (645, 32, 1, 0), (16448 + 5, 8, 4, 0)]


@pytest.mark.parametrize('splits', [1, 10 ** 6])
@pytest.mark.parametrize('shape', SHAPES)
def test_record_builders_reproduce_the_plan(shape, splits):
    M, N, K, dt = shape
    p = W.plan(M, N, K, splits, dt, N + 8, K + 8, 1)
    job = dict(G=1 << 20, X=2 << 20, P=3 << 20, bias=True, ldg=N + 8, ldx=K + 8, M=M, N=N, K=K, dt=dt, plan=p)
    other = dict(job, P=5 << 20, bias=False)
    flat, total = W.grouped_table([job, other])
    assert len(flat) == 32 and total == 2 * p['blocks']
    r0, r1 = flat[:16], flat[16:]
    assert r0[14] == 0 and r1[14] == p['blocks'] and r0[15] == 0
    assert r0[10] * r0[11] * r0[12] == p['blocks']                                 # gx gy S
    assert r0[3] == r0[2] + 4 * p['boff'] and r1[3] == 0
    assert (r0[12] - 1) * r0[9] < max(M, 1) <= r0[12] * r0[9]                      # the row ranges tile [0, M)
    # every block of the table maps to a row range and a tile of its record
    for rel in range(p['blocks']):
        bz, bx, by = W.deal(rel, p['gx'], p['gy'], p['S'])
        assert bz < p['S'] and bx < p['gx'] and by < p['gy']
    nc = W.ceil_div(p['S'], W.RED_CHUNK)
    assert p['boff'] == (p['S'] + nc) * N * K and p['psize'] == (p['S'] + nc) * (N * K + N)
    # the reduction records of the same job (flush_wgrads -> sink_record): weight, then bias
    recs = [dict(P=job['P'], dst=7 << 20, S=p['S'], rows=N, cols=K, ld=K, pstride=N * K, rkind=2),
            dict(P=job['P'] + 4 * p['boff'], dst=8 << 20, S=p['S'], rows=1, cols=N, ld=N, pstride=N, rkind=2)]
    (t1, b1), (t2, b2) = W.red_tables(recs)
    chunked = p['S'] > W.RED_CHUNK
    assert b1 == (nc if chunked else 1) * (W.red_blocks(N * K) + W.red_blocks(N))
    assert t1[7] >> 8 == 0 and t1[15] >> 8 == (nc if chunked else 1) * W.red_blocks(N * K)
    assert bool(t1[7] & 64) == chunked and bool(t1[15] & 64) == chunked
    if chunked:
        assert b2 == W.red_blocks(N * K) + W.red_blocks(N) and t2[2] == nc and t2[10] == nc
        assert t2[0] == job['P'] + 4 * p['S'] * N * K and t2[8] == job['P'] + 4 * (p['boff'] + p['S'] * N)
        assert t2[7] & 255 == 2 and t2[7] >> 8 == 0 and t2[15] >> 8 == W.red_blocks(N * K)
    else:
        assert not t2 and b2 == 0 and t1[7] & 63 == 2


@pytest.mark.parametrize('M,N,K', [(64 * 257, 8, 4), (64 * 513, 4, 1), (64 * 600 - 3, 1, 4), (64 * 256 + 1, 54, 6)])
def test_chunk_sum_planes_of_a_chunked_record_lie_inside_the_partial_area(M, N, K):
    p = W.plan(M, N, K, 10 ** 6, 0, N, K, 1)
    S, nc = p['S'], W.ceil_div(p['S'], W.RED_CHUNK)
    assert S > W.RED_CHUNK and p['mper'] == 64
    last_w = (W.chunk_plane(S, nc - 1) + 1) * N * K                               # one past the last chunk sum of the products
    assert S * N * K <= W.chunk_plane(S, 0) * N * K and last_w <= p['boff']       # behind the partials, before the bias partials
    last_b = p['boff'] + (W.chunk_plane(S, nc - 1) + 1) * N
    assert p['boff'] + S * N <= p['boff'] + W.chunk_plane(S, 0) * N and last_b <= p['psize']


def test_partials_ref_sums_to_the_whole_contraction():
    g = np.random.Generator(np.random.PCG64(5))
    G, X = g.standard_normal((200, 5)), g.standard_normal((200, 3))
    prod, aprod, col, acol = W.partials_ref(G, X, 200, 64, 5)                     # the fifth range is empty
    assert np.allclose(prod.sum(0), G.T @ X, rtol=0, atol=1e-12) and np.allclose(col.sum(0), G.sum(0), rtol=0, atol=1e-12)
    assert not prod[4].any() and not col[4].any() and (aprod >= np.abs(prod) - 1e-12).all() and (acol >= np.abs(col) - 1e-12).all()
    assert np.array_equal(prod[3], G[192:].T @ X[192:])
