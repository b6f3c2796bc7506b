"""Helpers of tests/test_wgrad_queue_host.py and tests/test_gpu_wgrad_queue.py: the two record tables of the weight-gradient queue as
csrc/mdx_fast.cpp (flush_wgrads, sink_record) lays them out, the block -> (row range, tile) map of wgrad_grouped_kernel restated in
Python, and the float64 partials of one contraction.  Nothing here needs a GPU: the library's host entry points and numpy only."""
import ctypes
import os

import numpy as np

LIB = os.path.join(os.path.dirname(__file__), '..', 'moldiff_amd', 'libmoldiff_hip.so')
RED_CHUNK, RED_ELEMS, HW_MC = 256, 128, 64      # csrc/mdx_train_plan.h
PLAN_KEYS = ('kind', 'gx', 'gy', 'S', 'mper', 'boff', 'psize', 'blocks')
_lib = None


def lib():
    """the shared library with the argtypes of the queue's entry points bound (moldiff_amd/_lib.py declares only what Python calls)"""
    global _lib
    if _lib is None:
        L = ctypes.CDLL(LIB)
        c64, c32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
        L.mdx_last_error.restype = ctypes.c_char_p
        L.mdx_op_wgrad_plan.argtypes = [c64, c64, c64, c32, c32, c64, c64, c32, ctypes.POINTER(c64)]
        L.mdx_op_wgrad_layout.argtypes = [c64, c64, c64, c32, c32, ctypes.POINTER(c64), ctypes.POINTER(c64)]
        L.mdx_op_wgrad_grouped.argtypes = [vp, c32, c64, c32, vp]
        L.mdx_op_reduce_deferred.argtypes = [vp, c32, c64, vp]
        L.mdx_op_xgemm_tn_t.argtypes = [vp, c64, vp, c64, vp, c64, vp, c64, c64, c64, c32, vp, c32, c32, c32, vp]
        _lib = L
    return _lib


def ceil_div(a, b):
    return (a + b - 1) // b


def plan(M, N, K, splits, dt, ldg, ldx, aligned):
    out = (ctypes.c_int64 * 8)()
    rc = lib().mdx_op_wgrad_plan(M, N, K, splits, dt, ldg, ldx, int(bool(aligned)), out)
    assert rc == 0, lib().mdx_last_error()
    return dict(zip(PLAN_KEYS, (int(v) for v in out)))


def per_call_layout(M, N, K, splits):
    """(S, mper, bias offset) of mdx_op_xgemm_tn_t's half-precision kernels for the same call"""
    S, boff = ctypes.c_int64(), ctypes.c_int64()
    assert lib().mdx_op_wgrad_layout(M, N, K, splits, 1, ctypes.byref(S), ctypes.byref(boff)) == 0
    mper = ceil_div(ceil_div(max(M, 1), max(splits, 1)), HW_MC) * HW_MC
    return int(S.value), mper, int(boff.value)


# ---- the grouped table (flush_wgrads) -------------------------------------------------------------------------------------------------
def grouped_record(G, X, P, Pb, ldg, ldx, M, N, K, p, dt, first_block):
    """16 x int64 {dY, X, P, Pb, ldg, ldx, M, N, K, mper, gx, gy, S, dt, first_block, 0}; G, X, P, Pb are addresses, p a plan()"""
    return [G, X, P, Pb, ldg, ldx, M, N, K, p['mper'], p['gx'], p['gy'], p['S'], dt, first_block, 0]


def grouped_table(jobs):
    """jobs: dicts(G, X, P, bias, ldg, ldx, M, N, K, dt, plan) -> (flat int64 list, total blocks).  Pb = P + 4 * boff where the job
    wants its bias partials, else 0; first_block is the running sum of the jobs' blocks."""
    flat, fb = [], 0
    for j in jobs:
        p = j['plan']
        flat += grouped_record(j['G'], j['X'], j['P'], j['P'] + 4 * p['boff'] if j['bias'] else 0, j['ldg'], j['ldx'], j['M'], j['N'], j['K'],
                               p, j['dt'], fb)
        fb += p['blocks']
    return flat, fb


def deal(rel, gx, gy, S):
    """block `rel` of a record -> (row range bz, k tile bx, n tile by): chunks of 8 row ranges, inside a chunk id i works on row range
    i % w and tile i / w, w = the chunk's row ranges (8, or what is left in the last one)"""
    T = gx * gy
    chunk, i = divmod(rel, 8 * T)
    w = min(8, S - 8 * chunk)
    bz, t = 8 * chunk + i % w, i // w
    return bz, t % gx, t // gx


# ---- the reduction tables (sink_record) -----------------------------------------------------------------------------------------------
def red_blocks(elems):
    return ceil_div(elems, RED_ELEMS)


def red_record(P, dst, S, rows, cols, ld, pstride, rkind, first_block, chunked=False, store=False):
    """8 x int64 {P, dst, S, rows, cols, ld, pstride, rkind | chunked << 6 | store << 7 | first_block << 8} -> (record, its blocks)"""
    nch = ceil_div(S, RED_CHUNK) if chunked else 1
    return [P, dst, S, rows, cols, ld, pstride, rkind | (int(chunked) << 6) | (int(store) << 7) | (first_block << 8)], nch * red_blocks(rows * cols)


def chunk_plane(S, c):
    return S + c


def red_tables(records):
    """records: dicts(P, dst, S, rows, cols, ld, pstride, rkind, store) -> ((table 1, blocks), (table 2, blocks)) as sink_record fills
    them: more than RED_CHUNK partials give a chunked record in the first table and a plain one over the chunk sums in the second."""
    t1, b1, t2, b2 = [], 0, [], 0
    for r in records:
        store = bool(r.get('store', False))
        if r['S'] > RED_CHUNK:
            nc = ceil_div(r['S'], RED_CHUNK)
            rec, nb = red_record(r['P'], r['dst'], r['S'], r['rows'], r['cols'], r['ld'], r['pstride'], 0, b1, chunked=True)
            t1, b1 = t1 + rec, b1 + nb
            rec, nb = red_record(r['P'] + 4 * chunk_plane(r['S'], 0) * r['pstride'], r['dst'], nc, r['rows'], r['cols'], r['ld'], r['pstride'],
                                 r['rkind'], b2, store=store)
            t2, b2 = t2 + rec, b2 + nb
        else:
            rec, nb = red_record(r['P'], r['dst'], r['S'], r['rows'], r['cols'], r['ld'], r['pstride'], r['rkind'], b1, store=store)
            t1, b1 = t1 + rec, b1 + nb
    return (t1, b1), (t2, b2)


# ---- float64 reference ----------------------------------------------------------------------------------------------------------------
def partials_ref(G, X, M, mper, S):
    """G (M,N), X (M,K) float64 -> per row range z: G[z]^T X[z] (S,N,K), sum |terms| of it (S,N,K), column sums of G[z] (S,N) and
    their sum |terms| (S,N).  A range past the last row is all zeros."""
    G, X = np.asarray(G, dtype=np.float64), np.asarray(X, dtype=np.float64)
    N, K = G.shape[1], X.shape[1]
    prod, aprod = np.zeros((S, N, K)), np.zeros((S, N, K))
    col, acol = np.zeros((S, N)), np.zeros((S, N))
    for z in range(S):
        g, x = G[z * mper:min(M, (z + 1) * mper)], X[z * mper:min(M, (z + 1) * mper)]
        prod[z], aprod[z] = g.T @ x, np.abs(g).T @ np.abs(x)
        col[z], acol[z] = g.sum(0), np.abs(g).sum(0)
    return prod, aprod, col, acol
