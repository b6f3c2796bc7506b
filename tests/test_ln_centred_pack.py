"""Host-only checks of the centred weight packs (csrc/mdx_pack.cpp centre_columns).  No GPU.

A Linear W x + b that feeds a LayerNorm over its F output features is packed with the column means of W and the mean of b taken out
(float64, rounded to float32 once), so that the pre-activation has mean zero over the features and the kernels' LayerNorm skips the
mean (csrc/mdx_row.h row_layernorm_centred).

What the rounding leaves.  Every centred entry is off by at most half an ulp, 2^-24 |w|, so column k keeps a residual mean of at most
r_k = 2^-24 max_f |Wc[f, k]| -- asserted below for every centred layer of the recipe and of the stress weights, and by the pack code
itself at upload.  The pre-activation's residual mean is then at most  sum_k r_k |x_k| <= K 2^-24 max|Wc| max|x|,  which is the size of
the rounding error of ONE fp32 dot product of that layer (K products of relative error 2^-24 each): the centred LayerNorm sees a mean
no larger than the noise the two-pass LayerNorm's inputs already carry.  It enters the variance squared, relative to var + 1e-5.
Numbers (printed by test_bound_of_the_shipped_weights).  Recipe weights: K = 64 .. 321, max|Wc| <= 0.52, worst residual column mean
2.2e-9; the pre-activation's residual mean is at most 5.0e-6 max|x| (all signs aligned; ~K^-1/2 of that typically), i.e. <= 5e-5 for
activations up to 10, squared 2.5e-9 against var + 1e-5.  Stress weights: the same matrices (the stress recipe scales biases x 8 and
LayerNorm gains up to 30, which centring does not touch: bias residuals <= 7.4e-9), but un-normalised products up to 3.7e4 enter the
K = 128 / 256 inter layers: residual mean <= 5.0e-6 * 3.7e4 = 0.19 on rows whose entries are sums of such products (variance of
order 1e8) -- the same 2^-24 relative to the size of the terms being summed that their fp32 accumulation loses anyway.
"""
import numpy as np
import pytest
import torch

from moldiff_amd import _lib
from tests import util as U

EPS = 2.0 ** -24


def _centred_layers(P):
    """(weight key, bias key) of every Linear the edge kernels read from a centred pack"""
    out = []
    nb = len({k.split('.')[2] for k in P if k.startswith('denoiser.edge_embs.')})
    for i in range(nb):
        n, e, p = (f'denoiser.{s}.{i}' for s in ('node_blocks_with_edge', 'edge_blocks', 'pos_blocks'))
        pres = [n + '.gate.net.0', n + '.edge_net.net.0']
        for side in ('left', 'right'):
            pres += [f'{e}.bond_ffn_{side}.gate.net.0', f'{e}.bond_ffn_{side}.inter_module.net.0']
        pres += [p + '.edge_lin.gate.net.0', p + '.edge_lin.inter_module.net.0']
        out += [(q + '.weight', q + '.bias') for q in pres]
    return out


def _check(W):
    W = W.detach().cpu().float()
    Wc, worst = _lib.centre_host(W)
    w64 = W.double().numpy()
    want = (w64 - w64.mean(axis=0, keepdims=True)).astype(np.float32)
    got = Wc.numpy()
    # float64 sums of <= 256 floats differ from numpy's pairwise order by ~1e-16 relative: the rounded float32 can differ in its last bit
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.abs(want) * 2 * EPS + 1e-45)
    res = np.abs(got.astype(np.float64).mean(axis=0))
    bound = EPS * np.abs(got).max(axis=0).astype(np.float64)
    assert np.all(res <= bound), float((res / np.maximum(bound, 1e-300)).max())
    assert worst <= 1.0
    return float(np.abs(got).max()), float(res.max())


@pytest.mark.parametrize('weights', ['recipe', 'stress'])
def test_bound_of_the_shipped_weights(weights):
    m = U.moldiff('MolDiff_simple') if weights == 'recipe' else U.moldiff_stress('cpu', 'MolDiff_simple')
    P = U.params(m)
    layers = _centred_layers(P)
    assert len(layers) == 8 * 6
    for wk, bk in layers:
        wmax, res = _check(P[wk])
        bmax, bres = _check(P[bk].reshape(-1, 1))
        K = P[wk].shape[1]
        print(f'{weights} {wk}: F x K = {tuple(P[wk].shape)}, max|Wc| {wmax:.3g}, worst residual column mean {res:.3g}, '
              f'pre-activation residual mean <= K 2^-24 max|Wc| max|x| = {K * EPS * wmax:.3g} max|x|; bias {bmax:.3g} / {bres:.3g}')


def test_random_and_degenerate_matrices():
    g = U.rng(5)
    for F, K, scale in ((32, 129, 1.0), (256, 321, 30.0), (128, 128, 1e-3), (256, 1, 8.0)):
        _check(U.t32(g.standard_normal((F, K)) * scale + g.standard_normal((1, K)) * 5 * scale))
    z, worst = _lib.centre_host(torch.zeros(32, 64))     # pass-through gates (all-zero layers) stay all zero
    assert worst == 0.0 and not z.any()
    c, worst = _lib.centre_host(torch.full((32, 4), 3.25))  # a constant column centres to exactly zero
    assert worst == 0.0 and not c.any()


# ---- the packed arena itself (mdx_debug_pack_host): which packs pack_model centred, and that nothing else moved -----------------------
#
# Every pack is decoded from its fragment order back to a matrix (layouts: csrc/mdx_pack.cpp Packer::pack, the two
# index maps and two element formats).  Split packs hold w as fp16 hi + fp16 lo 2^-11: re-rounding a centred fp32 entry costs at most
# 2^-11 of |w - hi| <= 2^-11 |w|, i.e. 2^-22 |w| (plus 2^-35 where lo is an fp16 subnormal), so a split pack's residual column mean
# is bounded by (2^-24 + 2^-22) max|w| + 2^-35, not by 2^-24 max|w|.

def _dec_dense(a, F, K):
    FT, G = (F + 15) // 16, K // 16
    return a[:G * FT * 256].reshape(G, FT, 4, 16, 4).transpose(1, 3, 0, 2, 4).reshape(16 * FT, 16 * G)


def _dec_stream(a, F, K):
    FTP, KG = (F + 31) // 32, K // 16
    assert not a[FTP * KG * 512:].any()          # the ring's zero tail
    return a[:FTP * KG * 512].reshape(FTP, KG, 2, 4, 16, 4).transpose(0, 2, 4, 1, 3, 5).reshape(32 * FTP, 16 * KG)


def _halves(h):
    hi, lo = h[0].view(np.float16).astype(np.float64), h[1].view(np.float16).astype(np.float64)
    return hi + lo / 2048.0, h


def _dec_stream_split(a, F, K):
    FTP, KG = (F + 31) // 32, (K + 31) // 32
    assert not a[FTP * KG * 1024:].any()
    h = a[:FTP * KG * 1024].view(np.uint16).reshape(FTP, KG, 2, 2, 4, 16, 2, 4)    # ftp g h j q c t4 tr
    return _halves(h.transpose(2, 0, 3, 5, 1, 6, 4, 7).reshape(2, 32 * FTP, 32 * KG))


def _dec_dense_split(a, F, K):
    FT, G = (F + 15) // 16, (K + 31) // 32
    h = a[:G * FT * 512].view(np.uint16).reshape(G, FT, 2, 4, 16, 2, 4)              # g ft h q c t4 tr
    return _halves(h.transpose(2, 1, 4, 0, 5, 3, 6).reshape(2, 16 * FT, 32 * G))


def _split_bits(W):
    """hi / lo halves of an fp32 matrix as the pack code forms them"""
    W = W.astype(np.float32)
    hi = W.astype(np.float16)
    lo = ((W - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return np.stack([hi.view(np.uint16), lo.view(np.uint16)])


def _pad(W, rows, cols):
    out = np.zeros((rows, cols), dtype=W.dtype)
    out[:W.shape[0], :W.shape[1]] = W
    return out


def _engine_params(kind):
    """(an un-finalized handle with the model's parameters set, the parameter dict under the handle's keys)"""
    from moldiff_amd.graph import synth_gates
    if kind == 'moldiff':
        m = U.moldiff('MolDiff')
        d = m.denoiser
        eng = _lib.Model(_lib.MDX_KIND_MOLDIFF, num_blocks=d.num_blocks, cutoff=d.cutoff, update_pos=d.update_pos,
                         time_dim=m.config.diff.time_dim, num_timesteps=m.num_timesteps, num_node_types=m.num_node_types,
                         num_edge_types=m.num_edge_types, node_dim=d.node_dim, edge_dim=d.edge_dim, num_gaussians=16)
        sd = {**m.state_dict(), **synth_gates(d, 'denoiser.')}
    elif kind == 'bondpred':
        m = U.bondpred()
        e = m.encoder
        eng = _lib.Model(_lib.MDX_KIND_BONDPRED, num_blocks=e.num_blocks, cutoff=e.cutoff, update_pos=False, time_dim=m.time_dim,
                         num_timesteps=m.num_timesteps, num_node_types=m.num_node_types, num_edge_types=m.num_edge_types,
                         node_dim=e.node_dim, edge_dim=e.edge_dim, num_gaussians=16)
        sd = {**m.state_dict(), **synth_gates(e, 'encoder.')}
    else:  # the bare network handle of the block-level modules
        d = U.moldiff('MolDiff').denoiser
        eng = _lib.Model(_lib.MDX_KIND_NET, num_blocks=d.num_blocks, cutoff=d.cutoff, update_pos=d.update_pos, node_dim=d.node_dim,
                         edge_dim=d.edge_dim, num_gaussians=16)
        sd = {**d.state_dict(), **synth_gates(d)}
    eng.set_params(sd)
    return eng, {k: v.detach().cpu().float().numpy() for k, v in sd.items() if v.is_floating_point()}


_packs = {}


def _pack(kind, on):
    if (kind, on) not in _packs:
        eng, P = _engine_params(kind)
        _packs[kind, on] = _lib.pack_host(eng, on) + (P,)
    return _packs[kind, on]


def _wcat(P, net, i, centre):
    """the node kernel's concatenated table weights (960 x 256) of block i, rows of the three gates centred or as stored"""
    nb, eb = f'{net}node_blocks_with_edge.{i}', f'{net}edge_blocks.{i}'
    gate = lambda k: (_lib.centre_host(P[k])[0].numpy() if centre else P[k])[:, 64:320]
    return np.concatenate([P[nb + '.centroid_lin.weight'], gate(nb + '.gate.net.0.weight'),
                           P[eb + '.bond_ffn_left.node_linear.weight'], P[eb + '.bond_ffn_right.node_linear.weight'],
                           P[eb + '.node_ffn_left.weight'], P[eb + '.node_ffn_right.weight'],
                           gate(eb + '.bond_ffn_left.gate.net.0.weight'), gate(eb + '.bond_ffn_right.gate.net.0.weight')])


def _source(sl, P, net):
    """the fp32 matrix (or vector) a named slot must hold: the stored parameter, or its centred copy for a centred slot"""
    key = sl['key']
    if key.startswith('wcat.'):
        return _wcat(P, net, int(key[5:]), sl['centred'])
    W = P[key]
    if sl['centred']:
        if W.ndim == 1:
            W = _lib.centre_host(W.reshape(-1, 1))[0].numpy().reshape(-1)
        else:
            W = _lib.centre_host(W)[0].numpy()
    if sl['kind'] == 'v':
        return W if W.ndim == 1 else W[:, sl['col0']]
    W = W[:, sl['col0']:sl['col0'] + (sl['F'] if sl['transposed'] else sl['K'])]
    return np.ascontiguousarray(W.T) if sl['transposed'] else W


def _check_slots(kind, on, net):
    """every named pack of the arena holds exactly its source, the packs tile the arena, and the rest is zero padding"""
    arena, slots, P = _pack(kind, on)
    covered = np.zeros(arena.size, dtype=bool)
    for sl in slots:
        seg = arena[sl['off']:sl['off'] + sl['n']]
        assert not covered[sl['off']:sl['off'] + sl['n']].any(), sl
        covered[sl['off']:sl['off'] + sl['n']] = True
        if sl['key'] is None:
            continue
        src = _source(sl, P, net)
        if sl['kind'] == 'v':
            assert np.array_equal(seg[:src.size].view(np.uint32), src.astype(np.float32).view(np.uint32)), sl
            assert not seg[src.size:].any(), sl
        elif sl['kind'] in 'ds':
            got = (_dec_dense if sl['kind'] == 'd' else _dec_stream)(seg, sl['F'], sl['K'])
            assert np.array_equal(got.view(np.uint32), _pad(src.astype(np.float32), *got.shape).view(np.uint32)), sl
        else:
            _, bits = (_dec_dense_split if sl['kind'] == 'D' else _dec_stream_split)(seg, sl['F'], sl['K'])
            assert np.array_equal(bits, _split_bits(_pad(src, *bits.shape[1:]))), sl
    assert not arena[~covered].any()
    return arena, slots, P


def _expected_centred(nblocks):
    want = set()
    for i in range(nblocks):
        n, e, p = (f'denoiser.{s}.{i}' for s in ('node_blocks_with_edge', 'edge_blocks', 'pos_blocks'))
        gates = [(n + '.gate.net.0', 320, (0,)), (e + '.bond_ffn_left.gate.net.0', 320, (0,)), (e + '.bond_ffn_right.gate.net.0', 320, (0,)),
                 (p + '.edge_lin.gate.net.0', 128, (0, 64))]
        for pre, tcol, cols in gates:       # streamed column ranges, the time column, the bias
            want |= {(k, pre + '.weight', c) for k in 'sS' for c in cols} | {('v', pre + '.weight', tcol), ('v', pre + '.bias', 0)}
        for pre in (n + '.edge_net.net.0', e + '.bond_ffn_left.inter_module.net.0', e + '.bond_ffn_right.inter_module.net.0',
                    p + '.edge_lin.inter_module.net.0'):
            want |= {('s', pre + '.weight', 0), ('S', pre + '.weight', 0), ('v', pre + '.bias', 0)}
        want |= {('d', f'wcat.{i}', 0), ('D', f'wcat.{i}', 0)}      # the gates' node parts: rows GX, GXL, GXR of the table GEMM
    return want


def test_uncentred_packs_hold_the_stored_weights_bit_for_bit():
    """Centring off, and every handle kind: each named pack decodes to the stored parameter it is cut from, bit for bit -- the pack a
    build without centred packs makes."""
    for kind, net in (('moldiff', 'denoiser.'), ('bondpred', 'encoder.'), ('net', '')):
        arena, slots, _ = _check_slots(kind, False, net)
        assert not any(sl['centred'] for sl in slots), kind


def test_predictor_and_network_handles_are_never_centred():
    for kind in ('bondpred', 'net'):
        a0, s0, _ = _pack(kind, False)
        a1, s1, _ = _pack(kind, True)
        assert s0 == s1 and np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), kind


def test_centred_handle_differs_in_the_listed_packs_only_and_those_are_centred():
    a0, s0, P = _pack('moldiff', False)
    a1, s1, _ = _check_slots('moldiff', True, 'denoiser.')       # centred slots hold centre_host(stored weights), bit for bit
    geom = lambda s: [(x['kind'], x['off'], x['n'], x['F'], x['K'], x['col0'], x['transposed'], x['key']) for x in s]
    assert geom(s0) == geom(s1)
    got = {(sl['kind'], sl['key'], sl['col0']) for sl in s1 if sl['centred']}
    assert got == _expected_centred(6), (sorted(got - _expected_centred(6)), sorted(_expected_centred(6) - got))
    GATE_ROWS = np.r_[256:512, 896:960]
    for sl in s1:
        x0, x1 = (a[sl['off']:sl['off'] + sl['n']] for a in (a0, a1))
        if not sl['centred']:
            assert np.array_equal(x0.view(np.uint32), x1.view(np.uint32)), sl
            continue
        F, K = sl['F'], sl['K']
        if sl['kind'] == 'v':
            cols, slack = x1[:F].astype(np.float64).reshape(F, 1), EPS
        elif sl['kind'] in 'ds':
            cols, slack = (_dec_dense if sl['kind'] == 'd' else _dec_stream)(x1, F, K).astype(np.float64)[:F], EPS
        else:
            cols, slack = (_dec_dense_split if sl['kind'] == 'D' else _dec_stream_split)(x1, F, K)[0][:F], EPS + 2.0 ** -22
        if sl['key'].startswith('wcat.'):
            dec = _dec_dense if sl['kind'] == 'd' else (lambda a, F, K: _dec_dense_split(a, F, K)[0])
            w0 = np.asarray(dec(x0, F, K), dtype=np.float64)
            other = np.setdiff1d(np.arange(960), GATE_ROWS)
            assert np.array_equal(w0[other], cols[other]), sl          # only the gates' rows of the table moved
            groups = [cols[256:512], cols[896:928], cols[928:960]]
        else:
            groups = [cols]
        for g in groups:
            res, bound = np.abs(g.mean(axis=0)), slack * np.abs(g).max(axis=0) + 2.0 ** -35
            assert np.all(res <= bound), (sl, float((res / bound).max()))
