"""The typed row operators of the training path (csrc/mdx_train_rows.hip and csrc/mdx_train.hip `mdx_op_*_t`, reached through moldiff_amd/train_ops.py) with float16
CONTAINERS, one operator at a time, against a float64 restatement of that operator on the same float16-representable inputs.

Rounding model of every bound below: the kernels compute in fp32 and round to nearest even ONCE into the container at each stated
rounding point.
  * a rounding point into float16 allows  2^-11 |ref| + 2^-25   (half an ulp; the second term covers subnormals),
  * an fp32 accumulation allows           2e-6 * sum |terms|    (the convention of tests/test_gpu_train_ops.py; sum |terms| in float64),
  * LayerNorm values / gradients take their fp32 term from the fp32 twin test (test_layernorm_relu): 5e-6 of the tensor's maximum for
    the forward, 2e-5 for dx, dgamma, dbeta; the container term is added where the output is float16.
Where the fp32 arithmetic is exact (a product of two float16 values has 22 significant bits) the result must EQUAL the float64 result
cast to float16.  Each comparison prints `PARITY <case> <quantity> <largest error / bound>`; the table of one run is kept in
profiles/typed_ops_parity.txt.  Shapes are the smallest that reach each kernel and each of its edges; no element is left out of any
assertion."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util as U
from moldiff_amd import _lib
from moldiff_amd import train_ops as T
from moldiff_amd._lib import ptr, stream

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

H_EPS, H_TINY = 2.0 ** -11, 2.0 ** -25      # one rounding point into a float16 container: H_EPS |ref| + H_TINY
ACC = 2e-6                                  # fp32 accumulation: ACC * sum |terms|
MDX_ERR_ARG, MDX_ERR_UNSUPPORTED = 1, 4     # include/moldiff_hip.h


def _rounding(ref, points=1):
    return points * (H_EPS * ref.abs() + H_TINY)


def _d(t):
    return t.detach().double().cpu()


def _check(case, name, got, ref, bound):
    """every element of |got - ref| <= bound (float64, element-wise; a zero bound demands equality); prints the largest ratio"""
    got, ref = _d(got), _d(ref)
    bound = torch.as_tensor(bound, dtype=torch.float64).cpu().expand_as(ref)
    assert got.shape == ref.shape, (case, name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (case, name)
    err = (got - ref).abs()
    zero = bound == 0
    assert not bool((err[zero] > 0).any()), (case, name, 'differs where the model is exact')
    ratio = float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0
    print(f'PARITY {case} {name} {ratio:.3f}')
    assert ratio <= 1.0, (case, name, ratio)


def _exact(case, name, got, ref64):
    """the fp32 arithmetic is exact: the result is the float64 result rounded once into the container"""
    want = ref64.to(got.dtype).to(got.device)
    ok = torch.equal(got.detach(), want)
    print(f'PARITY {case} {name} {"exact" if ok else "DIFFERS"}')
    assert ok, (case, name, float((_d(got) - _d(want)).abs().max()))


def _half(g, *shape, scale=1.0):
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32)).to(DEV).half()


def _f32(g, *shape, scale=1.0):
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32)).to(DEV)


def _h(t):
    return 1 if (t is not None and t.dtype == torch.float16) else 0


def _mask(*ts):
    return sum(_h(t) << i for i, t in enumerate(ts))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. element-wise pairs
# ---------------------------------------------------------------------------------------------------------------------------------
OPS = {'add': (T.add, T.ADD), 'sub': (T.sub, T.SUB), 'mul': (T.mul, T.MUL), 'gate': (T.gate, T.GATE)}
SATURATING = (12.0, -12.0, 20.0, -20.0)     # b values where the sigmoid saturates in float16 (1 - 6e-6 -> 1, 6e-6 subnormal, 2e-9 -> 0)


def _ew_model(op, a, b, g, exact_products):
    """float64 values and fp32-arithmetic allowances of out, da, db:  {name: (ref, fp32 term)}.
    `exact_products`: both factors are float16 values, their fp32 product is exact."""
    a, b, g = _d(a), _d(b), _d(g)
    z = torch.zeros_like(a)
    if op == 'add':
        return {'out': (a + b, ACC * (a.abs() + b.abs())), 'da': (g, z), 'db': (g, z)}
    if op == 'sub':
        return {'out': (a - b, ACC * (a.abs() + b.abs())), 'da': (g, z), 'db': (-g, z)}
    if op == 'mul':
        e = (lambda r: z) if exact_products else (lambda r: ACC * r.abs())
        return {'out': (a * b, e(a * b)), 'da': (g * b, e(g * b)), 'db': (g * a, e(g * a))}
    s = torch.sigmoid(b)
    # forward (fp16 mode): a * f16(sigmoid(b)) -- the sigmoid's own rounding point, plus one more half ulp of it for an fp32 sigmoid
    # that lands across a float16 boundary, both scaled by |a|; the product of the two float16 values is exact
    out_e = a.abs() * 2 * (H_EPS * s + H_TINY)
    # backward: fp32 throughout from the UNROUNDED sigmoid.  da = g s;  db = g a s (1 - s), whose subtraction 1 - s is an fp32 sum of
    # the terms 1 and s (at b = 20 the fp32 sigmoid is 1 and the factor cancels to 0)
    return {'out': (a * s, out_e), 'da': (g * s, ACC * (g * s).abs()), 'db': (g * a * s * (1 - s), ACC * (g * a).abs() * s * (1 + s))}


def _ew_run(opname, a, b, gy):
    a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    with T.precision('fp16'):
        y = OPS[opname][0](a, b)
        y.backward(gy)
    return y.detach(), a.grad, b.grad


def _ew_assert(case, opname, a, b, gy, y, da, db, rounded):
    """rounded: which of (out, da, db) end in a float16 value"""
    halves = a.dtype == torch.float16 and b.dtype == torch.float16
    model = _ew_model(opname, a, b, gy, halves and gy.dtype == torch.float16)
    for (name, got), rnd in zip((('out', y), ('da', da), ('db', db)), rounded):
        ref, e32 = model[name]
        if name == 'out' and opname == 'mul':
            e32 = torch.zeros_like(ref) if halves else ACC * ref.abs()     # (the forward's factors are a and b whatever g is)
        if rnd and not bool((e32 != 0).any()):
            _exact(case, name, got, ref.half().double())
        else:
            _check(case, name, got, ref, e32 + (_rounding(ref) if rnd else 0.0))
        if name == 'out' and opname == 'gate':
            _gate_rounds_the_sigmoid(case, a, b, got)


def _gate_rounds_the_sigmoid(case, a, b, got):
    """The bound of the gate is three half ulps wide, which an UNROUNDED sigmoid would also meet.  The contract is sharper: the result
    is f16(a * f16(s)) unless the fp32 sigmoid lands across a float16 boundary.  The fp32 sigmoid is within ACC * s of s, the rounding
    boundaries around s are one float16 ulp >= H_EPS * s apart, so at most the fraction 2 ACC / H_EPS (0.8 %) of the values can cross."""
    want = (_d(a) * torch.sigmoid(_d(b)).half().double()).half()
    frac = float((_d(got) != want.double()).double().mean())
    print(f'PARITY {case} out!=f16(a*f16(sigmoid)) fraction {frac:.5f} (allowed {2 * ACC / H_EPS:.5f})')
    assert frac <= 2 * ACC / H_EPS, (case, frac)


@pytest.mark.parametrize('opname', list(OPS))
@pytest.mark.parametrize('shape', [(1024, 8), (1237, 1), (333, 7)])
def test_elementwise_pair_in_float16_containers(opname, shape):
    """out, da, db of add / sub / mul / gate on float16 containers under precision('fp16'): (1024, 8) takes the 4-wide kernels
    (ew_fwd_kernel<4> / ew_bwd_kernel<4>), (1237, 1) and (333, 7) the scalar float16 kernels (ew_fwd_kernel<1> / ew_bwd_kernel<1>: n % 4 != 0).
    Model: add / sub = one fp32 addition, one rounding; their gradients are copies (exact).  mul and its gradients = the exact product of
    two float16 values rounded once: must EQUAL f16(a b).  gate = f16(a * f16(sigmoid(b))): see _ew_model; b holds +-12 and +-20."""
    g = U.rng(101)
    a, b, gy = _half(g, *shape), _half(g, *shape, scale=3.0), _half(g, *shape)
    b.view(-1)[:4] = torch.tensor(SATURATING, device=DEV).half()
    y, da, db = _ew_run(opname, a, b, gy)
    assert y.dtype == da.dtype == db.dtype == torch.float16
    _ew_assert(f'ew[{opname}-{shape[0]}x{shape[1]}]', opname, a, b, gy, y, da, db, (True, True, True))


@pytest.mark.parametrize('opname', list(OPS))
def test_elementwise_pair_on_a_two_byte_aligned_base(opname):
    """A 1-D float16 tensor sliced at element 1 with n % 4 == 0: the base is only 2-byte aligned, so the 4-wide kernels do not apply
    and the scalar ones must give the same values -- bit for bit those of the aligned copy, and inside the model's bounds."""
    g = U.rng(102)
    n = 2048
    base = [_half(g, n + 1), _half(g, n + 1, scale=3.0), _half(g, n + 1)]
    base[1][1:5] = torch.tensor(SATURATING, device=DEV).half()
    sliced = [t[1:] for t in base]
    assert all(t.data_ptr() % 8 == 2 and t.is_contiguous() for t in sliced)
    aligned = [t.clone() for t in sliced]
    assert all(t.data_ptr() % 16 == 0 for t in aligned)
    r1, r2 = _ew_run(opname, *sliced), _ew_run(opname, *aligned)
    for p, q in zip(r1, r2):
        assert torch.equal(p, q)
    _ew_assert(f'ew_sliced[{opname}]', opname, *aligned, *r1, (True, True, True))


@pytest.mark.parametrize('opname', list(OPS))
def test_elementwise_pair_in_mixed_containers_goes_through_fp32(opname):
    """a float16, b fp32 (values float16 cannot hold): train_ops._same converts both to fp32 containers.  The result is an fp32
    container -- holding float16 VALUES for mul / gate (fp16 mode rounds products) --, da comes back in a's container (the fp32
    gradient rounded once), db in b's (fp32 arithmetic only)."""
    g = U.rng(103)
    shape = (333, 7)
    a, b, gy = _half(g, *shape), _f32(g, *shape, scale=3.0), _f32(g, *shape)
    b.view(-1)[:4] = torch.tensor(SATURATING, device=DEV)
    y, da, db = _ew_run(opname, a, b, gy)
    assert y.dtype == torch.float32 and da.dtype == torch.float16 and db.dtype == torch.float32
    if opname in ('mul', 'gate'):
        assert torch.equal(y, y.half().float())
    _ew_assert(f'ew_mixed[{opname}]', opname, a, b, gy, y, da, db, (opname in ('mul', 'gate'), True, False))


@pytest.mark.parametrize('opname', list(OPS))
@pytest.mark.parametrize('shape', [(1024, 8), (333, 7)])
def test_elementwise_backward_with_one_gradient_only(opname, shape):
    """mdx_op_ew_bwd_t called directly with da = NULL, then with db = NULL: the gradient that is asked for equals the one of the call
    that writes both (and meets the model's bound)."""
    g = U.rng(104)
    a, b, gy = _half(g, *shape), _half(g, *shape, scale=3.0), _half(g, *shape)
    L = _lib.lib()
    n = a.numel()

    def run(want_a, want_b):
        da = torch.full_like(a, 7.0) if want_a else None
        db = torch.full_like(b, 7.0) if want_b else None
        dt = 1 | 2 | 4 | (8 if want_a else 0) | (16 if want_b else 0)
        _lib.check(L.mdx_op_ew_bwd_t(OPS[opname][1], ptr(a), ptr(b), ptr(gy), ptr(da), ptr(db), n, dt, stream()))
        return da, db

    da, db = run(True, True)
    assert torch.equal(run(True, False)[0], da) and torch.equal(run(False, True)[1], db)
    model = _ew_model(opname, a, b, gy, True)
    for name, got in (('da', da), ('db', db)):
        ref, e32 = model[name]
        if bool((e32 != 0).any()):
            _check(f'ew_bwd_direct[{opname}-{shape[0]}x{shape[1]}]', name, got, ref, e32 + _rounding(ref))
        else:
            _exact(f'ew_bwd_direct[{opname}-{shape[0]}x{shape[1]}]', name, got, ref)


@pytest.mark.parametrize('opname', ['mul', 'gate'])
@pytest.mark.parametrize('n', [2048, 1237])          # ew_fwd_kernel<4> / ew_fwd_kernel<1>
def test_float16_product_into_an_fp32_container_is_still_a_float16_value(opname, n):
    """mdx_op_ew_fwd_t with float16 operands and an fp32 result (dt = 3, a mask the wrappers do not produce) and rounding kind 2: the
    container does not round, so only the kernel's own rounding makes the result a float16 value -- f16(a b) exactly for mul."""
    g = U.rng(105)
    a, b = _half(g, n), _half(g, n, scale=3.0)
    b[:4] = torch.tensor(SATURATING, device=DEV).half()
    out = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().mdx_op_ew_fwd_t(OPS[opname][1] | (2 << 8), ptr(a), ptr(b), ptr(out), n, 3, stream()))
    assert torch.equal(out, out.half().float())
    case = f'ew_fwd_direct[{opname}-n{n}]'
    if opname == 'mul':
        _exact(case, 'out', out, (_d(a) * _d(b)).half().double())
    else:
        ref, e32 = _ew_model('gate', a, b, a, True)['out']
        _check(case, 'out', out, ref, e32 + _rounding(ref))
        _gate_rounds_the_sigmoid(case, a, b, out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the k-way gradient sum
# ---------------------------------------------------------------------------------------------------------------------------------
def _sum_n_direct(srcs, out):
    k = len(srcs)
    ptrs = (ctypes.c_void_p * k)(*[s.data_ptr() for s in srcs])
    halfs = (ctypes.c_int32 * k)(*[_h(s) for s in srcs])
    _lib.check(_lib.lib().mdx_op_sum_n(ptrs, halfs, k, out.numel(), ptr(out), _h(out), stream()))
    return out


def _sum_n_bound(srcs, out_half):
    ref = sum(_d(s) for s in srcs)
    e = ACC * sum(_d(s).abs() for s in srcs)
    return ref, e + (_rounding(ref) if out_half else 0.0)


@pytest.mark.parametrize('k', [3, 12])
@pytest.mark.parametrize('shape', [(256, 8), (515, 3)])       # sum_n_kernel<4> / sum_n_kernel<1> (n % 4 != 0)
@pytest.mark.parametrize('half', [True, False])
def test_fanout_gradient_is_one_fp32_sum_rounded_once(k, shape, half):
    """T.fanout's backward (mdx_op_sum_n): the fp32 sum of the k consumers' gradients in argument order, rounded ONCE into x's
    container -- not the k - 1 pairwise-rounded additions of autograd (those would leave up to k - 1 half ulps)."""
    g = U.rng(201)
    x = (_half(g, *shape) if half else _f32(g, *shape)).requires_grad_(True)
    grads = [(_half if half else _f32)(g, *shape, scale=1.0 + j) for j in range(k)]
    with T.precision('fp16'):
        outs = T.fanout(x, k)
        assert len(outs) == k and all(o.data_ptr() == x.data_ptr() for o in outs)
        torch.autograd.backward(list(outs), grads)
    assert x.grad.dtype == x.dtype
    ref, bound = _sum_n_bound(grads, half)
    _check(f'fanout[k{k}-{shape[0]}x{shape[1]}-{"f16" if half else "f32"}]', 'dx', x.grad, ref, bound)


@pytest.mark.parametrize('k', [3, 12])
@pytest.mark.parametrize('n', [2048, 515 * 3])
@pytest.mark.parametrize('out_half', [True, False])
def test_sum_n_with_mixed_operand_containers(k, n, out_half):
    """mdx_op_sum_n called directly: float16 and fp32 operands alternating (the fp32 ones hold values float16 cannot), float16 and
    fp32 result.  Same model: fp32 sum in argument order, one rounding where the result is float16."""
    g = U.rng(202)
    srcs = [(_half if j % 2 == 0 else _f32)(g, n, scale=1.0 + j) for j in range(k)]
    out = torch.full((n,), 7.0, dtype=torch.float16 if out_half else torch.float32, device=DEV)
    _sum_n_direct(srcs, out)
    ref, bound = _sum_n_bound(srcs, out_half)
    _check(f'sum_n[k{k}-n{n}-{"f16" if out_half else "f32"}]', 'out', out, ref, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. row gather / segment sums
# ---------------------------------------------------------------------------------------------------------------------------------
# segment lengths on every boundary of the dealt kernels' loops (`j + 12 < e; j += 16`, then `j < e; j += 4`, four threads per element)
SEG_LENGTHS = (0, 1, 2, 3, 4, 5, 12, 13, 15, 16, 17, 28, 29, 31, 32, 33, 64, 65)


@functools.lru_cache(maxsize=None)
def _designed_index():
    """(index on the CPU, number of targets): one segment of every length in SEG_LENGTHS, the first and the last target empty, rows
    assigned in shuffled order (the CSR `order` is not monotone)."""
    lens = (0,) + SEG_LENGTHS[1:9] + (0,) + SEG_LENGTHS[9:] + (0,)
    assert sorted(set(lens)) == sorted(SEG_LENGTHS) and lens[0] == 0 and lens[-1] == 0
    idx = np.repeat(np.arange(len(lens)), lens)
    U.rng(301).shuffle(idx)
    return torch.from_numpy(idx), len(lens)


def _designed_plan():
    idx, n = _designed_index()
    plan = T.IndexPlan(idx.to(DEV), n)
    order = plan.order.cpu()
    assert bool((order[1:] < order[:-1]).any())
    counts = torch.bincount(idx, minlength=n)
    assert sorted(set(counts.tolist())) == sorted(SEG_LENGTHS)
    return plan


def _rows(g, M, Fd, half=True):
    """row j carries its own scale: a dropped or doubled row shows in its segment only"""
    v = g.standard_normal((M, Fd)) * (1.0 + 0.01 * np.arange(M))[:, None]
    t = torch.from_numpy(v.astype(np.float32)).to(DEV)
    return t.half() if half else t


def _segsum64(src, idx, n):
    s = _d(src)
    ref = torch.zeros(n, s.shape[1], dtype=torch.float64).index_add_(0, idx, s)
    mag = torch.zeros(n, s.shape[1], dtype=torch.float64).index_add_(0, idx, s.abs())
    return ref, mag


def _segsum_direct(src, plan, out_dtype, extra=0):
    Fd = src.shape[1]
    out = torch.full((plan.n, Fd), 7.0, dtype=out_dtype, device=DEV)
    rc = _lib.lib().mdx_op_segsum_rows_t(ptr(src), ptr(plan.order), ptr(plan.ptr), plan.n, Fd, ptr(out), _h(src) | (_h(out) << 1) | extra,
                                         stream())
    return rc, out


@pytest.mark.parametrize('Fd', [4, 12, 64, 256])
def test_gather_and_segment_sum_of_float16_rows(Fd):
    """Every container mask the wrappers produce for float16 rows, on the designed segment lengths.  F % 8 != 0 (4, 12) takes
    segsum_rows_kernel<4, 4>, F % 8 == 0 (64, 256) segsum_rows_kernel<8, 4>.
    gather forward float16 -> float16: a copy (exact).  Its backward, a segment sum float16 -> float16: fp32 sum of the segment's
    rows, one rounding.  scatter_sum forward float16 -> fp32: the fp32 sum, no rounding.  Its backward, a gather fp32 -> float16:
    the fp32 gradient rounded once (exact).  Empty segments are exact zeros (their bound is the subnormal term alone / zero)."""
    g = U.rng(302 + Fd)
    plan = _designed_plan()
    idx, n = _designed_index()
    M = idx.numel()
    case = f'segsum[F{Fd}]'
    x, gy = _half(g, n, Fd).requires_grad_(True), _rows(g, M, Fd)
    src, gs = _rows(g, M, Fd).requires_grad_(True), _f32(g, n, Fd)
    with T.precision('fp16'):
        y = T.gather(x, plan)
        y.backward(gy)
        s = T.scatter_sum(src, plan)
        s.backward(gs)
    assert y.dtype == torch.float16 and x.grad.dtype == torch.float16 and s.dtype == torch.float32 and src.grad.dtype == torch.float16
    _exact(case, 'gather', y, _d(x)[idx])
    ref, mag = _segsum64(gy, idx, n)
    _check(case, 'gather_bwd(f16->f16)', x.grad, ref, ACC * mag + _rounding(ref))
    ref, mag = _segsum64(src, idx, n)
    _check(case, 'scatter_sum(f16->f32)', s, ref, ACC * mag)
    _exact(case, 'scatter_sum_bwd(f32->f16)', src.grad, _d(gs)[idx])


@pytest.mark.parametrize('Fd', [3, 8])
def test_segment_sum_of_fp32_rows_in_the_autocast_mode(Fd):
    """fp32 rows with the autocast bit (dt & 4; what train_ops sets under precision('fp16')): F = 3 takes the dealt scalar kernel
    segsum_rows_kernel<1, 4>, F = 8 segsum_rows_kernel<4, 4> on fp32 rows.  Model: an fp32 sum (any order), fp32 result."""
    g = U.rng(310 + Fd)
    plan = _designed_plan()
    idx, n = _designed_index()
    src = _rows(g, idx.numel(), Fd, half=False)
    with T.precision('fp16'):
        s = T.scatter_sum(src, plan)
    ref, mag = _segsum64(src, idx, n)
    _check(f'segsum_f32_autocast[F{Fd}]', 'scatter_sum', s, ref, ACC * mag)


@pytest.mark.parametrize('out_dtype', [torch.float32, torch.float16])
def test_eight_wide_and_four_wide_dealt_sums_are_bit_identical(out_dtype):
    """The same F = 64 float16 rows through both dealt kernels, selected by the source base: 16-byte aligned -> segsum_rows_kernel<8, 4>,
    8- but not 16-byte aligned (a larger allocation offset by 4 halves) -> segsum_rows_kernel<4, 4>.  The code promises the same sums in
    the same order: torch.equal."""
    g = U.rng(320)
    plan = _designed_plan()
    idx, n = _designed_index()
    M, Fd = idx.numel(), 64
    src = _rows(g, M, Fd)
    buf = torch.zeros(M * Fd + 8, dtype=torch.float16, device=DEV)
    off = buf[4:4 + M * Fd].view(M, Fd)
    off.copy_(src)
    assert src.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 8
    rc8, o8 = _segsum_direct(src, plan, out_dtype)
    rc4, o4 = _segsum_direct(off, plan, out_dtype)
    assert rc8 == 0 and rc4 == 0
    assert torch.equal(o8, o4)
    ref, mag = _segsum64(src, idx, n)
    half = out_dtype == torch.float16
    _check(f'segsum_8s_vs_4s[{"f16" if half else "f32"}]', 'out', o8, ref, ACC * mag + (_rounding(ref) if half else 0.0))


@pytest.mark.parametrize('Fd', [3, 8])
def test_fp32_segment_sum_keeps_the_sequential_csr_order(Fd):
    """fp32 mode (dt = 0): the sum of a segment is `s = 0; s += src[order[j]]` over the CSR order in float32 -- bit for bit (F = 8:
    segsum_rows_kernel<4, 1>, F = 3: segsum_rows_kernel<1, 1>)."""
    g = U.rng(330 + Fd)
    plan = _designed_plan()
    idx, n = _designed_index()
    src = _rows(g, idx.numel(), Fd, half=False)
    out = T.scatter_sum(src, plan)
    order, seg, s = plan.order.cpu().numpy(), plan.ptr.cpu().numpy(), src.cpu().numpy()
    want = np.zeros((n, Fd), dtype=np.float32)
    for r in range(n):
        acc = np.zeros(Fd, dtype=np.float32)
        for j in range(seg[r], seg[r + 1]):
            acc = acc + s[order[j]]
        want[r] = acc
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), torch.from_numpy(want))


ORDER_LENGTHS = (0, 1, 3, 4, 5, 12, 13, 16, 17, 33)   # empty; the tail alone; the main loop's first and second turn; every k of the dealt tail


@functools.lru_cache(maxsize=None)
def _order_plan():
    """(plan, order, ptr): one segment of every length in ORDER_LENGTHS, source rows assigned by a permutation"""
    idx = np.repeat(np.arange(len(ORDER_LENGTHS)), ORDER_LENGTHS)
    U.rng(350).shuffle(idx)
    plan = T.IndexPlan(torch.from_numpy(idx).to(DEV), len(ORDER_LENGTHS))
    order, seg = plan.order.cpu().numpy(), plan.ptr.cpu().numpy()
    assert sorted(order.tolist()) == list(range(idx.size)) and bool((order != np.arange(idx.size)).any())
    assert tuple(np.diff(seg).tolist()) == ORDER_LENGTHS
    return plan, order, seg


def _order_models(s, order, seg):
    """The two summation orders in float32, element by element.  sequential: s = 0; s = s + row over the segment in CSR order.
    dealt: partial k = 0..3 takes rows k, k + 4, ... of the segment in that order; the result is ((p0 + p1) + p2) + p3."""
    assert s.dtype == np.float32
    n, Fd = len(seg) - 1, s.shape[1]
    seq, dealt = np.zeros((n, Fd), dtype=np.float32), np.zeros((n, Fd), dtype=np.float32)
    for r in range(n):
        acc = np.zeros(Fd, dtype=np.float32)
        for j in range(seg[r], seg[r + 1]):
            acc = acc + s[order[j]]
        seq[r] = acc
        p = np.zeros((4, Fd), dtype=np.float32)
        for k in range(4):
            for j in range(seg[r] + k, seg[r + 1], 4):
                p[k] = p[k] + s[order[j]]
        dealt[r] = ((p[0] + p[1]) + p[2]) + p[3]
    return seq, dealt


@pytest.mark.parametrize('arm', ['f32_F3', 'f32_F8', 'f16_F4', 'f16_F64_on_16_bytes', 'f16_F64_off_by_4_halves'])
def test_segment_sums_add_in_the_stated_order_bit_for_bit(arm):
    """Both summation orders of mdx_op_segsum_rows_t as float32 numpy models, torch.equal on fp32 outputs (no rounding hides the order).
    fp32 rows: the sequential order with dt = 0 and the dealt order with dt & 4, at F = 3 (one feature per thread) and F = 8 (four).
    float16 rows are always dealt: F = 4 four-wide, F = 64 on a 16-byte base eight-wide, F = 64 offset by four halves four-wide.
    Magnitudes spread over 2^-12 .. 2^12, so float32 addition depends on the order: the two models must differ."""
    plan, order, seg = _order_plan()
    g = U.rng(351)
    half, Fd = arm.startswith('f16'), int(arm.split('_')[1][1:])
    M = order.size
    v = g.standard_normal((M, Fd)) * 2.0 ** g.integers(-12, 13, (M, Fd))
    src = torch.from_numpy(v.astype(np.float32)).to(DEV)
    if half:
        src = src.half()
        if arm.endswith('off_by_4_halves'):
            buf = torch.zeros(M * Fd + 8, dtype=torch.float16, device=DEV)
            buf[4:4 + M * Fd].view(M, Fd).copy_(src)
            src = buf[4:4 + M * Fd].view(M, Fd)
        assert src.data_ptr() % 16 == (8 if arm.endswith('off_by_4_halves') else 0)
    seq, dealt = _order_models(src.float().cpu().numpy(), order, seg)
    assert bool((seq != dealt).any())
    if not half:
        rc, out = _segsum_direct(src, plan, torch.float32)
        assert rc == 0 and torch.equal(out.cpu(), torch.from_numpy(seq)), (arm, 'sequential')
    rc, out = _segsum_direct(src, plan, torch.float32, extra=0 if half else 4)
    assert rc == 0 and torch.equal(out.cpu(), torch.from_numpy(dealt)), (arm, 'dealt')


def test_float16_segment_sum_beyond_2_to_22_items_takes_the_sequential_kernel():
    """R = 16400 targets x F = 1024 is 4,198,400 >= 2^22 four-wide items: float16 rows then fall back from the dealt kernels to
    segsum_rows_kernel<4, 1>.  600 source rows onto 40 targets; every other target is an exact zero; single-row segments are copies."""
    g = U.rng(340)
    R, Fd, M = 16400, 1024, 600
    assert R * (Fd // 4) >= 2 ** 22
    targets = np.sort(g.choice(R, 40, replace=False))
    idx = np.concatenate([targets[:10], targets[10 + g.integers(0, 30, M - 10)]])     # ten single-row segments, 590 rows onto thirty
    perm = g.permutation(M)
    idx = torch.from_numpy(idx[perm])
    src = _rows(g, M, Fd)
    plan = T.IndexPlan(idx.to(DEV), R)
    with T.precision('fp16'):
        out = T.scatter_sum(src, plan)
    pop = torch.unique(idx)
    assert out.shape == (R, Fd) and out.dtype == torch.float32
    assert torch.equal((out != 0).any(1).nonzero().flatten().cpu(), pop)
    s = _d(src)
    pos = torch.searchsorted(pop, idx)
    ref = torch.zeros(pop.numel(), Fd, dtype=torch.float64).index_add_(0, pos, s)
    mag = torch.zeros(pop.numel(), Fd, dtype=torch.float64).index_add_(0, pos, s.abs())
    _check('segsum_2^22', 'scatter_sum(f16->f32)', out[pop.to(DEV)], ref, ACC * mag)
    counts = torch.bincount(pos)
    singles = (counts == 1).nonzero().flatten()
    assert singles.numel() >= 10
    rows = torch.stack([(pos == int(t)).nonzero().flatten()[0] for t in singles])
    assert torch.equal(out[pop[singles].to(DEV)], src[rows.to(DEV)].float())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. mul_gather
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Fd', [4, 64, 256])
def test_mul_gather_in_float16_containers(Fd):
    """y = f16(a * t[idx]) and da = f16(g * t[idx]): products of two float16 values, exact in fp32, rounded once -- must EQUAL the
    float64 product cast to float16.  dtable[r] = the fp32 sum over segment r of the exact products g a, rounded once into float16;
    the designed segment lengths."""
    g = U.rng(400 + Fd)
    plan = _designed_plan()
    idx, n = _designed_index()
    M = idx.numel()
    a, tab = _rows(g, M, Fd).requires_grad_(True), _half(g, n, Fd).requires_grad_(True)
    gy = _half(g, M, Fd)
    with T.precision('fp16'):
        y = T.mul_gather(a, tab, plan)
        y.backward(gy)
    assert y.dtype == a.grad.dtype == tab.grad.dtype == torch.float16
    case = f'mul_gather[F{Fd}]'
    _exact(case, 'out', y, _d(a) * _d(tab)[idx])
    _exact(case, 'da', a.grad, _d(gy) * _d(tab)[idx])
    prod = _d(gy) * _d(a)
    ref = torch.zeros(n, Fd, dtype=torch.float64).index_add_(0, idx, prod)
    mag = torch.zeros(n, Fd, dtype=torch.float64).index_add_(0, idx, prod.abs())
    _check(case, 'dtable', tab.grad, ref, ACC * mag + _rounding(ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. / 6. LayerNorm(+ReLU) and its rank-1 backward
# ---------------------------------------------------------------------------------------------------------------------------------
LN_F = (32, 64, 128, 256)                       # lanes per row 8, 16, 32, 64 (F = 32 alone takes the row_ror:8 step)
LN_M = (1, 7, 16, 17, 63, 64, 65, 67, 1003)     # below one row group; one wave of MDX_LN_RPW = 16 rows; one workgroup of four waves; one past each;
                                                # two workgroups, the second with one short wave
KINK_ROUNDS = 8


def _kink_rows(x, gamma, beta):
    """rows holding an element whose pre-activation gamma x_hat + beta lies within 2^-10 (relative to its two terms) of the ReLU kink"""
    xd = x.double()
    xh = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-5)
    t = xh * gamma.double()
    return ((t + beta.double()).abs() < 2.0 ** -10 * (t.abs() + beta.double().abs())).any(1)


@functools.lru_cache(maxsize=None)
def _ln_case(Fd, M, relu):
    """Inputs (CPU; x, dy float16, the parameters fp32) and the float64 LayerNorm(+ReLU) of them with all its gradients, for the plain
    upstream gradient dy and for the rank-1 one f16(f16(g1) f16(w1)).  gamma has both signs, beta an offset.  With the ReLU, rows that
    hold an element near the kink are drawn again until none is left (at most KINK_ROUNDS rounds), so that no element needs to be left
    out of a comparison."""
    g = U.rng(500000 + 1000 * Fd + 2 * M + int(relu))
    gamma = torch.from_numpy(g.standard_normal(Fd).astype(np.float32))
    beta = torch.from_numpy((0.25 + 0.3 * g.standard_normal(Fd)).astype(np.float32))
    assert bool((gamma > 0).any()) and bool((gamma < 0).any())

    def draw(n):
        return torch.from_numpy((2.0 * g.standard_normal((n, Fd)) + g.standard_normal((n, 1))).astype(np.float32)).half()

    x, rounds = draw(M), 0
    while relu:
        bad = _kink_rows(x, gamma, beta)
        if not bool(bad.any()):
            break
        rounds += 1
        assert rounds <= KINK_ROUNDS, (Fd, M, rounds)
        x[bad] = draw(int(bad.sum()))
    dy = torch.from_numpy(g.standard_normal((M, Fd)).astype(np.float32)).half()
    g1 = torch.from_numpy(g.standard_normal(M).astype(np.float32))
    w1 = torch.from_numpy((g.standard_normal(Fd) * Fd ** -0.5).astype(np.float32))
    dy1 = (g1.half().double()[:, None] * w1.half().double()[None, :]).half()      # (an exact product: one rounding)

    xd = x.double()
    mean = xd.mean(1)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)
    ref = {}
    for key, up in (('', dy), ('r1_', dy1)):
        xs, gs, bs = (t.double().requires_grad_(True) for t in (x, gamma, beta))
        y = F.layer_norm(xs, (Fd,), gs, bs, 1e-5)
        y = F.relu(y) if relu else y
        y.backward(up.double())
        ref.update({'y': y.detach(), key + 'dx': xs.grad, key + 'dgamma': gs.grad, key + 'dbeta': bs.grad})
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, g1=g1, w1=w1, mean=mean, rstd=rstd, rounds=rounds, **ref)


def _tmax(t):
    return float(t.abs().max())


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('M', LN_M)
@pytest.mark.parametrize('Fd', LN_F)
def test_layernorm_relu_in_float16_containers(Fd, M, relu):
    """ln_relu_fwd4_kernel<F/4> and ln_relu_bwd4_kernel<F/4> on float16 x, y, dy, dx (parameters, statistics and parameter gradients
    fp32) against float64.  Model: fp32 arithmetic (5e-6 of max |y|; 2e-5 of the maximum of dx, dgamma, dbeta -- the bounds of the
    fp32 twin test) and one rounding of y and of dx into their float16 containers; mean to 1e-6 of the row's mean |x| (an fp32 sum of
    F terms), rstd to 1e-5 relative.  dgamma / dbeta through autograd (partial rows reduced at once) and through an active gradient
    sink (partial rows left for the deferred reduction); the two dx are the same launch and must be equal."""
    from moldiff_amd.trainer import FlatParams
    c = _ln_case(Fd, M, relu)
    case = f'layernorm[F{Fd}-M{M}-{"relu" if relu else "plain"}]'
    x, dy = c['x'].to(DEV), c['dy'].to(DEV)
    # forward and statistics, straight from the C entry
    y = torch.full((M, Fd), 7.0, dtype=torch.float16, device=DEV)
    stats = torch.full((M, 2), 7.0, dtype=torch.float32, device=DEV)
    gam, bet = c['gamma'].to(DEV), c['beta'].to(DEV)
    _lib.check(_lib.lib().mdx_op_ln_relu_fwd_t(ptr(x), ptr(gam), ptr(bet), M, Fd, int(relu), ptr(y), ptr(stats), 3, stream()))
    _check(case, 'y', y, c['y'], 5e-6 * _tmax(c['y']) + _rounding(c['y']))
    _check(case, 'mean', stats[:, 0], c['mean'], 1e-6 * c['x'].double().abs().mean(1))
    _check(case, 'rstd', stats[:, 1], c['rstd'], 1e-5 * c['rstd'])
    bdx = 2e-5 * _tmax(c['dx']) + _rounding(c['dx'])
    # operator through autograd
    xs, gs, bs = x.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    with T.precision('fp16'):
        y2 = T.ln_relu(xs, gs, bs, relu)
        y2.backward(dy)
    assert y2.dtype == torch.float16 and torch.equal(y2, y) and xs.grad.dtype == torch.float16
    _check(case, 'dx', xs.grad, c['dx'], bdx)
    _check(case, 'dgamma', gs.grad, c['dgamma'], 2e-5 * _tmax(c['dgamma']))
    _check(case, 'dbeta', bs.grad, c['dbeta'], 2e-5 * _tmax(c['dbeta']))
    # the same inside a gradient sink: the parameter gradients arrive in the flat gradient buffer at the flush
    ln = torch.nn.LayerNorm(Fd).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(gam)
        ln.bias.copy_(bet)
    flat = FlatParams(ln)
    flat.zero_grad()
    xk = x.clone().requires_grad_(True)
    with T.grad_sink(flat), T.precision('fp16'):
        T.ln_relu(xk, ln.weight, ln.bias, relu).backward(dy)
        T.flush_grad_sink()
        got = flat.grad.clone()
    assert torch.equal(xk.grad, xs.grad)
    _check(case, 'dgamma(sink)', got[:Fd], c['dgamma'], 2e-5 * _tmax(c['dgamma']))
    _check(case, 'dbeta(sink)', got[Fd:], c['dbeta'], 2e-5 * _tmax(c['dbeta']))


def _r1_call(c, M, Fd, relu, g1, ws_offset=0, x=None):
    L = _lib.lib()
    x = c['x'].to(DEV) if x is None else x
    stats = torch.stack([c['mean'], c['rstd']], 1).float().contiguous().to(DEV)
    gam, bet, w1 = c['gamma'].to(DEV), c['beta'].to(DEV), c['w1'].to(DEV)
    dx = torch.full(x.shape, 7.0, dtype=torch.float16, device=DEV)
    ws = torch.zeros(L.mdx_op_ln_relu_bwd_ws(M, Fd) // 4 + 8, dtype=torch.float32, device=DEV)
    assert ws.data_ptr() % 16 == 0
    rc = L.mdx_op_ln_relu_bwd_r1_t(ptr(g1), ptr(w1), ptr(x), ptr(stats), ptr(gam), ptr(bet), M, x.shape[1], int(relu), ptr(dx),
                                   ws.data_ptr() + 4 * ws_offset, _mask(g1, x, dx), stream())
    return rc, dx, ws


@pytest.mark.parametrize('g1_half', [True, False])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('M', LN_M)
@pytest.mark.parametrize('Fd', LN_F)
def test_layernorm_backward_with_a_rank_one_upstream_gradient(Fd, M, relu, g1_half):
    """mdx_op_ln_relu_bwd_r1_t: the LayerNorm backward whose upstream gradient is formed in the kernel as dy = f16(f16(g1) f16(w1))
    (g1 in a float16 or an fp32 container; w1 fp32 with values float16 cannot hold).  The float64 reference takes that dy through the
    same LayerNorm backward; the statistics handed in are the float64 ones rounded to fp32.  dx as in the test above (2e-5 of its
    maximum + one rounding into float16); the per-workgroup partial rows left in ws, summed in float64, are dgamma and dbeta to
    2e-5 of their maximum."""
    c = _ln_case(Fd, M, relu)
    case = f'layernorm_r1[F{Fd}-M{M}-{"relu" if relu else "plain"}-g1{"f16" if g1_half else "f32"}]'
    g1 = c['g1'].to(DEV)
    g1 = g1.half() if g1_half else g1
    rc, dx, ws = _r1_call(c, M, Fd, relu, g1)
    assert rc == 0, _lib.lib().mdx_last_error()
    _check(case, 'dx', dx, c['r1_dx'], 2e-5 * _tmax(c['r1_dx']) + _rounding(c['r1_dx']))
    rows = int(_lib.lib().mdx_op_ln_relu_bwd_rows(M))
    assert rows == ((M + 15) // 16 + 3) // 4
    dgb = ws[:rows * 2 * Fd].view(rows, 2 * Fd).double().sum(0)
    _check(case, 'dgamma(partial rows)', dgb[:Fd], c['r1_dgamma'], 2e-5 * _tmax(c['r1_dgamma']))
    _check(case, 'dbeta(partial rows)', dgb[Fd:], c['r1_dbeta'], 2e-5 * _tmax(c['r1_dbeta']))


def test_rank_one_layernorm_backward_refuses_what_it_is_not_built_for():
    """An unsupported width (F = 48) and a workspace that is not 16-byte aligned return MDX_ERR_UNSUPPORTED and leave dx untouched."""
    c = _ln_case(64, 17, True)
    g1 = c['g1'].to(DEV).half()
    rc, dx, _ = _r1_call(c, 17, 64, True, g1, ws_offset=1)
    assert rc == MDX_ERR_UNSUPPORTED and bool((dx == 7.0).all())
    rc, dx, _ = _r1_call(c, 17, 48, True, g1, x=c['x'][:, :48].contiguous().to(DEV))
    assert rc == MDX_ERR_UNSUPPORTED and bool((dx == 7.0).all())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. host contracts: refusals are return codes, nothing is launched with the refused arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_float16_containers_with_rows_that_are_no_multiple_of_four_are_refused():
    """gather, segment sum, LayerNorm forward / backward and mul_gather (forward and backward) have only 4-wide float16 kernels: the C
    entries refuse float16 containers at F = 6 and leave the outputs untouched; mul_gather's backward also refuses a base that is
    not vector-aligned, like its forward."""
    L = _lib.lib()
    g = U.rng(700)
    plan = _designed_plan()
    idx, n = _designed_index()
    M, Fd = idx.numel(), 6
    rows, tab = _half(g, M, Fd), _half(g, n, Fd)
    gam, bet = _f32(g, Fd), _f32(g, Fd)
    stats = torch.ones(M, 2, dtype=torch.float32, device=DEV)
    fresh = lambda r: torch.full((r, Fd), 7.0, dtype=torch.float16, device=DEV)
    untouched = lambda *ts: all(bool((t == 7.0).all()) for t in ts)

    y = fresh(M)
    assert L.mdx_op_gather_rows_t(ptr(tab), ptr(plan.index), M, Fd, ptr(y), 3, stream()) == MDX_ERR_ARG and untouched(y)
    out = fresh(n)
    assert L.mdx_op_segsum_rows_t(ptr(rows), ptr(plan.order), ptr(plan.ptr), n, Fd, ptr(out), 3, stream()) == MDX_ERR_ARG and untouched(out)
    st = torch.full((M, 2), 7.0, dtype=torch.float32, device=DEV)
    assert L.mdx_op_ln_relu_fwd_t(ptr(rows), ptr(gam), ptr(bet), M, Fd, 1, ptr(y), ptr(st), 3, stream()) == MDX_ERR_ARG and untouched(y, st)
    dgb = torch.full((2 * Fd,), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.zeros(L.mdx_op_ln_relu_bwd_ws(M, Fd) // 4 + 8, dtype=torch.float32, device=DEV)
    assert L.mdx_op_ln_relu_bwd_t(ptr(rows), ptr(rows), ptr(stats), ptr(gam), ptr(bet), M, Fd, 1, ptr(y), ptr(dgb), ptr(ws), 7,
                                  stream()) == MDX_ERR_ARG and untouched(y, dgb)
    assert L.mdx_op_mul_gather_fwd_t(ptr(rows), ptr(tab), ptr(plan.index), M, Fd | (2 << 16), ptr(y), 7, stream()) == MDX_ERR_ARG and untouched(y)
    dtab = fresh(n)
    assert L.mdx_op_mul_gather_bwd_t(ptr(rows), ptr(rows), ptr(tab), ptr(plan.index), ptr(plan.order), ptr(plan.ptr), M, n, Fd, ptr(y),
                                     ptr(dtab), 31, stream()) == MDX_ERR_ARG and untouched(y, dtab)

    # mul_gather backward, F = 8, every operand in turn on a base that is 4 bytes past vector alignment (room left behind each)
    Fd = 8
    ok = {k: torch.zeros(r * Fd + 8, dtype=torch.float16, device=DEV) for k, r in (('g', M), ('a', M), ('t', n), ('da', M), ('dtab', n))}
    for k in ('da', 'dtab'):
        ok[k].fill_(7.0)

    def call(shift):
        p = {k: v.data_ptr() + (4 if k == shift else 0) for k, v in ok.items()}
        return L.mdx_op_mul_gather_bwd_t(p['g'], p['a'], p['t'], ptr(plan.index), ptr(plan.order), ptr(plan.ptr), M, n, Fd, p['da'], p['dtab'],
                                         31, stream())

    for shift in ok:
        assert call(shift) == MDX_ERR_ARG, shift
        assert untouched(ok['da'], ok['dtab']), shift
    assert call(None) == 0
    torch.cuda.synchronize()
    assert bool((ok['da'][:M * Fd] == 0).all()) and bool((ok['dtab'][:n * Fd] == 0).all())


def test_wrappers_route_float16_rows_that_are_no_multiple_of_four_through_fp32():
    """F = 6, float16 input: train_ops converts to fp32 containers (the fp32 kernels take any width) and the values are still right:
    gather a copy; scatter_sum an fp32 sum; LayerNorm to the fp32 twin's 5e-6 with an fp32 result; mul_gather = mul of the gathered
    rows, a float16 VALUE (exact product, rounded once) in an fp32 container."""
    g = U.rng(701)
    plan = _designed_plan()
    idx, n = _designed_index()
    M, Fd = idx.numel(), 6
    case = 'wrappers[F6]'
    x, src, a = _half(g, n, Fd), _rows(g, M, Fd), _half(g, M, Fd)
    gam, bet = _f32(g, Fd), _f32(g, Fd)
    with T.precision('fp16'):
        y, s, ln, mg = T.gather(x, plan), T.scatter_sum(src, plan), T.ln_relu(src, gam, bet, False), T.mul_gather(a, x, plan)
    _exact(case, 'gather', y, _d(x)[idx])
    ref, mag = _segsum64(src, idx, n)
    _check(case, 'scatter_sum', s, ref, ACC * mag)
    want = F.layer_norm(_d(src), (Fd,), _d(gam), _d(bet), 1e-5)
    assert ln.dtype == torch.float32
    _check(case, 'layernorm', ln, want, 5e-6 * _tmax(want))
    assert mg.dtype == torch.float32
    _exact(case, 'mul_gather', mg, (_d(a) * _d(x)[idx]).half().double())


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. every arm of the launchers' dispatch (csrc/mdx_train.hip, csrc/mdx_train_rows.hip `pick`), through the C ABI.  Bounds are those of the operators' own tests:
#    fp32 accumulation 2e-6 * sum |terms| (tests/test_gpu_train_ops.py); a rounded output is the unrounded output rounded once (the
#    kernel rounds the same fp32 value), so it must EQUAL it after the cast.
# ---------------------------------------------------------------------------------------------------------------------------------
def _xgemm_nt(x, w, b, M, N, K, half_kind, round_out, c_half, ln=None):
    """mdx_op_xgemm_nt_t, or with ln = (gamma, beta, relu) mdx_op_xgemm_nt_ln_t -> (rc, C[, post, stats]) on the first M rows of x"""
    L = _lib.lib()
    c = torch.empty(M, N, dtype=torch.float16 if c_half else torch.float32, device=DEV)
    dt = _h(x) | (4 if c_half else 0)
    if ln is None:
        return L.mdx_op_xgemm_nt_t(ptr(x), x.stride(0), ptr(w), K, ptr(b), None, 0, ptr(c), N, M, N, K, half_kind, round_out, dt, stream()), c
    post, stats = torch.empty(M, N, dtype=torch.float16, device=DEV), torch.empty(M, 2, dtype=torch.float32, device=DEV)
    rc = L.mdx_op_xgemm_nt_ln_t(ptr(x), x.stride(0), ptr(w), K, ptr(b), None, 0, ptr(c), N, ptr(ln[0]), ptr(ln[1]), ptr(post), N, ptr(stats),
                                int(ln[2]), M, N, K, half_kind, round_out, dt | 8, stream())
    return rc, c, post, stats


@pytest.mark.parametrize('N', [32, 64, 128, 256])
@pytest.mark.parametrize('K', [32, 64, 128, 256])
def test_row_owner_gemm_arms_at_the_smallest_size_that_takes_it(K, N):
    """M = 1,024 float16 rows: the row-owner kernel with column groups (few rows for the device) and, with the launchers capped to 8
    compute units, at full width; both values of round_out; the LayerNorm form; M = 1,023 falls to the tiled kernel, which computes the
    same products in the same order."""
    g = U.rng(7000 + K + 3 * N)
    M = 1024
    x, w, b = _half(g, M, K), _f32(g, N, K, scale=K ** -0.5), _f32(g, N)
    gam, bet = 1 + 0.3 * _f32(g, N), 0.2 * _f32(g, N)
    case = f'rows_gemm[{K}x{N}]'
    ref = _d(x) @ _d(w.half()).t() + _d(b)
    mag = _d(x).abs() @ _d(w.half()).abs().t() + 1
    assert _lib.lib().mdx_op_xgemm_nt_ln_supported(M, N, K) == 1 and _lib.lib().mdx_op_xgemm_nt_ln_supported(M - 1, N, K) == 0
    outs = {}
    for cap in (None, 8):
        with (_lib.cu_cap(cap) if cap else contextlib.nullcontext()):
            for ro in (0, 1):
                rc, c = _xgemm_nt(x, w, b, M, N, K, 2, ro, bool(ro))
                _lib.check(rc)
                rc, cl, post, stats = _xgemm_nt(x, w, b, M, N, K, 2, ro, bool(ro), ln=(gam, bet, True))
                _lib.check(rc)
                outs[cap, ro] = (c, cl, post, stats)
    c0 = outs[None, 0][0]
    _check(case, 'C', c0, ref, ACC * mag)
    assert torch.equal(outs[None, 1][0], c0.half())                              # rounded once
    for (cap, ro), (c, cl, post, stats) in outs.items():
        assert torch.equal(c, outs[None, ro][0]) and torch.equal(cl, c), (cap, ro)   # column groups, full width, LayerNorm form: same rows
        want = F.relu(F.layer_norm(_d(c), (N,), _d(gam), _d(bet), 1e-5))
        assert float((_d(post) - want).abs().max()) <= 4e-3 * float(want.abs().max()), (cap, ro)
        assert float((_d(stats[:, 0]) - _d(c).mean(1)).abs().max()) <= 1e-5 * float(_d(c).abs().max()), (cap, ro)
    # one row fewer: the tiled kernel (same products, same order), and the LayerNorm form is refused
    for ro in (0, 1):
        rc, c = _xgemm_nt(x, w, b, M - 1, N, K, 2, ro, bool(ro))
        _lib.check(rc)
        assert torch.equal(c, outs[None, ro][0][:M - 1])
        assert _xgemm_nt(x, w, b, M - 1, N, K, 2, ro, bool(ro), ln=(gam, bet, True))[0] == MDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()


@pytest.mark.parametrize('N', [64, 192])                                       # 64-wide column tile; 128-wide, two of them, the second half empty
@pytest.mark.parametrize('half_kind,a_half', [(1, False), (2, False), (2, True)])
def test_tiled_gemm_arms(half_kind, a_half, N):
    """hgemm_nt_kernel for bfloat16 and float16 arithmetic, an fp32 and a float16 A, both column tiles, both values of round_out: ragged
    rows (200 = 128 + 72) and a ragged K loop (80 = 64 + 16)."""
    g = U.rng(7100 + 10 * half_kind + N)
    M, K = 200, 80
    low = (lambda t: t.bfloat16()) if half_kind == 1 else (lambda t: t.half())
    x, w, b = _f32(g, M, K), _f32(g, N, K, scale=K ** -0.5), _f32(g, N)
    x = low(x) if a_half else x
    rc, c0 = _xgemm_nt(x, w, b, M, N, K, half_kind, 0, False)
    _lib.check(rc)
    xr, wr = _d(low(x)), _d(low(w))
    _check(f'tiled_gemm[{half_kind}-{int(a_half)}-{N}]', 'C', c0, xr @ wr.t() + _d(b), ACC * (xr.abs() @ wr.abs().t() + 1))
    rc, c1 = _xgemm_nt(x, w, b, M, N, K, half_kind, 1, False)
    _lib.check(rc)
    assert torch.equal(c1, low(c0).float())                                      # rounded once, held in fp32
    if half_kind == 2:
        rc, ch = _xgemm_nt(x, w, b, M, N, K, half_kind, 1, True)
        _lib.check(rc)
        assert torch.equal(ch, c0.half())


@pytest.mark.parametrize('with_db', [True, False])
@pytest.mark.parametrize('splits', [1, 3])
@pytest.mark.parametrize('N,K,half', [(64, 64, True), (64, 128, True), (128, 64, True), (128, 128, True), (54, 6, False)])
def test_weight_gradient_arms(N, K, half, splits, with_db):
    """mdx_op_xgemm_tn_t on 200 rows: the transpose-read kernel's four tile shapes (float16 containers) and the converting kernel (fp32
    operands rounded to float16), one and three row ranges, with and without the bias gradient; no output rounding, so the error is fp32
    summation error on exact products."""
    g = U.rng(7200 + N + 3 * K)
    M = 200
    dy, x = _half(g, M, N), _half(g, M, K)
    if not half:
        dy, x = _f32(g, M, N), _f32(g, M, K)
    dyr, xr = _d(dy.half()), _d(x.half())
    part = torch.empty((splits + 1) * (N * K + N), dtype=torch.float32, device=DEV)
    dw = torch.full((N, K), float('nan'), dtype=torch.float32, device=DEV)
    db = torch.full((N,), float('nan'), dtype=torch.float32, device=DEV) if with_db else None
    _lib.check(_lib.lib().mdx_op_xgemm_tn_t(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(dw), K, ptr(db), M, N, K, splits, ptr(part), 2, 0,
                                            _mask(dy, x), stream()))
    case = f'wgrad[{N}x{K}-{splits}-{int(with_db)}]'
    _check(case, 'dW', dw, dyr.t() @ xr, ACC * float((dyr.abs().t() @ xr.abs()).max()))
    if with_db:
        _check(case, 'db', db, dyr.sum(0), ACC * float(dyr.abs().sum(0).max()))


@pytest.mark.parametrize('opname', list(OPS))
@pytest.mark.parametrize('layout', ['odd', 'offset'])
def test_elementwise_pair_in_fp32_containers_off_the_vector_path(opname, layout):
    """fp32 tensors the 4-wide kernels do not take -- n = 1,237, or n = 2,048 from a base that is 4 bytes past 16 -- run the typed scalar
    kernels with fp32 containers: add, sub, mul and their gradients are single fp32 operations and EQUAL torch's; the gate is within the
    bound of test_gpu_train_ops.test_elementwise_pairs (1e-6 / 2e-6 of the largest value)."""
    g = U.rng(7300)
    n = 1237 if layout == 'odd' else 2048
    off = 0 if layout == 'odd' else 1
    a, b, gy, out, da, db = (_f32(g, n + off)[off:] for _ in range(6))
    if off:
        assert all(t.data_ptr() % 16 == 4 for t in (a, b, gy, out, da, db))
    L, op = _lib.lib(), OPS[opname][1]
    _lib.check(L.mdx_op_ew_fwd_t(op, ptr(a), ptr(b), ptr(out), n, 0, stream()))
    _lib.check(L.mdx_op_ew_bwd_t(op, ptr(a), ptr(b), ptr(gy), ptr(da), ptr(db), n, 0, stream()))
    sg = torch.sigmoid(b)
    want = {'add': (a + b, gy, gy), 'sub': (a - b, gy, -gy), 'mul': (a * b, gy * b, gy * a),
            'gate': (a * sg, gy * sg, gy * a * sg * (1 - sg))}[opname]
    for name, got, ref, tol in zip(('out', 'da', 'db'), (out, da, db), want, (1e-6, 2e-6, 2e-6)):
        if opname == 'gate':
            assert float((_d(got) - _d(ref)).abs().max()) <= tol * float(_d(ref).abs().max()), name
        else:
            assert torch.equal(got, ref), name
