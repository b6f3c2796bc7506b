"""Differentiable layer operators of the training path: ``torch.autograd.Function`` shells around the HIP forward /
backward kernels of ``csrc/mdx_train.hip`` and ``csrc/mdx_train_fused.hip`` (C-ABI ``mdx_op_*``).

torch is the graph engine and the allocator here (it records which operator produced which tensor and calls the
backward entry points in reverse order); every O(rows x features) computation -- Linear forward, data and weight
gradients (MFMA SGEMM), LayerNorm(+ReLU), gates, gathers / segmented sums, edge geometry -- runs in the library.  There
is no CPU fallback: CPU tensors raise.  Replaces, for training, ``torch.nn.functional.linear / layer_norm / relu``,
``torch_scatter.scatter_sum`` and index_select as used by the reference's models/graph.py and models/common.py.

Every operator whose host side matters for the step time -- Linear, LayerNorm(+ReLU), Linear+LayerNorm+ReLU, the element-wise pairs and
the four fused row-owner operators -- has ONE host body, in the C++ extension (``csrc/mdx_fast.cpp``), for every precision mode and every
route by which a parameter gradient leaves a backward.  The functions here are shells: they call the extension unconditionally
(``linear``, ``ln_relu``, ``linear_ln_relu``, ``add`` ...), forward to the functions its nodes are made of (``sgemm_nt``, ``sgemm_tn``,
``transpose`` ...), or, for the fused operators, marshal the index plans and choose between the two routes of their parameter gradients.
The remaining nodes (gather / segment sum, edge geometry, smearing, force, the loss tail) have their host bodies here, over ctypes.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import ptr, stream, check

ADD, SUB, MUL, GATE = 0, 1, 2, 3

# ---- the C++ extension (round 6; csrc/mdx_fast.cpp -> moldiff_amd/_mdx_fast.so) --------------------------------------------------------
# With every operator body in Python the host needed ~20 ms per training step (a Linear node 32 us, a fused BondFFN node 110 us) -- as
# long as the GPU needs for the step.  `_mdx_fast` holds, against the same C ABI:
#   * the gradient sink and the weight-gradient queue, which exist only there, as C++ state: every sink record and queue entry goes
#     through it, in any precision mode;
#   * the Linear / LayerNorm / Linear+LayerNorm+ReLU / element-wise nodes as C++ autograd functions, in every mode, with or without a sink;
#   * the only host body of the four fused row-owner operators, in every mode that runs them (see "fused row-owner operators" below).
# A missing extension is an error, not a silent slow path.
_FASTMOD = None
# False: the parameter gradients of the fused row-owner operators take their Python route (_fused_param_grads) in the float16 sink too.
# For the test that holds the two routes bit-identical (tests/test_gpu_trainer.py); not an environment switch.
_CPP_NODES = True


def _fast():
    """the C++ extension"""
    global _FASTMOD
    if _FASTMOD is None:
        _lib.lib()      # libmoldiff_hip.so first (the extension links it)
        try:
            from . import _mdx_fast
        except ImportError as e:
            raise RuntimeError('moldiff_amd/_mdx_fast.so (the C++ fast path of the training operators) is not built or does not load: run '
                               f'`python -c "import __graft_entry__ as g; g.build()"` (make -C moldiff_amd/csrc).  [{e}]') from e
        _FASTMOD = _mdx_fast
        _FASTMOD.set_options(_WG_ON, WGRAD_ROWS, WGRAD_QUEUE_BYTES, ROWS_MIN)
        _fast_sync_precision()
    return _FASTMOD


def _fast_sync_precision():
    if _FASTMOD is not None:
        a = _AMP
        _FASTMOD.set_precision(*((int(a[0]), int(a[1]), int(a[2])) if a is not None else (0, 0, 0)))


def _L():
    return _lib.lib()


def _c(t):
    _lib._need_gpu(t)
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


# Mixed precision of the Linear layers: None = exact fp32, else (half_kind, autocast) with half_kind 1 = bfloat16, 2 = float16.
#   autocast = False ('bf16'): operands rounded, everything else fp32 (round 2's mode).
#   autocast = True  ('fp16', 'bf16_autocast'): the arithmetic of the reference's training loop, which wraps get_loss in
#     torch.autocast(dtype=float16) (scripts/train_drug3d.py:93): a Linear takes operands AND returns its result in the half type
#     (fp32 accumulation), so do its data / weight / bias gradients; products of two such results (gates, pairwise products) are
#     half too; LayerNorm, softmax, the posteriors, the loss and every segment sum stay fp32.  Tensors live in fp32 containers
#     holding half-representable values.
#   store = True ('fp16'): those half VALUES also live in float16 CONTAINERS (every Linear / LayerNorm / product result and its
#     gradient) -- the operators are memory-bound, so this halves what limits them; 'fp16_f32store' keeps fp32 containers (round 3's
#     first cut; the two differ only where the half container rounds a LayerNorm output one operator earlier -- the node residual stream
#     is not promoted to fp32 in either, unlike under the reference's autocast: see train_graph.node_edge_net).
_AMP = None
KINDS = {'f32': None, 'bf16': (1, False, False), 'fp16': (2, True, True), 'fp16_f32store': (2, True, False),
         'bf16_autocast': (1, True, False)}


class precision:
    """Context manager selecting the precision of `linear` (forward, data and weight gradients) and of the element-wise products:
    'f32' (default: exact fp32 MFMA), 'bf16' (GEMM operands rounded to bf16, fp32 accumulate and results), 'fp16' / 'bf16_autocast'
    (autocast-equivalent: see _AMP above)."""

    def __init__(self, kind):
        if isinstance(kind, str):
            if kind not in KINDS:
                raise ValueError(kind)
            kind = KINDS[kind]
        self.kind = kind

    def __enter__(self):
        global _AMP
        self.prev, _AMP = _AMP, self.kind
        _fast_sync_precision()
        return self

    def __exit__(self, *exc):
        global _AMP
        _AMP = self.prev
        _fast_sync_precision()


def _round_kind():
    return _AMP[0] if (_AMP is not None and _AMP[1]) else 0


def _t(t):
    """device tensor, contiguous, in its own container type (fp32 or float16); anything else is converted to fp32"""
    _lib._need_gpu(t)
    t = t.detach()
    if t.dtype not in (torch.float32, torch.float16):
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _h(t):
    return 1 if (t is not None and t.dtype == torch.float16) else 0


def _same(a, b):
    """two operands of an element-wise operator in one container type (mixed -> fp32; any length: the library falls back to its scalar
    kernels when the 4-wide float16 ones do not apply)"""
    a, b = _t(a), _t(b)
    if a.dtype != b.dtype:
        a, b = a.float(), b.float()
    return a, b


def _t4(t):
    """like _t, but a float16 tensor whose rows are not a multiple of 4 wide goes through fp32 (the half kernels are 4-wide)"""
    t = _t(t)
    return t.float() if (t.dtype == torch.float16 and t.shape[-1] % 4) else t


# ---- deferred parameter gradients (round 3) ----------------------------------------------------------------------------------
# While a `grad_sink` is active (Trainer.step), a Linear / LayerNorm whose parameters live in the sink's flat parameter buffer does
# not hand its weight / bias / affine gradients to autograd: it leaves the split partials of its weight-gradient GEMM (LayerNorm: its
# per-wave partial rows) where they are, records {partials, destination slot in the flat GRADIENT buffer, sizes} and returns None.
# `flush_grad_sink()` -- called once after backward -- sums every record in ONE launch (`mdx_op_reduce_deferred`, same fixed order as
# the per-layer reduction kernels) straight into the flat gradient buffer.  That replaces ~660 reduction launches and ~540 of torch's
# accumulation / slice-gradient kernels per step.  Without a sink everything goes through autograd as before.  The records live in
# the extension (csrc/mdx_fast.cpp sink_record / flush_sink: the chunked two-stage records, a repeated destination flushing first).
_SINK = None      # (parameter buffer address, gradient buffer address, bytes) of the active sink


class grad_sink:
    """Sinks do not nest; the flat buffers must be on the GPU."""

    def __init__(self, flat):
        self.flat = flat

    def __enter__(self):
        global _SINK
        f = self.flat
        _lib._need_gpu(f.data)
        F = _fast()
        _fast_sync_precision()
        F.set_options(_WG_ON, WGRAD_ROWS, WGRAD_QUEUE_BYTES, ROWS_MIN)
        F.sink_begin(f.data, f.grad)          # (raises inside an active sink)
        _SINK = (f.data.data_ptr(), f.grad.data_ptr(), f.data.numel() * 4)
        return self

    def __exit__(self, *exc):
        global _SINK
        _SINK = None
        _FASTMOD.sink_end()                   # (flushes what is left)


def _sink_dst(t):
    """address of `t`'s slot in the flat gradient buffer when t (a parameter or a view of one) lives in the sink's parameter buffer"""
    if _SINK is None or t is None:
        return None
    off = t.data_ptr() - _SINK[0]
    return _SINK[1] + off if 0 <= off < _SINK[2] else None


def _sink_record(part_ptr, dst, S, rows, cols, ld, pstride, rkind, keep):
    _FASTMOD.sink_record(part_ptr, dst, S, rows, cols, ld, pstride, rkind, keep)


def flush_grad_sink():
    """every recorded gradient summed into its slot of the flat gradient buffer: one launch, plus one over the chunk sums of the
    records that had more than 256 partials"""
    if _SINK is not None:
        _FASTMOD.flush()


# The functions below forward to the ones the extension's Linear / LayerNorm nodes are made of (csrc/mdx_fast.cpp); tests and the
# scripts under tools/ call them by these names.
def sgemm_nt(a, b, bias=None, splits=1, addend=None, keep32=False, out_dtype=None):
    """a (M,K) @ b (N,K)^T + bias + addend -> (M,N).  Rows of a / b may be strided (column slices of a wider matrix).
    keep32: in an autocast mode, do not round the result (it is a partial sum that enters another Linear as its addend).
    a / addend may be fp32 or float16 containers (mixed precision only); out_dtype: container of the result (default: the mode's)."""
    return _fast().sgemm_nt(a, b, bias, splits, addend, keep32, -1 if out_dtype is None else int(out_dtype == torch.float16))


ROWS_MIN = 16384   # from this many rows on a Linear runs on the row-owner kernel (one wave per 16 rows; the weight is re-packed per call)


def linear_rows_ok(a, n, k, addend=None):
    """Can `a` (M,k) @ W -> (M,n) take the row-owner kernel?  Shape built, enough rows, 16-byte aligned rows, fp32 mode."""
    return _fast().linear_rows_ok(a, n, k, addend)


def linear_rows(a, w, trans_w, bias=None, addend=None):
    """a (M,K) @ W^T (W (N,K), trans_w = False) or a @ W (W (K,N), trans_w = True) + bias + addend -> (M,N) on the row-owner
    kernel (csrc/mdx_linear_rows.hip)."""
    return _fast().linear_rows(a, w, bool(trans_w), bias, addend)


def _wgrad_layout(M, N, K, splits, half):
    """(row ranges actually used, offset of the bias partials) of a weight-gradient call: a pure function of its arguments"""
    return _fast().wgrad_layout(M, N, K, splits, half)


# ---- queued weight gradients (round 6) -----------------------------------------------------------------------------------------
# Inside a gradient sink, in the float16 autocast mode, a deferred weight gradient is not launched where autograd reaches it: the
# contraction is QUEUED in the extension (operands kept alive) and its flush -- at the end of backward, or when the queue holds
# WGRAD_QUEUE_BYTES of operands -- runs the whole queue as one launch per tile class (csrc wgrad_grouped_kernel) with the partials in ONE
# buffer; the sink records are made then (csrc/mdx_fast.cpp wq_append / flush_wgrads).  ~260 launches (and as many partial-buffer
# allocations) per step become <= 5; the row ranges are chosen for the queue as a whole (WGRAD_ROWS rows per block; a stand-alone launch
# needs ~512 blocks of its own to fill the chip, i.e. up to 128 row ranges = 33 MB of partials for one 256 x 256 weight).
# MDX_WGRAD_GROUPED=0 keeps the per-call launches.
_WG_ON = os.environ.get('MDX_WGRAD_GROUPED', '1') != '0'
WGRAD_ROWS = int(os.environ.get('MDX_WGRAD_ROWS', '2048'))
WGRAD_QUEUE_BYTES = int(float(os.environ.get('MDX_WGRAD_QUEUE_GB', '24')) * 2 ** 30)


def sgemm_tn(g, x, splits, want_bias=False, defer=None):
    """g (M,N)^T @ x (M,K) -> (N,K): the weight gradient, straight from the row-major tensors; with want_bias also the
    column sums of g (the bias gradient) from the same pass -> (dW, db).
    defer = (dst_w, ldw, dst_b): queue the contraction (float16 kind, queue on) or leave its split partials for `flush_grad_sink`
    (destinations in the flat gradient buffer) -> None.  The three routes are csrc/mdx_fast.cpp weight_grad."""
    dst_w, ldw, dst_b = defer if defer is not None else (0, 0, 0)
    dw, db = _fast().weight_grad(g, x, int(splits), bool(want_bias), dst_w, ldw, dst_b or 0)
    return None if defer is not None else ((dw, db) if want_bias else dw)


# Transposed weights of the step (Trainer.refresh_transposed): the flat parameter buffer's 2-D tensors, each transposed at its own
# offset of a second flat buffer by ONE launch per step.  A weight W (N,K) or a column slice W[:, a:b] of it (the hoisted layers
# split their weights by columns, train_graph.py) then has its transpose as a VIEW: rows a..b of W^T (K,N).
_WT = None


class TransposedParams:
    def __init__(self, flat):
        self.base, self.nbytes = flat.data.data_ptr(), 4 * flat.numel
        # every W^T starts on 16 bytes in its own buffer (round 6: with the parameter buffer's offsets a third of the weights' transposes
        # were unaligned and fell back to a transpose launch per data gradient)
        self.buf = torch.empty(flat.numel + 4 * len(flat.params) + 4, dtype=torch.float32, device=flat.data.device)
        pad = (-self.buf.data_ptr() // 4) % 4
        self.entries, desc, off, doff, tiles = {}, [], 0, pad, 1
        for p in flat.params:
            n = p.numel()
            if p.dim() == 2 and p.shape[0] % 4 == 0:     # W^T rows are R = shape[0] floats: 16-byte aligned rows for the GEMM loads
                R, C = p.shape
                self.entries[4 * off] = (off, R, C, doff)
                desc += [self.base + 4 * off, self.buf.data_ptr() + 4 * doff, R, C]
                tiles = max(tiles, ((R + 31) // 32) * ((C + 31) // 32))
                doff += (n + 3) // 4 * 4
            off += n
        self.offsets = sorted(self.entries)
        self.n, self.tiles = len(desc) // 4, tiles
        self.desc = torch.tensor(desc, dtype=torch.int64, device=flat.data.device)

    def refresh(self):
        check(_L().mdx_op_transpose_batch(ptr(self.desc), self.n, self.tiles, stream()))

    def table(self):
        """what the extension's lookup takes: (parameter buffer address, bytes, W^T buffer, sorted byte offsets, (off, R, C, dst off) per offset)"""
        return self.base, self.nbytes, self.buf, self.offsets, [list(self.entries[o]) for o in self.offsets]

    def view(self, w):
        """W^T of a parameter matrix or of a column slice of one, as a view into the transposed buffer; None if `w` is neither (or if
        its rows there would not start on 16 bytes).  The lookup is the one the nodes use (csrc/mdx_fast.cpp wt_view).  For tests and
        tools: every call hands the whole table over (O(entries)); the nodes look up in the copy that transposed_params installed."""
        base, nbytes, buf, offsets, entries = self.table()
        r = _fast().wt_view(base, nbytes, buf.data_ptr(), offsets, entries, w)
        if r is None:
            return None
        start, R = r
        return buf[start:start + R * w.shape[1]].view(w.shape[1], R)


class transposed_params:
    """context: the dgrad GEMMs inside take W^T from `tp` (a TransposedParams refreshed for the current weights)"""

    def __init__(self, tp):
        self.tp = tp

    def __enter__(self):
        global _WT
        self.prev, _WT = _WT, self.tp
        _fast_sync_wt()

    def __exit__(self, *a):
        global _WT
        _WT = self.prev
        _fast_sync_wt()


def _fast_sync_wt():
    F = _fast() if (_WT is None or _WT.buf.is_cuda) else None
    if F is not None:
        tp = _WT
        if tp is None:
            F.set_wt(0, 0, None, [], [])
        else:
            F.set_wt(*tp.table())


def transpose(x, pad=4):
    """(R,C) -> contiguous-rows (C,R) view whose leading dimension is padded to a multiple of `pad` floats (so that the
    SGEMM's 16-byte loads stay aligned for any R); a view into the step's transposed parameters where `x` has one."""
    return _fast().transpose(x, pad)


def colreduce(x, y=None):
    return _fast().colreduce(x, y)


def _splits_for(rows, n, k, half=False):
    """row ranges of a weight gradient launched on its own (csrc/mdx_fast.cpp splits_for): enough to fill the chip, each >= 128 rows"""
    return _fast().splits_for(rows, n, k, bool(half))


def _rows(t):
    """device matrix (fp32 or float16 container) whose rows are contiguous (row stride arbitrary: column slices of a weight stay views)."""
    return _fast().rows(t.detach())


def linear(x, w, b=None, addend=None, keep32=False):
    """y = x @ w.T + b + addend for 2-D x (rows, in_features); `addend` (rows, out_features) is added in the GEMM epilogue
    (used for the per-node part of a layer whose reference input is a concatenation [edge part | node part | time]).
    keep32: the result is itself such a partial sum -- an autocast mode must not round it (the reference rounds the WHOLE layer's
    result once)."""
    return _fast().linear(x, w, b, addend, bool(keep32))


def ln_relu(x, gamma, beta, relu=True):
    return _fast().ln_relu(x, gamma, beta, bool(relu))


def linear_ln_ok(x, w, addend):
    """Can Linear(x) -> LayerNorm -> ReLU take the fused launch (csrc mdx_op_xgemm_nt_ln_t)?  float16 mode, float16 rows of x, widths
    the row-owner kernel is built for."""
    return _fast().linear_ln_ok(x, w, addend)


def linear_ln_relu(x, w, b, gamma, beta, addend=None):
    """relu(LayerNorm(x @ w.T + b + addend)): one launch where the fused kernel is built, the two operators otherwise"""
    return _fast().linear_ln_relu(x, w, b, addend, gamma, beta)


def linear_ln_relu_dot(x, w, b, gamma, beta, w2, b2):
    """linear(relu(LayerNorm(x @ w.T + b)), w2, b2) with w2 of ONE row -- common.MLP(…, 1) as PosUpdate's inter module uses it.  In the
    float16 sink one node whose backward forms the second Linear's rank-1 data gradient inside the LayerNorm backward (csrc
    mdx_op_ln_relu_bwd_r1_t); otherwise the two operators."""
    return _fast().linear_ln_relu_dot(x, w, b, gamma, beta, w2, b2)


def _ew(op, a, b):
    return _fast().ew(op, a, b)


def add(a, b):
    return _ew(ADD, a, b)


def sub(a, b):
    return _ew(SUB, a, b)


def mul(a, b):
    return _ew(MUL, a, b)


def gate(a, b):
    """a * sigmoid(b)"""
    return _ew(GATE, a, b)


class _Fanout(torch.autograd.Function):
    """k aliases of x for its k consumers; the backward sums their gradients in ONE launch (csrc sum_n4_kernel: fp32 sum in consumer
    order, one rounding to x's container) where autograd would run k - 1 element-wise adds."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.dtype, ctx.shape = x.dtype, x.shape
        return tuple(x.view_as(x) for _ in range(k))

    @staticmethod
    def backward(ctx, *gs):
        gs = [_t(g) for g in gs if g is not None]
        if not gs:
            return None, None
        if len(gs) == 1:
            g = gs[0]
            return (g if g.dtype == ctx.dtype else g.to(ctx.dtype)), None
        odt = ctx.dtype if ctx.dtype in (torch.float16, torch.float32) else torch.float32
        out = torch.empty(ctx.shape, dtype=odt, device=gs[0].device)
        k = len(gs)
        ptrs = (ctypes.c_void_p * k)(*[g.data_ptr() for g in gs])
        halfs = (ctypes.c_int32 * k)(*[_h(g) for g in gs])
        check(_L().mdx_op_sum_n(ptrs, halfs, k, out.numel(), ptr(out), _h(out), stream()))
        return (out if odt == ctx.dtype else out.to(ctx.dtype)), None


def fanout(x, k):
    """k aliases of x, one per consumer (see _Fanout); plain repetition when there is nothing to gain"""
    if k < 3 or k > 12 or not x.is_cuda or not x.requires_grad or not torch.is_grad_enabled():
        return (x,) * k
    return _Fanout.apply(x, k)


class IndexPlan:
    """An index vector (rows -> targets in [0, n)) with the CSR needed to sum rows per target without atomics:
    `order` = stable argsort, `ptr` = segment starts.  Built once per batch (index bookkeeping, not arithmetic)."""

    def __init__(self, index, n):
        _lib._need_gpu(index)
        self.index = index.detach().to(torch.int64).contiguous()
        self.n = int(n)
        srt = torch.sort(self.index, stable=True)
        self.order = srt.indices.contiguous()
        # segment starts from the sorted values (torch.bincount would read the maximum back to the host: a device sync per plan)
        self.ptr = torch.searchsorted(srt.values, torch.arange(self.n + 1, dtype=torch.int64, device=index.device))


class FlippedPlan:
    """IndexPlan of the RIGHT end points of a directed edge list [half-edges ; flipped half-edges] derived from the plan of the left ones
    (csrc plan_flip_kernel): same segment starts, the order by one launch instead of a second stable sort."""

    def __init__(self, left_plan, index, n_half):
        self.index = index.detach().to(torch.int64).contiguous()
        self.n, self.ptr = left_plan.n, left_plan.ptr
        self.order = torch.empty_like(left_plan.order)
        check(_L().mdx_op_plan_flip(ptr(left_plan.order), ptr(left_plan.ptr), self.n, int(n_half), ptr(self.order), stream()))


def _gather_raw(x, plan, out_dtype=None):
    M, F = plan.index.numel(), x.shape[1]
    y = torch.empty(M, F, dtype=out_dtype or x.dtype, device=x.device)
    check(_L().mdx_op_gather_rows_t(ptr(x), ptr(plan.index), M, F, ptr(y), _h(x) | (_h(y) << 1), stream()))
    return y


def _segsum_raw(src, plan, out_dtype=torch.float32):
    F = src.shape[1]
    out = torch.empty(plan.n, F, dtype=out_dtype, device=src.device)
    # bit 2: in an autocast mode fp32 rows may be summed in the dealt order too (the fp32 mode keeps the reference's sequential order)
    check(_L().mdx_op_segsum_rows_t(ptr(src), ptr(plan.order), ptr(plan.ptr), plan.n, F, ptr(out),
                                    _h(src) | (_h(out) << 1) | (4 if (_AMP is not None and _AMP[1]) else 0), stream()))
    return out


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan, ctx.dtype = plan, x.dtype
        return _gather_raw(_t4(x), plan)

    @staticmethod
    def backward(ctx, g):
        g = _t4(g)
        half = ctx.dtype == torch.float16 and g.shape[-1] % 4 == 0
        r = _segsum_raw(g, ctx.plan, torch.float16 if half else torch.float32)
        return (r if r.dtype == ctx.dtype else r.to(ctx.dtype)), None


class _SegSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, plan):
        ctx.plan, ctx.dtype = plan, src.dtype
        return _segsum_raw(_t4(src), plan)            # sums are fp32 whatever the rows' container

    @staticmethod
    def backward(ctx, g):
        g = _t4(g)
        half = ctx.dtype == torch.float16 and g.shape[-1] % 4 == 0
        r = _gather_raw(g, ctx.plan, torch.float16 if half else torch.float32)
        return (r if r.dtype == ctx.dtype else r.to(ctx.dtype)), None


def gather(x, plan):
    """x[plan.index] for 2-D x."""
    return _Gather.apply(x, plan)


def scatter_sum(src, plan):
    """torch_scatter.scatter_sum(src, plan.index, dim=0, dim_size=plan.n)."""
    return _SegSum.apply(src, plan)


class _MulGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, table, plan):
        ctx.dtypes = (a.dtype, table.dtype)
        ac, tc = _same(a, table)
        M, F = ac.shape
        y = torch.empty_like(ac)
        check(_L().mdx_op_mul_gather_fwd_t(ptr(ac), ptr(tc), ptr(plan.index), M, F | (_round_kind() << 16), ptr(y),
                                           _h(ac) | (_h(tc) << 1) | (_h(y) << 2), stream()))
        ctx.plan = plan
        ctx.save_for_backward(ac, tc)
        return y

    @staticmethod
    def backward(ctx, g):
        a, t = ctx.saved_tensors
        g, plan = _t(g), ctx.plan
        M, F = a.shape
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        check(_L().mdx_op_mul_gather_bwd_t(ptr(g), ptr(a), ptr(t), ptr(plan.index), ptr(plan.order), ptr(plan.ptr), M, plan.n, F, ptr(da),
                                           ptr(dt), _h(g) | (_h(a) << 1) | (_h(t) << 2) | (_h(da) << 3) | (_h(dt) << 4), stream()))
        if da is not None and da.dtype != ctx.dtypes[0]:
            da = da.to(ctx.dtypes[0])
        if dt is not None and dt.dtype != ctx.dtypes[1]:
            dt = dt.to(ctx.dtypes[1])
        return da, dt, None


def mul_gather(a, table, plan):
    """a * table[plan.index] for 2-D a (rows, F), F % 4 == 0, without materialising the gathered rows."""
    if a.shape[1] % 4:
        return mul(a, gather(table, plan))
    return _MulGather.apply(a, table, plan)


class _EdgeGeom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, pl, pr):
        p = _c(pos)
        E = pl.index.numel()
        rel = torch.empty(E, 3, dtype=torch.float32, device=p.device)
        dist = torch.empty(E, dtype=torch.float32, device=p.device)
        check(_L().mdx_op_edge_geom_fwd(ptr(p), ptr(pl.index), ptr(pr.index), E, ptr(rel), ptr(dist), stream()))
        ctx.pl, ctx.pr, ctx.prec = pl, pr, _AMP
        ctx.save_for_backward(rel, dist)
        return rel, dist

    @staticmethod
    def backward(ctx, grel, gdist):
        rel, dist = ctx.saved_tensors
        E = rel.shape[0]
        g = torch.empty_like(rel)
        check(_L().mdx_op_edge_geom_bwd(ptr(rel), ptr(dist), ptr(_c(grel) if grel is not None else None),
                                        ptr(_c(gdist) if gdist is not None else None), E, ptr(g), stream()))
        with precision(ctx.prec):
            gl, gr = _segsum_raw(g, ctx.pl), _segsum_raw(g, ctx.pr)
        out = torch.empty_like(gl)
        check(_L().mdx_op_ew_fwd_t(SUB, ptr(gl), ptr(gr), ptr(out), gl.numel(), 0, stream()))
        return out, None, None


def edge_geom(pos, plan_left, plan_right):
    """rel = pos[left] - pos[right] (E,3), dist = |rel| (E,)."""
    return _EdgeGeom.apply(pos, plan_left, plan_right)


class _Smear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dist, offset, coeff, lo, hi):
        d, off, co = _c(dist), _c(offset), _c(coeff)
        E, G = d.numel(), off.numel()
        out = torch.empty(E, G, dtype=torch.float32, device=d.device)
        check(_L().mdx_op_smear_fwd(ptr(d), ptr(off), ptr(co), G, float(lo), float(hi), E, ptr(out), stream()))
        ctx.save_for_backward(d, off, co)
        ctx.lohi = (float(lo), float(hi))
        return out

    @staticmethod
    def backward(ctx, g):
        d, off, co = ctx.saved_tensors
        gd = torch.empty_like(d)
        check(_L().mdx_op_smear_bwd(ptr(d), ptr(off), ptr(co), off.numel(), ctx.lohi[0], ctx.lohi[1], d.numel(), ptr(_c(g)), ptr(gd),
                                    stream()))
        return gd, None, None, None, None


def smear(dist, offset, coeff, lo, hi):
    """GaussianSmearing with per-gaussian coefficients: exp(coeff_k (clamp(d, lo, hi) - offset_k)^2)."""
    return _Smear.apply(dist, offset, coeff, lo, hi)


class _Force(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, rel, dist):
        wc, rc, dc = _c(w).reshape(-1), _c(rel), _c(dist)
        out = torch.empty_like(rc)
        check(_L().mdx_op_force_fwd(ptr(wc), ptr(rc), ptr(dc), dc.numel(), ptr(out), stream()))
        ctx.save_for_backward(wc, rc, dc)
        ctx.wshape, ctx.wdtype = w.shape, w.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        w, rel, d = ctx.saved_tensors
        gw, grel, gd = torch.empty_like(w), torch.empty_like(rel), torch.empty_like(d)
        check(_L().mdx_op_force_bwd(ptr(w), ptr(rel), ptr(d), ptr(_c(g)), d.numel(), ptr(gw), ptr(grel), ptr(gd), stream()))
        return gw.reshape(ctx.wshape).to(ctx.wdtype), grel, gd


def force(w, rel, dist):
    """w * rel / dist / (dist + 1) per edge (PosUpdate, models/graph.py:393)."""
    return _Force.apply(w, rel, dist)


# ---- fused row-owner operators (round 6; csrc/mdx_train_fused.hip) -------------------------------------------------------------------
# BondFFN + the scatter_sum that follows it, the EdgeBlock tail, the PosUpdate front and the NodeBlock message path, each as ONE autograd
# node.  The BondFFN: 2 launches forward (fused chain, segment sum) and 9 backward (fused data-gradient chain, 6 weight-gradient
# contractions, 2 segment sums) where the per-operator composition issues 12 and ~28.  float16 autocast mode with float16 containers
# only; every other mode keeps the per-operator path.
# Each operator has one host body, in the extension (csrc/mdx_fast.cpp *_fwd / *_bwd): it normalises the operands, allocates the buffers,
# fills the argument block, launches and runs the segment sums.  The classes below marshal the index plans and call it.  Only the
# parameter gradients leave a backward by one of two routes (_fused_backward):
#   * inside a float16 sink that holds every parameter of the node (`all_in_sink`; Trainer.step), the C++ side queues the weight-gradient
#     contractions and records the LayerNorm partial rows itself: no parameter gradient passes through autograd;
#   * otherwise it hands the contractions and the LayerNorm slices back as tensors, and _fused_param_grads defers each into the sink
#     or returns it through autograd, parameter by parameter.
FUSED_MIN_ROWS = 1024   # below this the per-operator path runs (tests lower it to cover the fused path on small graphs)
_FUSED = os.environ.get('MDX_TRAIN_FUSED', '1') != '0'
_FUSED_TAIL = True
_FUSED_POS = True
_FUSED_NODE = True


def _fused_mode():
    """the mode the fused kernels are built for: float16 autocast with float16 containers"""
    return _FUSED and _AMP is not None and _AMP[0] == 2 and _AMP[1] and _AMP[2]


def _wgrad_into(grads, need, ps, gy, xin, wi, bi):
    """weight (+ bias) gradient of one Linear inside a fused node (parameters ps[wi], ps[bi]; bi < 0: no bias): deferred into the flat
    gradient buffer when a sink holds the parameter, else returned through `grads`"""
    if not need[wi]:
        return
    w = ps[wi]
    want_b = bi >= 0 and need[bi]
    dst_w = _sink_dst(w)
    dst_b = _sink_dst(ps[bi]) if want_b else None
    sp = _splits_for(gy.shape[0], gy.shape[1], xin.shape[1], _h(gy) and _h(xin))
    if dst_w is not None and (not want_b or dst_b is not None):
        sgemm_tn(gy, xin, sp, want_bias=want_b, defer=(dst_w, w.stride(0), dst_b))
    else:
        r = sgemm_tn(gy, xin, sp, want_bias=want_b)
        grads[wi], gb_ = r if want_b else (r, None)
        if want_b:
            grads[bi] = gb_


def _fused_param_grads(ps, need, contractions, lnp, slices):
    """The Python route of a fused backward's parameter gradients -> one gradient (or None) per parameter of `ps`.  contractions:
    [(gy, xin, weight index, bias index)]; slices: [(parameter index, float offset in lnp, width)] of the LayerNorm-parameter
    gradients, one partial row per workgroup in lnp."""
    grads = [None] * len(ps)
    for gy, xin, wi, bi in contractions:
        _wgrad_into(grads, need, ps, gy, xin, wi, bi)
    nwg, lnf = lnp.shape
    for pi, off, F in slices:
        if not need[pi]:
            continue
        dst = _sink_dst(ps[pi])
        if dst is not None:
            _sink_record(lnp.data_ptr() + 4 * off, dst, nwg, 1, F, F, lnf, 0, lnp)
        else:
            grads[pi] = lnp[:, off:off + F].sum(0)
    return grads


def _fused_backward(ctx, n_in, bwd):
    """backward of a fused node whose first three inputs of n_in are differentiable tensors and whose parameters (ctx.ps) follow them.
    bwd(F, needs_input_grad, dispose) calls the operator's F.*_bwd, in the precision of the forward."""
    ni, ps = ctx.needs_input_grad, ctx.ps
    with precision(ctx.prec):
        F = _fast()
        if _CPP_NODES and F.all_in_sink(ps):
            g, pgrads = bwd(F, ni, True), [None] * len(ps)
        else:
            g, contractions, lnp, slices = bwd(F, ni, False)
            pgrads = _fused_param_grads(ps, ni[n_in:], contractions, lnp, slices)
    gx = g[0]
    if gx is not None and gx.dtype != ctx.x_dtype:
        gx = gx.to(ctx.x_dtype)
    ctx.saved = None
    return (gx, g[1], g[2]) + (None,) * (n_in - 3) + tuple(pgrads)


def bondffn_fused_ok(bond_in, node_lin, gate_node, dims):
    """dims = (bond, inter, out, gate hidden, node columns of the gate): the kernel is built for (64, 128, 64, 32, any)."""
    return (_fused_mode() and bond_in.dtype == torch.float16 and bond_in.dim() == 2
            and bond_in.shape[0] >= FUSED_MIN_ROWS and dims[:4] == (64, 128, 64, 32) and node_lin.dtype == torch.float16
            and gate_node.dtype == torch.float32)


class _BondFfnScatter(torch.autograd.Function):
    """scatter_sum(BondFFN(bond_in, h_node[idx], time), oidx) with the node-side Linears hoisted by the caller:
    args = bond_in (E,64) f16, NL = node_linear(h) (N,128) f16, GN = gate.net.0[:, node columns](h) (N,32) fp32, time (E,1) fp32,
    plan_in (idx), plan_out (oidx), then the parameters in the order of PARAMS."""
    PARAMS = ('Wb', 'Wi1', 'bi1', 'g1', 'be1', 'Wi2', 'bi2', 'Wg1', 'bg1', 'gg', 'gbe', 'Wt', 'Wg2', 'bg2')

    @staticmethod
    def forward(ctx, bond_in, NL, GN, time, plan_in, plan_out, *params):
        ps = list(params)
        r = _fast().bondffn_fwd(bond_in, NL, GN, time, plan_in.index, plan_out.order, plan_out.ptr, plan_out.n, ps)
        ctx.saved, ctx.ps, ctx.plan_in, ctx.plan_out = r[1:], ps, plan_in, plan_out
        t2 = time.detach()
        ctx.time2d = t2 if t2.dim() == 2 else t2.reshape(-1, 1)
        ctx.prec, ctx.x_dtype = _AMP, bond_in.dtype
        return r[0]

    @staticmethod
    def backward(ctx, gS):
        pi = ctx.plan_in
        return _fused_backward(ctx, 6, lambda F, ni, dispose: F.bondffn_bwd(
            gS, ctx.saved, pi.index, pi.order, pi.ptr, pi.n, ctx.plan_out.index, ctx.time2d, ctx.ps, ni[0], ni[1], ni[2], dispose))


def bondffn_scatter(bond_in, node_lin, gate_node, time, plan_in, plan_out, params):
    """params: dict with the keys of _BondFfnScatter.PARAMS (parameters or column slices of them)"""
    return _BondFfnScatter.apply(bond_in, node_lin, gate_node, time, plan_in, plan_out, *[params[k] for k in _BondFfnScatter.PARAMS])


def edge_tail_fused_ok(h_bond, by_left, by_right):
    return (_fused_mode() and _FUSED_TAIL and h_bond.dtype == torch.float16 and h_bond.dim() == 2
            and h_bond.shape[1] == 64 and h_bond.shape[0] >= FUSED_MIN_ROWS and by_left.dtype == torch.float16 and by_right.dtype == torch.float16
            and by_left.shape[1] == 64 and by_right.shape[1] == 64)


class _EdgeTail(torch.autograd.Function):
    """h + out_transform(relu(LN(self_ffn(h) + BL[left] + BR[right]))) (models/graph.py:281-294 + the residual of :360) as one node:
    args = h (E,64) f16, BL, BR (N,64) f16, plan_left, plan_right, then PARAMS."""
    PARAMS = ('Ws', 'bs', 'lng', 'lnb', 'Wo', 'bo')

    @staticmethod
    def forward(ctx, h, BL, BR, plan_l, plan_r, *params):
        ps = list(params)
        r = _fast().edge_tail_fwd(h, BL, BR, plan_l.index, plan_r.index, ps)
        ctx.saved, ctx.ps, ctx.plan_l, ctx.plan_r = r[1:], ps, plan_l, plan_r
        ctx.prec, ctx.x_dtype = _AMP, h.dtype
        return r[0]

    @staticmethod
    def backward(ctx, g_out):
        pl, pr = ctx.plan_l, ctx.plan_r
        return _fused_backward(ctx, 5, lambda F, ni, dispose: F.edge_tail_bwd(
            g_out, ctx.saved, pl.index, pr.index, pl.order, pl.ptr, pr.order, pr.ptr, pl.n, ctx.ps, ni[0], ni[1], ni[2], dispose))


def edge_tail(h, by_left, by_right, plan_l, plan_r, params):
    return _EdgeTail.apply(h, by_left, by_right, plan_l, plan_r, *[params[k] for k in _EdgeTail.PARAMS])


def posffn_fused_ok(h_edge, lf, rf, dims):
    """dims = (bond, node, inter, gate hidden, out): the kernel is built for PosUpdate's BondFFN (64, 64, 256, 32, 1)"""
    return (_fused_mode() and _FUSED_POS and h_edge.dtype == torch.float16 and h_edge.dim() == 2
            and h_edge.shape[0] >= FUSED_MIN_ROWS and dims == (64, 64, 256, 32, 1) and lf.dtype == torch.float16 and rf.dtype == torch.float16
            and lf.shape[1] == 64 and rf.shape[1] == 64)


class _PosFfnFront(torch.autograd.Function):
    """(prod, gate) of PosUpdate's BondFFN (models/graph.py:388-390 with :133-141): prod = bond_linear(h_edge) * node_linear(a) (E,256),
    gate = gate MLP([h_edge | a | t]) (E,1), a = LF[left] * RF[right].  args = h_edge (E,64) f16, LF, RF (N,64) f16, time (E,1) fp32,
    plan_left, plan_right, then PARAMS."""
    PARAMS = ('Wb', 'Wn', 'Wg1x', 'Wg1a', 'Wt', 'bg1', 'gg', 'gbe', 'Wg2', 'bg2')

    @staticmethod
    def forward(ctx, h_edge, LF, RF, time, plan_l, plan_r, *params):
        ps = list(params)
        r = _fast().posffn_fwd(h_edge, LF, RF, time, plan_l.index, plan_r.index, ps)
        # the outputs [prod, gate] through save_for_backward (on ctx itself they would form a cycle output -> grad_fn -> ctx -> output),
        # the rest [x, LF, RF, te, a, gpre, gpost] on ctx
        ctx.save_for_backward(r[0], r[1])
        ctx.saved, ctx.ps, ctx.plan_l, ctx.plan_r = r[2:], ps, plan_l, plan_r
        ctx.time2d = time.detach().reshape(-1, 1)
        ctx.prec, ctx.x_dtype = _AMP, h_edge.dtype
        return r[0], r[1]

    @staticmethod
    def backward(ctx, g_prod, g_gate):
        pl, pr = ctx.plan_l, ctx.plan_r
        saved = ctx.saved + list(ctx.saved_tensors)
        return _fused_backward(ctx, 6, lambda F, ni, dispose: F.posffn_bwd(
            g_prod, g_gate, saved, pl.index, pr.index, pl.order, pl.ptr, pr.order, pr.ptr, pl.n, ctx.time2d, ctx.ps, ni[0], ni[1], ni[2], dispose))


def posffn_front(h_edge, lf, rf, time, plan_l, plan_r, params):
    return _PosFfnFront.apply(h_edge, lf, rf, time, plan_l, plan_r, *[params[k] for k in _PosFfnFront.PARAMS])


def nodemsg_fused_ok(edge_attr, hn, pn, shapes):
    """shapes = (edge_net.0, edge_net.3, msg_net, gate.0 edge columns, gate.3 weight shapes): built for 64 -> 256 -> 256"""
    return (_fused_mode() and _FUSED_NODE and edge_attr.dtype == torch.float16
            and edge_attr.dim() == 2 and edge_attr.shape[1] == 64 and edge_attr.shape[0] >= FUSED_MIN_ROWS and hn.dtype == torch.float16
            and hn.shape[1] == 256 and pn.dtype == torch.float32 and pn.shape[1] == 256
            and shapes == ((256, 64), (256, 256), (256, 256), (256, 64), (256, 256)))


class _NodeMsg(torch.autograd.Function):
    """scatter_sum(msg, left) of the NodeBlock message path (models/graph.py:40-50) as one node:
    args = edge_attr (E,64) f16, HN = node_net(x) (N,256) f16, PN = gate.net.0[:, node + time columns](cat(x, t)) (N,256) fp32,
    plan_col (right), plan_row (left), then PARAMS."""
    PARAMS = ('W1e', 'b1e', 'lng_e', 'lnb_e', 'W2e', 'b2e', 'Wm', 'bm', 'Wg1', 'bg1', 'lng_g', 'lnb_g', 'Wg2', 'bg2')

    @staticmethod
    def forward(ctx, edge_attr, HN, PN, plan_col, plan_row, *params):
        ps = list(params)
        r = _fast().nodemsg_fwd(edge_attr, HN, PN, plan_col.index, plan_row.order, plan_row.ptr, plan_row.n, ps)
        ctx.saved, ctx.ps, ctx.plan_col, ctx.plan_row = r[1:], ps, plan_col, plan_row
        ctx.prec, ctx.x_dtype = _AMP, edge_attr.dtype
        return r[0]

    @staticmethod
    def backward(ctx, gA):
        pc = ctx.plan_col
        return _fused_backward(ctx, 5, lambda F, ni, dispose: F.nodemsg_bwd(
            gA, ctx.saved, pc.index, pc.order, pc.ptr, pc.n, ctx.plan_row.index, ctx.ps, ni[0], ni[1], ni[2], dispose))


def nodemsg(edge_attr, hn, pn, plan_col, plan_row, params):
    return _NodeMsg.apply(edge_attr, hn, pn, plan_col, plan_row, *[params[k] for k in _NodeMsg.PARAMS])


# ---- the categorical loss tail as one node (round 6; csrc/mdx_transition.hip cat_loss_kernel) -----------------------------------------
class _CatLoss(torch.autograd.Function):
    """100 x mean over rows of {KL(q(v_{t-1} | v_t, v_0) || p_theta) for t > 0 | decoder NLL at t == 0} (models/model.py:170-189) as ONE
    launch that also leaves d row / d logits; the backward is a scaling.  Replaces ~45 torch launches forward and ~50 backward per loss
    term (log_softmax, the posterior algebra of transition.q_v_posterior_autograd, compute_v_Lt)."""

    @staticmethod
    def forward(ctx, logits, q_mats, qT, log_vt, log_v0, t, batch):
        lg, lvt, lv0 = _c(logits), _c(log_vt), _c(log_v0)
        n, K = lg.shape
        tt = t.detach().to(torch.int64).contiguous()
        bb = batch.detach().to(torch.int64).contiguous()
        row = torch.empty(n, dtype=torch.float32, device=lg.device)
        dl = torch.empty(n, K, dtype=torch.float32, device=lg.device)
        check(_L().mdx_op_cat_loss(ptr(q_mats), ptr(qT), K, q_mats.shape[0], ptr(lg), ptr(lvt), ptr(lv0), ptr(tt), ptr(bb), n, ptr(row), ptr(dl),
                                   stream()))
        ctx.save_for_backward(dl)
        ctx.scale, ctx.dtype = 100.0 / max(n, 1), logits.dtype
        return torch.mean(row) * 100

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        gl = dl * (g * ctx.scale)
        return (gl if gl.dtype == ctx.dtype else gl.to(ctx.dtype)), None, None, None, None, None, None


def cat_loss(transition, logits, log_vt, log_v0, t, batch):
    """torch.mean(transition.compute_v_Lt(q_v_posterior(log_v0, log_vt), q_v_posterior(log_softmax(logits), log_vt), log_v0)) * 100"""
    return _CatLoss.apply(logits, transition.q_mats, transition.transpopse_q_onestep_mats, log_vt, log_v0, t, batch)
