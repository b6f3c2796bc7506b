// Host side of the training step in C++ (round 6): a pybind11 extension of the torch build in this image over the C ABI of
// libmoldiff_hip.so (include/moldiff_hip.h).  torch is plumbing here too: allocation, autograd edges, the current stream.
//   * The gradient sink and the weight-gradient queue, as C++ state.  They exist only here: train_ops.grad_sink / flush_grad_sink
//     forward to it, and every sink record and queue entry of every precision mode is made here.
//   * Linear, LayerNorm(+ReLU), Linear+LayerNorm+ReLU and the element-wise operators as torch::autograd::Function nodes: their ONE host
//     body, in every precision mode and on every route by which a parameter gradient leaves a backward (queued, recorded in the sink,
//     returned to autograd: weight_grad / ln_param_grads).  train_ops.linear / ln_relu / linear_ln_relu / ew are shells around them, and
//     train_ops.sgemm_nt / sgemm_tn / transpose / ... forward to the functions the nodes are made of.
//   * The ONE host body of each of the four fused row-owner operators (*_fwd / *_bwd: argument blocks, buffers, launches, segment sums),
//     in any mode that runs them.  Only the disposal of their parameter gradients has two routes: queued and recorded here when the
//     sink holds every parameter, else handed back to train_ops as lists of tensors (param_grads below).
// With these bodies in Python the host needed ~20 ms per step -- as long as the GPU (profiles/r6_train_host_profile.txt: a Linear node
// 32 us, a fused BondFFN node 110 us forward) -- for ~850 launches through ~190 autograd nodes.
// Reference lines replaced are those train_ops.py cites (models/common.py:181-201, models/graph.py:29-55,133-141,268-295,384-396).
#include <torch/extension.h>
#include <torch/csrc/autograd/custom_function.h>
#include <c10/hip/HIPStream.h>

#include <array>
#include <tuple>
#include <unordered_set>
#include <vector>

#include "../../include/moldiff_hip.h"
#include "mdx_train_plan.h"

namespace {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

inline void chk(int rc) {
  if (rc != 0) throw std::runtime_error(std::string("libmoldiff_hip error ") + std::to_string(rc) + ": " + mdx_last_error());
}
inline void* cur_stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }
inline void* P(const Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; }
inline int64_t A(const Tensor& t) { return t.defined() ? (int64_t)(uintptr_t)t.data_ptr() : 0; }
inline int H(const Tensor& t) { return (t.defined() && t.scalar_type() == at::kHalf) ? 1 : 0; }
inline const float* F32(const Tensor& t) { return reinterpret_cast<const float*>(t.data_ptr()); }
inline const int64_t* I64(const Tensor& t) { return reinterpret_cast<const int64_t*>(t.data_ptr()); }
inline void need_gpu(const Tensor& t) {
  TORCH_CHECK(!t.defined() || t.is_cuda(), "moldiff_amd runs on a ROCm device only (got a CPU tensor); there is no CPU fallback.");
}
// operand normalisation.  rows: fp32 or float16 container, unit column stride (row stride arbitrary: column slices of a weight stay views)
inline Tensor rows(const Tensor& t) {
  need_gpu(t);
  Tensor r = t;
  if (r.scalar_type() != at::kFloat && r.scalar_type() != at::kHalf) r = r.to(at::kFloat);
  return r.stride(-1) == 1 ? r : r.contiguous();
}
// tc: own container type (fp32 or float16; anything else is converted to fp32), contiguous
inline Tensor tc(const Tensor& t) {
  need_gpu(t);
  Tensor r = t;
  if (r.scalar_type() != at::kFloat && r.scalar_type() != at::kHalf) r = r.to(at::kFloat);
  return r.is_contiguous() ? r : r.contiguous();
}
// fc: fp32, contiguous
inline Tensor fc(const Tensor& t) {
  need_gpu(t);
  Tensor r = t.scalar_type() == at::kFloat ? t : t.to(at::kFloat);
  return r.is_contiguous() ? r : r.contiguous();
}
inline Tensor aligned_rows(const Tensor& t, int64_t ld_mult, int64_t ptr_mult) {
  Tensor r = rows(t);
  if (r.stride(0) % ld_mult || ((uintptr_t)r.data_ptr()) % ptr_mult) r = r.contiguous();
  return r;
}
inline Tensor half_empty(int64_t E, int64_t F, const Tensor& like) { return at::empty({E, F}, like.options().dtype(at::kHalf)); }

struct Job {
  Tensor g, x;
  int64_t plan[8];
  int64_t M, N, K, dt, dst_w, ldw, dst_b, rk;
};

// train_ops.TransposedParams: the flat parameter buffer's 2-D tensors, each transposed at its own offset of a second buffer
struct WtTable {
  int64_t base = 0, nbytes = 0, buf = 0;             // parameter buffer (address, bytes), transposed buffer (address)
  std::vector<int64_t> off;                          // sorted byte offsets of the entries in the parameter buffer
  std::vector<std::array<int64_t, 4>> ent;           // (element offset in the parameter buffer, R, C, element offset of W^T) per entry
};

struct State {
  // precision of the running step (train_ops._AMP): half kind (2 = float16), autocast, float16 containers
  int amp0 = 0, amp_auto = 0, amp_store = 0;
  // gradient sink
  bool sink = false;
  int64_t s_data = 0, s_grad = 0, s_nbytes = 0;
  std::vector<int64_t> recs, recs2;
  int64_t blocks = 0, blocks2 = 0;
  std::unordered_set<int64_t> seen;
  std::vector<Tensor> keep;
  Tensor like;  // any tensor of the sink's device (allocation options)
  // weight-gradient queue
  std::vector<Job> wq;
  int64_t wq_bytes = 0, wgrad_rows = 2048, wq_cap = (int64_t)24 << 30;
  bool wq_on = true;
  WtTable wt;          // transposed parameters of the running step (train_ops.transposed_params)
  Tensor wt_buf;       // ... their buffer, for the views handed to Python
  int64_t rows_min = 16384;   // train_ops.ROWS_MIN
  int64_t n_launch = 0;
} S;

// a node's backward runs in the precision of its forward (train_ops: `with precision(ctx.prec)`), whatever the mode is by then
inline int64_t amp_pack() { return S.amp0 | (S.amp_auto << 4) | (S.amp_store << 5); }
struct AmpGuard {
  int a0, a1, a2;
  explicit AmpGuard(int64_t packed) : a0(S.amp0), a1(S.amp_auto), a2(S.amp_store) {
    S.amp0 = (int)(packed & 15), S.amp_auto = (int)((packed >> 4) & 1), S.amp_store = (int)((packed >> 5) & 1);
  }
  ~AmpGuard() { S.amp0 = a0, S.amp_auto = a1, S.amp_store = a2; }
};

bool fast_mode() { return S.sink && S.amp0 == 2 && S.amp_auto && S.amp_store; }

int64_t sink_dst(const Tensor& t) {
  if (!S.sink || !t.defined()) return 0;
  const int64_t off = A(t) - S.s_data;
  return (off >= 0 && off < S.s_nbytes) ? S.s_grad + off : 0;
}

void flush_sink();

void sink_add(std::vector<int64_t>& recs, int64_t& counter, int64_t Pp, int64_t dst, int64_t Sn, int64_t rows_, int64_t cols, int64_t ld,
              int64_t pstride, int64_t rkind, int64_t nchunks = 1) {
  const int64_t r[8] = {Pp, dst, Sn, rows_, cols, ld, pstride, rkind | (counter << 8)};
  recs.insert(recs.end(), r, r + 8);
  counter += nchunks * red_blocks(rows_ * cols);
}

// one gradient record: a repeated destination flushes what is recorded first (the reduction's read-modify-writes are not atomic); more
// than RED_CHUNK partials take the two fixed-order stages of the per-layer reduction (a chunked record, then one over the chunk sums)
void sink_record(int64_t Pp, int64_t dst, int64_t Sn, int64_t rows_, int64_t cols, int64_t ld, int64_t pstride, int64_t rkind,
                 const Tensor& keep) {
  TORCH_CHECK(S.sink, "sink_record outside a gradient sink");
  if (S.seen.count(dst)) flush_sink();
  S.seen.insert(dst);
  if (Sn > RED_CHUNK) {
    const int64_t nc = ceil_div(Sn, RED_CHUNK);
    sink_add(S.recs, S.blocks, Pp, dst, Sn, rows_, cols, ld, pstride, 64, nc);
    sink_add(S.recs2, S.blocks2, Pp + 4 * red_chunk_plane(Sn, 0) * pstride, dst, nc, rows_, cols, ld, pstride, rkind);
  } else {
    sink_add(S.recs, S.blocks, Pp, dst, Sn, rows_, cols, ld, pstride, rkind);
  }
  if (keep.defined()) S.keep.push_back(keep);
}

Tensor to_device_i64(const std::vector<int64_t>& v) {
  Tensor host = at::empty({(int64_t)v.size()}, at::TensorOptions().dtype(at::kLong).pinned_memory(true));
  std::memcpy(host.data_ptr(), v.data(), v.size() * sizeof(int64_t));
  Tensor dev = at::empty({(int64_t)v.size()}, S.like.options().dtype(at::kLong));
  dev.copy_(host, /*non_blocking=*/true);
  S.keep.push_back(host);   // (until the next flush: the copy is asynchronous)
  return dev;
}

// run the queued weight gradients (one launch per tile class, the long blocks first) and hand their partials to the sink
void flush_wgrads() {
  if (!S.sink || S.wq.empty()) return;
  std::vector<Job> jobs;
  jobs.swap(S.wq);
  S.wq_bytes = 0;
  int64_t total = 0;
  for (auto& j : jobs) total += (j.plan[6] + 3) / 4 * 4;
  Tensor part = at::empty({total}, S.like.options().dtype(at::kFloat));
  const int64_t base = A(part);
  struct Placed { int64_t Pp, Sn, N, K, boff, dst_w, ldw, dst_b, rk; };
  std::vector<Placed> placed;
  placed.reserve(jobs.size());
  std::vector<std::array<int64_t, 16>> by_kind[8];
  int64_t off = 0;
  for (auto& j : jobs) {
    const int64_t kind = j.plan[0], gx = j.plan[1], gy = j.plan[2], Sn = j.plan[3], mper = j.plan[4], boff = j.plan[5], psize = j.plan[6],
                  blocks = j.plan[7];
    const int64_t Pp = base + 4 * off;
    by_kind[kind].push_back({A(j.g), A(j.x), Pp, j.dst_b ? Pp + 4 * boff : 0, j.g.stride(0), j.x.stride(0), j.M, j.N, j.K, mper, gx, gy, Sn,
                             j.dt, 0, blocks});
    placed.push_back({Pp, Sn, j.N, j.K, boff, j.dst_w, j.ldw, j.dst_b, j.rk});
    off += (psize + 3) / 4 * 4;
  }
  std::vector<int64_t> rows_;
  struct Launch { int kind; int64_t start, n, tb; };
  std::vector<Launch> launches;
  for (int kind = 0; kind < 8; ++kind) {
    auto& recs = by_kind[kind];
    if (recs.empty()) continue;
    std::stable_sort(recs.begin(), recs.end(), [](const std::array<int64_t, 16>& a, const std::array<int64_t, 16>& b) { return a[9] > b[9]; });
    int64_t fb = 0;
    for (auto& r : recs) {
      r[14] = fb;
      fb += r[15];
    }
    launches.push_back({kind, (int64_t)rows_.size() / 16, (int64_t)recs.size(), fb});
    for (auto& r : recs) rows_.insert(rows_.end(), r.begin(), r.end());
  }
  Tensor desc = to_device_i64(rows_);
  void* st = cur_stream();
  for (auto& l : launches) {
    chk(mdx_op_wgrad_grouped(reinterpret_cast<const int64_t*>(desc.data_ptr()) + 16 * l.start, (int32_t)l.n, l.tb, l.kind, st));
    ++S.n_launch;
  }
  S.keep.push_back(part);
  S.keep.push_back(desc);
  for (auto& p : placed) {
    sink_record(p.Pp, p.dst_w, p.Sn, p.N, p.K, p.ldw, p.N * p.K, p.rk, Tensor());
    if (p.dst_b) sink_record(p.Pp + 4 * p.boff, p.dst_b, p.Sn, 1, p.N, p.N, p.N, p.rk, Tensor());
  }
  S.keep.push_back(part);   // (again: a repeated destination above flushes the sink, which drops its references)
  S.keep.push_back(desc);
  // the operands (jobs) are released here: the launches above are enqueued, the allocator reuses memory in stream order
}

// every recorded gradient summed into its slot of the flat gradient buffer (train_ops.flush_grad_sink)
void flush_sink() {
  if (!S.sink) return;
  flush_wgrads();
  if (S.recs.empty()) return;
  void* st = cur_stream();
  std::vector<Tensor> descs;
  if (!S.recs.empty()) {
    Tensor d = to_device_i64(S.recs);
    chk(mdx_op_reduce_deferred(reinterpret_cast<const int64_t*>(d.data_ptr()), (int32_t)(S.recs.size() / 8), S.blocks, st));
    descs.push_back(d);
    ++S.n_launch;
  }
  if (!S.recs2.empty()) {
    Tensor d = to_device_i64(S.recs2);
    chk(mdx_op_reduce_deferred(reinterpret_cast<const int64_t*>(d.data_ptr()), (int32_t)(S.recs2.size() / 8), S.blocks2, st));
    descs.push_back(d);
    ++S.n_launch;
  }
  // the partial buffers may be reused once the launches above are enqueued (stream order).  The pinned staging tensors of THIS flush
  // stay referenced until the next one (their copies are asynchronous).
  std::vector<Tensor> staging;
  for (auto& t : S.keep)
    if (t.defined() && !t.is_cuda()) staging.push_back(t);
  S.keep.clear();
  for (auto& t : staging) S.keep.push_back(t);
  for (auto& t : descs) S.keep.push_back(t);
  S.recs.clear();
  S.recs2.clear();
  S.blocks = S.blocks2 = 0;
  S.seen.clear();
}

// queue one weight gradient dW = g^T x (+ bias column sums): the first route of weight_grad
void wq_append(const Tensor& g, const Tensor& x, int64_t dst_w, int64_t ldw, int64_t dst_b, int64_t rk) {
  TORCH_CHECK(S.sink && dst_w, "wq_append: no sink destination");
  TORCH_CHECK(g.stride(1) == 1 && x.stride(1) == 1, "wq_append: unit column stride expected");
  Job j;
  j.g = g, j.x = x;
  j.M = g.size(0), j.N = g.size(1), j.K = x.size(1);
  j.dt = H(g) | (H(x) << 1);
  const int aligned = (((uintptr_t)g.data_ptr()) % 16 == 0 && ((uintptr_t)x.data_ptr()) % 16 == 0) ? 1 : 0;
  const int64_t splits = std::max<int64_t>(1, (j.M + S.wgrad_rows - 1) / S.wgrad_rows);
  chk(mdx_op_wgrad_plan(j.M, j.N, j.K, (int32_t)splits, (int32_t)j.dt, g.stride(0), x.stride(0), aligned, j.plan));
  j.dst_w = dst_w, j.ldw = ldw, j.dst_b = dst_b, j.rk = rk;
  S.wq_bytes += g.numel() * g.element_size() + x.numel() * x.element_size();
  S.wq.push_back(std::move(j));
  if (S.wq_bytes > S.wq_cap) flush_wgrads();
}
inline int64_t rk_now() { return S.amp_auto ? S.amp0 : 0; }

// W^T of a parameter matrix or of a column slice of one as (pointer, leading dimension) in the transposed buffer of `T`; false if `w` is
// neither, or if its rows there would not start on 16 bytes (the GEMM's operand loads).  TransposedParams.view forwards here.
bool wt_view(const WtTable& T, const Tensor& w, int64_t& ptr, int64_t& ld) {
  if (!T.base || w.dim() != 2 || w.scalar_type() != at::kFloat || w.stride(1) != 1) return false;
  const int64_t rel = A(w) - T.base;
  if (rel < 0 || rel >= T.nbytes) return false;
  auto it = std::upper_bound(T.off.begin(), T.off.end(), rel);
  if (it == T.off.begin()) return false;
  const auto& e = T.ent[(it - T.off.begin()) - 1];
  const int64_t off = e[0], R = e[1], C = e[2], doff = e[3];
  const int64_t col = rel / 4 - off;
  if (col < 0 || col >= C || w.stride(0) != C || w.size(0) != R || col + w.size(1) > C) return false;
  const int64_t p = T.buf + 4 * (doff + col * R);
  if (p % 16) return false;
  ptr = p, ld = R;
  return true;
}
// w (R,C)^T as (pointer, leading dimension): a view into the step's transposed parameters where there is one, else one launch into a
// buffer whose rows are padded to a multiple of `pad` floats -- returned, to be kept until the consumer is enqueued
Tensor transposed(const Tensor& w, int64_t pad, int64_t& ptr, int64_t& ld) {
  if (wt_view(S.wt, w, ptr, ld)) return Tensor();
  need_gpu(w);
  const int64_t R = w.size(0), C = w.size(1);
  ld = (R + pad - 1) / pad * pad;
  Tensor buf = at::empty({C, ld}, w.options());
  chk(mdx_op_transpose(F32(w), w.stride(0), R, C, reinterpret_cast<float*>(buf.data_ptr()), ld, cur_stream()));
  ++S.n_launch;
  ptr = A(buf);
  return buf;
}

// ---- the GEMMs of a Linear, in the precision of the running step ---------------------------------------------------------------------------
// a (M,K) @ B (N,K; row stride ldb)^T + bias + addend -> (M,N).  An autocast mode takes mdx_op_xgemm_nt_t: a / addend fp32 or float16
// containers, the result in out_dtype (default: the mode's container, fp32 under keep32 -- a partial sum that enters another Linear as
// its addend and must not be rounded).  The fp32-exact mode, or splits > 1, takes mdx_op_sgemm_nt.
Tensor gemm_nt(const Tensor& a, const void* B, int64_t ldb, int64_t N, int64_t K, const Tensor& bias, const Tensor& addend, bool keep32,
               c10::optional<at::ScalarType> out_dtype, int64_t splits = 1) {
  need_gpu(a);
  const int64_t M = a.size(0);
  const float* Bf = reinterpret_cast<const float*>(B);
  if (S.amp0 && splits <= 1) {
    const at::ScalarType od = out_dtype ? *out_dtype : (keep32 ? at::kFloat : (S.amp_store ? at::kHalf : at::kFloat));
    Tensor out = at::empty({M, N}, a.options().dtype(od));
    const int rnd = ((S.amp_auto && !keep32) || od == at::kHalf) ? 1 : 0;
    chk(mdx_op_xgemm_nt_t(a.data_ptr(), a.stride(0), Bf, ldb, reinterpret_cast<const float*>(P(bias)), P(addend),
                          addend.defined() ? addend.stride(0) : 0, out.data_ptr(), N, M, N, K, S.amp0, rnd, H(a) | (H(addend) << 1) | (H(out) << 2),
                          cur_stream()));
    ++S.n_launch;
    return out;
  }
  TORCH_CHECK(a.scalar_type() == at::kFloat && (!addend.defined() || addend.scalar_type() == at::kFloat), "fp32 GEMM: fp32 operands expected");
  Tensor out = at::empty({M, N}, a.options());
  Tensor part = splits > 1 ? at::empty({splits * M * N}, a.options()) : Tensor();
  chk(mdx_op_sgemm_nt(F32(a), a.stride(0), Bf, ldb, reinterpret_cast<const float*>(P(bias)), reinterpret_cast<const float*>(P(addend)),
                      addend.defined() ? addend.stride(0) : 0, reinterpret_cast<float*>(out.data_ptr()), N, M, N, K, (int32_t)splits,
                      reinterpret_cast<float*>(P(part)), cur_stream()));
  ++S.n_launch;
  return out;
}

// Can a (M,k) @ W -> (M,n) take the row-owner kernel (csrc/mdx_linear_rows.hip)?  fp32 mode, shape built, enough rows, 16-byte aligned rows.
bool linear_rows_ok(const Tensor& a, int64_t n, int64_t k, const Tensor& addend) {
  auto aligned = [](const Tensor& t) { return t.stride(1) == 1 && t.stride(0) % 4 == 0 && A(t) % 16 == 0; };
  return !S.amp0 && a.scalar_type() == at::kFloat && a.size(0) >= S.rows_min && aligned(a) && (!addend.defined() || aligned(addend)) &&
         mdx_op_linear_rows_supported(n, k) == 1;
}
// a (M,K) @ W^T (W (N,K), trans_w = false) or a @ W (W (K,N), trans_w = true) + bias + addend -> (M,N) on the row-owner kernel
Tensor linear_rows(const Tensor& a, const Tensor& w, bool trans_w, const Tensor& bias, const Tensor& addend) {
  need_gpu(a), need_gpu(w);
  const int64_t M = a.size(0), K = a.size(1), N = trans_w ? w.size(1) : w.size(0);
  TORCH_CHECK(w.stride(1) == 1 && (trans_w ? w.size(0) : w.size(1)) == K, "linear_rows: weight shape");
  Tensor out = at::empty({M, N}, a.options());
  Tensor ws = at::empty({(int64_t)(mdx_op_linear_rows_ws(N, K) / 4)}, a.options());
  chk(mdx_op_linear_rows(F32(a), a.stride(0), F32(w), w.stride(0), trans_w ? 1 : 0, reinterpret_cast<const float*>(P(bias)),
                         reinterpret_cast<const float*>(P(addend)), addend.defined() ? addend.stride(0) : 0,
                         reinterpret_cast<float*>(out.data_ptr()), N, M, N, K, reinterpret_cast<float*>(ws.data_ptr()), cur_stream()));
  ++S.n_launch;
  return out;
}
// column sums of x (M,N), times y element-wise where given
Tensor colreduce(const Tensor& x, const Tensor& y) {
  need_gpu(x);
  const int64_t M = x.size(0), N = x.size(1);
  Tensor out = at::empty({N}, x.options());
  Tensor ws = M > 512 ? at::empty({(M + 511) / 512 * N}, x.options()) : Tensor();
  chk(mdx_op_colreduce(F32(x), reinterpret_cast<const float*>(P(y)), x.stride(0), M, N, reinterpret_cast<float*>(out.data_ptr()),
                       reinterpret_cast<float*>(P(ws)), cur_stream()));
  ++S.n_launch;
  return out;
}

// Row ranges of a weight gradient launched on its own (the contraction runs over `rows`): enough of them to fill the chip with workgroups,
// each >= 128 rows.  fp32 / converting kernels: 64 x 64 tiles, ~1024 workgroups (flat between 512 and 4096; each loops over its rows in
// short steps, many short loops hide the load latency better than few long ones).  float16 containers with tile-aligned widths take the
// transpose-read kernel (csrc hgemm_tn_tr_kernel): 128-wide tiles where the layer allows, ~512 workgroups = one resident set (two per
// CU); more ranges mean more split partials to write and reduce (measured per step: 384 -> 34.2, 512 -> 33.5, 768 -> 34.1, 1024 -> 34.8 ms).
int64_t splits_for(int64_t rows_, int64_t n, int64_t k, bool half) {
  const bool tr = half && n % 64 == 0 && k % 64 == 0;
  const int64_t tiles = tr ? (n / (n % 128 == 0 ? 128 : 64)) * (k / (k % 128 == 0 ? 128 : 64)) : ((n + 63) / 64) * ((k + 63) / 64);
  const int64_t wgs = tr ? 512 : 1024;
  return std::max<int64_t>(1, std::min(rows_ / 128, (wgs + tiles - 1) / tiles));
}

// ---- the routes by which a parameter gradient leaves a backward -----------------------------------------------------------------------------
// The weight gradient dW (N,K) = g (M,N)^T x (M,K), with want_bias also db = the column sums of g from the same pass.  dst_w / dst_b are
// the parameters' slots in the flat gradient buffer (sink_dst; ldw: row stride of the weight there), 0 = the parameter is in no sink:
//   * a destination, float16 kind, queue on, unit column strides: QUEUED for the grouped launch (wq_append) -> {};
//   * a destination otherwise: launched now over `splits` row ranges, the split partials RECORDED for the sink's reduction -> {};
//   * no destination: launched now and RETURNED -> {dW, db}.
std::pair<Tensor, Tensor> weight_grad(const Tensor& g, const Tensor& x, int64_t splits, bool want_bias, int64_t dst_w, int64_t ldw,
                                      int64_t dst_b) {
  need_gpu(g), need_gpu(x);
  const int64_t M = g.size(0), N = g.size(1), K = x.size(1);
  splits = std::max<int64_t>(1, splits);
  if (dst_w && S.wq_on && S.sink && S.amp0 == 2 && g.stride(1) == 1 && x.stride(1) == 1) {
    wq_append(g, x, dst_w, ldw, want_bias ? dst_b : 0, rk_now());
    return {};
  }
  const auto f32 = g.options().dtype(at::kFloat);
  const SplitLayout L = split_layout(M, N, K, splits, S.amp0 ? HW_MC : W_MC);   // (what the two kernels below compute for themselves)
  Tensor part = at::empty({L.total}, f32), dW, db;
  float* pp = reinterpret_cast<float*>(part.data_ptr());
  if (!dst_w) dW = at::empty({N, K}, f32), db = want_bias ? at::empty({N}, f32) : Tensor();
  float* pw = reinterpret_cast<float*>(P(dW));
  float* pb = dst_w ? (want_bias ? pp : nullptr) : reinterpret_cast<float*>(P(db));   // (deferred: any non-null pointer asks for the bias partials)
  if (S.amp0) {
    chk(mdx_op_xgemm_tn_t(g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), pw, K, pb, M, N, K, (int32_t)splits, pp, S.amp0, S.amp_auto,
                          H(g) | (H(x) << 1), cur_stream()));
  } else {
    TORCH_CHECK(g.scalar_type() == at::kFloat && x.scalar_type() == at::kFloat, "fp32 weight gradient: fp32 operands expected");
    chk(mdx_op_sgemm_tn(F32(g), g.stride(0), F32(x), x.stride(0), pw, K, pb, M, N, K, (int32_t)splits, pp, cur_stream()));
  }
  ++S.n_launch;
  if (dst_w) {
    sink_record(A(part), dst_w, L.S, N, K, ldw, N * K, rk_now(), part);
    if (want_bias) sink_record(A(part) + 4 * L.bias_off, dst_b, L.S, 1, N, N, N, rk_now(), part);
  }
  return {dW, db};
}
// ... of a Linear with parameters w (and b): deferred when the sink holds every parameter the gradient is wanted for
std::pair<Tensor, Tensor> linear_param_grads(const Tensor& gy, const Tensor& x, const Tensor& w, const Tensor& b, bool want_b) {
  int64_t dst_w = sink_dst(w), dst_b = want_b ? sink_dst(b) : 0;
  if (!dst_w || (want_b && !dst_b)) dst_w = dst_b = 0;
  const int64_t splits = splits_for(x.size(0), gy.size(1), x.size(1), H(gy) && H(x) && S.amp0 == 2);
  return weight_grad(gy, x, splits, want_b, dst_w, w.stride(0), dst_b);
}

// [dgamma | dbeta] of a LayerNorm over F features of M rows.  launch(dgb, ws) runs the backward kernel, which leaves one partial row of
// 2F floats per workgroup in ws and, where dgb is not null, their sum in dgb.  Both parameters in the sink (and ws on 16 bytes): dgb is
// null and the partial rows are RECORDED for the sink's reduction -> {}; otherwise RETURNED -> {dgamma, dbeta}.
template <class Launch>
std::pair<Tensor, Tensor> ln_param_grads(int64_t M, int64_t F, const Tensor& gamma, const Tensor& beta, const Tensor& like, Launch launch) {
  const auto f32 = like.options().dtype(at::kFloat);
  Tensor ws = at::empty({ln_bwd_ws_floats(M, F) + 1}, f32);
  const int64_t dst_g = sink_dst(gamma), dst_b = sink_dst(beta);
  const bool defer = dst_g && dst_b && M > 0 && A(ws) % 16 == 0;
  Tensor dgb = defer ? Tensor() : at::empty({2 * F}, f32);
  launch(reinterpret_cast<float*>(P(dgb)), reinterpret_cast<float*>(ws.data_ptr()));
  ++S.n_launch;
  if (!defer) return {dgb.narrow(0, 0, F), dgb.narrow(0, F, F)};
  const int64_t nrows = ln_bwd_rows(M);
  sink_record(A(ws), dst_g, nrows, 1, F, F, 2 * F, 0, ws);
  sink_record(A(ws) + 4 * F, dst_b, nrows, 1, F, F, 2 * F, 0, ws);
  return {};
}

// ---- Linear: y = x w^T + b + addend -----------------------------------------------------------------------------------------------------
// What a Linear's backward needs: the normalised operands, which inputs were there, their container types.  lin_save / lin_load carry it
// through a node whose saved variables start with [x, w, b] and whose tensor arguments start with x, w, [b], [addend].
struct LinCtx {
  Tensor x, w, b;            // (b: the parameter view, for its sink address)
  bool has_bias = false, has_addend = false, need_x = false, need_w = false, need_b = false, need_add = false;
  at::ScalarType x_dtype = at::kFloat, add_dtype = at::kFloat;
};
inline bool given(const c10::optional<Tensor>& t) { return t && t->defined(); }
void lin_save(AutogradContext* ctx, const Tensor& x, const c10::optional<Tensor>& b, const c10::optional<Tensor>& addend) {
  ctx->saved_data["f"] = (int64_t)(given(b) | (given(addend) << 1));
  ctx->saved_data["xd"] = (int64_t)x.scalar_type();
  ctx->saved_data["ad"] = (int64_t)(given(addend) ? addend->scalar_type() : at::kFloat);
}
LinCtx lin_load(AutogradContext* ctx, const variable_list& sv) {
  LinCtx c;
  c.x = sv[0], c.w = sv[1], c.b = sv[2];
  const int64_t f = ctx->saved_data["f"].toInt();
  c.has_bias = f & 1, c.has_addend = f & 2;
  // (needs_input_grad counts the TENSOR arguments that were present: x, w, [b], [addend], ...)
  c.need_x = ctx->needs_input_grad(0), c.need_w = ctx->needs_input_grad(1);
  c.need_b = c.has_bias && ctx->needs_input_grad(2);
  c.need_add = c.has_addend && ctx->needs_input_grad(2 + (c.has_bias ? 1 : 0));
  c.x_dtype = (at::ScalarType)ctx->saved_data["xd"].toInt();
  c.add_dtype = (at::ScalarType)ctx->saved_data["ad"].toInt();
  return c;
}
struct LinOps { Tensor x, w, b, addend; };
LinOps linear_operands(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, const c10::optional<Tensor>& addend) {
  LinOps o{rows(x), rows(w), given(b) ? fc(*b) : Tensor(), Tensor()};
  TORCH_CHECK(o.x.dim() == 2 && o.w.dim() == 2 && o.w.scalar_type() == at::kFloat, "linear: 2-D input and fp32 2-D weight expected");
  if (!S.amp0 && o.x.scalar_type() != at::kFloat) o.x = o.x.to(at::kFloat);
  if (given(addend)) o.addend = S.amp0 ? rows(*addend) : fc(*addend);
  return o;
}

struct LinGrads { Tensor gx, gw, gb, ga; };
// data gradient, weight (+ bias) gradient by its route, addend gradient of one Linear
LinGrads linear_backward(const LinCtx& c, const Tensor& gy_in) {
  LinGrads r;
  Tensor gy = S.amp0 ? tc(gy_in) : fc(gy_in);
  const int64_t N = c.w.size(0), K = c.w.size(1);
  if (c.need_x) {
    if (linear_rows_ok(gy, K, N, Tensor())) {
      r.gx = linear_rows(gy, c.w, true, Tensor(), Tensor());          // (M,N) @ (N,K), the weight read transposed by the pack
    } else {                                                          // (M,N) @ (K,N)^T; the gradient lives in x's container type
      int64_t wtp = 0, wtld = 0;
      Tensor keep = transposed(c.w, 4, wtp, wtld);
      r.gx = gemm_nt(gy, (const void*)wtp, wtld, K, N, Tensor(), Tensor(), false,
                     S.amp0 ? c10::optional<at::ScalarType>(c.x.scalar_type()) : c10::nullopt);
    }
    if (r.gx.scalar_type() != c.x_dtype) r.gx = r.gx.to(c.x_dtype);
  }
  if (c.need_w) {
    std::tie(r.gw, r.gb) = linear_param_grads(gy, c.x, c.w, c.b, c.need_b);
  } else if (c.need_b) {
    r.gb = colreduce(gy.scalar_type() == at::kFloat ? gy : gy.to(at::kFloat), Tensor());
  }
  if (c.need_add) r.ga = gy.scalar_type() == c.add_dtype ? gy : gy.to(c.add_dtype);
  return r;
}

class LinearFn : public torch::autograd::Function<LinearFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b,
                        const c10::optional<Tensor>& addend, bool keep32) {
    const LinOps o = linear_operands(x, w, b, addend);
    const int64_t N = o.w.size(0), K = o.w.size(1);
    Tensor out = linear_rows_ok(o.x, N, K, o.addend) ? linear_rows(o.x, o.w, false, o.b, o.addend)
                                                     : gemm_nt(o.x, o.w.data_ptr(), o.w.stride(0), N, K, o.b, o.addend, keep32, c10::nullopt);
    ctx->save_for_backward({o.x, o.w, given(b) ? *b : Tensor()});
    lin_save(ctx, x, b, addend);
    ctx->saved_data["amp"] = amp_pack();
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    AmpGuard guard(ctx->saved_data["amp"].toInt());
    const LinGrads r = linear_backward(lin_load(ctx, ctx->get_saved_variables()), grads[0]);
    return {r.gx, r.gw, r.gb, r.ga, Tensor()};
  }
};

// ---- LayerNorm (+ReLU) ---------------------------------------------------------------------------------------------------------------------
inline bool ln_half_width(int64_t F) { return F == 32 || F == 64 || F == 128 || F == 256; }   // the widths the float16 kernels cover
struct LnFwd { Tensor x, g, b, y, stats; };
LnFwd ln_forward(const Tensor& x, const Tensor& gamma, const Tensor& beta, bool relu) {
  LnFwd r{tc(x), fc(gamma), fc(beta), Tensor(), Tensor()};
  const int64_t M = r.x.size(0), F = r.x.size(1);
  if (!ln_half_width(F) && r.x.scalar_type() != at::kFloat) r.x = r.x.to(at::kFloat);
  // the only consumers of a LayerNorm result are Linears, which round their operand to half anyway: a half container is exact
  r.y = at::empty({M, F}, r.x.options().dtype((S.amp0 && S.amp_store && ln_half_width(F)) ? at::kHalf : at::kFloat));
  r.stats = at::empty({M, 2}, r.x.options().dtype(at::kFloat));
  chk(mdx_op_ln_relu_fwd_t(r.x.data_ptr(), F32(r.g), F32(r.b), M, (int32_t)F, relu ? 1 : 0, r.y.data_ptr(),
                           reinterpret_cast<float*>(r.stats.data_ptr()), H(r.x) | (H(r.y) << 1), cur_stream()));
  ++S.n_launch;
  return r;
}
struct LnGrads { Tensor dx, dgamma, dbeta; };
// x, g, b: the normalised operands of the forward; gamma, beta: the parameters themselves (their sink addresses)
LnGrads ln_backward(const Tensor& gy_in, const Tensor& x, const Tensor& stats, const Tensor& g, const Tensor& b, const Tensor& gamma,
                    const Tensor& beta, int relu) {
  LnGrads r;
  Tensor gy = tc(gy_in);
  const int64_t M = x.size(0), F = x.size(1);
  if (!ln_half_width(F) && gy.scalar_type() != at::kFloat) gy = gy.to(at::kFloat);
  r.dx = at::empty_like(x);
  std::tie(r.dgamma, r.dbeta) = ln_param_grads(M, F, gamma, beta, x, [&](float* dgb, float* ws) {
    chk(mdx_op_ln_relu_bwd_t(gy.data_ptr(), x.data_ptr(), F32(stats), F32(g), F32(b), M, (int32_t)F, relu, r.dx.data_ptr(), dgb, ws,
                             H(gy) | (H(x) << 1) | (H(r.dx) << 2), cur_stream()));
  });
  return r;
}

class LnReluFn : public torch::autograd::Function<LnReluFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& gamma, const Tensor& beta, bool relu) {
    const LnFwd f = ln_forward(x, gamma, beta, relu);
    ctx->save_for_backward({f.x, f.g, f.b, f.stats, gamma, beta});
    ctx->saved_data["relu"] = relu;
    ctx->saved_data["xd"] = (int64_t)x.scalar_type();
    return f.y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto sv = ctx->get_saved_variables();
    LnGrads r = ln_backward(grads[0], sv[0], sv[3], sv[1], sv[2], sv[4], sv[5], ctx->saved_data["relu"].toBool() ? 1 : 0);
    const auto xd = (at::ScalarType)ctx->saved_data["xd"].toInt();
    return {r.dx.scalar_type() == xd ? r.dx : r.dx.to(xd), r.dgamma, r.dbeta, Tensor()};
  }
};

// ---- Linear + LayerNorm + ReLU as one launch forward (the LayerNorm runs in the GEMM's epilogue, csrc hgemm_nt_rows_kernel<.., LN>): the
// first two layers of every common.MLP (reference models/common.py:191-196).  The Linear's result and the row statistics are stored for
// the backward, which is the LayerNorm's backward followed by the Linear's.
// Is the fused launch built for this call?  float16 mode with float16 containers, float16 rows of x, widths of the row-owner kernel.
bool linear_ln_ok(const Tensor& x, const Tensor& w, const Tensor& addend) {
  if (S.amp0 != 2 || !S.amp_store || x.scalar_type() != at::kHalf || x.dim() != 2 || w.dim() != 2) return false;
  return mdx_op_xgemm_nt_ln_supported(x.size(0), w.size(0), x.size(1)) == 1 && x.stride(1) == 1 && x.stride(0) % 8 == 0 && A(x) % 16 == 0 &&
         w.stride(1) == 1 && (!addend.defined() || (addend.dim() == 2 && addend.stride(1) == 1));
}
struct LinLnFwd { LinOps o; Tensor g, bt, pre, post, stats; };
LinLnFwd linear_ln_forward(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, const c10::optional<Tensor>& addend,
                           const Tensor& gamma, const Tensor& beta) {
  LinLnFwd r{linear_operands(x, w, b, addend), fc(gamma), fc(beta), Tensor(), Tensor(), Tensor()};
  const Tensor &xc = r.o.x, &wc = r.o.w, &ac = r.o.addend;
  const int64_t M = xc.size(0), K = xc.size(1), N = wc.size(0);
  r.pre = half_empty(M, N, xc), r.post = half_empty(M, N, xc);
  r.stats = at::empty({M, 2}, xc.options().dtype(at::kFloat));
  chk(mdx_op_xgemm_nt_ln_t(xc.data_ptr(), xc.stride(0), F32(wc), wc.stride(0), reinterpret_cast<const float*>(P(r.o.b)), P(ac),
                           ac.defined() ? ac.stride(0) : 0, r.pre.data_ptr(), N, F32(r.g), F32(r.bt), r.post.data_ptr(), N,
                           reinterpret_cast<float*>(r.stats.data_ptr()), 1, M, N, K, S.amp0, 1, 1 | (H(ac) << 1) | 4 | 8, cur_stream()));
  ++S.n_launch;
  return r;
}

class LinearLnReluFn : public torch::autograd::Function<LinearLnReluFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b,
                        const c10::optional<Tensor>& addend, const Tensor& gamma, const Tensor& beta) {
    const LinLnFwd f = linear_ln_forward(x, w, b, addend, gamma, beta);
    ctx->save_for_backward({f.o.x, f.o.w, given(b) ? *b : Tensor(), f.pre, f.g, f.bt, f.stats, gamma, beta});
    lin_save(ctx, x, b, addend);
    ctx->saved_data["amp"] = amp_pack();
    return f.post;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    AmpGuard guard(ctx->saved_data["amp"].toInt());
    auto sv = ctx->get_saved_variables();
    const LnGrads n = ln_backward(grads[0], sv[3], sv[6], sv[4], sv[5], sv[7], sv[8], 1);
    const LinGrads r = linear_backward(lin_load(ctx, sv), n.dx);
    return {r.gx, r.gw, r.gb, r.ga, n.dgamma, n.dbeta};
  }
};

// ---- Linear + LayerNorm + ReLU + Linear to ONE output (common.MLP of PosUpdate's inter module: 256 -> 256 -> 1) -----------------------------
// forward: the fused Linear+LayerNorm launch, then the row dot as a GEMM with N = 1.  backward: the second Linear's weight gradient by its
// route, its data gradient is the rank-1 product g1[row] * w2[c], formed INSIDE the LayerNorm backward (mdx_op_ln_relu_bwd_r1_t): the
// (E,256) gradient tensor, the K = 1 GEMM and the weight transpose of the per-operator path are gone.  That kernel leaves the LayerNorm
// parameter gradients as partial rows only, so the node runs where they are deferred: the float16 sink with every parameter in it.
class LinearLnReluDotFn : public torch::autograd::Function<LinearLnReluDotFn> {
 public:
  static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& w, const Tensor& b, const Tensor& gamma, const Tensor& beta,
                        const Tensor& w2, const Tensor& b2) {
    const LinLnFwd f = linear_ln_forward(x, w, b, c10::nullopt, gamma, beta);
    Tensor w2c = rows(w2), b2c = fc(b2);
    const int64_t N = f.o.w.size(0);
    TORCH_CHECK(w2c.size(0) == 1 && w2c.size(1) == N, "linear_ln_relu_dot: second weight must be (1, N)");
    Tensor y = gemm_nt(f.post, w2c.data_ptr(), w2c.stride(0), 1, N, b2c, Tensor(), false, c10::nullopt);
    ctx->save_for_backward({f.o.x, f.o.w, b, f.pre, f.g, f.bt, f.stats, gamma, beta, f.post, w2c, b2, w2});
    lin_save(ctx, x, b, c10::nullopt);
    ctx->saved_data["amp"] = amp_pack();
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    AmpGuard guard(ctx->saved_data["amp"].toInt());
    auto sv = ctx->get_saved_variables();
    const Tensor &pre = sv[3], &g = sv[4], &bt = sv[5], &stats = sv[6], &post = sv[9], &w2c = sv[10];
    Tensor gy = tc(grads[0]);                                  // (M,1)
    const int64_t M = pre.size(0), F = pre.size(1);
    Tensor gw2, gb2, gg, gbt;
    std::tie(gw2, gb2) = linear_param_grads(gy, post, sv[12], sv[11], true);
    // LayerNorm backward with the rank-1 upstream gradient
    Tensor gpre = at::empty_like(pre);
    std::tie(gg, gbt) = ln_param_grads(M, F, sv[7], sv[8], pre, [&](float* dgb, float* ws) {
      TORCH_CHECK(!dgb, "linear_ln_relu_dot: LayerNorm parameters left the gradient sink between forward and backward");
      chk(mdx_op_ln_relu_bwd_r1_t(gy.data_ptr(), F32(w2c), pre.data_ptr(), F32(stats), F32(g), F32(bt), M, (int32_t)F, 1, gpre.data_ptr(), ws,
                                  H(gy) | (H(pre) << 1) | (H(gpre) << 2), cur_stream()));
    });
    const LinGrads r = linear_backward(lin_load(ctx, sv), gpre);     // first Linear
    return {r.gx, r.gw, r.gb, gg, gbt, gw2, gb2};
  }
};
// inside the float16 sink (queue on), is `p` a trained parameter held by the sink?
inline bool sunk(const Tensor& p) { return sink_dst(p) && p.requires_grad(); }
bool linear_fast_ok(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b) {
  return fast_mode() && S.wq_on && x.dim() == 2 && w.dim() == 2 && x.is_cuda() && w.scalar_type() == at::kFloat && w.stride(1) == 1 && sunk(w) &&
         (!given(b) || sunk(*b));
}
// does the rank-1 dot form apply?  (see LinearLnReluDotFn)
bool linear_ln_dot_fast_ok(const Tensor& x, const Tensor& w, const Tensor& b, const Tensor& gamma, const Tensor& beta, const Tensor& w2,
                           const Tensor& b2) {
  if (!linear_fast_ok(x, w, b) || !sunk(gamma) || !sunk(beta) || !sunk(w2) || !sunk(b2)) return false;
  const int64_t F = w.size(0);
  return w2.dim() == 2 && w2.size(0) == 1 && w2.size(1) == F && w2.stride(1) == 1 && ln_half_width(F) && x.scalar_type() == at::kHalf;
}

// ---- what train_ops calls ---------------------------------------------------------------------------------------------------------------------
inline Tensor opt(const c10::optional<Tensor>& t) { return given(t) ? *t : Tensor(); }
Tensor linear(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, const c10::optional<Tensor>& addend, bool keep32) {
  return LinearFn::apply(x, w, b, addend, keep32);
}
// relu(LayerNorm(x @ w.T + b + addend)): one launch where the fused kernel is built, the two operators otherwise
Tensor linear_ln_relu(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, const c10::optional<Tensor>& addend, const Tensor& gamma,
                      const Tensor& beta) {
  if (linear_ln_ok(x, w, opt(addend))) return LinearLnReluFn::apply(x, w, b, addend, gamma, beta);
  return LnReluFn::apply(linear(x, w, b, addend, false), gamma, beta, true);
}
// linear(relu(LayerNorm(x @ w.T + b)), w2, b2) with w2 of ONE row: one node where the rank-1 dot form applies, else the operators
Tensor linear_ln_relu_dot(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, const Tensor& gamma, const Tensor& beta,
                          const Tensor& w2, const c10::optional<Tensor>& b2) {
  if (given(b) && given(b2) && linear_ln_ok(x, w, Tensor()) && linear_ln_dot_fast_ok(x, w, *b, gamma, beta, w2, *b2))
    return LinearLnReluDotFn::apply(x, w, *b, gamma, beta, w2, *b2);
  return linear(linear_ln_relu(x, w, b, c10::nullopt, gamma, beta), w2, b2, c10::nullopt, false);
}

// ---- element-wise: add 0, sub 1, mul 2, gate 3 ------------------------------------------------------------------------------------------------
class EwFn : public torch::autograd::Function<EwFn> {
 public:
  static Tensor forward(AutogradContext* ctx, int64_t op, const Tensor& a, const Tensor& b) {
    // one container type for both operands (mixed -> fp32; any length: the library falls back to its scalar kernels when the 4-wide
    // float16 ones do not apply)
    Tensor ac = tc(a), bc = tc(b);
    if (ac.scalar_type() != bc.scalar_type()) ac = ac.to(at::kFloat), bc = bc.to(at::kFloat);
    TORCH_CHECK(ac.sizes() == bc.sizes(), "element-wise operands differ in shape");
    Tensor out = at::empty_like(ac);
    const int64_t rk = (op == 2 || op == 3) ? rk_now() : 0;     // autocast: a product of two half tensors is a half tensor
    chk(mdx_op_ew_fwd_t((int32_t)(op | (rk << 8)), ac.data_ptr(), bc.data_ptr(), out.data_ptr(), ac.numel(), H(ac) | (H(bc) << 1) | (H(out) << 2),
                        cur_stream()));
    ++S.n_launch;
    ctx->save_for_backward({ac, bc});
    ctx->saved_data["op"] = op;
    ctx->saved_data["da"] = (int64_t)a.scalar_type();
    ctx->saved_data["db"] = (int64_t)b.scalar_type();
    return out;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    auto sv = ctx->get_saved_variables();
    const Tensor &a = sv[0], &b = sv[1];
    Tensor g = tc(grads[0]);
    Tensor da = ctx->needs_input_grad(0) ? at::empty_like(a) : Tensor();     // (indices over the tensor arguments: a, b)
    Tensor db = ctx->needs_input_grad(1) ? at::empty_like(b) : Tensor();
    chk(mdx_op_ew_bwd_t((int32_t)ctx->saved_data["op"].toInt(), a.data_ptr(), b.data_ptr(), g.data_ptr(), P(da), P(db), a.numel(),
                        H(a) | (H(b) << 1) | (H(g) << 2) | (H(da) << 3) | (H(db) << 4), cur_stream()));
    ++S.n_launch;
    const auto ta = (at::ScalarType)ctx->saved_data["da"].toInt(), tb = (at::ScalarType)ctx->saved_data["db"].toInt();
    if (da.defined() && da.scalar_type() != ta) da = da.to(ta);
    if (db.defined() && db.scalar_type() != tb) db = db.to(tb);
    return {Tensor(), da, db};
  }
};

// ---- segment sum / gather bodies (train_ops._segsum_raw / _gather_raw) ------------------------------------------------------------------
Tensor segsum_raw(const Tensor& src, const Tensor& order, const Tensor& ptr, int64_t n, bool out_half) {
  const int64_t F = src.size(1);
  Tensor out = at::empty({n, F}, src.options().dtype(out_half ? at::kHalf : at::kFloat));
  chk(mdx_op_segsum_rows_t(src.data_ptr(), I64(order), I64(ptr), n, (int32_t)F, out.data_ptr(), H(src) | (H(out) << 1), cur_stream()));
  ++S.n_launch;
  return out;
}

// ---- the four fused row-owner operators (csrc/mdx_train_fused.hip): the one host body of each ------------------------------------------
// train_ops._BondFfnScatter / _EdgeTail / _PosFfnFront / _NodeMsg are autograd shells around *_fwd / *_bwd below; nothing else fills a
// fused operator's argument block.  The forward halves need neither a sink nor the float16 sink mode.  A backward half launches, then
// disposes of the parameter gradients by one of two routes (param_grads), then runs the segment sums.
void check_params(const std::vector<Tensor>& p) {
  for (auto& t : p) TORCH_CHECK(t.scalar_type() == at::kFloat && t.stride(-1) == 1, "fused operator: fp32 parameters with unit column stride expected");
}
// one partial row of LayerNorm-parameter gradients per workgroup of a fused backward
inline Tensor lnp_empty(int64_t lnf, const Tensor& like) { return at::empty({mdx_op_bondffn_workgroups(), lnf}, like.options().dtype(at::kFloat)); }
inline Tensor seg(bool need, const Tensor& src, const Tensor& order, const Tensor& ptr, int64_t n, bool out_half) {
  return need ? segsum_raw(src, order, ptr, n, out_half) : Tensor();
}
bool all_in_sink(const std::vector<Tensor>& ps) {
  if (!fast_mode() || !S.wq_on) return false;
  for (auto& p : ps)
    if (!sink_dst(p) || !p.requires_grad()) return false;
  return true;
}

// The parameter-gradient work of a fused backward, stated once per operator as two tables over its parameter list `p`:
struct WGrad { int gy, xin, w, b; };      // dW[w] = ops[gy]^T ops[xin], its column sums -> bias b (-1: none); ops = the backward's operand list
struct LnSlice { int p, off, width; };    // d p = column sums of lnp[:, off : off + width]
// dispose (every parameter in the sink, float16 sink mode: all_in_sink): the contractions are queued and the slices recorded here, in table
// order -> None.  Otherwise the tables resolved to tensors, for train_ops._fused_param_grads to defer or return each through autograd:
// ([(gy, xin, w, b)], lnp, [(p, off, width)]).
template <size_t NW, size_t NL>
py::object param_grads(bool dispose, const std::vector<Tensor>& p, const Tensor* const* ops, const WGrad (&wgs)[NW], const LnSlice (&lns)[NL],
                       const Tensor& lnp) {
  if (!dispose) {
    std::vector<std::tuple<Tensor, Tensor, int, int>> cs;
    std::vector<std::tuple<int, int, int>> ls;
    for (auto& c : wgs) cs.emplace_back(*ops[c.gy], *ops[c.xin], c.w, c.b);
    for (auto& s : lns) ls.emplace_back(s.p, s.off, s.width);
    return py::make_tuple(cs, lnp, ls);
  }
  for (auto& c : wgs) {
    const Tensor& w = p[c.w];
    const int64_t dst_w = sink_dst(w), dst_b = c.b >= 0 ? sink_dst(p[c.b]) : 0;
    TORCH_CHECK(dst_w && (c.b < 0 || dst_b), "fused backward: weight not in the gradient sink");
    wq_append(*ops[c.gy], *ops[c.xin], dst_w, w.stride(0), dst_b, rk_now());
  }
  for (auto& s : lns) {
    const int64_t dst = sink_dst(p[s.p]);
    TORCH_CHECK(dst, "fused backward: LayerNorm parameter not in the gradient sink");
    sink_record(A(lnp) + 4 * s.off, dst, lnp.size(0), 1, s.width, s.width, lnp.size(1), 0, lnp);
  }
  return py::none();
}
// what a *_bwd returns: [g_x, g_a, g_b] after disposal here, else ([g_x, g_a, g_b], contractions, lnp, slices)
inline py::object bwd_result(const py::object& tables, std::vector<Tensor> grads) {
  return tables.is_none() ? py::cast(grads) : py::object(py::make_tuple(grads) + py::tuple(tables));
}

// ---- fused BondFFN + scatter_sum (train_ops._BondFfnScatter) -----------------------------------------------------------------------------
// params: Wb, Wi1, bi1, g1, be1, Wi2, bi2, Wg1, bg1, gg, gbe, Wt, Wg2, bg2
enum { B_Wb, B_Wi1, B_bi1, B_g1, B_be1, B_Wi2, B_bi2, B_Wg1, B_bg1, B_gg, B_gbe, B_Wt, B_Wg2, B_bg2 };
enum { BO_g_inter, BO_g_gate, BO_g_pre1, BO_g_bf, BO_g_gpre, BO_post1, BO_gpost, BO_prod, BO_x, BO_time };   // bondffn_bwd's `ops`
constexpr WGrad B_WG[] = {{BO_g_inter, BO_post1, B_Wi2, B_bi2}, {BO_g_gate, BO_gpost, B_Wg2, B_bg2}, {BO_g_pre1, BO_prod, B_Wi1, B_bi1},
                          {BO_g_bf, BO_x, B_Wb, -1},            {BO_g_gpre, BO_x, B_Wg1, B_bg1},     {BO_g_gpre, BO_time, B_Wt, -1}};
constexpr LnSlice B_LN[] = {{B_g1, 0, 128}, {B_be1, 128, 128}, {B_gg, 256, 32}, {B_gbe, 288, 32}};
void bondffn_fill(mdx_bondffn_args& a, const Tensor& x, const Tensor& NL, const Tensor& GN, const Tensor& te, const Tensor& idx,
                  const std::vector<Tensor>& p, const std::vector<Tensor>& bufs) {
  a.X = x.data_ptr(), a.ldx = x.stride(0);
  a.Wb = F32(p[B_Wb]), a.ldwb = p[B_Wb].stride(0);
  a.Wi1 = F32(p[B_Wi1]), a.ldwi1 = p[B_Wi1].stride(0), a.bi1 = F32(p[B_bi1]), a.g1 = F32(p[B_g1]), a.be1 = F32(p[B_be1]);
  a.Wi2 = F32(p[B_Wi2]), a.ldwi2 = p[B_Wi2].stride(0), a.bi2 = F32(p[B_bi2]);
  a.Wg1 = F32(p[B_Wg1]), a.ldwg1 = p[B_Wg1].stride(0), a.bg1 = F32(p[B_bg1]), a.gg = F32(p[B_gg]), a.gbe = F32(p[B_gbe]);
  a.Wt = F32(p[B_Wt]), a.ldwt = p[B_Wt].stride(0);
  a.Wg2 = F32(p[B_Wg2]), a.ldwg2 = p[B_Wg2].stride(0), a.bg2 = F32(p[B_bg2]);
  a.NL = NL.data_ptr(), a.ldnl = NL.stride(0), a.GN = F32(GN), a.ldgn = GN.stride(0);
  a.idx = I64(idx), a.te = F32(te);
  a.prod = bufs[0].data_ptr(), a.pre1 = bufs[1].data_ptr(), a.post1 = bufs[2].data_ptr(), a.inter = bufs[3].data_ptr();
  a.gpre = bufs[4].data_ptr(), a.gpost = bufs[5].data_ptr(), a.gate = bufs[6].data_ptr(), a.out = bufs[7].data_ptr();
  a.E = x.size(0);
}
// -> [S (n_out,64) fp32, x, NL, GN, te, prod, pre1, post1, inter, gpre, gpost, gate, out]
std::vector<Tensor> bondffn_fwd(const Tensor& bond_in, const Tensor& NL, const Tensor& GN, const Tensor& time, const Tensor& idx,
                                const Tensor& o_order, const Tensor& o_ptr, int64_t n_out, const std::vector<Tensor>& params) {
  check_params(params);
  Tensor x = aligned_rows(bond_in, 8, 16), NLc = rows(NL), GNc = rows(GN), te = fc(time).reshape({-1});
  const int64_t E = x.size(0);
  std::vector<Tensor> bufs = {half_empty(E, 128, x), half_empty(E, 128, x), half_empty(E, 128, x), half_empty(E, 64, x),
                              half_empty(E, 32, x),  half_empty(E, 32, x),  half_empty(E, 64, x),  half_empty(E, 64, x)};
  mdx_bondffn_args a;
  bondffn_fill(a, x, NLc, GNc, te, idx, params, bufs);
  chk(mdx_op_bondffn_fwd(&a, cur_stream()));
  ++S.n_launch;
  std::vector<Tensor> r = {segsum_raw(bufs[7], o_order, o_ptr, n_out, false), x, NLc, GNc, te};
  r.insert(r.end(), bufs.begin(), bufs.end());
  return r;
}
// saved = what bondffn_fwd returned after S; -> [g_x, g_NL, g_GN] (see bwd_result)
py::object bondffn_bwd(const Tensor& gS_in, const std::vector<Tensor>& saved, const Tensor& idx, const Tensor& i_order, const Tensor& i_ptr,
                       int64_t n_in, const Tensor& oidx, const Tensor& time2d, const std::vector<Tensor>& params, bool need_x, bool need_nl,
                       bool need_gn, bool dispose) {
  const Tensor &x = saved[0], &NL = saved[1], &GN = saved[2], &te = saved[3];
  std::vector<Tensor> bufs(saved.begin() + 4, saved.begin() + 12);
  const int64_t E = x.size(0);
  Tensor gS = fc(gS_in);
  Tensor g_inter = half_empty(E, 64, x), g_gate = half_empty(E, 64, x), g_pre1 = half_empty(E, 128, x), g_bf = half_empty(E, 128, x),
         g_nl = half_empty(E, 128, x), g_gpre = half_empty(E, 32, x), g_x = half_empty(E, 64, x);
  Tensor lnp = lnp_empty(mdx_op_bondffn_lnp_floats(), x);
  mdx_bondffn_bwd_args b;
  bondffn_fill(b.f, x, NL, GN, te, idx, params, bufs);
  b.gS = F32(gS), b.ldgs = gS.stride(0), b.oidx = I64(oidx);
  b.g_inter = g_inter.data_ptr(), b.g_gate = g_gate.data_ptr(), b.g_pre1 = g_pre1.data_ptr(), b.g_bf = g_bf.data_ptr();
  b.g_nl = g_nl.data_ptr(), b.g_gpre = g_gpre.data_ptr(), b.g_x = g_x.data_ptr(), b.lnp = reinterpret_cast<float*>(lnp.data_ptr());
  chk(mdx_op_bondffn_bwd(&b, cur_stream()));
  ++S.n_launch;
  const Tensor* ops[] = {&g_inter, &g_gate, &g_pre1, &g_bf, &g_gpre, &bufs[2], &bufs[5], &bufs[0], &x, &time2d};
  py::object tables = param_grads(dispose, params, ops, B_WG, B_LN, lnp);
  return bwd_result(tables, {need_x ? g_x : Tensor(), seg(need_nl, g_nl, i_order, i_ptr, n_in, true), seg(need_gn, g_gpre, i_order, i_ptr, n_in, false)});
}

// ---- fused EdgeBlock tail (train_ops._EdgeTail) ---------------------------------------------------------------------------------------------
// params: Ws, bs, lng, lnb, Wo, bo
enum { T_Ws, T_bs, T_lng, T_lnb, T_Wo, T_bo };
enum { TO_g_out, TO_g_pre, TO_post, TO_x };   // edge_tail_bwd's `ops`
constexpr WGrad T_WG[] = {{TO_g_out, TO_post, T_Wo, T_bo}, {TO_g_pre, TO_x, T_Ws, T_bs}};
constexpr LnSlice T_LN[] = {{T_lng, 0, 64}, {T_lnb, 64, 64}};
void edge_tail_fill(mdx_edge_tail_args& a, const Tensor& x, const Tensor& BL, const Tensor& BR, const Tensor& il, const Tensor& ir,
                    const std::vector<Tensor>& p, const Tensor& pre, const Tensor& post, const Tensor& out) {
  a.H = x.data_ptr(), a.ldh = x.stride(0), a.BL = BL.data_ptr(), a.ldbl = BL.stride(0), a.BR = BR.data_ptr(), a.ldbr = BR.stride(0);
  a.il = I64(il), a.ir = I64(ir);
  a.Ws = F32(p[T_Ws]), a.ldws = p[T_Ws].stride(0), a.bs = F32(p[T_bs]), a.lng = F32(p[T_lng]), a.lnb = F32(p[T_lnb]);
  a.Wo = F32(p[T_Wo]), a.ldwo = p[T_Wo].stride(0), a.bo = F32(p[T_bo]);
  a.pre = pre.data_ptr(), a.post = post.data_ptr(), a.out = out.defined() ? out.data_ptr() : nullptr;
  a.E = x.size(0);
}
// -> [out, x, BL, BR, pre, post]
std::vector<Tensor> edge_tail_fwd(const Tensor& h, const Tensor& BL, const Tensor& BR, const Tensor& il, const Tensor& ir,
                                  const std::vector<Tensor>& params) {
  check_params(params);
  Tensor x = aligned_rows(h, 8, 16), BLc = rows(BL), BRc = rows(BR);
  const int64_t E = x.size(0);
  Tensor pre = half_empty(E, 64, x), post = half_empty(E, 64, x), out = half_empty(E, 64, x);
  mdx_edge_tail_args a;
  edge_tail_fill(a, x, BLc, BRc, il, ir, params, pre, post, out);
  chk(mdx_op_edge_tail_fwd(&a, cur_stream()));
  ++S.n_launch;
  return {out, x, BLc, BRc, pre, post};
}
// -> [g_h, g_BL, g_BR] (see bwd_result)
py::object edge_tail_bwd(const Tensor& g_out_in, const std::vector<Tensor>& saved, const Tensor& il, const Tensor& ir, const Tensor& l_order,
                         const Tensor& l_ptr, const Tensor& r_order, const Tensor& r_ptr, int64_t n, const std::vector<Tensor>& params,
                         bool need_h, bool need_bl, bool need_br, bool dispose) {
  const Tensor &x = saved[0], &BL = saved[1], &BR = saved[2], &pre = saved[3], &post = saved[4];
  const int64_t E = x.size(0);
  Tensor g_out = rows(g_out_in);
  if (g_out.scalar_type() != at::kHalf) g_out = g_out.to(at::kHalf);
  if (g_out.stride(0) % 4 || ((uintptr_t)g_out.data_ptr()) % 8) g_out = g_out.contiguous();
  Tensor g_pre = half_empty(E, 64, x), g_h = half_empty(E, 64, x);
  Tensor lnp = lnp_empty(mdx_op_edge_tail_lnp_floats(), x);
  mdx_edge_tail_bwd_args b;
  edge_tail_fill(b.f, x, BL, BR, il, ir, params, pre, post, Tensor());
  b.g_out = g_out.data_ptr(), b.ldg = g_out.stride(0), b.g_pre = g_pre.data_ptr(), b.g_h = g_h.data_ptr();
  b.lnp = reinterpret_cast<float*>(lnp.data_ptr());
  chk(mdx_op_edge_tail_bwd(&b, cur_stream()));
  ++S.n_launch;
  const Tensor* ops[] = {&g_out, &g_pre, &post, &x};
  py::object tables = param_grads(dispose, params, ops, T_WG, T_LN, lnp);
  return bwd_result(tables, {need_h ? g_h : Tensor(), seg(need_bl, g_pre, l_order, l_ptr, n, true), seg(need_br, g_pre, r_order, r_ptr, n, true)});
}

// ---- fused PosUpdate front (train_ops._PosFfnFront) -----------------------------------------------------------------------------------------
// params: Wb, Wn, Wg1x, Wg1a, Wt, bg1, gg, gbe, Wg2, bg2
enum { P_Wb, P_Wn, P_Wg1x, P_Wg1a, P_Wt, P_bg1, P_gg, P_gbe, P_Wg2, P_bg2 };
enum { PO_g_bf, PO_g_nf, PO_g_gpre, PO_g_gate, PO_x, PO_a, PO_gpost, PO_time };   // posffn_bwd's `ops`
constexpr WGrad P_WG[] = {{PO_g_bf, PO_x, P_Wb, -1},     {PO_g_nf, PO_a, P_Wn, -1},      {PO_g_gpre, PO_x, P_Wg1x, P_bg1},
                          {PO_g_gpre, PO_a, P_Wg1a, -1}, {PO_g_gpre, PO_time, P_Wt, -1}, {PO_g_gate, PO_gpost, P_Wg2, P_bg2}};
constexpr LnSlice P_LN[] = {{P_gg, 0, 32}, {P_gbe, 32, 32}};
// the kernel reads gate.net.3's weight row and bias without a stride: contiguous copies where they are not
std::vector<Tensor> posffn_params(const std::vector<Tensor>& params) {
  check_params(params);
  std::vector<Tensor> p = params;
  p[P_Wg2] = fc(p[P_Wg2]), p[P_bg2] = fc(p[P_bg2]);
  return p;
}
void posffn_fill(mdx_posffn_args& a, const Tensor& x, const Tensor& LF, const Tensor& RF, const Tensor& te, const Tensor& il, const Tensor& ir,
                 const std::vector<Tensor>& p, const std::vector<Tensor>& bufs) {
  a.X = x.data_ptr(), a.ldx = x.stride(0), a.LF = LF.data_ptr(), a.ldlf = LF.stride(0), a.RF = RF.data_ptr(), a.ldrf = RF.stride(0);
  a.il = I64(il), a.ir = I64(ir), a.te = F32(te);
  a.Wb = F32(p[P_Wb]), a.ldwb = p[P_Wb].stride(0), a.Wn = F32(p[P_Wn]), a.ldwn = p[P_Wn].stride(0);
  a.Wg1x = F32(p[P_Wg1x]), a.ldwg1x = p[P_Wg1x].stride(0), a.Wg1a = F32(p[P_Wg1a]), a.ldwg1a = p[P_Wg1a].stride(0);
  a.Wt = F32(p[P_Wt]), a.ldwt = p[P_Wt].stride(0);
  a.bg1 = F32(p[P_bg1]), a.gg = F32(p[P_gg]), a.gbe = F32(p[P_gbe]), a.Wg2 = F32(p[P_Wg2]), a.bg2 = F32(p[P_bg2]);
  a.a = bufs[0].data_ptr(), a.prod = bufs[1].data_ptr(), a.gpre = bufs[2].data_ptr(), a.gpost = bufs[3].data_ptr(), a.gate = bufs[4].data_ptr();
  a.E = x.size(0);
}
// -> [prod, gate, x, LF, RF, te, a, gpre, gpost]
std::vector<Tensor> posffn_fwd(const Tensor& h_edge, const Tensor& LF, const Tensor& RF, const Tensor& time, const Tensor& il, const Tensor& ir,
                               const std::vector<Tensor>& params) {
  const std::vector<Tensor> p = posffn_params(params);
  Tensor x = aligned_rows(h_edge, 8, 16), LFc = aligned_rows(LF, 8, 16), RFc = aligned_rows(RF, 8, 16), te = fc(time).reshape({-1});
  const int64_t E = x.size(0);
  std::vector<Tensor> bufs = {half_empty(E, 64, x), half_empty(E, 256, x), half_empty(E, 32, x), half_empty(E, 32, x), half_empty(E, 1, x)};
  mdx_posffn_args a;
  posffn_fill(a, x, LFc, RFc, te, il, ir, p, bufs);
  chk(mdx_op_posffn_fwd(&a, cur_stream()));
  ++S.n_launch;
  return {bufs[1], bufs[4], x, LFc, RFc, te, bufs[0], bufs[2], bufs[3]};
}
// saved = [x, LF, RF, te, a, gpre, gpost, prod, gate]; -> [g_x, g_LF, g_RF] (see bwd_result)
py::object posffn_bwd(const c10::optional<Tensor>& g_prod_in, const c10::optional<Tensor>& g_gate_in, const std::vector<Tensor>& saved,
                      const Tensor& il, const Tensor& ir, const Tensor& l_order, const Tensor& l_ptr, const Tensor& r_order, const Tensor& r_ptr,
                      int64_t n, const Tensor& time2d, const std::vector<Tensor>& params, bool need_x, bool need_lf, bool need_rf, bool dispose) {
  const Tensor &x = saved[0], &LF = saved[1], &RF = saved[2], &te = saved[3];
  std::vector<Tensor> bufs = {saved[4], saved[7], saved[5], saved[6], saved[8]};
  const int64_t E = x.size(0);
  auto f16 = [&](const c10::optional<Tensor>& t, int64_t f) {
    if (!t || !t->defined()) return at::zeros({E, f}, x.options().dtype(at::kHalf));
    Tensor r = t->scalar_type() == at::kHalf ? *t : t->to(at::kHalf);
    return r.contiguous();
  };
  Tensor g_prod = f16(g_prod_in, 256), g_gate = f16(g_gate_in, 1);
  Tensor g_bf = half_empty(E, 256, x), g_nf = half_empty(E, 256, x), g_gpre = half_empty(E, 32, x), g_x = half_empty(E, 64, x),
         g_lf = half_empty(E, 64, x), g_rf = half_empty(E, 64, x);
  Tensor lnp = lnp_empty(mdx_op_posffn_lnp_floats(), x);
  mdx_posffn_bwd_args b;
  posffn_fill(b.f, x, LF, RF, te, il, ir, posffn_params(params), bufs);
  b.g_prod = g_prod.data_ptr(), b.ldgp = g_prod.stride(0), b.g_gate = g_gate.data_ptr(), b.lnp = reinterpret_cast<float*>(lnp.data_ptr());
  b.g_bf = g_bf.data_ptr(), b.g_nf = g_nf.data_ptr(), b.g_gpre = g_gpre.data_ptr(), b.g_x = g_x.data_ptr(), b.g_lf = g_lf.data_ptr(),
  b.g_rf = g_rf.data_ptr();
  chk(mdx_op_posffn_bwd(&b, cur_stream()));
  ++S.n_launch;
  const Tensor* ops[] = {&g_bf, &g_nf, &g_gpre, &g_gate, &x, &bufs[0], &bufs[3], &time2d};
  py::object tables = param_grads(dispose, params, ops, P_WG, P_LN, lnp);
  return bwd_result(tables, {need_x ? g_x : Tensor(), seg(need_lf, g_lf, l_order, l_ptr, n, true), seg(need_rf, g_rf, r_order, r_ptr, n, true)});
}

// ---- fused NodeBlock message path (train_ops._NodeMsg) ----------------------------------------------------------------------------------------
// params: W1e, b1e, lng_e, lnb_e, W2e, b2e, Wm, bm, Wg1, bg1, lng_g, lnb_g, Wg2, bg2
enum { N_W1e, N_b1e, N_lng_e, N_lnb_e, N_W2e, N_b2e, N_Wm, N_bm, N_Wg1, N_bg1, N_lng_g, N_lnb_g, N_Wg2, N_bg2 };
enum { NO_g_m0, NO_g_gt, NO_g_gpre, NO_g_he, NO_g_pre, NO_p, NO_g_post, NO_he_post, NO_x };   // nodemsg_bwd's `ops`
constexpr WGrad N_WG[] = {{NO_g_m0, NO_p, N_Wm, N_bm},          {NO_g_gt, NO_g_post, N_Wg2, N_bg2}, {NO_g_gpre, NO_x, N_Wg1, N_bg1},
                          {NO_g_he, NO_he_post, N_W2e, N_b2e}, {NO_g_pre, NO_x, N_W1e, N_b1e}};
constexpr LnSlice N_LN[] = {{N_lng_e, 0, 256}, {N_lnb_e, 256, 256}, {N_lng_g, 512, 256}, {N_lnb_g, 768, 256}};
// the ten A-operand packs of a call (one buffer, one launch): five forward, then their five transposes for the backward
struct PackSpec { int w, n_out, n_in, perm, trans; };
constexpr PackSpec PACKS[10] = {{N_W1e, 256, 64, 0, 0},  {N_W2e, 256, 256, 1, 0}, {N_Wm, 256, 256, 1, 0},  {N_Wg1, 256, 64, 0, 0},
                                {N_Wg2, 256, 256, 1, 0}, {N_Wg2, 256, 256, 1, 1}, {N_Wg1, 64, 256, 1, 1},  {N_Wm, 256, 256, 1, 1},
                                {N_W2e, 256, 256, 1, 1}, {N_W1e, 64, 256, 1, 1}};
void nodemsg_fill(mdx_nodemsg_args& a, const Tensor& x, const Tensor& HN, const Tensor& PN, const Tensor& col, const std::vector<Tensor>& p,
                  const int64_t* packs, const std::vector<Tensor>& bufs) {
  a.X = x.data_ptr(), a.ldx = x.stride(0), a.HN = HN.data_ptr(), a.ldhn = HN.stride(0), a.PN = F32(PN), a.ldpn = PN.stride(0);
  a.col = I64(col);
  a.pk_w1e = (const void*)packs[0], a.pk_w2e = (const void*)packs[1], a.pk_wm = (const void*)packs[2], a.pk_wg1 = (const void*)packs[3],
  a.pk_wg2 = (const void*)packs[4];
  a.b1e = F32(p[N_b1e]), a.lng_e = F32(p[N_lng_e]), a.lnb_e = F32(p[N_lnb_e]), a.b2e = F32(p[N_b2e]), a.bm = F32(p[N_bm]), a.bg1 = F32(p[N_bg1]);
  a.lng_g = F32(p[N_lng_g]), a.lnb_g = F32(p[N_lnb_g]), a.bg2 = F32(p[N_bg2]);
  a.he_pre = bufs[0].data_ptr(), a.he_post = bufs[1].data_ptr(), a.he = bufs[2].data_ptr(), a.p = bufs[3].data_ptr(), a.m0 = bufs[4].data_ptr();
  a.g_pre = bufs[5].data_ptr(), a.g_post = bufs[6].data_ptr(), a.gt = bufs[7].data_ptr(), a.msg = bufs[8].data_ptr();
  a.E = x.size(0);
}
void pack_ptrs(const Tensor& buf, int64_t* packs) {
  int64_t off = 0;
  for (int i = 0; i < 10; ++i) {
    packs[i] = A(buf) + 2 * off;
    off += (int64_t)PACKS[i].n_out * PACKS[i].n_in;
  }
}
// -> [out (n,256) fp32, x, HN, PN, packbuf, he_pre, he_post, he, p, m0, g_pre, g_post, gt]
std::vector<Tensor> nodemsg_fwd(const Tensor& edge_attr, const Tensor& HN, const Tensor& PN, const Tensor& col, const Tensor& r_order,
                                const Tensor& r_ptr, int64_t n, const std::vector<Tensor>& params) {
  check_params(params);
  Tensor x = aligned_rows(edge_attr, 8, 16), HNc = rows(HN), PNc = rows(PN);
  const int64_t E = x.size(0);
  int64_t total = 0;
  for (auto& s : PACKS) total += (int64_t)s.n_out * s.n_in;
  Tensor buf = at::empty({total}, x.options().dtype(at::kHalf));
  int64_t packs[10];
  pack_ptrs(buf, packs);
  mdx_pack_jobs jobs;
  for (int i = 0; i < 10; ++i) {
    const Tensor& w = params[PACKS[i].w];
    jobs.job[i] = {F32(w), w.stride(0), PACKS[i].n_out, PACKS[i].n_in, PACKS[i].perm, PACKS[i].trans, (void*)packs[i]};
  }
  jobs.n = 10;
  chk(mdx_op_pack_a(&jobs, cur_stream()));
  ++S.n_launch;
  std::vector<Tensor> bufs(9);
  for (auto& b : bufs) b = half_empty(E, 256, x);
  mdx_nodemsg_args a;
  nodemsg_fill(a, x, HNc, PNc, col, params, packs, bufs);
  chk(mdx_op_nodemsg_fwd(&a, cur_stream()));
  ++S.n_launch;
  std::vector<Tensor> r = {segsum_raw(bufs[8], r_order, r_ptr, n, false), x, HNc, PNc, buf};
  r.insert(r.end(), bufs.begin(), bufs.begin() + 8);   // (msg is not kept)
  return r;
}
// saved = [x, HN, PN, packbuf, he_pre, he_post, he, p, m0, g_pre, g_post, gt]; -> [g_x, g_HN, g_PN] (see bwd_result)
py::object nodemsg_bwd(const Tensor& gA_in, const std::vector<Tensor>& saved, const Tensor& col, const Tensor& c_order, const Tensor& c_ptr,
                       int64_t n, const Tensor& row, const std::vector<Tensor>& params, bool need_x, bool need_hn, bool need_pn, bool dispose) {
  const Tensor &x = saved[0], &HN = saved[1], &PN = saved[2], &buf = saved[3];
  std::vector<Tensor> bufs(saved.begin() + 4, saved.begin() + 12);
  bufs.push_back(saved[8]);   // (the forward's msg buffer is gone; the backward does not read it)
  const int64_t E = x.size(0);
  Tensor gA = fc(gA_in);
  Tensor g_m0 = half_empty(E, 256, x), g_gt = half_empty(E, 256, x), g_gpre = half_empty(E, 256, x), g_hne = half_empty(E, 256, x),
         g_he = half_empty(E, 256, x), g_pre = half_empty(E, 256, x), g_x = half_empty(E, 64, x);
  Tensor lnp = lnp_empty(mdx_op_nodemsg_lnp_floats(), x);
  int64_t packs[10];
  pack_ptrs(buf, packs);
  mdx_nodemsg_bwd_args b;
  nodemsg_fill(b.f, x, HN, PN, col, params, packs, bufs);
  b.gA = F32(gA), b.ldga = gA.stride(0), b.row = I64(row);
  b.pk_wg2t = (const void*)packs[5], b.pk_wg1t = (const void*)packs[6], b.pk_wmt = (const void*)packs[7], b.pk_w2et = (const void*)packs[8],
  b.pk_w1et = (const void*)packs[9];
  b.g_m0 = g_m0.data_ptr(), b.g_gt = g_gt.data_ptr(), b.g_gpre = g_gpre.data_ptr(), b.g_hne = g_hne.data_ptr(), b.g_he = g_he.data_ptr(),
  b.g_pre = g_pre.data_ptr(), b.g_x = g_x.data_ptr(), b.lnp = reinterpret_cast<float*>(lnp.data_ptr());
  chk(mdx_op_nodemsg_bwd(&b, cur_stream()));
  ++S.n_launch;
  const Tensor* ops[] = {&g_m0, &g_gt, &g_gpre, &g_he, &g_pre, &bufs[3], &bufs[6], &bufs[1], &x};
  py::object tables = param_grads(dispose, params, ops, N_WG, N_LN, lnp);
  return bwd_result(tables, {need_x ? g_x : Tensor(), seg(need_hn, g_hne, c_order, c_ptr, n, true), seg(need_pn, g_gpre, c_order, c_ptr, n, false)});
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "moldiff_amd training host side in C++: operator bodies, gradient sink and weight-gradient queue (csrc/mdx_fast.cpp)";
  m.def("set_precision", [](int a0, int autoc, int store) { S.amp0 = a0, S.amp_auto = autoc, S.amp_store = store; });
  m.def("set_options", [](bool wq_on, int64_t rows_, int64_t cap_bytes, int64_t rows_min) {
    S.wq_on = wq_on, S.wgrad_rows = rows_, S.wq_cap = cap_bytes, S.rows_min = rows_min;
  });
  m.def("sink_begin", [](const Tensor& data, const Tensor& grad) {
    TORCH_CHECK(!S.sink, "gradient sinks do not nest");
    S.sink = true, S.s_data = A(data), S.s_grad = A(grad), S.s_nbytes = data.numel() * 4, S.like = data;
    S.recs.clear(), S.recs2.clear(), S.keep.clear(), S.seen.clear(), S.wq.clear();
    S.blocks = S.blocks2 = S.wq_bytes = 0;
  });
  m.def("sink_end", []() {
    if (S.sink && (!S.recs.empty() || !S.wq.empty())) flush_sink();
    S.sink = false;
    S.wq.clear(), S.keep.clear(), S.like = Tensor();
  });
  m.def("sink_active", []() { return S.sink; });
  m.def("fast_mode", &fast_mode);
  m.def("sink_dst", &sink_dst);
  m.def("sink_record", [](int64_t Pp, int64_t dst, int64_t Sn, int64_t rows_, int64_t cols, int64_t ld, int64_t pstride, int64_t rkind,
                          const c10::optional<Tensor>& keep) {
    sink_record(Pp, dst, Sn, rows_, cols, ld, pstride, rkind, (keep && keep->defined()) ? *keep : Tensor());
  });
  m.def("wq_append", &wq_append);
  m.def("flush", &flush_sink);
  m.def("set_wt", [](int64_t base, int64_t nbytes, const c10::optional<Tensor>& buf, std::vector<int64_t> offs,
                     std::vector<std::array<int64_t, 4>> ents) {
    S.wt_buf = opt(buf);
    S.wt = WtTable{base, nbytes, A(S.wt_buf), std::move(offs), std::move(ents)};
  });
  // (element offset in the transposed buffer at `buf`, leading dimension) of w's transpose in a table given as set_wt takes it, or None
  m.def("wt_view", [](int64_t base, int64_t nbytes, int64_t buf, std::vector<int64_t> offs, std::vector<std::array<int64_t, 4>> ents,
                      const Tensor& w) -> py::object {
    int64_t p = 0, ld = 0;
    if (!wt_view(WtTable{base, nbytes, buf, std::move(offs), std::move(ents)}, w, p, ld)) return py::none();
    return py::make_tuple((p - buf) / 4, ld);
  });
  m.def("launches", []() { return S.n_launch; });
  // the autograd nodes
  m.def("linear", &linear);
  m.def("ln_relu", [](const Tensor& x, const Tensor& gamma, const Tensor& beta, bool relu) { return LnReluFn::apply(x, gamma, beta, relu); });
  m.def("linear_ln_relu", &linear_ln_relu);
  m.def("linear_ln_relu_dot", &linear_ln_relu_dot);
  m.def("ew", [](int64_t op, const Tensor& a, const Tensor& b) { return EwFn::apply(op, a, b); });
  m.def("linear_ln_ok", [](const Tensor& x, const Tensor& w, const c10::optional<Tensor>& addend) { return linear_ln_ok(x, w, opt(addend)); });
  m.def("linear_ln_dot_fast_ok", &linear_ln_dot_fast_ok);
  // Python calls neither of these any more (fast_mode above likewise): linear_fast_ok is a part of linear_ln_dot_fast_ok, and
  // linear_ln_fast_ok is the former name of linear_ln_ok.  They stay bound because tests/test_host_logic.py lists them.
  m.def("linear_fast_ok", &linear_fast_ok);
  m.attr("linear_ln_fast_ok") = m.attr("linear_ln_ok");
  // the functions the nodes are made of, under their train_ops names (tests and tools call them)
  m.def("rows", &rows);
  m.def("sgemm_nt", [](const Tensor& a, const Tensor& b, const c10::optional<Tensor>& bias, int64_t splits, const c10::optional<Tensor>& addend,
                       bool keep32, int64_t out_half) {   // out_half: -1 = the mode's container, 0 = fp32, 1 = float16
    TORCH_CHECK(a.stride(1) == 1 && b.stride(1) == 1 && b.scalar_type() == at::kFloat, "sgemm_nt: unit column strides and an fp32 weight expected");
    return gemm_nt(a, b.data_ptr(), b.stride(0), b.size(0), a.size(1), opt(bias), opt(addend), keep32,
                   out_half < 0 ? c10::nullopt : c10::optional<at::ScalarType>(out_half ? at::kHalf : at::kFloat), splits);
  });
  m.def("weight_grad", &weight_grad);
  m.def("splits_for", &splits_for);
  m.def("wgrad_layout", [](int64_t M, int64_t N, int64_t K, int64_t splits, int64_t half) {
    int64_t Sn = 0, boff = 0;
    chk(mdx_op_wgrad_layout(M, N, K, (int32_t)splits, (int32_t)half, &Sn, &boff));
    return std::make_pair(Sn, boff);
  });
  m.def("transpose", [](const Tensor& x, int64_t pad) {
    int64_t p = 0, ld = 0;
    Tensor buf = transposed(x, pad, p, ld);
    return buf.defined() ? buf.narrow(1, 0, x.size(0)) : S.wt_buf.as_strided({x.size(1), ld}, {ld, 1}, (p - S.wt.buf) / 4);
  });
  m.def("colreduce", [](const Tensor& x, const c10::optional<Tensor>& y) { return colreduce(x, opt(y)); });
  m.def("linear_rows_ok", [](const Tensor& a, int64_t n, int64_t k, const c10::optional<Tensor>& addend) { return linear_rows_ok(a, n, k, opt(addend)); });
  m.def("linear_rows", [](const Tensor& a, const Tensor& w, bool trans_w, const c10::optional<Tensor>& bias, const c10::optional<Tensor>& addend) {
    return linear_rows(a, w, trans_w, opt(bias), opt(addend));
  });
  // The forwards of the LayerNorm and Linear+LayerNorm nodes without the node: a C++ node does not show what it saved, so
  // tests/test_gpu_train_ops.py repeats the launch through these two to look at the Linear's stored result and the row statistics.
  m.def("ln_relu_fwd", [](const Tensor& x, const Tensor& gamma, const Tensor& beta, bool relu) {   // -> (y, stats)
    const LnFwd f = ln_forward(x, gamma, beta, relu);
    return std::make_pair(f.y, f.stats);
  });
  m.def("linear_ln_fwd", [](const Tensor& x, const Tensor& w, const c10::optional<Tensor>& b, const c10::optional<Tensor>& addend,
                            const Tensor& gamma, const Tensor& beta) {   // -> (post, pre, stats) of the fused launch
    const LinLnFwd f = linear_ln_forward(x, w, b, addend, gamma, beta);
    return std::make_tuple(f.post, f.pre, f.stats);
  });
  m.def("all_in_sink", &all_in_sink);
  m.def("bondffn_fwd", &bondffn_fwd);
  m.def("bondffn_bwd", &bondffn_bwd);
  m.def("edge_tail_fwd", &edge_tail_fwd);
  m.def("edge_tail_bwd", &edge_tail_bwd);
  m.def("posffn_fwd", &posffn_fwd);
  m.def("posffn_bwd", &posffn_bwd);
  m.def("nodemsg_fwd", &nodemsg_fwd);
  m.def("nodemsg_bwd", &nodemsg_bwd);
}
