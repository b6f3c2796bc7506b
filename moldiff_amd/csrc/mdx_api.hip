// Host side of libmoldiff_hip.so: handles, weight packing, CSR planning, launch orchestration, C ABI.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/moldiff_hip.h"
#include "mdx_kernels.h"
#include "mdx_pack.h"
#include "mdx_plan.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int mdx_set_error(int code, const char* msg) { return fail(code, "%s", msg); }  // for the other translation units
#define HIPCHK(x)                                                                           \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess) return fail(MDX_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_));   \
  } while (0)

// compute units of the current device (grid sizes of the persistent kernels; for the other translation units), read by the
// launchers at every launch: edge kernels A and B, the guidance backward, linear_rows, the training GEMMs' grid heuristics and the
// eight fused float16 training kernels of mdx_train_fused.hip.  A test may cap it (mdx_debug_set_num_cus): nothing made at model or
// graph creation depends on it (the work-queue counter sets hold MDX_WQ_PAIRS >= #CUs lines whatever the count), and a cap only
// lowers it.  The fused training backwards leave one partial row of LayerNorm-parameter gradients per workgroup = per compute unit of
// this count (mdx_op_bondffn_workgroups): a cap must not change between such a launch and the reduction of its rows.
static int g_cu_cap = 0;  // 0: none
int mdx_num_cus() {
  static const int n = [] {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 256;
    return p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }();
  const int cap = g_cu_cap;
  return cap > 0 && cap < n ? cap : n;
}
extern "C" int mdx_debug_set_num_cus(int32_t n) {
  g_cu_cap = n > 0 ? n : 0;
  return MDX_OK;
}

extern "C" const char* mdx_last_error(void) { return g_err; }
extern "C" int mdx_version(void) { return 100; }
extern "C" int mdx_device_count(int* count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  if (count) *count = n;
  return MDX_OK;
}

// ------------------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------------------
struct mdx_model_s : ModelW {  // the weight blocks (mdx_pack.h): pointers into `arena` once finalized
  mdx_config cfg;
  ParamMap params;
  bool finalized = false;
  float smear_start = 0.f;  // lower clamp of the distance smearing (mdx_model_set_smear_start)
  float* arena = nullptr;  // device
  size_t arena_floats = 0;
  // matrix path of the row-owner edge kernels: 0 = exact fp32 MFMA (default), 1 = split float16 (mdx_split.h).  Both weight
  // packs are always built; split_ok is false when a weight would overflow the scaled float16 range (the path is then refused).
  int matrix_path = 0;
  bool split_ok = true;
  float split_wmax = 0.f;
  // Centred packs (mdx_pack.cpp Layer::centred) for the MolDiff denoiser's edge kernels.  On by default; a test
  // may turn them off and re-pack (mdx_debug_set_ln_centred).  Never for the bond predictor: its tape keeps pre-LayerNorm values that
  // the guidance backward re-normalises against the un-centred transposed packs.
  bool ln_centred = true;
};

// the centring on the host alone, for tests/test_ln_centred_pack.py
extern "C" int mdx_debug_centre_host(const float* W, int32_t F, int32_t ldw, float* out, double* worst) {
  if (!W || !out || !worst || F < 1 || ldw < 1) return MDX_ERR_ARG;
  *worst = centre_columns(W, F, ldw, out);
  return MDX_OK;
}

namespace {

// Packs the handle's parameters on the host (mdx_pack.cpp), uploads the arena and binds the weight blocks to it.
int finalize_model(mdx_model_s* m) {
  PackResult pk;
  pack_model(m->cfg, m->params, m->ln_centred, m, &pk);
  m->finalized = false;
  if (!pk.error.empty()) return fail(MDX_ERR_STATE, "%s", pk.error.c_str());
  m->split_ok = pk.split_ok;
  m->split_wmax = pk.split_wmax;
  if (m->arena) hipFree(m->arena);
  m->arena = nullptr;
  m->arena_floats = pk.arena.size();
  HIPCHK(hipMalloc((void**)&m->arena, m->arena_floats * sizeof(float)));
  HIPCHK(hipMemcpy(m->arena, pk.arena.data(), m->arena_floats * sizeof(float), hipMemcpyHostToDevice));
  for (auto& f : pk.fix) *f.first = m->arena + f.second;
  m->finalized = true;
  // a handle re-finalized with weights the split path cannot hold falls back to the exact path instead of silently running
  // float16 operands that overflowed at pack time (the caller's next mdx_model_set_matrix_path(split) is refused as usual)
  if (!m->split_ok) m->matrix_path = MDX_MATRIX_EXACT_F32;
  return MDX_OK;
}

}  // namespace

extern "C" int mdx_model_create(const mdx_config* cfg, mdx_model_t* out) {
  if (!cfg || !out) return fail(MDX_ERR_ARG, "null argument");
  if (cfg->node_dim != MDX_ND || cfg->edge_dim != MDX_ED || cfg->num_gaussians != MDX_NG)
    return fail(MDX_ERR_UNSUPPORTED, "kernels are built for node_dim=%d edge_dim=%d num_gaussians=%d (got %d/%d/%d)", MDX_ND,
                MDX_ED, MDX_NG, cfg->node_dim, cfg->edge_dim, cfg->num_gaussians);
  if (cfg->num_blocks < 1 || cfg->num_blocks > 64) return fail(MDX_ERR_ARG, "num_blocks out of range");
  if (cfg->kind != MDX_KIND_NET) {
    if (cfg->num_node_types < 1 || cfg->num_node_types > 8 || cfg->num_edge_types < 1 || cfg->num_edge_types > 8)
      return fail(MDX_ERR_UNSUPPORTED, "class counts must be in 1..8");
    if (cfg->time_dim < 0 || cfg->time_dim >= MDX_ED) return fail(MDX_ERR_ARG, "time_dim out of range");
  }
  mdx_model_s* m = new mdx_model_s();
  m->cfg = *cfg;
  *out = m;
  return MDX_OK;
}

extern "C" int mdx_model_destroy(mdx_model_t m) {
  if (!m) return MDX_OK;
  if (m->arena) hipFree(m->arena);
  delete m;
  return MDX_OK;
}

extern "C" int mdx_model_set_param(mdx_model_t m, const char* key, const float* h_data, const int64_t* shape,
                                   int32_t ndim) {
  if (!m || !key || !h_data || (ndim > 0 && !shape) || ndim < 0 || ndim > 4) return fail(MDX_ERR_ARG, "bad argument");
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] < 0) return fail(MDX_ERR_ARG, "negative dim");
    t.shape.push_back(shape[i]);
    n *= (size_t)shape[i];
  }
  t.data.assign(h_data, h_data + n);
  m->params[key] = std::move(t);
  m->finalized = false;
  return MDX_OK;
}

extern "C" int mdx_model_finalize(mdx_model_t m) {
  if (!m) return fail(MDX_ERR_ARG, "null model");
  return finalize_model(m);
}

// Matrix path of the row-owner edge kernels (the products of models/common.py:181-201 MLP / models/graph.py:29-55,133-141,268-295
// Linear layers evaluated per edge): MDX_MATRIX_EXACT_F32 = v_mfma_f32_16x16x4_f32, bit-for-bit an fmaf chain (default);
// MDX_MATRIX_SPLIT_F16 = operands split into float16 hi + lo halves, three v_mfma_f32_16x16x32_f16 per k-group, fp32 accumulation
// (mdx_split.h).  Per-node layers, reductions, LayerNorm, gates and transitions are fp32 in both.
extern "C" int mdx_model_set_matrix_path(mdx_model_t m, int32_t path) {
  if (!m) return fail(MDX_ERR_ARG, "null model");
  if (path != MDX_MATRIX_EXACT_F32 && path != MDX_MATRIX_SPLIT_F16) return fail(MDX_ERR_ARG, "unknown matrix path %d", (int)path);
  if (path == MDX_MATRIX_SPLIT_F16) {
    if (!m->finalized) return fail(MDX_ERR_STATE, "model not finalized (call mdx_model_finalize)");
    if (!m->split_ok)
      return fail(MDX_ERR_UNSUPPORTED, "split float16 path refused: a weight of magnitude %g is outside float16's range (|w| < 65504)",
                  (double)m->split_wmax);
  }
  m->matrix_path = path;
  return MDX_OK;
}
// TEST AID: pack the denoiser's edge-kernel layers centred (1, the default) or as stored (0) and re-pack the handle, so that a test
// can run both conventions on one handle.  Not a tuning switch: the two differ in the last bits only.  The arena is freed and
// allocated again, so whatever cached device pointers into it (a captured graph, a live sampler) must be re-created afterwards.
extern "C" int mdx_debug_set_ln_centred(mdx_model_t m, int32_t on) {
  if (!m) return fail(MDX_ERR_ARG, "null model");
  if (!m->finalized) return fail(MDX_ERR_STATE, "model not finalized (call mdx_model_finalize)");
  if (hipDeviceSynchronize() != hipSuccess) return fail(MDX_ERR_HIP, "device synchronize failed");  // the old arena may still be read
  m->ln_centred = on != 0;
  return finalize_model(m);  // (the matrix path is kept: finalize_model only leaves the split path when the weights do not fit it)
}
// TEST AID, host only: what finalize would upload for this handle's parameters with centred packs on or off -- the arena (floats)
// and one text line per pack, "kind offset floats F K col0 transposed centred key" (mdx_pack.h PackSlot).  Call with arena / slots null
// to get the sizes.  The handle itself is not touched.
extern "C" int mdx_debug_pack_host(mdx_model_t m, int32_t ln_centred, float* arena, size_t* n_floats, char* slots, size_t* n_slot_bytes) {
  if (!m || !n_floats || !n_slot_bytes) return fail(MDX_ERR_ARG, "null argument");
  ModelW w;
  PackResult hp;
  pack_model(m->cfg, m->params, ln_centred != 0, &w, &hp);
  if (!hp.error.empty()) return fail(MDX_ERR_STATE, "%s", hp.error.c_str());
  std::string txt;
  for (const auto& sl : hp.slots) {
    char line[512];
    snprintf(line, sizeof(line), "%c %zu %zu %d %d %d %d %d %s\n", sl.kind, sl.off, sl.n, sl.F, sl.K, sl.col0, sl.transposed, sl.centred,
             sl.key.empty() ? "-" : sl.key.c_str());
    txt += line;
  }
  if (arena) {
    if (*n_floats < hp.arena.size()) return fail(MDX_ERR_ARG, "arena buffer too small");
    std::memcpy(arena, hp.arena.data(), hp.arena.size() * sizeof(float));
  }
  if (slots) {
    if (*n_slot_bytes < txt.size() + 1) return fail(MDX_ERR_ARG, "slot buffer too small");
    std::memcpy(slots, txt.c_str(), txt.size() + 1);
  }
  *n_floats = hp.arena.size();
  *n_slot_bytes = txt.size() + 1;
  return MDX_OK;
}
extern "C" int mdx_model_set_smear_start(mdx_model_t m, float start) {
  if (!m) return fail(MDX_ERR_ARG, "null model");
  if (!(start >= 0.f) || !(start < m->cfg.cutoff)) return fail(MDX_ERR_ARG, "smearing start %g outside [0, cutoff)", (double)start);
  m->smear_start = start;
  return MDX_OK;
}
extern "C" int mdx_model_get_matrix_path(mdx_model_t m, int32_t* path) {
  if (!m || !path) return fail(MDX_ERR_ARG, "null argument");
  *path = m->matrix_path;
  return MDX_OK;
}

// ------------------------------------------------------------------------------------------------
// graph
// ------------------------------------------------------------------------------------------------
constexpr int MDX_WQ_SETS = 4, MDX_WQ_SET_INTS = 512 * 32;  // mdx_row.h: MDX_WQ_PAIRS lines of MDX_WQ_STRIDE ints per set
struct mdx_graph_s {
  int64_t N = 0, E = 0, Eh = 0, B = 0;
  int32_t* dev = nullptr;   // one int32 slab
  int64_t* mol_ids = nullptr;
  const int32_t *left, *right, *int2ref, *ref2int, *row_ptr, *col_ptr, *col_eids, *node_graph, *node_local, *he_graph,
      *he_local, *half_of_int, *node_ptr, *he_ptr;
  // graph-aligned 16-row units of edge kernel A's in-kernel aggregation (EA_AGG, mdx_kernels.h): units (2 ints per unit: first
  // edge, rows), per-edge partial-row offset, per-node partial-row ranges
  const int32_t *units = nullptr, *epo = nullptr, *pbase = nullptr;
  int64_t nunits = 0, nparts = 0;
  // the same in BY-RIGHT order (positions of col_eids), for the guidance backward's in-kernel sums of its by-right payloads
  // (round 5): units_r (first col position, rows), epo_r per col position, pbase_r per node; col_left / col_right = the end
  // points of edge col_eids[j] (so a tile's indices are independent loads)
  const int32_t *units_r = nullptr, *epo_r = nullptr, *pbase_r = nullptr, *col_left = nullptr, *col_right = nullptr;
  int64_t nunits_r = 0, nparts_r = 0;
  hipEvent_t ev_in = nullptr, ev_done = nullptr;  // stream hand-offs of mdx_sample_step_full's concurrent guidance chain
  // work-queue counter sets of the persistent edge kernels, one per launching stream (wq_for)
  int* wq = nullptr;
  hipStream_t wq_stream[MDX_WQ_SETS] = {};
  int wq_n = 0;
  std::mutex wq_mu;
};

namespace {
struct HostPlan {
  std::vector<int32_t> left, right, int2ref, ref2int, row_ptr, col_ptr, col_eids;
};

// Units of 16 positions of a CSR order (ptr = row_ptr: edges by left node, col_ptr: col_eids by right node) aligned to each graph's
// first position: graph b owns the positions ptr[node_ptr[b]] .. ptr[node_ptr[b+1]] (batch_node is non-decreasing).  Two ints per
// unit: first position, rows.
std::vector<int32_t> aligned_units(const std::vector<int32_t>& ptr, const std::vector<int32_t>& node_ptr) {
  std::vector<int32_t> units;
  for (size_t b = 0; b + 1 < node_ptr.size(); ++b) {
    const int32_t lo = ptr[node_ptr[b]], hi = ptr[node_ptr[b + 1]];
    for (int32_t p0 = lo; p0 < hi; p0 += 16) {
      units.push_back(p0);
      units.push_back(std::min<int32_t>(16, hi - p0));
    }
  }
  return units;
}

int plan_graph(int64_t N, int64_t E, const int64_t* ei, HostPlan& p) {
  if (N < 0 || E < 0 || N > INT32_MAX / 4 || E > INT32_MAX / 4) return fail(MDX_ERR_ARG, "graph too large");
  const int64_t* L = ei;
  const int64_t* R = ei + E;
  for (int64_t e = 0; e < E; ++e)
    if (L[e] < 0 || L[e] >= N || R[e] < 0 || R[e] >= N) return fail(MDX_ERR_ARG, "edge_index out of range at %lld", (long long)e);
  p.int2ref.resize(E);
  std::iota(p.int2ref.begin(), p.int2ref.end(), 0);
  std::stable_sort(p.int2ref.begin(), p.int2ref.end(), [&](int32_t a, int32_t b) {
    if (L[a] != L[b]) return L[a] < L[b];
    return R[a] < R[b];
  });
  p.left.resize(E);
  p.right.resize(E);
  p.ref2int.resize(E);
  p.row_ptr.assign(N + 1, 0);
  p.col_ptr.assign(N + 1, 0);
  for (int64_t i = 0; i < E; ++i) {
    const int32_t e = p.int2ref[i];
    p.left[i] = (int32_t)L[e];
    p.right[i] = (int32_t)R[e];
    p.ref2int[e] = (int32_t)i;
    p.row_ptr[L[e] + 1]++;
    p.col_ptr[R[e] + 1]++;
  }
  for (int64_t v = 0; v < N; ++v) {
    p.row_ptr[v + 1] += p.row_ptr[v];
    p.col_ptr[v + 1] += p.col_ptr[v];
  }
  p.col_eids.resize(E);
  std::vector<int32_t> cur(p.col_ptr.begin(), p.col_ptr.end() - 1);
  for (int64_t i = 0; i < E; ++i) p.col_eids[cur[p.right[i]]++] = (int32_t)i;
  return MDX_OK;
}
}  // namespace

extern "C" int mdx_graph_plan_host(int64_t N, int64_t E, const int64_t* ei, int32_t* left, int32_t* right,
                                   int32_t* int2ref, int32_t* row_ptr, int32_t* col_ptr, int32_t* col_eids) {
  if ((E > 0 && !ei) || !left || !right || !int2ref || !row_ptr || !col_ptr || !col_eids) return fail(MDX_ERR_ARG, "null argument");
  HostPlan p;
  int rc = plan_graph(N, E, ei, p);
  if (rc) return rc;
  std::copy(p.left.begin(), p.left.end(), left);
  std::copy(p.right.begin(), p.right.end(), right);
  std::copy(p.int2ref.begin(), p.int2ref.end(), int2ref);
  std::copy(p.row_ptr.begin(), p.row_ptr.end(), row_ptr);
  std::copy(p.col_ptr.begin(), p.col_ptr.end(), col_ptr);
  std::copy(p.col_eids.begin(), p.col_eids.end(), col_eids);
  return MDX_OK;
}

extern "C" int mdx_debug_work_plan_host(int32_t nunits, int32_t nslots, int32_t can_split, int32_t* plan) {
  if (!plan || nunits < 0 || nslots <= 0) return fail(MDX_ERR_ARG, "work plan: null output, negative units or no slots");
  const EdgePlan p = make_plan(nunits, nslots, can_split != 0);
  plan[0] = p.nslots; plan[1] = p.nf; plan[2] = p.rem; plan[3] = p.split; plan[4] = p.m;
  return MDX_OK;
}

extern "C" int mdx_debug_launch_units_host(int64_t N, int64_t E, const int64_t* ei, const int64_t* bn, int64_t B, int32_t n_cus,
                                           int32_t* launches) {
  if (!launches || (E > 0 && !ei) || (N > 0 && !bn) || B < 0) return fail(MDX_ERR_ARG, "launch units: bad argument");
  if (n_cus <= 0) n_cus = mdx_num_cus();  // what the launchers see right now
  HostPlan p;
  int rc = plan_graph(N, E, ei, p);
  if (rc) return rc;
  std::vector<int32_t> node_ptr(B + 1, 0);
  for (int64_t v = 0; v < N; ++v) {
    if (bn[v] < 0 || bn[v] >= B || (v && bn[v] < bn[v - 1])) return fail(MDX_ERR_ARG, "batch_node must be non-decreasing in [0, n_graphs)");
    node_ptr[bn[v] + 1]++;
  }
  for (int64_t b = 0; b < B; ++b) node_ptr[b + 1] += node_ptr[b];
  const int ua = (int)aligned_units(p.row_ptr, node_ptr).size() / 2, ur = (int)aligned_units(p.col_ptr, node_ptr).size() / 2;
  // work items as the launchers count them: kernel A RR graph-aligned units each (rows / 16), kernel B `rows` edges each, the
  // backward one by-right unit each
  const RowOwnerShape sh[6] = {shape_edge_a2(), shape_edge_a2s(), shape_edge_b2(), shape_edge_b2s(), shape_edge_bwd2(), shape_edge_bwd2s()};
  for (int k = 0; k < 6; ++k) {
    const int rr = sh[k].rows / 16;
    const int nunits = k < 2 ? (ua + rr - 1) / rr : k < 4 ? (int)((E + sh[k].rows - 1) / sh[k].rows) : ur;
    const int grid = nunits > 0 ? row_owner_grid(nunits, n_cus, sh[k].wps) : 0;
    const WorkQ w = make_workq(nullptr, nunits, grid, n_cus);
    int32_t* o = launches + 8 * k;
    o[0] = nunits; o[1] = grid; o[2] = grid > 0 ? w.npairs : 0;
    o[3] = o[4] = o[5] = o[6] = o[7] = 0;
    for (int pr = 0; grid > 0 && pr < w.npairs; ++pr) {
      int beg, end;
      wq_range(w, xcd_remap(pr, w.npairs), beg, end);
      const int waves = wq_waves(w, 4, (unsigned)grid, pr), cnt = end - beg, tail = waves * EA_WQ_TAIL8 >> 3;  // four waves per workgroup
      o[cnt < tail ? 3 : cnt == tail ? 4 : waves == 4 ? 5 : 6]++;
    }
  }
  return MDX_OK;
}

extern "C" int mdx_graph_create(int64_t N, int64_t E, const int64_t* ei, const int64_t* bn, int64_t B,
                                const int64_t* mol_ids, mdx_graph_t* out) {
  if (!out || (E > 0 && !ei) || (N > 0 && !bn) || B < 0) return fail(MDX_ERR_ARG, "null argument");
  HostPlan p;
  int rc = plan_graph(N, E, ei, p);
  if (rc) return rc;
  std::vector<int32_t> node_graph(N), node_local(N);
  {
    int64_t prev = -1, cnt = 0;
    for (int64_t v = 0; v < N; ++v) {
      if (bn[v] < 0 || bn[v] >= B) return fail(MDX_ERR_ARG, "batch_node[%lld] out of range", (long long)v);
      if (bn[v] < prev) return fail(MDX_ERR_ARG, "batch_node must be non-decreasing");
      if (bn[v] != prev) cnt = 0;
      node_graph[v] = (int32_t)bn[v];
      node_local[v] = (int32_t)cnt++;
      prev = bn[v];
    }
  }
  // half-edge bookkeeping (reference order: first E/2 columns are the i<j pairs, model.py:269)
  const int64_t Eh = E / 2;
  std::vector<int32_t> he_graph(Eh), he_local(Eh);
  {
    int64_t prev = -1, cnt = 0;
    for (int64_t h = 0; h < Eh; ++h) {
      const int64_t gph = bn[ei[h]];
      if (gph != prev) cnt = 0;
      he_graph[h] = (int32_t)gph;
      he_local[h] = (int32_t)cnt++;
      prev = gph;
    }
  }
  mdx_graph_s* g = new mdx_graph_s();
  g->N = N; g->E = E; g->Eh = Eh; g->B = B;
  std::vector<int32_t> slab;
  auto add = [&](const std::vector<int32_t>& v) {
    size_t off = (slab.size() + 63) & ~size_t(63);
    slab.resize(off + v.size() + 1, 0);
    std::copy(v.begin(), v.end(), slab.begin() + off);
    return off;
  };
  const size_t o_l = add(p.left), o_r = add(p.right), o_i2r = add(p.int2ref), o_r2i = add(p.ref2int), o_rp = add(p.row_ptr),
               o_cp = add(p.col_ptr), o_ce = add(p.col_eids), o_ng = add(node_graph), o_nl = add(node_local),
               o_hg = add(he_graph), o_hl = add(he_local);
  std::vector<int32_t> node_ptr(B + 1, 0), he_ptr(B + 1, 0);
  for (int64_t v = 0; v < N; ++v) node_ptr[bn[v] + 1]++;
  for (int64_t h = 0; h < Eh; ++h) he_ptr[he_graph[h] + 1]++;
  for (int64_t b = 0; b < B; ++b) { node_ptr[b + 1] += node_ptr[b]; he_ptr[b + 1] += he_ptr[b]; }
  const size_t o_np = add(node_ptr), o_hp = add(he_ptr);
  // Units of 16 edges aligned to each graph's first edge (aligned_units; edges are sorted by left node).  A node's run is cut
  // where a unit ends, so the cuts -- and the association of the in-kernel sums -- are a function of the graph alone, not of its
  // offset in the batch.
  const std::vector<int32_t> units = aligned_units(p.row_ptr, node_ptr);
  std::vector<int32_t> epo(E), pbase(N + 1, 0);
  {
    const int64_t U = (int64_t)units.size() / 2;
    int64_t u = 0;  // unit of the current edge (units are in edge order)
    for (int64_t v = 0; v < N; ++v) {
      const int32_t r0 = p.row_ptr[v], r1 = p.row_ptr[v + 1];
      int32_t pieces = 0, ufirst = 0;
      if (r1 > r0) {
        while (u + 1 < U && units[2 * (u + 1)] <= r0) ++u;
        ufirst = (int32_t)u;
        int64_t ul = u;
        while (ul + 1 < U && units[2 * (ul + 1)] <= r1 - 1) ++ul;
        pieces = (int32_t)(ul - u + 1);
      }
      pbase[v + 1] = pbase[v] + pieces;
      for (int32_t e = r0; e < r1; ++e) epo[e] = pbase[v] - ufirst;
    }
  }
  g->nunits = (int64_t)units.size() / 2;
  g->nparts = pbase[N];
  const size_t o_un = add(units), o_epo = add(epo), o_pb = add(pbase);
  // by-right twin: graph b owns the col positions col_ptr[node_ptr[b]] .. col_ptr[node_ptr[b+1]] (col_eids is ordered by right node)
  const std::vector<int32_t> units_r = aligned_units(p.col_ptr, node_ptr);
  std::vector<int32_t> epo_r(E), pbase_r(N + 1, 0), col_left(E), col_right(E);
  for (int64_t j = 0; j < E; ++j) { col_left[j] = p.left[p.col_eids[j]]; col_right[j] = p.right[p.col_eids[j]]; }
  {
    const int64_t U = (int64_t)units_r.size() / 2;
    int64_t u = 0;
    for (int64_t v = 0; v < N; ++v) {
      const int32_t r0 = p.col_ptr[v], r1 = p.col_ptr[v + 1];
      int32_t pieces = 0, ufirst = 0;
      if (r1 > r0) {
        while (u + 1 < U && units_r[2 * (u + 1)] <= r0) ++u;
        ufirst = (int32_t)u;
        int64_t ul = u;
        while (ul + 1 < U && units_r[2 * (ul + 1)] <= r1 - 1) ++ul;
        pieces = (int32_t)(ul - u + 1);
      }
      pbase_r[v + 1] = pbase_r[v] + pieces;
      for (int32_t j = r0; j < r1; ++j) epo_r[j] = pbase_r[v] - ufirst;
    }
  }
  g->nunits_r = (int64_t)units_r.size() / 2;
  g->nparts_r = pbase_r[N];
  const size_t o_unr = add(units_r), o_epor = add(epo_r), o_pbr = add(pbase_r), o_cl = add(col_left), o_cr = add(col_right);
  std::vector<int32_t> half_of_int(E);
  for (int64_t i = 0; i < E; ++i) half_of_int[i] = Eh > 0 ? (int32_t)(p.int2ref[i] % Eh) : 0;
  const size_t o_hoi = add(half_of_int);
  const size_t o_wq = add(std::vector<int32_t>((size_t)MDX_WQ_SET_INTS * MDX_WQ_SETS, 0));  // work-queue counters: all zero between launches
  if (hipMalloc((void**)&g->dev, slab.size() * 4) != hipSuccess ||
      hipMemcpy(g->dev, slab.data(), slab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    delete g;
    return fail(MDX_ERR_HIP, "graph upload failed: %s", hipGetErrorString(hipGetLastError()));
  }
  std::vector<int64_t> ids(B);
  for (int64_t i = 0; i < B; ++i) ids[i] = mol_ids ? mol_ids[i] : i;
  if (hipMalloc((void**)&g->mol_ids, std::max<int64_t>(B, 1) * 8) != hipSuccess ||
      (B > 0 && hipMemcpy(g->mol_ids, ids.data(), B * 8, hipMemcpyHostToDevice) != hipSuccess)) {
    hipFree(g->dev);
    delete g;
    return fail(MDX_ERR_HIP, "graph upload failed");
  }
  g->left = g->dev + o_l; g->right = g->dev + o_r; g->int2ref = g->dev + o_i2r; g->ref2int = g->dev + o_r2i;
  g->row_ptr = g->dev + o_rp; g->col_ptr = g->dev + o_cp; g->col_eids = g->dev + o_ce; g->node_graph = g->dev + o_ng;
  g->node_local = g->dev + o_nl; g->he_graph = g->dev + o_hg; g->he_local = g->dev + o_hl;
  g->half_of_int = g->dev + o_hoi;
  g->node_ptr = g->dev + o_np;
  g->he_ptr = g->dev + o_hp;
  g->units = g->dev + o_un; g->epo = g->dev + o_epo; g->pbase = g->dev + o_pb;
  g->units_r = g->dev + o_unr; g->epo_r = g->dev + o_epor; g->pbase_r = g->dev + o_pbr; g->col_left = g->dev + o_cl;
  g->col_right = g->dev + o_cr;
  g->wq = g->dev + o_wq;
  *out = g;
  return MDX_OK;
}

extern "C" int mdx_graph_destroy(mdx_graph_t g) {
  if (!g) return MDX_OK;
  if (g->dev) hipFree(g->dev);
  if (g->mol_ids) hipFree(g->mol_ids);
  if (g->ev_in) hipEventDestroy(g->ev_in);
  if (g->ev_done) hipEventDestroy(g->ev_done);
  delete g;
  return MDX_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
namespace {
struct Ws {
  float *Hn, *H, *NT, *NT2, *aggr, *SL, *SR, *Lf, *Rf, *tn, *posA, *posB;
  float *HeA, *HeB, *M, *FL, *FR, *Fe, *te, *tnr, *tmpE;  // tmpE: (E,64) scratch for boundary permutes
  float *P, *PR;  // partial rows of the in-kernel aggregation: (2N + E/16 + 1) x 256 / x 64 (bound on a graph's partial rows)
  bool tnr_set;  // tnr holds node_time[right] (only the bare NodeEdgeNet API can make it differ from te)
  size_t bytes;
};

size_t ws_layout(int64_t N, int64_t E, char* base, Ws* w) {
  size_t off = 0;
  auto take = [&](size_t nfloat) {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += ((nfloat * 4 + 255) / 256) * 256;
    return p;
  };
  const size_t n = (size_t)std::max<int64_t>(N, 1), e = (size_t)std::max<int64_t>(E, 1);
  Ws t{};
  t.Hn = take(n * MDX_ND); t.H = take(n * MDX_ND); t.NT = take(n * MDX_NTW); t.NT2 = take(n * MDX_NTW); t.aggr = take(n * MDX_ND);
  t.SL = take(n * 64); t.SR = take(n * 64); t.Lf = take(n * 64); t.Rf = take(n * 64); t.tn = take(n);
  t.posA = take(n * 3); t.posB = take(n * 3);
  t.HeA = take(e * 64); t.HeB = take(e * 64); t.M = take(e * MDX_ND); t.FL = take(e * 64); t.FR = take(e * 64);
  t.Fe = take(e * 3); t.te = take(e); t.tnr = take(e); t.tmpE = take(e * 64);
  // every node with edges has one piece per unit its run touches: <= N + (#units) <= N + (E/16 + #graphs) <= 2N + E/16 rows
  const size_t np = 2 * n + e / 16 + 1;
  t.P = take(np * MDX_ND); t.PR = take(np * 64);
  t.bytes = off;
  if (w) *w = t;
  return off;
}
}  // namespace

extern "C" size_t mdx_workspace_bytes(int64_t N, int64_t E) { return ws_layout(N, E, nullptr, nullptr); }

// ------------------------------------------------------------------------------------------------
// small utility kernels (permutes at the ABI boundary)
// ------------------------------------------------------------------------------------------------
__global__ void gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ idx, float* __restrict__ dst,
                                   int n, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n * C) return;
  const int r = i / C, c = i - (size_t)r * C;
  dst[i] = src[(size_t)idx[r] * C + c];
}
static void gather_rows(const float* src, const int* idx, float* dst, int64_t n, int C, hipStream_t s) {
  if (n <= 0) return;
  const size_t tot = (size_t)n * C;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((tot + 255) / 256), dim3(256), 0, s, src, idx, dst, (int)n, C);
}



// ------------------------------------------------------------------------------------------------
// live kernel timing (hipEvents on the launch stream) -- used by bench.py for the roofline numbers
// ------------------------------------------------------------------------------------------------
namespace {
enum { PK_EDGE_A = 0, PK_EDGE_B = 1, PK_NODE = 2, PK_AGGR = 3, PK_EDGE_BWD = 4, PK_COUNT = 5 };
constexpr int PROF_RING = 1024;
struct ProfSlot {
  hipEvent_t a[PROF_RING], b[PROF_RING];
  bool made = false;
  int head = 0, pending = 0;
  double total_ms = 0.0;
  long long count = 0;
};
unsigned g_prof_mask = 0;  // bit k: kernel k is timed
ProfSlot g_prof[PK_COUNT];

void prof_drain(ProfSlot& p, int n) {
  for (; n > 0 && p.pending > 0; --n, --p.pending) {
    const int i = (p.head - p.pending + PROF_RING * 4) % PROF_RING;
    hipEventSynchronize(p.b[i]);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a[i], p.b[i]) == hipSuccess) {
      p.total_ms += ms;
      p.count++;
    }
  }
}
struct ProfScope {
  ProfSlot* p = nullptr;
  hipStream_t s;
  int i = 0;
  ProfScope(int k, hipStream_t st) : s(st) {
    if (!((g_prof_mask >> k) & 1u)) return;
    p = &g_prof[k];
    if (!p->made) {
      for (int j = 0; j < PROF_RING; ++j) {
        hipEventCreate(&p->a[j]);
        hipEventCreate(&p->b[j]);
      }
      p->made = true;
    }
    if (p->pending == PROF_RING) prof_drain(*p, PROF_RING / 2);
    i = p->head;
    hipEventRecord(p->a[i], s);
  }
  ~ProfScope() {
    if (!p) return;
    hipEventRecord(p->b[i], s);
    p->head = (p->head + 1) % PROF_RING;
    p->pending++;
  }
};
}  // namespace

extern "C" int mdx_profile_enable(int32_t on) {
  g_prof_mask = on == 1 ? ~0u : (unsigned)on >> 1;  // 0 off, 1 all kernels, else bit (k+1) selects kernel k
  if (on)
    for (auto& p : g_prof) { prof_drain(p, PROF_RING); p.total_ms = 0.0; p.count = 0; }
  return MDX_OK;
}
// name of the kernel function slot `kernel` brackets in THIS build (bench.py checks a committed PMC summary against it before
// quoting its traffic figure)
extern "C" const char* mdx_profile_kernel_name(int32_t kernel) {
  switch (kernel) {
    case PK_EDGE_A: return "edge_a2_kernel<15>";
    case PK_EDGE_B: return "edge_b2_kernel";
    case PK_NODE: return "node_kernel";
    case PK_AGGR: return "";   // the reduction left after edge kernel A's in-kernel sums runs inside node_kernel
    case PK_EDGE_BWD: return "edge_bwd2_kernel";
    default: return "";
  }
}
extern "C" int mdx_profile_read(int32_t kernel, int64_t* count, double* total_ms) {
  if (kernel < 0 || kernel >= PK_COUNT || !count || !total_ms) return fail(MDX_ERR_ARG, "bad argument");
  prof_drain(g_prof[kernel], PROF_RING);
  *count = g_prof[kernel].count;
  *total_ms = g_prof[kernel].total_ms;
  return MDX_OK;
}

// ------------------------------------------------------------------------------------------------
// block driver
// ------------------------------------------------------------------------------------------------
namespace {

#define CHECK_READY(m, g, ws, ws_bytes)                                                                    \
  if (!(m) || !(g)) return fail(MDX_ERR_ARG, "null handle");                                               \
  if (!(m)->finalized) return fail(MDX_ERR_STATE, "model not finalized (call mdx_model_finalize)");        \
  if (!(ws) || (ws_bytes) < mdx_workspace_bytes((g)->N, (g)->E))                                           \
    return fail(MDX_ERR_STATE, "workspace too small: need %zu bytes", mdx_workspace_bytes((g)->N, (g)->E)); \
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(MDX_ERR_ARG, "workspace must be 256-byte aligned");

EdgeAArgs make_ea(const mdx_model_s* m, const mdx_graph_s* g, const Ws& w, int i, const float* pos, const float* He_in,
                  float* He_out, int flags, const float* NT = nullptr) {
  EdgeAArgs a{};
  a.E = (int)g->E; a.flags = flags; a.l = g->left; a.r = g->right; a.te = w.te; a.tn_r = w.tnr_set ? w.tnr : nullptr;
  a.pos = pos; a.dist_in = nullptr;
  a.soff = m->soff; a.scoef = m->scoef; a.cutoff = m->cfg.cutoff; a.smear_start = m->smear_start; a.He_in = He_in; a.He_out = He_out; a.H = w.H; a.NT = NT ? NT : w.NT;
  a.M = w.M; a.F[0] = w.FL; a.F[1] = w.FR; a.w = m->blocks[i].ea;
  if (flags & EA_AGG) {  // segment sums inside the kernel: M and the BondFFN-right rows stay out of HBM
    a.M = nullptr; a.F[1] = nullptr;
    a.units = g->units; a.nunits = (int)g->nunits; a.epo = g->epo; a.P = w.P; a.PR = w.PR;
  }
  return a;
}

#define LCHK(x)                    \
  do {                             \
    const int rc_ = (x);           \
    if (rc_ != MDX_OK) return rc_; \
  } while (0)

EdgeBArgs make_eb(const mdx_model_s* m, const mdx_graph_s* g, const Ws& w, int i, const float* pos, const float* Hep,
                  float* He_out, int flags, const float* NT = nullptr) {
  EdgeBArgs a{};
  a.E = (int)g->E; a.flags = flags; a.l = g->left; a.r = g->right; a.te = w.te; a.pos = pos; a.rel_in = nullptr;
  a.dist_in = nullptr; a.Hep = Hep; a.SL = w.SL; a.SR = w.SR; a.NT = NT ? NT : w.NT; a.He_out = He_out; a.Lf = w.Lf; a.Rf = w.Rf;
  a.Fe = w.Fe; a.w = m->blocks[i].eb;
  return a;
}

// Work-queue counters of the persistent edge kernels (mdx_row.h, WorkQ): a set per stream that launches on this graph, because
// launches that share a set must be ordered (the guidance chain runs on a second stream beside the denoiser).  A fifth stream
// gets none: its launches use the static split.  MDX_STATIC_SPLIT=1 turns the queues off (A/B).
int* wq_for(const mdx_graph_s* gc, hipStream_t s) {
  static const bool off = [] {
    const char* e = getenv("MDX_STATIC_SPLIT");
    return e && e[0] == '1';
  }();
  mdx_graph_s* g = const_cast<mdx_graph_s*>(gc);
  if (off || !g->wq) return nullptr;
  std::lock_guard<std::mutex> lk(g->wq_mu);
  for (int i = 0; i < g->wq_n; ++i)
    if (g->wq_stream[i] == s) return g->wq + (size_t)MDX_WQ_SET_INTS * i;
  if (g->wq_n == MDX_WQ_SETS) return nullptr;
  g->wq_stream[g->wq_n] = s;
  return g->wq + (size_t)MDX_WQ_SET_INTS * g->wq_n++;
}
// The split float16 forward kernels take the STATIC split: their waves then run identical programs from a common start and stay close
// enough for the L1 to serve the weight fragments one wave pulled to the other three (tools/ubench_split.hip UB_DESYNC: 23 vs 29
// cycles per MFMA), which is worth more to them than the queues' balance -- kernel A 373.5 vs 385.0 us per launch, kernel B 134.5 vs
// 136.0 (profiles/r4_split_phase_trace.txt).  The exact kernels are bound by the matrix pipe and keep the queues (6.95 vs 6.96 ms per
// step either way).  Results do not depend on the distribution (tests/test_gpu_round3.py static-vs-queue parity).
int run_ea(const mdx_graph_s* g, EdgeAArgs a, hipStream_t s) {
  a.wq = (a.flags & EA_SPLIT) ? nullptr : wq_for(g, s);
  return launch_edge_a(a, s);
}
int run_eb(const mdx_graph_s* g, EdgeBArgs a, hipStream_t s) {
  a.wq = (a.flags & EB_SPLIT) ? nullptr : wq_for(g, s);
  return launch_edge_b(a, s);
}

NodeArgs make_nd(const mdx_model_s* m, const mdx_graph_s* g, const Ws& w, int imid, int ipre, int flags,
                 const float* NTin = nullptr, float* NTout = nullptr) {
  NodeArgs a{};
  a.N = (int)g->N; a.flags = flags; a.Hn = w.Hn; a.aggr = w.aggr; a.NTin = NTin ? NTin : w.NT; a.dHn = nullptr; a.Lf = w.Lf;
  a.Rf = w.Rf; a.H = w.H; a.NT = NTout ? NTout : w.NT;
  if (imid >= 0) { a.wmid = m->blocks[imid].nd; a.smid = m->blocks[imid].nds; }
  if (ipre >= 0) { a.wpre = m->blocks[ipre].nd; a.spre = m->blocks[ipre].nds; }
  if (m->matrix_path == MDX_MATRIX_SPLIT_F16) a.flags |= ND_SPLIT;
  return a;
}

// Runs all blocks.  In: w.Hn, w.HeA (internal order), pos_in, w.tn / w.te.  Out: w.Hn, He (returned pointer), pos (returned).
// (Round 3 tried the next block's PRE stage on a low-priority side stream behind edge kernel B, to back-fill the CUs its early
// finishers free: the dispatcher interleaves both kernels from the start and the step got slower, 7.41 vs 6.99 ms; removed.)
int run_blocks(const mdx_model_s* m, mdx_graph_s* g, const Ws& w, const float* pos_in, const float** He_final,
               const float** pos_final, hipStream_t s, float* pos_out = nullptr) {
  const int nb = m->cfg.num_blocks;
  const bool upos = m->cfg.update_pos != 0;
  const float* pos = pos_in;
  float* pos_next = w.posA;
  // The per-node table is double-buffered: edge kernel B of block i still reads block i's table (node_ffn columns)
  // after the node kernel has already produced block i+1's table.
  float* NTcur = w.NT;
  float* NTnxt = w.NT2;
  const int split_a = m->matrix_path == MDX_MATRIX_SPLIT_F16 ? EA_SPLIT : 0, split_b = split_a ? EB_SPLIT : 0;
  launch_node(make_nd(m, g, w, -1, 0, ND_PRE, nullptr, NTcur), s);
  for (int i = 0; i < nb; ++i) {
    {
      ProfScope ps(PK_EDGE_A, s);
      LCHK(run_ea(g, make_ea(m, g, w, i, pos, w.HeA, w.HeB, EA_EMB | EA_NODE | EA_FFN | EA_AGG | split_a, NTcur), s));
    }
    // The reduction that is left after edge kernel A's in-kernel sums (combine ~2.5 partial rows per node, the by-right BondFFN sum)
    // is done by the node kernel itself for its 16 nodes: MID of this block + PRE of the next in one launch.
    const bool pre = i + 1 < nb;
    {
      ProfScope ps(PK_NODE, s);
      NodeArgs na = make_nd(m, g, w, i, pre ? i + 1 : -1, ND_MID | (upos ? ND_POSMLP : 0) | (pre ? ND_PRE : 0), NTcur, NTnxt);
      na.P = w.P; na.PR = w.PR; na.FL = w.FL; na.pbase = g->pbase; na.col_ptr = g->col_ptr; na.col_eids = g->col_eids;
      na.SL = w.SL; na.SR = w.SR;
      launch_node(na, s);
    }
    {
      ProfScope ps(PK_EDGE_B, s);
      LCHK(run_eb(g, make_eb(m, g, w, i, pos, w.HeB, w.HeA, EB_EDGE | (upos ? EB_POS : 0) | split_b, NTcur), s));
    }
    if (upos) {
      if (pos_out && i + 1 == nb) pos_next = pos_out;  // the last update lands in the caller's buffer (no copy afterwards)
      launch_seg_reduce(w.Fe, g->row_ptr, nullptr, pos_next, pos, (int)g->N, 3, s);
      pos = pos_next;
      pos_next = (pos_next == w.posA) ? w.posB : w.posA;
    }
    std::swap(NTcur, NTnxt);
  }
  *He_final = w.HeA;
  *pos_final = pos;
  return MDX_OK;
}

}  // namespace

extern "C" int mdx_net_forward(mdx_model_t m, mdx_graph_t g, const float* h_node, const float* pos, const float* h_edge,
                               const float* node_time, const float* edge_time, float* h_node_out, float* pos_out,
                               float* h_edge_out, void* ws, size_t ws_bytes, void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (!h_node || !pos || !h_edge || !node_time || !edge_time) return fail(MDX_ERR_ARG, "null input");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  HIPCHK(hipMemcpyAsync(w.Hn, h_node, (size_t)g->N * MDX_ND * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(w.tn, node_time, (size_t)g->N * 4, hipMemcpyDeviceToDevice, s));
  gather_rows(h_edge, g->int2ref, w.HeA, g->E, 64, s);
  gather_rows(edge_time, g->int2ref, w.te, g->E, 1, s);
  gather_rows(node_time, g->right, w.tnr, g->E, 1, s);
  w.tnr_set = true;
  const float *He, *pf;
  LCHK(run_blocks(m, g, w, pos, &He, &pf, s));
  if (h_node_out) HIPCHK(hipMemcpyAsync(h_node_out, w.Hn, (size_t)g->N * MDX_ND * 4, hipMemcpyDeviceToDevice, s));
  if (pos_out) HIPCHK(hipMemcpyAsync(pos_out, pf, (size_t)g->N * 12, hipMemcpyDeviceToDevice, s));
  if (h_edge_out) gather_rows(He, g->ref2int, h_edge_out, g->E, 64, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_node_block(mdx_model_t m, mdx_graph_t g, int32_t i, const float* x, const float* edge_attr,
                              const float* node_time, float* out, void* ws, size_t ws_bytes, void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (i < 0 || i >= m->cfg.num_blocks || !x || !edge_attr || !node_time || !out) return fail(MDX_ERR_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  HIPCHK(hipMemcpyAsync(w.Hn, x, (size_t)g->N * MDX_ND * 4, hipMemcpyDeviceToDevice, s));
  gather_rows(edge_attr, g->int2ref, w.HeA, g->E, 64, s);
  // NodeBlock's gate sees node_time[col]: per-edge time = node_time[right]
  gather_rows(node_time, g->right, w.te, g->E, 1, s);
  launch_node(make_nd(m, g, w, -1, i, ND_PRE), s);
  LCHK(run_ea(g, make_ea(m, g, w, i, nullptr, w.HeA, w.HeA, EA_NODE), s));
  launch_seg_reduce(w.M, g->row_ptr, nullptr, w.aggr, nullptr, (int)g->N, 256, s);
  NodeArgs na = make_nd(m, g, w, i, -1, ND_MID | ND_DELTA);
  na.dHn = out;
  launch_node(na, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_edge_block(mdx_model_t m, mdx_graph_t g, int32_t i, const float* h_bond, const float* h_node,
                              const float* bond_time, float* out, void* ws, size_t ws_bytes, void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (i < 0 || i >= m->cfg.num_blocks || !h_bond || !h_node || !bond_time || !out) return fail(MDX_ERR_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  HIPCHK(hipMemcpyAsync(w.Hn, h_node, (size_t)g->N * MDX_ND * 4, hipMemcpyDeviceToDevice, s));
  gather_rows(h_bond, g->int2ref, w.HeA, g->E, 64, s);
  gather_rows(bond_time, g->int2ref, w.te, g->E, 1, s);
  launch_node(make_nd(m, g, w, -1, i, ND_PRE), s);
  LCHK(run_ea(g, make_ea(m, g, w, i, nullptr, w.HeA, w.HeA, EA_FFN), s));
  launch_seg_reduce(w.FL, g->col_ptr, g->col_eids, w.SL, nullptr, (int)g->N, 64, s);
  launch_seg_reduce(w.FR, g->row_ptr, nullptr, w.SR, nullptr, (int)g->N, 64, s);
  LCHK(run_eb(g, make_eb(m, g, w, i, nullptr, w.HeA, w.HeB, EB_EDGE | EB_DELTA), s));
  gather_rows(w.HeB, g->ref2int, out, g->E, 64, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_bond_ffn(mdx_model_t m, mdx_graph_t g, int32_t i, int32_t side, const float* bond_feat, const float* node_feat,
                            const float* time, float* out, void* ws, size_t ws_bytes, void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (i < 0 || i >= m->cfg.num_blocks || side < 0 || side > 1 || !bond_feat || !node_feat || !time || !out)
    return fail(MDX_ERR_ARG, "bad argument");
  if (g->N != g->E) return fail(MDX_ERR_ARG, "mdx_bond_ffn expects the identity graph (edge e joins node e to itself)");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  // every edge is its own node: the hoisted node_linear / gate node parts become per-edge rows of the node table
  HIPCHK(hipMemcpyAsync(w.Hn, node_feat, (size_t)g->N * MDX_ND * 4, hipMemcpyDeviceToDevice, s));
  gather_rows(bond_feat, g->int2ref, w.HeA, g->E, 64, s);
  gather_rows(time, g->int2ref, w.te, g->E, 1, s);
  launch_node(make_nd(m, g, w, -1, i, ND_PRE), s);
  LCHK(run_ea(g, make_ea(m, g, w, i, nullptr, w.HeA, w.HeA, EA_FFN), s));
  gather_rows(side ? w.FR : w.FL, g->ref2int, out, g->E, 64, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_pos_update(mdx_model_t m, mdx_graph_t g, int32_t i, const float* h_node, const float* h_edge,
                              const float* rel, const float* dist, const float* edge_time, float* out, void* ws,
                              size_t ws_bytes, void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (!m->cfg.update_pos) return fail(MDX_ERR_STATE, "model has no pos blocks");
  if (i < 0 || i >= m->cfg.num_blocks || !h_node || !h_edge || !rel || !dist || !edge_time || !out)
    return fail(MDX_ERR_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  HIPCHK(hipMemcpyAsync(w.Hn, h_node, (size_t)g->N * MDX_ND * 4, hipMemcpyDeviceToDevice, s));
  gather_rows(h_edge, g->int2ref, w.HeA, g->E, 64, s);
  gather_rows(edge_time, g->int2ref, w.te, g->E, 1, s);
  gather_rows(rel, g->int2ref, w.M, g->E, 3, s);        // M reused as scratch for rel (E,3)
  gather_rows(dist, g->int2ref, w.FL, g->E, 1, s);      // FL reused as scratch for dist (E)
  launch_node(make_nd(m, g, w, i, -1, ND_POSMLP), s);
  EdgeBArgs eb = make_eb(m, g, w, i, nullptr, w.HeA, nullptr, EB_POS);
  eb.rel_in = w.M;
  eb.dist_in = w.FL;
  LCHK(run_eb(g, eb, s));
  launch_seg_reduce(w.Fe, g->row_ptr, nullptr, out, nullptr, (int)g->N, 3, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_segment_sum(mdx_graph_t g, const float* src, int32_t C, int32_t by_right, float* out, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!g || !src || !out) return fail(MDX_ERR_ARG, "null argument");
  if (C != 3 && C != 64 && C != 256) return fail(MDX_ERR_UNSUPPORTED, "C must be 3, 64 or 256");
  if (!ws || ws_bytes < mdx_workspace_bytes(g->N, g->E)) return fail(MDX_ERR_STATE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  const float* rows = src;
  if (!(by_right & 2)) {  // reference edge order -> internal order (bit 1 set: src already is in the graph plan's internal order)
    gather_rows(src, g->int2ref, w.M, g->E, C, s);
    rows = w.M;
  }
  if (by_right & 1)
    launch_seg_reduce(rows, g->col_ptr, g->col_eids, out, nullptr, (int)g->N, C, s);
  else
    launch_seg_reduce(rows, g->row_ptr, nullptr, out, nullptr, (int)g->N, C, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_moldiff_forward(mdx_model_t m, mdx_graph_t g, const float* h_node_pert, const float* pos_pert,
                                   const float* h_edge_pert, const float* h_halfedge_pert, const int64_t* t,
                                   float* pred_node, float* pred_pos, float* pred_halfedge, void* ws, size_t ws_bytes,
                                   void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (m->cfg.kind != MDX_KIND_MOLDIFF) return fail(MDX_ERR_STATE, "not a MolDiff model handle");
  if (g->N == 0) return MDX_OK;  // empty batch: nothing to compute, outputs are empty
  if (!h_node_pert || !pos_pert || (g->E > 0 && !h_edge_pert && !h_halfedge_pert) || !t)
    return fail(MDX_ERR_ARG, "null input");
  if (g->E % 2) return fail(MDX_ERR_ARG, "MolDiff.forward needs E = 2*Eh directed edges");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  const mdx_config& cf = m->cfg;
  EmbedArgs ea{};
  ea.N = (int)g->N; ea.E = (int)g->E; ea.Kn = cf.num_node_types; ea.Ke = cf.num_edge_types; ea.time_dim = cf.time_dim;
  ea.T = std::max(cf.num_timesteps, 1); ea.nd_emb = MDX_ND - cf.time_dim; ea.ed_emb = MDX_ED - cf.time_dim; ea.xn = h_node_pert;
  ea.int2ref = g->int2ref; ea.l = g->left; ea.r = g->right; ea.node_graph = g->node_graph; ea.t = t; ea.Wn = m->Wn;
  ea.We = m->We; ea.toff = m->toff; ea.tcoef = m->tcoef; ea.Hn = w.Hn; ea.He = w.HeA; ea.tn = w.tn; ea.te = w.te;
  if (h_edge_pert) {
    ea.xe = h_edge_pert;
  } else {  // both directions share the half-edge one-hot (model.py:273): the embed kernel folds reference row r onto r mod Eh
    ea.xe = h_halfedge_pert;
    ea.half_rows = (int)g->Eh;
  }
  launch_embed(ea, s);
  const float *He, *pf;
  LCHK(run_blocks(m, g, w, pos_pert, &He, &pf, s, m->cfg.update_pos ? pred_pos : nullptr));
  DecodeArgs da{};
  da.N = (int)g->N; da.Eh = (int)g->Eh; da.Kn = cf.num_node_types; da.Ke = cf.num_edge_types; da.Hn = w.Hn; da.He = He;
  da.ref2int = g->ref2int; da.nodedec = m->nodedec; da.edgedec = m->edgedec; da.pred_node = pred_node;
  da.pred_halfedge = pred_halfedge;
  launch_decode(da, s);
  if (pred_pos && pf != pred_pos) HIPCHK(hipMemcpyAsync(pred_pos, pf, (size_t)g->N * 12, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

// The transition of one move: position posterior, node posterior + Gumbel-max, half-edge posterior + Gumbel-max.  The rows come from the
// one-step tables `tb`, or, when the move is a jump (strided sampling), from `jr`.  MolDiff's class counts 8 / 6 take all five launches
// in one; other class counts the stand-alone ones.
static int step_transition(const mdx_config& cf, const mdx_tables* tb, const StepJumpRows* jr, int N, int Eh, const int64_t* t,
                           const int64_t* batch_node, const int64_t* batch_halfedge, const mdx_state* cur, const mdx_state* next,
                           const float* pred_node, const float* pred_pos, const float* pred_halfedge, const float* eps_pos,
                           const float* u_node, const float* u_halfedge, uint8_t* node_cls, uint8_t* halfedge_cls, hipStream_t s) {
  if (cf.num_node_types == 8 && cf.num_edge_types == 6) {
    StepTransArgs ta{};
    ta.N = N; ta.Eh = Eh; ta.T = cf.num_timesteps; ta.c0 = tb->pos_coef_x0; ta.ct = tb->pos_coef_xt; ta.sd = tb->pos_std;
    ta.node_q = tb->node_q_mats; ta.node_qT1 = tb->node_qT_onestep; ta.edge_q = tb->edge_q_mats; ta.edge_qT1 = tb->edge_qT_onestep;
    ta.t = t; ta.batch_node = batch_node; ta.batch_half = batch_halfedge; ta.pos = cur->pos; ta.pred_pos = pred_pos; ta.eps = eps_pos;
    ta.pred_node = pred_node; ta.log_node = cur->log_node; ta.u_node = u_node; ta.pred_half = pred_halfedge;
    ta.log_half = cur->log_halfedge; ta.u_half = u_halfedge; ta.pos_next = next->pos; ta.log_node_next = next->log_node;
    ta.h_node_next = next->h_node; ta.log_half_next = next->log_halfedge; ta.h_half_next = next->h_halfedge; ta.node_cls = node_cls;
    ta.half_cls = halfedge_cls;
    if (jr) launch_step_jump(ta, *jr, s);
    else launch_step_transition(ta, s);
    return MDX_OK;
  }
  if (jr && (cf.num_node_types < 2 || cf.num_node_types > 8 || cf.num_edge_types < 2 || cf.num_edge_types > 8))
    return fail(MDX_ERR_UNSUPPORTED, "jump posteriors: class counts %d / %d outside 2..8", cf.num_node_types, cf.num_edge_types);
  // a jump reads its tables' row with the schedule position as a launch scalar
  auto cat = [&](const float* q, const float* qT1, const float* qT_jump, int K, const float* pred, const float* log_vt,
                 const int64_t* batch, int n, float* out) {
    if (jr) launch_cat_posterior_jump(q, qT_jump, K, pred, 1, log_vt, t, nullptr, nullptr, jr->s, jr->row, batch, n, out, s);
    else launch_cat_posterior(q, qT1, K, cf.num_timesteps, pred, 1, log_vt, t, batch, n, out, s);
  };
  if (jr) launch_pos_posterior_jump(jr->c0, jr->ct, jr->sd, cur->pos, pred_pos, eps_pos, t, nullptr, jr->row, batch_node, N, next->pos, s);
  else launch_pos_posterior(tb->pos_coef_x0, tb->pos_coef_xt, tb->pos_std, cur->pos, pred_pos, eps_pos, t, batch_node, N, next->pos, s);
  cat(tb->node_q_mats, tb->node_qT_onestep, jr ? jr->node_qT : nullptr, cf.num_node_types, pred_node, cur->log_node, batch_node, N,
      next->log_node);
  launch_gumbel_argmax(next->log_node, u_node, cf.num_node_types, N, nullptr, next->h_node, s, node_cls);
  if (Eh > 0) {
    cat(tb->edge_q_mats, tb->edge_qT_onestep, jr ? jr->edge_qT : nullptr, cf.num_edge_types, pred_halfedge, cur->log_halfedge,
        batch_halfedge, Eh, next->log_halfedge);
    launch_gumbel_argmax(next->log_halfedge, u_halfedge, cf.num_edge_types, Eh, nullptr, next->h_halfedge, s, halfedge_cls);
  }
  return MDX_OK;
}

static int sample_step_core(mdx_model_t m, mdx_graph_t g, const mdx_tables* tb, const int64_t* t, const int64_t* batch_node,
                            const int64_t* batch_halfedge, const mdx_state* cur, const mdx_state* next, float* pred_node,
                            float* pred_pos, float* pred_halfedge, const float* eps_pos, const float* u_node,
                            const float* u_halfedge, uint8_t* node_cls, uint8_t* halfedge_cls, void* ws, size_t ws_bytes,
                            void* stream, const StepJumpRows* jr = nullptr) {  // jr: the move is a jump (strided sampling)
  if (!tb || !cur || !next) return fail(MDX_ERR_ARG, "null tables / state");
  if (!m || !g) return fail(MDX_ERR_ARG, "null handle");
  const int N = (int)g->N, Eh = (int)g->Eh;
  if (N == 0) return MDX_OK;
  if (!pred_node || !pred_pos || (Eh > 0 && !pred_halfedge) || !eps_pos || !u_node || (Eh > 0 && !u_halfedge) || !batch_node ||
      (Eh > 0 && !batch_halfedge))
    return fail(MDX_ERR_ARG, "null buffer");
  LCHK(mdx_moldiff_forward(m, g, cur->h_node, cur->pos, nullptr, cur->h_halfedge, t, pred_node, pred_pos, pred_halfedge, ws, ws_bytes,
                           stream));
  LCHK(step_transition(m->cfg, tb, jr, N, Eh, t, batch_node, batch_halfedge, cur, next, pred_node, pred_pos, pred_halfedge, eps_pos,
                       u_node, u_halfedge, node_cls, halfedge_cls, (hipStream_t)stream));
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_sample_step(mdx_model_t m, mdx_graph_t g, const mdx_tables* tb, const int64_t* t, const int64_t* batch_node,
                               const int64_t* batch_halfedge, const mdx_state* cur, const mdx_state* next, float* pred_node,
                               float* pred_pos, float* pred_halfedge, const float* eps_pos, const float* u_node,
                               const float* u_halfedge, void* ws, size_t ws_bytes, void* stream) {
  return sample_step_core(m, g, tb, t, batch_node, batch_halfedge, cur, next, pred_node, pred_pos, pred_halfedge, eps_pos, u_node,
                          u_halfedge, nullptr, nullptr, ws, ws_bytes, stream);
}

// every pointer of a state the transitions write (the half-edge ones only where there are half-edges)
static bool state_complete(const mdx_state* st, int Eh) {
  return st && st->h_node && st->pos && st->log_node && (Eh == 0 || (st->h_halfedge && st->log_halfedge));
}

// The noise of one move: drawn by the library into the caller's buffers (draw >= 0: one Philox launch, which also fills the time tensor
// t_buf with `step` when given one), or the caller's buffers as they are (draw < 0; t_buf then takes a launch of its own).
static int draw_or_use_noise(const mdx_graph_s* g, const mdx_step_noise* noise, int Kn, int Ke, hipStream_t s, int64_t* t_buf = nullptr,
                             int32_t step = 0) {
  if (!noise || !noise->eps_pos || !noise->u_node || (g->Eh > 0 && !noise->u_halfedge)) return fail(MDX_ERR_ARG, "null noise buffer");
  if (noise->draw >= 0)
    launch_philox_noise(noise->seed, noise->draw, g->node_graph, g->node_local, g->he_graph, g->he_local, g->mol_ids, (int)g->N,
                        (int)g->Eh, Kn, Ke, noise->eps_pos, noise->u_node, noise->u_halfedge, s, t_buf, step, t_buf ? (int)g->B : 0);
  else if (t_buf)
    launch_fill_i64(t_buf, step, (int)g->B, s);
  return MDX_OK;
}

// the body of mdx_sample_step_full and mdx_sample_jump_full: jr == nullptr is the chain's ordinary move step -> step - 1
static int sample_step_full_impl(mdx_model_t m, mdx_graph_t g, const mdx_tables* tb, int32_t step, const int64_t* batch_node,
                                 const int64_t* batch_halfedge, const mdx_state* cur, const mdx_state* next, float* pred_node,
                                 float* pred_pos, float* pred_halfedge, const mdx_step_noise* noise, int64_t* t_buf,
                                 uint8_t* node_cls, uint8_t* halfedge_cls, const mdx_guidance* gd, void* ws, size_t ws_bytes,
                                 void* stream, const StepJumpRows* jr) {
  if (!m || !g || !tb || !cur || !next || !noise || !t_buf) return fail(MDX_ERR_ARG, "null argument");
  if (m->cfg.kind != MDX_KIND_MOLDIFF) return fail(MDX_ERR_STATE, "not a MolDiff model handle");
  if (step < 0 || step >= m->cfg.num_timesteps) return fail(MDX_ERR_ARG, "step %d outside [0, %d)", step, m->cfg.num_timesteps);
  if (g->N == 0) return MDX_OK;
  hipStream_t s = (hipStream_t)stream;
  const mdx_config& cf = m->cfg;
  if (noise->draw >= 0 && (cf.num_node_types > 8 || cf.num_edge_types > 8)) return fail(MDX_ERR_ARG, "class counts must be in 1..8");
  LCHK(draw_or_use_noise(g, noise, cf.num_node_types, cf.num_edge_types, s, t_buf, step));
  // the guidance chain (default 'uncertainty' objective): on a side stream it is enqueued BEFORE the denoiser, so that it runs under
  // it; in line it comes after and reuses the denoiser's workspace
  const bool side = gd && gd->side_stream;
  hipStream_t gs = side ? (hipStream_t)gd->side_stream : s;
  auto chain = [&]() -> int {
    void* gws = side ? gd->ws2 : ws;
    const size_t gwb = side ? gd->ws2_bytes : ws_bytes;
    LCHK(mdx_bondpred_forward(gd->predictor, g, cur->h_node, cur->pos, t_buf, gd->logits, gws, gwb, gd->tape, gd->tape_bytes, gs));
    launch_uncertainty_grad(gd->logits, gd->predictor->cfg.num_edge_types, (int)g->Eh, gd->glogits, gs);
    return mdx_bondpred_backward(gd->predictor, g, cur->pos, gd->glogits, -gd->scale, gd->delta, gws, gwb, gd->tape, gd->tape_bytes, gs);
  };
  if (gd && (!gd->predictor || !gd->tape || !gd->logits || !gd->glogits || !gd->delta)) return fail(MDX_ERR_ARG, "incomplete mdx_guidance");
  if (side) {
    if (!gd->ws2) return fail(MDX_ERR_ARG, "a concurrent guidance chain needs its own workspace (ws2)");
    if (!g->ev_in) {
      HIPCHK(hipEventCreateWithFlags(&g->ev_in, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&g->ev_done, hipEventDisableTiming));
    }
    // everything the chain reads (state, t_buf) and the previous step's use of `delta` is ordered before this point
    HIPCHK(hipEventRecord(g->ev_in, s));
    HIPCHK(hipStreamWaitEvent(gs, g->ev_in, 0));
    LCHK(chain());
    HIPCHK(hipEventRecord(g->ev_done, gs));
  }
  LCHK(sample_step_core(m, g, tb, t_buf, batch_node, batch_halfedge, cur, next, pred_node, pred_pos, pred_halfedge, noise->eps_pos,
                        noise->u_node, noise->u_halfedge, node_cls, halfedge_cls, ws, ws_bytes, stream, jr));
  if (!gd) return MDX_OK;
  if (side) HIPCHK(hipStreamWaitEvent(s, g->ev_done, 0));
  else LCHK(chain());
  launch_add_inplace(next->pos, gd->delta, 3 * (int)g->N, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_sample_step_full(mdx_model_t m, mdx_graph_t g, const mdx_tables* tb, int32_t step, const int64_t* batch_node,
                                    const int64_t* batch_halfedge, const mdx_state* cur, const mdx_state* next, float* pred_node,
                                    float* pred_pos, float* pred_halfedge, const mdx_step_noise* noise, int64_t* t_buf,
                                    uint8_t* node_cls, uint8_t* halfedge_cls, const mdx_guidance* gd, void* ws, size_t ws_bytes,
                                    void* stream) {
  return sample_step_full_impl(m, g, tb, step, batch_node, batch_halfedge, cur, next, pred_node, pred_pos, pred_halfedge, noise, t_buf,
                               node_cls, halfedge_cls, gd, ws, ws_bytes, stream, nullptr);
}

extern "C" int mdx_sample_jump_full(mdx_model_t m, mdx_graph_t g, const mdx_tables* tb, const mdx_jump_tables* jt, int32_t position,
                                    int32_t step, const int64_t* batch_node, const int64_t* batch_halfedge, const mdx_state* cur,
                                    const mdx_state* next, float* pred_node, float* pred_pos, float* pred_halfedge,
                                    const mdx_step_noise* noise, int64_t* t_buf, uint8_t* node_cls, uint8_t* halfedge_cls,
                                    const mdx_guidance* gd, void* ws, size_t ws_bytes, void* stream) {
  if (!m || !jt) return fail(MDX_ERR_ARG, "null argument");
  if (!jt->levels || !jt->pos_coef_x0 || !jt->pos_coef_xt || !jt->pos_std || !jt->node_qT_jump || !jt->edge_qT_jump)
    return fail(MDX_ERR_ARG, "incomplete mdx_jump_tables");
  if (position < 0 || position >= jt->num) return fail(MDX_ERR_ARG, "schedule position %d outside [0, %d)", position, jt->num);
  const int T = m->cfg.num_timesteps;
  const int32_t t = jt->levels[position], sl = position + 1 < jt->num ? jt->levels[position + 1] : -1;
  if (t != step) return fail(MDX_ERR_ARG, "schedule position %d is level %d, not step %d", position, t, step);
  if (t < 0 || t >= T || sl >= t || sl < -1 || (sl < 0 && t != 0))
    return fail(MDX_ERR_ARG, "schedule levels %d -> %d at position %d: not a downward move inside [0, %d) that ends at 0", t, sl, position, T);
  StepJumpRows jr{};
  jr.c0 = jt->pos_coef_x0; jr.ct = jt->pos_coef_xt; jr.sd = jt->pos_std; jr.node_qT = jt->node_qT_jump; jr.edge_qT = jt->edge_qT_jump;
  jr.row = position; jr.s = sl > 0 ? sl : 0;
  return sample_step_full_impl(m, g, tb, step, batch_node, batch_halfedge, cur, next, pred_node, pred_pos, pred_halfedge, noise, t_buf,
                               node_cls, halfedge_cls, gd, ws, ws_bytes, stream, &jr);
}

extern "C" int mdx_scaffold_merge(mdx_graph_t g, const mdx_scaffold_tables* tb, int32_t level, const mdx_scaffold* sc,
                                  const mdx_step_noise* noise, const mdx_state* next, float log_off, uint8_t* node_cls,
                                  uint8_t* halfedge_cls, float* pred_node, float* pred_pos, float* pred_halfedge, void* stream) {
  if (!g || !tb || !sc || !next) return fail(MDX_ERR_ARG, "null argument");
  if (tb->Kn < 2 || tb->Kn > 8 || tb->Ke < 2 || tb->Ke > 8) return fail(MDX_ERR_UNSUPPORTED, "class counts must be in 2..8");
  if (level < -1 || level >= tb->T) return fail(MDX_ERR_ARG, "level %d outside [-1, %d)", level, tb->T);
  const int N = (int)g->N, Eh = (int)g->Eh;
  if (N == 0) return MDX_OK;
  if (!sc->node_type || !sc->node_pos || (Eh > 0 && !sc->halfedge_type) || !state_complete(next, Eh))
    return fail(MDX_ERR_ARG, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  ScaffoldMergeArgs a{};
  if (level >= 0) {
    if (!tb->alphas_bar || !tb->node_q_mats || (Eh > 0 && !tb->edge_q_mats)) return fail(MDX_ERR_ARG, "null table");
    LCHK(draw_or_use_noise(g, noise, tb->Kn, tb->Ke, s));
    a.eps = noise->eps_pos; a.u_node = noise->u_node; a.u_half = noise->u_halfedge;
  }
  a.N = N; a.Eh = Eh; a.Kn = tb->Kn; a.Ke = tb->Ke; a.level = level; a.log_off = log_off;
  a.alphas_bar = tb->alphas_bar; a.node_q = tb->node_q_mats; a.edge_q = tb->edge_q_mats;
  a.node_mask = sc->node_mask; a.half_mask = sc->halfedge_mask; a.node_type = sc->node_type; a.half_type = sc->halfedge_type;
  a.node_pos = sc->node_pos;
  a.pos = next->pos; a.h_node = next->h_node; a.log_node = next->log_node; a.h_half = next->h_halfedge; a.log_half = next->log_halfedge;
  a.node_cls = node_cls; a.half_cls = halfedge_cls;
  a.pred_node = pred_node; a.pred_pos = pred_pos; a.pred_half = pred_halfedge;
  launch_scaffold_merge(a, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_forward_jump(mdx_graph_t g, const mdx_forward_tables* tb, int32_t row, const uint8_t* node_cls_cur,
                                const uint8_t* halfedge_cls_cur, const float* pos_cur, const mdx_step_noise* noise,
                                const mdx_state* next, float log_off, uint8_t* node_cls, uint8_t* halfedge_cls, void* stream) {
  if (!g || !tb || !noise || !next) return fail(MDX_ERR_ARG, "null argument");
  if (tb->Kn < 2 || tb->Kn > 8 || tb->Ke < 2 || tb->Ke > 8) return fail(MDX_ERR_UNSUPPORTED, "class counts must be in 2..8");
  if (row < 0 || row >= tb->num) return fail(MDX_ERR_ARG, "table row %d outside [0, %d)", row, tb->num);
  const int N = (int)g->N, Eh = (int)g->Eh;
  if (N == 0) return MDX_OK;
  if (!tb->pos_coef_a || !tb->pos_coef_s || !tb->node_qT_jump || (Eh > 0 && !tb->edge_qT_jump)) return fail(MDX_ERR_ARG, "incomplete mdx_forward_tables");
  if (!node_cls_cur || !pos_cur || (Eh > 0 && !halfedge_cls_cur) || !state_complete(next, Eh)) return fail(MDX_ERR_ARG, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  LCHK(draw_or_use_noise(g, noise, tb->Kn, tb->Ke, s));
  ForwardJumpArgs a{};
  a.N = N; a.Eh = Eh; a.Kn = tb->Kn; a.Ke = tb->Ke; a.row = row; a.log_off = log_off;
  a.ca = tb->pos_coef_a; a.cs = tb->pos_coef_s; a.node_qT = tb->node_qT_jump; a.edge_qT = tb->edge_qT_jump;
  a.node_cls = node_cls_cur; a.half_cls = halfedge_cls_cur; a.pos = pos_cur;
  a.eps = noise->eps_pos; a.u_node = noise->u_node; a.u_half = noise->u_halfedge;
  a.pos_next = next->pos; a.h_node = next->h_node; a.log_node = next->log_node; a.h_half = next->h_halfedge; a.log_half = next->log_halfedge;
  a.node_cls_next = node_cls; a.half_cls_next = halfedge_cls;
  launch_forward_jump(a, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

// ------------------------------------------------------------------------------------------------
// bond predictor: forward with a per-block tape, and the data-gradient backward w.r.t. positions
// ------------------------------------------------------------------------------------------------
namespace {
struct TapeBlock {
  float *Hep, *Hn, *H, *NT, *aggr, *SL, *SR;
  float *SG, *HE, *M;  // (E,256): sigmoid(gate), edge_net output, gated message -- read back by edge_bwd instead of recomputed
  float *BL[2], *H1[2], *O[2];  // BondFFN intermediates (EdgeAArgs tBL / tH1 / tO), left and right: 2.5 KB per edge and block
};
struct Tape {
  std::vector<TapeBlock> b;
  float *HeF, *HnF, *te;                       // final states + per-edge time
  float *GGX, *GNL0, *GNL1, *GGXS0, *GGXS1, *GBN, *gdist, *tmpE3;  // backward scratch
  size_t bytes;
};
size_t tape_layout(int64_t N, int64_t E, int nb, char* base, Tape* t) {
  size_t off = 0;
  auto take = [&](size_t nfloat) {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += ((nfloat * 4 + 255) / 256) * 256;
    return p;
  };
  const size_t n = (size_t)std::max<int64_t>(N, 1), e = (size_t)std::max<int64_t>(E, 1);
  Tape tp;
  tp.b.resize(nb);
  for (int i = 0; i < nb; ++i) {
    TapeBlock& k = tp.b[i];
    k.Hep = take(e * 64); k.Hn = take(n * MDX_ND); k.H = take(n * MDX_ND); k.NT = take(n * MDX_NTW);
    k.aggr = take(n * MDX_ND); k.SL = take(n * 64); k.SR = take(n * 64);
    k.SG = take(e * MDX_ND); k.HE = take(e * MDX_ND); k.M = take(e * MDX_ND);
    for (int sd = 0; sd < 2; ++sd) { k.BL[sd] = take(e * 128); k.H1[sd] = take(e * 128); k.O[sd] = take(e * 64); }
  }
  tp.HeF = take(e * 64); tp.HnF = take(n * MDX_ND); tp.te = take(e);
  tp.GGX = take(e * MDX_ND); tp.GNL0 = take(e * 128); tp.GNL1 = take(e * 128); tp.GGXS0 = take(e * 32);
  tp.GGXS1 = take(e * 32); tp.GBN = take(e * 128); tp.gdist = take(e); tp.tmpE3 = take(e * 3);
  tp.bytes = off;
  if (t) *t = std::move(tp);
  return off;
}
}  // namespace

extern "C" size_t mdx_bondpred_tape_bytes(int64_t N, int64_t E, int32_t num_blocks) {
  return tape_layout(N, E, num_blocks, nullptr, nullptr);
}

extern "C" int mdx_bondpred_forward(mdx_model_t m, mdx_graph_t g, const float* h_node, const float* pos, const int64_t* t,
                                    float* logits, void* ws, size_t ws_bytes, void* tape, size_t tape_bytes, void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (m->cfg.kind != MDX_KIND_BONDPRED) return fail(MDX_ERR_STATE, "not a BondPredictor model handle");
  if (!h_node || !pos || !t || !logits) return fail(MDX_ERR_ARG, "null input");
  if (g->E % 2) return fail(MDX_ERR_ARG, "BondPredictor.forward needs E = 2*Eh directed edges");
  const int nb = m->cfg.num_blocks;
  if (tape && (tape_bytes < mdx_bondpred_tape_bytes(g->N, g->E, nb) || (reinterpret_cast<uintptr_t>(tape) & 255)))
    return fail(MDX_ERR_STATE, "tape too small or misaligned: need %zu bytes", mdx_bondpred_tape_bytes(g->N, g->E, nb));
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  Tape tp;
  if (tape) tape_layout(g->N, g->E, nb, (char*)tape, &tp);
  const mdx_config& cf = m->cfg;
  EmbedArgs ea{};
  ea.N = (int)g->N; ea.E = (int)g->E; ea.Kn = cf.num_node_types; ea.Ke = cf.num_edge_types; ea.time_dim = cf.time_dim;
  ea.T = std::max(cf.num_timesteps, 1); ea.nd_emb = MDX_ND - cf.time_dim; ea.ed_emb = MDX_ED - cf.time_dim; ea.xn = h_node; ea.xe = nullptr;
  ea.zero_time = cf.num_timesteps == 0;  // time-free predictor: the reference replaces t by zeros (bond_predictor.py:141-144), whatever the caller passes
  ea.int2ref = g->int2ref; ea.l = g->left; ea.r = g->right; ea.node_graph = g->node_graph; ea.t = t; ea.Wn = m->Wn;
  ea.We = m->We; ea.toff = m->toff; ea.tcoef = m->tcoef; ea.Hn = w.Hn; ea.He = w.HeA; ea.tn = w.tn;
  ea.te = tape ? tp.te : w.te;
  launch_embed(ea, s);
  Ws wr = w;
  wr.te = ea.te;
  const size_t nHn = (size_t)g->N * MDX_ND * 4;
  const int split_a = m->matrix_path == MDX_MATRIX_SPLIT_F16 ? EA_SPLIT : 0, split_b = split_a ? EB_SPLIT : 0;
  for (int i = 0; i < nb; ++i) {
    // same sequence as run_blocks (update_pos = false), with the per-block outputs redirected into the tape
    Ws wi = wr;
    float* Hep = wr.HeB;
    if (tape) {
      const TapeBlock& k = tp.b[i];
      wi.H = k.H; wi.NT = k.NT; wi.aggr = k.aggr; wi.SL = k.SL; wi.SR = k.SR; wi.M = k.M;
      Hep = k.Hep;
      HIPCHK(hipMemcpyAsync(k.Hn, wr.Hn, nHn, hipMemcpyDeviceToDevice, s));
    }
    // tape + in-kernel sums: the reduction, MID of this block and PRE of the next are ONE node launch as in run_blocks (round 3; it
    // used to be three plus the reduction kernel), with every output pointed straight at its tape buffer
    const bool fused_tape = tape != nullptr;
    if (i == 0) launch_node(make_nd(m, g, wi, -1, i, ND_PRE, nullptr, wi.NT), s);
    {
      EdgeAArgs ea_args = make_ea(m, g, wi, i, pos, wr.HeA, Hep, EA_EMB | EA_NODE | EA_FFN | EA_AGG, wi.NT);
      if (tape) {  // the launch also writes the guidance tape (template flags of the kernel)
        ea_args.flags |= EA_TAPE | EA_TAPE_FFN;
        ea_args.tSG = tp.b[i].SG;
        ea_args.tHE = tp.b[i].HE;
        ea_args.M = tp.b[i].M;  // the backward reads the gated message back (with EA_AGG it is no longer the reduction's input)
        for (int sd = 0; sd < 2; ++sd) { ea_args.tBL[sd] = tp.b[i].BL[sd]; ea_args.tH1[sd] = tp.b[i].H1[sd]; ea_args.tO[sd] = tp.b[i].O[sd]; }
      }
      ea_args.flags |= split_a;  // split float16 matrix path: the same launch on mdx_edge2s.hip
      { ProfScope ps(PK_EDGE_A, s); LCHK(run_ea(g, ea_args, s)); }
    }
    if (fused_tape) {
      const bool pre = i + 1 < nb;
      NodeArgs na = make_nd(m, g, wi, i, pre ? i + 1 : -1, ND_MID | (pre ? ND_PRE : 0), wi.NT, pre ? tp.b[i + 1].NT : nullptr);
      if (pre) na.H = tp.b[i + 1].H;
      na.P = wi.P; na.PR = wi.PR; na.FL = wi.FL; na.pbase = g->pbase; na.col_ptr = g->col_ptr; na.col_eids = g->col_eids;
      na.SL = wi.SL; na.SR = wi.SR; na.aggr_out = wi.aggr;
      launch_node(na, s);
      LCHK(run_eb(g, make_eb(m, g, wi, i, pos, Hep, wr.HeA, EB_EDGE | split_b, wi.NT), s));
      continue;
    }
    // no tape: the reduction left after the in-kernel sums as a launch of its own, then MID of this block fused with the next
    // block's PRE (tables double-buffered like run_blocks)
    launch_seg_reduce_block2(wi.P, wi.PR, wi.FL, g->pbase, g->col_ptr, g->col_eids, wi.aggr, wi.SL, wi.SR, (int)g->N, s);
    float* NTn = (wr.NT == w.NT) ? w.NT2 : w.NT;
    launch_node(make_nd(m, g, wi, i, i + 1 < nb ? i + 1 : -1, ND_MID | (i + 1 < nb ? ND_PRE : 0), wi.NT, NTn), s);
    LCHK(run_eb(g, make_eb(m, g, wi, i, pos, Hep, wr.HeA, EB_EDGE | split_b, wi.NT), s));
    wr.NT = NTn;
  }
  if (tape) {
    HIPCHK(hipMemcpyAsync(tp.HnF, wr.Hn, nHn, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(tp.HeF, wr.HeA, (size_t)g->E * 64 * 4, hipMemcpyDeviceToDevice, s));
  }
  BondDecArgs da{};
  da.Eh = (int)g->Eh; da.Ke = cf.num_edge_types; da.He = wr.HeA; da.Hn = wr.Hn; da.ref2int = g->ref2int; da.left = g->left;
  da.right = g->right; da.logits = logits; da.w = m->dec;
  launch_bond_decode(da, false, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

// gpos (N,3) = scale * dL/dpos given glogits = dL/dlogits (Eh,Ke); needs the tape of the matching forward.
extern "C" int mdx_bondpred_backward(mdx_model_t m, mdx_graph_t g, const float* pos, const float* glogits, float scale,
                                     float* gpos, void* ws, size_t ws_bytes, void* tape, size_t tape_bytes, void* stream) {
  CHECK_READY(m, g, ws, ws_bytes);
  if (m->cfg.kind != MDX_KIND_BONDPRED) return fail(MDX_ERR_STATE, "not a BondPredictor model handle");
  if (!pos || !glogits || !gpos || !tape) return fail(MDX_ERR_ARG, "null argument");
  const int nb = m->cfg.num_blocks;
  if (tape_bytes < mdx_bondpred_tape_bytes(g->N, g->E, nb) || (reinterpret_cast<uintptr_t>(tape) & 255))
    return fail(MDX_ERR_STATE, "tape too small or misaligned");
  hipStream_t s = (hipStream_t)stream;
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  Tape tp;
  tape_layout(g->N, g->E, nb, (char*)tape, &tp);
  const mdx_config& cf = m->cfg;
  const int N = (int)g->N, E = (int)g->E;
  // scratch mapping onto the (now dead) forward workspace
  float *gHn = w.Hn, *GNT = w.NT, *gH = w.H, *gHe = w.HeA, *GU = w.FL, *GHEP = w.FR, *GH = w.M;
  HIPCHK(hipMemsetAsync(tp.gdist, 0, (size_t)std::max(E, 1) * 4, s));
  BondDecArgs da{};
  da.Eh = (int)g->Eh; da.Ke = cf.num_edge_types; da.He = tp.HeF; da.Hn = tp.HnF; da.ref2int = g->ref2int; da.left = g->left;
  da.right = g->right; da.glogits = glogits; da.gHe = gHe; da.GBN = tp.GBN; da.w = m->dec;
  launch_bond_decode(da, true, s);
  launch_seg_reduce_ld(tp.GBN, g->row_ptr, g->half_of_int, gHn, MDX_ND, N, 256, s);
  for (int i = nb - 1; i >= 0; --i) {
    const TapeBlock& k = tp.b[i];
    NodeBwdArgs nt{};
    nt.N = N; nt.flags = NB_TAIL; nt.gHn = gHn; nt.Hn = k.Hn; nt.NTin = k.NT; nt.aggr = k.aggr; nt.GNT = GNT; nt.gH = gH;
    nt.w = m->blocks[i].nd; nt.wt = m->nbw[i]; nt.ws = m->blocks[i].nds; nt.wts = m->nbws[i];
    const int nb_split = m->matrix_path == MDX_MATRIX_SPLIT_F16 ? NB_SPLIT : 0;
    nt.flags |= nb_split;
    launch_node_bwd(nt, s);
    // EdgeBlock-tail backward: for the last block a launch of its own (its dL/dHe'' comes from the decoder); for every other
    // block it ran inside block i + 1's edge kernel, fused behind that block's edge_embs backward (GU, GHEP are ready)
    const bool split_bwd = m->matrix_path == MDX_MATRIX_SPLIT_F16;
    int* wq = wq_for(g, s);
    if (i == nb - 1) {
      EdgeTailBwdArgs et{};
      et.E = E; et.l = g->left; et.r = g->right; et.te = tp.te; et.Hep = k.Hep; et.gHe = gHe; et.SL = k.SL; et.SR = k.SR;
      et.NT = k.NT; et.GU = GU; et.GHEP = GHEP; et.w = m->blocks[i].eb;
      et.sWselfT = m->ebw[i].s.WselfT; et.sWoutT = m->ebw[i].s.WoutT; et.wq = wq;
      et.ssWselfT = m->ebw[i].ss.WselfT; et.ssWoutT = m->ebw[i].ss.WoutT;
      et.split = split_bwd ? 1 : 0;
      if (split_bwd) launch_edge_tail_bwd2s(et, s);
      else launch_edge_tail_bwd2(et, s);
    }
    launch_seg_reduce_tail_block(GU, g->row_ptr, g->col_ptr, g->col_eids, GNT, N, s);
    EdgeBwdArgs eb{};
    eb.E = E; eb.l = g->left; eb.r = g->right; eb.te = tp.te; eb.pos = pos; eb.soff = m->soff; eb.scoef = m->scoef;
    eb.cutoff = cf.cutoff; eb.smear_start = m->smear_start; eb.Hep = k.Hep; eb.GHEP = GHEP; eb.H = k.H; eb.NT = k.NT; eb.GNT = GNT;
    eb.SG = k.SG; eb.HE = k.HE; eb.M = k.M;
    for (int sd = 0; sd < 2; ++sd) { eb.BL[sd] = k.BL[sd]; eb.H1[sd] = k.H1[sd]; eb.O[sd] = k.O[sd]; }
    eb.gdist = tp.gdist; eb.GH = GH; eb.GGX = tp.GGX; eb.GNL[0] = tp.GNL0; eb.GNL[1] = tp.GNL1; eb.GGXS[0] = tp.GGXS0;
    eb.GGXS[1] = tp.GGXS1; eb.w = m->blocks[i].ea; eb.wt = m->ebw[i]; eb.wq = wq;
    eb.split = split_bwd ? 1 : 0;
    eb.fuse_tail = i > 0;
    if (i > 0) {
      const TapeBlock& kp = tp.b[i - 1];
      const EdgeBW& wb = m->blocks[i - 1].eb;
      eb.tHep = kp.Hep; eb.tSL = kp.SL; eb.tSR = kp.SR; eb.tNT = kp.NT; eb.tGU = GU; eb.tGHEP = GHEP;
      eb.tWself = split_bwd ? wb.ss.Wself : wb.s.Wself;
      eb.tWoutT = split_bwd ? m->ebw[i - 1].ss.WoutT : m->ebw[i - 1].s.WoutT;
      eb.tWselfT = split_bwd ? m->ebw[i - 1].ss.WselfT : m->ebw[i - 1].s.WselfT;
      eb.tbself = wb.bself; eb.tlng = wb.lng; eb.tlnb = wb.lnb;
    }
    eb.units_r = g->units_r; eb.epo_r = g->epo_r; eb.col_eids = g->col_eids; eb.col_left = g->col_left; eb.col_right = g->col_right;
    eb.nunits_r = (int)g->nunits_r;
    {
      ProfScope ps(PK_EDGE_BWD, s);
      if (split_bwd) {
        if (launch_edge_bwd2s(eb, s) != 0) return fail(MDX_ERR_STATE, "split float16 backward: the forward tape holds no BondFFN intermediates");
      } else launch_edge_bwd2(eb, s);
    }
    {
      SegBwdArgs sr{};
      sr.N = N; sr.row_ptr = g->row_ptr; sr.col_ptr = g->col_ptr; sr.col_eids = g->col_eids; sr.pbase_r = g->pbase_r; sr.GH = GH; sr.GGX = tp.GGX;
      sr.GNL0 = tp.GNL0; sr.GNL1 = tp.GNL1; sr.GGXS0 = tp.GGXS0; sr.GGXS1 = tp.GGXS1; sr.gH = gH; sr.GNT = GNT;
      launch_seg_reduce_bwd_block(sr, s);
    }
    nt.flags = NB_PRE | nb_split;
    launch_node_bwd(nt, s);
  }
  launch_dist_to_pos(tp.gdist, pos, g->left, g->right, g->row_ptr, g->col_ptr, g->col_eids, tp.tmpE3, nullptr, gpos, scale, N,
                     E, cf.cutoff, s);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

// ------------------------------------------------------------------------------------------------
// transitions
// ------------------------------------------------------------------------------------------------
extern "C" int mdx_pos_posterior(const float* c0, const float* ct, const float* sd, const float* x_t, const float* x_recon,
                                 const float* eps, const int64_t* t, const int64_t* batch, int64_t n, float* out,
                                 void* stream) {
  if (n < 0 || (n > 0 && (!c0 || !ct || !sd || !x_t || !x_recon || !eps || !t || !batch || !out)))
    return fail(MDX_ERR_ARG, "bad argument");
  launch_pos_posterior(c0, ct, sd, x_t, x_recon, eps, t, batch, (int)n, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_gauss_posterior(const float* c0, const float* ct, const float* sd, const float* x_t, const float* x_recon,
                                   const float* eps, const int64_t* t, const int64_t* batch, int64_t n, int32_t C, float* out,
                                   void* stream) {
  if (n < 0 || C < 1 || (n > 0 && (!c0 || !ct || !sd || !x_t || !x_recon || !eps || !t || !batch || !out)))
    return fail(MDX_ERR_ARG, "bad argument");
  launch_gauss_posterior(c0, ct, sd, x_t, x_recon, eps, t, batch, (int)n, (int)C, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_pos_posterior_jump(const float* c0, const float* ct, const float* sd, const float* x_t, const float* x_recon,
                                      const float* eps, const int64_t* t, const int64_t* row, const int64_t* batch, int64_t n, float* out,
                                      void* stream) {
  if (n == 0) return MDX_OK;
  if (!c0 || !ct || !sd || !x_t || !x_recon || !eps || !t || !row || !batch || !out) return fail(MDX_ERR_ARG, "null buffer");
  launch_pos_posterior_jump(c0, ct, sd, x_t, x_recon, eps, t, row, 0, batch, (int)n, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_cat_posterior_jump(const float* q_mats, const float* qT_jump, int32_t K, const float* in0, int32_t is_logits,
                                      const float* log_vt, const int64_t* t, const int64_t* t_prev, const int64_t* row,
                                      const int64_t* batch, int64_t n, float* out, void* stream) {
  if (K < 2 || K > 8) return fail(MDX_ERR_UNSUPPORTED, "class count %d outside 2..8", K);
  if (n == 0) return MDX_OK;
  if (!q_mats || !qT_jump || !in0 || !log_vt || !t || !t_prev || !row || !batch || !out) return fail(MDX_ERR_ARG, "null buffer");
  launch_cat_posterior_jump(q_mats, qT_jump, K, in0, is_logits, log_vt, t, t_prev, row, 0, 0, batch, (int)n, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_cat_posterior(const float* q_mats, const float* qT, int32_t K, int32_t T, const float* in0,
                                 int32_t is_logits, const float* log_vt, const int64_t* t, const int64_t* batch, int64_t n,
                                 float* out, void* stream) {
  if (K < 2 || K > 8) return fail(MDX_ERR_UNSUPPORTED, "K must be in 2..8");
  if (n < 0 || (n > 0 && (!q_mats || !qT || !in0 || !log_vt || !t || !batch || !out))) return fail(MDX_ERR_ARG, "bad argument");
  launch_cat_posterior(q_mats, qT, K, T, in0, is_logits, log_vt, t, batch, (int)n, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_op_cat_add_noise(const float* q_mats, int32_t K, int32_t T, const int64_t* v, const int64_t* t, const int64_t* batch,
                                    const float* u, int64_t n, float log_off, float* onehot, float* log_vt, float* log_v0, void* stream) {
  if (K < 2 || K > 8) return fail(MDX_ERR_UNSUPPORTED, "K must be in 2..8");
  if (n < 0 || T < 1 || (n > 0 && (!q_mats || !v || !t || !batch || !u || !onehot || !log_vt || !log_v0))) return fail(MDX_ERR_ARG, "bad argument");
  launch_cat_add_noise(q_mats, K, v, t, batch, u, (int)n, log_off, onehot, log_vt, log_v0, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_op_cat_loss(const float* q_mats, const float* qT, int32_t K, int32_t T, const float* logits, const float* log_vt,
                               const float* log_v0, const int64_t* t, const int64_t* batch, int64_t n, float* row_loss, float* dlogits,
                               void* stream) {
  if (K < 2 || K > 8) return fail(MDX_ERR_UNSUPPORTED, "K must be in 2..8");
  if (n < 0 || T < 1 || (n > 0 && (!q_mats || !qT || !logits || !log_vt || !log_v0 || !t || !batch || !row_loss || !dlogits)))
    return fail(MDX_ERR_ARG, "bad argument");
  launch_cat_loss(q_mats, qT, K, logits, log_vt, log_v0, t, batch, (int)n, row_loss, dlogits, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_gumbel_argmax(const float* logits, const float* u, int32_t K, int64_t n, int64_t* cls, float* onehot,
                                 void* stream) {
  if (K < 1 || n < 0 || (n > 0 && (!logits || !u))) return fail(MDX_ERR_ARG, "bad argument");
  launch_gumbel_argmax(logits, u, K, (int)n, cls, onehot, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_prior_draw(const double* logits64, int32_t K, const void* u, int32_t u_is_f64, int64_t n, int64_t* cls,
                              float* onehot, float* log_onehot, float log_off, uint8_t* cls8, void* stream) {
  if (K < 1 || K > 8 || n < 0 || !logits64 || (n > 0 && !u)) return fail(MDX_ERR_ARG, "bad argument");
  launch_prior_draw(logits64, K, u, u_is_f64 != 0, (int)n, cls, onehot, log_onehot, log_off, cls8, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

void launch_decode_output(const float* pred_node, int Kn, const float* pred_pos, const float* pred_halfedge, int Ke, int N,
                          int Eh, int B, const int* node_ptr, const int* he_ptr, const int* ref2int, const int* left,
                          const int* right, int num_element, int num_bond_types, int* scratch_i, float* scratch_f,
                          int* atom_type, float* atom_prob, float* atom_pos, int* n_atoms, int* bond_type,
                          float* bond_prob, int* bond_index, int* n_bonds, hipStream_t s);

extern "C" int mdx_decode_output(mdx_graph_t g, const float* pred_node, int32_t Kn, const float* pred_pos,
                                 const float* pred_halfedge, int32_t Ke, int32_t num_element, int32_t num_bond_types,
                                 int32_t* atom_type, float* atom_prob, float* atom_pos, int32_t* n_atoms,
                                 int32_t* bond_type, float* bond_prob, int32_t* bond_index, int32_t* n_bonds, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!g || !pred_node || !pred_pos || !pred_halfedge || !atom_type || !atom_prob || !atom_pos || !n_atoms || !bond_type ||
      !bond_prob || !bond_index || !n_bonds)
    return fail(MDX_ERR_ARG, "null argument");
  if (Kn < 1 || Ke < 1) return fail(MDX_ERR_ARG, "bad class count");
  if (!ws || ws_bytes < mdx_workspace_bytes(g->N, g->E)) return fail(MDX_ERR_STATE, "workspace too small");
  Ws w;
  ws_layout(g->N, g->E, (char*)ws, &w);
  if ((size_t)(2 * g->N + g->Eh) > (size_t)std::max<int64_t>(g->E, 1) * MDX_ND ||
      (size_t)(g->N + g->Eh) > (size_t)std::max<int64_t>(g->E, 1) * 64)
    return fail(MDX_ERR_UNSUPPORTED, "graph too sparse for the decode scratch layout");
  // scratch: ints in M (>= 2N + Eh words), floats in HeA (>= N + Eh words)
  launch_decode_output(pred_node, Kn, pred_pos, pred_halfedge, Ke, (int)g->N, (int)g->Eh, (int)g->B, g->node_ptr, g->he_ptr,
                       g->ref2int, g->left, g->right, num_element, num_bond_types, reinterpret_cast<int*>(w.M), w.HeA,
                       atom_type, atom_prob, atom_pos, n_atoms, bond_type, bond_prob, bond_index, n_bonds,
                       (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

// both entries use the first 3N ints of the workspace: labels | fragment sizes (mdx_mol_check), old -> new atom index (keep)
static int molcheck_scratch(mdx_graph_t g, void* ws, size_t ws_bytes, int** scratch) {
  const size_t need = (size_t)std::max<int64_t>(g->N, 1) * 3 * sizeof(int);
  if (!ws || ws_bytes < need) return fail(MDX_ERR_ARG, "workspace too small: need %zu bytes", need);
  if (reinterpret_cast<uintptr_t>(ws) & 3) return fail(MDX_ERR_ARG, "workspace must be 4-byte aligned");
  *scratch = reinterpret_cast<int*>(ws);
  return MDX_OK;
}

extern "C" int mdx_mol_check(mdx_graph_t g, const int32_t* atom_type, const float* atom_pos, const int32_t* n_atoms,
                             const int32_t* bond_type, const int32_t* bond_index, const int32_t* n_bonds, int32_t num_element,
                             int32_t num_bond_types, const int32_t* max_valence, int32_t* component, int32_t* valence2,
                             int32_t* n_components, int32_t* largest_size, int32_t* largest_label, int32_t* n_overvalent,
                             float* min_dist, float* max_bond_len, void* ws, size_t ws_bytes, void* stream) {
  if (!g || !atom_type || !atom_pos || !n_atoms || !bond_type || !bond_index || !n_bonds || !max_valence || !component ||
      !valence2 || !n_components || !largest_size || !largest_label || !n_overvalent || !min_dist || !max_bond_len)
    return fail(MDX_ERR_ARG, "null argument");
  if (num_element < 1 || num_bond_types < 1) return fail(MDX_ERR_ARG, "bad class count");
  int* scratch = nullptr;
  if (int rc = molcheck_scratch(g, ws, ws_bytes, &scratch)) return rc;
  MolCheckArgs a{(int)g->N, (int)g->Eh, (int)g->B, num_element, num_bond_types, g->node_ptr, g->he_ptr, atom_type, atom_pos,
                 n_atoms, bond_type, bond_index, n_bonds, max_valence, scratch, component, valence2, n_components,
                 largest_size, largest_label, n_overvalent, min_dist, max_bond_len};
  launch_mol_check(a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_mol_keep_component(mdx_graph_t g, const int32_t* select, const int32_t* label, const int32_t* component,
                                      int32_t* atom_type, float* atom_prob, float* atom_pos, int32_t* n_atoms,
                                      int32_t* bond_type, float* bond_prob, int32_t* bond_index, int32_t* n_bonds, void* ws,
                                      size_t ws_bytes, void* stream) {
  if (!g || !select || !label || !component || !atom_type || !atom_prob || !atom_pos || !n_atoms || !bond_type || !bond_prob ||
      !bond_index || !n_bonds)
    return fail(MDX_ERR_ARG, "null argument");
  int* scratch = nullptr;
  if (int rc = molcheck_scratch(g, ws, ws_bytes, &scratch)) return rc;
  MolKeepArgs a{(int)g->N, (int)g->Eh, (int)g->B, g->node_ptr, g->he_ptr, select, label, component, scratch + 2 * g->N,
                atom_type, atom_prob, atom_pos, n_atoms, bond_type, bond_prob, bond_index, n_bonds};
  launch_mol_keep_component(a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" size_t mdx_mol_local3d_ws_bytes(int64_t N_cap, int64_t Eh_stride) { return local3d_ws_bytes(N_cap, Eh_stride); }

extern "C" int mdx_mol_local3d(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms,
                               const int32_t* n_bonds, const int32_t* atom_type, const float* atom_pos, int64_t N_cap,
                               const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride, int32_t num_element,
                               int32_t num_bond_types, const int32_t* select, const int32_t* patterns, const int32_t* kind_ptr,
                               const float* bin_range, const int32_t* bin_count, int64_t* hist, int64_t* outside, int64_t* n_items,
                               void* ws, size_t ws_bytes, void* stream) {
  Local3DArgs a{};
  const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select);
  if (why) return fail(MDX_ERR_ARG, "%s", why);
  if (!atom_pos || !patterns || !kind_ptr || !bin_range || !bin_count || !hist || !outside || !n_items) return fail(MDX_ERR_ARG, "null argument");
  if (N_cap > L3_MAX_ATOMS) return fail(MDX_ERR_UNSUPPORTED, "more than 2^24 atoms in one call");
  if (int rc = local3d_prepare(&a, patterns, kind_ptr, bin_range, bin_count, num_element, num_bond_types, &why)) return fail(rc, "%s", why);
  const size_t need = local3d_ws_bytes(N_cap, Eh_stride);
  if (!ws || ws_bytes < need) return fail(MDX_ERR_ARG, "workspace too small: need %zu bytes", need);
  if (reinterpret_cast<uintptr_t>(ws) & 3) return fail(MDX_ERR_ARG, "workspace must be 4-byte aligned");
  a.B = B, a.atom_pos = atom_pos;
  a.num_element = num_element, a.num_bond_types = num_bond_types;
  a.hist = reinterpret_cast<unsigned long long*>(hist), a.outside = reinterpret_cast<unsigned long long*>(outside);
  a.n_items = reinterpret_cast<long long*>(n_items);
  a.ws_cur = reinterpret_cast<int*>(ws), a.ws_adj = a.ws_cur + std::max<int64_t>(N_cap, 1);
  launch_mol_local3d(a, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_guidance_uncertainty_grad(const float* logits, int32_t K, int64_t n, float* glogits, void* stream) {
  if (K < 1 || n < 0 || (n > 0 && (!logits || !glogits))) return fail(MDX_ERR_ARG, "bad argument");
  launch_uncertainty_grad(logits, K, (int)n, glogits, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_add_inplace(float* dst, const float* src, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!dst || !src))) return fail(MDX_ERR_ARG, "bad argument");
  launch_add_inplace(dst, src, (int)n, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}

extern "C" int mdx_noise(mdx_graph_t g, uint64_t seed, int32_t draw, int32_t Kn, int32_t Ke, float* eps_pos, float* u_node,
                         float* u_halfedge, void* stream) {
  if (!g) return fail(MDX_ERR_ARG, "null graph");
  if (Kn < 1 || Kn > 8 || Ke < 1 || Ke > 8) return fail(MDX_ERR_ARG, "class counts must be in 1..8");
  launch_philox_noise(seed, draw, g->node_graph, g->node_local, g->he_graph, g->he_local, g->mol_ids, (int)g->N,
                      (int)g->Eh, Kn, Ke, eps_pos, u_node, u_halfedge, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return MDX_OK;
}
