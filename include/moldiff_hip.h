/* moldiff_hip.h -- C ABI of libmoldiff_hip.so: the MI355X (gfx950) implementation of MolDiff's
 * denoising hot path.  Plain C: opaque handles, raw pointers, sizes; no C++/torch types.
 *
 * The reference (pengxingang/MolDiff @ 2024_08_07) has no FFI layer of its own -- its boundary is
 * the Python model API plus one third-party op -- so each entry point below names the reference
 * function (file:line) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - every function returns MDX_OK (0) or an error code; mdx_last_error() gives the message
 *     (thread-local).  No C++ exception crosses this boundary.
 *   - pointers named h_* / *_host are HOST pointers; everything else is a DEVICE pointer valid on
 *     the current HIP device.  `stream` is a hipStream_t passed as void*.
 *   - no hidden per-call device allocation: forward-type calls take a caller-owned workspace of
 *     at least mdx_workspace_bytes() bytes (256-byte aligned).  Handles own only their packed
 *     weights / graph index arrays.
 *   - edge-indexed tensors crossing this boundary use the REFERENCE edge order
 *     (edge_index = cat[halfedge_index, flip(halfedge_index)], models/model.py:269); the library
 *     re-orders internally.  float = IEEE fp32, indices = int64 like the reference's LongTensors.
 */
#ifndef MOLDIFF_HIP_H
#define MOLDIFF_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_OK 0
#define MDX_ERR_ARG 1         /* bad argument / shape */
#define MDX_ERR_HIP 2         /* HIP runtime error (no device, launch failure, OOM) */
#define MDX_ERR_STATE 3       /* missing parameters, workspace too small, call order */
#define MDX_ERR_UNSUPPORTED 4 /* configuration outside what the kernels are built for */

#define MDX_KIND_MOLDIFF 0  /* models/model.py:13-46         (embedders + denoiser + 2 decoders) */
#define MDX_KIND_BONDPRED 1 /* models/bond_predictor.py:12-37 (embedders + encoder + edge decoder) */
#define MDX_KIND_NET 2      /* a bare NodeEdgeNet, models/graph.py:298-346 */

typedef struct mdx_model_s* mdx_model_t;
typedef struct mdx_graph_s* mdx_graph_t;

typedef struct mdx_config {
  int32_t kind;           /* MDX_KIND_* */
  int32_t node_dim;       /* 256 */
  int32_t edge_dim;       /* 64  */
  int32_t num_blocks;     /* 6 (denoiser) / 8 (bond predictor encoder) */
  float cutoff;           /* distance smearing stop: 15 / 20 */
  int32_t num_gaussians;  /* 16 */
  int32_t update_pos;     /* 1 / 0 */
  int32_t time_dim;       /* 10 / 20 (ignored for MDX_KIND_NET) */
  int32_t num_timesteps;  /* 1000 */
  int32_t num_node_types; /* 8 */
  int32_t num_edge_types; /* 6 (MolDiff) / 5 (bond predictor) */
} mdx_config;

const char* mdx_last_error(void);
int mdx_version(void);
int mdx_device_count(int* count); /* 0 devices is MDX_OK with *count = 0 */

/* ---- model handle: parameters enter by state_dict key (Appendix B of SURVEY.md; the strict
 * load_state_dict contract of scripts/sample_drug3d.py:79) ---------------------------------- */
int mdx_model_create(const mdx_config* cfg, mdx_model_t* out);
int mdx_model_destroy(mdx_model_t m);
/* h_data: host fp32, row-major, `ndim` dims in `shape`.  Key prefix for MDX_KIND_NET is "" (keys as
 * inside NodeEdgeNet, e.g. "edge_embs.0.weight"), otherwise the full model key ("denoiser.edge_embs.0.weight"). */
int mdx_model_set_param(mdx_model_t m, const char* key, const float* h_data, const int64_t* shape, int32_t ndim);
/* Packs all weights into MFMA fragment order and uploads them.  Fails with MDX_ERR_STATE listing the
 * first missing key.  Must be called after the last set_param and before any forward. */
int mdx_model_finalize(mdx_model_t m);
/* Matrix path of the per-edge Linear layers (reference models/common.py:181-201, models/graph.py:29-55,133-141,268-295; the
 * reference computes them in fp32).  MDX_MATRIX_EXACT_F32 (default): fp32-input MFMA, bit-for-bit an fmaf chain.
 * MDX_MATRIX_SPLIT_F16 (opt-in): every operand split into float16 hi + lo halves (22 significand bits), three float16 MFMAs
 * per k-group with fp32 accumulation -- same parity tests, ~2x the matrix throughput.  Needs a finalized model; refused with
 * MDX_ERR_UNSUPPORTED if a weight lies outside float16's range (|w| >= 65504); a handle that is re-finalized with such weights
 * drops back to the exact path.  ACTIVATION RANGE: operands of the per-edge layers must stay below 65504 in magnitude too -- only the
 * weights can be checked at pack time.  LayerNorm outputs are bounded by their gains; the un-normalised operands are the pairwise
 * products bond_linear(b) * node_linear(n) and edge_net(e) * node_net(h[col]) (graph.py:45,139) and the raw inputs of a bare
 * NodeEdgeNet: beyond the range they become inf / NaN on this path where the exact path stays finite (NaN/inf are propagated
 * silently, like the reference does).  tests/golden/stress.npz exercises 3.7e4.  Takes effect on the next forward / step. */
#define MDX_MATRIX_EXACT_F32 0
#define MDX_MATRIX_SPLIT_F16 1
int mdx_model_set_matrix_path(mdx_model_t m, int32_t path);
int mdx_model_get_matrix_path(mdx_model_t m, int32_t* path);
/* Lower clamp of the distance smearing, GaussianSmearing(start, stop = cutoff) of models/graph.py:330-333 / common.py:233-235.
 * 0 (the default) in every shipped config; the offset / coeff tables always come from the state_dict.  Any time before a forward. */
int mdx_model_set_smear_start(mdx_model_t m, float start);

/* ---- graph handle: CSR plan of one packed batch (utils/transforms.py:125-156 produces the inputs) */
/* h_edge_index: (2,E) int64 row-major, row 0 = left/row, row 1 = right/col; h_batch_node: (N) int64,
 * non-decreasing.  h_mol_ids: (n_graphs) int64 global molecule ids for noise keying, or NULL = 0..n_graphs-1. */
int mdx_graph_create(int64_t n_nodes, int64_t n_edges, const int64_t* h_edge_index, const int64_t* h_batch_node,
                     int64_t n_graphs, const int64_t* h_mol_ids, mdx_graph_t* out);
int mdx_graph_destroy(mdx_graph_t g);
/* Host-only plan (no GPU needed; used by the CPU tests).  All outputs int32, caller-allocated:
 * left/right/int2ref/col_eids: E, row_ptr/col_ptr: N+1. */
int mdx_graph_plan_host(int64_t n_nodes, int64_t n_edges, const int64_t* h_edge_index, int32_t* left, int32_t* right,
                        int32_t* int2ref, int32_t* row_ptr, int32_t* col_ptr, int32_t* col_eids);

/* ---- test aids of the persistent kernels' work distribution (tests/test_gpu_work_plan.py).  Not for production code. */
/* Caps the compute-unit count the launchers size their grids by (edge kernels A and B, the guidance backward, linear_rows, the
 * grid heuristics of the training GEMMs and the eight fused float16 training kernels read it at launch time), so that a batch of
 * a few hundred edges loops its persistent waves the way a full batch does on the whole device.  n <= 0, or n beyond the device's
 * count, restores the device's own.  Process-wide; results never depend on it -- except that a fused training backward leaves one
 * partial row of LayerNorm-parameter gradients per workgroup (mdx_op_bondffn_workgroups, = this count): keep one cap from a backward
 * launch to the reduction of its rows. */
int mdx_debug_set_num_cus(int32_t n);
/* Centred packs of the MolDiff denoiser's edge kernels: on = 1 (the default) packs every Linear that feeds
 * a LayerNorm in edge kernels A and B with the mean over its output features taken out, on = 0 packs the weights as stored; the
 * handle is re-packed either way (synchronises the device).  The two conventions differ in rounding only.  No effect on a
 * bond-predictor or plain-network handle.  The weight arena is freed and allocated again: whatever holds device pointers into the
 * old one -- a captured graph, a live sampler of this handle -- must be re-created after the call. */
int mdx_debug_set_ln_centred(mdx_model_t model, int32_t on);
/* Host only: what finalize would upload for the handle's parameters with centred packs on (1) or off (0).  arena: *n_floats floats;
 * slots: one text line per pack, "kind offset floats F K col0 transposed centred key" (kind d dense, s stream, S split stream,
 * D split dense, v vector; key "-" where the pack is not cut from one named parameter).  With arena / slots NULL only the sizes are
 * returned; otherwise *n_floats / *n_slot_bytes are the buffers' capacities on entry.  The handle is not touched. */
int mdx_debug_pack_host(mdx_model_t model, int32_t ln_centred, float* arena, size_t* n_floats, char* slots, size_t* n_slot_bytes);
/* The centring itself, on the host alone: W (F x ldw, row-major) -> out, every column's mean over the F rows taken out in float64 and
 * rounded to float once; *worst = the largest |residual column mean| / (2^-24 max|out[:, k]|) over the columns (<= 1). */
int mdx_debug_centre_host(const float* W, int32_t F, int32_t ldw, float* out, double* worst);
/* The static plan edge kernel A's launcher makes for nunits work items on nslots persistent waves: plan[5] = nslots, nf (full
 * rounds), rem (items of the last round), split (0 none, 1, 2), m (units per BondFFN slot of a split round).  Host only. */
int mdx_debug_work_plan_host(int32_t nunits, int32_t nslots, int32_t can_split, int32_t* plan);
/* What the six row-owner launches of a batch (graph arguments as mdx_graph_create) do on a device of n_cus compute units
 * (n_cus <= 0: the count the launchers read right now, i.e. the device's or the cap).
 * launches[6][8], rows: edge kernel A exact / split build, edge kernel B exact / split, guidance backward exact / split; columns:
 * work items, grid (workgroups of four waves), workgroup pairs of the work queue, then, of those pairs under kernel A's queue (its
 * last `tail` items are cut by section): pairs whose range is shorter than the tail, equal to it, longer with one workgroup,
 * longer with two.  Host only. */
int mdx_debug_launch_units_host(int64_t n_nodes, int64_t n_edges, const int64_t* h_edge_index, const int64_t* h_batch_node,
                                int64_t n_graphs, int32_t n_cus, int32_t* launches);
/* The grid of one of the eight fused float16 training kernels (mdx_op_bondffn / edge_tail / posffn / nodemsg _fwd / _bwd) for n_rows rows
 * on a device of n_cus compute units (n_cus <= 0: the count the launchers read right now): the launchers' own arithmetic.  A wave owns
 * 16-row tiles and walks them with a stride of grid x waves.  out[6] = grid (workgroups), waves per workgroup, tiles, rounds (trips of
 * the first wave's tile loop), tiles in the last round, rows in the last tile.  Host only. */
enum {
  MDX_FUSED_BONDFFN_FWD = 0, MDX_FUSED_BONDFFN_BWD = 1, MDX_FUSED_EDGE_TAIL_FWD = 2, MDX_FUSED_EDGE_TAIL_BWD = 3,
  MDX_FUSED_POSFFN_FWD = 4, MDX_FUSED_POSFFN_BWD = 5, MDX_FUSED_NODEMSG_FWD = 6, MDX_FUSED_NODEMSG_BWD = 7, MDX_FUSED_KERNELS = 8
};
int mdx_debug_fused_grid_host(int32_t kernel, int64_t n_rows, int32_t n_cus, int32_t* out);

size_t mdx_workspace_bytes(int64_t n_nodes, int64_t n_edges);

/* ---- network (models/graph.py) ---------------------------------------------------------------- */
/* NodeEdgeNet.forward, graph.py:348-367.  node_time (N), edge_time (E, reference order) are t/T floats. */
int mdx_net_forward(mdx_model_t m, mdx_graph_t g, const float* h_node, const float* pos, const float* h_edge,
                    const float* node_time, const float* edge_time, float* h_node_out, float* pos_out,
                    float* h_edge_out, void* ws, size_t ws_bytes, void* stream);
/* NodeBlock.forward, graph.py:29-55: out (N,256) = block `i`'s node update (no residual). */
int mdx_node_block(mdx_model_t m, mdx_graph_t g, int32_t i, const float* x, const float* edge_attr,
                   const float* node_time, float* out, void* ws, size_t ws_bytes, void* stream);
/* EdgeBlock.forward, graph.py:268-295: out (E,64) reference order (no residual). */
int mdx_edge_block(mdx_model_t m, mdx_graph_t g, int32_t i, const float* h_bond, const float* h_node,
                   const float* bond_time, float* out, void* ws, size_t ws_bytes, void* stream);
/* BondFFN.forward of an EdgeBlock (models/graph.py:133-141) on its own:
 *   out[e] = inter_module((W_bl bond[e]) * (W_nl node[e])) * sigmoid(gate([bond[e] | node[e] | time[e]]))
 * side 0 = edge_blocks[i].bond_ffn_left, 1 = bond_ffn_right.  node_feat holds one ALREADY GATHERED row per edge (the
 * reference calls it with h_node[left] / h_node[right]), so `g` must be the identity graph of E nodes and E edges
 * (edge e = (e, e)); bond_feat (E,64), node_feat (E,256), time (E), out (E,64). */
int mdx_bond_ffn(mdx_model_t m, mdx_graph_t g, int32_t i, int32_t side, const float* bond_feat, const float* node_feat,
                 const float* time, float* out, void* ws, size_t ws_bytes, void* stream);
/* PosUpdate.forward, graph.py:384-396: rel (E,3), dist (E) reference order; out (N,3) = delta_pos. */
int mdx_pos_update(mdx_model_t m, mdx_graph_t g, int32_t i, const float* h_node, const float* h_edge,
                   const float* rel, const float* dist, const float* edge_time, float* out, void* ws,
                   size_t ws_bytes, void* stream);
/* torch_scatter.scatter_sum(src, index, dim=0, dim_size=N) for index = left (by_right = 0) or right
 * (by_right = 1) of the graph; src (E,C) reference order, C in {3, 64, 256}; call sites graph.py:50,279,283,394.
 * by_right | 2: src is already in the plan's internal edge order (mdx_graph_plan_host) -- the segment-sum kernel alone, without the
 * boundary permutation (what bench.py times as the scatter/gather primitive). */
int mdx_segment_sum(mdx_graph_t g, const float* src, int32_t C, int32_t by_right, float* out, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- model forward ------------------------------------------------------------------------------ */
/* MolDiff.forward, model.py:204-234.  h_node_pert (N,Kn), h_edge_pert (E,Ke) reference order (may be NULL
 * when h_halfedge_pert (Eh,Ke) is given: then both directions use it, model.py:273), t (n_graphs) int64. */
int mdx_moldiff_forward(mdx_model_t m, mdx_graph_t g, const float* h_node_pert, const float* pos_pert,
                        const float* h_edge_pert, const float* h_halfedge_pert, const int64_t* t, float* pred_node,
                        float* pred_pos, float* pred_halfedge, void* ws, size_t ws_bytes, void* stream);
/* BondPredictor.forward, bond_predictor.py:128-162: logits (Eh, num_edge_types).  `tape` (caller-owned,
 * mdx_bondpred_tape_bytes(), 256-byte aligned) records the per-block state the backward needs; NULL = inference only. */
size_t mdx_bondpred_tape_bytes(int64_t n_nodes, int64_t n_edges, int32_t num_blocks);
int mdx_bondpred_forward(mdx_model_t m, mdx_graph_t g, const float* h_node, const float* pos, const int64_t* t,
                         float* logits, void* ws, size_t ws_bytes, void* tape, size_t tape_bytes, void* stream);
/* The autograd call of the guidance block, model.py:312-325 (torch.autograd.grad(scalar(logits), pos_in)):
 * gpos (N,3) = scale * dL/dpos given glogits = dL/dlogits (Eh, num_edge_types) and the tape of the matching
 * forward (same model, graph, pos).  Hand-written data-gradient backward through all encoder blocks. */
int mdx_bondpred_backward(mdx_model_t m, mdx_graph_t g, const float* pos, const float* glogits, float scale,
                          float* gpos, void* ws, size_t ws_bytes, void* tape, size_t tape_bytes, void* stream);

/* ---- transitions (models/transition.py, models/diffusion.py) -------------------------------------- */
/* ContigousTransition.get_prev_from_recon, transition.py:44-63 (eps passed in). x (n,3). */
int mdx_pos_posterior(const float* coef_x0, const float* coef_xt, const float* std, const float* x_t,
                      const float* x_recon, const float* eps, const int64_t* t, const int64_t* batch, int64_t n,
                      float* out, void* stream);
/* The same for rows of any width C: x (n,C).  categorical_space = 'continuous' runs the atom (C = num_node_types) and bond
 * (C = num_edge_types) features through it with their own schedules, models/model.py:301-304. */
int mdx_gauss_posterior(const float* coef_x0, const float* coef_xt, const float* std, const float* x_t,
                        const float* x_recon, const float* eps, const int64_t* t, const int64_t* batch, int64_t n, int32_t C,
                        float* out, void* stream);
/* GeneralCategoricalTransition.q_v_posterior(v0_prob=True), transition.py:285-315.  in0 = log_v0, or raw
 * logits when is_logits != 0 (fuses F.log_softmax of model.py:291,297).  (n,K), K <= 8. */
int mdx_cat_posterior(const float* q_mats, const float* qT_onestep, int32_t K, int32_t T, const float* in0,
                      int32_t is_logits, const float* log_vt, const int64_t* t, const int64_t* batch, int64_t n,
                      float* out, void* stream);
/* Jump forms of the two posteriors above, for strided sampling: q(x_s | x_t, x0_hat) of the SAME forward process for any level s < t
 * (NO reference line: models/transition.py:44-63 and :285-315 know s = t - 1 only; DESIGN.md "strided sampling").  The caller builds
 * one table row per (t, s) pair it asks for (moldiff_amd/transition.py jump_coefs / jump_mats): c0 = sqrt(abar_s) (1 - a) / (1 - abar_t),
 * ct = sqrt(a) (1 - abar_s) / (1 - abar_t), sd = sqrt((1 - abar_s) (1 - a) / (1 - abar_t)) with a = abar_t / abar_s, and
 * qT_jump = (Q_{s+1} ... Q_t)^T; rows with s = t - 1 are copies of the one-step tables.  Per graph, int64: t (B) the level read and
 * row (B) the table row of the graph's pair, for both entries; t_prev (B) the level written (< 0 where t == 0: read as 0) for the
 * categorical entry only, which indexes q_mats with it -- the position entry needs nothing but its table row.  Same row arithmetic
 * as the one-step kernels; where t == 0 the output is the posterior mean / log v0_hat. */
int mdx_pos_posterior_jump(const float* jump_coef_x0, const float* jump_coef_xt, const float* jump_std, const float* x_t,
                           const float* x_recon, const float* eps, const int64_t* t, const int64_t* row, const int64_t* batch,
                           int64_t n, float* out, void* stream);
int mdx_cat_posterior_jump(const float* q_mats, const float* qT_jump, int32_t K, const float* in0, int32_t is_logits,
                           const float* log_vt, const int64_t* t, const int64_t* t_prev, const int64_t* row, const int64_t* batch,
                           int64_t n, float* out, void* stream);
/* Training / add_noise: GeneralCategoricalTransition.add_noise (models/transition.py:266-283: index_to_log_onehot, q_vt_pred, the
 * Gumbel-max draw of q_vt_sample with the uniforms u (n,K) passed in, onehot_encode) in one launch: v (n) class ids of the clean batch
 * -> onehot (n,K) of the drawn classes, log_vt = log(clamp(onehot, 1e-30)), log_v0 = log(clamp(onehot(v), 1e-30)).  log_off = log(1e-30)
 * as the caller's torch evaluates it in fp32.  Ids outside [0, K) are clamped (the caller reports them, models/diffusion.py:54). */
int mdx_op_cat_add_noise(const float* q_mats, int32_t K, int32_t T, const int64_t* v, const int64_t* t, const int64_t* batch, const float* u,
                         int64_t n, float log_off, float* onehot, float* log_vt, float* log_v0, void* stream);
/* Training: the categorical loss rows of models/model.py:170-189 and their gradient w.r.t. the decoder logits in one launch --
 * log_softmax, q_v_posterior (transition.py:285-315) of the true and the predicted classes, compute_v_Lt (transition.py:317-327:
 * KL for t > 0, decoder NLL at t == 0) and the backward torch.autograd would run through them.  logits / log_vt / log_v0 (n,K), K <= 8;
 * row_loss (n); dlogits (n,K) = d row_loss[i] / d logits[i][:] (the caller scales by 100 / n x the upstream gradient). */
int mdx_op_cat_loss(const float* q_mats, const float* qT_onestep, int32_t K, int32_t T, const float* logits, const float* log_vt,
                    const float* log_v0, const int64_t* t, const int64_t* batch, int64_t n, float* row_loss, float* dlogits,
                    void* stream);
/* log_sample_categorical, diffusion.py:79-85 (u passed in) + onehot_encode, transition.py:255. */
int mdx_gumbel_argmax(const float* logits, const float* u, int32_t K, int64_t n, int64_t* cls, float* onehot,
                      void* stream);
/* GeneralCategoricalTransition.sample_init, transition.py:331-339 (called at model.py:245-246): the prior draw.  The
 * reference's logits there are FLOAT64 (log(init_prob + 1e-30).clamp_min(-32) of a float64 numpy array), so rand_like,
 * the Gumbel transform of diffusion.py:79-85 and the argmax all run in float64; this entry point does the same.
 * logits64: K (<= 8) doubles on the HOST (one row, the reference repeats it n times); u: (n,K) uniforms on the device,
 * float64 when u_is_f64 else float32 (widened exactly); outputs (any may be NULL): cls (n) int64, onehot (n,K),
 * log_onehot (n,K) = log(onehot.clamp(min=1e-30)) with log_off = the float32 log(1e-30) of the caller's libm,
 * cls8 (n) one byte per row (compact trajectory frame). */
int mdx_prior_draw(const double* logits64, int32_t K, const void* u, int32_t u_is_f64, int64_t n, int64_t* cls,
                   float* onehot, float* log_onehot, float log_off, uint8_t* cls8, void* stream);
/* dU/dlogits of the default 'uncertainty' guidance objective U = sum_h log sigmoid(-logsumexp_k logits[h,k])
 * (model.py:322-324); glogits (n,K).  Feed to mdx_bondpred_backward with scale = -guidance_scale to get delta. */
int mdx_guidance_uncertainty_grad(const float* logits, int32_t K, int64_t n, float* glogits, void* stream);
/* dst[i] += src[i]  (pos_prev = pos_prev + delta, model.py:362). */
int mdx_add_inplace(float* dst, const float* src, int64_t n, void* stream);
/* Philox4x32-10 noise for draw index `draw` (0 = prior, i+1 = loop iteration i): eps_pos (N,3) ~ N(0,1),
 * u_node (N,Kn), u_halfedge (Eh,Ke) ~ U[0,1).  Any output may be NULL.  Replaces torch.randn_like /
 * rand_like at transition.py:60, diffusion.py:80. */
int mdx_noise(mdx_graph_t g, uint64_t seed, int32_t draw, int32_t Kn, int32_t Ke, float* eps_pos, float* u_node,
              float* u_halfedge, void* stream);

/* ---- one iteration of the reverse chain in a single call (models/model.py:272-308: denoiser forward, Gaussian
 * posterior on the positions, categorical posteriors + Gumbel-max draws on atom and bond types).  Guidance, when wanted,
 * is applied by the caller afterwards (mdx_bondpred_forward / mdx_guidance_uncertainty_grad / mdx_bondpred_backward /
 * mdx_add_inplace).  All pointers are device pointers; `cur` is read, `next` and `pred_*` are written.
 *   tables: the frozen schedule tensors of the checkpoint (pos_transition.coef_x0 / coef_xt / std (T);
 *           node/edge_transition.q_mats and transpopse_q_onestep_mats (T,K,K)).
 *   t (B) int64 must hold `step` for every molecule; batch_node (N) / batch_halfedge (Eh) int64 as in the reference.
 *   eps_pos (N,3) ~ N(0,1), u_node (N,Kn), u_halfedge (Eh,Ke) ~ U[0,1): this step's draws (mdx_noise or the caller's own). */
typedef struct {
  const float *pos_coef_x0, *pos_coef_xt, *pos_std;
  const float *node_q_mats, *node_qT_onestep;
  const float *edge_q_mats, *edge_qT_onestep;
} mdx_tables;
typedef struct {
  float *h_node, *pos, *h_halfedge;   /* (N,Kn) one-hot, (N,3), (Eh,Ke) one-hot */
  float *log_node, *log_halfedge;     /* (N,Kn), (Eh,Ke) log-probabilities of the current types */
} mdx_state;
int mdx_sample_step(mdx_model_t m, mdx_graph_t g, const mdx_tables* tables, const int64_t* t, const int64_t* batch_node,
                    const int64_t* batch_halfedge, const mdx_state* cur, const mdx_state* next, float* pred_node, float* pred_pos,
                    float* pred_halfedge, const float* eps_pos, const float* u_node, const float* u_halfedge, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- the WHOLE loop body of MolDiff.sample in one call (models/model.py:271-372): per-graph time tensor (:272), noise
 * draws (transition.py:60, diffusion.py:80), denoiser forward (:274-284), Gaussian posterior (:287-288), categorical
 * posteriors + Gumbel-max draws (:291-307) and, when `guide` is given, the bond-predictor guidance with the default
 * 'uncertainty' objective (:309-362: predictor forward at the step's INPUT state, dU/dlogits, hand-written backward
 * w.r.t. the positions, pos_prev += -scale * grad).  With guide->side_stream set, the guidance chain runs on that stream
 * concurrently with the denoiser of the same step (both only read the input state); the library orders the two streams
 * with events and `stream` ends up holding the complete result.  A C caller runs the chain with
 *     for (i = 0; i < T; ++i) { mdx_sample_step_full(..., T - 1 - i, ..., frames i and i + 1, ...); }
 *   step        : the diffusion step id (the reference's `step`), identical for every molecule of the batch
 *   noise       : draw >= 0: Philox draw index (0 = prior, i + 1 = loop iteration i), the buffers receive this step's noise
 *                 (mdx_noise with `seed`); draw < 0: the buffers already hold it (explicit noise, e.g. parity tests)
 *   t_buf       : (n_graphs) int64 device scratch that receives `step` (the reference's time_step tensor)
 *   node_cls / halfedge_cls : optional (N) / (Eh) uint8 outputs = the sampled class ids of `next` (a frame of the compact
 *                 trajectory: one byte per atom / half-edge instead of a one-hot fp32 row, models/model.py:365-367)
 *   guide       : NULL = no guidance */
typedef struct {
  mdx_model_t predictor;          /* BondPredictor handle (MDX_KIND_BONDPRED) */
  float scale;                    /* sample.guidance[1] */
  void* tape;                     /* mdx_bondpred_tape_bytes(N, E, predictor blocks), 256-byte aligned */
  size_t tape_bytes;
  void* ws2;                      /* a second workspace of mdx_workspace_bytes(N, E): the predictor's own */
  size_t ws2_bytes;
  float *logits, *glogits;        /* (Eh, Kb) scratch: predictor logits and dU/dlogits */
  float* delta;                   /* (N,3) out: the increment added to next->pos */
  void* side_stream;              /* NULL = run the guidance chain in line on `stream` */
} mdx_guidance;
typedef struct {
  uint64_t seed;
  int32_t draw;
  float *eps_pos, *u_node, *u_halfedge;   /* (N,3), (N,Kn), (Eh,Ke) */
} mdx_step_noise;
int mdx_sample_step_full(mdx_model_t m, mdx_graph_t g, const mdx_tables* tables, int32_t step, const int64_t* batch_node,
                         const int64_t* batch_halfedge, const mdx_state* cur, const mdx_state* next, float* pred_node,
                         float* pred_pos, float* pred_halfedge, const mdx_step_noise* noise, int64_t* t_buf, uint8_t* node_cls,
                         uint8_t* halfedge_cls, const mdx_guidance* guide, void* ws, size_t ws_bytes, void* stream);

/* ---- strided sampling: one iteration of a reverse chain that visits a subset tau_0 > tau_1 > ... > tau_{num-1} = 0 of the levels
 * (NO reference line: the loop of models/model.py:271-372 visits every level).  The same single call as the entry above -- Philox launch
 * that also fills the time tensor with step = tau_position, denoiser forward at that time, ONE transition launch, optional guidance in
 * line or on the side stream -- with the transition reading row `position` of the jump tables and q_mats[tau_{position+1}], i.e. drawing
 * from q(x_{tau_{position+1}} | x_{tau_position}, x0_hat).  The last position (level 0) is the ordinary t == 0 step.
 *   jump     : one row per schedule position (moldiff_amd/transition.py jump_coefs / jump_mats; rows of stride-1 pairs and the last
 *              row are copies of `tables`, so a schedule T-1, T-2, ..., 0 reproduces the loop above bit for bit); `levels` is a HOST array
 *   step     : must equal levels[position]
 *   noise    : the draw index of the move leaving level t is T - t under every schedule (what the full chain uses there); a scaffold
 *              merge after it uses T + (T - t), with level = levels[position + 1], or -1 after the last position
 * A C caller: for (j = 0; j < num; ++j) the call with position j, step levels[j], frames j and j + 1. */
typedef struct {
  const float *pos_coef_x0, *pos_coef_xt, *pos_std;   /* (num) device */
  const float *node_qT_jump, *edge_qT_jump;           /* (num,Kn,Kn) / (num,Ke,Ke) device: (Q_{s+1} ... Q_t)^T, row-major */
  const int32_t* levels;                              /* (num) host: the schedule, strictly decreasing, ends at 0 */
  int32_t num;
} mdx_jump_tables;
int mdx_sample_jump_full(mdx_model_t m, mdx_graph_t g, const mdx_tables* tables, const mdx_jump_tables* jump, int32_t position,
                         int32_t step, const int64_t* batch_node, const int64_t* batch_halfedge, const mdx_state* cur,
                         const mdx_state* next, float* pred_node, float* pred_pos, float* pred_halfedge, const mdx_step_noise* noise,
                         int64_t* t_buf, uint8_t* node_cls, uint8_t* halfedge_cls, const mdx_guidance* guide, void* ws,
                         size_t ws_bytes, void* stream);

/* ---- scaffold-constrained sampling (replacement conditioning; NO reference line: the reference has no conditional sampling).
 * Overwrites the FIXED rows of the state `next` with a draw from q(x_level | x_0) of a known molecule, in one launch and without
 * a host synchronisation; free rows are neither read nor written.  A conditioned chain calls it after every
 * mdx_sample_step_full (and after the caller's guidance) with level = step - 1, and once on the prior draw with level = T - 1.
 *   level >= 0  : pos = sqrt(alphas_bar[level]) x0 + sqrt(1 - alphas_bar[level]) eps in fp32 (ContigousTransition.add_noise,
 *                 models/transition.py:28-37); class = the Gumbel-max draw of GeneralCategoricalTransition.add_noise
 *                 (transition.py:245-283) at t = level with the row's uniforms -- the row function of mdx_op_cat_add_noise.  A fixed
 *                 row receives its one-hot row, its log row log(clamp(onehot, 1e-30)) (log_off as for mdx_prior_draw), its uint8
 *                 class id (node_cls / halfedge_cls, optional) and its position.
 *   level == -1 : the end of the chain: fixed rows receive x0 bit for bit and onehot(v0), and the fixed rows of pred_node / pred_pos /
 *                 pred_halfedge (optional; ignored for level >= 0) the log-one-hot row of v0 and x0, so that mdx_decode_output returns
 *                 the known atoms and bonds as given, with confidence 1.
 *   scaffold    : node_mask (N) / halfedge_mask (Eh) bytes, non-zero = fixed, NULL = every row; node_type (N) / halfedge_type (Eh)
 *                 int64 class ids in [0, K) (checked by the caller; clamped here); node_pos (N,3).  Values on free rows are not read.
 *   noise       : draw >= 0: the buffers are filled with Philox draw `draw` first (mdx_noise with `seed`; one more launch) -- the
 *                 chain's own draws are 0..T, a conditioned chain uses T + 1 + i after loop iteration i and 2T + 1 for the initial
 *                 state; draw < 0: the buffers already hold the noise.  Not read at level -1. */
typedef struct {
  const float* alphas_bar;                 /* pos_transition.alphas_bar (T) */
  const float *node_q_mats, *edge_q_mats;  /* node / edge_transition.q_mats (T,Kn,Kn) / (T,Ke,Ke) */
  int32_t Kn, Ke, T;                       /* class counts in 2..8 */
} mdx_scaffold_tables;
typedef struct {
  const uint8_t *node_mask, *halfedge_mask;
  const int64_t *node_type, *halfedge_type;
  const float* node_pos;
} mdx_scaffold;
int mdx_scaffold_merge(mdx_graph_t g, const mdx_scaffold_tables* tables, int32_t level, const mdx_scaffold* scaffold,
                       const mdx_step_noise* noise, const mdx_state* next, float log_off, uint8_t* node_cls, uint8_t* halfedge_cls,
                       float* pred_node, float* pred_pos, float* pred_halfedge, void* stream);

/* ---- resampling (RePaint's loop around replacement conditioning; NO reference line: the reference's chain only walks down).
 * Moves EVERY row of a sampler state UP from level s to level t > s, i.e. draws x_t ~ q(x_t | x_s) of the forward process, in one launch
 * and without a host synchronisation.  A resampling chain calls it between two walks down the same block of levels
 * (moldiff_amd/schedule.py resampling_path); fixed rows of a scaffold move too -- their x_s is a draw of q(x_s | x_0), pushed forward it
 * is a draw of q(x_t | x_0), and the merge after the next step overwrites them anyway -- so the call is valid without a scaffold.
 *   tables  : one row per (s, t) pair the caller asks for, with a = abar_t / abar_s: pos_coef_a = sqrt(a), pos_coef_s = sqrt(1 - a)
 *             (ContigousTransition.forward_coefs: float64, rounded once); node / edge_qT_jump = (Q_{s+1} ... Q_t)^T, the SAME tables as
 *             the node / edge_qT_jump of strided sampling, jump_mats(t, s): column x_s of the stored matrix is q(x_t | x_s)
 *   row     : the pair's table row
 *   reads   : node_cls_cur (N) / halfedge_cls_cur (Eh) uint8 class ids of the current state (a frame of the compact trajectory; ids >= K
 *             are clamped) and pos_cur (N,3)
 *   position: x_t = pos_coef_a x_s + pos_coef_s eps in fp32, two products and one sum, each rounded once (no contraction)
 *   class   : Gumbel-max over log(Q_{t|s}[x_s, k] + 1e-30).clamp_min(-32) with the row's K uniforms -- the row function of
 *             mdx_op_cat_add_noise (GeneralCategoricalTransition.add_noise, transition.py:245-283) with the jump matrix in place of the
 *             cumulative one, so a forward jump from a one-hot x_s and training's add_noise are one arithmetic
 *   writes  : for every row of `next` its one-hot row, its log row log(clamp(onehot, 1e-30)) (log_off as for mdx_prior_draw), its
 *             position and (optional) its uint8 class id node_cls / halfedge_cls.  `next` must not overlap the buffers read.
 *   noise   : as for mdx_scaffold_merge (draw >= 0: one Philox launch first); a resampling chain uses draw 2T + 2 + t for the move that
 *             ARRIVES at level t, plus k (3T + 2) in the k-th walk of a block (moldiff_amd/schedule.py draw_index).
 * Row-local: a row's result depends on that row's inputs and noise only, hence not on how a batch is sharded.  Class counts in 2..8. */
typedef struct {
  const float *pos_coef_a, *pos_coef_s;               /* (num) device */
  const float *node_qT_jump, *edge_qT_jump;           /* (num,Kn,Kn) / (num,Ke,Ke) device, row-major */
  int32_t Kn, Ke, num;
} mdx_forward_tables;
int mdx_forward_jump(mdx_graph_t g, const mdx_forward_tables* tables, int32_t row, const uint8_t* node_cls_cur,
                     const uint8_t* halfedge_cls_cur, const float* pos_cur, const mdx_step_noise* noise, const mdx_state* next,
                     float log_off, uint8_t* node_cls, uint8_t* halfedge_cls, void* stream);

/* ---- harness consumer of the path's outputs (next-row) ---------------------------------------
 * seperate_outputs (utils/sample.py:4-30) + FeaturizeMol.decode_output (utils/transforms.py:65-122) on the device:
 * arg-max class + soft-max confidence per atom / half-edge, mask-type atoms (class >= num_element) dropped and the
 * survivors re-indexed per molecule, bonds = half-edges with 0 < class <= num_bond_types whose atoms survived.
 * Outputs are compacted IN PLACE at each molecule's original offsets (atoms at node offset, bonds at half-edge
 * offset; order preserved): atom_type/atom_prob (N), atom_pos (N,3), n_atoms (n_graphs); bond_type/bond_prob (Eh),
 * bond_index (2,Eh) molecule-local new atom indices, n_bonds (n_graphs).  One direction per bond (the reference
 * mirrors them on the host). */
int mdx_decode_output(mdx_graph_t g, const float* pred_node, int32_t Kn, const float* pred_pos, const float* pred_halfedge,
                      int32_t Ke, int32_t num_element, int32_t num_bond_types, int32_t* atom_type, float* atom_prob,
                      float* atom_pos, int32_t* n_atoms, int32_t* bond_type, float* bond_prob, int32_t* bond_index,
                      int32_t* n_bonds, void* ws, size_t ws_bytes, void* stream);

/* ---- quality check of the decoded molecules -------------------------------------------------------------------
 * Stands in, as far as that goes without RDKit, for the reference's test of a finished molecule (scripts/sample_drug3d.py:141-153:
 * the molecule sanitises and its SMILES has no '.') and for the valence half of Chem.SanitizeMol (utils/reconstruct.py:245-271).
 * Reads the compact arrays mdx_decode_output wrote (same graph handle), one workgroup per molecule, and writes
 *   per compact atom : component (N) = molecule-local index of the smallest atom of the atom's fragment; valence2 (N) = TWICE the
 *                      bond-order sum (types 1, 2, 3 count 2, 4, 6; the last type num_bond_types, aromatic, counts 3) -- integers;
 *   per molecule     : n_components (0 without atoms), largest_size, largest_label (component value of the largest fragment, ties
 *                      to the smaller label, -1 without atoms), n_overvalent = atoms with valence2 / 2 (integer division: half
 *                      bonds round down) > max_valence[atom_type], min_dist = shortest distance over ALL pairs of distinct atoms
 *                      (+inf below two atoms), max_bond_len (0 without bonds); distances are sqrt(dx*dx + dy*dy + dz*dz) in fp32.
 * max_valence: num_element int32 on the device, supplied by the caller (chemistry is data).  Results do not depend on the order
 * atomic updates land in, nor on a molecule's place in the batch.
 * What it does NOT do: no kekulisation, no aromaticity perception, no formal charges, no hydrogens, no bond-length rule.  A clean
 * molecule here is one RDKit's valence check cannot refuse for the explicit valences above -- a NECESSARY condition of the
 * reference's sanitisation, not a restatement: a molecule the reference fails on kekulisation passes here.
 * ws: at least 12 * max(N, 1) bytes (any mdx_workspace_bytes() workspace is enough); too small is MDX_ERR_ARG. */
int mdx_mol_check(mdx_graph_t g, const int32_t* atom_type, const float* atom_pos, const int32_t* n_atoms, const int32_t* bond_type,
                  const int32_t* bond_index, const int32_t* n_bonds, int32_t num_element, int32_t num_bond_types,
                  const int32_t* max_valence, int32_t* component, int32_t* valence2, int32_t* n_components, int32_t* largest_size,
                  int32_t* largest_label, int32_t* n_overvalent, float* min_dist, float* max_bond_len, void* ws, size_t ws_bytes,
                  void* stream);
/* Restricts every molecule m with select[m] != 0 (select, label: n_graphs int32, device) to the atoms whose `component` (from
 * mdx_mol_check) equals label[m]; the others are untouched.  Rewrites the compact arrays IN PLACE -- atom_type / atom_prob /
 * atom_pos / n_atoms and bond_type / bond_prob / bond_index / n_bonds -- with order preserved and bonds re-indexed; label -1
 * empties the molecule.  This is what "keep the largest fragment" pipelines do after the reference's '.' test
 * (scripts/sample_drug3d.py:141-153); the reference itself discards such molecules.  It does NOT re-run the check (`component`
 * and `valence2` keep describing the molecule as decoded; a kept atom's valence is unchanged, its bonds all lie in its fragment)
 * and does not choose the fragment: the caller forms `select` and `label`.  ws as for mdx_mol_check. */
int mdx_mol_keep_component(mdx_graph_t g, const int32_t* select, const int32_t* label, const int32_t* component, int32_t* atom_type,
                           float* atom_prob, float* atom_pos, int32_t* n_atoms, int32_t* bond_type, float* bond_prob,
                           int32_t* bond_index, int32_t* n_bonds, void* ws, size_t ws_bytes, void* stream);

/* ---- local 3D geometry statistics of decoded molecules ------------------------------------------------------------
 * Bond lengths, bond angles and dihedral angles histogrammed per bond pattern -- what the reference's Local3D
 * (utils/evaluation.py:156-329) collects per SMARTS such as c:c, [#6]-[#7]-[#6] or c:c:c:c -- without RDKit and of the molecule AS
 * DECODED (the reference measures RDKit's reconstruction).  One workgroup per molecule over compact arrays: molecule m has its atoms
 * at atom_ptr[m] .. + n_atoms[m] of atom_type (class index) / atom_pos, and its bonds at bond_ptr[m] .. + n_bonds[m] of bond_type
 * (1 .. num_bond_types) / bond_index (row 0 at bond_index, row 1 at bond_index + Eh_stride; molecule-local atom indices, one
 * direction per bond).  The four per-molecule arrays are device int32, so the entry serves mdx_decode_output's layout (molecules at
 * their original offsets: atom_ptr / bond_ptr = the batch's node / half-edge offsets) and a densely packed list alike.  N_cap and
 * Eh_stride are the extents of the atom and bond arrays; a molecule reaching past them is skipped.  A bond whose index lies outside
 * its molecule, or with i = j, is ignored.
 * Items: length = a bond; angle = a centre with two bonds to neighbours a < c; dihedral = a path a-b-c-d along three bonds with four
 *   distinct atoms.  A path and its reverse are ONE item, counted once (RDKit's uniquified match of a linear pattern).
 * Patterns (HOST): P rows of 7 int32 (e0, b01, e1, b12, e2, b23, e3), class indices and bond type ids; kind_ptr[4] (host) = rows of
 *   lengths | angles | dihedrals; a length row uses 3 fields, an angle row 5.  An item belongs to the row whose chain equals the
 *   item's chain or its reverse; no wildcards, so at most one row.  Rows are canonicalised here; two rows that are equal or each
 *   other's reverse are MDX_ERR_ARG, more than 64 rows of one kind MDX_ERR_UNSUPPORTED.
 * Values, fp32, every operation rounded on its own (no contraction), from coordinate differences:
 *   length |i - j|; angle at b atan2f(|u x v|, u.v) * 180/pi with u = a - b, v = c - b; dihedral atan2f((n1 x n2).b2 / |b2|, n1.n2)
 *   * 180/pi with b1 = b - a, b2 = c - b, b3 = d - c, n1 = b1 x b2, n2 = b2 x b3: IUPAC sign, in [-180, 180]; a = (1,0,0),
 *   b = (0,0,0), c = (0,0,1), d = (0,1,1) gives +90.  Coincident or collinear atoms give whatever atan2f gives.
 * Bins (HOST): bin_range = 3 x (lo, hi), bin_count = 3 x n, for lengths, angles, dihedrals.  Bin k holds lo + k w <= v < lo + (k+1) w,
 *   w = (hi - lo) / n, the last bin includes hi (numpy.histogram's rule).  Which side a value within fp32 rounding of an edge falls
 *   on is NOT specified.  A value outside [lo, hi], NaN included, adds 1 to outside[row] and nothing to hist.
 * Outputs (device int64): hist = for each kind in turn (rows of the kind) x n_kind bins, and outside (P), are ADDED TO, so calls
 *   over consecutive batches accumulate; n_items (3, B) is written: every enumerated item of the kind in molecule m, matched or not.
 *   select (B int32, device, or NULL): a molecule with select[m] == 0 contributes nothing and its n_items are 0.
 *   All results are integer counts: bit-reproducible and independent of a molecule's place in the batch.
 * Storage: a molecule of at most 512 atoms and 2,048 bonds keeps its neighbour lists in LDS, a larger one in ws.  Histograms of at
 *   most 8,192 bins in all are counted per workgroup in LDS and flushed with one atomic add per non-zero bin; larger ones are added
 *   to in global memory item by item.
 * ws: mdx_mol_local3d_ws_bytes(N_cap, Eh_stride) = 4 * (max(N_cap, 1) + 2 * max(Eh_stride, 1)) bytes; smaller is MDX_ERR_ARG.
 * MDX_ERR_ARG, outputs untouched: a null operand (select excepted), B < 0, n <= 0, hi <= lo, a pattern field out of range,
 * num_element > 255, num_bond_types > 254.  MDX_ERR_UNSUPPORTED: N_cap > 2^24. */
size_t mdx_mol_local3d_ws_bytes(int64_t N_cap, int64_t Eh_stride);
int mdx_mol_local3d(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                    const int32_t* atom_type, const float* atom_pos, int64_t N_cap, const int32_t* bond_type,
                    const int32_t* bond_index, int64_t Eh_stride, int32_t num_element, int32_t num_bond_types, const int32_t* select,
                    const int32_t* patterns, const int32_t* kind_ptr, const float* bin_range, const int32_t* bin_count, int64_t* hist,
                    int64_t* outside, int64_t* n_items, void* ws, size_t ws_bytes, void* stream);

/* ---- set-level similarity of decoded molecules: fingerprint, key, Tanimoto -----------------------------------------
 * What the reference's `similarity` block (scripts/evaluate_all.py:164-174, utils/scoring_func.py:102-223) computes from RDKit
 * fingerprints and canonical SMILES -- uniqueness, diversity, similarity to and novelty against a reference set -- needs, per
 * molecule, a bit vector and an identity.  Both are defined HERE, by this project: the fingerprint is NOT Chem.RDKFingerprint and the
 * key is NOT a canonical SMILES, and the molecule is the one AS DECODED.  All arithmetic below is unsigned 32-bit and wrapping.
 *
 * mdx_mol_fingerprint: one workgroup per molecule over the compact layout of mdx_mol_local3d -- molecule m has its atoms at
 * atom_ptr[m] .. + n_atoms[m] of atom_type and its bonds at bond_ptr[m] .. + n_bonds[m] of bond_type / bond_index (row 0 at
 * bond_index, row 1 at bond_index + Eh_stride; molecule-local atom indices, one direction per bond); the four per-molecule arrays
 * are device int32, so mdx_decode_output's arrays and a densely packed list are served alike.  N_cap and Eh_stride are the extents
 * of the atom and bond arrays.  A bond whose index lies outside its molecule, or with i = j, is ignored.  atom_type (class index)
 * and bond_type (1 .. num_bond_types) enter as the unsigned values they are: the entry knows no featuriser.
 *   mix(h)     = murmur3's fmix32: h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16.
 *   round 0    : id_0[a] = mix(class[a] + 1 + 0x9e3779b9 * (deg[a] + 1)), deg[a] = the number of valid bonds at a.
 *   round r + 1: id_{r+1}[a] = mix(id_r[a] * 0x01000193 + (r + 1) + SUM over the valid bonds (a, b, t) of mix(id_r[b] + 0x9e3779b9 * t)).
 *                The neighbour term is a plain wrapping sum: independent of the order of bonds and atoms.
 *   bits       : for r = 0 .. radius and every atom, bit (id_r[a] mod nbits) of the row is set; bit k is bit k % 32 of word k / 32.
 *                No duplicate-substructure removal as in ECFP.  nbits: a multiple of 32, 32 .. 32768; row m of `bits` holds
 *                nbits / 32 words; n_on[m] = the row's popcount.
 *   key        : the rounds continue to key_rounds (radius <= key_rounds <= 64);
 *                key_lo = SUM over r <= key_rounds and a of mix(id_r[a] + r), key_hi = the same sum of mix(id_r[a] ^ 0x5bd1e995);
 *                key[m] = key_hi << 32 | key_lo as one int64.  An isomorphism INVARIANT: relabelled copies of a molecule always
 *                agree; two different molecules can agree, because colour refinement cannot tell them apart or by a hash collision.
 *                The number of distinct keys is a lower bound of the number of distinct molecules, not a proof of identity.
 *   A molecule without atoms has a zero row, n_on 0 and key 0.  So has one with select[m] == 0 (select: B int32, device, or NULL) and
 *   one reaching past N_cap / Eh_stride.  Results do not depend on a molecule's place in the batch nor on the order atomics land in.
 * Storage: a molecule of at most 1,024 atoms keeps its two id arrays in LDS (8 KB, with 4 KB of bits: 8 resident workgroups, the
 *   most a CU's 32 waves allow, take 96 of its 160 KB); a larger one keeps them in ws.
 * ws: mdx_mol_fingerprint_ws_bytes(N_cap) = 8 * max(N_cap, 1) bytes, 4-byte aligned; smaller is MDX_ERR_ARG.
 * MDX_ERR_ARG, outputs untouched: a null operand (select excepted), a negative size, nbits or the rounds outside the above. */
size_t mdx_mol_fingerprint_ws_bytes(int64_t N_cap);
int mdx_mol_fingerprint(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                        const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index,
                        int64_t Eh_stride, const int32_t* select, int32_t radius, int32_t key_rounds, int32_t nbits, int32_t* bits,
                        int32_t* n_on, int64_t* key, void* ws, size_t ws_bytes, void* stream);
/* mdx_fp_tanimoto: every row of set A (Na rows) against every row of set B (Nb rows); a row is nbits / 32 words, n_on_a / n_on_b
 * (device int32) are the rows' popcounts as mdx_mol_fingerprint writes them.  For a pair: c = popcount(a & b), u = n_on_a + n_on_b - c,
 * q = (float)c / (float)u, ONE correctly rounded fp32 division, and q = 0 where u <= 0 (two empty rows: this project's choice).
 * With exclude_diagonal != 0 (legal for Na == Nb only: a set against itself) the pair i == j is left out.  Per row i of A:
 *   row_max[i]    fp32: the largest q (0 without a partner);
 *   row_argmax[i] int32: the SMALLEST j attaining it, -1 without a partner (Nb = 0, or Nb = 1 with the diagonal excluded);
 *   row_sum[i]    int64: SUM over j of q * 2^40.  Every non-zero q is >= 2^-16 (c >= 1, u <= 2 * 32768), so its fp32 ulp is >= 2^-39
 *                 and q * 2^40 is an exact integer below 2^41; the sum stays below 2^63 for Nb <= 2^22.  An integer sum is exact,
 *                 bit-reproducible and independent of tiling and arrival order; form means from it on the host in float64.
 * Every Na, Nb >= 0 is served.  ws: mdx_fp_tanimoto_ws_bytes(Na) = 8 * max(Na, 1) bytes, 8-byte aligned.
 * MDX_ERR_ARG, outputs untouched: nbits not a multiple of 32 in 32 .. 32768, exclude_diagonal with Na != Nb, a negative size, a
 * null operand of a non-empty set, a workspace too small.  MDX_ERR_UNSUPPORTED: Nb > 2^22, Na > 2^30. */
size_t mdx_fp_tanimoto_ws_bytes(int64_t Na);
int mdx_fp_tanimoto(const int32_t* bits_a, const int32_t* n_on_a, int64_t Na, const int32_t* bits_b, const int32_t* n_on_b, int64_t Nb,
                    int32_t nbits, int32_t exclude_diagonal, float* row_max, int32_t* row_argmax, int64_t* row_sum, void* ws,
                    size_t ws_bytes, void* stream);

/* ---- ring perception and composition counts of decoded molecules ------------------------------------------------------
 * The pure graph quantities of the reference's evaluation (utils/evaluation.py:24-37, 52-83: `count_prop`'s n_rings and n_rotatable,
 * `frags_counts`' element, bond type and ring-size counts, `ring_topo`'s ring atoms) without RDKit, of the molecule AS DECODED.  Every
 * output is defined so that its value is UNIQUE: no tie-break, atom order or traversal order enters, and a plain restatement
 * (moldiff_amd/rings.py: rings_ref) must agree exactly.
 *
 * mdx_mol_rings: one workgroup per molecule over the compact layout of mdx_mol_fingerprint (atom_ptr, bond_ptr, n_atoms, n_bonds,
 * atom_type, N_cap, bond_type, bond_index, Eh_stride, select: as there).  A bond whose index lies outside its molecule, or with
 * i = j, is ignored.  Two bonds between the same pair of atoms are a PRECONDITION VIOLATION (mdx_decode_output cannot produce them):
 * the results of such a molecule are unspecified, the kernel stays in bounds and ends.  With n atoms, b valid bonds, c fragments:
 *   n_rings[m]      = b - n + c, the cyclomatic number.
 *   ring_hist[m][k] , k = 0 .. ring_bins - 1 (1 .. 64; 7 = sizes 3 .. 9+ as the reference): the rings of size 3 + k of a MINIMUM CYCLE
 *                     BASIS, the last bin also every larger ring.  Such a basis is not unique, the sorted list of its ring sizes is:
 *                     the number of basis rings of size <= L is the GF(2) rank of all cycles of length <= L, and that is the
 *                     definition.  SUM over k of ring_hist[m][k] = n_rings[m].  This is NOT RDKit's symmetrised SSSR
 *                     (GetSymmSSSR): cubane has 5 four-rings here and 6 there.
 *   bond_ring_min   per bond slot (Eh_stride): the size of the smallest ring through the bond = 1 + the distance between its ends with
 *                     the bond removed; 0 for a bridge and for an ignored bond.  A bond is a RING BOND iff this is not 0.
 *   atom_ring_min   per atom slot (N_cap): the smallest bond_ring_min > 0 over the atom's bonds, 0 for an atom without a ring bond.
 *   n_ring_bonds[m] , n_ring_atoms[m]: the bonds / atoms with a non-zero entry.
 *   n_rotatable[m]  this project's rule, not RDKit's SMARTS: the valid bonds of type 1 that are no ring bond, both of whose atoms have
 *                     at least two valid bonds and neither of whose atoms carries a bond of type 3.  There is NO amide exclusion.
 *   elem_count[m][k], k < num_element: the atoms of class k; bond_count[m][t - 1], t = 1 .. num_bond_types: the valid bonds of type t.
 *                     An atom or bond of another class / type is counted in neither (the bond is still a bond of the graph).
 *   status[m]       0 measured; 1 too large: n_atoms > 256 or n_bonds > 512 (ignored bonds included); 2 too many rings: n_rings > 64.
 *                     With a non-zero status every other output of the molecule is 0, its slots of bond_ring_min / atom_ring_min
 *                     included.  A molecule with select[m] == 0 has status 0 and all outputs 0; so has one reaching past N_cap /
 *                     Eh_stride, whose slots are not written.  Slots of the two arrays that belong to no molecule are not written.
 * The number of basis rings an atom lies in and ring SMILES are not offered: both depend on the basis chosen.
 * Caps: 256 atoms, 512 bonds, 64 independent rings per molecule (GEOM-Drugs stays far below), so that a cycle is one 64-bit word and
 * everything fits in LDS: 23.6 KB per workgroup of 256 threads -- 6 workgroups per CU by LDS, 8 by waves.  There is no workspace.
 * All outputs are device int32, written with plain stores by the molecule's own workgroup: bit-reproducible and independent of a
 * molecule's place in the batch.
 * MDX_ERR_ARG, outputs untouched: a null operand (select excepted), a negative size, ring_bins outside 1 .. 64, num_element outside
 * 1 .. 255, num_bond_types outside 1 .. 254. */
int mdx_mol_rings(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                  const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                  const int32_t* select, int32_t num_element, int32_t num_bond_types, int32_t ring_bins, int32_t* n_rings,
                  int32_t* ring_hist, int32_t* n_ring_atoms, int32_t* n_ring_bonds, int32_t* n_rotatable, int32_t* elem_count,
                  int32_t* bond_count, int32_t* status, int32_t* bond_ring_min, int32_t* atom_ring_min, void* stream);

/* ---- substructure matching on decoded molecules: functional-group counts ----------------------------------------------
 * "Does this small labelled subgraph occur in the molecule, how often, and at which atoms" -- the primitive behind the reference's
 * `groups_counts` (utils/evaluation.py:86-94), the donor / acceptor counts of `count_prop` (:27-28), the PAINS filter
 * (utils/scoring_func.py:28-35) and the SMARTS counts of Local3D.get_counts (:308-313) -- without RDKit, of the molecule AS DECODED.
 * The pattern language is THIS PROJECT'S OWN: it is NOT SMARTS (no negation, no recursion, no charges, implicit hydrogens from a
 * caller-supplied table) and a pattern set written in it is not RDKit's `Fragments`.  Every output is defined so that its value is
 * UNIQUE -- no atom order, bond order or traversal order enters -- and a plain restatement (moldiff_amd/groups.py: groups_ref) must
 * agree exactly.
 *
 * The molecule: atoms of class atom_type[a]; its VALID bonds (both indices inside the molecule, i != j; the others are ignored).  A
 *   bond type outside 1 .. num_bond_types leaves the bond in the graph, adds no valence and satisfies no pattern bond.  Per atom:
 *   deg = its valid bonds; valence2 = mdx_mol_check's: types 1, 2, 3 count 2, 4, 6 and the last type (aromatic) counts 3;
 *   h = max(0, normal_valence[class] - (valence2 + 1) / 2) in integer division, the IMPLICIT HYDROGENS (normal_valence: num_element
 *   int32 on the HOST, 0 .. 64 each: chemistry is data); ring class of an atom / a bond from atom_ring_min / bond_ring_min of
 *   mdx_mol_rings: 0 no ring bond, 1 .. 5 smallest ring 3 .. 7, 6 a ring of 8 or more.  Two bonds between one pair of atoms are a
 *   PRECONDITION VIOLATION as for mdx_mol_rings: results unspecified, the kernel stays in bounds and ends.
 * A pattern: a connected graph of 1 .. MDX_GROUPS_ATOMS atoms and 0 .. MDX_GROUPS_BONDS bonds, no two bonds between one pair of atoms.
 *   Pattern atom: elem_mask (bit c allows class c, so num_element <= 32), deg_mask (bit d allows d bonds, bit 7: 7 or more), h_mask
 *   (bit h allows h implicit hydrogens, bit 4: 4 or more), rsize_mask (bit r allows ring class r; 0x7f = any), arom (0 any, 1 the atom
 *   carries a bond of the last type, 2 it carries none).  Pattern bond (i, j): type_mask (bit t allows bond type t, 1 .. num_bond_types
 *   <= 16), rsize_mask over the bond's ring class.  All constraints of an atom / a bond must hold.  No negation, no recursion.
 *   ORDER: every pattern atom k > 0 has a bond to an atom before it (a set that is not ordered so is refused); the earliest such atom
 *   is k's PARENT.  Pattern atom 0 is the ANCHOR.
 * Pattern table (HOST int32): P records of MDX_GROUPS_RECORD = 90 values, P in 1 .. MDX_GROUPS_PATTERNS:
 *   [0] atoms, [1] bonds, [2 + 5 k ..] elem_mask, deg_mask, h_mask, rsize_mask, arom of atom k (8 slots), [42 + 4 e ..] i, j,
 *   type_mask, rsize_mask of bond e (12 slots).  Slots beyond the counts are not read.  The table and normal_valence are validated,
 *   translated and sent to `ws` as kernel arguments of this call: the caller may overwrite both arrays as soon as the call returns.
 * An EMBEDDING is an injective map of pattern atoms to molecule atoms under which every pattern atom's constraints hold and every
 *   pattern bond lands on a valid molecule bond that satisfies the bond's constraints.  Matching is NON-INDUCED: further molecule
 *   bonds among the images are allowed.
 * Outputs (device int32; [m][p] = element m * P + p):
 *   n_embed[m][p]    the number of embeddings.  On the host n_match = n_embed / |Aut(pattern)|, Aut = the permutations of the pattern's
 *                    atoms that preserve bonds and every constraint field exactly; Aut acts freely on embeddings, so the division is
 *                    exact.  n_match equals RDKit's uniquified match count except where one atom set carries several inequivalent
 *                    embeddings: a 3-atom path in a triangle gives 3 here and 1 there.
 *   n_anchor[m][p]   the distinct molecule atoms that are the image of pattern atom 0 in at least one embedding.
 *   atom_hit         per atom slot (N_cap): bit p is set iff the atom is such an anchor for pattern p.
 *   steps[m][p]      the candidates tested = SUM over the start atoms a of steps_a; steps_a = 1 (the start candidate) + SUM over
 *                    k = 1 .. atoms - 1 and over every PARTIAL EMBEDDING of pattern atoms 0 .. k - 1 with atom 0 at a (all constraints
 *                    among them hold) of deg(image of k's parent).  Order-independent by construction.
 *   pat_status[m][p] 0 measured; 3 budget exceeded: some start atom's steps_a > max_steps (1 .. 2^20).  Then n_embed, n_anchor and
 *                    steps are 0 and bit p is clear in the molecule's atom_hit.  The budget is what lets a wildcard pattern meet
 *                    the nearly complete bond graphs of untrained weights: a thread stops after max_steps candidates.
 *   status[m]        0 measured; 1 too large: n_atoms > 256 or n_bonds > 512, the caps of mdx_mol_rings; 2 the ring data say "not
 *                    measured": ring_status[m] != 0.  With a non-zero status every other output of the molecule is 0, its atom_hit
 *                    slots included.  select, and a molecule reaching past N_cap / Eh_stride, as for mdx_mol_rings: status 0, all
 *                    outputs 0 (the slots of the latter are not written).  Slots of atom_hit that belong to no molecule are not written.
 * Ring inputs: atom_ring_min (N_cap), bond_ring_min (Eh_stride), ring_status (B), exactly as mdx_mol_rings wrote them for the same
 *   arrays; all three or none.  None is legal iff every rsize_mask of the set is 0x7f.
 * One workgroup of 256 threads per molecule, the molecule staged once in LDS (about 13 KB: 8 workgroups per CU, the bound of its
 * waves), the patterns looped over inside; thread a searches from start atom a.  All outputs are written with plain stores by the
 * molecule's own workgroup: bit-reproducible and independent of a molecule's place in the batch.
 * ws: device, mdx_mol_groups_ws_bytes(P) = 128 * (1 + P) bytes, 4-byte aligned; written by this call, read by its kernel.
 * MDX_ERR_ARG, every output untouched: a null operand (select and the ring inputs excepted), a negative size, P outside 1 .. 32,
 * max_steps outside 1 .. 2^20, num_element outside 1 .. 32, num_bond_types outside 1 .. 16, a normal valence outside 0 .. 64, a
 * pattern field out of range, an empty or out-of-range mask, a repeated or self bond, atoms not ordered as above (which covers a
 * pattern that is not connected), one or two of the three ring inputs, a ring constraint without them, a workspace too small.
 * B = 0 is accepted and writes nothing. */
#define MDX_GROUPS_ATOMS 8
#define MDX_GROUPS_BONDS 12
#define MDX_GROUPS_PATTERNS 32
#define MDX_GROUPS_RECORD 90
size_t mdx_mol_groups_ws_bytes(int32_t P);
int mdx_mol_groups(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                   const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                   const int32_t* select, int32_t num_element, int32_t num_bond_types, const int32_t* normal_valence,
                   const int32_t* patterns, int32_t P, int32_t max_steps, const int32_t* atom_ring_min, const int32_t* bond_ring_min,
                   const int32_t* ring_status, int32_t* n_embed, int32_t* n_anchor, int32_t* steps, int32_t* pat_status,
                   int32_t* status, int32_t* atom_hit, void* ws, size_t ws_bytes, void* stream);

/* ---- Kekulé assignment of the aromatic bonds of decoded molecules ---------------------------------------------------------
 * The reference hands its decoded bond graph, aromatic bonds included, to RDKit's sanitisation (utils/reconstruct.py:245-271) and
 * counts a molecule as generated only if that succeeds; it fails when an atom is above its valence (mdx_mol_check) or when the
 * aromatic system has no Kekulé structure, and `fix_valence` / `fix_aromatic` (:295-387) retry with a hydrogen or a positive charge on
 * ring N and S.  mdx_mol_kekulize is THIS PROJECT'S OWN MODEL of that second test, without RDKit and UNVERIFIED AGAINST IT, of the
 * molecule AS DECODED.  The structure it reports is the FIRST ONE FOUND in the search order below, not a charge-minimal one.  Every
 * output is defined so that its value is unique, and a plain restatement (moldiff_amd/kekule.py: kekulize_ref) must agree exactly.
 *
 * The molecule: the compact layout of mdx_mol_rings (atom_ptr .. select: as there); its VALID bonds only (both indices inside the
 *   molecule, i != j; the others are ignored).  A bond type outside 1 .. num_bond_types leaves the bond in the graph, adds nothing and
 *   is not aromatic.  The last type, num_bond_types, is AROMATIC.  Two bonds between one pair of atoms are a PRECONDITION VIOLATION as
 *   for mdx_mol_rings: results unspecified, the kernel stays in bounds and ends.
 * Chemistry is data: three HOST tables indexed by atom class, validated by the call and sent as kernel arguments (the caller may
 *   overwrite them as soon as the call returns).  normal_valence V[c], 0 .. 64; charged_valence Vc[c], 0 .. 64: 0 = none, otherwise
 *   the valence with one positive charge; flexible: bit c set = class c takes a hydrogen instead of a double bond.  An atom of a class
 *   outside 0 .. num_element - 1 has V = Vc = 0 and is not flexible.  (The shipped featuriser's defaults, moldiff_amd/kekule.py:
 *   V = C 4, N 3, O 2, F 1, P 3, S 2, Cl 1; Vc = N 4, S 3; flexible = {N}: this project's choice.)
 * Per atom: sigma = the sum of the orders of its valid non-aromatic bonds (types 1 .. num_bond_types - 1 count their number) + the
 *   number of its aromatic bonds; adeg = the number of its aromatic bonds.  An atom with adeg >= 1 has one ROLE:
 *     NOT  (1)  adeg > 3; or neither case below applies (no room, or over-valent);
 *     MUST (2)  V - sigma >= 1 and the class is not flexible;
 *     MAY  (3)  V - sigma >= 1 and the class is flexible (it takes a hydrogen instead); or V - sigma < 1 and Vc - sigma >= 1 (it takes
 *               a charge if matched).
 *   An atom without an aromatic bond has role 0.
 * The connected components of the aromatic bonds are treated independently.  Within a component a KEKULÉ STRUCTURE is a matching on
 *   aromatic bonds: both ends of every bond in it have a role other than NOT, and it covers every MUST atom.
 * THE CANONICAL STRUCTURE is the first one found by this search; the order is part of the definition:
 *   1. walk the component's atoms in ascending index;
 *   2. skip an atom that is NOT or already matched;
 *   3. otherwise its options are, in this order: "stay unmatched" (MAY atoms only), then each aromatic neighbour with a higher index
 *      that is not NOT and not yet matched, in ascending index;
 *   4. try the next option and go on to the next atom;
 *   5. with no option left, undo and return to the previous deciding atom;
 *   6. passing the last atom is success; exhausting the first deciding atom's options is "no structure".
 *   steps counts the options tried, each try one step, up to the success or the exhaustion.  A component whose steps would exceed
 *   max_steps (1 .. 2^20, per component) is OVER BUDGET.  A component is UNSOLVED when it has no structure or is over budget.
 * Outputs (device int32, plain stores by the molecule's own workgroup: bit-reproducible, independent of the place in the batch):
 *   kek_order  per bond slot (Eh_stride): types 1 .. num_bond_types - 1 unchanged; an aromatic bond 2 if in the matching, else 1; an
 *              ignored bond, a type outside 1 .. num_bond_types and an aromatic bond of an unsolved component 0.
 *   val        per atom slot (N_cap): sigma + 1 if the atom is matched, else sigma.
 *   charge     1 iff V < val <= Vc, else 0 (a non-aromatic four-valent N gets its charge too, as fix_valence does).
 *   kek_h      max(0, (Vc if charge else V) - val): the hydrogens of the assignment.
 *   atom_flag  bits 0-1 the role, bit 2 matched, bit 3 val > max(V, Vc), bit 4 the atom's component is unsolved.  Atoms of an unsolved
 *              component have kek_h 0, charge 0, bit 2 clear and bit 4 set; all other atoms of the molecule are still measured.
 *   mol_stats  [m][k], k < MDX_KEKULE_STATS = 11:
 *     0 status         0 measured; 1 too large: n_atoms > 256 or n_bonds > 512 (the caps of mdx_mol_rings; ignored bonds included), or
 *                      an aromatic component of more than 64 atoms.  Every other output of the molecule is then 0, its slots included.
 *     1 n_arom_atoms   atoms with adeg >= 1             2 n_arom_bonds    valid aromatic bonds
 *     3 n_components   aromatic components              4 n_failed        components with no structure
 *     5 n_over_budget  components over budget           6 n_double        aromatic bonds in the matchings
 *     7 n_charged      atoms with charge 1              8 n_hydrogens     the sum of kek_h
 *     9 n_overvalent   atoms with flag bit 3           10 steps           summed over the components; one over budget adds 0
 *   select, and a molecule reaching past N_cap / Eh_stride, as for mdx_mol_rings: status 0, all outputs 0 (the slots of the latter are
 *   not written).  Slots that belong to no molecule are not written.  A molecule is KEKULIZABLE iff status == 0 and n_failed ==
 *   n_over_budget == 0.
 * One workgroup of 256 threads per molecule, the molecule staged once in LDS (about 8 KB); each component is searched by one thread
 * with its state in registers, which is what the cap of 64 atoms per component is for.  There is no workspace.
 * MDX_ERR_ARG, every output untouched: a null operand (select excepted), a negative size, num_element outside 1 .. 32, num_bond_types
 * outside 1 .. 16, a table value outside 0 .. 64, a flexible bit at or above num_element, max_steps outside 1 .. 2^20.
 * B = 0 is accepted and writes nothing. */
#define MDX_KEKULE_STATS 11
int mdx_mol_kekulize(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                     const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                     const int32_t* select, int32_t num_element, int32_t num_bond_types, const int32_t* normal_valence,
                     const int32_t* charged_valence, uint32_t flexible, int32_t max_steps, int32_t* kek_order, int32_t* val,
                     int32_t* charge, int32_t* kek_h, int32_t* atom_flag, int32_t* mol_stats, void* stream);

/* ---- Canonical labelling of decoded molecules: exact keys, symmetry classes, the canonical atom order -------------------
 * The reference reports uniqueness and novelty from RDKit's canonical SMILES (utils/scoring_func.py:172-175).  mdx_mol_canon is THIS
 * PROJECT'S OWN DEFINITION of a canonical form, without RDKit: it is NOT RDKit's canonical ranking (CanonicalRankAtoms) and what is
 * written from it is not RDKit's canonical SMILES.  It is canonical among runs of this project.  Every output has one value whatever
 * the order of the atoms or of the traversal, and a plain restatement (moldiff_amd/canon.py: canon_ref) must agree exactly.
 *
 * INPUT.  The compact layout of mdx_mol_rings (atom_ptr .. select: as there).  A molecule has n atoms and a list of bonds
 *   (i, j, type); a bond with an index outside the molecule or with i = j is ignored, as everywhere.  Several bonds between one pair
 *   of atoms are allowed: the bonds are a multiset and nothing below minds.  `type` is the low 8 bits of bond_type.  Every atom has a
 *   label L(v) >= 0: atom_type[v], or atom_label[v] when the caller gives that array (device int32 in [0, 65536), the layout of
 *   atom_type; it folds in charge or hydrogen count; the range is the caller's word and is checked by the Python wrappers on host
 *   arrays).  mix is murmur3's fmix32, as in mdx_mol_fingerprint.
 * COLOURS.  A colouring c gives every atom a number in [0, n): always "how many atoms have a strictly smaller key".  Equal keys share
 *   a colour, and a cell of size s at colour k leaves k + 1 .. k + s - 1 unused.
 *     initial:  the key is L(v).
 *     a round:  h(v) = SUM over the valid bonds {v, u} of v of mix(mix(c(u) + 1) + type), a wrapping 32-bit sum;
 *               key(v) = c(v) * 2^32 + h(v);  c'(v) = #{u : key(u) < key(v)};  repeat until c' = c.
 *   A hash collision can only leave a cell unsplit and the search below is exact regardless; every step depends on nothing but the
 *   graph.
 * SEARCH TREE.  A node is a refined colouring.  If all colours are distinct it is a LEAF with rank(v) = c(v).  Otherwise its TARGET
 *   CELL is the non-singleton cell of smallest colour k, and it has one child per atom v of that cell: from the node's colouring,
 *   c(u) = k + 1 for every other atom u of the cell while v keeps k, then refinement.  The root is the refined initial colouring, at
 *   depth 0.  There is NO PRUNING OF ANY KIND: the tree, its node count and its leaf count are properties of the graph alone, and so
 *   is every status below.
 * CERTIFICATE of a leaf: every valid bond as the word lo * 2^20 + hi * 2^8 + type, lo < hi the ranks of its atoms, the words sorted
 *   ascending; certificates compare lexicographically.  The CANONICAL certificate is the smallest over all leaves.  The FULL
 *   CERTIFICATE of the molecule is the int32 sequence n, the labels at ranks 0 .. n - 1, the number of valid bonds, the words: two
 *   molecules are the same labelled graph iff their full certificates are equal.  cert_hash is FNV-1a-64 over those values taken as
 *   uint32: h = 0xcbf29ce484222325, then h = (h xor w) * 0x100000001b3 mod 2^64 per value.  It is for grouping on the device;
 *   equality of molecules is always decided on the full certificate.
 * OUTPUTS (device, plain stores by the molecule's own workgroup: bit-reproducible, independent of the place in the batch):
 *   mol_stats  [m][k], k < MDX_CANON_STATS = 5 (int32):
 *     0 status         0 measured; 1 more than 256 atoms or 512 bonds (the caps of mdx_mol_rings; ignored bonds included); 2 search
 *                      abandoned: the tree has more than max_nodes nodes (1 .. 2^20) or a node deeper than 64 -- one status, because
 *                      whichever the walk meets first the answer is the same.
 *     1 n_nodes  2 n_leaves   the size of the tree, the root counted
 *     3 n_aut          the leaves that attain the canonical certificate = the order of the automorphism group of the labelled graph
 *     4 canon_n_bonds  the valid bonds
 *   cert_hash  (B) int64.
 *   rank       per atom slot (N_cap): the rank vector of the optimal leaf whose vector (rank[0], rank[1], ..) is lexicographically
 *              smallest among the optimal leaves (a minimum over a set: it looks at the input order, not at the traversal).
 *   orbit      per atom slot: the smallest index of an atom that some automorphism maps v to = the smallest atom found at rank[v] in
 *              any optimal leaf.
 *   canon_atom_type, canon_atom_label (iff atom_label), canon_pos (iff atom_pos; 3 floats per slot): the atom of rank p in slot
 *              atom_ptr[m] + p.  canon_bond_index (2 rows of Eh_stride: lo, hi) and canon_bond_type at bond_ptr[m] ..: the words of
 *              the canonical certificate in order; the molecule's bond slots behind canon_n_bonds are 0.  Isomorphic inputs give
 *              identical canonical arrays, the positions permuted alike.  The canonical arrays with canon_n_bonds are again a
 *              compact molecule: mdx_mol_kekulize, mdx_mol_groups and mdx_mol_rings run on them directly.
 *   With a non-zero status, under select, and for a molecule reaching past N_cap / Eh_stride (whose slots are not written): rank -1
 *   and every other output 0, status as said (0 for the latter two).  Slots that belong to no molecule are not written.
 * One workgroup of 256 threads per molecule, thread a = atom a, the whole state in about 30 KB of LDS (the stack of 64 colour
 * snapshots is 16 KB of it).  There is no workspace.
 * MDX_ERR_ARG, every output untouched: a null operand (select, atom_pos, atom_label and their two outputs excepted), atom_label
 * without canon_atom_label or atom_pos without canon_pos or the reverse, a negative size, max_nodes outside 1 .. 2^20.
 * B = 0 is accepted and writes nothing. */
#define MDX_CANON_STATS 5
int mdx_mol_canon(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                  const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                  const int32_t* select, const float* atom_pos, const int32_t* atom_label, int32_t max_nodes, int32_t* rank,
                  int32_t* orbit, int32_t* canon_atom_type, int32_t* canon_atom_label, float* canon_pos, int32_t* canon_bond_index,
                  int32_t* canon_bond_type, int32_t* mol_stats, int64_t* cert_hash, void* stream);

/* ---- Stereo perception of decoded molecules: tetrahedral parities, cis / trans codes, the isomeric key ---------------------
 * The reference's uniqueness and novelty come from Chem.MolToSmiles of molecules read back from 3D mol blocks
 * (utils/scoring_func.py:170, utils/evaluation.py:360), where RDKit perceives stereo from the coordinates; the certificate of
 * mdx_mol_canon sees the constitution only.  mdx_mol_stereo turns the coordinates into labels that do not depend on atom order,
 * rotation, translation or the choice among automorphisms.  It is THIS PROJECT'S OWN DEFINITION: it is NOT RDKit's stereo perception
 * and NOT the CIP rules, and it is UNVERIFIED AGAINST RDKit.  It is blind to allenes and cumulenes, to atropisomers and to nitrogen
 * inversion (an N with 4 bonds is a centre, one with 3 is not), and every label depends on flat_tol and bond_tol.  A plain
 * restatement (moldiff_amd/stereo.py: stereo_ref) must agree with the device on every output.
 *
 * INPUT.  The compact layout of mdx_mol_rings (atom_ptr .. select: as there; valid bonds only: a bond with an index outside the
 *   molecule or with i = j is ignored); `type` is the low 8 bits of bond_type.  atom_pos (3 floats per atom slot), required.  rank
 *   (N_cap) and canon_status (B: column 0 of canon's mol_stats, as an array of its own) exactly as mdx_mol_canon wrote them for the
 *   same arrays and the same atom_label (the convention mdx_mol_framework uses for the rings outputs); the optional atom_label is
 *   passed again.  Two bonds between one pair of atoms are a PRECONDITION VIOLATION as for mdx_mol_rings: results unspecified, the
 *   kernel stays in bounds and ends.  centre4_mask / centre3_mask: bit c set = atom class c may be a centre (classes from 32 on
 *   never are); the defaults of the Python side are C, N, P, S and C.
 * GEOMETRY, computed once per molecule in float64 from the float32 positions, every product and sum rounded on its own (no fused
 *   multiply-add), (a.b) = (ax bx + ay by) + az bz, det[a, b, c] = (ax (by cz - bz cy) - ay (bx cz - bz cx)) + az (bx cy - by cx).
 *   Nothing below reads a coordinate again.
 *   TETRAHEDRAL CANDIDATE: an atom with 4 valid bonds whose class bit is set in centre4_mask, or with 3 valid bonds, all of type 1,
 *     whose class bit is set in centre3_mask (the centre with one implicit hydrogen).  With d_i the vector from the atom to its i-th
 *     neighbour in ascending atom index and u_i = d_i / sqrt(d_i.d_i):  3 neighbours: v = det[u1, u2, u3], threshold flat_tol;
 *     4 neighbours: v = det[u2 - u1, u3 - u1, u4 - u1], threshold 4 flat_tol (ideal values 0.77 and 3.08).  g = +1 if v > threshold,
 *     -1 if v < -threshold, else 0; g = 0 also when d_i.d_i is not above 0 or a coordinate of the atom or of a neighbour is not
 *     finite.  The default flat_tol of 0.1 is this project's untuned choice.
 *   DOUBLE-BOND CANDIDATE: a valid bond a-b of type exactly 2 whose ends each have 1 or 2 other valid bonds, none of them of type 2
 *     or 3.  Cumulenes and allene axes are OUT OF SCOPE: their bonds are no candidates.  For every pairing (x another neighbour of a,
 *     y another neighbour of b), up to four per bond: e = (p_b - p_a) / |p_b - p_a|; dx = p_x - p_a, dy = p_y - p_b;
 *     x' = dx - (dx.e) e, y' = dy - (dy.e) e; c = (x'.y') / (sqrt(x'.x') sqrt(y'.y')); d(x, y) = 1 (cis) if c > bond_tol, 2 (trans) if
 *     c < -bond_tol, else 0; 0 also when p_b = p_a, x'.x' or y'.y' is not above 0 or a coordinate of the four atoms is not finite.
 *     The default bond_tol is 0.1.  There is no ring exclusion: a small-ring double bond is simply always cis.
 * WORD OF A LEAF.  An OPTIMAL LEAF of canon's search tree is a leaf whose certificate equals the canonical one; there are n_aut of
 *   them.  For an optimal leaf with rank vector pi the word w(pi) has n + canon_n_bonds values:
 *     p < n: the code of the atom at leaf rank p.  0: no candidate, or g = 0.  Otherwise list the leaf ranks of its neighbours in
 *       ascending atom index; s = +1 if that list has an even number of inversions, else -1 (the sign of the permutation that sorts
 *       the neighbours by rank); the code is 1 if g s > 0 and 2 if g s < 0.
 *     k < canon_n_bonds: w[n + k] is the code of the bond whose ends carry the ranks of word k of the canonical certificate: 0 if it
 *       is no candidate, otherwise d(x, y) with x and y the other neighbours of smallest leaf rank on each end.
 *   The MIRROR WORD is w with the atom codes 1 and 2 swapped.
 * CANONICAL STEREO WORD.  W is the lexicographic minimum of w(pi) over all optimal leaves, M the minimum of the mirror words.  Both
 *   are functions of the labelled graph and the geometry only: the set of optimal leaves is carried onto itself by every relabelling
 *   of the input, and the codes are built from ranks and from signs that change together under a renumbering.  They do not depend on
 *   atom order, traversal, rotation or translation; a reflection swaps W and M.  The molecule is CHIRAL iff W != M.  stereo_rank is
 *   the lexicographically smallest rank vector among the leaves attaining W (the tie rule of rank).
 *   The ISOMERIC KEY of a molecule is (full certificate of mdx_mol_canon, W); equality is decided on that pair, never on the hashes.
 * OUTPUTS (device, plain stores by the molecule's own workgroup: bit-reproducible, independent of the place in the batch):
 *   canon_tetra (N_cap) and canon_bond_stereo (Eh_stride) hold W: W[p] at atom_ptr[m] + p, W[n + k] at bond_ptr[m] + k, aligned with
 *              canon_atom_type and canon_bond_index of the canon call; the molecule's bond slots behind canon_n_bonds are 0.
 *   mirror_tetra (N_cap) and mirror_bond_stereo (Eh_stride) hold M alike: the W of the mirror image, so that "the enantiomer occurs"
 *              is decided on the words themselves.
 *   stereo_rank (N_cap).   atom_tetra (N_cap): atom_tetra[v] = W[stereo_rank[v]], in input order.
 *   bond_stereo (Eh_stride): per input bond slot the code W[n + k] of the bond, k its word's place under stereo_rank; 0 for an
 *              ignored bond.
 *   stereo_hash, mirror_hash (B) int64: FNV-1a-64 over the n + canon_n_bonds values of W and of M, with the constants of cert_hash.
 *   mol_stats  [m][k], k < MDX_STEREO_STATS = 9 (int32):
 *     0 status               0 measured; 1 no canonical form: canon_status[m] != 0, more than 256 atoms or 512 bonds, or a rank that
 *                            is not canon's for these arrays (outside 0 .. n - 1, or no leaf attains its certificate); 2 the walk
 *                            exceeded max_nodes (1 .. 2^20) or depth 64 -- never with canon's own max_nodes: it is the same tree.
 *     1 n_centre_candidates  2 n_centres: non-zero atom codes in W       3 n_flat: candidates with g = 0
 *     4 n_bond_candidates    5 n_stereo_bonds: non-zero bond codes in W
 *     6 n_stereogenic        centres with a non-zero code whose neighbours lie in pairwise distinct orbits of canon (the implicit
 *                            hydrogen is one more neighbour, distinct from all).  The orbits are taken from this walk.
 *     7 chiral   W != M      8 n_aut: the optimal leaves seen; equals canon's.
 *   With a non-zero status, under select, and for a molecule reaching past N_cap / Eh_stride (whose slots are not written):
 *   stereo_rank -1 and every other output 0, status as said (0 for the latter two).  Slots that belong to no molecule are not written.
 * One workgroup of 256 threads per molecule, thread a = atom a, the walk of mdx_mol_canon (csrc/mdx_canon_body.h) with the whole state
 * in about 35 KB of LDS.  There is no workspace and there are no global atomics.
 * MDX_ERR_ARG, every output untouched: a null operand (select and atom_label excepted), a negative size, flat_tol or bond_tol outside
 * [0, 1) or NaN, max_nodes outside 1 .. 2^20.  B = 0 is accepted and writes nothing. */
#define MDX_STEREO_STATS 9
int mdx_mol_stereo(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                   const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                   const int32_t* select, const float* atom_pos, const int32_t* atom_label, const int32_t* rank,
                   const int32_t* canon_status, uint32_t centre4_mask, uint32_t centre3_mask, double flat_tol, double bond_tol,
                   int32_t max_nodes, int32_t* canon_tetra, int32_t* canon_bond_stereo, int32_t* mirror_tetra,
                   int32_t* mirror_bond_stereo, int32_t* stereo_rank, int32_t* atom_tetra, int32_t* bond_stereo, int32_t* mol_stats, int64_t* stereo_hash, int64_t* mirror_hash, void* stream);

/* ---- Symmetry-aware best RMSD between conformers of one constitution ------------------------------------------------------
 * The reference's `global_3d` metric is get_rdkit_rmsd (utils/scoring_func.py:56-74): rdMolAlign.GetBestRMS(mol, mol3d), the RMSD
 * after optimal rigid superposition, minimised over every atom mapping that the symmetry of the molecule allows.  mdx_mol_bestrms is
 * the alignment half of it.  There is NO CONFORMER GENERATION in this entry: conformers come from mdx_mol_bounds + mdx_mol_embed and
 * mdx_mol_relax below (this project's own distance geometry and force field, not the reference's ETKDG + UFF) or from another program, the atoms
 * are the HEAVY ATOMS of the compact molecule, and the symmetry group is that of THIS PROJECT'S LABELLED GRAPH (mdx_mol_canon; aromatic
 * bonds are a type of their own), which can be smaller than RDKit's substructure match on a kekulised input.  It is pure mathematics;
 * a plain restatement (moldiff_amd/rmsd.py: best_rms_ref, numpy's SVD) agrees to a tolerance derived from float64 alone.  Agreement
 * with RDKit's GetBestRMS beyond this shared definition is UNMEASURED.
 *
 * THE QUANTITY.  A probe molecule A and a target B with the same full certificate of mdx_mol_canon: the same n, the same canonical
 *   atom labels and the same canonical bond words.
 *   ATOM MAPS.  Every OPTIMAL LEAF of A's search tree (its certificate equals the canonical one) has a rank vector c; it gives the
 *     atom map a -> B's canonical atom c[a].  Over all optimal leaves these are exactly the n_aut graph-preserving maps of A onto B.
 *   ONE MAP, all in float64: both point sets are centred (p_a: A's atoms; q_k: B's atoms in canonical order);
 *     Ga = sum |p_a|^2, Gb = sum |q_k|^2, H = sum p_a q_{c[a]}^T, s1 >= s2 >= s3 >= 0 the singular values of H;
 *     msd        = max(0, Ga + Gb - 2 (s1 + s2 + sign(det H) s3)) / n     proper rotations only, as GetBestRMS
 *     msd_mirror = max(0, Ga + Gb - 2 (s1 + s2 - sign(det H) s3)) / n     the same against the mirror image of B
 *   PER PAIR: msd and msd_mirror are the minima over all maps; msd_first is msd of the map given by A's own canonical rank (no symmetry
 *     search: msd_first - msd is what the search bought); n_maps the maps evaluated (canon's n_aut).  n = 0 and n = 1 give 0.
 *     These are MEAN SQUARED deviations; the RMSD is their root and is taken on the host, so that a comparison is not amplified
 *     near zero.  Non-finite coordinates give unspecified values.
 * INPUT.  The compact layout of mdx_mol_rings for the probes (atom_ptr .. select: as there); atom_pos, rank, canon_status and the
 *   optional atom_label exactly as for mdx_mol_stereo.  The pairs as CSR: probe m owns the pairs pair_ptr[m] .. pair_ptr[m + 1]
 *   (pair_ptr holds B + 1 values), pair_target[p] is the pair's target in 0 .. T - 1, and the per-pair arrays hold P_cap rows.  The
 *   targets: tgt_ptr (T), tgt_n (T) and tgt_pos (tgt_atoms x 3, float32) IN CANONICAL ATOM ORDER -- what canon_pos of mdx_mol_canon
 *   holds.  That a target has the probe's constitution is the CALLER'S WORD: the kernel only guards memory.
 * OUTPUTS (device, plain stores by the probe's own workgroup, every sum in a fixed order: bit-reproducible, independent of the place
 *   in the batch):
 *   msd, msd_mirror, msd_first (P_cap) float64.    pair_stats [p][2] (int32): n_maps, status.
 *   mol_stats [m][k], k < MDX_BESTRMS_STATS = 3 (int32): status, the nodes of the walk, the optimal leaves seen (canon's n_nodes, n_aut).
 *   status of a pair: 0 measured; 1 no canonical form: canon_status[m] != 0, more than 256 atoms or 512 bonds, or a rank that is
 *     not canon's for these arrays (outside 0 .. n - 1, or no leaf attains its certificate); 2 the walk exceeded this call's
 *     max_nodes (1 .. 2^20) or depth 64; 3 the target cannot be this probe's: pair_target outside 0 .. T - 1, tgt_n != n, or an
 *     extent outside tgt_pos.  1 and 2 are the probe's and stand in its mol_stats too.  With a non-zero status the floats and n_maps
 *     are 0.  A probe under select gets status 0 and zeros.  A probe reaching past N_cap / Eh_stride is not read and nothing is
 *     written for it; a pair extent outside 0 .. P_cap is no pair at all.  Rows that belong to no probe are not written.
 * One workgroup of 256 threads per probe, thread a = atom a, the walk of mdx_mol_canon (csrc/mdx_canon_body.h); at an optimal leaf
 * wave w takes the pairs w, w + 4, ..., sums H over its lanes and solves Horn's 4 x 4 quaternion matrix by cyclic Jacobi.  About 59 KB
 * of LDS; no workspace, no global atomics.
 * MDX_ERR_ARG, every output untouched: a null operand (select and atom_label excepted), a negative size, P_cap or tgt_atoms from 2^31
 * on, max_nodes outside 1 .. 2^20.  B = 0 is accepted and writes nothing. */
#define MDX_BESTRMS_STATS 3
int mdx_mol_bestrms(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                    const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                    const int32_t* select, const float* atom_pos, const int32_t* atom_label, const int32_t* rank,
                    const int32_t* canon_status, const int32_t* pair_ptr, const int32_t* pair_target, int64_t P_cap, int32_t T,
                    const int32_t* tgt_ptr, const int32_t* tgt_n, const float* tgt_pos, int64_t tgt_atoms, int32_t max_nodes,
                    double* msd, double* msd_mirror, double* msd_first, int32_t* pair_stats, int32_t* mol_stats, void* stream);

/* ---- Frameworks and ring systems of decoded molecules: the skeleton without its decoration, as compact molecules ------
 * The reference's `ring_type` metric (utils/evaluation.py: RingAnalyzer.get_count_ring, get_freq_rings, get_ring_topo, fr_bicyclic)
 * reports which rings occur and how often, and scaffold uniqueness / diversity / novelty are the usual second half of a generative
 * model's report.  mdx_mol_rings offers no ring SMILES because a ring basis is a choice; a RING SYSTEM and the FRAMEWORK are unique
 * functions of the graph.  mdx_mol_framework cuts every molecule into framework, ring systems, linkers and side chains and hands the
 * pieces back as compact molecules, so that mdx_mol_canon gives each an exact key with one more launch.  It is THIS PROJECT'S OWN
 * DEFINITION in the spirit of Bemis and Murcko; it is NOT rdkit.Chem.Scaffolds.MurckoScaffold and is UNVERIFIED AGAINST RDKit.  Every
 * output has one value whatever the order of the traversal, and a plain restatement (moldiff_amd/framework.py: framework_ref) must
 * agree exactly.
 *
 * INPUT.  The compact layout of mdx_mol_rings (atom_ptr .. select: as there); atom_pos (3 floats per atom slot) is optional.  A bond
 *   with an index outside the molecule or with i = j is ignored.  Two bonds between one pair of atoms are a PRECONDITION VIOLATION as
 *   for mdx_mol_rings: results unspecified, the kernel stays in bounds and ends.  bond_ring_min (Eh_stride) and ring_status (B)
 *   exactly as mdx_mol_rings wrote them for the same arrays (the convention of mdx_mol_groups).  mode: bit 0 MDX_FW_EXO, bit 1
 *   MDX_FW_GENERIC.  sys_bins in 1 .. 16.
 * DEFINITIONS.  G is the graph of the valid bonds.
 *   A RING BOND is a valid bond with bond_ring_min != 0 (no bridge), a RING ATOM an atom with at least one ring bond.
 *   The CORE F0 is what remains after deleting, until nothing changes, every atom that has at most one remaining bond: the 2-core of
 *     G, the ring atoms and the atoms on paths between them.  An acyclic molecule has an empty core.  A core atom without a ring
 *     bond is a LINKER ATOM.
 *   With EXO an atom outside F0 is an EXO ATOM, and joins the framework with its bond, when it has exactly one valid bond, that bond
 *     has type 2 and leads to an atom of F0 (carbonyl O on a ring or a linker; not acetone's O: no core).
 *   The FRAMEWORK F is F0 plus the exo atoms, with every valid bond between two atoms of F0 and the exo bonds.
 *   A RING SYSTEM is a connected component of (ring atoms, ring bonds).  Spiro and fused rings share atoms and form one system;
 *     biphenyl has two.  Systems are numbered 0, 1, .. by their smallest atom index; one with a atoms and b bonds has b - a + 1 rings.
 *   A FUSION ATOM is a ring atom with at least three ring bonds.
 * OUTPUTS (device int32, fw_pos / sys_pos float and present iff atom_pos; plain stores by the molecule's own workgroup, every slot
 *   written once: bit-reproducible, independent of the place in the batch):
 *   atom_role    per atom slot (N_cap): 0 side chain, 1 linker, 2 ring, 3 exo.
 *   atom_system  per atom slot: the ordinal of the atom's ring system, -1 for an atom in none.
 *   bond_role    per bond slot (Eh_stride): 0 not in F (ignored bonds included), 1 framework bond that is no ring bond, 2 ring bond,
 *                3 exo bond.
 *   mol_stats    [m][k], k < MDX_FW_STATS = 10:
 *     0 status   0 measured; 1 too large: n_atoms > 256 or n_bonds > 512 (the caps of mdx_mol_rings); 2 ring_status[m] != 0
 *     1 framework atoms      2 framework bonds     3 ring systems     4 linker atoms     5 side-chain atoms     6 exo atoms
 *     7 fusion atoms         8 atoms of the largest system            9 rings of the system with most rings
 *   sys_hist     [m][k], k < sys_bins: the systems with 1 + k rings, the last bin also every larger one.  SUM = mol_stats[m][3].
 *   THE FRAMEWORK AS A COMPACT MOLECULE in the molecule's own slots: fw_atom_type, fw_atom_map (the original local index) and fw_pos
 *     from atom_ptr[m]; fw_bond_index (2 rows of Eh_stride: renumbered, direction kept) and fw_bond_type from bond_ptr[m].  Atoms and
 *     bonds keep their relative order; the counts are mol_stats[m][1] and [2]; the molecule's atom and bond slots behind the counts
 *     are 0.
 *   THE RING SYSTEMS AS COMPACT MOLECULES, disjoint and so again in the molecule's own slots: system k of molecule m has its record
 *     at slot atom_ptr[m] + k of sys_atom_ptr, sys_bond_ptr, sys_n_atoms, sys_n_bonds (N_cap each).  Its atoms lie contiguously from
 *     sys_atom_ptr = atom_ptr[m] + the sizes of the earlier systems, its bonds likewise from bond_ptr[m]; within a system both keep
 *     their relative order.  Per atom sys_atom_type, sys_atom_map (the original local index), sys_pos; per bond sys_bond_index (2
 *     rows, local to the system, direction kept) and sys_bond_type.  Record slots of the molecule at or behind its system count hold
 *     0 in all four arrays; so do the atom and bond slots behind the ring atoms / ring bonds.
 *   GENERIC writes class 0 for every atom and type 1 for every bond in the fw_* and sys_* type arrays; roles, stats and maps are
 *     unchanged.
 *   With a non-zero status, under select, and for a molecule reaching past N_cap / Eh_stride (whose slots are not written): every
 *   count is 0, atom_system -1, every other output 0, status as said (0 for the latter two).  Slots that belong to no molecule are
 *   not written.
 * One workgroup of 256 threads per molecule, thread a = atom a, the whole state in about 19 KB of LDS.  There is no workspace.
 * MDX_ERR_ARG, every output untouched: a null operand (select, atom_pos and its two outputs excepted), atom_pos without fw_pos or
 * sys_pos or the reverse, a negative size, mode bits above 1, sys_bins outside 1 .. 16.
 * B = 0 is accepted and writes nothing. */
#define MDX_FW_STATS 10
#define MDX_FW_EXO 1
#define MDX_FW_GENERIC 2
int mdx_mol_framework(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                      const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                      const int32_t* select, const float* atom_pos, const int32_t* bond_ring_min, const int32_t* ring_status,
                      int32_t mode, int32_t sys_bins, int32_t* atom_role, int32_t* atom_system, int32_t* bond_role, int32_t* mol_stats,
                      int32_t* sys_hist, int32_t* fw_atom_type, int32_t* fw_atom_map, float* fw_pos, int32_t* fw_bond_index,
                      int32_t* fw_bond_type, int32_t* sys_atom_ptr, int32_t* sys_bond_ptr, int32_t* sys_n_atoms, int32_t* sys_n_bonds,
                      int32_t* sys_atom_type, int32_t* sys_atom_map, float* sys_pos, int32_t* sys_bond_index, int32_t* sys_bond_type,
                      void* stream);

/* ---- Explicit hydrogens with 3D coordinates for decoded molecules, and their contacts ------------------------------------
 * Every molecule this project writes is heavy-atom only; the reference itself reaches hydrogens only through Chem.AddHs inside
 * get_rdkit_rmsd (utils/scoring_func.py:56-74).  mdx_mol_hydrogens places the hydrogens that a Kekulé assignment counts from the local
 * geometry of the heavy atoms and measures the all-atom contacts of what it placed.  It is THIS PROJECT'S OWN IDEALISED PLACEMENT: NOT
 * RDKit's AddHs(addCoords=True) and UNVERIFIED AGAINST IT.  Torsions of rotors (methyl, hydroxyl, amine) are fixed by the rule below,
 * not by an energy; a pyramidal nitrogen takes the side set by the order of its neighbours; an atom without neighbours, and an atom
 * whose only neighbour has no other, use fixed world axes, so such hydrogens do not turn with the molecule (WORLD_FRAME).  The length
 * table and clash_tol are conventions.  Every output has exactly one value, and a plain restatement (moldiff_amd/hydrogens.py:
 * addh_ref) agrees in the integers exactly and in the floats to float64 rounding.
 *
 * INPUT.  The compact layout of mdx_mol_rings (atom_ptr .. select: as there); a bond with an index outside the molecule or with i = j
 *   is ignored.  atom_pos: 3 floats per atom slot, widened to float64 once; everything below is float64.  n_h (N_cap) and order
 *   (Eh_stride): int32 device arrays, normally kek_h and kek_order of mdx_mol_kekulize, but any caller's arrays are legal: h =
 *   n_h clamped to 0 .. 4 (CLAMPED when that changes it; an atom of a class outside 0 .. num_element - 1 has h = 0); the order of a
 *   valid bond is `order` clamped to 1 .. 3, so 0 counts as 1.  A bond of type num_bond_types is AROMATIC whatever its order.  Two
 *   bonds between one pair of atoms are a precondition violation as for mdx_mol_rings: unspecified results, in bounds.
 *   HOST tables by atom class, validated by the call and sent as kernel arguments: xh_length[c] in Angstrom, 0 < L <= 4 (the shipped
 *   defaults, moldiff_amd/hydrogens.py: C 1.09, N 1.01, O 0.96, F 0.92, P 1.42, S 1.34, Cl 1.27: this project's choice of textbook
 *   values); planar_mask: bit c set = class c flattens next to a pi system (default {N}).  deg_tol in (0, 1), default 1e-3.
 *   clash_tol in [0, 1000] Angstrom, default 1.5: a convention, untuned.
 * GEOMETRY of an atom with d valid bonds (neighbours) and h hydrogens:
 *   LINEAR (2, room 2)       it has a bond of order 3, or two of order 2;
 *   TRIGONAL (1, room 3)     else, if it has a bond of order 2 or an aromatic bond; or its class is in planar_mask, it is not
 *                            trigonal or linear by the rules so far, and some neighbour is (by those rules alone);
 *   TETRAHEDRAL (0, room 4)  else.
 *   NO_ROOM: h >= 1 and d + h > room.  None of the atom's hydrogens is placed.
 * PLACEMENT of an atom a at p with h >= 1 that has room.  u_k: the unit vectors (v / sqrt(v.v), v = neighbour - p) to the neighbours
 *   in ascending atom index; L: the class's length; hydrogen k stands at p + L dir_k.  (x.y = (x0 y0 + x1 y1) + x2 y2; |x| = sqrt(x.x);
 *   x X y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0).)  theta = acos(-1/3), or 120 degrees for TRIGONAL.
 *   d = 0  dir_k = the k-th fixed world direction.  TETRAHEDRAL: (1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1), each / sqrt 3; TRIGONAL:
 *          (1,0,0), (-1/2, sqrt 3 / 2, 0), (-1/2, -sqrt 3 / 2, 0); LINEAR: (1,0,0), (-1,0,0).  WORLD_FRAME.
 *   d = 1  e = u_1, n1 the neighbour.  LINEAR: dir_0 = -e.  Otherwise the reference w: walk n1's neighbours r != a in ascending
 *          index, skip one that coincides with n1 or is not finite, w = the unit vector from n1 to r, take the first with
 *          |e X w| >= deg_tol.  With none, w = the world axis with the smallest |e . axis|, the first of x, y, z among equals, and
 *          WORLD_FRAME.  f1 = (w - (w.e) e) normalised, f2 = e X f1, dir_k = cos theta e + sin theta (cos phi_k f1 + sin phi_k f2);
 *          TETRAHEDRAL phi_k = 180 + 120 k degrees (the first H anti to r), TRIGONAL phi = 180, then 0.
 *   d = 2  s = u_1 + u_2, c = u_1 X u_2.  TRIGONAL (h = 1): dir_0 = -s / |s|; needs |s| >= deg_tol.  TETRAHEDRAL: needs |c| >= deg_tol
 *          and |s| > 0; b = -s / |s|, n = c / |c|, beta = theta / 2: dir_0 = cos beta b + sin beta n, dir_1 = cos beta b - sin beta n.
 *   d = 3  TETRAHEDRAL (h = 1): s = (u_1 + u_2) + u_3, dir_0 = -s / |s|; needs |s| >= deg_tol.
 *   DEGENERATE: a needed condition fails, or a or a neighbour of it has a coordinate that is not finite, or a neighbour coincides
 *   with a.  None of the atom's hydrogens is placed.  WORLD_FRAME is reported for atoms whose hydrogens are placed only.
 *   The operation order of the restatement is part of the definition.
 * CONTACTS.  A contact is a pair (placed H, another atom of the molecule: a heavy atom with finite coordinates, or a placed H), each
 *   unordered pair once, without the 1-2 and 1-3 pairs: the H's parent, the parent's neighbours and the parent's other hydrogens.
 *   Its length is |other - H|.
 * OUTPUTS (device, plain stores by the molecule's own workgroup: bit-reproducible, independent of the place in the batch):
 *   h_pos        [N_cap][4][3] float64: atom slot a's k-th hydrogen, k < h_count[a]; the rest 0.
 *   h_count      per atom slot (int32): h when placed, else 0.
 *   atom_flag    bits 0-1 the geometry, 4 NO_ROOM, 8 DEGENERATE, 16 WORLD_FRAME, 32 CLAMPED.
 *   mol_stats    [m][k], k < MDX_HYDROGENS_STATS = 7 (int32):
 *     0 status        0 measured; 1 too large: n_atoms > 256 or n_bonds > 512.  Every other output of the molecule is then 0.
 *     1 n_h_wanted    the sum of h                      2 n_h_placed     the sum of h_count
 *     3 n_no_room     atoms flagged NO_ROOM             4 n_degenerate   atoms flagged DEGENERATE
 *     5 n_world_frame atoms flagged WORLD_FRAME         6 n_clash        contacts shorter than clash_tol
 *   min_contact  [m] float64: the shortest contact, +inf when a measured molecule has none.
 *   select, and a molecule reaching past N_cap / Eh_stride, as for mdx_mol_kekulize: status 0, all outputs 0, min_contact included
 *   (the slots of the latter are not written).  Slots that belong to no molecule are not written.
 * One workgroup of 256 threads per molecule; positions, adjacency and the 1024 x 3 table of hydrogens in LDS (about 41 KB); the
 * pairs are dealt over the threads and reduced with wave shuffles.  No workspace, no global atomics.
 * MDX_ERR_ARG, every output untouched: a null operand (select excepted), a negative size, num_element outside 1 .. 32, num_bond_types
 * outside 1 .. 16, a length outside (0, 4], a planar_mask bit at or above num_element, deg_tol outside (0, 1), clash_tol outside
 * [0, 1000].  B = 0 is accepted and writes nothing. */
#define MDX_HYDROGENS_STATS 7
int mdx_mol_hydrogens(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                      const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                      const int32_t* select, const float* atom_pos, const int32_t* n_h, const int32_t* order, int32_t num_element,
                      int32_t num_bond_types, const double* xh_length, uint32_t planar_mask, double deg_tol, double clash_tol,
                      double* h_pos, int32_t* h_count, int32_t* atom_flag, int32_t* mol_stats, double* min_contact, void* stream);

/* ---- Force-field relaxation of the all-atom molecule: strain energy and heavy-atom displacement ---------------------------
 * The reference's global_3d metric relaxes every molecule with UFFOptimizeMolecule between AddHs and GetBestRMS.  mdx_mol_relax
 * relaxes the all-atom molecule of mdx_mol_hydrogens in a force field of UFF's FUNCTIONAL FORMS by L-BFGS and reports the energy
 * before and after, the final gradient and how far the heavy atoms moved.  It is THIS PROJECT'S OWN MODEL: NOT RDKit's
 * UFFOptimizeMolecule and UNVERIFIED AGAINST IT; the shipped rows (configs/forcefield_default.yml) are a transcription from memory of
 * Rappe et al. 1992 and UNVERIFIED; hypervalent P and S use their tetrahedral row; there are no charges.  A plain restatement
 * (moldiff_amd/relax.py: energy_ref, relax_ref) repeats every operation in the same order.  Units: kcal/mol and Angstrom; float64.
 *
 * INPUT.  The compact layout of mdx_mol_rings; atom_pos, order as for mdx_mol_hydrogens; h_pos, h_count, atom_flag as
 *   mdx_mol_hydrogens wrote them (h = h_count clamped to 0 .. 4).  THE MOLECULE: the n heavy atoms in their order, then the hydrogens in
 *   (atom, k) order, n_all atoms; the valid compact bonds plus one X-H bond per hydrogen.  n > 256, n_bonds > 512 or n_all > 256:
 *   status TOO_LARGE.  A heavy atom's VARIANT is bits 0-1 of atom_flag (0 TETRAHEDRAL, 1 TRIGONAL, 2 LINEAR; 3 counts as 0), or RESONANT
 *   (3) when it has a bond of type num_bond_types; a class outside 0 .. num_element - 1 is clamped into it.  The ORDER n of a bond is 1.5
 *   for type num_bond_types, else `order` clamped to 1 .. 3, and 1 for X-H.
 *   ff_rows: HOST, n_rows x 11 doubles: class (-1 = hydrogen: exactly one row), variant, r, theta0 (degrees), x, D, Z, chi, V, U, K_inv;
 *   at most 32 rows, one per (class, variant), every class with its variant-0 row; a missing (class, variant) falls back to the
 *   class's variant-0 row (counted in n_fallback).  The host takes c0 = cos theta0 (-1 for 180), sqrt chi, sqrt D and ln n.
 * ENERGY.  (x.y = (x0 y0 + x1 y1) + x2 y2; every formula is evaluated as moldiff_amd/relax.py writes it.)
 *   BOND a-b: E = 1/2 k (r - r_ab)^2; r_ab = (ri + rj) - 0.1332 (ri + rj) ln n - ri rj (sqrt chi_i - sqrt chi_j)^2 / (chi_i ri + chi_j rj),
 *     k = 664.12 Zi Zj / r_ab^3, the lower atom index first.
 *   ANGLE i-j-k (i < k in the row of j), c = cos theta: K = 664.12 Zi Zk / r_ik^5 [3 r_ij r_jk (1 - c0^2) - r_ik^2 c0] with
 *     r_ik^2 = r_ij^2 + r_jk^2 - 2 r_ij r_jk c0 and c0 of the centre's row.  Centre LINEAR or c0 = -1: E = K (1 + c); TRIGONAL or
 *     RESONANT: E = K/9 (1 - (4 c^3 - 3 c)); else E = K (C0 + C1 c + C2 (2 c^2 - 1)), C2 = 1 / (4 (1 - c0^2)), C1 = -4 C2 c0,
 *     C0 = C2 (2 c0^2 + 1).
 *   TORSION about a bond j-k whose ends both have >= 2 neighbours and are not LINEAR; every quadruple i-j-k-l with i != l contributes
 *     with Vq = V / ((deg j - 1)(deg k - 1)); c = A.B / (|A||B|), A = (xi - xj) X (xj - xk), B = (xl - xk) X (xj - xk); skipped when
 *     |A| or |B| < deg_tol.  Neither end planar (TRIGONAL, RESONANT): 1/2 Vq (1 + (4 c^3 - 3 c)), V = sqrt(Vj Vk); both planar:
 *     1/2 Vq (1 - (2 c^2 - 1)), V = 5 sqrt(Uj Uk) (1 + 4.18 ln n); mixed: 1/2 Vq (1 - (32 c^6 - 48 c^4 + 18 c^2 - 1)), V = 1.
 *   INVERSION at a TRIGONAL or RESONANT centre j with exactly three neighbours and K_inv > 0 (shipped: C and N, 6): for each apex l of
 *     the three, the others i < k: E = (K_inv / 3)(1 - sqrt(1 - y^2)), y the cosine between xl - xj and (xi - xj) X (xk - xj); skipped
 *     when that normal is shorter than deg_tol or the apex lies on the centre.
 *   VAN DER WAALS, every pair a < b that is neither bonded nor shares a neighbour, no cutoff: E = D (q^12 - 2 q^6), q^2 = xa xb / r^2,
 *     D = sqrt Da sqrt Db.
 *   ACCUMULATION.  Thread a gathers the gradient on atom a in this order, rows ascending by neighbour: its bonds; the angles centred
 *     on it (q1 < q2); the angles it ends (its neighbour j, j's other neighbours k); the torsions about its bonds (k, then i, then l);
 *     the torsions it ends (j, k, l); the inversions centred on it (apex = neighbour 0, 1, 2); those of its neighbours; the pairs
 *     b = 0 .. n_all - 1.  A term's energy is added once, by the lower atom of a bond or pair, the centre of an angle or inversion,
 *     the lower central atom of a torsion, in the same walk.  Every sum over atoms (the five components, every dot product) is the
 *     per-thread value, a xor butterfly (32, 16, .. 1) in each wave of 64, then ((w0 + w1) + w2) + w3; total = (((bond + angle) +
 *     torsion) + inversion) + vdw.  No floating-point atomics: every output is bit-reproducible and independent of the batch.
 * MINIMISER.  L-BFGS, history 8.  Loop: rms = sqrt(g.g / (3 n_all)); rms <= gtol: stop CONVERGED; iterations = max_iters: stop
 *   MAXITER.  Direction: -g without history, else the two-loop recursion (alpha_i = s_i.q / s_i.y_i, newest first; r = (s.y / y.y of
 *   the newest) q; r += (alpha_i - y_i.r / s_i.y_i) s_i, oldest first; d = -r); g.d >= 0 drops the history, d = -g.  Step cap: with
 *   big = the largest |d_a|, big > max_step scales d by max_step / big.  Line search: t = 1, 1/2, .. at most 20 trials, accept when
 *   E(x + t d) is finite and <= E + (1e-4 t) g.d.  Exhausted: with a history, drop it and search once more along -g; else stop
 *   LINESEARCH.  Accepted: s = x_new - x, y = g_new - g are stored when s.y > 1e-10 sqrt(s.s y.y).  max_iters = 0 is a plain
 *   energy / gradient evaluation.  A starting energy or g.g that is not finite: status NONFINITE.
 *   Only the starting g.g is tested for finiteness.  A later accepted point has a finite energy; should its gradient not be finite, no
 *   comparison with it holds any more (rms <= gtol, g.d < 0 and every acceptance test are false with a NaN), the largest |d_a| is taken
 *   with fmax, which drops a NaN, and the run ends LINESEARCH at that point, the same on the device and in the restatement.
 * OUTPUTS (device, plain stores by the molecule's own workgroup):
 *   pos_out, grad_out [N_cap][3]; h_pos_out, h_grad_out [N_cap][4][3] float64: the relaxed point and the gradient there, hydrogen
 *     slots k >= h are 0.
 *   mol_stats [m][k], k < MDX_RELAX_STATS = 11 (int32): 0 status (0 relaxed, 1 TOO_LARGE, 2 NONFINITE; every other output of the
 *     molecule is 0 for 1 and 2)  1 stop reason (0 CONVERGED, 1 MAXITER, 2 LINESEARCH)  2 iterations  3 energy evaluations  4 n_all
 *     5 bonds  6 angles  7 torsion quadruples that contribute  8 inversion terms that contribute  9 pairs  10 atoms on a fall-back row
 *     (5 .. 9 at the starting point).
 *   mol_energy [m][k], k < MDX_RELAX_ENERGIES = 14 (float64): 0-4 bond, angle, torsion, inversion, vdw and 5 their total at the start;
 *     6-11 the same at the end; 12 the final rms gradient; 13 rmsd_heavy = sqrt(sum |x_a - x0_a|^2 / n) over the heavy atoms, unaligned.
 *   select, and a molecule reaching past N_cap / Eh_stride, as for mdx_mol_hydrogens.
 * ws: B x 16 x 768 doubles of device memory (the history; each thread touches its own atom's entries), ws_bytes its size.
 * One workgroup of 256 threads per molecule, about 53 KB of LDS.  MDX_ERR_ARG, every output untouched: a null operand (select
 * excepted), a negative size, a workspace too small, num_element outside 1 .. 32, num_bond_types outside 1 .. 16, a bad row (see
 * csrc/mdx_relax_args.h), deg_tol outside (0, 1), gtol outside (0, 1e6], max_step outside (0, 10], max_iters outside 0 .. 100000.
 * B = 0 is accepted and writes nothing. */
#define MDX_RELAX_STATS 11
#define MDX_RELAX_ENERGIES 14
int mdx_mol_relax(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                  const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                  const int32_t* select, const float* atom_pos, const int32_t* order, const double* h_pos, const int32_t* h_count,
                  const int32_t* atom_flag, int32_t num_element, int32_t num_bond_types, const double* ff_rows, int32_t n_rows,
                  double deg_tol, double gtol, double max_step, int32_t max_iters, double* pos_out, double* h_pos_out, double* grad_out,
                  double* h_grad_out, int32_t* mol_stats, double* mol_energy, double* ws, size_t ws_bytes, void* stream);

/* ---- Conformer generation: distance bounds of the all-atom molecule and coordinates embedded from them ---------------------
 * The reference's global_3d metric embeds n_conf conformers (EmbedMultipleConfs) between AddHs and UFFOptimizeMolecule.
 * mdx_mol_bounds + mdx_mol_embed are that stage: distance geometry with random starting coordinates, in the spirit of RDKit's
 * useRandomCoords embedding.  It is THIS PROJECT'S OWN MODEL: NOT ETKDG (no torsion preferences, no chiral-volume constraints, so a
 * conformer may be the MIRROR IMAGE at a stereocentre) and UNVERIFIED AGAINST RDKit; its lengths and angles come from the UNVERIFIED
 * rows of mdx_mol_relax.  A restatement (moldiff_amd/embed.py: bounds_ref, embed_ref) repeats every operation in the same order.
 * Angstrom; float64.
 *
 * mdx_mol_bounds.  INPUT: the compact layout, order, h_count, atom_flag, ff_rows exactly as for mdx_mol_relax (same molecule, same
 *   atom order, same typing, same rest lengths r_ab by relax_pair; no positions are read).  tol12, tol13, tol14 in [0, 1] Angstrom
 *   (conventions: 0.01, 0.04, 0.06) and vdw_scale in (0, 2] (convention 0.6); na_cap in 1 .. 256.
 *   THE INITIAL BOUNDS of a pair {a, d}, by the shortest bond path between them (a pair on several shortest paths takes the smallest
 *   lower and the largest upper bound of them; every path is evaluated from its lower end atom to its higher one; a lower bound below
 *   0 is 0):
 *     1-2: r_ab -+ tol12.
 *     1-3 a-b-d: l = sqrt((r1 r1 + r2 r2) - ((2 r1) r2) c), l -+ tol13, with c = cos theta0 of the centre b's row, or cos 60 / 90 /
 *       108 degrees when the angle a-b-d lies in a ring of 3 / 4 / 5 atoms (a, d bonded; else a and d share a neighbour other than b;
 *       else a neighbour x != b of a is bonded to a neighbour y != b of d): the shortest cycle through both bonds.  The host takes the
 *       cosines (cos(deg pi / 180), as c0).
 *     1-4 a-b-c-d: with c1, c2 the cosines at b and c as above, s = sqrt(1 - c c), dx = (r2 - r3 c2) - r1 c1: cis = sqrt(dx dx +
 *       (r3 s2 - r1 s1)^2), trans = sqrt(dx dx + (r3 s2 + r1 s1)^2); [cis - tol14, trans + tol14].  No planarity preference: a stated
 *       limitation, relaxation restores most of it.
 *     every other pair: lower = vdw_scale (0.5 (x_a + x_b)) from the rows' x, upper = 1000.  The diagonal is 0.
 *   SMOOTHING (Floyd-Warshall, k = 0 .. n_all - 1 outermost, a barrier per k): first U[i][j] = min(U[i][j], U[k][i] + U[k][j]), then with
 *   the final U: L[i][j] = max(max(L[i][j], L[k][i] - U[k][j]), L[k][j] - U[k][i]).  Sums and min / max only.  L > U for some pair
 *   afterwards: status INCONSISTENT.
 *   bounds_ws (device): B x 2 x na_cap^2 doubles, [m][0] the lower and [m][1] the upper bounds as full symmetric matrices of row stride
 *   na_cap (the lanes a of mdx_mol_embed read [b][a]: consecutive words), then B x na_cap^2 bytes, the class of every pair in the same
 *   layout (0 other or diagonal, 1 1-2, 2 1-3, 3 1-4): ws_bytes >= 17 B na_cap^2.  Entries past n_all are not written.
 *   mol_stats [m][k], k < MDX_BOUNDS_STATS = 7 (int32): 0 status (0 OK, 1 TOO_LARGE: n > 256, n_bonds > 512 or n_all > na_cap, 3
 *   INCONSISTENT)  1 n_all  2-4 the 1-2 / 1-3 / 1-4 pairs  5 angles i-j-k (i < k in the row of j) in a ring of 3, 4 or 5  6 pairs whose
 *   lower or upper bound smoothing changed.  A masked molecule or one past the arrays: all 0.  About 60 KB of LDS.
 *
 * mdx_mol_embed.  One workgroup of 256 threads per (molecule m, conformer c), thread a = atom a; h_count as above; bounds_ws, na_cap and
 *   bounds_stats (the mol_stats above) from mdx_mol_bounds on the same arrays; mol_ids (int64, B) or NULL for id = m.
 *   START (attempt t = 0, 1, ..): 4D coordinates uniform in [-L/2, L/2), L = 2 x the largest smoothed upper bound of the 1-2, 1-3 and
 *   1-4 pairs.  Philox4x32-10, key = the 64-bit seed (low, high word), counter = (2 a + j, c, id low word, (id >> 32) << 8 | t), j = 0:
 *   coordinates 0 and 1 from words (x, y) and (z, w), j = 1: coordinates 2 and 3.  Words (p, q) -> u = ((p >> 5) 2^26 + (q >> 6)) 2^-53,
 *   exactly; coordinate = (u - 0.5) L.  The seed is the key and the conformer, the id and the attempt are counter words: every (seed, id,
 *   conformer, attempt, atom) has its own block.  Only bits 0 .. 55 of an id enter the counter: ids that differ only above bit 55 share their numbers.
 *   mol_ids is device memory, which this entry does not read on the host: embed.embed_mols refuses an id outside 0 .. 2^56 - 1.
 *   ERROR.  d2 = (((dx dx + dy dy) + dz dz) + dw dw) of x_a - x_b; for every b = 0 .. n_all - 1 in order (the diagonal contributes
 *   nothing): d2 > ub^2: v = d2 / ub^2 - 1, e = v v, g_a += ((4 v) / ub^2)(x_a - x_b); d2 < lb^2: q = lb^2 + d2, v = (2 lb^2) / q - 1,
 *   e = v v, g_a += -(((8 lb^2) v) / (q q))(x_a - x_b); e is added by the lower atom; then e += w4 (x4 x4), g_a4 += (2 w4) x4.  Sums over
 *   atoms as in mdx_mol_relax (butterfly, then ((w0 + w1) + w2) + w3), dot products ((x x' + y y') + z z') + w w'.  No atomics.
 *   MINIMISER: the L-BFGS of mdx_mol_relax (history 8, step cap max_step, 20 Armijo halvings with 1e-4, curvature test 1e-10) over the
 *   4 n_all coordinates, rms = sqrt(g.g / (4 n_all)) <= gtol; the same code (csrc/mdx_lbfgs.h).  Stage A with w4 = 0.1 and stage B with
 *   w4 = 1.0 from A's end point, each with an empty history and at most max_iters iterations; then the fourth coordinate is dropped.
 *   ACCEPTANCE.  In 3D, d = sqrt((dx dx + dy dy) + dz dz): the largest of (d - ub) / ub for d > ub and (lb - d) / lb for d < lb over
 *   the 1-2 and 1-3 pairs and of (lb - d) / lb over the other pairs (1-4 pairs are not tested) must be <= viol_tol (convention 0.1);
 *   otherwise the next attempt, at most max_attempts; then status FAILED with the last attempt's numbers and coordinates.
 *   OUTPUTS: pos_out [c][N_cap][3], h_pos_out [c][N_cap][4][3] float64 in the layout of mdx_mol_relax's inputs with a leading conformer
 *   axis, hydrogen slots k >= h are 0 (mdx_mol_relax takes float32 heavy positions: the CALLER rounds them once);
 *   conf_stats [m][c][k], k < MDX_EMBED_STATS = 5 (int32): 0 status (0 OK, 1 TOO_LARGE, 2 NONFINITE: a starting error that is not finite,
 *   3 INCONSISTENT, 4 FAILED; for 1, 2, 3 every other output is 0)  1 attempts used  2, 3 iterations of A and B of the last attempt  4
 *   error evaluations over all attempts;  conf_values [m][c][k], k < MDX_EMBED_VALUES = 3 (float64): the final error of A, of B, the
 *   largest violation.  select and a molecule past the arrays as for mdx_mol_relax.
 *   hist: B x n_confs x 64 x na_cap doubles (the history), hist_bytes its size.
 * MDX_ERR_ARG, every output untouched: a null operand (select, mol_ids excepted), a negative size, a workspace too small, na_cap
 * outside 1 .. 256, a tolerance or vdw_scale outside its range, a bad row, n_confs outside 1 .. 65535, max_iters outside 0 .. 100000,
 * max_attempts outside 1 .. 64, gtol outside (0, 1e6], max_step outside (0, 10], viol_tol outside (0, 10].  B = 0 writes nothing. */
#define MDX_BOUNDS_STATS 7
#define MDX_EMBED_STATS 5
#define MDX_EMBED_VALUES 3
int mdx_mol_bounds(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                   const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                   const int32_t* select, const int32_t* order, const int32_t* h_count, const int32_t* atom_flag, int32_t num_element,
                   int32_t num_bond_types, const double* ff_rows, int32_t n_rows, double tol12, double tol13, double tol14, double vdw_scale,
                   int32_t na_cap, void* bounds_ws, size_t ws_bytes, int32_t* mol_stats, void* stream);
int mdx_mol_embed(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                  const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                  const int32_t* select, const int32_t* h_count, const int64_t* mol_ids, const void* bounds_ws, size_t ws_bytes, int32_t na_cap,
                  const int32_t* bounds_stats, int32_t n_confs, uint64_t seed, int32_t max_iters, int32_t max_attempts, double gtol,
                  double max_step, double viol_tol, double* pos_out, double* h_pos_out, int32_t* conf_stats, double* conf_values,
                  double* hist, size_t hist_bytes, void* stream);

/* ---- layer-level operators of the training path (next-row) ---------------------------------
 * The loss forward + backward of MolDiff.get_loss / BondPredictor.get_loss (models/model.py:128-201,
 * models/bond_predictor.py:84-124 + torch.autograd) is composed from these forward/backward pairs, one layer at a
 * time, by moldiff_amd/train_ops.py; activations stay in HBM between them.  All fp32, row-major, device pointers.
 *
 * sgemm_nt: C[M,N] (ldc) = A[M,K] (lda) * B[N,K]^T (ldb) + bias[N] + addend[M,N] (ldd) (bias / addend may be NULL; the
 *   addend carries the per-node part of a layer whose input is a concatenation).  nn.Linear forward (B = weight),
 *   its data gradient (B = weight^T) and, with splits > 1 and `partial` = splits*M*N floats, its weight gradient
 *   (A = dY^T, B = X^T, K = number of rows; partial sums are combined in a fixed order -> deterministic).
 * transpose: out[Cn,R] (ldo) = in[R,Cn]^T (ldi).
 * colreduce: out[N] = sum over M rows of X[M,N] (ld), times Y element-wise if Y != NULL (bias / LayerNorm parameter
 *   gradients); ws = ceil(M/512)*N floats. */
int mdx_op_sgemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, const float* addend, int64_t ldd,
                    float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int32_t splits, float* partial, void* stream);
/* sgemm_tn: dW[N,K] (ldw) = G[M,N]^T (ldg) * X[M,K] (ldx), the weight gradient straight from the stored row-major
 *   tensors; `splits` ranges of rows, partial = (splits + ceil(splits/256))*(N*K + N) floats, fixed-order two-stage
 *   reduction; db (may be NULL) receives the bias gradient = column sums of G from the same pass. */
int mdx_op_sgemm_tn(const float* G, int64_t ldg, const float* X, int64_t ldx, float* dW, int64_t ldw, float* db, int64_t M, int64_t N,
                    int64_t K, int32_t splits, float* partial, void* stream);
/* The same Linear on MANY rows (the edge rows of a training batch) with the row-owner decomposition of the sampling kernels:
 * Y (M,N) = X (M,K) W^T + bias + addend with W (N,K) [transW = 0], or X W with W (K,N) [transW = 1: the grad_input GEMM, no
 * separate transpose].  K % 16 == 0, K/16 in {1,2,4,5,8,16}, N % 4 == 0, N <= 256 (mdx_op_linear_rows_supported); rows 16-byte
 * aligned.  pack_ws: mdx_op_linear_rows_ws(N, K) bytes of scratch (the weight in streaming order, rebuilt per call). */
int mdx_op_linear_rows_supported(int64_t N, int64_t K);
size_t mdx_op_linear_rows_ws(int64_t N, int64_t K);
int mdx_op_linear_rows(const float* X, int64_t ldx, const float* W, int64_t ldw, int32_t transW, const float* bias, const float* addend,
                       int64_t ldd, float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, float* pack_ws, void* stream);
int mdx_op_transpose(const float* in, int64_t ldi, int64_t R, int64_t Cn, float* out, int64_t ldo, void* stream);
/* n contiguous row-major matrices transposed by one launch (every weight of a model once per optimisation step: the grad_input
 * GEMMs read W^T).  desc (device): 4 int64 per matrix {src pointer, dst pointer, R, C}; dst receives (C,R) contiguous.
 * max_tiles = the largest matrix's count of 32 x 32 tiles (sizes the launch). */
int mdx_op_transpose_batch(const int64_t* desc, int64_t n, int64_t max_tiles, void* stream);
int mdx_op_colreduce(const float* X, const float* Y, int64_t ld, int64_t M, int64_t N, float* out, float* ws, void* stream);
/* y = relu?(LayerNorm(x) * gamma + beta) over F <= 1024 features (nn.LayerNorm eps 1e-5, models/common.py MLP);
 * stats (M,2) receives (mean, rstd) for the backward.  Backward: dx (M,F), dgb (2F) = [dgamma | dbeta]; ws =
 * mdx_op_ln_relu_bwd_ws(M, F) bytes.  Entry points: mdx_op_ln_relu_fwd_t / mdx_op_ln_relu_bwd_t below. */
size_t mdx_op_ln_relu_bwd_ws(int64_t M, int32_t F);
/* The same backward when the layer after the LayerNorm is a Linear to ONE output (PosUpdate's inter MLP, 256 -> 1, reference
 * models/graph.py:388-392 through models/common.py:191-198): the upstream gradient dy[row][c] = f16(g1[row] * f16(w1[c])) is formed
 * in the kernel from g1 (M values; dt bit 0: float16) and the Linear's weight row w1 (F, fp32) -- autograd's `grad_input` GEMM with
 * K = 1, its weight transpose and the (M,F) gradient tensor are not materialised.  Leaves the [dgamma | dbeta] partial rows in ws
 * (mdx_op_ln_relu_bwd_rows(M) rows of 2F floats) for mdx_op_reduce_deferred.  F in {32, 64, 128, 256}; dt bit 1: x, bit 2: dx float16. */
int mdx_op_ln_relu_bwd_r1_t(const void* g1, const float* w1, const void* x, const float* stats, const float* gamma, const float* beta,
                            int64_t M, int32_t F, int32_t relu, void* dx, float* ws, int32_t dt, void* stream);
/* The element-wise, gather / segment-sum and product-with-gathered-row operators exist in their `_t` forms only (below):
 * ew: element-wise pairs, op: 0 a+b, 1 a-b, 2 a*b, 3 a*sigmoid(b).  Backward writes da / db (either may be NULL).
 * gather_rows / segsum_rows: y[i] = x[idx[i]] (rows of F floats) and its adjoint out[r] = sum_{j in [ptr[r],ptr[r+1])} src[order[j]]
 *   (torch_scatter.scatter_sum with `order` = stable argsort of the index; sequential per output -> deterministic).
 * mul_gather: y = a * t[idx] (product with a gathered per-node row, e.g. h_edge * h_node[col], models/graph.py:44) without the
 *   gathered (rows x F) intermediate; backward: da = g * t[idx], dt[r] = sum over the rows of segment r of g * a. */
/* rel = pos[l] - pos[r], dist = |rel| (models/graph.py:349-350); backward: g (E,3) = drel + ddist * rel / dist, the
 * caller scatters +g to l and -g to r.  drel / ddist may be NULL. */
int mdx_op_edge_geom_fwd(const float* pos, const int64_t* l, const int64_t* r, int64_t E, float* rel, float* dist, void* stream);
int mdx_op_edge_geom_bwd(const float* rel, const float* dist, const float* drel, const float* ddist, int64_t E, float* g, void* stream);
/* GaussianSmearing (models/common.py): out[e,k] = exp(coef[k] * (clamp(d[e], lo, hi) - off[k])^2) and d/dd. */
int mdx_op_smear_fwd(const float* d, const float* off, const float* coef, int32_t G, float lo, float hi, int64_t E, float* out,
                     void* stream);
int mdx_op_smear_bwd(const float* d, const float* off, const float* coef, int32_t G, float lo, float hi, int64_t E, const float* gout,
                     float* gd, void* stream);
/* PosUpdate force (models/graph.py:393): out[e] = w[e] * rel[e] / d[e] / (d[e] + 1) and its three gradients. */
int mdx_op_force_fwd(const float* w, const float* rel, const float* d, int64_t E, float* out, void* stream);
int mdx_op_force_bwd(const float* w, const float* rel, const float* d, const float* g, int64_t E, float* gw, float* grel, float* gd,
                     void* stream);

/* Optimizer step on flat buffers (torch.optim.AdamW + torch.nn.utils.clip_grad_norm_, reference utils/train.py:64-70,
 * scripts/train_drug3d.py:107-108).  sumsq: out[0] = sum x^2 (fixed-order two-stage; ws = 1024 floats).  adamw: one
 * decoupled-weight-decay Adam step, step = 1, 2, ...; when gnorm2 != NULL the gradient is scaled by
 * min(max_norm / (sqrt(*gnorm2) + 1e-6), 1) on the fly. */
int mdx_op_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream);
int mdx_op_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int64_t step, const float* gnorm2, float max_norm, void* stream);

/* Mixed-precision forms of mdx_op_sgemm_nt / mdx_op_sgemm_tn (the reference trains under torch.autocast(dtype=float16) + GradScaler,
 * scripts/train_drug3d.py:86-109): operands rounded to half_kind (1 = bfloat16, 2 = float16) on their way into LDS, half MFMAs,
 * fp32 accumulation; round_out != 0 rounds the result to the same type before it is stored in its fp32 container -- the value a
 * Linear (and the gradient of a weight autocast cast to half) has there; float16 overflows to +-inf beyond 65504.
 * mdx_op_ew_fwd_t: op | (kind << 8) and mdx_op_mul_gather_fwd_t: F | (kind << 16) round their products the same way.
 * Entry points: mdx_op_xgemm_nt_t / mdx_op_xgemm_tn_t below. */

/* Half storage (round 3): the `_t` forms of the training operators take `dt`, a bit mask of the tensors that are stored as float16
 * instead of fp32 (element strides and feature counts are unchanged).  In the mixed-precision mode every Linear / LayerNorm / product
 * result is a float16 VALUE; keeping it in a float16 container halves the HBM traffic these memory-bound operators are limited by.
 * Bits, in argument order -- xgemm_nt_t: 0 A, 1 addend, 2 C (needs half_kind 2);  xgemm_tn_t: 0 G, 1 X (dW, db stay fp32);
 * ln_relu_fwd_t: 0 x, 1 y;  ln_relu_bwd_t: 0 dy, 1 x, 2 dx;  ew_fwd_t: 0 a, 1 b, 2 out;  ew_bwd_t: 0 a, 1 b, 2 g, 3 da, 4 db;
 * gather_rows_t: 0 x, 1 y;  segsum_rows_t: 0 src, 1 out;  mul_gather_fwd_t: 0 a, 1 t, 2 y;  mul_gather_bwd_t: 0 g, 1 a, 2 t, 3 da, 4 dt.
 * dt = 0 is the fp32 operator (these operators have no other entry point).  Half storage needs feature counts that are multiples of 4. */
int mdx_op_xgemm_nt_t(const void* A, int64_t lda, const float* B, int64_t ldb, const float* bias, const void* addend, int64_t ldd,
                      void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int32_t half_kind, int32_t round_out, int32_t dt, void* stream);
int mdx_op_xgemm_tn_t(const void* G, int64_t ldg, const void* X, int64_t ldx, float* dW, int64_t ldw, float* db, int64_t M, int64_t N,
                      int64_t K, int32_t splits, float* partial, int32_t half_kind, int32_t round_out, int32_t dt, void* stream);
/* Linear + LayerNorm(+ReLU) in ONE launch (common.MLP's first two layers, reference models/common.py:191-196; replaces
 * F.linear + F.layer_norm + F.relu there): C = the Linear's result exactly as mdx_op_xgemm_nt_t stores it (the backward needs it),
 * post (M,N; row stride ldp) = relu(LN(C)), stats (M,2) = mean, rstd -- mdx_op_ln_relu_fwd_t's formula on C in another summation order
 * (equal to rounding, not bit for bit) and what mdx_op_ln_relu_bwd_t reads.  A float16 C requires round_out = 1.  dt bits: 0 A, 1 addend, 2 C, 3 post.  Built for float16 rows on the row-owner kernel only (A float16,
 * M >= 1024, K in {32, 64, 128, 256}, N in {32, 64, 128, 256}: mdx_op_xgemm_nt_ln_supported); anything else returns
 * MDX_ERR_UNSUPPORTED and the caller runs the two operators. */
int mdx_op_xgemm_nt_ln_supported(int64_t M, int64_t N, int64_t K);
int mdx_op_xgemm_nt_ln_t(const void* A, int64_t lda, const float* B, int64_t ldb, const float* bias, const void* addend, int64_t ldd,
                         void* C, int64_t ldc, const float* gamma, const float* beta, void* post, int64_t ldp, float* stats, int32_t relu,
                         int64_t M, int64_t N, int64_t K, int32_t half_kind, int32_t round_out, int32_t dt, void* stream);
int mdx_op_ln_relu_fwd_t(const void* x, const float* gamma, const float* beta, int64_t M, int32_t F, int32_t relu, void* y, float* stats,
                         int32_t dt, void* stream);
int mdx_op_ln_relu_bwd_t(const void* dy, const void* x, const float* stats, const float* gamma, const float* beta, int64_t M, int32_t F,
                         int32_t relu, void* dx, float* dgb, float* ws, int32_t dt, void* stream);
int mdx_op_ew_fwd_t(int32_t op, const void* a, const void* b, void* out, int64_t n, int32_t dt, void* stream);
/* out = srcs[0] + ... + srcs[k-1] (k <= 12 tensors of n elements, half[j] != 0: float16 container), summed in fp32 in argument order,
 * stored once: the gradient of a tensor with several consumers in one launch (torch.autograd accumulates them pairwise). */
/* Segment order of the right end points from that of the left ones for a directed edge list [half-edges ; flipped half-edges]
 * (models/model.py:269): order_left = stable argsort of left (E = 2 Eh), ptr (R + 1) its segment starts (shared by both index vectors);
 * order_right receives the stable argsort of right.  Replaces a second sort per training step. */
int mdx_op_plan_flip(const int64_t* order_left, const int64_t* ptr, int64_t R, int64_t Eh, int64_t* order_right, void* stream);
int mdx_op_sum_n(const void* const* srcs, const int32_t* half, int32_t k, int64_t n, void* out, int32_t out_half, void* stream);
int mdx_op_ew_bwd_t(int32_t op, const void* a, const void* b, const void* g, void* da, void* db, int64_t n, int32_t dt, void* stream);
int mdx_op_gather_rows_t(const void* x, const int64_t* idx, int64_t M, int32_t F, void* y, int32_t dt, void* stream);
/* (segsum_rows_t: dt bit 0 / 1 = src / out float16; bit 2 = the caller accepts a summation order other than the sequential CSR order -- fp32
 * rows are then dealt to four threads per element like float16 rows always are; without it fp32 sums keep the order of torch's index_add) */
int mdx_op_segsum_rows_t(const void* src, const int64_t* order, const int64_t* ptr, int64_t R, int32_t F, void* out, int32_t dt,
                         void* stream);
int mdx_op_mul_gather_fwd_t(const void* a, const void* t, const int64_t* idx, int64_t M, int32_t F, void* y, int32_t dt, void* stream);
int mdx_op_mul_gather_bwd_t(const void* g, const void* a, const void* t, const int64_t* idx, const int64_t* order, const int64_t* ptr,
                            int64_t M, int64_t R, int32_t F, void* da, void* dtab, int32_t dt, void* stream);

/* Deferred gradient reduction: mdx_op_sgemm_tn / mdx_op_xgemm_tn_t with dW == NULL (db != NULL still requests the bias partials)
 * and mdx_op_ln_relu_bwd_t with dgb == NULL leave their split partials in the caller's buffer (layout: mdx_op_wgrad_layout -> number
 * of partials S and the float offset of the [S][N] bias partials; LayerNorm: mdx_op_ln_relu_bwd_rows(M) rows of 2F floats in ws).
 * mdx_op_reduce_deferred sums every record of a device table in ONE launch and ADDS it to its destination (a parameter's slot in a flat
 * gradient buffer): record = 8 x int64 {P, dst, S, rows, cols, ld, pstride, rkind | chunked << 6 | store << 7 | first_block << 8};
 * total_blocks = sum of ceil(rows * cols / 128) (x ceil(S / 256) for a chunked record; first_block counts the same blocks).  A record
 * with S > 256 is given as `chunked`: the launch stores the sum of every 256 partials in the scratch planes behind them
 * (P + (S + c) * pstride, which mdx_op_wgrad_layout / mdx_op_ln_relu_bwd_ws reserve), and the caller sums those ceil(S / 256) planes
 * with a plain record {P + S * pstride, dst, ceil(S / 256), ...} in a second call.  Same fixed summation order as the per-layer reduction kernels. */
int mdx_op_wgrad_layout(int64_t M, int64_t N, int64_t K, int32_t splits, int32_t half, int64_t* S, int64_t* bias_off);
int64_t mdx_op_ln_relu_bwd_rows(int64_t M);
int mdx_op_reduce_deferred(const int64_t* desc, int32_t n, int64_t total_blocks, void* stream);

/* Queued (grouped) weight gradients, float16 autocast mode.  A step's weight-gradient contractions dW = dY^T X (the backward of every
 * nn.Linear of reference models/common.py:181-201 and models/graph.py, i.e. torch.autograd's mm_backward for the weight) feed nothing
 * before the optimizer, so the host may queue them and run a whole table per launch.  mdx_op_wgrad_plan: tile class and layout of one
 * contraction -- out[0..7] = kind (0..3 transpose-read kernel with tiles 128x128 / 128x64 / 64x128 / 64x64 (n x k), 4 converting kernel,
 * 5 / 6 the transpose-read kernel with 32x64 / 64x32 tiles, 7 a scaled column sum for N == 1 or K == 1),
 * gx, gy (tiles along K, N), S (row ranges), mper (rows per range), float offset of the [S][N] bias partials, floats of the whole partial
 * area (the layout of mdx_op_xgemm_tn_t / mdx_op_wgrad_layout), blocks.  dt bit 0 / 1: dY / X stored as float16; `aligned`: both start on
 * 16 bytes.  mdx_op_wgrad_grouped: one launch over a DEVICE table of n records of one kind -- 16 x int64 {dY, X, P, Pb (0 = no bias
 * partials), ldg, ldx, M, N, K, mper, gx, gy, S, dt, first_block, 0}, first_block = running sum of the records' blocks,
 * total_blocks = their sum; every record's partials are bit-identical to mdx_op_xgemm_tn_t(dW = NULL) with the same row ranges and are
 * summed by mdx_op_reduce_deferred. */
int mdx_op_wgrad_plan(int64_t M, int64_t N, int64_t K, int32_t splits, int32_t dt, int64_t ldg, int64_t ldx, int32_t aligned, int64_t* out);
int mdx_op_wgrad_grouped(const int64_t* desc, int32_t n, int64_t total_blocks, int32_t kind, void* stream);

/* ---- fused row-owner training operators (round 6; csrc/mdx_train_fused.hip) ---------------------------------------------------------
 * One forward and one backward launch for a whole BondFFN of the EdgeBlock in the float16 autocast arithmetic
 * (replaces, for training, reference models/graph.py:133-141 -- bond_linear, the product with node_linear(h)[idx], the inter MLP
 * models/common.py:191-198, the gate MLP on [bond | node | time] and the sigmoid product -- as called from models/graph.py:272-279,
 * plus torch.autograd's backward through them).  Widths are those of the shipped networks: bond 64, inter 128, out 64, gate hidden 32.
 * Row tensors are float16, row-major and dense unless a stride is given; weights are fp32 (N outputs x K inputs, row stride ld*, so
 * column slices of a wider matrix are passed as they are); Wt is the gate's time COLUMN (element j at Wt[j * ldwt]).
 * NL = node_linear(h_node) (N,128) float16 and GN = the node columns of the gate's first Linear applied to h_node (N,32) fp32 are
 * computed per NODE by the caller (Linear(h[idx]) == Linear(h)[idx]); idx (E) selects the node whose features enter each row.
 * Forward writes what the backward and the weight gradients read: prod (E,128), pre1 / post1 (E,128: before / after LayerNorm+ReLU
 * of the inter MLP), inter (E,64), gpre / gpost (E,32), gate (E,64), out = inter * sigmoid(gate) (E,64). */
typedef struct {
  const void* X; int64_t ldx;                                            /* (E,64) float16, rows 16-byte aligned */
  const float* Wb; int64_t ldwb;                                         /* bond_linear.weight (128,64) */
  const float* Wi1; int64_t ldwi1; const float* bi1; const float* g1; const float* be1;   /* inter_module.net.0 (128,128) + bias, .1 LayerNorm(128) */
  const float* Wi2; int64_t ldwi2; const float* bi2;                      /* inter_module.net.3 (64,128) + bias */
  const float* Wg1; int64_t ldwg1; const float* bg1; const float* gg; const float* gbe;  /* gate.net.0 bond columns (32,64) + bias, .1 LayerNorm(32) */
  const float* Wt; int64_t ldwt;                                         /* gate.net.0 time column (32) */
  const float* Wg2; int64_t ldwg2; const float* bg2;                      /* gate.net.3 (64,32) + bias */
  const void* NL; int64_t ldnl;                                          /* (N,128) float16 */
  const float* GN; int64_t ldgn;                                         /* (N,32) fp32 */
  const int64_t* idx;                                                    /* (E) */
  const float* te;                                                       /* (E) the time input (already t / T) */
  void *prod, *pre1, *post1, *inter, *gpre, *gpost, *gate, *out;         /* float16 outputs (inputs of the backward) */
  int64_t E;
} mdx_bondffn_args;
/* Backward: gS (N,64; fp32, row stride ldgs) = dL/d scatter_sum(out, oidx); row e takes gS[oidx[e]] rounded to float16 (the gather the
 * per-operator path's scatter_sum backward performs).  Writes the float16 row gradients the weight-gradient contractions read
 * -- g_inter, g_gate (E,64), g_pre1, g_bf (E,128), g_gpre (E,32) -- plus g_x = dL/dX (E,64) and g_nl (E,128) = the per-edge dL/dNL rows
 * (the caller sums them per node with mdx_op_segsum_rows_t; dL/dGN is the same sum of g_gpre).  lnp: mdx_op_bondffn_workgroups() rows
 * of mdx_op_bondffn_lnp_floats() = 320 floats [d gamma1 | d beta1 (128 each) | d gamma_g | d beta_g (32 each)], one per workgroup,
 * to be summed by the caller (mdx_op_reduce_deferred record: S = workgroups, pstride = 320). */
typedef struct {
  mdx_bondffn_args f;
  const float* gS; int64_t ldgs;
  const int64_t* oidx;
  void *g_inter, *g_gate, *g_pre1, *g_bf, *g_nl, *g_gpre, *g_x;
  float* lnp;
} mdx_bondffn_bwd_args;
/* EdgeBlock tail + residual in one launch (replaces, for training, reference models/graph.py:281-294 and the `h_edge + ...` of :360):
 * out = H + out_transform(relu(LN(self_ffn(H) + BL[il] + BR[ir]))), BL / BR (N,64) float16 = the per-node sums S_L + node_ffn_left(h),
 * S_R + node_ffn_right(h).  pre / post (E,64): the LayerNorm's input / relu(output), kept for the backward and out_transform's weight
 * gradient.  Backward: g_out (E,64) float16 -> g_pre (E,64) = dL/d pre (self_ffn's weight gradient operand; summed per node by il / ir it
 * is dL/dBL / dL/dBR), g_h = g_out + self_ffn^T g_pre, lnp: mdx_op_bondffn_workgroups() rows of 128 floats [d gamma | d beta]. */
typedef struct {
  const void* H; int64_t ldh;
  const void* BL; int64_t ldbl; const void* BR; int64_t ldbr;
  const int64_t* il; const int64_t* ir;
  const float* Ws; int64_t ldws; const float* bs; const float* lng; const float* lnb;
  const float* Wo; int64_t ldwo; const float* bo;
  void *pre, *post, *out;
  int64_t E;
} mdx_edge_tail_args;
typedef struct {
  mdx_edge_tail_args f;
  const void* g_out; int64_t ldg;
  void *g_pre, *g_h;
  float* lnp;
} mdx_edge_tail_bwd_args;
/* PosUpdate, front of its BondFFN (replaces, for training, reference models/graph.py:388-390 with :133-141 up to the inter MLP's input):
 * a = LF[il] * RF[ir] (LF / RF (N,64) float16 = left_lin_edge(h), right_lin_edge(h), hoisted), prod = bond_linear(X) * node_linear(a)
 * (E,256), gate = gate MLP on [X | a | t] (E,1).  Weights: Wb, Wn (256,64); Wg1x, Wg1a (32,64) and Wt (32) = the bond / node / time
 * columns of gate.net.0; Wg2 (32) / bg2 (1) = gate.net.3.  Outputs (float16): a (E,64), prod (E,256), gpre / gpost (E,32), gate (E).
 * Backward: g_prod (E,256; row stride ldgp), g_gate (E) -> g_bf, g_nf (E,256) = dL/d bond_linear(X), dL/d node_linear(a); g_gpre (E,32);
 * g_x (E,64) = dL/dX; g_lf, g_rf (E,64) = the per-edge dL/dLF[il], dL/dRF[ir] rows (summed per node by the caller); lnp:
 * mdx_op_bondffn_workgroups() rows of 64 floats [d gamma | d beta] of the gate's LayerNorm. */
typedef struct {
  const void* X; int64_t ldx;
  const void* LF; int64_t ldlf; const void* RF; int64_t ldrf;
  const int64_t* il; const int64_t* ir;
  const float* te;
  const float* Wb; int64_t ldwb; const float* Wn; int64_t ldwn;
  const float* Wg1x; int64_t ldwg1x; const float* Wg1a; int64_t ldwg1a; const float* Wt; int64_t ldwt;
  const float* bg1; const float* gg; const float* gbe;
  const float* Wg2; const float* bg2;
  void *a, *prod, *gpre, *gpost, *gate;
  int64_t E;
} mdx_posffn_args;
typedef struct {
  mdx_posffn_args f;
  const void* g_prod; int64_t ldgp;
  const void* g_gate;
  void *g_bf, *g_nf, *g_gpre, *g_x, *g_lf, *g_rf;
  float* lnp;
} mdx_posffn_bwd_args;
/* NodeBlock message path in one forward and one backward launch (replaces, for training, reference models/graph.py:40-48: edge_net,
 * the product with node_net(x)[col], msg_net, the gate MLP and the sigmoid product; the scatter_sum of :50 stays the caller's).
 * Weights arrive as float16 A-operand packs written by mdx_op_pack_a (one launch for up to 10 matrices): job = {W (fp32, row stride ld),
 * n_out, n_in, perm (1: the layer's input is the previous layer's accumulators), trans (1: pack W^T), out (n_out * n_in halves)}.
 * Forward packs: W1e (256 x 64, perm 0), W2e, Wm (256 x 256, perm 1), Wg1 (the gate's edge columns, 256 x 64, perm 0), Wg2 (256 x 256,
 * perm 1); backward packs (trans 1, perm 1): Wg2^T, Wm^T, W2e^T (256 x 256), Wg1^T, W1e^T (64 x 256).
 * HN = node_net(x) (N,256) float16, PN = the gate's node + time columns applied per node (N,256) fp32, col (E) = right end point.
 * Forward outputs, (E,256) float16 each: he_pre / he_post (edge_net's LayerNorm input / relu(output)), he, p = he * HN[col], m0 =
 * msg_net(p), g_pre / g_post (gate LayerNorm), gt, msg = m0 * sigmoid(gt).  Backward: gA (N,256 fp32) = dL/d scatter_sum(msg, row);
 * writes g_m0, g_gt, g_gpre, g_he, g_pre (weight-gradient operands), g_hne = per-edge dL/dHN[col], g_x (E,64) and
 * mdx_op_bondffn_workgroups() partial rows of 1024 floats [d gamma_e | d beta_e | d gamma_g | d beta_g]. */
typedef struct { const float* W; int64_t ld; int32_t n_out, n_in, perm, trans; void* out; } mdx_pack_job;
typedef struct { mdx_pack_job job[10]; int32_t n; } mdx_pack_jobs;
typedef struct {
  const void* X; int64_t ldx;
  const void* HN; int64_t ldhn;
  const float* PN; int64_t ldpn;
  const int64_t* col;
  const void *pk_w1e, *pk_w2e, *pk_wm, *pk_wg1, *pk_wg2;
  const float *b1e, *lng_e, *lnb_e, *b2e, *bm, *bg1, *lng_g, *lnb_g, *bg2;
  void *he_pre, *he_post, *he, *p, *m0, *g_pre, *g_post, *gt, *msg;
  int64_t E;
} mdx_nodemsg_args;
typedef struct {
  mdx_nodemsg_args f;
  const float* gA; int64_t ldga;
  const int64_t* row;
  const void *pk_wg2t, *pk_wg1t, *pk_wmt, *pk_w2et, *pk_w1et;
  void *g_m0, *g_gt, *g_gpre, *g_hne, *g_he, *g_pre, *g_x;
  float* lnp;
} mdx_nodemsg_bwd_args;
int mdx_op_pack_a(const mdx_pack_jobs* jobs, void* stream);
int mdx_op_nodemsg_fwd(const mdx_nodemsg_args* a, void* stream);
int mdx_op_nodemsg_bwd(const mdx_nodemsg_bwd_args* a, void* stream);
int mdx_op_nodemsg_lnp_floats(void);
int mdx_op_posffn_fwd(const mdx_posffn_args* a, void* stream);
int mdx_op_posffn_bwd(const mdx_posffn_bwd_args* a, void* stream);
int mdx_op_posffn_lnp_floats(void);
int mdx_op_edge_tail_fwd(const mdx_edge_tail_args* a, void* stream);
int mdx_op_edge_tail_bwd(const mdx_edge_tail_bwd_args* a, void* stream);
int mdx_op_edge_tail_lnp_floats(void);
int mdx_op_bondffn_fwd(const mdx_bondffn_args* a, void* stream);
int mdx_op_bondffn_bwd(const mdx_bondffn_bwd_args* a, void* stream);
int mdx_op_bondffn_workgroups(void);
int mdx_op_bondffn_lnp_floats(void);

/* One optimisation step with torch.cuda.amp.GradScaler semantics and ALL of its state on the device (no host round trip):
 * g = gradient of (S x loss).  state (16 floats): [0] loss scale S, [1] growth tracker, [2] optimizer steps taken, [3] steps skipped,
 * [4] unscaled squared gradient norm of this step (inf / nan if a gradient overflowed); [5..8] internal.  Finite: clip to max_norm
 * (<= 0: none), AdamW with t = ++state[2]; after growth_interval consecutive finite steps S *= growth.  Not finite: no update, the
 * step count does not advance, S *= backoff.  S = growth = backoff = 1 is the plain fp32 step.  ws: 1024 floats. */
int mdx_op_amp_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, float max_norm, float* state, float growth, float backoff, int32_t growth_interval, float* ws,
                     void* stream);

/* ---- measurement hooks (bench.py): hipEvent timing of the block kernels on their launch stream.
 * kernel: 0 = fused edge kernel A (MFMA), 1 = fused edge kernel B, 2 = node kernel, 3 = message aggregation
 * (segment sum (E,256)->(N,256), the HBM-bound scatter/gather pass), 4 = the guidance backward's fused edge kernel
 * (edge_bwd2_kernel, MFMA).  enable(0) = off, enable(1) = every kernel, enable(m > 1) = kernel k iff bit (k+1) of m is set
 * (an event pair costs ~3.4 us of stream time, 25 pairs per step: bench.py times only the roofline kernel inside its timed
 * region).  read() drains pending events. */
int mdx_profile_enable(int32_t on);
int mdx_profile_read(int32_t kernel, int64_t* count, double* total_ms);
/* the kernel function name slot `kernel` brackets in this build ("" for an unknown slot); static storage */
const char* mdx_profile_kernel_name(int32_t kernel);

#ifdef __cplusplus
}
#endif
#endif /* MOLDIFF_HIP_H */
