// Weight blocks of the kernels: pointers into the packed weight arena, filled by the host packer (mdx_pack.cpp) and carried by value in
// the kernels' argument blocks (mdx_kernels.h).  Plain C++, no HIP types: the packer and tools/pack_host_check.cpp compile this header
// with the host compiler alone.
#pragma once

#define MDX_ND 256  // node feature width (shipped configs; other widths are rejected at create)
#define MDX_ED 64   // edge feature width
#define MDX_NG 16   // distance gaussians

// Column layout of the per-node table NT (N, MDX_NTW) written by the node kernel (PRE stage) and
// gathered by the edge kernels:  everything that is Linear(h_node)[idx] in the reference is hoisted
// to one per-node GEMM (exact for a plain Linear; for the first layer of the gate MLPs it splits the
// 321-wide contraction into edge + node + time parts, see DESIGN.md "hoisting").
#define MDX_NT_C 0       // centroid_lin(x) + bias                         (256)
#define MDX_NT_GX 256    // gate.net.0.weight[:, 64:320] x   (no bias)      (256)
#define MDX_NT_NLL 512   // bond_ffn_left.node_linear x                     (128)
#define MDX_NT_NLR 640   // bond_ffn_right.node_linear x                    (128)
#define MDX_NT_NFL 768   // node_ffn_left(x) + bias                         (64)
#define MDX_NT_NFR 832   // node_ffn_right(x) + bias                        (64)
#define MDX_NT_GXL 896   // bond_ffn_left.gate.net.0.weight[:, 64:320] x    (32)
#define MDX_NT_GXR 928   // bond_ffn_right.gate.net.0.weight[:, 64:320] x   (32)
#define MDX_NTW 960

struct MlpW {  // Linear -> LN -> ReLU -> Linear, all packed for gemm_tile (node kernel, decoders)
  const float *W1, *b1, *g, *be, *W2, *b2;
};
struct MlpV {  // the vectors of such an MLP in the edge kernels, which read its two matrices from their stream packs
  const float *b1, *g, *be, *b2;
};

struct FfnW {  // BondFFN of the EdgeBlock (bond 64, node 256 hoisted, inter 128, gate hidden 32, out 64): vectors; matrices in FfnS
  MlpV inter;                          // 128 -> 128 -> 64
  const float *bg1, *wtg1, *gg, *gb;   // gate first layer: bias, time column, LN
  const float* bg2;                    // gate second layer
};

// "stream packs" of the row-owner kernels (mdx_row.h, mdx_edge2.hip): the matrices in consumption order
struct FfnS {
  const float *Wbl, *Wg1e, *W1, *W2, *Wg2;  // bond_linear (128 x 64), gate edge part (32 x 64), inter (128 x 128, 64 x 128), gate (64 x 32)
};
struct EdgeAS {
  // edge_embs (64 x 80), NodeBlock gate: edge part (256 x 64) and second layer (256 x 256), edge_net 64 -> 256 -> 256, msg_net (256 x 256)
  const float *Wemb, *Wg1e, *Wg2, *W1, *W2, *Wm;
  FfnS ffn[2];
};
struct EdgeBS {
  // EdgeBlock tail (64 x 64 each); PosUpdate.edge_lin: bond / node linear (256 x 64 each), gate first layer split into its He part and
  // its a part (32 x 64 each), inter_module first layer (256 x 256)
  const float *Wself, *Wout, *Wbl, *Wnl, *Wg1h, *Wg1a, *Wi1;
};

struct EdgeAW {  // weights of edge kernel A for one block
  const float* bemb;                          // edge_embs bias
  const float *bg1, *wtg1, *gg, *gb, *bg2;    // NodeBlock gate: bias, time col, LN, second bias
  MlpV en;                                    // edge_net 64 -> 256 -> 256
  const float* bm;                            // msg_net bias
  FfnW ffn[2];                                // left, right
  EdgeAS s;
  EdgeAS ss;  // the same streams split into float16 hi / lo halves (mdx_split.h; EA_SPLIT launches)
  // 1: every Linear that feeds a LayerNorm in this kernel (both gates' and edge_net's / inter's first layers, with their biases, time
  // columns and the GX / GXL / GXR rows of the node table) was packed centred over its output features (mdx_pack.cpp Layer::centred)
  int lnc;
};

struct EdgeBW {  // weights of edge kernel B for one block
  const float *bself, *lng, *lnb, *bout;  // EdgeBlock tail
  // PosUpdate.edge_lin (BondFFN bond 64, node 64, inter 256, out 1)
  const float *bi1, *ig, *ib;      // inter_module first layer: bias + LN
  const float* wi2;                // (256) second layer row
  float bi2;
  const float *bg1, *wtg1, *gg, *gb;  // gate first layer: bias, time col, LN
  const float* wg2;                // (32)
  float bg2;
  EdgeBS s;
  EdgeBS ss;  // split float16 streams (EB_SPLIT launches)
  int lnc;    // 1: the PosUpdate gate's and inter module's first layers were packed centred (see EdgeAW)
};

struct NodeW {  // weights of the node kernel
  // MID stage (block i): NodeBlock tail + PosUpdate per-node MLPs
  const float *lng, *lnb, *Wout, *bout;
  MlpW left, right;  // 256 -> 64 -> 64
  // PRE stage (block i or i+1)
  MlpW nn;                     // node_net 256 -> 256 -> 256
  const float *Wcat, *bcat;    // concatenated (960 x 256) + bias (960, zeros where the reference has none)
};

struct NodeWS {  // the node kernel's matrices as dense split float16 packs (mdx_node_s.hip; mdx_pack.cpp DENSE_SPLIT)
  const float *Wout, *leftW1, *leftW2, *rightW1, *rightW2;  // MID stage
  const float *nnW1, *nnW2, *Wcat;                          // PRE stage
};

// ---- backward (bond-predictor guidance gradient; dgrad only, no weight gradients): transposed packs (contraction over the forward's
// output features)
struct FfnTS {  // stream packs (mdx_row.h) of the transposed BondFFN matrices
  const float *WblT, *Wi1T, *Wi2T, *Wg1eT, *Wg2T;
};
struct EdgeBwdS {
  const float *WembHT, *WembDT;                 // edge_embs^T: -> 64 (He part), -> 16 (distance part)
  const float *Wg1eT, *Wg2T, *W1T, *W2T, *WmT;  // NodeBlock gate / edge_net / msg_net
  FfnTS ffn[2];
  const float *WselfT, *WoutT;                  // EdgeBlock tail
};
struct EdgeBwdW {
  EdgeBwdS s;   // row-owner kernel (mdx_bwd2.hip)
  EdgeBwdS ss;  // the same as split float16 streams (mdx_bwd2s.hip)
};
struct NodeBwdW {
  const float* WoutT;      // NodeBlock out_transform^T
  const float *W1T, *W2T;  // node_net^T
  const float* WcatT[4];   // (960 x 256)^T in 4 K-chunks: 256, 256, 256, 192
};
struct NodeBwdWS {  // split float16 dense packs of NodeBwdW (mdx_bondpred.hip node_bwd_s_kernel)
  const float *WoutT, *W1T, *W2T, *WcatT[4];
};

struct BondDecW {
  const float *W1e, *W1n, *b1, *g1, *be1, *W2, *b2, *g2, *be2, *W3, *b3;
  const float *W1eT, *W1nT, *W2T, *W3T;
};
