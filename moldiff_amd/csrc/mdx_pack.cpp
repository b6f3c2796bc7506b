// Host packer of the weight arena (mdx_pack.h): pure host arithmetic, no HIP.
#include "mdx_pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>

// Centring of a Linear whose output feeds a LayerNorm over its F output features: the mean of W x + b over
// the features is (column mean of W) . x + mean(b), so with the column means taken out of W (and mean(b) out of b) the
// pre-activation has mean zero whatever x is, and the kernel's LayerNorm needs no mean (mdx_row.h row_layernorm_centred).  Done in
// float64 from the fp32 weights and rounded to fp32 once.  What the rounding leaves: each entry is off by at most half an ulp,
// 2^-24 |w|, so a column's residual mean is at most 2^-24 max|w| of that column -- checked here, column by column; the return value
// is the worst residual / bound ratio (<= 1 when the pack is good).  W: F x ldw row-major, all ldw columns are centred.
double centre_columns(const float* W, int F, int ldw, float* out) {
  double worst = 0.0;
  for (int k = 0; k < ldw; ++k) {
    double mu = 0.0;
    for (int f = 0; f < F; ++f) mu += (double)W[(size_t)f * ldw + k];
    mu /= F;
    double res = 0.0, amax = 0.0;
    for (int f = 0; f < F; ++f) {
      const float c = (float)((double)W[(size_t)f * ldw + k] - mu);
      out[(size_t)f * ldw + k] = c;
      res += (double)c;
      amax = std::max(amax, std::fabs((double)c));
    }
    const double bound = std::ldexp(amax, -24);
    res = std::fabs(res / F);
    if (res > 0.0) worst = std::max(worst, bound > 0.0 ? res / bound : 2.0);
  }
  return worst;
}

uint16_t f32_to_f16_bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((u >> 13) & 0x3ffu));  // NaN, quieted
  if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                          // >= 65520 rounds to infinity
  uint32_t h, rem, half;
  if (u < 0x38800000u) {  // below 2^-14: a float16 subnormal, in units of 2^-24
    const int shift = 126 - (int)(u >> 23);
    if (shift > 24) return (uint16_t)sign;
    const uint32_t mant = (u & 0x7fffffu) | 0x800000u;
    h = mant >> shift, rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
  } else {
    h = (u - 0x38000000u) >> 13, rem = u & 0x1fffu, half = 0x1000u;
  }
  if (rem > half || (rem == half && (h & 1u))) ++h;  // nearest, ties to even; a carry moves into the exponent as it should
  return (uint16_t)(sign | h);
}
float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 0) {
    const float v = std::ldexp((float)m, -24);
    return sign ? -v : v;
  }
  const uint32_t u = sign | (e == 31 ? 0x7f800000u : (e + 112u) << 23) | (m << 13);
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

// ------------------------------------------------------------------------------------------------
// the one pack function
// ------------------------------------------------------------------------------------------------
size_t Packer::reserve(size_t n) {
  size_t off = (arena.size() + 63) & ~size_t(63);
  arena.resize(off + n, 0.f);
  return off;
}

// Every pack is made of 1-KiB fragments: 64 lanes x 4 floats (fp32) or 64 lanes x 8 halves (split), one per (feature tile ft of 16
// rows, k-group g) -- and per half h for the split formats, which hold W = hi + lo 2^-11 with hi = fp16(W), lo = fp16((W - hi) 2^11)
// (2^MDX_LO_SHIFT), h = 0: hi, h = 1: lo.  Rows and columns beyond the matrix are zero.
//
// Element formats (what lane (q, c) = (lane >> 4, lane & 15) of the fragment (ft, g) holds):
//   fp32   float s = 0..3:  W[16 ft + c][col0 + 16 g + 4 q + s]                        k-groups of 16
//   split  half  t = 0..7:  W[16 ft + c][col0 + 32 g + 16 (t / 4) + 4 q + t % 4]       k-groups of 32, K padded to 32
//
// Index maps (where the fragment goes, in fragments; NH = 1 fp32, 2 split):
//   dense  (gemm_tile, mdx_node_s.hip gemm_tile_s)   (g*FT + ft)*NH + h,  FT = ceil(F / 16)
//          fp32:  float index ((g*FT + ft)*64 + lane)*4 + s;  split: 1-KiB fragment index (g*FT + ft)*2 + h
//   stream (mdx_row.h rgemm, mdx_split.h rgemm_s: the same fragments in consumption order)   ((ftp*KG + g)*NH + h)*2 + j,  ft = 2 ftp + j
//          fp32:  float index ((((ftp*KG + g)*2 + j)*64 + lane)*4 + s) <- W[16*(2 ftp + j) + (lane & 15)][col0 + 16 g + 4 (lane >> 4) + s]
//          split: half-step hs = (ftp*KG + g)*2 + h carries the fragments of feature tiles 2 ftp + j, j = 0,1, 64 lanes x 8 halves each:
//                 half index ((hs*2 + j)*64 + lane)*8 + t
//          F is padded to a multiple of 32 with zero rows, plus MDX_RING_PAD = 4 zero steps (half-steps) of 512 floats as tail so a ring
//          may over-fetch.  The split stream has the same bytes as the fp32 stream's size for K % 32 == 0.
size_t Packer::pack(const float** slot, const PackView& v, PackLayout layout) {
  const bool split = layout == PACK_DENSE_SPLIT || layout == PACK_STREAM_SPLIT;
  const bool stream = layout == PACK_STREAM || layout == PACK_STREAM_SPLIT;
  const int R = v.rows(), C = v.cols();
  const int NH = split ? 2 : 1, KW = split ? 32 : 16;
  const int FT = stream ? 2 * ((R + 31) / 32) : (R + 15) / 16, G = (C + KW - 1) / KW;
  const size_t n = (size_t)FT * G * NH * 256 + (stream ? 4 * 512 : 0);
  const size_t off = reserve(n);
  float* o = arena.data() + off;
  for (int ft = 0; ft < FT; ++ft)
    for (int g = 0; g < G; ++g) {
      const size_t frag = stream ? (((size_t)(ft / 2) * G + g) * NH) * 2 + ft % 2 : ((size_t)g * FT + ft) * NH;
      const size_t next_half = stream ? 2 : 1;  // fragments from the hi to the lo half
      if (!split) {
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < 4; ++s) o[frag * 256 + lane * 4 + s] = v.at(16 * ft + (lane & 15), 16 * g + 4 * (lane >> 4) + s);
        continue;
      }
      uint16_t hi[512], lo[512];
      for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < 8; ++t) {
          const float w = v.at(16 * ft + (lane & 15), 32 * g + 16 * (t / 4) + 4 * (lane >> 4) + t % 4);
          if (!(std::fabs(w) < 65504.0f)) split_ok = false;
          split_wmax = std::max(split_wmax, std::fabs(w));
          hi[lane * 8 + t] = f32_to_f16_bits(w);
          lo[lane * 8 + t] = f32_to_f16_bits((w - f16_bits_to_f32(hi[lane * 8 + t])) * 2048.0f);
        }
      std::memcpy(o + frag * 256, hi, sizeof(hi));
      std::memcpy(o + (frag + next_half) * 256, lo, sizeof(lo));
    }
  slots.push_back(PackSlot{"dsDS"[layout], off, n, R, C, v.col0, v.transposed ? 1 : 0, v.centred ? 1 : 0, v.key});
  fix.emplace_back(slot, off);
  return off;
}

size_t Packer::vec(const float** slot, const std::string& key, const float* v, int n, int pad_to, int col0, bool centred) {
  const size_t len = (size_t)std::max(n, pad_to), off = reserve(len);
  std::copy(v, v + n, arena.begin() + off);
  slots.push_back(PackSlot{'v', off, len, n, 1, col0, 0, centred ? 1 : 0, key});
  fix.emplace_back(slot, off);
  return off;
}

// ------------------------------------------------------------------------------------------------
// the model: each Linear named once, each kernel's packs emitted from a table
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int ND = MDX_ND, ED = MDX_ED, NG = MDX_NG, GIN = ED + ND + 1;  // 321

// One Linear (pre + ".weight": F x ldw, pre + ".bias": F).  centred: this handle packs it with the mean over its output features taken
// out (centre_columns) -- a property of the layer, so its stream packs, its split packs, its time column, its rows of the node table and
// its bias all come from the one centred copy.  The convention is "every addend of a pre-LayerNorm sum, or none".
struct Layer {
  std::string pre;
  int F, ldw;
  bool centred = false;
  std::string w() const { return pre + ".weight"; }
  std::string b() const { return pre + ".bias"; }
};
struct Mlp {  // common.MLP: Linear -> LayerNorm -> ReLU -> Linear
  Layer l1, l2;
  std::string ln;
};
Mlp mlp_of(const std::string& pre, int in, int hid, int out, bool centre1 = false) {
  return Mlp{{pre + ".net.0", hid, in, centre1}, {pre + ".net.3", out, hid}, pre + ".net.1"};
}
struct Ffn {  // BondFFN of the EdgeBlock
  Layer bl, nl;
  Mlp inter, gate;
};
struct BlockLayers {
  // NodeBlock, edge side (edge kernel A): edge_embs, gate over [He' | x | t], edge_net, msg_net
  Layer emb;
  Mlp gate, en;
  Layer msg;
  Ffn ffn[2];  // EdgeBlock's bond_ffn_left / right (edge kernel A)
  // EdgeBlock tail (edge kernel B)
  Layer self, eout, nf[2];
  std::string eln;
  // PosUpdate.edge_lin (edge kernel B): a BondFFN with one output
  Layer pbl, pnl;
  Mlp pinter, pgate;
  // NodeBlock, node side (node kernel) and PosUpdate's per-node MLPs
  Layer centroid, nout;
  std::string nln;
  Mlp nn, left, right;
};
// lnc: the Linears that feed a LayerNorm inside an edge kernel are centred -- the gates' and edge_net's / the inter modules' first layers
BlockLayers block_layers(const std::string& net, int i, bool lnc) {
  const std::string si = std::to_string(i);
  const std::string nb = net + "node_blocks_with_edge." + si, eb = net + "edge_blocks." + si, el = net + "pos_blocks." + si + ".edge_lin",
                    pb = net + "pos_blocks." + si;
  BlockLayers L;
  L.emb = {net + "edge_embs." + si, ED, ED + NG};
  L.gate = mlp_of(nb + ".gate", GIN, ND, ND, lnc);
  L.en = mlp_of(nb + ".edge_net", ED, ND, ND, lnc);
  L.msg = {nb + ".msg_net", ND, ND};
  for (int s = 0; s < 2; ++s) {
    const std::string fp = eb + (s ? ".bond_ffn_right" : ".bond_ffn_left");
    L.ffn[s] = Ffn{{fp + ".bond_linear", 2 * ED, ED}, {fp + ".node_linear", 2 * ED, ND}, mlp_of(fp + ".inter_module", 2 * ED, 2 * ED, ED, lnc),
                   mlp_of(fp + ".gate", GIN, 32, ED, lnc)};
    L.nf[s] = {eb + (s ? ".node_ffn_right" : ".node_ffn_left"), ED, ND};
  }
  L.self = {eb + ".self_ffn", ED, ED};
  L.eout = {eb + ".out_transform", ED, ED};
  L.eln = eb + ".layer_norm";
  L.pbl = {el + ".bond_linear", ND, ED};
  L.pnl = {el + ".node_linear", ND, ED};
  L.pinter = mlp_of(el + ".inter_module", ND, ND, 1, lnc);
  L.pgate = mlp_of(el + ".gate", 2 * ED + 1, 32, 1, lnc);
  L.centroid = {nb + ".centroid_lin", ND, ND};
  L.nout = {nb + ".out_transform", ND, ND};
  L.nln = nb + ".layer_norm";
  L.nn = mlp_of(nb + ".node_net", ND, ND, ND);
  L.left = mlp_of(pb + ".left_lin_edge", ND, ED, ED);
  L.right = mlp_of(pb + ".right_lin_edge", ND, ED, ED);
  return L;
}

// One matrix operand of a kernel: the layer, the columns the kernel contracts over, and where the pointer of each emitted pass goes.
struct Mat {
  const Layer* l;
  int col0, K;
  const float** dst[2];
};
struct Pass {
  PackLayout layout;
  bool transposed;
};
const Pass STREAMS[2] = {{PACK_STREAM, false}, {PACK_STREAM_SPLIT, false}}, DENSES[2] = {{PACK_DENSE, false}, {PACK_DENSE_SPLIT, false}},
           STREAMS_T[2] = {{PACK_STREAM, true}, {PACK_STREAM_SPLIT, true}}, DENSES_T[2] = {{PACK_DENSE, true}, {PACK_DENSE_SPLIT, true}},
           DENSE_AND_T[2] = {{PACK_DENSE, false}, {PACK_DENSE, true}};

struct Ctx {
  const ParamMap& params;
  PackResult& out;
  std::string missing;
  const HostTensor* get(const std::string& key, std::initializer_list<int64_t> shape) {
    auto it = params.find(key);
    if (it == params.end()) {
      if (missing.empty()) missing = key;
      return nullptr;
    }
    if (it->second.shape != std::vector<int64_t>(shape)) {
      if (missing.empty()) missing = key + " (shape mismatch)";
      return nullptr;
    }
    return &it->second;
  }
  // Centred copy of a Linear -- centre_columns -- made once per layer and shared by every pack cut from it.
  struct Centred {
    std::vector<float> W, b;
  };
  std::map<std::string, Centred> cen;
  std::string centre_bad;  // first layer whose rounded pack missed the residual-mean bound (never, unless the arithmetic above is wrong)
  const Centred* centred(const Layer& l) {
    auto it = cen.find(l.pre);
    if (it != cen.end()) return &it->second;
    const HostTensor* t = get(l.w(), {l.F, l.ldw});
    const HostTensor* bt = get(l.b(), {l.F});
    if (!t || !bt) return nullptr;
    Centred c;
    c.W.resize(t->data.size());
    c.b.resize(l.F);
    const double w1 = centre_columns(t->data.data(), l.F, l.ldw, c.W.data());
    const double w2 = centre_columns(bt->data.data(), l.F, 1, c.b.data());
    if (!(w1 <= 1.0 && w2 <= 1.0) && centre_bad.empty()) centre_bad = l.w();
    return &(cen[l.pre] = std::move(c));
  }
  // the layer's weight (F x ldw) and bias (F) as this handle packs them: stored, or the centred copy; null = missing (noted)
  const float* weight(const Layer& l) {
    if (l.centred) {
      const Centred* c = centred(l);
      return c ? c->W.data() : nullptr;
    }
    const HostTensor* t = get(l.w(), {l.F, l.ldw});
    return t ? t->data.data() : nullptr;
  }
  const float* bias_of(const Layer& l) {
    if (l.centred) {
      const Centred* c = centred(l);
      return c ? c->b.data() : nullptr;
    }
    const HostTensor* t = get(l.b(), {l.F});
    return t ? t->data.data() : nullptr;
  }

  // a kernel's table, once per pass: all matrices in the first layout, then all in the second
  void emit(const std::vector<Mat>& mats, const Pass* passes, int npasses) {
    for (int p = 0; p < npasses; ++p)
      for (const Mat& m : mats)
        if (const float* W = weight(*m.l))
          out.pack(m.dst[p], PackView{m.l->w(), W, m.l->F, m.l->ldw, m.col0, m.K, passes[p].transposed, m.l->centred}, passes[p].layout);
  }
  void bias(const float** slot, const Layer& l, int pad_to = 0) {
    if (const float* b = bias_of(l)) out.vec(slot, l.b(), b, l.F, pad_to, 0, l.centred);
  }
  void column(const float** slot, const Layer& l, int col) {  // one column of the weight as a vector (the gates' time columns)
    const float* W = weight(l);
    if (!W) return;
    std::vector<float> v(l.F);
    for (int f = 0; f < l.F; ++f) v[f] = W[(size_t)f * l.ldw + col];
    out.vec(slot, l.w(), v.data(), l.F, 0, col, l.centred);
  }
  void vec(const float** slot, const std::string& key, int n) {
    if (const HostTensor* t = get(key, {n})) out.vec(slot, key, t->data.data(), n);
  }
  void raw(const float** slot, const std::vector<float>& v) { out.vec(slot, "", v.data(), (int)v.size()); }  // not one named parameter
  void layernorm(const float** g, const float** b, const std::string& pre, int n) {
    vec(g, pre + ".weight", n);
    vec(b, pre + ".bias", n);
  }
  template <class M>  // MlpW or MlpV: the vectors of an MLP
  void mlp_vecs(M* w, const Mlp& m, int out_pad = 0) {
    bias(&w->b1, m.l1);
    layernorm(&w->g, &w->be, m.ln, m.l1.F);
    bias(&w->b2, m.l2, out_pad);
  }
  // an MLP whose second layer has ONE output (PosUpdate's inter module and gate): the row as a vector, the bias as a scalar
  void row_and_scalar(const float** row, float* scalar, const Layer& l) {
    if (const HostTensor* t = get(l.w(), {1, l.ldw})) raw(row, t->data);
    if (const HostTensor* t = get(l.b(), {1})) *scalar = t->data[0];
  }
};

void pack_edge_a(Ctx& c, const BlockLayers& L, EdgeAW& a) {
  a.lnc = L.gate.l1.centred ? 1 : 0;
  c.bias(&a.bemb, L.emb);
  c.bias(&a.bg1, L.gate.l1);
  c.column(&a.wtg1, L.gate.l1, GIN - 1);
  c.layernorm(&a.gg, &a.gb, L.gate.ln, ND);
  c.bias(&a.bg2, L.gate.l2);
  c.mlp_vecs(&a.en, L.en);
  c.bias(&a.bm, L.msg);
  std::vector<Mat> mats = {{&L.emb, 0, ED + NG, {&a.s.Wemb, &a.ss.Wemb}}, {&L.gate.l1, 0, ED, {&a.s.Wg1e, &a.ss.Wg1e}},
                           {&L.gate.l2, 0, ND, {&a.s.Wg2, &a.ss.Wg2}},    {&L.en.l1, 0, ED, {&a.s.W1, &a.ss.W1}},
                           {&L.en.l2, 0, ND, {&a.s.W2, &a.ss.W2}},        {&L.msg, 0, ND, {&a.s.Wm, &a.ss.Wm}}};
  for (int s = 0; s < 2; ++s) {
    const Ffn& F = L.ffn[s];
    FfnW& f = a.ffn[s];
    FfnS &fs = a.s.ffn[s], &fss = a.ss.ffn[s];
    c.mlp_vecs(&f.inter, F.inter);
    c.bias(&f.bg1, F.gate.l1);
    c.column(&f.wtg1, F.gate.l1, GIN - 1);
    c.layernorm(&f.gg, &f.gb, F.gate.ln, 32);
    c.bias(&f.bg2, F.gate.l2);
    mats.insert(mats.end(), {{&F.bl, 0, ED, {&fs.Wbl, &fss.Wbl}},
                             {&F.gate.l1, 0, ED, {&fs.Wg1e, &fss.Wg1e}},
                             {&F.inter.l1, 0, 2 * ED, {&fs.W1, &fss.W1}},
                             {&F.inter.l2, 0, 2 * ED, {&fs.W2, &fss.W2}},
                             {&F.gate.l2, 0, 32, {&fs.Wg2, &fss.Wg2}}});
  }
  c.emit(mats, STREAMS, 2);
}

void pack_edge_b(Ctx& c, const BlockLayers& L, bool update_pos, EdgeBW& b) {
  c.bias(&b.bself, L.self);
  c.layernorm(&b.lng, &b.lnb, L.eln, ED);
  c.bias(&b.bout, L.eout);
  std::vector<Mat> mats = {{&L.self, 0, ED, {&b.s.Wself, &b.ss.Wself}}, {&L.eout, 0, ED, {&b.s.Wout, &b.ss.Wout}}};
  if (update_pos) {  // PosUpdate.edge_lin
    b.lnc = L.pgate.l1.centred ? 1 : 0;
    c.bias(&b.bi1, L.pinter.l1);
    c.layernorm(&b.ig, &b.ib, L.pinter.ln, ND);
    c.row_and_scalar(&b.wi2, &b.bi2, L.pinter.l2);
    c.bias(&b.bg1, L.pgate.l1);
    c.column(&b.wtg1, L.pgate.l1, 2 * ED);
    c.layernorm(&b.gg, &b.gb, L.pgate.ln, 32);
    c.row_and_scalar(&b.wg2, &b.bg2, L.pgate.l2);
    mats.insert(mats.end(), {{&L.pbl, 0, ED, {&b.s.Wbl, &b.ss.Wbl}},
                             {&L.pnl, 0, ED, {&b.s.Wnl, &b.ss.Wnl}},
                             {&L.pinter.l1, 0, ND, {&b.s.Wi1, &b.ss.Wi1}},
                             {&L.pgate.l1, 0, ED, {&b.s.Wg1h, &b.ss.Wg1h}},     // He part of [He'' | a | t]
                             {&L.pgate.l1, ED, ED, {&b.s.Wg1a, &b.ss.Wg1a}}});  // a part
  }
  c.emit(mats, STREAMS, 2);
}

// the node kernel's packs of a block; *wcat receives the dense (960 x 256) concatenated node-table weights
void pack_node(Ctx& c, const BlockLayers& L, int i, bool update_pos, bool lnc, NodeW& n, NodeWS& ns, std::vector<float>* wcat) {
  c.layernorm(&n.lng, &n.lnb, L.nln, ND);
  c.bias(&n.bout, L.nout);
  c.mlp_vecs(&n.nn, L.nn);
  std::vector<Mat> mats = {
      {&L.nout, 0, ND, {&n.Wout, &ns.Wout}}, {&L.nn.l1, 0, ND, {&n.nn.W1, &ns.nnW1}}, {&L.nn.l2, 0, ND, {&n.nn.W2, &ns.nnW2}}};
  if (update_pos) {
    c.mlp_vecs(&n.left, L.left);
    c.mlp_vecs(&n.right, L.right);
    mats.insert(mats.end(), {{&L.left.l1, 0, ND, {&n.left.W1, &ns.leftW1}},
                             {&L.left.l2, 0, ED, {&n.left.W2, &ns.leftW2}},
                             {&L.right.l1, 0, ND, {&n.right.W1, &ns.rightW1}},
                             {&L.right.l2, 0, ED, {&n.right.W2, &ns.rightW2}}});
  }
  c.emit(mats, DENSES, 2);
  // concatenated per-node table weights (960 x 256) + bias: columns col0 .. col0 + 256 of each layer at its rows of the table (the
  // gates' node parts, gathered by edge kernel A into centred sums, come from the gates' centred copies like everything else of theirs)
  std::vector<float>& W = *wcat;
  W.assign((size_t)MDX_NTW * ND, 0.f);
  std::vector<float> bias(MDX_NTW, 0.f);
  struct Rows {
    const Layer* l;
    int col0, dst_row;
    bool with_bias;
  };
  const Rows rows[] = {{&L.centroid, 0, MDX_NT_C, true},       {&L.gate.l1, ED, MDX_NT_GX, false},         {&L.ffn[0].nl, 0, MDX_NT_NLL, false},
                       {&L.ffn[1].nl, 0, MDX_NT_NLR, false},   {&L.nf[0], 0, MDX_NT_NFL, true},            {&L.nf[1], 0, MDX_NT_NFR, true},
                       {&L.ffn[0].gate.l1, ED, MDX_NT_GXL, false}, {&L.ffn[1].gate.l1, ED, MDX_NT_GXR, false}};
  for (const Rows& r : rows) {
    const float* src = c.weight(*r.l);
    if (!src) continue;
    for (int f = 0; f < r.l->F; ++f)
      for (int k = 0; k < ND; ++k) W[(size_t)(r.dst_row + f) * ND + k] = src[(size_t)f * r.l->ldw + r.col0 + k];
    if (r.with_bias)
      if (const float* b = c.bias_of(*r.l)) std::copy(b, b + r.l->F, bias.begin() + r.dst_row);
  }
  const PackView table{"wcat." + std::to_string(i), W.data(), MDX_NTW, ND, 0, ND, false, lnc};  // (centred: its GX / GXL / GXR rows)
  c.out.pack(&n.Wcat, table, PACK_DENSE);
  c.out.pack(&ns.Wcat, table, PACK_DENSE_SPLIT);
  c.raw(&n.bcat, bias);
}

// transposed packs of a block for the data-gradient backward (guidance)
void pack_backward(Ctx& c, const BlockLayers& L, const std::vector<float>& wcat, EdgeBwdW& e, NodeBwdW& n, NodeBwdWS& ns) {
  std::vector<Mat> mats = {{&L.emb, 0, ED, {&e.s.WembHT, &e.ss.WembHT}},  {&L.emb, ED, NG, {&e.s.WembDT, &e.ss.WembDT}},
                           {&L.gate.l1, 0, ED, {&e.s.Wg1eT, &e.ss.Wg1eT}}, {&L.gate.l2, 0, ND, {&e.s.Wg2T, &e.ss.Wg2T}},
                           {&L.en.l1, 0, ED, {&e.s.W1T, &e.ss.W1T}},       {&L.en.l2, 0, ND, {&e.s.W2T, &e.ss.W2T}},
                           {&L.msg, 0, ND, {&e.s.WmT, &e.ss.WmT}},         {&L.self, 0, ED, {&e.s.WselfT, &e.ss.WselfT}},
                           {&L.eout, 0, ED, {&e.s.WoutT, &e.ss.WoutT}}};
  for (int s = 0; s < 2; ++s) {
    const Ffn& F = L.ffn[s];
    FfnTS &f = e.s.ffn[s], &fs = e.ss.ffn[s];
    mats.insert(mats.end(), {{&F.bl, 0, ED, {&f.WblT, &fs.WblT}},
                             {&F.inter.l1, 0, 2 * ED, {&f.Wi1T, &fs.Wi1T}},
                             {&F.inter.l2, 0, 2 * ED, {&f.Wi2T, &fs.Wi2T}},
                             {&F.gate.l1, 0, ED, {&f.Wg1eT, &fs.Wg1eT}},
                             {&F.gate.l2, 0, 32, {&f.Wg2T, &fs.Wg2T}}});
  }
  c.emit(mats, STREAMS_T, 2);
  c.emit({{&L.nout, 0, ND, {&n.WoutT, &ns.WoutT}}, {&L.nn.l1, 0, ND, {&n.W1T, &ns.W1T}}, {&L.nn.l2, 0, ND, {&n.W2T, &ns.W2T}}}, DENSES_T, 2);
  if (!wcat.empty())
    for (int ch = 0; ch < 4; ++ch) {  // the node table's matrix transposed, in K-chunks of its 960 rows
      const int kc = ch < 3 ? 256 : 192;
      std::vector<float> Mt((size_t)ND * kc);
      for (int f = 0; f < ND; ++f)
        for (int k = 0; k < kc; ++k) Mt[(size_t)f * kc + k] = wcat[(size_t)(256 * ch + k) * ND + f];
      const PackView chunk{"", Mt.data(), ND, kc, 0, kc, false, false};
      c.out.pack(&n.WcatT[ch], chunk, PACK_DENSE);
      c.out.pack(&ns.WcatT[ch], chunk, PACK_DENSE_SPLIT);
    }
}

}  // namespace

void pack_model(const mdx_config& cf, const ParamMap& params, bool ln_centred, ModelW* w, PackResult* out) {
  *w = ModelW{};
  *out = PackResult{};
  Ctx c{params, *out};
  const std::string net = cf.kind == MDX_KIND_MOLDIFF ? "denoiser." : cf.kind == MDX_KIND_BONDPRED ? "encoder." : "";
  // Centred packs: the denoiser only.  Never the bond predictor: its tape keeps pre-LayerNorm values that the guidance backward
  // re-normalises against the un-centred transposed packs.
  const bool lnc = ln_centred && cf.kind == MDX_KIND_MOLDIFF;
  w->blocks.assign(cf.num_blocks, BlockW{});
  std::vector<BlockLayers> layers;
  std::vector<std::vector<float>> wcat(cf.num_blocks);
  c.vec(&w->soff, net + "distance_expansion.offset", NG);
  c.vec(&w->scoef, net + "distance_expansion.coeff", NG);
  for (int i = 0; i < cf.num_blocks; ++i) {
    layers.push_back(block_layers(net, i, lnc));
    BlockW& b = w->blocks[i];
    pack_edge_a(c, layers[i], b.ea);
    pack_edge_b(c, layers[i], cf.update_pos != 0, b.eb);
    pack_node(c, layers[i], i, cf.update_pos != 0, lnc, b.nd, b.nds, &wcat[i]);
  }
  if (cf.kind == MDX_KIND_MOLDIFF || cf.kind == MDX_KIND_BONDPRED) {
    const int nd_emb = ND - cf.time_dim, ed_emb = ED - cf.time_dim;
    const int ein = cf.kind == MDX_KIND_MOLDIFF ? cf.num_edge_types : 2 * cf.num_node_types;
    if (const HostTensor* t = c.get("node_embedder.weight", {nd_emb, cf.num_node_types})) c.raw(&w->Wn, t->data);
    if (const HostTensor* t = c.get("edge_embedder.weight", {ed_emb, ein})) c.raw(&w->We, t->data);
    const std::string te = cf.kind == MDX_KIND_MOLDIFF ? "time_emb.0." : "time_emb.";
    if (cf.time_dim > 0) {  // 0: the time-free bond predictor (models/bond_predictor.py:27-31) has no time embedding
      c.vec(&w->toff, te + "offset", cf.time_dim);
      c.vec(&w->tcoef, te + "coeff", cf.time_dim);
    }
  }
  if (cf.kind == MDX_KIND_MOLDIFF) {  // the two decoders, second layers padded to 16 outputs
    const Mlp nd = mlp_of("node_decoder", ND, ND, cf.num_node_types), ed = mlp_of("edge_decoder", ED, ED, cf.num_edge_types);
    c.mlp_vecs(&w->nodedec, nd, 16);
    c.mlp_vecs(&w->edgedec, ed, 16);
    c.emit({{&nd.l1, 0, ND, {&w->nodedec.W1}}, {&nd.l2, 0, ND, {&w->nodedec.W2}}, {&ed.l1, 0, ED, {&w->edgedec.W1}}, {&ed.l2, 0, ED, {&w->edgedec.W2}}},
           DENSES, 1);
  }
  if (cf.kind == MDX_KIND_BONDPRED) {
    // bond decoder: Linear([He | Hn]) -> LN -> ReLU -> Linear -> LN -> ReLU -> Linear, each matrix dense and transposed
    const std::string d = "edge_decoder.net.";
    const Layer d0{d + "0", ED, ED + ND}, d3{d + "3", ED, ED}, d6{d + "6", cf.num_edge_types, ED};
    BondDecW& bd = w->dec;
    c.bias(&bd.b1, d0);
    c.layernorm(&bd.g1, &bd.be1, d + "1", ED);
    c.bias(&bd.b2, d3);
    c.layernorm(&bd.g2, &bd.be2, d + "4", ED);
    c.bias(&bd.b3, d6, 16);
    c.emit({{&d0, 0, ED, {&bd.W1e, &bd.W1eT}}, {&d0, ED, ND, {&bd.W1n, &bd.W1nT}}, {&d3, 0, ED, {&bd.W2, &bd.W2T}}, {&d6, 0, ED, {&bd.W3, &bd.W3T}}},
           DENSE_AND_T, 2);
    w->ebw.assign(cf.num_blocks, EdgeBwdW{});
    w->nbw.assign(cf.num_blocks, NodeBwdW{});
    w->nbws.assign(cf.num_blocks, NodeBwdWS{});
    for (int i = 0; i < cf.num_blocks; ++i) pack_backward(c, layers[i], wcat[i], w->ebw[i], w->nbw[i], w->nbws[i]);
  }
  if (!c.missing.empty()) out->error = "missing or mis-shaped parameter: " + c.missing;
  else if (!c.centre_bad.empty()) out->error = "centred pack of " + c.centre_bad + " misses its residual-mean bound";
}
