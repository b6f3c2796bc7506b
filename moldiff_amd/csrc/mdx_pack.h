// Host packer of the weight arena: parameter map -> one block of floats in the kernels' fragment orders, plus the pointer fix-ups that
// bind every weight-block member (mdx_weights.h) to its offset.  Plain C++17, no HIP: mdx_api.hip allocates, uploads and applies the
// fix-ups; tools/pack_host_check.cpp builds this unit with the host compiler alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/moldiff_hip.h"
#include "mdx_weights.h"

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};
using ParamMap = std::map<std::string, HostTensor>;

struct BlockW {
  EdgeAW ea;
  EdgeBW eb;
  NodeW nd;  // mid fields = tail of this block, pre fields = pre-stage of this block
  NodeWS nds;  // the same matrices as split float16 packs
};

// Every weight block of a model.  pack_model sizes the vectors and sets the scalars; the pointers are null until the fix-ups of its
// PackResult are applied (they point INTO this object: it must not be copied or resized in between).
struct ModelW {
  std::vector<BlockW> blocks;
  const float *soff = nullptr, *scoef = nullptr;  // distance smearing
  // heads
  const float *Wn = nullptr, *We = nullptr, *toff = nullptr, *tcoef = nullptr;
  MlpW nodedec{}, edgedec{};
  // bond predictor: decoder + transposed packs for the guidance backward
  BondDecW dec{};
  std::vector<EdgeBwdW> ebw;
  std::vector<NodeBwdW> nbw;
  std::vector<NodeBwdWS> nbws;
};

// A matrix to pack is a view plus a layout.  The view: columns col0 .. col0 + K of a row-major F x ldw source; transposed, the packed
// matrix is out[k][f] = W[f][col0 + k], K x F with F zero padded to 16 (contraction over the forward's output features).  key / centred
// only go into the slot record: the parameter the view is cut from (empty: none) and whether W is that parameter's centred copy.
struct PackView {
  std::string key;
  const float* W;
  int F, ldw, col0, K;
  bool transposed, centred;
  int rows() const { return transposed ? K : F; }
  int cols() const { return transposed ? (F + 15) / 16 * 16 : K; }
  float at(int r, int c) const {  // the packed matrix, zero beyond its rows and columns
    if (r >= rows() || c >= cols()) return 0.f;
    if (transposed) return c < F ? W[(size_t)c * ldw + col0 + r] : 0.f;
    return W[(size_t)r * ldw + col0 + c];
  }
};
enum PackLayout {
  PACK_DENSE,         // fp32 fragments for gemm_tile (mdx_tile.h)
  PACK_STREAM,        // fp32 fragments in the consumption order of rgemm (mdx_row.h), with the ring's zero tail
  PACK_DENSE_SPLIT,   // float16 hi / lo fragments for gemm_tile_s (mdx_tile_split.h)
  PACK_STREAM_SPLIT,  // float16 hi / lo fragments in the consumption order of rgemm_s (mdx_split.h), with the ring's zero tail
};

// What went where, for mdx_debug_pack_host (tests/test_ln_centred_pack.py reads the arena through it): one record per pack -- kind (d
// dense, s stream, S split stream, D split dense, v vector), arena offset and size in floats, the packed matrix's F x K, the parameter
// it was cut from (empty: not one named parameter), the first column, whether it was transposed and whether it came from a centred copy.
struct PackSlot {
  char kind;
  size_t off, n;
  int F, K, col0, transposed, centred;
  std::string key;
};

struct Packer {
  std::vector<float> arena;
  std::vector<std::pair<const float**, size_t>> fix;  // pointer slot <- arena offset
  std::vector<PackSlot> slots;
  // the split packs' range: false once a weight does not fit float16 (|w| >= 65504), and the largest magnitude seen
  bool split_ok = true;
  float split_wmax = 0.f;
  // reserves, fills, records the slot and binds the pointer; returns the offset
  size_t pack(const float** slot, const PackView& v, PackLayout layout);
  size_t vec(const float** slot, const std::string& key, const float* v, int n, int pad_to = 0, int col0 = 0, bool centred = false);

 private:
  size_t reserve(size_t n);
};

struct PackResult : Packer {
  std::string error;  // empty, or: missing / mis-shaped parameter, centring bound missed
};

// Centring of a Linear whose output feeds a LayerNorm over its F output features; returns the worst residual
// column mean / bound ratio (<= 1 when the pack is good).  W, out: F x ldw row-major, all ldw columns are centred.
double centre_columns(const float* W, int F, int ldw, float* out);

// float -> IEEE binary16 bits, round to nearest even (what a conversion instruction does; the host compiler need not know _Float16)
uint16_t f32_to_f16_bits(float x);
float f16_bits_to_f32(uint16_t h);

// Packs every weight of a model of configuration cf from its parameters.  ln_centred: centred packs for the denoiser's edge kernels (no
// effect on the other handle kinds).  *w is reset and sized; out->error says what went wrong, if anything.
void pack_model(const mdx_config& cf, const ParamMap& params, bool ln_centred, ModelW* w, PackResult* out);
