// Stand-alone check of the weight packer (moldiff_amd/csrc/mdx_pack.cpp, the unit the library links): every layout, straight and
// transposed, is packed from small random matrices and decoded back through the INVERSE index map, which is written here and shares
// nothing with the packer; the result must equal the zero-padded source bit for bit (hi and lo halves for the split layouts, whose
// float16 rounding is redone here by arithmetic, not by the packer's bit manipulation), the ring's tail must be zero, and the slot
// record and pointer fix-up must say what was packed.  Also: a centred view, the float16 range bookkeeping, the error string of a
// missing parameter.  No HIP, no GPU; tests/test_pack_host.py builds and runs it, and it can be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/pack_host_check tools/pack_host_check.cpp moldiff_amd/csrc/mdx_pack.cpp
//     /tmp/pack_host_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../moldiff_amd/csrc/mdx_pack.h"

static int failures = 0;
#define EXPECT(c, ...)                                       \
  do {                                                       \
    if (!(c)) {                                              \
      if (++failures <= 20) {                                \
        std::printf("FAILED line %d: %s  [", __LINE__, #c);  \
        std::printf(__VA_ARGS__);                            \
        std::printf("]\n");                                  \
      }                                                      \
    }                                                        \
  } while (0)

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

// float -> nearest float16 (ties to even) by arithmetic: the bits, and the value it stands for
struct Half {
  uint16_t bits;
  float value;
};
static Half ref_half(float x) {
  const uint16_t sign = std::signbit(x) ? 0x8000 : 0;
  const double a = std::fabs((double)x);
  if (a == 0.0) return {sign, sign ? -0.f : 0.f};
  if (a >= 65520.0) return {(uint16_t)(sign | 0x7c00), sign ? -INFINITY : INFINITY};
  int e;
  std::frexp(a, &e);                                                     // a = m 2^e, m in [0.5, 1)
  const double quantum = std::ldexp(1.0, std::max(e - 1, -14) - 10);     // spacing of float16 at a: 2^-24 below 2^-14
  const double v = std::nearbyint(a / quantum) * quantum;                // default rounding mode: to nearest, ties to even
  uint16_t h;
  if (v < std::ldexp(1.0, -14)) h = (uint16_t)(v / std::ldexp(1.0, -24));
  else {
    const int E = std::ilogb(v);
    h = (uint16_t)(((E + 15) << 10) + (int)(v / std::ldexp(1.0, E - 10)) - 1024);
  }
  return {(uint16_t)(sign | h), (float)(sign ? -v : v)};
}

static std::mt19937 rng(20240807);
static std::vector<float> random_matrix(int F, int ldw, float scale = 1.f) {
  std::normal_distribution<float> n(0.f, scale);
  std::vector<float> W((size_t)F * ldw);
  for (float& w : W) w = n(rng);
  return W;
}

// what the packed matrix must hold at (r, c): the view's element, zero beyond it
static float expected(const std::vector<float>& W, int F, int ldw, int col0, int K, bool tr, int r, int c) {
  if (tr) return r < K && c < F ? W[(size_t)c * ldw + col0 + r] : 0.f;
  return r < F && c < K ? W[(size_t)r * ldw + col0 + c] : 0.f;
}

static long elements_checked = 0;

static void check_pack(PackLayout layout, int F, int K, int col0, bool tr) {
  const bool split = layout == PACK_DENSE_SPLIT || layout == PACK_STREAM_SPLIT, stream = layout == PACK_STREAM || layout == PACK_STREAM_SPLIT;
  const int ldw = col0 + K + 7;
  const std::vector<float> W = random_matrix(F, ldw, split && F == 5 ? 1e-4f : 1.f);  // (small weights: lo halves that are float16 subnormals)
  Packer pk;
  const float* bound = nullptr;
  const float* other = nullptr;
  pk.vec(&other, "first", W.data(), 3);  // something before it, so that the offset is not 0
  const size_t off = pk.pack(&bound, PackView{"w", W.data(), F, ldw, col0, K, tr, false}, layout);
  const int R = tr ? K : F, C = tr ? (F + 15) / 16 * 16 : K;  // the packed matrix
  const int kw = split ? 32 : 16, G = (C + kw - 1) / kw, FT = (R + 15) / 16, FTP = (R + 31) / 32;
  const size_t body = (size_t)(stream ? 2 * FTP : FT) * G * (split ? 512 : 256), n = body + (stream ? 4 * 512 : 0);
  const char* what = "dsDS";
  EXPECT(pk.slots.size() == 2 && pk.fix.size() == 2, "%zu slots", pk.slots.size());
  const PackSlot& sl = pk.slots.back();
  EXPECT(sl.kind == what[layout] && sl.off == off && sl.n == n && sl.F == R && sl.K == C && sl.col0 == col0 && sl.transposed == (int)tr &&
             sl.centred == 0 && sl.key == "w",
         "%c off %zu n %zu (want %zu) F %d K %d", sl.kind, sl.off, sl.n, n, sl.F, sl.K);
  EXPECT(off % 64 == 0 && off >= 3 && pk.arena.size() == off + n, "off %zu size %zu", off, pk.arena.size());
  EXPECT(pk.fix.back().first == &bound && pk.fix.back().second == off, "fix-up");
  if (pk.arena.size() != off + n) return;
  const float* o = pk.arena.data() + off;
  for (size_t i = body; i < n; ++i) EXPECT(bits(o[i]) == 0, "ring tail not zero at %zu", i);
  if (!split) {
    for (size_t idx = 0; idx < body; ++idx) {  // inverse maps of the fp32 layouts
      const int s = idx % 4, lane = (idx / 4) % 64;
      const size_t frag = idx / 256;
      int ft, g;
      if (stream) {
        const size_t step = frag / 2;
        ft = 2 * (int)(step / G) + (int)(frag % 2), g = (int)(step % G);
      } else {
        ft = (int)(frag % FT), g = (int)(frag / FT);
      }
      const int r = 16 * ft + (lane & 15), c = 16 * g + 4 * (lane >> 4) + s;
      const float want = expected(W, F, ldw, col0, K, tr, r, c);
      EXPECT(bits(o[idx]) == bits(want), "layout %d F %d K %d col0 %d tr %d: (%d, %d) holds %g, want %g", layout, F, K, col0, tr, r, c, o[idx], want);
      ++elements_checked;
    }
    EXPECT(pk.split_ok && pk.split_wmax == 0.f, "fp32 packs do not touch the float16 range");
    return;
  }
  std::vector<uint16_t> hbuf(body * 2);
  std::memcpy(hbuf.data(), o, body * 4);
  float wmax = 0.f;
  for (size_t idx = 0; idx < hbuf.size(); ++idx) {  // inverse maps of the split layouts
    const int t = idx % 8, lane = (idx / 8) % 64;
    const size_t frag = idx / 512;
    int ft, g, h;
    if (stream) {
      const size_t hs = frag / 2, step = hs / 2;
      h = (int)(hs % 2), ft = 2 * (int)(step / G) + (int)(frag % 2), g = (int)(step % G);
    } else {
      h = (int)(frag % 2), ft = (int)((frag / 2) % FT), g = (int)((frag / 2) / FT);
    }
    const int r = 16 * ft + (lane & 15), c = 32 * g + 16 * (t / 4) + 4 * (lane >> 4) + t % 4;
    const float w = expected(W, F, ldw, col0, K, tr, r, c);
    wmax = std::max(wmax, std::fabs(w));
    const Half hi = ref_half(w), lo = ref_half((w - hi.value) * 2048.0f);
    const uint16_t want = h ? lo.bits : hi.bits;
    EXPECT(hbuf[idx] == want, "layout %d F %d K %d col0 %d tr %d: (%d, %d) half %d holds %04x, want %04x (w = %g)", layout, F, K, col0, tr, r, c, h,
           hbuf[idx], want, w);
    ++elements_checked;
  }
  EXPECT(pk.split_ok && pk.split_wmax == wmax, "wmax %g, want %g", pk.split_wmax, wmax);
}

// the conversions against the arithmetic reference, over every float16 and the floats around each rounding boundary
static void check_conversions() {
  for (uint32_t h = 0; h < 0x10000; ++h) {
    if ((h & 0x7c00) == 0x7c00) continue;  // infinities and NaNs
    const float v = f16_bits_to_f32((uint16_t)h);
    EXPECT(ref_half(v).bits == h && f32_to_f16_bits(v) == h, "round trip of %04x", h);
    const float up = f16_bits_to_f32((uint16_t)(h + 1));
    if ((h & 0x7fff) == 0x7bff || !std::isfinite(up)) continue;
    const float mid = 0.5f * v + 0.5f * up;  // exactly representable: the tie between h and h + 1
    for (float x : {std::nextafter(mid, v), mid, std::nextafter(mid, up), std::nextafter(v, up), std::nextafter(up, v)})
      EXPECT(f32_to_f16_bits(x) == ref_half(x).bits, "%a -> %04x, want %04x", x, f32_to_f16_bits(x), ref_half(x).bits);
  }
  for (float x : {65503.f, 65504.f, 65519.99f, 65520.f, 70000.f, 1e30f, 2.9e-8f, 2.98023224e-8f, 3e-8f, 1e-10f, 0.f, -0.f, -65520.f})
    EXPECT(f32_to_f16_bits(x) == ref_half(x).bits, "%a -> %04x, want %04x", x, f32_to_f16_bits(x), ref_half(x).bits);
  EXPECT(f32_to_f16_bits(INFINITY) == 0x7c00 && std::isinf(f16_bits_to_f32(0xfc00)) && std::isnan(f16_bits_to_f32(f32_to_f16_bits(NAN))), "inf / nan");
}

// a Linear (32 x 65) + bias packed centred: the stream of columns 0..63, the last column as a vector, the bias
static void check_centred() {
  const int F = 32, ldw = 65;
  std::vector<float> W = random_matrix(F, ldw), b = random_matrix(F, 1);
  for (int f = 0; f < F; ++f)
    for (int k = 0; k < ldw; ++k) W[(size_t)f * ldw + k] += 0.1f * (float)(k % 7);  // columns with a mean worth taking out
  std::vector<float> Wc(W.size()), bc(F);
  const double w1 = centre_columns(W.data(), F, ldw, Wc.data()), w2 = centre_columns(b.data(), F, 1, bc.data());
  EXPECT(w1 <= 1.0 && w2 <= 1.0, "residual / bound %g %g", w1, w2);
  for (int k = 0; k <= ldw; ++k) {  // the centring itself: float64 mean taken out, rounded once; k == ldw: the bias
    const float* src = k < ldw ? W.data() + k : b.data();
    const float* got = k < ldw ? Wc.data() + k : bc.data();
    const int ld = k < ldw ? ldw : 1;
    double mu = 0.0, res = 0.0, amax = 0.0;
    for (int f = 0; f < F; ++f) mu += (double)src[(size_t)f * ld];
    mu /= F;
    for (int f = 0; f < F; ++f) {
      EXPECT(bits(got[(size_t)f * ld]) == bits((float)((double)src[(size_t)f * ld] - mu)), "column %d row %d", k, f);
      res += (double)got[(size_t)f * ld], amax = std::max(amax, std::fabs((double)got[(size_t)f * ld]));
    }
    EXPECT(std::fabs(res / F) <= std::ldexp(amax, -24), "column %d keeps a mean of %g", k, res / F);
  }
  Packer pk;
  const float *pw = nullptr, *pt = nullptr, *pb = nullptr;
  const size_t off = pk.pack(&pw, PackView{"gate.weight", Wc.data(), F, ldw, 0, 64, false, true}, PACK_STREAM);
  std::vector<float> col(F);
  for (int f = 0; f < F; ++f) col[f] = Wc[(size_t)f * ldw + 64];
  const size_t toff = pk.vec(&pt, "gate.weight", col.data(), F, 0, 64, true), boff = pk.vec(&pb, "gate.bias", bc.data(), F, 0, 0, true);
  EXPECT(pk.slots.size() == 3 && pk.slots[0].centred == 1 && pk.slots[0].kind == 's' && pk.slots[0].K == 64, "stream slot");
  EXPECT(pk.slots[1].kind == 'v' && pk.slots[1].centred == 1 && pk.slots[1].col0 == 64 && pk.slots[1].F == F && pk.slots[1].K == 1 && pk.slots[1].n == (size_t)F &&
             pk.slots[1].key == "gate.weight",
         "time column slot");
  EXPECT(pk.slots[2].kind == 'v' && pk.slots[2].centred == 1 && pk.slots[2].col0 == 0 && pk.slots[2].key == "gate.bias", "bias slot");
  const float* o = pk.arena.data() + off;
  for (int f = 0; f < F; ++f) {
    for (int k = 0; k < 64; ++k) {  // stream: step = ftp*KG + g = k / 16 (one pair of feature tiles), j = f / 16
      const size_t idx = ((((size_t)(k / 16)) * 2 + f / 16) * 64 + (16 * ((k % 16) / 4) + f % 16)) * 4 + k % 4;
      EXPECT(bits(o[idx]) == bits(Wc[(size_t)f * ldw + k]), "centred stream (%d, %d)", f, k);
    }
    EXPECT(bits(pk.arena[toff + f]) == bits(Wc[(size_t)f * ldw + 64]) && bits(pk.arena[boff + f]) == bits(bc[f]), "centred vectors, row %d", f);
  }
  for (size_t i = 4 * 512; i < 4 * 512 + 4 * 512; ++i) EXPECT(bits(o[i]) == 0, "ring tail");
}

static void check_range_and_errors() {
  for (PackLayout layout : {PACK_DENSE_SPLIT, PACK_STREAM_SPLIT})
    for (float big : {65503.f, 65504.f, -70000.f, INFINITY}) {
      std::vector<float> W = random_matrix(16, 32);
      W[5 * 32 + 9] = big;
      Packer pk;
      const float* p = nullptr;
      pk.pack(&p, PackView{"", W.data(), 16, 32, 0, 32, false, false}, layout);
      EXPECT(pk.split_ok == (std::fabs(big) < 65504.f) && pk.split_wmax == std::fabs(big), "weight %g: split_ok %d wmax %g", big, pk.split_ok, pk.split_wmax);
      EXPECT(pk.slots[0].key.empty(), "a view without a key has none in its record");
    }
  // a handle without parameters: the first key the packer asks for is the error
  mdx_config cf{};
  cf.kind = MDX_KIND_NET, cf.node_dim = MDX_ND, cf.edge_dim = MDX_ED, cf.num_blocks = 2, cf.num_gaussians = MDX_NG, cf.update_pos = 1;
  ParamMap params;
  ModelW w;
  PackResult out;
  pack_model(cf, params, true, &w, &out);
  EXPECT(out.error == "missing or mis-shaped parameter: distance_expansion.offset", "%s", out.error.c_str());
  EXPECT(w.blocks.size() == 2 && w.ebw.empty(), "weight blocks sized");
  params["distance_expansion.offset"] = HostTensor{{MDX_NG + 1}, std::vector<float>(MDX_NG + 1, 0.f)};
  pack_model(cf, params, true, &w, &out);
  EXPECT(out.error == "missing or mis-shaped parameter: distance_expansion.offset (shape mismatch)", "%s", out.error.c_str());
}

int main() {
  check_conversions();
  for (int tr = 0; tr < 2; ++tr)
    for (int F : {5, 16, 32, 33})
      for (int col0 : {0, 16}) {
        for (int K : {16, 32, 48})
          for (PackLayout layout : {PACK_DENSE, PACK_STREAM}) check_pack(layout, F, K, col0, tr != 0);
        for (int K : {16, 40, 64})
          for (PackLayout layout : {PACK_DENSE_SPLIT, PACK_STREAM_SPLIT}) check_pack(layout, F, K, col0, tr != 0);
      }
  check_centred();
  check_range_and_errors();
  if (failures) {
    std::printf("pack_host_check: %d FAILURES\n", failures);
    return 1;
  }
  std::printf("pack_host_check ok: %ld packed elements decoded\n", elements_checked);
  return 0;
}
