// Stand-alone check of the host-side preparation of mdx_mol_bounds and mdx_mol_embed (moldiff_amd/csrc/mdx_embed_args.h): validation of
// the tolerances, the workspace sizes and the minimiser's scalars, the ring cosines, the two distance formulas of the bounds model and
// the mapping of two Philox words to a double.  No HIP, no GPU; meant to be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/embed_host_check.cpp -o /tmp/embed_host_check
//     /tmp/embed_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../moldiff_amd/csrc/mdx_embed_args.h"

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static bool says(const char* why, const char* word) { return why && std::strstr(why, word); }

int main() {
  BoundsParams* p = (BoundsParams*)std::malloc(sizeof(BoundsParams));  // on the heap: a write past it is an AddressSanitizer report
  EXPECT(bounds_prepare(p, 0.01, 0.04, 0.06, 0.6, 256) == nullptr);
  EXPECT(p->tol12 == 0.01 && p->tol13 == 0.04 && p->tol14 == 0.06 && p->vdw_scale == 0.6 && p->na_cap == 256);
  EXPECT(std::fabs(p->ring_c0[0] - 0.5) < 1e-15 && std::fabs(p->ring_c0[1]) < 1e-15 && std::fabs(p->ring_c0[2] - (1.0 - std::sqrt(5.0)) / 4.0) < 1e-15);
  EXPECT(says(bounds_prepare(p, -0.01, 0.04, 0.06, 0.6, 256), "tol12"));
  EXPECT(says(bounds_prepare(p, 0.01, NAN, 0.06, 0.6, 256), "tol13"));
  EXPECT(says(bounds_prepare(p, 0.01, 0.04, 1.5, 0.6, 256), "tol14"));
  EXPECT(says(bounds_prepare(p, 0.01, 0.04, 0.06, 0.0, 256), "vdw_scale"));
  EXPECT(says(bounds_prepare(p, 0.01, 0.04, 0.06, 0.6, 0), "na_cap") && says(bounds_prepare(p, 0.01, 0.04, 0.06, 0.6, 257), "na_cap"));
  std::free(p);

  char ws[8];
  EXPECT(bounds_ws_bytes(3, 16) == 3u * 17u * 256u && bounds_ws_bytes(0, 256) == 0u);
  EXPECT(bounds_ws_bytes(32767, 256) == (size_t)32767 * 17u * 65536u);  // past 2^32
  EXPECT(bounds_ws_check(3, 16, ws, 3 * 17 * 256) == nullptr && says(bounds_ws_check(3, 16, ws, 3 * 17 * 256 - 1), "workspace"));
  EXPECT(says(bounds_ws_check(3, 16, nullptr, 1 << 20), "null") && bounds_ws_check(0, 16, ws, 0) == nullptr);

  EmbedParams* e = (EmbedParams*)std::malloc(sizeof(EmbedParams));
  const size_t need = (size_t)4 * 3 * EM_HIST_PER_ATOM * 32 * sizeof(double);
  EXPECT(embed_prepare(e, 4, 32, 3, 7u, 400, 4, 1e-3, 1.0, 0.1, need) == nullptr);
  EXPECT(e->n_confs == 3 && e->max_iters == 400 && e->max_attempts == 4 && e->seed == 7u && e->na_cap == 32 && e->viol_tol == 0.1);
  EXPECT(says(embed_prepare(e, 4, 32, 3, 7u, 400, 4, 1e-3, 1.0, 0.1, need - 1), "history"));
  EXPECT(embed_prepare(e, 0, 32, 3, 7u, 400, 4, 1e-3, 1.0, 0.1, 0) == nullptr);
  EXPECT(says(embed_prepare(e, 4, 32, 0, 7u, 400, 4, 1e-3, 1.0, 0.1, need), "n_confs"));
  EXPECT(says(embed_prepare(e, 4, 32, 3, 7u, -1, 4, 1e-3, 1.0, 0.1, need), "max_iters"));
  EXPECT(says(embed_prepare(e, 4, 32, 3, 7u, 400, 65, 1e-3, 1.0, 0.1, need), "max_attempts"));
  EXPECT(says(embed_prepare(e, 4, 32, 3, 7u, 400, 4, 0.0, 1.0, 0.1, need), "gtol"));
  EXPECT(says(embed_prepare(e, 4, 32, 3, 7u, 400, 4, 1e-3, 11.0, 0.1, need), "max_step"));
  EXPECT(says(embed_prepare(e, 4, 32, 3, 7u, 400, 4, 1e-3, 1.0, NAN, need), "viol_tol"));
  std::free(e);

  // the distance formulas: a right angle, a straight chain, and the cis / trans pair of a planar zigzag
  EXPECT(std::fabs(bounds_13(3.0, 4.0, 0.0) - 5.0) < 1e-15 && bounds_13(1.0, 2.0, -1.0) == 3.0);
  EXPECT(bounds_13(1.5, 1.1, -0.3) == bounds_13(1.1, 1.5, -0.3));
  double cis, trans;
  bounds_14(1.0, 1.0, 1.0, 0.0, 0.0, &cis, &trans);
  EXPECT(std::fabs(cis - 1.0) < 1e-15 && std::fabs(trans - std::sqrt(5.0)) < 1e-15);
  bounds_14(1.0, 2.0, 3.0, -1.0, -1.0, &cis, &trans);
  EXPECT(cis == 6.0 && trans == 6.0);
  bounds_14(1.5, 1.4, 1.1, -0.5, -1.0 / 3.0, &cis, &trans);
  EXPECT(cis > 0.0 && trans > cis && trans < 1.5 + 1.4 + 1.1);

  EXPECT(embed_u53(0u, 0u) == 0.0 && embed_u53(0xffffffffu, 0xffffffffu) == 1.0 - 1.1102230246251565e-16 && embed_u53(0x80000000u, 0u) == 0.5);
  EXPECT(embed_u53(0u, 64u) == 1.1102230246251565e-16 && embed_u53(32u, 0u) == 67108864.0 * 1.1102230246251565e-16);

  std::printf(failures ? "%d check(s) failed\n" : "embed_host_check ok\n", failures);
  return failures ? 1 : 0;
}
