// Stand-alone check of the host-side preparation of mdx_mol_kekulize (moldiff_amd/csrc/mdx_kekule_args.h): validation of the three
// chemistry tables and their packing.  No HIP, no GPU; meant to be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/kekule_host_check.cpp -o /tmp/kekule_host_check
//     /tmp/kekule_host_check
//
// The tables are heap-allocated at exactly num_element entries, so a read past them is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moldiff_amd/csrc/mdx_kekule_args.h"

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static int prep(KekuleTable* t, const std::vector<int32_t>& v, const std::vector<int32_t>& vc, uint32_t flexible, int ne, int nbt, int steps,
                const char** why) {
  int32_t* a = (int32_t*)std::malloc(v.size() * sizeof(int32_t) + 1);
  int32_t* b = (int32_t*)std::malloc(vc.size() * sizeof(int32_t) + 1);
  std::memcpy(a, v.data(), v.size() * sizeof(int32_t));
  std::memcpy(b, vc.data(), vc.size() * sizeof(int32_t));
  const int rc = kekule_prepare(t, a, b, flexible, ne, nbt, steps, why);
  std::free(a);
  std::free(b);
  return rc;
}

int main() {
  const std::vector<int32_t> V = {4, 3, 2, 1, 3, 2, 1}, Vc = {0, 4, 0, 0, 0, 3, 0};
  KekuleTable t;
  const char* why = "";
  EXPECT(prep(&t, V, Vc, 2u, 7, 4, 1 << 16, &why) == KK_PREP_OK);
  for (int c = 0; c < KK_MAX_ELEMENTS; ++c) EXPECT(t.valence[c] == (c < 7 ? (uint16_t)(V[c] | Vc[c] << 8) : 0));
  EXPECT(t.flexible == 2u);
  EXPECT(prep(&t, V, Vc, 1u << 6, 7, 4, 1, &why) == KK_PREP_OK);
  EXPECT(prep(&t, V, Vc, 1u << 7, 7, 4, 1, &why) == KK_PREP_ARG && std::strstr(why, "flexible"));
  EXPECT(prep(&t, V, Vc, 2u, 0, 4, 1, &why) == KK_PREP_ARG && prep(&t, V, Vc, 2u, 33, 4, 1, &why) == KK_PREP_ARG);
  EXPECT(prep(&t, V, Vc, 2u, 7, 0, 1, &why) == KK_PREP_ARG && prep(&t, V, Vc, 2u, 7, 17, 1, &why) == KK_PREP_ARG);
  EXPECT(prep(&t, V, Vc, 2u, 7, 4, 0, &why) == KK_PREP_ARG && std::strstr(why, "max_steps"));
  EXPECT(prep(&t, V, Vc, 2u, 7, 4, (1 << 20) + 1, &why) == KK_PREP_ARG && prep(&t, V, Vc, 2u, 7, 4, 1 << 20, &why) == KK_PREP_OK);
  std::vector<int32_t> bad = V;
  bad[6] = 65;
  EXPECT(prep(&t, bad, Vc, 2u, 7, 4, 1, &why) == KK_PREP_ARG && std::strstr(why, "0 .. 64"));
  bad[6] = -1;
  EXPECT(prep(&t, V, bad, 2u, 7, 4, 1, &why) == KK_PREP_ARG);
  bad[6] = 64;
  EXPECT(prep(&t, bad, bad, 2u, 7, 4, 1, &why) == KK_PREP_OK && t.valence[6] == (64 | 64 << 8));
  EXPECT(kekule_prepare(&t, nullptr, Vc.data(), 2u, 7, 4, 1, &why) == KK_PREP_ARG && std::strstr(why, "null"));
  // 32 classes: every bit of flexible is legal and every entry is read
  const std::vector<int32_t> wide(32, 5);
  EXPECT(prep(&t, wide, wide, 0xffffffffu, 32, 16, 1, &why) == KK_PREP_OK && t.valence[31] == (5 | 5 << 8) && t.flexible == 0xffffffffu);
  std::printf(failures ? "%d FAILED\n" : "kekule_host_check ok\n", failures);
  return failures != 0;
}
