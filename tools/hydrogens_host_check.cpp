// Stand-alone check of the host-side preparation of mdx_mol_hydrogens (moldiff_amd/csrc/mdx_hydrogens_args.h and the operand check of
// mdx_mol.h): validation of the length table, the planar mask and the two tolerances, and their packing.  No HIP, no GPU; meant to be
// built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/hydrogens_host_check.cpp -o /tmp/hydrogens_host_check
//     /tmp/hydrogens_host_check
//
// The table is heap-allocated at exactly num_element entries, so a read past it is an AddressSanitizer report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moldiff_amd/csrc/mdx_hydrogens_args.h"
#include "../moldiff_amd/csrc/mdx_mol.h"

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static int prep(HydrogenTable* t, const std::vector<double>& len, uint32_t planar, int ne, int nbt, double deg, double clash, const char** why) {
  double* a = (double*)std::malloc(len.size() * sizeof(double) + 1);
  std::memcpy(a, len.data(), len.size() * sizeof(double));
  const int rc = hydrogens_prepare(t, a, planar, ne, nbt, deg, clash, why);
  std::free(a);
  return rc;
}

int main() {
  const std::vector<double> L = {1.09, 1.01, 0.96, 0.92, 1.42, 1.34, 1.27};
  HydrogenTable t;
  const char* why = "";
  EXPECT(prep(&t, L, 2u, 7, 4, 1e-3, 1.5, &why) == HY_PREP_OK);
  for (int c = 0; c < HY_MAX_ELEMENTS; ++c) EXPECT(t.length[c] == (c < 7 ? L[c] : 0.0));
  EXPECT(t.planar == 2u && t.deg_tol == 1e-3 && t.clash_tol == 1.5);
  // the planar mask
  EXPECT(prep(&t, L, 1u << 6, 7, 4, 1e-3, 1.5, &why) == HY_PREP_OK);
  EXPECT(prep(&t, L, 1u << 7, 7, 4, 1e-3, 1.5, &why) == HY_PREP_ARG && std::strstr(why, "planar_mask"));
  // the sizes
  EXPECT(prep(&t, L, 2u, 0, 4, 1e-3, 1.5, &why) == HY_PREP_ARG && prep(&t, L, 2u, 33, 4, 1e-3, 1.5, &why) == HY_PREP_ARG);
  EXPECT(prep(&t, L, 2u, 7, 0, 1e-3, 1.5, &why) == HY_PREP_ARG && prep(&t, L, 2u, 7, 17, 1e-3, 1.5, &why) == HY_PREP_ARG);
  EXPECT(std::strstr(why, "num_element"));
  // the tolerances
  EXPECT(prep(&t, L, 2u, 7, 4, 0.0, 1.5, &why) == HY_PREP_ARG && std::strstr(why, "deg_tol"));
  EXPECT(prep(&t, L, 2u, 7, 4, 1.0, 1.5, &why) == HY_PREP_ARG && prep(&t, L, 2u, 7, 4, -1e-3, 1.5, &why) == HY_PREP_ARG);
  EXPECT(prep(&t, L, 2u, 7, 4, std::nan(""), 1.5, &why) == HY_PREP_ARG);
  EXPECT(prep(&t, L, 2u, 7, 4, 1e-3, -0.5, &why) == HY_PREP_ARG && std::strstr(why, "clash_tol"));
  EXPECT(prep(&t, L, 2u, 7, 4, 1e-3, 1000.5, &why) == HY_PREP_ARG && prep(&t, L, 2u, 7, 4, 1e-3, std::nan(""), &why) == HY_PREP_ARG);
  EXPECT(prep(&t, L, 2u, 7, 4, 1e-3, 0.0, &why) == HY_PREP_OK && prep(&t, L, 2u, 7, 4, 1e-3, 1000.0, &why) == HY_PREP_OK);
  // the lengths
  std::vector<double> bad = L;
  bad[6] = 0.0;
  EXPECT(prep(&t, bad, 2u, 7, 4, 1e-3, 1.5, &why) == HY_PREP_ARG && std::strstr(why, "xh_length"));
  bad[6] = 4.5;
  EXPECT(prep(&t, bad, 2u, 7, 4, 1e-3, 1.5, &why) == HY_PREP_ARG);
  bad[6] = -1.0;
  EXPECT(prep(&t, bad, 2u, 7, 4, 1e-3, 1.5, &why) == HY_PREP_ARG);
  bad[6] = std::nan("");
  EXPECT(prep(&t, bad, 2u, 7, 4, 1e-3, 1.5, &why) == HY_PREP_ARG);
  bad[6] = 4.0;
  EXPECT(prep(&t, bad, 2u, 7, 4, 1e-3, 1.5, &why) == HY_PREP_OK && t.length[6] == 4.0);
  EXPECT(hydrogens_prepare(&t, nullptr, 2u, 7, 4, 1e-3, 1.5, &why) == HY_PREP_ARG && std::strstr(why, "null"));
  // 32 classes: every bit of the mask is legal and every entry is read
  const std::vector<double> wide(32, 1.5);
  EXPECT(prep(&t, wide, 0xffffffffu, 32, 16, 0.5, 1.5, &why) == HY_PREP_OK && t.length[31] == 1.5 && t.planar == 0xffffffffu);
  // the device operands: each one missing is refused
  float pos = 0.f;
  double d = 0.0;
  int32_t i = 0;
  const HydrogenOperands full = {&pos, &i, &i, &d, &i, &i, &i, &d};
  EXPECT(hydrogens_check(full) == nullptr);
  for (int k = 0; k < 8; ++k) {
    HydrogenOperands o = full;
    if (k == 0) o.atom_pos = nullptr;
    if (k == 1) o.n_h = nullptr;
    if (k == 2) o.order = nullptr;
    if (k == 3) o.h_pos = nullptr;
    if (k == 4) o.h_count = nullptr;
    if (k == 5) o.atom_flag = nullptr;
    if (k == 6) o.mol_stats = nullptr;
    if (k == 7) o.min_contact = nullptr;
    const char* w = hydrogens_check(o);
    EXPECT(w && std::strstr(w, "null"));
  }
  // the compact arrays: null operands and negative sizes
  MolArrays m;
  EXPECT(mol_arrays_fill(&m, 1, &i, &i, &i, &i, &i, 1, &i, &i, 1, nullptr) == nullptr && m.bond_j == &i + 1);
  EXPECT(mol_arrays_fill(&m, 1, nullptr, &i, &i, &i, &i, 1, &i, &i, 1, nullptr) != nullptr);
  EXPECT(mol_arrays_fill(&m, -1, &i, &i, &i, &i, &i, 1, &i, &i, 1, nullptr) != nullptr);
  EXPECT(mol_arrays_fill(&m, 1, &i, &i, &i, &i, &i, -1, &i, &i, 1, nullptr) != nullptr);
  EXPECT(mol_arrays_fill(&m, 1, &i, &i, &i, &i, &i, 1, &i, &i, -1, nullptr) != nullptr);
  std::printf(failures ? "%d FAILED\n" : "hydrogens_host_check ok\n", failures);
  return failures != 0;
}
