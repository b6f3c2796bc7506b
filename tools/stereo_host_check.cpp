// Stand-alone check of the host-side validation of mdx_mol_stereo (moldiff_amd/csrc/mdx_stereo_args.h and the shared operand prefix of
// moldiff_amd/csrc/mdx_mol.h).  No HIP, no GPU; meant to be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/stereo_host_check.cpp -o /tmp/stereo_host_check
//     /tmp/stereo_host_check
//
// The validation reads no operand: every pointer below is a heap block of one element, so a dereference past it is an AddressSanitizer
// report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../moldiff_amd/csrc/mdx_mol.h"
#include "../moldiff_amd/csrc/mdx_stereo_args.h"

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
      ++failures;                                                    \
    }                                                                \
  } while (0)

int main() {
  int32_t* i32 = (int32_t*)std::malloc(sizeof(int32_t));
  float* f32 = (float*)std::malloc(sizeof(float));
  int64_t* i64 = (int64_t*)std::malloc(sizeof(int64_t));
  const StereoOperands full{f32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i64, i64};
  EXPECT(stereo_check(full, 0.1, 0.1, 1) == nullptr && stereo_check(full, 0.0, 0.0, 1 << 20) == nullptr);
  const char* why = stereo_check(full, 0.1, 0.1, 0);
  EXPECT(why && std::strstr(why, "max_nodes"));
  EXPECT(stereo_check(full, 0.1, 0.1, (1 << 20) + 1) && stereo_check(full, 0.1, 0.1, -1));
  EXPECT((why = stereo_check(full, -0.1, 0.1, 100)) && std::strstr(why, "flat_tol"));
  EXPECT((why = stereo_check(full, 1.0, 0.1, 100)) && std::strstr(why, "flat_tol"));
  EXPECT((why = stereo_check(full, std::nan(""), 0.1, 100)) && std::strstr(why, "flat_tol"));
  EXPECT((why = stereo_check(full, 0.1, 1.5, 100)) && std::strstr(why, "bond_tol"));
  EXPECT((why = stereo_check(full, 0.1, std::nan(""), 100)) && std::strstr(why, "bond_tol"));
  EXPECT(stereo_check(full, 0.1, INFINITY, 100) != nullptr);
  StereoOperands o = full;
  o.atom_label = nullptr;
  EXPECT(stereo_check(o, 0.1, 0.1, 100) == nullptr);  // the one optional operand
  o = full, o.atom_pos = nullptr;
  EXPECT((why = stereo_check(o, 0.1, 0.1, 100)) && std::strstr(why, "null"));
  const int32_t* StereoOperands::*inputs[] = {&StereoOperands::rank, &StereoOperands::canon_status};
  for (auto member : inputs) {
    o = full, o.*member = nullptr;
    EXPECT((why = stereo_check(o, 0.1, 0.1, 100)) && std::strstr(why, "null"));
  }
  int32_t* StereoOperands::*outputs[] = {&StereoOperands::canon_tetra, &StereoOperands::canon_bond_stereo, &StereoOperands::mirror_tetra,
                                         &StereoOperands::mirror_bond_stereo, &StereoOperands::stereo_rank, &StereoOperands::atom_tetra,
                                         &StereoOperands::bond_stereo, &StereoOperands::mol_stats};
  for (auto member : outputs) {
    o = full, o.*member = nullptr;
    EXPECT((why = stereo_check(o, 0.1, 0.1, 100)) && std::strstr(why, "null"));
  }
  o = full, o.stereo_hash = nullptr;
  EXPECT(stereo_check(o, 0.1, 0.1, 100) != nullptr);
  o = full, o.mirror_hash = nullptr;
  EXPECT(stereo_check(o, 0.1, 0.1, 100) != nullptr);
  // the shared prefix
  MolArrays a;
  EXPECT(mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, 10, i32, i32, 7, nullptr) == nullptr);
  EXPECT(a.bond_j == i32 + 7 && a.N_cap == 10 && a.E_cap == 7 && a.select == nullptr);
  EXPECT((why = mol_arrays_fill(&a, 3, i32, nullptr, i32, i32, i32, 10, i32, i32, 7, nullptr)) && std::strstr(why, "null"));
  EXPECT((why = mol_arrays_fill(&a, -1, i32, i32, i32, i32, i32, 10, i32, i32, 7, nullptr)) && std::strstr(why, "negative"));
  std::free(i32), std::free(f32), std::free(i64);
  std::printf(failures ? "%d FAILED\n" : "stereo_host_check ok\n", failures);
  return failures != 0;
}
