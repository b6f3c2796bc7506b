// Stand-alone check of the host-side validation of mdx_mol_canon (moldiff_amd/csrc/mdx_canon_args.h and the shared operand prefix of
// moldiff_amd/csrc/mdx_mol.h).  No HIP, no GPU; meant to be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/canon_host_check.cpp -o /tmp/canon_host_check
//     /tmp/canon_host_check
//
// The validation reads no operand: every pointer below is a heap block of one element, so a dereference past it is an AddressSanitizer
// report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../moldiff_amd/csrc/mdx_canon_args.h"
#include "../moldiff_amd/csrc/mdx_mol.h"

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
  const CanonOperands full{f32, i32, i32, i32, i32, i32, i32, i32, i32, f32, i64};
  EXPECT(canon_check(full, 1) == nullptr && canon_check(full, 1 << 20) == nullptr && canon_check(full, 65536) == nullptr);
  const char* why = canon_check(full, 0);
  EXPECT(why && std::strstr(why, "max_nodes"));
  EXPECT(canon_check(full, (1 << 20) + 1) && canon_check(full, -1));
  CanonOperands o = full;
  o.atom_pos = nullptr, o.canon_pos = nullptr, o.atom_label = nullptr, o.canon_atom_label = nullptr;
  EXPECT(canon_check(o, 100) == nullptr);  // both optional inputs absent
  o = full, o.canon_pos = nullptr;
  EXPECT((why = canon_check(o, 100)) && std::strstr(why, "atom_pos"));
  o = full, o.atom_pos = nullptr;
  EXPECT(canon_check(o, 100) != nullptr);
  o = full, o.canon_atom_label = nullptr;
  EXPECT((why = canon_check(o, 100)) && std::strstr(why, "atom_label"));
  o = full, o.atom_label = nullptr;
  EXPECT(canon_check(o, 100) != nullptr);
  int32_t* CanonOperands::*required[] = {&CanonOperands::rank, &CanonOperands::orbit, &CanonOperands::canon_atom_type,
                                         &CanonOperands::canon_bond_index, &CanonOperands::canon_bond_type, &CanonOperands::mol_stats};
  for (auto member : required) {
    o = full, o.*member = nullptr;
    EXPECT((why = canon_check(o, 100)) && std::strstr(why, "null"));
  }
  o = full, o.cert_hash = nullptr;
  EXPECT((why = canon_check(o, 100)) && std::strstr(why, "null"));
  // the shared prefix
  MolArrays a;
  EXPECT(mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, 10, i32, i32, 7, nullptr) == nullptr);
  EXPECT(a.bond_j == i32 + 7 && a.N_cap == 10 && a.E_cap == 7 && a.select == nullptr);
  EXPECT((why = mol_arrays_fill(&a, 3, nullptr, i32, i32, i32, i32, 10, i32, i32, 7, nullptr)) && std::strstr(why, "null"));
  EXPECT((why = mol_arrays_fill(&a, -1, i32, i32, i32, i32, i32, 10, i32, i32, 7, nullptr)) && std::strstr(why, "negative"));
  EXPECT(mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, -1, i32, i32, 7, nullptr) && mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, 1, i32, i32, -7, i32));
  std::free(i32), std::free(f32), std::free(i64);
  std::printf(failures ? "%d FAILED\n" : "canon_host_check ok\n", failures);
  return failures != 0;
}
