// Stand-alone check of the host-side validation of mdx_mol_framework (moldiff_amd/csrc/mdx_framework_args.h and the shared operand
// prefix of moldiff_amd/csrc/mdx_mol.h).  No HIP, no GPU; meant to be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/framework_host_check.cpp -o /tmp/framework_host_check
//     /tmp/framework_host_check
//
// The validation reads no operand: every pointer below is a heap block of one element, so a dereference past it is an AddressSanitizer
// report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../moldiff_amd/csrc/mdx_framework_args.h"
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
  const FrameworkOperands full{f32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, f32};
  for (int mode = 0; mode < 4; ++mode) EXPECT(framework_check(full, mode, 1) == nullptr && framework_check(full, mode, 16) == nullptr);
  const char* why = framework_check(full, 4, 8);
  EXPECT(why && std::strstr(why, "mode"));
  EXPECT(framework_check(full, -1, 8) && framework_check(full, 1 << 30, 8));
  EXPECT((why = framework_check(full, 0, 0)) && std::strstr(why, "sys_bins"));
  EXPECT(framework_check(full, 0, 17) && framework_check(full, 0, -3));
  FrameworkOperands o = full;
  o.atom_pos = nullptr, o.fw_pos = nullptr, o.sys_pos = nullptr;
  EXPECT(framework_check(o, 3, 8) == nullptr);  // no positions at all
  o = full, o.fw_pos = nullptr;
  EXPECT((why = framework_check(o, 0, 8)) && std::strstr(why, "atom_pos"));
  o = full, o.sys_pos = nullptr;
  EXPECT(framework_check(o, 0, 8) != nullptr);
  o = full, o.atom_pos = nullptr;
  EXPECT(framework_check(o, 0, 8) != nullptr);
  o = full, o.atom_pos = nullptr, o.fw_pos = nullptr;
  EXPECT(framework_check(o, 0, 8) != nullptr);
  int32_t* FrameworkOperands::*outputs[] = {
      &FrameworkOperands::atom_role,     &FrameworkOperands::atom_system,  &FrameworkOperands::bond_role,    &FrameworkOperands::mol_stats,
      &FrameworkOperands::sys_hist,      &FrameworkOperands::fw_atom_type, &FrameworkOperands::fw_atom_map,  &FrameworkOperands::fw_bond_index,
      &FrameworkOperands::fw_bond_type,  &FrameworkOperands::sys_atom_ptr, &FrameworkOperands::sys_bond_ptr, &FrameworkOperands::sys_n_atoms,
      &FrameworkOperands::sys_n_bonds,   &FrameworkOperands::sys_atom_type, &FrameworkOperands::sys_atom_map, &FrameworkOperands::sys_bond_index,
      &FrameworkOperands::sys_bond_type};
  for (auto member : outputs) {
    o = full, o.*member = nullptr;
    EXPECT((why = framework_check(o, 0, 8)) && std::strstr(why, "null"));
  }
  o = full, o.bond_ring_min = nullptr;
  EXPECT((why = framework_check(o, 0, 8)) && std::strstr(why, "null"));
  o = full, o.ring_status = nullptr;
  EXPECT((why = framework_check(o, 0, 8)) && std::strstr(why, "null"));
  // the shared prefix
  MolArrays a;
  EXPECT(mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, 10, i32, i32, 7, nullptr) == nullptr);
  EXPECT((why = mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, 10, i32, nullptr, 7, nullptr)) && std::strstr(why, "null"));
  EXPECT((why = mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, 10, i32, i32, -7, nullptr)) && std::strstr(why, "negative"));
  std::free(i32), std::free(f32);
  std::printf(failures ? "%d FAILED\n" : "framework_host_check ok\n", failures);
  return failures != 0;
}
