// Host-side preparation of mdx_mol_hydrogens (mdx_hydrogens.hip): validation of the caller's X-H length table, the planar mask and the
// two tolerances, and their packing into the block that travels as kernel arguments.  Plain C++ without HIP, so that it can be built
// on its own under a host sanitizer (tools/hydrogens_host_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int HY_MAX_ELEMENTS = 32, HY_MAX_BOND_TYPES = 16, HY_MAX_H = 4;
constexpr int HY_STATS = 7;  // = MDX_HYDROGENS_STATS of include/moldiff_hip.h
constexpr double HY_MAX_LENGTH = 4.0;

enum { HY_PREP_OK = 0, HY_PREP_ARG = 1 };  // = MDX_OK, MDX_ERR_ARG

// The length per class in Angstrom; a class at or above num_element holds 0 and carries no hydrogen.
struct HydrogenTable {
  double length[HY_MAX_ELEMENTS];
  uint32_t planar;
  double deg_tol, clash_tol;
};

// the caller's device operands beside the compact arrays: what is read, then what is written
struct HydrogenOperands {
  const float* atom_pos;
  const int32_t *n_h, *order;
  double* h_pos;
  int32_t *h_count, *atom_flag, *mol_stats;
  double* min_contact;
};

inline const char* hydrogens_check(const HydrogenOperands& o) {
  if (!o.atom_pos || !o.n_h || !o.order || !o.h_pos || !o.h_count || !o.atom_flag || !o.mol_stats || !o.min_contact) return "null argument";
  return nullptr;
}

// Validates the HOST table and the scalars and fills `t`.  On failure *why names the cause and `t` may be partly written.
inline int hydrogens_prepare(HydrogenTable* t, const double* xh_length, uint32_t planar_mask, int32_t num_element, int32_t num_bond_types,
                             double deg_tol, double clash_tol, const char** why) {
  if (num_element < 1 || num_element > HY_MAX_ELEMENTS || num_bond_types < 1 || num_bond_types > HY_MAX_BOND_TYPES)
    return *why = "num_element must lie in 1 .. 32 and num_bond_types in 1 .. 16", HY_PREP_ARG;
  if (!xh_length) return *why = "null argument", HY_PREP_ARG;
  if (num_element < 32 && (planar_mask >> num_element) != 0u) return *why = "planar_mask names a class >= num_element", HY_PREP_ARG;
  if (!(deg_tol > 0.0 && deg_tol < 1.0)) return *why = "deg_tol must lie in (0, 1)", HY_PREP_ARG;  // NaN fails
  if (!(clash_tol >= 0.0 && clash_tol <= 1.0e3)) return *why = "clash_tol must lie in [0, 1000]", HY_PREP_ARG;
  for (int c = 0; c < HY_MAX_ELEMENTS; ++c) {
    const double l = c < num_element ? xh_length[c] : 0.0;
    if (c < num_element && !(l > 0.0 && l <= HY_MAX_LENGTH)) return *why = "xh_length must lie in (0, 4]", HY_PREP_ARG;
    t->length[c] = l;
  }
  t->planar = planar_mask, t->deg_tol = deg_tol, t->clash_tol = clash_tol;
  return HY_PREP_OK;
}
