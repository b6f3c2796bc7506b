// Host-side validation of mdx_mol_canon (mdx_canon.hip): the operands behind the shared compact-molecule prefix.  Plain C++ without
// HIP, so that it can be built on its own under a host sanitizer (tools/canon_host_check.cpp).  The atom labels live on the device and
// are the caller's word there; the Python wrappers check the host arrays they are given.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int CN_MAX_NODES = 1 << 20, CN_MAX_DEPTH = 64;
constexpr int CN_STATS = 5;  // = MDX_CANON_STATS of include/moldiff_hip.h

// The optional inputs and every output of one call.
struct CanonOperands {
  const float* atom_pos;      // or nullptr
  const int32_t* atom_label;  // or nullptr: the label is atom_type
  int32_t *rank, *orbit, *canon_atom_type, *canon_atom_label, *canon_bond_index, *canon_bond_type, *mol_stats;
  float* canon_pos;
  int64_t* cert_hash;
};

// -> nullptr, or the reason the call is refused
inline const char* canon_check(const CanonOperands& o, int32_t max_nodes) {
  if (!o.rank || !o.orbit || !o.canon_atom_type || !o.canon_bond_index || !o.canon_bond_type || !o.mol_stats || !o.cert_hash)
    return "null argument";
  if ((o.atom_label != nullptr) != (o.canon_atom_label != nullptr)) return "atom_label and canon_atom_label: both or neither";
  if ((o.atom_pos != nullptr) != (o.canon_pos != nullptr)) return "atom_pos and canon_pos: both or neither";
  if (max_nodes < 1 || max_nodes > CN_MAX_NODES) return "max_nodes must lie in 1 .. 2^20";
  return nullptr;
}
