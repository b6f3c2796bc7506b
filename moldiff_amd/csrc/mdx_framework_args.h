// Host-side validation of mdx_mol_framework (mdx_framework.hip): the operands behind the shared compact-molecule prefix.  Plain C++
// without HIP, so that it can be built on its own under a host sanitizer (tools/framework_host_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int FW_STATS = 10;  // = MDX_FW_STATS of include/moldiff_hip.h
constexpr int FW_MODE_EXO = 1, FW_MODE_GENERIC = 2, FW_MAX_BINS = 16;

// The optional input, the ring data and every output of one call.
struct FrameworkOperands {
  const float* atom_pos;                         // or nullptr
  const int32_t *bond_ring_min, *ring_status;    // as mdx_mol_rings wrote them for the same arrays
  int32_t *atom_role, *atom_system, *bond_role, *mol_stats, *sys_hist;
  int32_t *fw_atom_type, *fw_atom_map, *fw_bond_index, *fw_bond_type;
  int32_t *sys_atom_ptr, *sys_bond_ptr, *sys_n_atoms, *sys_n_bonds;
  int32_t *sys_atom_type, *sys_atom_map, *sys_bond_index, *sys_bond_type;
  float *fw_pos, *sys_pos;                       // both iff atom_pos
};

// -> nullptr, or the reason the call is refused
inline const char* framework_check(const FrameworkOperands& o, int32_t mode, int32_t sys_bins) {
  if (!o.bond_ring_min || !o.ring_status || !o.atom_role || !o.atom_system || !o.bond_role || !o.mol_stats || !o.sys_hist ||
      !o.fw_atom_type || !o.fw_atom_map || !o.fw_bond_index || !o.fw_bond_type || !o.sys_atom_ptr || !o.sys_bond_ptr || !o.sys_n_atoms ||
      !o.sys_n_bonds || !o.sys_atom_type || !o.sys_atom_map || !o.sys_bond_index || !o.sys_bond_type)
    return "null argument";
  if ((o.atom_pos != nullptr) != (o.fw_pos != nullptr) || (o.atom_pos != nullptr) != (o.sys_pos != nullptr))
    return "atom_pos, fw_pos and sys_pos: all or none";
  if (mode < 0 || mode > (FW_MODE_EXO | FW_MODE_GENERIC)) return "mode has bits above 1";
  if (sys_bins < 1 || sys_bins > FW_MAX_BINS) return "sys_bins must lie in 1 .. 16";
  return nullptr;
}
