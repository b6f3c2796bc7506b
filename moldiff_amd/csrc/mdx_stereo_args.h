// Host-side validation of mdx_mol_stereo (mdx_stereo.hip): the operands behind the shared compact-molecule prefix.  Plain C++ without
// HIP, so that it can be built on its own under a host sanitizer (tools/stereo_host_check.cpp).  rank, canon_status and the atom labels
// live on the device and are the caller's word there; the kernel keeps every index it forms from them inside the molecule.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

constexpr int ST_MAX_NODES = 1 << 20;
constexpr int ST_STATS = 9;  // = MDX_STEREO_STATS of include/moldiff_hip.h

// The inputs behind the compact arrays and every output of one call.
struct StereoOperands {
  const float* atom_pos;
  const int32_t* atom_label;  // or nullptr: the label is atom_type
  const int32_t *rank, *canon_status;
  int32_t *canon_tetra, *canon_bond_stereo, *mirror_tetra, *mirror_bond_stereo, *stereo_rank, *atom_tetra, *bond_stereo, *mol_stats;
  int64_t *stereo_hash, *mirror_hash;
};

// -> nullptr, or the reason the call is refused
inline const char* stereo_check(const StereoOperands& o, double flat_tol, double bond_tol, int32_t max_nodes) {
  if (!o.atom_pos || !o.rank || !o.canon_status || !o.canon_tetra || !o.canon_bond_stereo || !o.mirror_tetra || !o.mirror_bond_stereo || !o.stereo_rank || !o.atom_tetra ||
      !o.bond_stereo || !o.mol_stats || !o.stereo_hash || !o.mirror_hash)
    return "null argument";
  if (!(flat_tol >= 0.0 && flat_tol < 1.0)) return "flat_tol must lie in [0, 1)";  // NaN fails both
  if (!(bond_tol >= 0.0 && bond_tol < 1.0)) return "bond_tol must lie in [0, 1)";
  if (max_nodes < 1 || max_nodes > ST_MAX_NODES) return "max_nodes must lie in 1 .. 2^20";
  return nullptr;
}
