// Host-side preparation of mdx_mol_groups (mdx_groups.hip): validation of the caller's pattern table and its translation into the
// words the kernel reads.  Plain C++ without HIP, so that it can be built on its own under a host sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int GP_ATOMS = 8, GP_BONDS = 12, GP_PATTERNS = 32, GP_RECORD = 90;  // = MDX_GROUPS_* of include/moldiff_hip.h
constexpr int GP_MAX_ELEMENTS = 32, GP_MAX_BOND_TYPES = 16, GP_MAX_STEPS = 1 << 20, GP_MAX_VALENCE = 64;
constexpr int GP_ANY_RING = 0x7f;
constexpr int GP_WORDS = 32;                           // device words per pattern, and of the valence table in front of them
constexpr int GP_TABLE_WORDS = GP_WORDS * (1 + GP_PATTERNS);

// Device words of pattern p, at table[GP_WORDS * (1 + p)]; table[0 .. 31] = normal_valence.  With k a pattern atom:
//   [0]        number of atoms
//   [1 + k]    elem_mask
//   [9 + k]    deg_mask | h_mask << 8 | rsize_mask << 13 | arom << 20 | parent << 22 | first closure << 25 | closures << 28
//   [16 + k]   k > 0: the bond to the parent (the earliest pattern neighbour): type_mask | rsize_mask << 17
//   [24 + c]   closure c (the bonds of atom k to earlier atoms other than its parent, in the order of k): the earlier atom |
//              rsize_mask << 3 | type_mask << 10
enum { GP_PREP_OK = 0, GP_PREP_ARG = 1 };  // = MDX_OK, MDX_ERR_ARG

inline size_t groups_ws_bytes(int32_t P) {
  const int p = P < 1 ? 1 : P > GP_PATTERNS ? GP_PATTERNS : P;
  return sizeof(uint32_t) * GP_WORDS * (size_t)(1 + p);
}

// Validates the HOST tables and fills table[0 .. 32 * (1 + P)); *needs_rings = some rsize_mask differs from 0x7f.  On failure *why
// names the cause and `table` may be partly written.
inline int groups_prepare(uint32_t* table, const int32_t* normal_valence, const int32_t* patterns, int32_t P, int32_t num_element,
                          int32_t num_bond_types, bool* needs_rings, const char** why) {
  if (num_element < 1 || num_element > GP_MAX_ELEMENTS || num_bond_types < 1 || num_bond_types > GP_MAX_BOND_TYPES)
    return *why = "num_element must lie in 1 .. 32 and num_bond_types in 1 .. 16", GP_PREP_ARG;
  if (P < 1 || P > GP_PATTERNS) return *why = "a pattern set holds 1 .. 32 patterns", GP_PREP_ARG;
  for (int c = 0; c < GP_WORDS; ++c) {
    const int32_t v = c < num_element ? normal_valence[c] : 0;
    if (v < 0 || v > GP_MAX_VALENCE) return *why = "normal_valence must lie in 0 .. 64", GP_PREP_ARG;
    table[c] = (uint32_t)v;
  }
  const uint32_t elem_all = num_element == 32 ? 0xffffffffu : (1u << num_element) - 1u;
  const uint32_t type_all = ((1u << num_bond_types) - 1u) << 1;  // bits 1 .. num_bond_types
  *needs_rings = false;
  for (int p = 0; p < P; ++p) {
    const int32_t* r = patterns + (size_t)GP_RECORD * p;
    uint32_t* w = table + GP_WORDS * (1 + p);
    for (int k = 0; k < GP_WORDS; ++k) w[k] = 0u;
    const int na = r[0], nb = r[1];
    if (na < 1 || na > GP_ATOMS || nb < 0 || nb > GP_BONDS) return *why = "a pattern has 1 .. 8 atoms and 0 .. 12 bonds", GP_PREP_ARG;
    w[0] = (uint32_t)na;
    for (int k = 0; k < na; ++k) {
      const int32_t* a = r + 2 + 5 * k;
      const uint32_t em = (uint32_t)a[0];
      if (em == 0u || (em & ~elem_all) != 0u) return *why = "elem_mask is empty or names a class >= num_element", GP_PREP_ARG;
      if (a[1] < 1 || a[1] > 0xff || a[2] < 1 || a[2] > 0x1f || a[3] < 1 || a[3] > GP_ANY_RING || a[4] < 0 || a[4] > 2)
        return *why = "a pattern atom's deg_mask, h_mask, rsize_mask or arom is out of range", GP_PREP_ARG;
      if (a[3] != GP_ANY_RING) *needs_rings = true;
      w[1 + k] = em;
      w[9 + k] = (uint32_t)a[1] | (uint32_t)a[2] << 8 | (uint32_t)a[3] << 13 | (uint32_t)a[4] << 20;
    }
    // bond_of[i][j], i < j: 1 + the bond's index
    int bond_of[GP_ATOMS][GP_ATOMS] = {};
    for (int e = 0; e < nb; ++e) {
      const int32_t* b = r + 42 + 4 * e;
      if (b[0] < 0 || b[0] >= na || b[1] < 0 || b[1] >= na || b[0] == b[1])
        return *why = "a pattern bond's atom index is outside the pattern, or the bond joins an atom to itself", GP_PREP_ARG;
      const uint32_t tm = (uint32_t)b[2];
      if (tm == 0u || (tm & ~type_all) != 0u) return *why = "type_mask is empty or names a type outside 1 .. num_bond_types", GP_PREP_ARG;
      if (b[3] < 1 || b[3] > GP_ANY_RING) return *why = "a pattern bond's rsize_mask is out of range", GP_PREP_ARG;
      if (b[3] != GP_ANY_RING) *needs_rings = true;
      const int i = b[0] < b[1] ? b[0] : b[1], j = b[0] < b[1] ? b[1] : b[0];
      if (bond_of[i][j]) return *why = "two pattern bonds between the same pair of atoms", GP_PREP_ARG;
      bond_of[i][j] = 1 + e;
    }
    int closures = 0;
    for (int k = 1; k < na; ++k) {
      int parent = -1, first = closures, count = 0;
      for (int i = 0; i < k; ++i) {
        if (!bond_of[i][k]) continue;
        const int32_t* b = r + 42 + 4 * (bond_of[i][k] - 1);
        if (parent < 0) {
          parent = i;
          w[16 + k] = (uint32_t)b[2] | (uint32_t)b[3] << 17;
        } else {
          if (closures >= 7) return *why = "a pattern bond table that cannot occur", GP_PREP_ARG;  // 12 bonds leave at most 7
          w[24 + closures++] = (uint32_t)i | (uint32_t)b[3] << 3 | (uint32_t)b[2] << 10;
          ++count;
        }
      }
      if (parent < 0) return *why = "pattern atoms are not ordered: an atom k > 0 has no bond to an earlier atom", GP_PREP_ARG;
      w[9 + k] |= (uint32_t)parent << 22 | (uint32_t)first << 25 | (uint32_t)count << 28;
    }
  }
  return GP_PREP_OK;
}
