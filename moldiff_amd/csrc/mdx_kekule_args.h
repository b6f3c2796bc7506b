// Host-side preparation of mdx_mol_kekulize (mdx_kekule.hip): validation of the caller's three chemistry tables and their packing into
// the words that travel as kernel arguments.  Plain C++ without HIP, so that it can be built on its own under a host sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int KK_MAX_ELEMENTS = 32, KK_MAX_BOND_TYPES = 16, KK_MAX_STEPS = 1 << 20, KK_MAX_VALENCE = 64;
constexpr int KK_STATS = 11;  // = MDX_KEKULE_STATS of include/moldiff_hip.h

enum { KK_PREP_OK = 0, KK_PREP_ARG = 1 };  // = MDX_OK, MDX_ERR_ARG

// One byte per class and table: V in valence[c] & 0xff, Vc in valence[c] >> 8.  A class at or above num_element holds 0 / 0 and is
// not flexible: such an atom has no room for anything.
struct KekuleTable {
  uint16_t valence[KK_MAX_ELEMENTS];
  uint32_t flexible;
};

// Validates the HOST tables and fills `t`.  On failure *why names the cause and `t` may be partly written.
inline int kekule_prepare(KekuleTable* t, const int32_t* normal_valence, const int32_t* charged_valence, uint32_t flexible,
                          int32_t num_element, int32_t num_bond_types, int32_t max_steps, const char** why) {
  if (num_element < 1 || num_element > KK_MAX_ELEMENTS || num_bond_types < 1 || num_bond_types > KK_MAX_BOND_TYPES)
    return *why = "num_element must lie in 1 .. 32 and num_bond_types in 1 .. 16", KK_PREP_ARG;
  if (max_steps < 1 || max_steps > KK_MAX_STEPS) return *why = "max_steps must lie in 1 .. 2^20", KK_PREP_ARG;
  if (!normal_valence || !charged_valence) return *why = "null argument", KK_PREP_ARG;
  if (num_element < 32 && (flexible >> num_element) != 0u) return *why = "flexible names a class >= num_element", KK_PREP_ARG;
  for (int c = 0; c < KK_MAX_ELEMENTS; ++c) {
    const int32_t v = c < num_element ? normal_valence[c] : 0, vc = c < num_element ? charged_valence[c] : 0;
    if (v < 0 || v > KK_MAX_VALENCE || vc < 0 || vc > KK_MAX_VALENCE)
      return *why = "normal_valence and charged_valence must lie in 0 .. 64", KK_PREP_ARG;
    t->valence[c] = (uint16_t)(v | vc << 8);
  }
  t->flexible = flexible;
  return KK_PREP_OK;
}
