// Parameter block of mol_local3d_kernel (mdx_local3d.hip) and its host-side preparation: validation of the caller's pattern table
// and bins, canonical pattern keys, histogram layout.  Plain C++ without HIP, so that tools/local3d_host_check.cpp can build it on
// its own under a host sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mdx_mol.h"

constexpr int L3_MAX_ROWS = 64;        // pattern rows per kind (the key table lives in LDS)
constexpr int L3_LDS_ATOMS = 512;      // a molecule within both limits keeps its neighbour lists, positions and element keys in LDS
constexpr int L3_LDS_BONDS = 2048;
constexpr int L3_LDS_BINS = 8192;      // histograms of at most this many bins over all rows are counted per workgroup in LDS (32 KB)
constexpr int L3_MAX_ATOMS = 1 << 24;  // a neighbour-list entry is (bond key << 24) | molecule-local atom index

struct Local3DArgs {  // passed to the kernel by value (about 1.8 KB of kernel arguments)
  int B;
  MolArrays mol;                                        // a molecule reaching past the extents is skipped
  const float* atom_pos;                                // (.,3) per compact atom
  int num_element, num_bond_types;
  int kptr[4];                                          // rows of lengths | angles | dihedrals
  float lo[3], hi[3], scale[3];                         // scale = n / (hi - lo)
  int nbins[3];
  long long hoff[3], total_bins;                        // first bin of each kind in `hist`
  int lds_hist;                                         // total_bins <= L3_LDS_BINS
  unsigned long long *hist, *outside;                   // ADDED to
  long long* n_items;                                   // (3,B) written
  int *ws_cur, *ws_adj;                                 // N_cap | 2 * E_cap ints
  unsigned long long keys[3 * L3_MAX_ROWS];             // canonical chain of each row, one byte per field, first field on top
};

// workspace of mdx_mol_local3d: degree / cursor per atom and two neighbour-list entries per bond, for molecules beyond the LDS limits
inline size_t local3d_ws_bytes(int64_t N_cap, int64_t Eh_stride) {
  return sizeof(int) * ((size_t)(N_cap > 1 ? N_cap : 1) + 2 * (size_t)(Eh_stride > 1 ? Eh_stride : 1));
}

enum { L3_PREP_OK = 0, L3_PREP_ARG = 1, L3_PREP_UNSUPPORTED = 4 };  // = MDX_OK, MDX_ERR_ARG, MDX_ERR_UNSUPPORTED

// Fills kptr, keys, lo / hi / scale / nbins, hoff, total_bins and lds_hist of `a` from the caller's HOST tables.  patterns: (P,7)
// int32 rows (e0, b01, e1, b12, e2, b23, e3), a length row uses the first 3 fields, an angle row the first 5; kind_ptr[4]: rows of
// lengths | angles | dihedrals; bin_range: 3 x (lo, hi); bin_count: 3.  On failure `a` may be partly written and *why names the cause.
inline int local3d_prepare(Local3DArgs* a, const int32_t* patterns, const int32_t* kind_ptr, const float* bin_range,
                           const int32_t* bin_count, int32_t num_element, int32_t num_bond_types, const char** why) {
  if (num_element < 1 || num_element > 255 || num_bond_types < 1 || num_bond_types > 254) return *why = "class count outside [1, 255]", L3_PREP_ARG;
  if (kind_ptr[0] != 0) return *why = "kind_ptr[0] must be 0", L3_PREP_ARG;
  for (int k = 0; k < 3; ++k) {
    if (kind_ptr[k + 1] < kind_ptr[k]) return *why = "kind_ptr must not decrease", L3_PREP_ARG;
    const float lo = bin_range[2 * k], hi = bin_range[2 * k + 1];
    if (!(hi > lo) || !(hi - lo < 3.0e38f) || bin_count[k] <= 0) return *why = "bins need a finite lo < hi and n > 0", L3_PREP_ARG;
  }
  for (int k = 0; k < 3; ++k)
    if (kind_ptr[k + 1] - kind_ptr[k] > L3_MAX_ROWS) return *why = "more than 64 patterns of one kind", L3_PREP_UNSUPPORTED;
  long long off = 0;
  for (int k = 0; k < 3; ++k) {
    a->kptr[k] = kind_ptr[k];
    const float lo = bin_range[2 * k], hi = bin_range[2 * k + 1];
    a->lo[k] = lo;
    a->hi[k] = hi;
    a->nbins[k] = bin_count[k];
    a->scale[k] = (float)((double)bin_count[k] / ((double)hi - (double)lo));
    a->hoff[k] = off;
    off += (long long)(kind_ptr[k + 1] - kind_ptr[k]) * bin_count[k];
    const int fields = 3 + 2 * k;
    for (int r = kind_ptr[k]; r < kind_ptr[k + 1]; ++r) {
      unsigned long long fwd = 0, rev = 0;
      for (int f = 0; f < fields; ++f) {
        const int32_t v = patterns[7 * (size_t)r + f];
        const bool ok = (f & 1) ? (v >= 1 && v <= num_bond_types) : (v >= 0 && v < num_element);
        if (!ok) return *why = "pattern row with an element or bond id out of range", L3_PREP_ARG;
        fwd = fwd << 8 | (unsigned long long)v;
        rev |= (unsigned long long)v << (8 * f);
      }
      const unsigned long long key = fwd < rev ? fwd : rev;
      for (int q = kind_ptr[k]; q < r; ++q)
        if (a->keys[q] == key) return *why = "duplicate pattern row (a chain and its reverse are one pattern)", L3_PREP_ARG;
      a->keys[r] = key;
    }
  }
  a->kptr[3] = kind_ptr[3];
  a->total_bins = off;
  a->lds_hist = off <= L3_LDS_BINS;
  return L3_PREP_OK;
}
