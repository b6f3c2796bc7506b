// The compact molecule arrays every evaluation kernel walks (mdx_mol_local3d, mdx_mol_fingerprint, mdx_mol_rings, mdx_mol_groups, mdx_mol_kekulize), defined
// once: molecule m has its atoms at atom_ptr[m] .. + n_atoms[m] and its bonds at bond_ptr[m] .. + n_bonds[m], one direction per bond,
// molecule-local atom indices -- what mdx_decode_output leaves and what moldiff_amd/molpack.py packs from a list of molecule dicts.
// The first part is plain C++ (mdx_local3d_args.h includes it and tools/local3d_host_check.cpp builds that without HIP); the second
// holds the device helpers the kernels share.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct MolArrays {
  const int *atom_ptr, *bond_ptr, *n_atoms, *n_bonds;  // (B) each
  const int* atom_type;                                 // class index per compact atom
  const int *bond_type, *bond_i, *bond_j;               // molecule-local atom indices, one direction per bond
  const int* select;                                    // (B) or nullptr: a molecule with 0 is masked out
  long long N_cap, E_cap;                               // extents of the atom / bond arrays
};

// Validates the operands the C entry points share and fills `a` from them.  -> nullptr, or the reason the call is refused.
inline const char* mol_arrays_fill(MolArrays* a, int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms,
                                   const int32_t* n_bonds, const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type,
                                   const int32_t* bond_index, int64_t Eh_stride, const int32_t* select) {
  if (!atom_ptr || !bond_ptr || !n_atoms || !n_bonds || !atom_type || !bond_type || !bond_index) return "null argument";
  if (B < 0 || N_cap < 0 || Eh_stride < 0) return "negative size";
  a->atom_ptr = atom_ptr, a->bond_ptr = bond_ptr, a->n_atoms = n_atoms, a->n_bonds = n_bonds;
  a->atom_type = atom_type, a->bond_type = bond_type, a->bond_i = bond_index, a->bond_j = bond_index + Eh_stride;
  a->select = select;
  a->N_cap = N_cap, a->E_cap = Eh_stride;
  return nullptr;
}

#ifdef __HIPCC__

struct MolView {
  long long n0, h0;  // first atom, first bond
  int n, nb;
  bool outside;      // the extent leaves the arrays (never from mdx_decode_output): nothing of the molecule may be read or written
  bool masked;       // select[m] == 0
};

__device__ inline MolView mol_view(const MolArrays& A, int m) {
  MolView v;
  v.n0 = A.atom_ptr[m], v.h0 = A.bond_ptr[m];
  v.n = A.n_atoms[m], v.nb = A.n_bonds[m];
  v.outside = v.n < 0 || v.nb < 0 || v.n0 < 0 || v.h0 < 0 || v.n0 + v.n > A.N_cap || v.h0 + v.nb > A.E_cap;
  v.masked = A.select && A.select[m] == 0;
  return v;
}

// a bond with an index outside the molecule or with i = j is ignored everywhere (mdx_mol_check alone keeps i = j: its own test)
__device__ inline bool mol_bond_ok(int i, int j, int n) { return (unsigned)i < (unsigned)n && (unsigned)j < (unsigned)n && i != j; }

template <class T>
__device__ inline T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline int wave_inclusive_scan(int v) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// Agent-scope accesses: what atomics update in global memory is read back past the CU's vector L1, which may hold the line from
// before another thread's atomic changed it.  The LDS form is a plain access between barriers, or the agent-scope one.
template <class T>
__device__ inline T ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ inline void st(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS, class T>
__device__ inline T ld(const T* p) {
  if constexpr (LDS) return *p;
  return ld(p);
}
template <bool LDS, class T>
__device__ inline void st(T* p, T v) {
  if constexpr (LDS)
    *p = v;
  else
    st(p, v);
}

// 256 threads: cur[tid] holds a count (the degree of atom tid; 0 past the molecule) -> off[tid] = cur[tid] = the sum of the counts
// before tid and off[256] = the total, whatever the molecule's size.  -> this thread's count.  One barrier inside; the caller places
// one before (the counts are complete) and one after (the offsets are visible).  wave_total: 4 ints of LDS.
__device__ inline int block_exclusive_scan_256(int* off, int* cur, int* wave_total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int deg = cur[tid];
  const int inc = wave_inclusive_scan(deg);
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += wave_total[w];
  off[tid] = before + inc - deg;
  cur[tid] = before + inc - deg;
  if (tid == 255) off[256] = before + inc;
  return deg;
}

#endif  // __HIPCC__
