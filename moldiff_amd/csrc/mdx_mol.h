// The compact molecule arrays every evaluation kernel walks (the mdx_mol_* entry points of include/moldiff_hip.h), defined once:
// molecule m has its atoms at atom_ptr[m] .. + n_atoms[m] and its bonds at bond_ptr[m] .. + n_bonds[m], one direction per bond,
// molecule-local atom indices -- what mdx_decode_output leaves and what moldiff_amd/molpack.py packs from a list of molecule dicts.
// The first part is plain C++ (mdx_local3d_args.h includes it and tools/local3d_host_check.cpp builds that without HIP); the second
// holds the device helpers the kernels share, the molecule staged in LDS among them, and the launch tail of the entry points.
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
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/moldiff_hip.h"

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

// ---- The staged molecule of the kernels that run one workgroup of 256 threads per molecule with thread a = atom a (rings, groups,
// kekule, canon / stereo / bestrms, framework, hydrogens): its limits, the guard, the bond word, and the adjacency as CSR in LDS.  Every
// kernel keeps its own __shared__ struct and hands the arrays in as pointers.
constexpr int MOL_ATOMS = 256, MOL_BONDS = 512;  // an atom index is a byte of the bond word, a bond index 9 bits of an adjacency word
constexpr int MOL_MEASURE = -1;

// -> MOL_MEASURE, or the status the kernel reports with every output of the molecule 0: 0 when it is outside the arrays or masked, 1
// when it is above the limits.  Uniform over the workgroup.  Past it n <= MOL_ATOMS, nb <= MOL_BONDS and the extents may be read.
__device__ inline int mol_guard(const MolView& v) {
  if (v.outside || v.masked) return 0;
  return v.n > MOL_ATOMS || v.nb > MOL_BONDS ? 1 : MOL_MEASURE;
}

// The bond word: i | j << 8 | payload << 16 | MOL_BOND_VALID, and 0 for an ignored bond (mol_bond_ok), so that `!word` tests for one
// whatever the payload is.  The 8 payload bits are the kernel's own.
constexpr unsigned MOL_BOND_VALID = 1u << 24;
__device__ inline unsigned mol_bond_word(int i, int j, unsigned payload) {
  return (unsigned)i | (unsigned)j << 8 | (payload & 0xffu) << 16 | MOL_BOND_VALID;
}
__device__ inline unsigned mol_bond_i(unsigned word) { return word & 0xffu; }
__device__ inline unsigned mol_bond_j(unsigned word) { return (word >> 8) & 0xffu; }
__device__ inline unsigned mol_bond_payload(unsigned word) { return (word >> 16) & 0xffu; }

// Bonds, degrees and row offsets of a molecule past mol_guard: bond[e] = the word of bond e for e < nb, off[a] .. off[a + 1] = the row
// of atom a in the adjacency, cur[a] = off[a] (the fill cursor of mol_stage_rows).  -> this thread's degree, 0 for tid >= n.
// payload(e, i, j) -> the payload bits; it runs once per VALID bond, in the thread of the bond.  It may read the caller's global arrays
// and update LDS words of the caller's, zeroed before the call, with integer atomics or with stores of one value: the first barrier
// here makes the zeros visible, the last one what the bonds left.
// A degree is counted exactly for the bonds with a non-zero word, which are the bonds mol_stage_rows places: a count without its entry
// would leave a slot of the row unwritten, an entry without its count would land in the next row.  An atom past n has degree 0, so
// off[MOL_ATOMS] is the total, 2 x the valid bonds, whatever n is.  Ends on a barrier.
template <class Payload>
__device__ inline int mol_stage_bonds(const MolArrays& M, long long h0, int n, int nb, unsigned* bond, int* off, int* cur, int* wave_total,
                                      Payload&& payload) {
  const int tid = threadIdx.x;
  const int *bi = M.bond_i + h0, *bj = M.bond_j + h0;
  cur[tid] = 0;
  __syncthreads();  // no degree is added before every cursor is 0
  for (int e = tid; e < nb; e += 256) {
    const int i = bi[e], j = bj[e];
    if (!mol_bond_ok(i, j, n)) {
      bond[e] = 0u;
      continue;
    }
    bond[e] = mol_bond_word(i, j, payload(e, i, j));
    atomicAdd(&cur[i], 1), atomicAdd(&cur[j], 1);
  }
  __syncthreads();  // the degrees are complete
  const int deg = block_exclusive_scan_256(off, cur, wave_total);
  __syncthreads();  // the offsets, the cursors and the bond words are visible
  return deg;
}

// The rows: for every valid bond e = (i, j), entry(j, e, word) into the row of i and entry(i, e, word) into the row of j.  The order
// inside a row is whatever the atomics give: a consumer sorts the row or does not depend on it.  Every slot lies below
// off[MOL_ATOMS] <= 2 nb <= 2 MOL_BONDS, the size of adj.  Ends on a barrier.
template <class T, class Entry>
__device__ inline void mol_stage_rows(int nb, const unsigned* bond, int* cur, T* adj, Entry&& entry) {
  for (int e = threadIdx.x; e < nb; e += 256) {
    const unsigned bd = bond[e];
    if (!bd) continue;
    const unsigned i = mol_bond_i(bd), j = mol_bond_j(bd);
    adj[atomicAdd(&cur[i], 1)] = entry(j, e, bd);
    adj[atomicAdd(&cur[j], 1)] = entry(i, e, bd);
  }
  __syncthreads();
}

// The tail of the mdx_mol_* entry points, after every argument check: one workgroup of 256 threads per molecule on the caller's stream.
// B == 0 is MDX_OK without a call into the runtime; a launch that fails is MDX_ERR_HIP with the kernel's name.
int mdx_set_error(int code, const char* msg);  // mdx_api.hip
template <class Args>
inline int mol_launch(void (*kernel)(Args), const char* name, int32_t B, void* stream, const Args& a) {
  if (B == 0) return MDX_OK;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  if (hipGetLastError() == hipSuccess) return MDX_OK;
  char msg[96];
  snprintf(msg, sizeof msg, "%s: launch failed", name);
  return mdx_set_error(MDX_ERR_HIP, msg);
}

#endif  // __HIPCC__
