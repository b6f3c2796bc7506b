// Canonical labelling of decoded molecules on the device (mdx_mol_canon): an exact canonical form of the labelled bond graph, the
// order of its automorphism group and the orbit of every atom, by colour refinement and an UNPRUNED individualisation search.  It is
// THIS PROJECT'S OWN DEFINITION, not RDKit's canonical ranking; the definition and every output are stated in include/moldiff_hip.h,
// moldiff_amd/canon.py restates the function (canon_ref) and the GPU tests compare every output exactly.
//
// One workgroup of 256 threads (4 waves) per molecule over the compact arrays of mdx_mol.h, thread a = atom a; a molecule has at most
// 256 atoms and 512 bonds (the caps of mdx_mol_rings).  Everything lives in LDS, 29,936 B, so five workgroups share a CU: the
// bonds, the adjacency as CSR (neighbour and type in 16 bits), the colours as bytes, the 64-bit keys of a refinement round, the
// depth-first stack of at most 64 colour snapshots (16 KB) with the target colour and the cursor of every level, and the best and the
// candidate certificate at 512 words each.  There is no workspace and no scratch: no array is indexed at run time outside LDS.
// The staging, the refinement and the walk are those of mdx_canon_body.h, which mdx_stereo.hip walks too; this file is the leaf.
//
// A refinement round: thread a sums mix(mix(c(u) + 1) + type) over its neighbours, writes key = c << 32 | h, and after a barrier
// counts the smaller and the equal keys over the n keys -- every lane reads the same address, a broadcast without bank conflicts.
// The count of smaller keys is the new colour, the count of equal ones the size of the atom's cell.  The loop ends when no colour
// changed (__syncthreads_or).  At a leaf the bond words are sorted across the workgroup (bitonic over the next power of two, two
// words per thread), compared with the best certificate in parallel (the first differing word by a block minimum), and the best
// certificate, n_aut, the rank tie-break and the per-rank minimum table are updated.  Every decision is taken from block-wide
// reductions, so depth, node count and status are uniform registers.  All outputs are plain vector stores by the molecule's own
// workgroup: no atomics on global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_canon_args.h"
#include "mdx_canon_body.h"
#include "mdx_mol.h"

namespace {

enum { C_STATUS, C_NODES, C_LEAVES, C_AUT, C_BONDS };
static_assert(C_BONDS + 1 == CN_STATS && CN_STATS == MDX_CANON_STATS, "the columns of mol_stats");

struct CnArgs {
  MolArrays mol;
  CanonOperands o;
  int max_nodes;
};

struct CnShared {
  CnGraph g;                           // the walk's own state (mdx_canon_body.h)
  unsigned best[MOL_BONDS], cand[MOL_BONDS];
  unsigned char best_rank[MOL_ATOMS], table[MOL_ATOMS];
};

// rank -1 and zeros for a molecule that is not measured; its per-atom and per-bond slots only when they are inside the arrays
__device__ inline void write_unmeasured(const CnArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  if (tid < CN_STATS) A.o.mol_stats[(size_t)m * CN_STATS + tid] = tid == C_STATUS ? status : 0;
  if (tid == 0) A.o.cert_hash[m] = 0;
  if (v.outside) return;
  for (long long a = v.n0 + tid; a < v.n0 + v.n; a += 256) {
    A.o.rank[a] = -1, A.o.orbit[a] = 0, A.o.canon_atom_type[a] = 0;
    if (A.o.canon_atom_label) A.o.canon_atom_label[a] = 0;
    if (A.o.canon_pos) A.o.canon_pos[3 * a] = 0.f, A.o.canon_pos[3 * a + 1] = 0.f, A.o.canon_pos[3 * a + 2] = 0.f;
  }
  for (long long e = v.h0 + tid; e < v.h0 + v.nb; e += 256)
    A.o.canon_bond_index[e] = 0, A.o.canon_bond_index[A.mol.E_cap + e] = 0, A.o.canon_bond_type[e] = 0;
}

__global__ __launch_bounds__(256) void mol_canon_kernel(const CnArgs A) {
  __shared__ CnShared s;
  const int m = blockIdx.x, tid = threadIdx.x;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  const bool in = tid < n;
  const int atype = in ? A.mol.atom_type[n0 + tid] : 0;
  const int label = in && A.o.atom_label ? A.o.atom_label[n0 + tid] : atype;
  const int nbv = stage_molecule(s.g, A.mol, h0, n, nb, label);  // the valid bonds
  int P = 2;  // the words are sorted over the next power of two
  while (P < nb) P <<= 1;

  int nodes = 1, leaves = 0, n_aut = 0;  // uniform
  const int status = canon_walk(s.g, n, A.max_nodes, nodes, [&]() {  // a leaf: the certificate
    ++leaves;
    for (int e = tid; e < P; e += 256) s.cand[e] = bond_word(e < nb ? s.g.bond[e] : 0u, s.g.col);
    sort_words(s.cand, P);
    int diff = CN_NONE;
    if (n_aut > 0)
      for (int e = tid; e < nbv; e += 256)
        if (s.cand[e] != s.best[e]) {
          diff = e;
          break;
        }
    diff = n_aut > 0 ? block_min(diff, s.g.red) : 0;
    const bool better = n_aut == 0 || (diff != CN_NONE && s.cand[diff] < s.best[diff]);
    __syncthreads();  // best[diff] has been read
    if (better) {
      n_aut = 1;
      for (int e = tid; e < nbv; e += 256) s.best[e] = s.cand[e];
      s.best_rank[tid] = s.g.col[tid];
      if (in) s.table[s.g.col[tid]] = (unsigned char)tid;
    } else if (diff == CN_NONE) {  // another optimal leaf
      ++n_aut;
      const int first = block_min(in && s.g.col[tid] != s.best_rank[tid] ? tid : CN_NONE, s.g.red);
      const bool smaller = first != CN_NONE && s.g.col[first] < s.best_rank[first];
      __syncthreads();  // best_rank[first] has been read
      if (smaller) s.best_rank[tid] = s.g.col[tid];
      if (in) s.table[s.g.col[tid]] = (unsigned char)min((int)s.table[s.g.col[tid]], tid);  // one thread per rank
    }
  });
  __syncthreads();
  if (status != 0) {  // uniform
    write_unmeasured(A, m, status, v);
    return;
  }

  // ---- results
  const int r = s.best_rank[tid];
  if (in) {
    A.o.rank[n0 + tid] = r, A.o.orbit[n0 + tid] = s.table[r], A.o.canon_atom_type[n0 + r] = atype;
    if (A.o.canon_atom_label) A.o.canon_atom_label[n0 + r] = label;
    if (A.o.canon_pos) {
      const float *p = A.o.atom_pos + 3 * (n0 + tid);
      float* q = A.o.canon_pos + 3 * (n0 + r);
      q[0] = p[0], q[1] = p[1], q[2] = p[2];
    }
    s.g.cur[r] = label;  // the labels by rank, for the hash
  }
  for (int e = tid; e < nb; e += 256) {
    const unsigned w = e < nbv ? s.best[e] : 0u;
    A.o.canon_bond_index[h0 + e] = (int)(w >> 20), A.o.canon_bond_index[A.mol.E_cap + h0 + e] = (int)((w >> 8) & 0xfffu);
    A.o.canon_bond_type[h0 + e] = (int)(w & 0xffu);
  }
  __syncthreads();
  if (tid == 0) {  // FNV-1a-64 over n, the labels by rank, the number of valid bonds, the words
    u64 h = 0xcbf29ce484222325ull;
    const u64 prime = 0x100000001b3ull;
    h = (h ^ (u64)(unsigned)n) * prime;
    for (int p = 0; p < n; ++p) h = (h ^ (u64)(unsigned)s.g.cur[p]) * prime;
    h = (h ^ (u64)(unsigned)nbv) * prime;
    for (int e = 0; e < nbv; ++e) h = (h ^ (u64)s.best[e]) * prime;
    A.o.cert_hash[m] = (int64_t)h;
  }
  if (tid < CN_STATS)
    A.o.mol_stats[(size_t)m * CN_STATS + tid] = tid == C_STATUS ? 0 : tid == C_NODES ? nodes : tid == C_LEAVES ? leaves : tid == C_AUT ? n_aut : nbv;
}

}  // namespace

extern "C" int mdx_mol_canon(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                             const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                             const int32_t* select, const float* atom_pos, const int32_t* atom_label, int32_t max_nodes, int32_t* rank,
                             int32_t* orbit, int32_t* canon_atom_type, int32_t* canon_atom_label, float* canon_pos,
                             int32_t* canon_bond_index, int32_t* canon_bond_type, int32_t* mol_stats, int64_t* cert_hash, void* stream) {
  CnArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  a.o = CanonOperands{atom_pos, atom_label, rank, orbit, canon_atom_type, canon_atom_label, canon_bond_index, canon_bond_type, mol_stats,
                      canon_pos, cert_hash};
  if (const char* why = canon_check(a.o, max_nodes)) return mdx_set_error(MDX_ERR_ARG, why);
  a.max_nodes = max_nodes;
  return mol_launch(mol_canon_kernel, "mol_canon_kernel", B, stream, a);
}
