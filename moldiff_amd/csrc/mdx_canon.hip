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
#include "mdx_mol.h"

int mdx_set_error(int code, const char* msg);  // mdx_api.hip

namespace {

typedef unsigned long long u64;

constexpr int CN_ATOMS = 256, CN_BONDS = 512, CN_NONE = 1 << 16;
constexpr unsigned CN_PAD = 0xffffffffu;  // sorts behind every word
enum { C_STATUS, C_NODES, C_LEAVES, C_AUT, C_BONDS };
static_assert(C_BONDS + 1 == CN_STATS && CN_STATS == MDX_CANON_STATS, "the columns of mol_stats");

struct CnArgs {
  MolArrays mol;
  CanonOperands o;
  int max_nodes;
};

struct CnShared {
  u64 key[CN_ATOMS];
  unsigned best[CN_BONDS], cand[CN_BONDS];
  unsigned bond[CN_BONDS];             // i | j << 8 | type << 16 | 1 << 24, or 0 for an ignored bond
  int off[CN_ATOMS + 1], cur[CN_ATOMS], wave_total[4], red[4];
  unsigned short adj[2 * CN_BONDS];    // neighbour | type << 8
  unsigned short cursor[CN_MAX_DEPTH];
  unsigned char snap[CN_MAX_DEPTH][CN_ATOMS];
  unsigned char col[CN_ATOMS], best_rank[CN_ATOMS], table[CN_ATOMS];
  unsigned char tcol[CN_MAX_DEPTH];
};

__device__ inline unsigned mix(unsigned h) {  // murmur3 fmix32
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}

// the smallest v over the workgroup, the same in every thread; two barriers: what was written before is visible after, and `red` is
// free again on return
__device__ inline int block_min(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = min(min(red[0], red[1]), min(red[2], red[3]));
  __syncthreads();
  return v;
}

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

// Refinement of s.col (visible on entry) until no colour changes -> the size of this thread's cell.  Ends on a barrier.
__device__ inline int refine(CnShared& s, int n) {
  const int tid = threadIdx.x;
  const int a0 = tid < n ? s.off[tid] : 0, a1 = tid < n ? s.off[tid + 1] : 0;
  for (;;) {
    const unsigned c = s.col[tid];
    unsigned h = 0u;
    for (int a = a0; a < a1; ++a) {
      const unsigned w = s.adj[a];
      h += mix(mix((unsigned)s.col[w & 0xffu] + 1u) + (w >> 8));
    }
    s.key[tid] = (u64)c << 32 | h;
    __syncthreads();
    const u64 k = s.key[tid];
    int less = 0, eq = 0;
    for (int u = 0; u < n; ++u) {
      const u64 ku = s.key[u];
      less += ku < k, eq += ku == k;
    }
    if (tid < n) s.col[tid] = (unsigned char)less;
    if (!__syncthreads_or(tid < n && (unsigned)less != c)) return eq;
  }
}

__global__ __launch_bounds__(256) void mol_canon_kernel(const CnArgs A) {
  __shared__ CnShared s;
  const int m = blockIdx.x, tid = threadIdx.x;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (v.outside || v.masked) {  // uniform
    write_unmeasured(A, m, 0, v);
    return;
  }
  if (n > CN_ATOMS || nb > CN_BONDS) {  // uniform
    write_unmeasured(A, m, 1, v);
    return;
  }
  const int *bi = A.mol.bond_i + h0, *bj = A.mol.bond_j + h0, *bt = A.mol.bond_type + h0;
  const bool in = tid < n;
  const int atype = in ? A.mol.atom_type[n0 + tid] : 0;
  const int label = in && A.o.atom_label ? A.o.atom_label[n0 + tid] : atype;

  // ---- the molecule into LDS: bonds, degrees, CSR
  s.cur[tid] = 0, s.col[tid] = 0;
  __syncthreads();
  for (int e = tid; e < nb; e += 256) {
    const int i = bi[e], j = bj[e];
    if (!mol_bond_ok(i, j, n)) {
      s.bond[e] = 0u;
      continue;
    }
    s.bond[e] = (unsigned)i | (unsigned)j << 8 | ((unsigned)bt[e] & 0xffu) << 16 | 1u << 24;
    atomicAdd(&s.cur[i], 1), atomicAdd(&s.cur[j], 1);
  }
  __syncthreads();
  block_exclusive_scan_256(s.off, s.cur, s.wave_total);
  __syncthreads();
  for (int e = tid; e < nb; e += 256) {
    const unsigned bd = s.bond[e];
    if (!bd) continue;
    const unsigned i = bd & 0xffu, j = (bd >> 8) & 0xffu, t = (bd >> 16) & 0xffu;
    s.adj[atomicAdd(&s.cur[i], 1)] = (unsigned short)(j | t << 8);  // the order inside a row does not matter: h is a sum
    s.adj[atomicAdd(&s.cur[j], 1)] = (unsigned short)(i | t << 8);
  }
  // ---- the initial colouring: how many labels are smaller
  s.key[tid] = (u64)(unsigned)label;
  __syncthreads();
  const int nbv = s.off[CN_ATOMS] / 2;  // the valid bonds
  {
    int less = 0;
    for (int u = 0; u < n; ++u) less += s.key[u] < (u64)(unsigned)label;
    if (in) s.col[tid] = (unsigned char)less;
  }
  __syncthreads();
  int P = 2;  // the words are sorted over the next power of two
  while (P < nb) P <<= 1;

  int depth = 0, nodes = 1, leaves = 0, n_aut = 0, status = 0;  // uniform
  int eq = refine(s, n);
  for (;;) {
    // ---- the node whose colouring is s.col, at `depth`, with `depth` snapshots below it
    const int k = block_min(in && eq > 1 ? (int)s.col[tid] : CN_NONE, s.red);
    if (k == CN_NONE) {  // a leaf: the certificate
      ++leaves;
      for (int e = tid; e < P; e += 256) {
        const unsigned bd = e < nb ? s.bond[e] : 0u;
        unsigned w = CN_PAD;
        if (bd) {
          const unsigned ci = s.col[bd & 0xffu], cj = s.col[(bd >> 8) & 0xffu];
          w = min(ci, cj) << 20 | max(ci, cj) << 8 | ((bd >> 16) & 0xffu);
        }
        s.cand[e] = w;
      }
      for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
          __syncthreads();
          if (tid < P / 2) {
            const int i = 2 * tid - (tid & (j - 1)), l = i | j;
            const unsigned a = s.cand[i], b = s.cand[l];
            if ((a > b) == ((i & kk) == 0)) s.cand[i] = b, s.cand[l] = a;
          }
        }
      __syncthreads();
      int diff = CN_NONE;
      if (n_aut > 0)
        for (int e = tid; e < nbv; e += 256)
          if (s.cand[e] != s.best[e]) {
            diff = e;
            break;
          }
      diff = n_aut > 0 ? block_min(diff, s.red) : 0;
      const bool better = n_aut == 0 || (diff != CN_NONE && s.cand[diff] < s.best[diff]);
      __syncthreads();  // best[diff] has been read
      if (better) {
        n_aut = 1;
        for (int e = tid; e < nbv; e += 256) s.best[e] = s.cand[e];
        s.best_rank[tid] = s.col[tid];
        if (in) s.table[s.col[tid]] = (unsigned char)tid;
      } else if (diff == CN_NONE) {  // another optimal leaf
        ++n_aut;
        const int first = block_min(in && s.col[tid] != s.best_rank[tid] ? tid : CN_NONE, s.red);
        const bool smaller = first != CN_NONE && s.col[first] < s.best_rank[first];
        __syncthreads();  // best_rank[first] has been read
        if (smaller) s.best_rank[tid] = s.col[tid];
        if (in) s.table[s.col[tid]] = (unsigned char)min((int)s.table[s.col[tid]], tid);  // one thread per rank
      }
    } else {
      if (depth == CN_MAX_DEPTH) {
        status = 2;
        break;
      }
      s.snap[depth][tid] = s.col[tid];
      if (tid == 0) s.tcol[depth] = (unsigned char)k, s.cursor[depth] = 0;
      ++depth;
    }
    // ---- the next child of the deepest level that still has one
    bool found = false;
    while (depth > 0) {
      __syncthreads();  // the snapshot, its cursor, and whatever the leaf wrote
      const int L = depth - 1, kk = s.tcol[L], from = s.cursor[L];
      const int c = s.snap[L][tid];
      const int pick = block_min(in && c == kk && tid >= from ? tid : CN_NONE, s.red);
      if (pick == CN_NONE) {
        --depth;
        continue;
      }
      if (++nodes > A.max_nodes) {
        status = 2;
        break;
      }
      if (tid == 0) s.cursor[L] = (unsigned short)(pick + 1);
      s.col[tid] = (unsigned char)(c == kk && tid != pick ? kk + 1 : c);
      __syncthreads();
      found = true;
      break;
    }
    if (status != 0 || !found) break;
    eq = refine(s, n);
  }
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
    s.cur[r] = label;  // the labels by rank, for the hash
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
    for (int p = 0; p < n; ++p) h = (h ^ (u64)(unsigned)s.cur[p]) * prime;
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
  if (B == 0) return MDX_OK;
  a.max_nodes = max_nodes;
  hipLaunchKernelGGL(mol_canon_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  if (hipGetLastError() != hipSuccess) return mdx_set_error(MDX_ERR_HIP, "mol_canon_kernel: launch failed");
  return MDX_OK;
}
