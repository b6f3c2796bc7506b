// The search tree of the canonical labelling, shared by mdx_canon.hip (mdx_mol_canon), mdx_stereo.hip (mdx_mol_stereo) and mdx_bestrms.hip (mdx_mol_bestrms): the molecule
// staged into LDS, colour refinement, and the unpruned walk (target cell, individualise, refine) with the leaf handled by the caller's
// visitor.  The definition is the one of include/moldiff_hip.h (mdx_mol_canon); all kernels walk the same nodes in the same order, so
// node count, depth and the set of leaves are the same in all.  One workgroup of 256 threads per molecule, thread a = atom a.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdx_canon_args.h"
#include "mdx_mol.h"

namespace {

typedef unsigned long long u64;

constexpr int CN_NONE = 1 << 16;
constexpr unsigned CN_PAD = 0xffffffffu;  // sorts behind every word

// what the walk keeps in LDS, 25,124 B: the bonds, the adjacency as CSR (neighbour and type in 16 bits), the colours as bytes, the
// 64-bit keys of a refinement round, the depth-first stack of at most 64 colour snapshots with the target colour and cursor of a level
struct CnGraph {
  u64 key[MOL_ATOMS];
  unsigned bond[MOL_BONDS];             // the bond word of mdx_mol.h, payload = the low byte of the type
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS], wave_total[4], red[4];
  unsigned short adj[2 * MOL_BONDS];   // neighbour | type << 8
  unsigned short cursor[CN_MAX_DEPTH];
  unsigned char snap[CN_MAX_DEPTH][MOL_ATOMS];
  unsigned char col[MOL_ATOMS];
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

// The molecule into LDS (bonds, degrees, CSR) and the initial colouring, how many labels are smaller -> the number of valid bonds.
// The molecule is past mol_guard.  Ends on a barrier.
__device__ inline int stage_molecule(CnGraph& s, const MolArrays& M, long long h0, int n, int nb, int label) {
  const int tid = threadIdx.x;
  const int* bt = M.bond_type + h0;
  s.col[tid] = 0;
  mol_stage_bonds(M, h0, n, nb, s.bond, s.off, s.cur, s.wave_total, [&](int e, int, int) { return (unsigned)bt[e]; });
  s.key[tid] = (u64)(unsigned)label;
  // the order inside a row does not matter: refine's h is a sum
  mol_stage_rows(nb, s.bond, s.cur, s.adj, [](unsigned other, int, unsigned bd) { return (unsigned short)(other | mol_bond_payload(bd) << 8); });
  int less = 0;
  for (int u = 0; u < n; ++u) less += s.key[u] < (u64)(unsigned)label;
  if (tid < n) s.col[tid] = (unsigned char)less;
  __syncthreads();
  return s.off[MOL_ATOMS] / 2;
}

// Refinement of s.col (visible on entry) until no colour changes -> the size of this thread's cell.  Ends on a barrier.
__device__ inline int refine(CnGraph& s, int n) {
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

// the bond word of a certificate from the colours (ranks) `col`, CN_PAD for an ignored bond
__device__ inline unsigned bond_word(unsigned bd, const unsigned char* col) {
  if (!bd) return CN_PAD;
  const unsigned ci = col[mol_bond_i(bd)], cj = col[mol_bond_j(bd)];
  return min(ci, cj) << 20 | max(ci, cj) << 8 | mol_bond_payload(bd);
}

// w[0 .. P) ascending across the workgroup: bitonic, P a power of two in 2 .. 512, two words per thread.  What was written to w before
// the call need not be visible yet; ends on a barrier.
__device__ inline void sort_words(unsigned* w, int P) {
  const int tid = threadIdx.x;
  for (int kk = 2; kk <= P; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      __syncthreads();
      if (tid < P / 2) {
        const int i = 2 * tid - (tid & (j - 1)), l = i | j;
        const unsigned a = w[i], b = w[l];
        if ((a > b) == ((i & kk) == 0)) w[i] = b, w[l] = a;
      }
    }
  __syncthreads();
}

// where `word` stands in cw[0 .. nbv) (ascending), -1 when it does not: a leaf is optimal iff every bond word of it stands in the
// sorted canonical certificate (the bonds of a simple graph give distinct words, so equal counts make it a bijection)
__device__ inline int find_word(const unsigned* cw, int nbv, unsigned word) {
  int lo = 0, hi = nbv;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cw[mid] < word) lo = mid + 1;
    else hi = mid;
  }
  return lo < nbv && cw[lo] == word ? lo : -1;
}

// The whole tree from the initial colouring in s.col: `leaf()` is called by all threads at every leaf, with the leaf's ranks in s.col
// and visible; what it writes is visible to the next one.  `nodes` counts the nodes, the root included.  -> 0, or 2 when the tree has
// more than max_nodes nodes or a node deeper than CN_MAX_DEPTH.  Every decision is taken from block-wide reductions, so depth, node
// count and the result are uniform.
template <class Leaf>
__device__ inline int canon_walk(CnGraph& s, int n, int max_nodes, int& nodes, Leaf&& leaf) {
  const int tid = threadIdx.x;
  const bool in = tid < n;
  int depth = 0;
  nodes = 1;
  int eq = refine(s, n);
  for (;;) {
    // ---- the node whose colouring is s.col, at `depth`, with `depth` snapshots below it
    const int k = block_min(in && eq > 1 ? (int)s.col[tid] : CN_NONE, s.red);
    if (k == CN_NONE) {
      leaf();
    } else {
      if (depth == CN_MAX_DEPTH) return 2;
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
      if (++nodes > max_nodes) return 2;
      if (tid == 0) s.cursor[L] = (unsigned short)(pick + 1);
      s.col[tid] = (unsigned char)(c == kk && tid != pick ? kk + 1 : c);
      __syncthreads();
      found = true;
      break;
    }
    if (!found) return 0;
    eq = refine(s, n);
  }
}

}  // namespace
