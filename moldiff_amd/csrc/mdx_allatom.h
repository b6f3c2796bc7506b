// The all-atom molecule of mdx_mol_relax, mdx_mol_bounds and mdx_mol_embed, staged once: the heavy atoms of the compact arrays
// (mdx_mol.h), then the hydrogens that mdx_mol_hydrogens counted, in (atom, k) order; at most 256 atoms in all, thread a owns atom a.
// moldiff_amd/relax.py (_stage) restates the staging.  As in mdx_mol.h every kernel keeps its own __shared__ struct: the scan takes
// its arrays as pointers, the staged molecule is one sub-struct that a kernel's struct derives from.  Device only.
#pragma once
#include "mdx_mol.h"
#include "mdx_relax_args.h"

constexpr int AA_BONDS = MOL_BONDS + MOL_ATOMS;  // the heavy bonds, then one X-H bond per hydrogen

struct AllAtomCount {
  int h, hoff, n_all;  // this thread's atom: its hydrogens (0 past the molecule) and those of the atoms before it; atoms in all
};

// Hydrogen k of heavy atom a is atom n + hoff + k.  off, cur, wave_total: the arrays of block_exclusive_scan_256, free for another
// use afterwards.  Uniform n_all; ends on a barrier.
__device__ inline AllAtomCount allatom_count(const int* h_count, int n, int* off, int* cur, int* wave_total) {
  const int tid = threadIdx.x;
  const int h = tid < n ? min(max(h_count[tid], 0), RX_MAX_H) : 0;
  cur[tid] = h;
  __syncthreads();
  block_exclusive_scan_256(off, cur, wave_total);
  __syncthreads();
  const AllAtomCount c = {h, off[tid], n + off[MOL_ATOMS]};
  __syncthreads();  // the offsets are read before the arrays are used again
  return c;
}

struct AllAtomShared {
  double br0[AA_BONDS];  // rest length per bond
  double par[RX_MAX_TYPES][RX_NPAR];
  double ln_order[4];
  unsigned bond[AA_BONDS];     // the bond word of mdx_mol.h, payload = the order index (0: 1, 1: 1.5, 2: 2, 3: 3)
  unsigned adj[2 * AA_BONDS];  // neighbour << 16 | bond: a row sorted by the word is sorted by neighbour
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS], wave_total[4];
  unsigned char typ[MOL_ATOMS], var[MOL_ATOMS], parent[MOL_ATOMS], arom[MOL_ATOMS];
  unsigned char type_of[RX_MAX_ELEMENTS * 4];
};

__device__ inline int row_nbr(unsigned w) { return (int)(w >> 16); }
__device__ inline int row_bond(unsigned w) { return (int)(w & 0xffffu); }

// Stages a molecule past mol_guard with c.n_all <= MOL_ATOMS: the heavy bonds and their degrees (mol_stage_bonds), then rows that also
// hold the X-H bonds (a second scan, mol_stage_rows, the hydrogens appended; a hydrogen's row is its parent), every row sorted by
// neighbour; type, variant and parent per atom, the derived parameter rows, and the rest length of every bond (its force constant
// into bk when that is not null).  order, atom_flag: the caller's arrays at the molecule's first bond / atom.  -> whether this
// thread's atom was typed by a fall-back row.  Ends on a barrier.
__device__ inline int allatom_stage(AllAtomShared& s, const MolArrays& M, const MolView& v, const RelaxTable& tab, const int* order, const int* atom_flag,
                                    const AllAtomCount& c, double* bk) {
  const int tid = threadIdx.x, n = v.n, nb = v.nb, n_all = c.n_all;
  const bool in = tid < n;
  s.arom[tid] = 0, s.parent[tid] = 0;
  for (int q = tid; q < RX_MAX_TYPES * RX_NPAR; q += 256) s.par[q / RX_NPAR][q % RX_NPAR] = tab.par[q / RX_NPAR][q % RX_NPAR];
  if (tid < RX_MAX_ELEMENTS * 4) s.type_of[tid] = tab.type_of[tid >> 2][tid & 3];
  if (tid < 4) s.ln_order[tid] = tab.ln_order[tid];
  __syncthreads();
  if (in)
    for (int k = 0; k < c.h; ++k) s.parent[n + c.hoff + k] = (unsigned char)tid;  // n + hoff + k < n_all <= 256
  const int* bt = M.bond_type + v.h0;
  const int nbt = tab.num_bond_types;
  const int deg_heavy = mol_stage_bonds(M, v.h0, n, nb, s.bond, s.off, s.cur, s.wave_total, [&](int e, int i, int j) {
    if (bt[e] == nbt) {
      s.arom[i] = 1, s.arom[j] = 1;
      return 1u;
    }
    const int o = min(max(order[e], 1), 3);
    return o == 1 ? 0u : (unsigned)o;
  });
  // the rows of the all-atom molecule: the heavy neighbours, then the atom's own hydrogens; a hydrogen's row is its parent
  s.cur[tid] = in ? deg_heavy + c.h : tid < n_all ? 1 : 0;
  __syncthreads();
  block_exclusive_scan_256(s.off, s.cur, s.wave_total);
  __syncthreads();
  mol_stage_rows(nb, s.bond, s.cur, s.adj, [](unsigned other, int e, unsigned) { return other << 16 | (unsigned)e; });
  if (in) {
    for (int k = 0; k < c.h; ++k) s.adj[s.off[tid] + deg_heavy + k] = (unsigned)(n + c.hoff + k) << 16 | (unsigned)(nb + c.hoff + k);
  } else if (tid < n_all) {
    const unsigned p = s.parent[tid];
    s.adj[s.off[tid]] = p << 16 | (unsigned)(nb + tid - n);
    s.bond[nb + tid - n] = mol_bond_word((int)p, tid, 0u);
  }
  int fallback = 0;
  if (in) {
    const int cls = min(max(M.atom_type[v.n0 + tid], 0), tab.num_element - 1);
    int var = atom_flag[tid] & 3;
    var = s.arom[tid] ? RX_RESONANT : var == 3 ? RX_TETRAHEDRAL : var;
    const unsigned code = s.type_of[4 * cls + var];
    s.typ[tid] = (unsigned char)(code & 0x7fu), s.var[tid] = (unsigned char)var;
    fallback = (code & RX_FALLBACK) != 0;
  } else {
    s.typ[tid] = (unsigned char)tab.h_type, s.var[tid] = RX_HYDROGEN;
  }
  __syncthreads();
  if (tid < n_all) {  // the rows arrive in any order: insertion sort by the word, the neighbour in its high bits, each thread its own row
    const int r0 = s.off[tid], r1 = s.off[tid + 1];
    for (int q = r0 + 1; q < r1; ++q) {
      const unsigned x = s.adj[q];
      int k = q - 1;
      for (; k >= r0 && s.adj[k] > x; --k) s.adj[k + 1] = s.adj[k];
      s.adj[k + 1] = x;
    }
  }
  for (int e = tid; e < nb + n_all - n; e += 256) {  // rest length and force constant, the lower atom first
    const unsigned w = s.bond[e];
    double r0 = 0.0, k = 0.0;
    if (w) {
      const int i = mol_bond_i(w), j = mol_bond_j(w);
      relax_pair(s.par[s.typ[min(i, j)]], s.par[s.typ[max(i, j)]], s.ln_order[mol_bond_payload(w) & 3u], &r0, &k);
    }
    s.br0[e] = r0;
    if (bk) bk[e] = k;
  }
  __syncthreads();
  return fallback;
}

// This thread's heavy atom a < n and its RX_MAX_H hydrogen slots (zeros past c.h) of an all-atom array -> the (n, 3) + (n, 4, 3)
// layout of the outputs: po and ho point at the atom's entries.  The first three coordinates are written.
template <int D>
__device__ inline void allatom_write(const double (&X)[D][MOL_ATOMS], int n, const AllAtomCount& c, double* po, double* ho) {
  for (int q = 0; q < 3; ++q) po[q] = X[q][threadIdx.x];
  for (int k = 0; k < RX_MAX_H; ++k) {
    const bool there = k < c.h;
    const int b = there ? n + c.hoff + k : 0;
    for (int q = 0; q < 3; ++q) ho[3 * k + q] = there ? X[q][b] : 0.0;
  }
}
