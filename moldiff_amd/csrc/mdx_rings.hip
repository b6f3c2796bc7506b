// Ring perception and composition counts of decoded molecules on the device (mdx_mol_rings): the cyclomatic number, the ring sizes of
// a minimum cycle basis, ring atoms and bonds, the smallest ring through every bond and atom, rotatable bonds, and the element and
// bond type histograms.  They stand in, without RDKit, for the graph quantities of the reference's `frags_counts`, `count_prop` and
// `ring_topo` blocks (utils/evaluation.py:24-37, 52-83).  The function is DEFINED in include/moldiff_hip.h; moldiff_amd/rings.py
// restates it in plain Python and the GPU tests compare every output exactly.  The ring sizes are those of a minimum cycle basis, NOT
// of RDKit's symmetrised SSSR (cubane: 5 four-rings here, 6 there).
//
// One workgroup of 256 threads (4 waves) per molecule over the compact arrays of mdx_mol.h; a molecule has at most 256
// atoms, 512 bonds and 64 independent rings, so everything lives in LDS (about 24 KB: 6 workgroups per CU by LDS, 8 by waves) and a
// cycle is one 64-bit word.  The graph work is a breadth-first search that ONE WAVE runs on its own: lane l owns atoms l, l + 64,
// l + 128, l + 192, and per level every unreached atom looks among its neighbours for one of the previous level ("pull": no queue, no
// atomics, nothing to race on).  Among several such neighbours the smallest (atom, bond) pair becomes the parent, so that the trees,
// and with them every intermediate value, do not depend on the order the adjacency lists were filled in.  A wave's lanes run in
// lockstep; what one lane stores to LDS and another loads goes through volatile accesses, which the wave issues in program order.
//   (a) adjacency lists in LDS (degrees by LDS integer atomics, offsets by a scan), element / bond type counts;
//   (b) wave 0: a breadth-first forest, rooted at the smallest unreached atom in turn -> fragments c, n_rings = b - n + c, and the
//       bonds outside the forest numbered 0 .. n_rings - 1 by a ballot prefix: a cycle is the set of those it uses;
//   (c) one search per bond with that bond removed, a wave each -> bond_ring_min (0: the search never reaches the other end, a bridge);
//   (d) for the lengths L that occur, upward: every wave grows the tree of a root v carrying each atom's depth and the XOR of the
//       numbered bonds on its tree path; a bond (x, y) gives the candidate cycle word[x] ^ word[y] ^ bit(bond) of nominal length
//       depth[x] + depth[y] + 1 (Horton's candidates; a degenerate one is a sum of strictly shorter cycles and never raises the rank
//       at its nominal length).  The waves take turns to insert their candidates of length L into an XOR basis of <= 64 words kept by
//       leading bit: lanes reduce their candidates against the basis in parallel, one survivor per round, picked by ballot, joins it.
//       ring_hist gets the rank gained at L; the smallest longer nominal length seen becomes the next L; the walk ends when the rank
//       reaches n_rings.  Which survivor joins changes the basis, never its rank.
// Outputs are written with plain stores by the workgroup that owns the molecule: no atomics on global memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_mol.h"

namespace {

typedef unsigned long long u64;

constexpr int RG_RINGS = 64, RG_WAVES = 4;
constexpr int RG_MAX_ELEMENTS = 255, RG_MAX_BOND_TYPES = 254;
constexpr unsigned short RG_FAR = 0xffff;  // depth of an atom not reached; parent bond of a root
constexpr int RG_INF = 1 << 30;

struct RgArgs {
  MolArrays mol;
  int num_element, num_bond_types, ring_bins;
  int *n_rings, *ring_hist, *n_ring_atoms, *n_ring_bonds, *n_rotatable, *elem_count, *bond_count, *status, *bond_ring_min,
      *atom_ring_min;
};

enum { S_MU, S_NRINGS, S_RANK, S_NEXT, S_LMIN, S_RING_ATOMS, S_RING_BONDS, S_ROTATABLE, S_COUNT };

struct RgShared {
  u64 word[RG_WAVES][MOL_ATOMS];            // per wave: XOR of the numbered bonds on the tree path to the atom
  u64 basis[RG_RINGS];                      // by leading bit; 0 = none
  unsigned adj[2 * MOL_BONDS];              // neighbour << 16 | bond
  unsigned bond[MOL_BONDS];                 // the bond word of mdx_mol.h, no payload
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS];   // adjacency offsets; degree, then fill cursor
  int elem[RG_MAX_ELEMENTS + 1], btc[RG_MAX_BOND_TYPES + 2], hist[RG_RINGS];
  int scal[S_COUNT], wave_total[RG_WAVES];
  unsigned short depth[RG_WAVES][MOL_ATOMS];  // per wave
  unsigned short brm[MOL_BONDS];             // bond_ring_min
  unsigned short pbond[MOL_ATOMS];           // forest: the bond to the parent
  unsigned char bnum[MOL_BONDS];             // number of a bond outside the forest, 255 for every other bond
  unsigned char triple[MOL_ATOMS];           // the atom carries a bond of type 3
};

// status and zeros for a molecule that is not measured; its slots of the per-bond / per-atom arrays only when they are inside the arrays
__device__ inline void write_unmeasured(const RgArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    A.status[m] = status;
    A.n_rings[m] = 0, A.n_ring_atoms[m] = 0, A.n_ring_bonds[m] = 0, A.n_rotatable[m] = 0;
  }
  for (int k = tid; k < A.ring_bins; k += 256) A.ring_hist[(size_t)m * A.ring_bins + k] = 0;
  for (int k = tid; k < A.num_element; k += 256) A.elem_count[(size_t)m * A.num_element + k] = 0;
  for (int k = tid; k < A.num_bond_types; k += 256) A.bond_count[(size_t)m * A.num_bond_types + k] = 0;
  if (v.outside) return;
  for (int a = tid; a < v.n; a += 256) A.atom_ring_min[v.n0 + a] = 0;
  for (int e = tid; e < v.nb; e += 256) A.bond_ring_min[v.h0 + e] = 0;
}

// Levels of one wave's breadth-first search until nothing new is reached, or until `target` is.  depth[] holds 0 at the root(s) and
// RG_FAR at every atom still to reach; bond `skip` is treated as absent.  WORDS: word[atom] = word[parent] ^ bit of the parent bond
// (the root's word is set by the caller); PARENT: s.pbond[atom] = the parent bond.
template <bool WORDS, bool PARENT>
__device__ inline void bfs_levels(RgShared& s, int n, int lane, volatile unsigned short* depth, volatile u64* word, int skip, int target) {
  volatile unsigned short* pbond = s.pbond;
  for (int level = 1; level < MOL_ATOMS; ++level) {  // a level reaches a new atom or is the last: never more than n - 1
    bool found = false;
    for (int k = 0; k < MOL_ATOMS / 64; ++k) {
      const int a = lane + 64 * k;
      if (a >= n || depth[a] != RG_FAR) continue;
      unsigned best = ~0u;
      const int p1 = s.off[a + 1];
      for (int p = s.off[a]; p < p1; ++p) {
        const unsigned ent = s.adj[p];
        // an atom reached in this very level holds `level`, never `level - 1`: the order of the stores below does not matter
        if ((int)(ent & 0xffffu) != skip && depth[ent >> 16] == level - 1) best = min(best, ent);
      }
      if (best == ~0u) continue;
      found = true;
      depth[a] = (unsigned short)level;
      if constexpr (PARENT) pbond[a] = (unsigned short)(best & 0xffffu);
      if constexpr (WORDS) {
        const unsigned bn = s.bnum[best & 0xffffu];
        word[a] = word[best >> 16] ^ (bn < RG_RINGS ? 1ull << bn : 0ull);
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (__ballot(found) == 0ull) break;
    if (target >= 0 && depth[target] != RG_FAR) break;
  }
}

__device__ inline void bfs_init(int n, int lane, volatile unsigned short* depth, volatile u64* word, int root) {
  for (int k = 0; k < MOL_ATOMS / 64; ++k) {
    const int a = lane + 64 * k;
    if (a >= n) continue;
    depth[a] = a == root ? 0 : RG_FAR;
    if (word) word[a] = 0ull;
  }
  __builtin_amdgcn_wave_barrier();
}

// One wave inserts the candidates of nominal length L of the tree it holds into the basis; the other waves wait at a barrier.
__device__ inline void insert_candidates(RgShared& s, int nb, int lane, const volatile unsigned short* depth, const volatile u64* word, int L,
                                         int mu) {
  volatile u64* basis = s.basis;
  volatile int* scal = s.scal;
  int rank = scal[S_RANK], next = RG_INF;
  for (int e0 = 0; e0 < nb && rank < mu; e0 += 64) {
    const int e = e0 + lane;
    u64 vec = 0ull;
    const unsigned bd = e < nb ? s.bond[e] : 0u;
    if (bd) {
      const int x = mol_bond_i(bd), y = mol_bond_j(bd);
      const unsigned dx = depth[x], dy = depth[y];
      if (dx != RG_FAR && dy != RG_FAR) {
        const unsigned bn = s.bnum[e];
        const u64 v = word[x] ^ word[y] ^ (bn < RG_RINGS ? 1ull << bn : 0ull);
        const int len = (int)(dx + dy) + 1;
        if (v != 0ull && len == L) vec = v;
        if (v != 0ull && len > L) next = min(next, len);
      }
    }
    for (;;) {
      while (vec != 0ull) {
        const u64 bv = basis[63 - __clzll((long long)vec)];
        if (bv == 0ull) break;
        vec ^= bv;
      }
      const u64 alive = __ballot(vec != 0ull);
      if (alive == 0ull) break;
      if (lane == __ffsll((long long)alive) - 1) {
        basis[63 - __clzll((long long)vec)] = vec;
        vec = 0ull;
      }
      ++rank;
      __builtin_amdgcn_wave_barrier();
      if (rank >= mu) break;
    }
  }
  for (int o = 32; o > 0; o >>= 1) next = min(next, __shfl_xor(next, o, 64));
  if (lane == 0) {
    scal[S_RANK] = rank;
    if (next < RG_INF) atomicMin(&s.scal[S_NEXT], next);
  }
}

__global__ __launch_bounds__(256) void mol_rings_kernel(const RgArgs A) {
  __shared__ RgShared s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  const int *atype = A.mol.atom_type + n0, *bt = A.mol.bond_type + h0;

  // ---- (a) adjacency lists and the two histograms
  s.triple[tid] = 0, s.elem[tid] = 0, s.btc[tid] = 0;
  if (tid < RG_RINGS) s.hist[tid] = 0, s.basis[tid] = 0ull;
  if (tid < S_COUNT) s.scal[tid] = tid == S_LMIN || tid == S_NEXT ? RG_INF : 0;
  mol_stage_bonds(A.mol, h0, n, nb, s.bond, s.off, s.cur, s.wave_total, [&](int e, int i, int j) {
    const int t = bt[e];
    if (t == 3) s.triple[i] = 1, s.triple[j] = 1;
    if (t >= 1 && t <= A.num_bond_types) atomicAdd(&s.btc[t - 1], 1);
    return 0u;
  });
  for (int a = tid; a < n; a += 256) {
    const int c = atype[a];
    if ((unsigned)c < (unsigned)A.num_element) atomicAdd(&s.elem[c], 1);
  }
  mol_stage_rows(nb, s.bond, s.cur, s.adj, [](unsigned other, int e, unsigned) { return other << 16 | (unsigned)e; });

  // ---- (b) wave 0: the forest, the fragments, the numbering of the bonds outside the forest
  if (wave == 0) {
    volatile unsigned short *depth = s.depth[0], *pbond = s.pbond;
    for (int k = 0; k < MOL_ATOMS / 64; ++k) {
      const int a = lane + 64 * k;
      if (a < n) depth[a] = RG_FAR, pbond[a] = RG_FAR;
    }
    __builtin_amdgcn_wave_barrier();
    int fragments = 0;
    for (;;) {
      int root = -1;
      for (int k = 0; k < MOL_ATOMS / 64 && root < 0; ++k) {
        const int a = lane + 64 * k;
        const u64 open = __ballot(a < n && depth[a] == RG_FAR);
        if (open) root = 64 * k + __ffsll((long long)open) - 1;
      }
      if (root < 0 || fragments >= n) break;  // uniform; every root is a new atom
      ++fragments;
      if (lane == 0) depth[root] = 0;
      __builtin_amdgcn_wave_barrier();
      // atoms of earlier fragments hold small depths too, but none of them has an unreached neighbour
      bfs_levels<false, true>(s, n, lane, depth, nullptr, -1, -1);
    }
    int numbered = 0, valid_bonds = 0;
    const u64 below = (1ull << lane) - 1ull;
    for (int e0 = 0; e0 < nb; e0 += 64) {
      const int e = e0 + lane;
      const unsigned bd = e < nb ? s.bond[e] : 0u;
      const bool outside_forest = bd && pbond[mol_bond_i(bd)] != e && pbond[mol_bond_j(bd)] != e;
      const u64 mo = __ballot(outside_forest);
      if (e < nb) s.bnum[e] = outside_forest ? (unsigned char)min(numbered + __popcll(mo & below), 255) : (unsigned char)255;
      numbered += __popcll(mo);
      valid_bonds += __popcll(__ballot(bd != 0u));
    }
    if (lane == 0) s.scal[S_MU] = numbered, s.scal[S_NRINGS] = valid_bonds - n + fragments;
  }
  __syncthreads();
  // without two bonds between one pair of atoms the two agree; with them (a precondition violation) the smaller guards the bit index
  const int mu = s.scal[S_MU], n_rings = s.scal[S_NRINGS];
  if (mu > RG_RINGS || n_rings > RG_RINGS) {  // uniform
    write_unmeasured(A, m, 2, v);
    return;
  }

  // ---- (c) the smallest ring through every bond: a search per bond without it, from one end until the other is reached
  if (mu == 0) {
    for (int e = tid; e < nb; e += 256) s.brm[e] = 0;
  } else {
    volatile unsigned short* depth = s.depth[wave];
    for (int e = wave; e < nb; e += RG_WAVES) {
      const unsigned bd = s.bond[e];  // uniform in the wave
      int size = 0;
      if (bd) {
        const int x = mol_bond_i(bd), y = mol_bond_j(bd);
        bfs_init(n, lane, depth, nullptr, x);
        bfs_levels<false, false>(s, n, lane, depth, nullptr, e, y);
        const unsigned d = depth[y];
        size = d == RG_FAR ? 0 : (int)d + 1;
        __builtin_amdgcn_wave_barrier();  // every lane has read depth[y] before the next search clears it
      }
      if (lane == 0) s.brm[e] = (unsigned short)size;
    }
  }
  __syncthreads();

  // ---- per-atom and per-bond results
  {
    int ring_atoms = 0, ring_bonds = 0, rotatable = 0, lmin = RG_INF;
    for (int a = tid; a < n; a += 256) {
      int best = RG_INF;
      for (int p = s.off[a]; p < s.off[a + 1]; ++p) {
        const int r = s.brm[s.adj[p] & 0xffffu];
        if (r > 0) best = min(best, r);
      }
      A.atom_ring_min[n0 + a] = best < RG_INF ? best : 0;
      ring_atoms += best < RG_INF;
    }
    for (int e = tid; e < nb; e += 256) {
      const unsigned bd = s.bond[e];
      const int r = bd ? s.brm[e] : 0;
      A.bond_ring_min[h0 + e] = r;
      if (!bd) continue;
      const int x = mol_bond_i(bd), y = mol_bond_j(bd);
      if (r > 0) ++ring_bonds, lmin = min(lmin, r);
      rotatable += bt[e] == 1 && r == 0 && s.off[x + 1] - s.off[x] >= 2 && s.off[y + 1] - s.off[y] >= 2 && !s.triple[x] && !s.triple[y];
    }
    ring_atoms = wave_sum(ring_atoms), ring_bonds = wave_sum(ring_bonds), rotatable = wave_sum(rotatable);
    for (int o = 32; o > 0; o >>= 1) lmin = min(lmin, __shfl_xor(lmin, o, 64));
    if (lane == 0) {
      atomicAdd(&s.scal[S_RING_ATOMS], ring_atoms);
      atomicAdd(&s.scal[S_RING_BONDS], ring_bonds);
      atomicAdd(&s.scal[S_ROTATABLE], rotatable);
      atomicMin(&s.scal[S_LMIN], lmin);
    }
  }
  __syncthreads();

  // ---- (d) the rank of the cycles of length <= L, for the lengths L that occur, upward from the smallest ring
  {
    volatile int* scal = s.scal;
    int rank = 0, L = scal[S_LMIN];
    while (rank < mu && L < RG_INF) {  // uniform: both come from LDS behind a barrier
      for (int v0 = 0; v0 < n; v0 += RG_WAVES) {
        if (scal[S_RANK] >= mu) break;  // uniform: the last store to it lies behind a barrier, the next one beyond the barrier below
        const int v = v0 + wave;
        if (v < n) {
          bfs_init(n, lane, s.depth[wave], s.word[wave], v);
          bfs_levels<true, false>(s, n, lane, s.depth[wave], s.word[wave], -1, -1);
        }
        __syncthreads();
        for (int w = 0; w < RG_WAVES; ++w) {
          if (w == wave && v < n) insert_candidates(s, nb, lane, s.depth[wave], s.word[wave], L, mu);
          __syncthreads();
        }
      }
      const int now = scal[S_RANK], next = scal[S_NEXT];
      __syncthreads();
      if (tid == 0) {
        s.hist[min(max(L - 3, 0), A.ring_bins - 1)] += now - rank;  // L < 3 only with two bonds between one pair of atoms
        scal[S_NEXT] = RG_INF;
      }
      __syncthreads();
      rank = now, L = next;
    }
  }

  // ---- results
  if (tid == 0) {
    A.status[m] = 0;
    A.n_rings[m] = n_rings;
    A.n_ring_atoms[m] = s.scal[S_RING_ATOMS], A.n_ring_bonds[m] = s.scal[S_RING_BONDS], A.n_rotatable[m] = s.scal[S_ROTATABLE];
  }
  for (int k = tid; k < A.ring_bins; k += 256) A.ring_hist[(size_t)m * A.ring_bins + k] = s.hist[k];
  for (int k = tid; k < A.num_element; k += 256) A.elem_count[(size_t)m * A.num_element + k] = s.elem[k];
  for (int k = tid; k < A.num_bond_types; k += 256) A.bond_count[(size_t)m * A.num_bond_types + k] = s.btc[k];
}

}  // namespace

extern "C" int mdx_mol_rings(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                             const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index,
                             int64_t Eh_stride, const int32_t* select, int32_t num_element, int32_t num_bond_types, int32_t ring_bins,
                             int32_t* n_rings, int32_t* ring_hist, int32_t* n_ring_atoms, int32_t* n_ring_bonds, int32_t* n_rotatable,
                             int32_t* elem_count, int32_t* bond_count, int32_t* status, int32_t* bond_ring_min, int32_t* atom_ring_min,
                             void* stream) {
  RgArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  if (!n_rings || !ring_hist || !n_ring_atoms || !n_ring_bonds || !n_rotatable || !elem_count || !bond_count || !status || !bond_ring_min ||
      !atom_ring_min)
    return mdx_set_error(MDX_ERR_ARG, "null argument");
  if (ring_bins < 1 || ring_bins > RG_RINGS) return mdx_set_error(MDX_ERR_ARG, "ring_bins must lie in 1 .. 64");
  if (num_element < 1 || num_element > RG_MAX_ELEMENTS || num_bond_types < 1 || num_bond_types > RG_MAX_BOND_TYPES)
    return mdx_set_error(MDX_ERR_ARG, "num_element must lie in 1 .. 255 and num_bond_types in 1 .. 254");
  a.num_element = num_element, a.num_bond_types = num_bond_types, a.ring_bins = ring_bins;
  a.n_rings = n_rings, a.ring_hist = ring_hist, a.n_ring_atoms = n_ring_atoms, a.n_ring_bonds = n_ring_bonds;
  a.n_rotatable = n_rotatable, a.elem_count = elem_count, a.bond_count = bond_count, a.status = status;
  a.bond_ring_min = bond_ring_min, a.atom_ring_min = atom_ring_min;
  return mol_launch(mol_rings_kernel, "mol_rings_kernel", B, stream, a);
}
