// Stereo perception of decoded molecules on the device (mdx_mol_stereo): tetrahedral parities and cis / trans codes from the 3D
// coordinates, made independent of atom order, rotation and the choice among automorphisms by taking the smallest stereo word over all
// optimal leaves of the canonical search.  It is THIS PROJECT'S OWN DEFINITION, not RDKit's stereo perception and not CIP; the
// definition and every output are stated in include/moldiff_hip.h, moldiff_amd/stereo.py restates the function (stereo_ref) and the GPU
// tests compare every output exactly.
//
// One workgroup of 256 threads (4 waves) per molecule, thread a = atom a, as mol_canon_kernel, and the same walk: the staging, the
// refinement and the tree of mdx_canon_body.h, so nodes, depth and leaves are canon's.  This file is the geometry and the leaf.
//   Geometry, once: thread a reads its 3 or 4 neighbours (sorted by index in registers), forms the unit vectors and the determinant in
//   float64 (built with -ffp-contract=off) and keeps a 2-bit code; one thread per bond keeps the other neighbours of both ends and
//   the up to four cis / trans codes of their pairings in 8 bits.  Nothing afterwards reads a coordinate.
//   The canonical certificate is rebuilt from the given rank and sorted once.  A leaf is optimal iff every bond word of the leaf is
//   found in it (binary search; the bonds of a simple graph give distinct words, so equal counts make it a bijection) -- no sort per
//   leaf -- and the position found is where the bond's code goes in the stereo word.
//   At an optimal leaf the word w (one byte per atom and per valid bond, at most 768) is written by the atoms and bonds themselves,
//   compared with the running minima W and M (the mirror word: atom codes 1 and 2 swapped) by a block-wide "first differing position"
//   minimum, and W, M, the rank tie-break and the per-rank minimum table (the orbits) are updated.
// Everything lives in LDS, 35,824 B, so four workgroups share a CU.  No workspace, no global atomics, no scratch: the neighbour lists
// are four named registers and every array indexed at run time is in LDS.  All outputs are plain stores by the molecule's own
// workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_canon_body.h"
#include "mdx_mol.h"
#include "mdx_stereo_args.h"

namespace {

enum { S_STATUS, S_CAND, S_CENTRES, S_FLAT, S_BOND_CAND, S_STEREO_BONDS, S_STEREOGENIC, S_CHIRAL, S_AUT };
static_assert(S_AUT + 1 == ST_STATS && ST_STATS == MDX_STEREO_STATS, "the columns of mol_stats");
constexpr int ST_WORD = MOL_ATOMS + MOL_BONDS;
enum { A_NONE, A_FLAT, A_PLUS, A_MINUS };  // an atom's geometry code: no candidate; candidate with g = 0; g = +1; g = -1

struct StArgs {
  MolArrays mol;
  StereoOperands o;
  unsigned centre4, centre3;
  double flat_tol, bond_tol;
  int max_nodes;
};

struct StShared {
  CnGraph g;                        // the walk's own state (mdx_canon_body.h)
  unsigned cw[MOL_BONDS];           // the canonical certificate, from the given rank
  unsigned others[MOL_BONDS];       // x0 | x1 << 8 | y0 << 16 | y1 << 24: the other neighbours of a candidate bond's ends, x0 <= x1, y0 <= y1
  unsigned nbr4[MOL_ATOMS];         // the 3 or 4 neighbours of a candidate atom in ascending index, a byte each
  unsigned short bpos[MOL_BONDS];   // where the bond's word stands in the canonical certificate, per leaf
  unsigned short dt[MOL_BONDS];     // bit 8: a candidate; bits 2 (2 xi + yi) ..: d(x_xi, y_yi)
  unsigned char w[ST_WORD], W[ST_WORD], M[ST_WORD];
  unsigned char acode[MOL_ATOMS], srank[MOL_ATOMS], table[MOL_ATOMS], crank[MOL_ATOMS];
};

struct D3 {
  double x, y, z;
};
__device__ inline D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline double det3(D3 a, D3 b, D3 c) {
  return (a.x * (b.y * c.z - b.z * c.y) - a.y * (b.x * c.z - b.z * c.x)) + a.z * (b.x * c.y - b.y * c.x);
}
// p -> ok stays set only when all three coordinates are finite
__device__ inline D3 load_pos(const float* pos, long long a, bool& ok) {
  const float x = pos[3 * a], y = pos[3 * a + 1], z = pos[3 * a + 2];
  ok = ok && isfinite(x) && isfinite(y) && isfinite(z);
  return {(double)x, (double)y, (double)z};
}
// d / |d| -> ok is cleared for a zero-length vector
__device__ inline D3 unit(D3 d, bool& ok) {
  const double dd = dot(d, d);
  if (!(dd > 0.0)) {
    ok = false;
    return {0.0, 0.0, 0.0};
  }
  const double l = sqrt(dd);
  return {d.x / l, d.y / l, d.z / l};
}

// d(x, y) of the double bond a-b: 1 cis, 2 trans, 0 neither or degenerate
__device__ inline unsigned pair_code(const float* pos, long long a, long long b, long long x, long long y, double tol) {
  bool ok = true;
  const D3 pa = load_pos(pos, a, ok), pb = load_pos(pos, b, ok), px = load_pos(pos, x, ok), py = load_pos(pos, y, ok);
  if (!ok) return 0u;
  const D3 e = unit(sub(pb, pa), ok);
  if (!ok) return 0u;
  const D3 dx = sub(px, pa), dy = sub(py, pb);
  const double tx = dot(dx, e), ty = dot(dy, e);
  const D3 xp = {dx.x - tx * e.x, dx.y - tx * e.y, dx.z - tx * e.z}, yp = {dy.x - ty * e.x, dy.y - ty * e.y, dy.z - ty * e.z};
  const double xx = dot(xp, xp), yy = dot(yp, yp);
  if (!(xx > 0.0) || !(yy > 0.0)) return 0u;
  const double c = dot(xp, yp) / (sqrt(xx) * sqrt(yy));
  return c > tol ? 1u : c < -tol ? 2u : 0u;
}

__device__ inline void order(unsigned& a, unsigned& b) {
  const unsigned lo = min(a, b), hi = max(a, b);
  a = lo, b = hi;
}

// the other neighbours of `a` on the bond a-b and whether `a` may be the end of a candidate: 1 or 2 others, none over a bond of type 2
// or 3 -> x0 <= x1 (equal when there is one).  `a` has 2 or 3 bonds.
__device__ inline bool bond_end(const StShared& s, unsigned a, unsigned b, unsigned& x0, unsigned& x1) {
  const int r0 = s.g.off[a], deg = s.g.off[a + 1] - r0;
  int cnt = 0;
  bool ok = true;
  x0 = x1 = a;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < deg) {
      const unsigned w = s.g.adj[r0 + k], u = w & 0xffu, t = w >> 8;
      if (u == b) continue;
      ok = ok && t != 2u && t != 3u;
      if (cnt == 0) x0 = x1 = u;
      else x1 = u;
      ++cnt;
    }
  order(x0, x1);
  return ok && cnt >= 1;
}

// stereo_rank -1 and zeros for a molecule that is not measured; its per-atom and per-bond slots only when they are inside the arrays
__device__ inline void write_unmeasured(const StArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  if (tid < ST_STATS) A.o.mol_stats[(size_t)m * ST_STATS + tid] = tid == S_STATUS ? status : 0;
  if (tid == 0) A.o.stereo_hash[m] = 0, A.o.mirror_hash[m] = 0;
  if (v.outside) return;
  for (long long a = v.n0 + tid; a < v.n0 + v.n; a += 256) A.o.stereo_rank[a] = -1, A.o.canon_tetra[a] = 0, A.o.mirror_tetra[a] = 0, A.o.atom_tetra[a] = 0;
  for (long long e = v.h0 + tid; e < v.h0 + v.nb; e += 256) A.o.canon_bond_stereo[e] = 0, A.o.mirror_bond_stereo[e] = 0, A.o.bond_stereo[e] = 0;
}

__device__ inline unsigned char mirrored(unsigned char c, bool atom) { return atom && c ? (unsigned char)(3 - c) : c; }

__device__ inline int64_t fnv_bytes(const unsigned char* w, int len) {
  u64 h = 0xcbf29ce484222325ull;
  for (int p = 0; p < len; ++p) h = (h ^ (u64)w[p]) * 0x100000001b3ull;
  return (int64_t)h;
}

__global__ __launch_bounds__(256) void mol_stereo_kernel(const StArgs A) {
  __shared__ StShared s;
  const int m = blockIdx.x, tid = threadIdx.x;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  if (A.o.canon_status[m] != 0) {  // uniform
    write_unmeasured(A, m, 1, v);
    return;
  }
  const bool in = tid < n;
  const int atype = in ? A.mol.atom_type[n0 + tid] : 0;
  const int label = in && A.o.atom_label ? A.o.atom_label[n0 + tid] : atype;
  const int given = in ? A.o.rank[n0 + tid] : 0;
  const int nbv = stage_molecule(s.g, A.mol, h0, n, nb, label);  // the valid bonds
  if (__syncthreads_or(in && (unsigned)given >= (unsigned)n)) {  // not a rank of mdx_mol_canon: nothing may be indexed with it
    write_unmeasured(A, m, 1, v);
    return;
  }
  const int L = n + nbv;  // the length of a stereo word
  const float* pos = A.o.atom_pos;

  // ---- geometry: the atoms
  unsigned code = A_NONE, nbrs = 0u;
  if (in) {
    const int r0 = s.g.off[tid], deg = s.g.off[tid + 1] - r0;
    const bool bit4 = (unsigned)atype < 32u && (A.centre4 >> atype & 1u), bit3 = (unsigned)atype < 32u && (A.centre3 >> atype & 1u);
    if ((deg == 4 && bit4) || (deg == 3 && bit3)) {
      unsigned a0 = s.g.adj[r0], a1 = s.g.adj[r0 + 1], a2 = s.g.adj[r0 + 2];
      unsigned a3 = deg == 4 ? s.g.adj[r0 + 3] & 0xffu : 0x1ffu;  // 0x1ff: no fourth neighbour, behind every atom and never an index
      const bool single = (a0 >> 8) == 1u && (a1 >> 8) == 1u && (a2 >> 8) == 1u;
      a0 &= 0xffu, a1 &= 0xffu, a2 &= 0xffu;
      order(a0, a1), order(a2, a3), order(a0, a2), order(a1, a3), order(a1, a2);
      if (deg == 4 || single) {
        bool ok = true;
        const D3 p = load_pos(pos, n0 + tid, ok);
        const D3 u0 = unit(sub(load_pos(pos, n0 + a0, ok), p), ok), u1 = unit(sub(load_pos(pos, n0 + a1, ok), p), ok);
        const D3 u2 = unit(sub(load_pos(pos, n0 + a2, ok), p), ok);
        double vol, thr;
        if (deg == 4) {
          const D3 u3 = unit(sub(load_pos(pos, n0 + a3, ok), p), ok);
          vol = det3(sub(u1, u0), sub(u2, u0), sub(u3, u0)), thr = 4.0 * A.flat_tol;
        } else {
          vol = det3(u0, u1, u2), thr = A.flat_tol;
        }
        code = !ok ? A_FLAT : vol > thr ? A_PLUS : vol < -thr ? A_MINUS : A_FLAT;
        nbrs = a0 | a1 << 8 | a2 << 16 | (deg == 4 ? a3 : 0u) << 24;
      }
    }
  }
  s.acode[tid] = (unsigned char)code, s.nbr4[tid] = nbrs;
  s.crank[tid] = (unsigned char)given;
  const int n_cand = __syncthreads_count(code != A_NONE), n_flat = __syncthreads_count(code == A_FLAT);

  // ---- geometry: the bonds
  int n_bond_cand = 0;
  for (int e0 = 0; e0 < MOL_BONDS; e0 += 256) {  // uniform trip count: the count below is a barrier
    const int e = e0 + tid;
    unsigned dt = 0u, oth = 0u;
    const unsigned bd = e < nb ? s.g.bond[e] : 0u;
    if (bd && mol_bond_payload(bd) == 2u) {
      const unsigned a = mol_bond_i(bd), b = mol_bond_j(bd);
      const int da = s.g.off[a + 1] - s.g.off[a], db = s.g.off[b + 1] - s.g.off[b];
      unsigned x0 = a, x1 = a, y0 = b, y1 = b;
      if (da >= 2 && da <= 3 && db >= 2 && db <= 3 && bond_end(s, a, b, x0, x1) && bond_end(s, b, a, y0, y1)) {
        const unsigned c00 = pair_code(pos, n0 + a, n0 + b, n0 + x0, n0 + y0, A.bond_tol);
        const unsigned c01 = y1 != y0 ? pair_code(pos, n0 + a, n0 + b, n0 + x0, n0 + y1, A.bond_tol) : c00;
        const unsigned c10 = x1 != x0 ? pair_code(pos, n0 + a, n0 + b, n0 + x1, n0 + y0, A.bond_tol) : c00;
        const unsigned c11 = x1 != x0 ? (y1 != y0 ? pair_code(pos, n0 + a, n0 + b, n0 + x1, n0 + y1, A.bond_tol) : c10) : c01;
        dt = 0x100u | c00 | c01 << 2 | c10 << 4 | c11 << 6;
        oth = x0 | x1 << 8 | y0 << 16 | y1 << 24;
      }
    }
    if (e < MOL_BONDS) s.dt[e] = (unsigned short)dt, s.others[e] = oth;
    n_bond_cand += __syncthreads_count(dt != 0u);
  }

  // ---- the canonical certificate from the given rank
  int P = 2;
  while (P < nb) P <<= 1;
  for (int e = tid; e < P; e += 256) s.cw[e] = bond_word(e < nb ? s.g.bond[e] : 0u, s.crank);
  sort_words(s.cw, P);

  int nodes = 1, n_aut = 0;  // uniform
  const int status = canon_walk(s.g, n, A.max_nodes, nodes, [&]() {
    // ---- is the leaf optimal: every bond word stands in the canonical certificate
    bool miss = false;
    for (int e = tid; e < nb; e += 256) {
      const unsigned bd = s.g.bond[e];
      if (!bd) continue;
      const int k = find_word(s.cw, nbv, bond_word(bd, s.g.col));
      if (k < 0) miss = true;
      else s.bpos[e] = (unsigned short)k;
    }
    if (__syncthreads_or(miss)) return;
    ++n_aut;
    // ---- its word
    if (in) {
      const unsigned c = s.acode[tid];
      unsigned out = 0u;
      if (c >= A_PLUS) {
        const unsigned q = s.nbr4[tid];
        const int r0 = s.g.col[q & 0xffu], r1 = s.g.col[(q >> 8) & 0xffu], r2 = s.g.col[(q >> 16) & 0xffu];
        int inv = (r0 > r1) + (r0 > r2) + (r1 > r2);  // the inversions of the ranks in index order: the permutation's sign
        if (s.g.off[tid + 1] - s.g.off[tid] == 4) {
          const int r3 = s.g.col[q >> 24];
          inv += (r0 > r3) + (r1 > r3) + (r2 > r3);
        }
        out = ((c == A_PLUS) == ((inv & 1) == 0)) ? 1u : 2u;
      }
      s.w[s.g.col[tid]] = (unsigned char)out;
    }
    for (int e = tid; e < nb; e += 256) {
      if (!s.g.bond[e]) continue;
      const unsigned dt = s.dt[e];
      unsigned out = 0u;
      if (dt) {
        const unsigned o = s.others[e];
        const unsigned xi = s.g.col[(o >> 8) & 0xffu] < s.g.col[o & 0xffu], yi = s.g.col[o >> 24] < s.g.col[(o >> 16) & 0xffu];
        out = (dt >> (2u * (2u * xi + yi))) & 3u;
      }
      s.w[n + s.bpos[e]] = (unsigned char)out;
    }
    __syncthreads();
    if (n_aut == 1) {
      for (int p = tid; p < L; p += 256) s.W[p] = s.w[p], s.M[p] = mirrored(s.w[p], p < n);
      s.srank[tid] = s.g.col[tid];
      if (in) s.table[s.g.col[tid]] = (unsigned char)tid;
      return;
    }
    int dW = CN_NONE, dM = CN_NONE;
    for (int p = tid; p < L && (dW == CN_NONE || dM == CN_NONE); p += 256) {
      if (dW == CN_NONE && s.w[p] != s.W[p]) dW = p;
      if (dM == CN_NONE && mirrored(s.w[p], p < n) != s.M[p]) dM = p;
    }
    dW = block_min(dW, s.g.red), dM = block_min(dM, s.g.red);
    const bool lessW = dW != CN_NONE && s.w[dW] < s.W[dW], lessM = dM != CN_NONE && mirrored(s.w[dM], dM < n) < s.M[dM];
    int first = CN_NONE;
    if (dW == CN_NONE) first = block_min(in && s.g.col[tid] != s.srank[tid] ? tid : CN_NONE, s.g.red);  // uniform branch
    const bool smaller = first != CN_NONE && s.g.col[first] < s.srank[first];
    __syncthreads();  // W, M and srank have been read
    if (lessW || smaller) s.srank[tid] = s.g.col[tid];
    for (int p = tid; p < L; p += 256) {
      if (lessW) s.W[p] = s.w[p];
      if (lessM) s.M[p] = mirrored(s.w[p], p < n);
    }
    if (in) s.table[s.g.col[tid]] = (unsigned char)min((int)s.table[s.g.col[tid]], tid);  // one thread per rank
  });
  __syncthreads();
  if (status != 0 || n_aut == 0) {  // uniform; no optimal leaf: the rank given is not canon's for these arrays
    write_unmeasured(A, m, status != 0 ? status : 1, v);
    return;
  }

  // ---- results
  int n_centres, n_stereogenic, n_stereo_bonds = 0;
  {
    const unsigned c = s.acode[tid];
    bool distinct = c >= A_PLUS;
    if (distinct) {
      const unsigned q = s.nbr4[tid];
      const int o0 = s.table[s.crank[q & 0xffu]], o1 = s.table[s.crank[(q >> 8) & 0xffu]], o2 = s.table[s.crank[(q >> 16) & 0xffu]];
      distinct = o0 != o1 && o0 != o2 && o1 != o2;
      if (s.g.off[tid + 1] - s.g.off[tid] == 4) {
        const int o3 = s.table[s.crank[q >> 24]];
        distinct = distinct && o0 != o3 && o1 != o3 && o2 != o3;
      }
    }
    n_centres = __syncthreads_count(c >= A_PLUS);
    n_stereogenic = __syncthreads_count(distinct);
  }
  if (in) {
    const int r = s.srank[tid];
    A.o.stereo_rank[n0 + tid] = r, A.o.canon_tetra[n0 + tid] = s.W[tid], A.o.mirror_tetra[n0 + tid] = s.M[tid], A.o.atom_tetra[n0 + tid] = s.W[r];
  }
  for (int e0 = 0; e0 < MOL_BONDS; e0 += 256) {  // uniform trip count
    const int e = e0 + tid;
    int cb = 0;
    if (e < nb) {
      cb = e < nbv ? s.W[n + e] : 0;
      const unsigned bd = s.g.bond[e];
      const int k = bd ? find_word(s.cw, nbv, bond_word(bd, s.srank)) : -1;
      A.o.canon_bond_stereo[h0 + e] = cb, A.o.mirror_bond_stereo[h0 + e] = e < nbv ? s.M[n + e] : 0;
      A.o.bond_stereo[h0 + e] = k >= 0 ? s.W[n + k] : 0;
    }
    n_stereo_bonds += __syncthreads_count(cb != 0);
  }
  int differ = 0;
  for (int p = tid; p < L; p += 256) differ |= s.W[p] != s.M[p];
  const int chiral = __syncthreads_or(differ) ? 1 : 0;
  if (tid == 0) A.o.stereo_hash[m] = fnv_bytes(s.W, L);
  if (tid == 64) A.o.mirror_hash[m] = fnv_bytes(s.M, L);
  if (tid < ST_STATS) {
    const int row[ST_STATS] = {0, n_cand, n_centres, n_flat, n_bond_cand, n_stereo_bonds, n_stereogenic, chiral, n_aut};
    int val = 0;
#pragma unroll
    for (int k = 0; k < ST_STATS; ++k) val = tid == k ? row[k] : val;
    A.o.mol_stats[(size_t)m * ST_STATS + tid] = val;
  }
}

}  // namespace

extern "C" int mdx_mol_stereo(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                              const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                              const int32_t* select, const float* atom_pos, const int32_t* atom_label, const int32_t* rank,
                              const int32_t* canon_status, uint32_t centre4_mask, uint32_t centre3_mask, double flat_tol, double bond_tol,
                              int32_t max_nodes, int32_t* canon_tetra, int32_t* canon_bond_stereo, int32_t* mirror_tetra,
                              int32_t* mirror_bond_stereo, int32_t* stereo_rank, int32_t* atom_tetra, int32_t* bond_stereo, int32_t* mol_stats, int64_t* stereo_hash, int64_t* mirror_hash, void* stream) {
  StArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  a.o = StereoOperands{atom_pos, atom_label, rank, canon_status, canon_tetra, canon_bond_stereo, mirror_tetra, mirror_bond_stereo, stereo_rank, atom_tetra, bond_stereo, mol_stats,
                       stereo_hash, mirror_hash};
  if (const char* why = stereo_check(a.o, flat_tol, bond_tol, max_nodes)) return mdx_set_error(MDX_ERR_ARG, why);
  a.centre4 = centre4_mask, a.centre3 = centre3_mask, a.flat_tol = flat_tol, a.bond_tol = bond_tol, a.max_nodes = max_nodes;
  return mol_launch(mol_stereo_kernel, "mol_stereo_kernel", B, stream, a);
}
