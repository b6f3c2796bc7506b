// Distance bounds of all-atom molecules on the device (mdx_mol_bounds): for every pair of atoms of the molecule that mdx_mol_relax
// relaxes (heavy atoms, then the hydrogens in (atom, k) order) a lower and an upper bound on their distance, from the rest lengths and
// angles of the force-field rows, triangle-smoothed.  mdx_mol_embed makes coordinates from them.  It is THIS PROJECT'S OWN MODEL, not
// RDKit's bounds matrix and unverified against it; include/moldiff_hip.h states it, moldiff_amd/embed.py (bounds_ref) restates it
// operation by operation, and this file is built with -ffp-contract=off so that the float64 arithmetic is the restatement's.
//
// One workgroup of 256 threads per molecule over the compact arrays of mdx_mol.h, staged by mdx_allatom.h as mdx_relax.hip stages them
// (bonds, rows with the X-H bonds appended, sorted by neighbour, rest length per bond).  Thread a owns COLUMN a of the two matrices, the
// entries [i][a] at i * na_cap + a: it writes the initial bounds of its pairs (both threads of a pair evaluate the same expression, the
// path taken from its lower end atom, so the matrices are symmetric bit for bit) and smooths its own column, reading row k of step k
// from LDS (row k = column k by symmetry, and step k leaves it unchanged).  No thread reads a global word another thread wrote.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_allatom.h"
#include "mdx_embed_args.h"

namespace {

enum { B_STATUS, B_NALL, B_N12, B_N13, B_N14, B_RING, B_TIGHT };
static_assert(B_TIGHT + 1 == EB_STATS && EB_STATS == MDX_BOUNDS_STATS, "the columns of the table");

struct BdArgs {
  MolArrays mol;
  RelaxTable tab;
  BoundsParams p;
  BoundsOperands o;
};

struct BdShared : AllAtomShared {
  double lrow[MOL_ATOMS], urow[MOL_ATOMS];
  unsigned m12[8][MOL_ATOMS], m13[8][MOL_ATOMS], m14[8][MOL_ATOMS], tight[8][MOL_ATOMS];  // bit i of word [i >> 5][a]: the pair (i, a)
  int ired[4][8];
};

__device__ inline bool has(const unsigned (*m)[MOL_ATOMS], int a, int i) { return (m[i >> 5][a] >> (i & 31)) & 1u; }
__device__ inline void mark(unsigned (*m)[MOL_ATOMS], int a, int i) { m[i >> 5][a] |= 1u << (i & 31); }

// the size (3, 4, 5) of the smallest ring that holds the angle a-b-c, or 0
__device__ inline int ring_size(const BdShared& s, int a, int b, int c) {
  if (has(s.m12, a, c)) return 3;
  for (int q = s.off[a]; q < s.off[a + 1]; ++q) {
    const int x = row_nbr(s.adj[q]);
    if (x != b && has(s.m12, x, c)) return 4;
  }
  for (int q = s.off[a]; q < s.off[a + 1]; ++q) {
    const int x = row_nbr(s.adj[q]);
    if (x == b) continue;
    for (int p = s.off[c]; p < s.off[c + 1]; ++p) {
      const int y = row_nbr(s.adj[p]);
      if (y != b && has(s.m12, x, y)) return 5;
    }
  }
  return 0;
}

__device__ inline double angle_c0(const BdShared& s, const BoundsParams& P, int a, int b, int c) {
  const int rs = ring_size(s, a, b, c);
  return rs ? P.ring_c0[rs - 3] : s.par[s.typ[b]][RX_C0];
}

__device__ inline void write_unmeasured(const BdArgs& A, int m, int status) {
  if (threadIdx.x < EB_STATS) A.o.mol_stats[(size_t)m * EB_STATS + threadIdx.x] = threadIdx.x == B_STATUS ? status : 0;
}

__global__ __launch_bounds__(256) void mol_bounds_kernel(const BdArgs A) {
  __shared__ BdShared s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MolView v = mol_view(A.mol, m);
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured);
    return;
  }
  const AllAtomCount aa = allatom_count(A.o.h_count + v.n0, v.n, s.off, s.cur, s.wave_total);
  const int n_all = aa.n_all, cap = A.p.na_cap;
  if (n_all > MOL_ATOMS || n_all > cap) {  // uniform
    write_unmeasured(A, m, EM_TOO_LARGE);
    return;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) s.m12[c][tid] = 0u, s.m13[c][tid] = 0u, s.m14[c][tid] = 0u, s.tight[c][tid] = 0u;  // its own column
  allatom_stage(s, A.mol, v, A.tab, A.o.order + v.h0, A.o.atom_flag + v.n0, aa, nullptr);
  const bool live = tid < n_all;
  const int r0 = s.off[tid], r1 = live ? s.off[tid + 1] : r0;
  for (int q = r0; q < r1; ++q) mark(s.m12, tid, row_nbr(s.adj[q]));
  __syncthreads();  // ring_size reads the bonds of other atoms

  // ---- the initial bounds of column tid: every entry [i][tid], i < n_all (i < cap, tid < cap: inside the molecule's two matrices)
  const size_t plane = (size_t)cap * (size_t)cap;
  double* L = A.o.bounds + (size_t)m * 2u * plane + tid;
  double* U = L + plane;
  unsigned char* C = A.o.cls + (size_t)m * plane + tid;
  const BoundsParams& P = A.p;
  int ring = 0;
  if (live) {
    const double xa = s.par[s.typ[tid]][RX_X];
    for (int i = 0; i < n_all; ++i) {
      const size_t at = (size_t)i * cap;
      const double lo = P.vdw_scale * (0.5 * (xa + s.par[s.typ[i]][RX_X]));
      L[at] = i == tid ? 0.0 : lo, U[at] = i == tid ? 0.0 : EB_FAR, C[at] = EB_OTHER;
    }
    auto widen = [&](unsigned (*mk)[MOL_ATOMS], int d, double lo, double hi, int cls) {
      const size_t at = (size_t)d * cap;
      lo = lo < 0.0 ? 0.0 : lo;
      if (!has(mk, tid, d)) {
        mark(mk, tid, d);
        L[at] = lo, U[at] = hi, C[at] = (unsigned char)cls;
      } else {
        L[at] = fmin(L[at], lo), U[at] = fmax(U[at], hi);
      }
    };
    for (int q = r0; q < r1; ++q) {  // 1-3
      const int b = row_nbr(s.adj[q]), eb = row_bond(s.adj[q]);
      for (int p = s.off[b]; p < s.off[b + 1]; ++p) {
        const int d = row_nbr(s.adj[p]), ed = row_bond(s.adj[p]);
        if (d == tid || has(s.m12, tid, d)) continue;
        const double c = angle_c0(s, P, min(tid, d), b, max(tid, d));
        const double l = tid < d ? bounds_13(s.br0[eb], s.br0[ed], c) : bounds_13(s.br0[ed], s.br0[eb], c);
        widen(s.m13, d, l - P.tol13, l + P.tol13, EB_13);
      }
    }
    for (int q = r0; q < r1; ++q) {  // 1-4
      const int b = row_nbr(s.adj[q]), e1 = row_bond(s.adj[q]);
      for (int p = s.off[b]; p < s.off[b + 1]; ++p) {
        const int c = row_nbr(s.adj[p]), e2 = row_bond(s.adj[p]);
        if (c == tid) continue;
        for (int t = s.off[c]; t < s.off[c + 1]; ++t) {
          const int d = row_nbr(s.adj[t]), e3 = row_bond(s.adj[t]);
          if (d == tid || d == b || has(s.m12, tid, d) || has(s.m13, tid, d)) continue;
          double cis, trans;
          if (tid < d) bounds_14(s.br0[e1], s.br0[e2], s.br0[e3], angle_c0(s, P, tid, b, c), angle_c0(s, P, b, c, d), &cis, &trans);
          else bounds_14(s.br0[e3], s.br0[e2], s.br0[e1], angle_c0(s, P, d, c, b), angle_c0(s, P, c, b, tid), &cis, &trans);
          widen(s.m14, d, cis - P.tol14, trans + P.tol14, EB_14);
        }
      }
    }
    for (int q = r0; q < r1; ++q) {  // 1-2
      const int b = row_nbr(s.adj[q]);
      const size_t at = (size_t)b * cap;
      const double r = s.br0[row_bond(s.adj[q])], lo = r - P.tol12;
      L[at] = lo < 0.0 ? 0.0 : lo, U[at] = r + P.tol12, C[at] = EB_12;
    }
    for (int q1 = r0; q1 < r1; ++q1)  // the ring angles centred here
      for (int q2 = q1 + 1; q2 < r1; ++q2) ring += ring_size(s, row_nbr(s.adj[q1]), tid, row_nbr(s.adj[q2])) != 0;
  }

  // ---- smoothing: the upper bounds, then the lower bounds
  for (int k = 0; k < n_all; ++k) {
    __syncthreads();  // the row of the step before is no longer read
    if (live) s.urow[tid] = U[(size_t)k * cap];
    __syncthreads();
    if (live) {
      const double uk = s.urow[tid];
      for (int i = 0; i < n_all; ++i) {
        const double via = s.urow[i] + uk, old = U[(size_t)i * cap];
        if (via < old) U[(size_t)i * cap] = via, mark(s.tight, tid, i);
      }
    }
  }
  for (int k = 0; k < n_all; ++k) {
    __syncthreads();
    if (live) s.urow[tid] = U[(size_t)k * cap], s.lrow[tid] = L[(size_t)k * cap];
    __syncthreads();
    if (live) {
      const double uk = s.urow[tid], lk = s.lrow[tid];
      for (int i = 0; i < n_all; ++i) {
        const double old = L[(size_t)i * cap];
        const double now = fmax(fmax(old, s.lrow[i] - uk), lk - s.urow[i]);
        if (now > old) L[(size_t)i * cap] = now, mark(s.tight, tid, i);
      }
    }
  }
  int bad = 0, c12 = 0, c13 = 0, c14 = 0, tight = 0;
  if (live)
    for (int i = 0; i < tid; ++i) {
      bad += L[(size_t)i * cap] > U[(size_t)i * cap];
      c12 += has(s.m12, tid, i), c13 += has(s.m13, tid, i), c14 += has(s.m14, tid, i), tight += has(s.tight, tid, i);
    }
  const int counted[6] = {c12, c13, c14, ring, tight, bad};
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int sum = wave_sum(counted[c]);
    if (lane == 0) s.ired[wave][c] = sum;
  }
  __syncthreads();
  auto total = [&](int c) { return (s.ired[0][c] + s.ired[1][c]) + (s.ired[2][c] + s.ired[3][c]); };
  if (tid < 5) A.o.mol_stats[(size_t)m * EB_STATS + B_N12 + tid] = total(tid);
  if (tid == 5) {
    A.o.mol_stats[(size_t)m * EB_STATS + B_STATUS] = total(5) ? EM_INCONSISTENT : EM_OK;
    A.o.mol_stats[(size_t)m * EB_STATS + B_NALL] = n_all;
  }
}

}  // namespace

extern "C" int mdx_mol_bounds(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                              const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                              const int32_t* select, const int32_t* order, const int32_t* h_count, const int32_t* atom_flag, int32_t num_element,
                              int32_t num_bond_types, const double* ff_rows, int32_t n_rows, double tol12, double tol13, double tol14,
                              double vdw_scale, int32_t na_cap, void* bounds_ws, size_t ws_bytes, int32_t* mol_stats, void* stream) {
  BdArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  if (!order || !h_count || !atom_flag || !mol_stats) return mdx_set_error(MDX_ERR_ARG, "null argument");
  if (const char* why = bounds_prepare(&a.p, tol12, tol13, tol14, vdw_scale, na_cap)) return mdx_set_error(MDX_ERR_ARG, why);
  if (const char* why = bounds_ws_check(B, na_cap, bounds_ws, ws_bytes)) return mdx_set_error(MDX_ERR_ARG, why);
  const char* why = "";
  if (relax_prepare(&a.tab, ff_rows, n_rows, num_element, num_bond_types, 1e-3, 1.0, 1.0, 0, &why) != RX_PREP_OK) return mdx_set_error(MDX_ERR_ARG, why);
  a.o = BoundsOperands{order, h_count, atom_flag, (double*)bounds_ws, (unsigned char*)bounds_ws + (size_t)B * 16u * (size_t)na_cap * (size_t)na_cap, mol_stats};
  return mol_launch(mol_bounds_kernel, "mol_bounds_kernel", B, stream, a);
}
