// Explicit hydrogens with 3D coordinates for decoded molecules on the device (mdx_mol_hydrogens): the hydrogens a Kekulé assignment
// counts (n_h and the bond orders, normally kek_h and kek_order of mdx_mol_kekulize) are placed from the local geometry of the heavy
// atoms, and the contacts of the placed hydrogens with every other atom of the molecule are measured in the same launch.  It is THIS
// PROJECT'S OWN IDEALISED PLACEMENT, not RDKit's AddHs(addCoords=True) and unverified against it: rotors sit where the rule puts them,
// not where an energy would.  The definition and every output are stated in include/moldiff_hip.h, moldiff_amd/hydrogens.py restates
// the function (addh_ref) operation by operation, and this file is built with -ffp-contract=off so that the float64 arithmetic is the
// restatement's.
//
// One workgroup of 256 threads (4 waves) per molecule over the compact arrays of mdx_mol.h; at most 256 atoms and 512 bonds.  Staged
// once in LDS: the positions widened to float64, the bonds, and the adjacency as CSR (the staging of mdx_mol.h), every row then sorted
// by its owner so that "ascending neighbour index" is what a walk of the row gives.  Thread a decides atom a's geometry, places its
// hydrogens into the LDS table of 1024 x 3 doubles and writes its own slots.  The placed slots are then listed (a second scan) and the
// pairs (placed H) x (heavy atom or later placed H) are dealt round-robin over the threads; an H is only ever placed on an atom with at
// most three neighbours, so the excluded set is the parent and the three neighbour bytes kept beside it.  Minimum and count are reduced
// with wave shuffles and then over the four waves through LDS.  About 41 KB of LDS, no atomics on global memory, no workspace, no
// scratch: every array indexed at run time is in LDS.  All outputs are plain stores by the molecule's own workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_hydrogens_args.h"
#include "mdx_mol.h"

namespace {

constexpr int HY_SLOTS = MOL_ATOMS * HY_MAX_H;
enum { GEOM_TETRAHEDRAL = 0, GEOM_TRIGONAL = 1, GEOM_LINEAR = 2 };
enum { FLAG_NO_ROOM = 4, FLAG_DEGENERATE = 8, FLAG_WORLD_FRAME = 16, FLAG_CLAMPED = 32 };
// the columns of mol_stats: MDX_HYDROGENS_* of include/moldiff_hip.h
enum { H_STATUS, H_WANTED, H_PLACED, H_NO_ROOM, H_DEGENERATE, H_WORLD_FRAME, H_CLASH };
static_assert(H_CLASH + 1 == HY_STATS && HY_STATS == MDX_HYDROGENS_STATS, "the columns of mol_stats");

// the constants of the definition, the same literals as moldiff_amd/hydrogens.py
constexpr double COS_TET = -0.3333333333333333, SIN_TET = 0.9428090415820635;   // theta = acos(-1/3)
constexpr double COS_TRI = -0.5, SIN_TRI = 0.8660254037844386;                  // 120 degrees
constexpr double COS_HALF = 0.5773502691896257, SIN_HALF = 0.816496580927726;   // beta = theta / 2
constexpr double INV_SQRT3 = 0.5773502691896258;

struct HyArgs {
  MolArrays mol;
  HydrogenTable tab;
  HydrogenOperands o;
  int num_element, num_bond_types;
};

struct D3 {
  double x, y, z;
};

struct HyShared {
  D3 pos[MOL_ATOMS];              // the heavy atoms, float64
  D3 hpos[HY_SLOTS];              // slot 4 a + k: atom a's k-th hydrogen
  unsigned bond[MOL_BONDS];       // the bond word of mdx_mol.h, payload = order (1 .. 3) | aromatic << 2: the low bits of an adj entry
  unsigned nb3[MOL_ATOMS];        // the first three neighbours in ascending index, a byte each | min(degree, 255) << 24
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS], wave_total[4];
  int red[4][HY_STATS];
  double wmin[4];
  double len[HY_MAX_ELEMENTS];        // the X-H length per class
  unsigned short adj[2 * MOL_BONDS];  // neighbour << 3 | aromatic << 2 | order: a row sorted by the word is sorted by neighbour
  unsigned short hlist[HY_SLOTS];     // the placed slots in (atom, k) order
  unsigned char g1[MOL_ATOMS];        // the geometry by the first rule
  unsigned char fin[MOL_ATOMS];       // every coordinate finite
};

__device__ inline D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline double norm(D3 a) { return sqrt(dot(a, a)); }
// p a + q b, component by component
__device__ inline D3 comb(double p, D3 a, double q, D3 b) { return {p * a.x + q * b.x, p * a.y + q * b.y, p * a.z + q * b.z}; }
// -a / l
__device__ inline D3 neg_over(D3 a, double l) { return {-a.x / l, -a.y / l, -a.z / l}; }
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

// the k-th fixed world direction of a geometry (d = 0)
__device__ inline D3 world_dir(int geom, int k) {
  if (geom == GEOM_TETRAHEDRAL) {
    const double c = INV_SQRT3;
    return k == 0 ? D3{c, c, c} : k == 1 ? D3{c, -c, -c} : k == 2 ? D3{-c, c, -c} : D3{-c, -c, c};
  }
  if (geom == GEOM_TRIGONAL) return k == 0 ? D3{1.0, 0.0, 0.0} : k == 1 ? D3{COS_TRI, SIN_TRI, 0.0} : D3{COS_TRI, -SIN_TRI, 0.0};
  return k == 0 ? D3{1.0, 0.0, 0.0} : D3{-1.0, 0.0, 0.0};
}

// The unit vector from atom `a` to its neighbour `b` -> ok cleared when either is not finite or they coincide
__device__ inline D3 to_neighbour(const HyShared& s, int a, int b, bool& ok) {
  if (!s.fin[b]) ok = false;
  return unit(sub(s.pos[b], s.pos[a]), ok);
}

// Places the h hydrogens of atom a (h >= 1, d + h <= room, d = its degree) into s.hpos[4 a ..] -> whether they are placed (false: the
// atom is DEGENERATE and its slots stay 0); world: the WORLD_FRAME flag
__device__ inline bool place_atom(HyShared& s, int a, int geom, int d, int h, double L, double deg_tol, bool& world) {
  world = false;
  if (!s.fin[a]) return false;
  const D3 p = s.pos[a];
  const unsigned w3 = s.nb3[a];
  D3 dir[HY_MAX_H] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // constant indices only: registers
  bool ok = true;
  if (d == 0) {
    world = true;
#pragma unroll
    for (int k = 0; k < HY_MAX_H; ++k) dir[k] = world_dir(geom, k);
  } else if (d == 1) {
    const int n1 = w3 & 0xffu;
    const D3 e = to_neighbour(s, a, n1, ok);
    if (!ok) return false;
    if (geom == GEOM_LINEAR) {
      dir[0] = {-e.x, -e.y, -e.z};
    } else {
      D3 w = {0.0, 0.0, 0.0};
      bool found = false;
      for (int q = s.off[n1]; q < s.off[n1 + 1] && !found; ++q) {  // ascending neighbour index
        const int r = s.adj[q] >> 3;
        if (r == a || !s.fin[r]) continue;
        bool okr = true;
        const D3 wv = unit(sub(s.pos[r], s.pos[n1]), okr);
        if (!okr) continue;
        if (norm(cross(e, wv)) >= deg_tol) w = wv, found = true;
      }
      if (!found) {
        const double ax = fabs(e.x), ay = fabs(e.y), az = fabs(e.z);
        w = ax <= ay && ax <= az ? D3{1.0, 0.0, 0.0} : ay <= az ? D3{0.0, 1.0, 0.0} : D3{0.0, 0.0, 1.0};
        world = true;
      }
      const double t = dot(w, e);
      const D3 f1 = unit(D3{w.x - t * e.x, w.y - t * e.y, w.z - t * e.z}, ok);
      if (!ok) return false;
      const D3 f2 = cross(e, f1);
      const bool tet = geom == GEOM_TETRAHEDRAL;
      const double ct = tet ? COS_TET : COS_TRI, st = tet ? SIN_TET : SIN_TRI;
      // phi = 180 + 120 k (tetrahedral), 180 then 0 (trigonal)
      const double cp[3] = {-1.0, tet ? 0.5 : 1.0, 0.5}, sp[3] = {0.0, tet ? -SIN_TRI : 0.0, SIN_TRI};
#pragma unroll
      for (int k = 0; k < 3; ++k) dir[k] = comb(ct, e, st, comb(cp[k], f1, sp[k], f2));
    }
  } else if (d == 2) {
    const D3 u0 = to_neighbour(s, a, w3 & 0xffu, ok), u1 = to_neighbour(s, a, (w3 >> 8) & 0xffu, ok);
    if (!ok) return false;
    const D3 sv = add(u0, u1);
    const double ns = norm(sv);
    if (geom == GEOM_TRIGONAL) {
      if (!(ns >= deg_tol)) return false;
      dir[0] = neg_over(sv, ns);
    } else {
      const D3 c = cross(u0, u1);
      const double nc = norm(c);
      if (!(nc >= deg_tol) || !(ns > 0.0)) return false;
      const D3 b = neg_over(sv, ns), nh = {c.x / nc, c.y / nc, c.z / nc};
      dir[0] = comb(COS_HALF, b, SIN_HALF, nh);
      dir[1] = comb(COS_HALF, b, -SIN_HALF, nh);
    }
  } else {  // d == 3: tetrahedral, one hydrogen
    const D3 u0 = to_neighbour(s, a, w3 & 0xffu, ok), u1 = to_neighbour(s, a, (w3 >> 8) & 0xffu, ok), u2 = to_neighbour(s, a, (w3 >> 16) & 0xffu, ok);
    if (!ok) return false;
    const D3 sv = add(add(u0, u1), u2);
    const double ns = norm(sv);
    if (!(ns >= deg_tol)) return false;
    dir[0] = neg_over(sv, ns);
  }
#pragma unroll
  for (int k = 0; k < HY_MAX_H; ++k)
    if (k < h) s.hpos[HY_MAX_H * a + k] = {p.x + L * dir[k].x, p.y + L * dir[k].y, p.z + L * dir[k].z};
  return true;
}

// status and zeros for a molecule that is not measured; its per-atom slots only when they are inside the arrays
__device__ inline void write_unmeasured(const HyArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  if (tid < HY_STATS) A.o.mol_stats[(size_t)m * HY_STATS + tid] = tid == H_STATUS ? status : 0;
  if (tid == 0) A.o.min_contact[m] = 0.0;
  if (v.outside) return;
  for (long long a = v.n0 + tid; a < v.n0 + v.n; a += 256) {
    A.o.h_count[a] = 0, A.o.atom_flag[a] = 0;
    for (int q = 0; q < 3 * HY_MAX_H; ++q) A.o.h_pos[3 * HY_MAX_H * a + q] = 0.0;
  }
}

__global__ __launch_bounds__(256) void mol_hydrogens_kernel(const HyArgs A) {
  __shared__ HyShared s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  const bool in = tid < n;
  const int *bt = A.mol.bond_type + h0, *bo = A.o.order + h0;
  const int nbt = A.num_bond_types;

  // ---- the molecule into LDS: positions, bonds, the adjacency as CSR with sorted rows
  {
    bool fin = false;
    D3 p = {0.0, 0.0, 0.0};
    if (in) {
      const float* q = A.o.atom_pos + 3 * (n0 + tid);
      const float x = q[0], y = q[1], z = q[2];
      fin = isfinite(x) && isfinite(y) && isfinite(z);
      p = {(double)x, (double)y, (double)z};
    }
    s.pos[tid] = p, s.fin[tid] = fin ? 1 : 0;
    if (tid < HY_MAX_ELEMENTS) s.len[tid] = A.tab.length[tid];
#pragma unroll
    for (int k = 0; k < HY_MAX_H; ++k) s.hpos[HY_MAX_H * tid + k] = {0.0, 0.0, 0.0};
  }
  mol_stage_bonds(A.mol, h0, n, nb, s.bond, s.off, s.cur, s.wave_total,
                  [&](int e, int, int) { return (unsigned)min(max(bo[e], 1), 3) | (bt[e] == nbt ? 4u : 0u); });
  mol_stage_rows(nb, s.bond, s.cur, s.adj, [](unsigned other, int, unsigned bd) { return (unsigned short)(other << 3 | mol_bond_payload(bd)); });
  int d = 0;
  {
    const int r0 = in ? s.off[tid] : 0, r1 = in ? s.off[tid + 1] : 0;
    d = r1 - r0;
    for (int q = r0 + 1; q < r1; ++q) {  // the rows arrive in any order: insertion sort by the word, the neighbour in its high bits, each thread its own row
      const unsigned short x = s.adj[q];
      int k = q - 1;
      for (; k >= r0 && s.adj[k] > x; --k) s.adj[k + 1] = s.adj[k];
      s.adj[k + 1] = x;
    }
    int n2 = 0, n3 = 0, arom = 0;
    unsigned w3 = (unsigned)min(d, 255) << 24;
    for (int q = r0; q < r1; ++q) {
      const unsigned w = s.adj[q], o = w & 3u;
      n2 += o == 2u, n3 += o == 3u, arom |= (w >> 2) & 1u;
      if (q - r0 < 3) w3 |= (w >> 3) << (8 * (q - r0));
    }
    s.nb3[tid] = w3;
    s.g1[tid] = (unsigned char)(n3 >= 1 || n2 >= 2 ? GEOM_LINEAR : n2 >= 1 || arom ? GEOM_TRIGONAL : GEOM_TETRAHEDRAL);
  }
  __syncthreads();

  // ---- geometry, placement, the atom's own slots
  int wanted = 0, placed = 0, flag = 0;
  if (in) {
    const int cls = A.mol.atom_type[n0 + tid];
    const bool known = (unsigned)cls < (unsigned)A.num_element;
    const int raw = A.o.n_h[n0 + tid];
    const int h = known ? min(max(raw, 0), HY_MAX_H) : 0;  // an atom of a class outside the table carries none
    int geom = s.g1[tid];
    if (geom == GEOM_TETRAHEDRAL && known && ((A.tab.planar >> cls) & 1u)) {
      bool pi = false;
      for (int q = s.off[tid]; q < s.off[tid + 1]; ++q) pi = pi || s.g1[s.adj[q] >> 3] != GEOM_TETRAHEDRAL;
      if (pi) geom = GEOM_TRIGONAL;
    }
    flag = geom | (h != raw ? FLAG_CLAMPED : 0);
    wanted = h;
    if (h >= 1) {
      if (d + h > 4 - geom) {
        flag |= FLAG_NO_ROOM;
      } else {
        bool world = false;
        if (place_atom(s, tid, geom, d, h, s.len[cls], A.tab.deg_tol, world)) placed = h, flag |= world ? FLAG_WORLD_FRAME : 0;
        else flag |= FLAG_DEGENERATE;
      }
    }
    A.o.h_count[n0 + tid] = placed, A.o.atom_flag[n0 + tid] = flag;
    double* out = A.o.h_pos + 3 * HY_MAX_H * (n0 + tid);
#pragma unroll
    for (int k = 0; k < HY_MAX_H; ++k) {
      const D3 q = s.hpos[HY_MAX_H * tid + k];  // written by this thread
      out[3 * k] = q.x, out[3 * k + 1] = q.y, out[3 * k + 2] = q.z;
    }
  }

  // ---- the placed slots in (atom, k) order
  __syncthreads();  // every row and offset has been read
  s.cur[tid] = placed;
  __syncthreads();
  block_exclusive_scan_256(s.off, s.cur, s.wave_total);
  __syncthreads();
  for (int k = 0; k < placed; ++k) s.hlist[s.off[tid] + k] = (unsigned short)(HY_MAX_H * tid + k);  // off[256] <= 1024
  __syncthreads();

  // ---- contacts: (placed H) x (heavy atom, or a later placed H), without the 1-2 and 1-3 pairs
  const int nH = s.off[MOL_ATOMS], M = n + nH, total = nH * M;  // at most 1024 * 1280
  double mn = INFINITY;
  int clash = 0;
  for (int it = tid; it < total; it += 256) {
    const int hi = it / M, j = it - hi * M;
    const int slot = s.hlist[hi], a = slot >> 2;
    D3 q;
    if (j < n) {
      const unsigned w3 = s.nb3[a];
      const int da = w3 >> 24;  // at most 3: the atom has a placed hydrogen
      if (!s.fin[j] || j == a || (da >= 1 && j == (int)(w3 & 0xffu)) || (da >= 2 && j == (int)((w3 >> 8) & 0xffu)) ||
          (da >= 3 && j == (int)((w3 >> 16) & 0xffu)))
        continue;
      q = s.pos[j];
    } else {
      const int hj = j - n;
      if (hj <= hi) continue;
      const int other = s.hlist[hj];
      if ((other >> 2) == a) continue;
      q = s.hpos[other];
    }
    const double dist = norm(sub(q, s.hpos[slot]));
    if (dist < mn) mn = dist;
    clash += dist < A.tab.clash_tol;
  }
  for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o, 64));
  const int row[HY_STATS] = {0, wanted, placed, (flag & FLAG_NO_ROOM) != 0, (flag & FLAG_DEGENERATE) != 0, (flag & FLAG_WORLD_FRAME) != 0, clash};
#pragma unroll
  for (int k = 1; k < HY_STATS; ++k) {
    const int sum = wave_sum(row[k]);
    if (lane == 0) s.red[wave][k] = sum;
  }
  if (lane == 0) s.wmin[wave] = mn;
  __syncthreads();
  if (tid < HY_STATS) A.o.mol_stats[(size_t)m * HY_STATS + tid] = tid == H_STATUS ? 0 : (s.red[0][tid] + s.red[1][tid]) + (s.red[2][tid] + s.red[3][tid]);
  if (tid == 64) A.o.min_contact[m] = fmin(fmin(s.wmin[0], s.wmin[1]), fmin(s.wmin[2], s.wmin[3]));
}

}  // namespace

extern "C" int mdx_mol_hydrogens(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                                 const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index,
                                 int64_t Eh_stride, const int32_t* select, const float* atom_pos, const int32_t* n_h, const int32_t* order,
                                 int32_t num_element, int32_t num_bond_types, const double* xh_length, uint32_t planar_mask, double deg_tol,
                                 double clash_tol, double* h_pos, int32_t* h_count, int32_t* atom_flag, int32_t* mol_stats,
                                 double* min_contact, void* stream) {
  HyArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  a.o = HydrogenOperands{atom_pos, n_h, order, h_pos, h_count, atom_flag, mol_stats, min_contact};
  if (const char* why = hydrogens_check(a.o)) return mdx_set_error(MDX_ERR_ARG, why);
  const char* why = "";
  if (hydrogens_prepare(&a.tab, xh_length, planar_mask, num_element, num_bond_types, deg_tol, clash_tol, &why) != HY_PREP_OK)
    return mdx_set_error(MDX_ERR_ARG, why);
  a.num_element = num_element, a.num_bond_types = num_bond_types;
  return mol_launch(mol_hydrogens_kernel, "mol_hydrogens_kernel", B, stream, a);
}
