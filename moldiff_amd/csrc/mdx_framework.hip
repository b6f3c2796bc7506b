// Frameworks and ring systems of decoded molecules on the device (mdx_mol_framework): every molecule is cut into its framework (the
// 2-core of the bond graph, optionally with the double-bonded exo atoms on it), its ring systems, linkers and side chains, and the
// framework and every ring system are handed back as compact molecules that mdx_mol_canon, mdx_mol_rings and mdx_mol_kekulize take
// unchanged.  It is THIS PROJECT'S OWN DEFINITION, not rdkit.Chem.Scaffolds.MurckoScaffold; the definition and every output are
// stated in include/moldiff_hip.h, moldiff_amd/framework.py restates the function (framework_ref) and the GPU tests compare every
// output exactly.
//
// One workgroup of 256 threads (4 waves) per molecule over the compact arrays of mdx_mol.h, thread a = atom a, the bonds strided over
// the block; a molecule has at most 256 atoms and 512 bonds (the caps of mdx_mol_rings, whose bond_ring_min and status are inputs).
// Everything lives in LDS, about 19 KB (8 workgroups per CU, the bound of its waves); there is no workspace and no scratch.
//   (a) the bonds with their ring flag, degrees by LDS integer atomics, offsets by a scan, adjacency lists;
//   (b) the core: every live atom counts its live neighbours and dies with at most one, round by round, until a block-wide "changed"
//       flag stays clear.  Deleting all such atoms of a round at once reaches the same fixed point as deleting them one by one;
//   (c) roles; ring systems by propagating the smallest atom index over the ring bonds to a fixed point; system ordinals, the new
//       atom and bond numbers of the framework by scans (a thread owns two neighbouring bonds, so the order is kept);
//   (d) thread k = system k walks the atoms and bonds once to count its own and once to place them, in ascending index;
//   (e) every output slot of the molecule is written ONCE, by the thread that owns the slot, through the inverse maps of (c) and (d):
//       plain vector stores, no atomics on global memory, no slot written twice.
// LDS atomics add integers only, so every value is independent of the order in which they land.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_framework_args.h"
#include "mdx_mol.h"

namespace {

constexpr int FW_NONE = 0x7fff;
constexpr unsigned FW_RING = 1u, FW_ADJ_RING = 1u << 17;  // a ring bond: in the payload of the bond word, in an adjacency entry
enum { ROLE_SIDE, ROLE_LINKER, ROLE_RING, ROLE_EXO };
enum { F_STATUS, F_ATOMS, F_BONDS, F_SYSTEMS, F_LINKER, F_SIDE, F_EXO, F_FUSION, F_LARGEST, F_MOST_RINGS };
static_assert(F_MOST_RINGS + 1 == FW_STATS && FW_STATS == MDX_FW_STATS, "the columns of mol_stats");

struct FwArgs {
  MolArrays mol;
  FrameworkOperands o;
  int mode, sys_bins;
};

struct FwShared {
  unsigned bond[MOL_BONDS];             // the bond word of mdx_mol.h, payload = FW_RING or 0
  unsigned adj[2 * MOL_BONDS];          // neighbour | bond << 8 | FW_ADJ_RING
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS];  // adjacency offsets; degree, then fill cursor
  int pre[MOL_ATOMS + 1], cnt[MOL_ATOMS];  // the scans of (c) and (d)
  int wave_total[4], hist[FW_MAX_BINS], top[2];
  short label[MOL_ATOMS];              // the smallest atom of the ring system, FW_NONE outside every system
  short asys[MOL_ATOMS], bsys[MOL_BONDS];  // the system ordinal of an atom / a ring bond, -1 without one
  unsigned short sys_a0[MOL_ATOMS], sys_b0[MOL_ATOMS], sys_na[MOL_ATOMS], sys_nb[MOL_ATOMS];  // per system, molecule-local
  unsigned short fw_atom[MOL_ATOMS], fw_atom_inv[MOL_ATOMS], fw_bond_inv[MOL_BONDS];      // new number of an atom; atom / bond of a new number
  unsigned short sys_atom[MOL_ATOMS], sys_atom_inv[MOL_ATOMS], sys_bond_inv[MOL_BONDS];   // place of an atom in the system arrays; the inverses
  unsigned char alive[MOL_ATOMS], role[MOL_ATOMS], brole[MOL_BONDS];
};

// status and zeros for a molecule that is not measured; its per-atom and per-bond slots only when they are inside the arrays
__device__ inline void write_unmeasured(const FwArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  const FrameworkOperands& o = A.o;
  if (tid < FW_STATS) o.mol_stats[(size_t)m * FW_STATS + tid] = tid == F_STATUS ? status : 0;
  if (tid < A.sys_bins) o.sys_hist[(size_t)m * A.sys_bins + tid] = 0;
  if (v.outside) return;
  for (long long a = v.n0 + tid; a < v.n0 + v.n; a += 256) {
    o.atom_role[a] = 0, o.atom_system[a] = -1;
    o.fw_atom_type[a] = 0, o.fw_atom_map[a] = 0, o.sys_atom_type[a] = 0, o.sys_atom_map[a] = 0;
    o.sys_atom_ptr[a] = 0, o.sys_bond_ptr[a] = 0, o.sys_n_atoms[a] = 0, o.sys_n_bonds[a] = 0;
    if (o.fw_pos)
      for (int c = 0; c < 3; ++c) o.fw_pos[3 * a + c] = 0.f, o.sys_pos[3 * a + c] = 0.f;
  }
  for (long long e = v.h0 + tid; e < v.h0 + v.nb; e += 256) {
    o.bond_role[e] = 0, o.fw_bond_type[e] = 0, o.sys_bond_type[e] = 0;
    o.fw_bond_index[e] = 0, o.fw_bond_index[A.mol.E_cap + e] = 0, o.sys_bond_index[e] = 0, o.sys_bond_index[A.mol.E_cap + e] = 0;
  }
}

__device__ inline bool in_core(int role) { return role == ROLE_LINKER || role == ROLE_RING; }

__global__ __launch_bounds__(256) void mol_framework_kernel(const FwArgs A) {
  __shared__ FwShared s;
  const int m = blockIdx.x, tid = threadIdx.x;
  const FrameworkOperands& o = A.o;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  if (o.ring_status[m] != 0) {  // uniform
    write_unmeasured(A, m, 2, v);
    return;
  }
  const int* bt = A.mol.bond_type + h0;
  const bool in = tid < n, generic = (A.mode & FW_MODE_GENERIC) != 0;

  // ---- (a) the molecule into LDS: bonds with their ring flag, degrees, adjacency lists
  if (tid < FW_MAX_BINS) s.hist[tid] = 0;
  if (tid < 2) s.top[tid] = 0;
  mol_stage_bonds(A.mol, h0, n, nb, s.bond, s.off, s.cur, s.wave_total,
                  [&](int e, int, int) { return o.bond_ring_min[h0 + e] != 0 ? FW_RING : 0u; });
  s.alive[tid] = in;
  // the order inside a row does not matter: rows are only counted and minimised over
  mol_stage_rows(nb, s.bond, s.cur, s.adj, [](unsigned other, int e, unsigned bd) {
    return other | (unsigned)e << 8 | (mol_bond_payload(bd) & FW_RING ? FW_ADJ_RING : 0u);
  });
  const int a0 = in ? s.off[tid] : 0, a1 = in ? s.off[tid + 1] : 0;
  int ring_deg = 0;
  for (int p = a0; p < a1; ++p) ring_deg += (s.adj[p] & FW_ADJ_RING) != 0;
  const bool ring = ring_deg > 0;

  // ---- (b) the core: an atom with at most one live neighbour dies; at most n / 2 rounds
  for (;;) {
    int live = 0;
    if (s.alive[tid])
      for (int p = a0; p < a1; ++p) live += s.alive[s.adj[p] & 0xffu];
    const bool die = s.alive[tid] && live <= 1;
    __syncthreads();  // every count of the round has been taken
    if (die) s.alive[tid] = 0;
    if (!__syncthreads_or(die)) break;
  }

  // ---- (c) roles
  const bool core = s.alive[tid] != 0;
  int role = core ? (ring ? ROLE_RING : ROLE_LINKER) : ROLE_SIDE;
  if ((A.mode & FW_MODE_EXO) && in && !core && a1 - a0 == 1) {
    const unsigned ent = s.adj[a0];
    if (bt[(ent >> 8) & 0x1ffu] == 2 && s.alive[ent & 0xffu]) role = ROLE_EXO;
  }
  s.role[tid] = (unsigned char)role;
  // ring systems: the smallest atom index spreads over the ring bonds
  s.label[tid] = (short)(ring ? tid : FW_NONE);
  __syncthreads();
  for (;;) {
    const int mine = s.label[tid];
    int least = mine;
    if (ring)
      for (int p = a0; p < a1; ++p) {
        const unsigned ent = s.adj[p];
        if (ent & FW_ADJ_RING) least = min(least, (int)s.label[ent & 0xffu]);
      }
    __syncthreads();  // every label of the round has been read
    if (least < mine) s.label[tid] = (short)least;
    if (!__syncthreads_or(least < mine)) break;
  }
  // the new atom numbers of the framework
  const bool in_fw = role != ROLE_SIDE;
  s.cnt[tid] = in_fw;
  __syncthreads();
  block_exclusive_scan_256(s.pre, s.cnt, s.wave_total);
  __syncthreads();
  const int n_fw = s.pre[MOL_ATOMS];
  s.fw_atom[tid] = (unsigned short)(in_fw ? s.pre[tid] : 0);
  if (in_fw) s.fw_atom_inv[s.pre[tid]] = (unsigned short)tid;
  __syncthreads();
  // the system ordinals: systems in the order of their smallest atoms
  const bool root = ring && s.label[tid] == tid;
  s.cnt[tid] = root;
  __syncthreads();
  block_exclusive_scan_256(s.pre, s.cnt, s.wave_total);
  __syncthreads();
  const int n_sys = s.pre[MOL_ATOMS];
  const int sys = ring ? s.pre[s.label[tid]] : -1;  // the roots before a root = its ordinal
  s.asys[tid] = (short)sys;
  __syncthreads();  // role, asys
  // bond roles and the new bond numbers of the framework
  for (int e = tid; e < nb; e += 256) {
    const unsigned bd = s.bond[e];
    int br = 0, bs = -1;
    if (bd) {
      const int ri = s.role[mol_bond_i(bd)], rj = s.role[mol_bond_j(bd)];
      if (mol_bond_payload(bd) & FW_RING)
        br = 2, bs = s.asys[mol_bond_i(bd)];
      else if (in_core(ri) && in_core(rj))
        br = 1;
      else if ((ri == ROLE_EXO && in_core(rj)) || (rj == ROLE_EXO && in_core(ri)))
        br = 3;
    }
    s.brole[e] = (unsigned char)br, s.bsys[e] = (short)bs;
  }
  __syncthreads();
  const int e0 = 2 * tid;  // this thread's two bonds
  const bool keep0 = e0 < nb && s.brole[e0] != 0, keep1 = e0 + 1 < nb && s.brole[e0 + 1] != 0;
  s.cnt[tid] = (int)keep0 + (int)keep1;
  __syncthreads();
  block_exclusive_scan_256(s.pre, s.cnt, s.wave_total);
  __syncthreads();
  const int n_fw_bonds = s.pre[MOL_ATOMS];
  if (keep0) s.fw_bond_inv[s.pre[tid]] = (unsigned short)e0;
  if (keep1) s.fw_bond_inv[s.pre[tid] + (int)keep0] = (unsigned short)(e0 + 1);
  __syncthreads();

  // ---- (d) thread k = system k: its sizes, then the places of its atoms and bonds in ascending index
  int na = 0, nbk = 0;
  if (tid < n_sys) {
    for (int a = 0; a < n; ++a) na += s.asys[a] == tid;
    for (int e = 0; e < nb; ++e) nbk += s.bsys[e] == tid;
  }
  s.cnt[tid] = na;
  __syncthreads();
  block_exclusive_scan_256(s.pre, s.cnt, s.wave_total);
  __syncthreads();
  const int first_atom = s.pre[tid], n_ring_atoms = s.pre[MOL_ATOMS];
  __syncthreads();
  s.cnt[tid] = nbk;
  __syncthreads();
  block_exclusive_scan_256(s.pre, s.cnt, s.wave_total);
  __syncthreads();
  const int first_bond = s.pre[tid], n_ring_bonds = s.pre[MOL_ATOMS];
  s.sys_a0[tid] = (unsigned short)first_atom, s.sys_b0[tid] = (unsigned short)first_bond;
  s.sys_na[tid] = (unsigned short)na, s.sys_nb[tid] = (unsigned short)nbk;
  if (tid < n_sys) {
    int p = first_atom;
    for (int a = 0; a < n; ++a)
      if (s.asys[a] == tid) s.sys_atom[a] = (unsigned short)p, s.sys_atom_inv[p++] = (unsigned short)a;
    p = first_bond;
    for (int e = 0; e < nb; ++e)
      if (s.bsys[e] == tid) s.sys_bond_inv[p++] = (unsigned short)e;
    const int rings = nbk - na + 1;  // >= 1 with the ring data of mdx_mol_rings; clamped for any other
    atomicAdd(&s.hist[min(max(rings - 1, 0), A.sys_bins - 1)], 1);
    atomicMax(&s.top[0], na), atomicMax(&s.top[1], rings);
  }
  const int n_linker = __syncthreads_count(in && role == ROLE_LINKER);
  const int n_side = __syncthreads_count(in && role == ROLE_SIDE);
  const int n_exo = __syncthreads_count(role == ROLE_EXO);
  const int n_fusion = __syncthreads_count(ring && ring_deg >= 3);

  // ---- (e) results: every slot of the molecule once, by the thread of the slot
  if (in) {
    const long long q = n0 + tid;
    o.atom_role[q] = role, o.atom_system[q] = sys;
    int src = -1;  // the framework atom of this slot
    if (tid < n_fw) src = s.fw_atom_inv[tid];
    o.fw_atom_type[q] = src >= 0 && !generic ? A.mol.atom_type[n0 + src] : 0, o.fw_atom_map[q] = max(src, 0);
    if (o.fw_pos)
      for (int c = 0; c < 3; ++c) o.fw_pos[3 * q + c] = src >= 0 ? o.atom_pos[3 * (n0 + src) + c] : 0.f;
    src = tid < n_ring_atoms ? (int)s.sys_atom_inv[tid] : -1;  // the ring atom of this slot
    o.sys_atom_type[q] = src >= 0 && !generic ? A.mol.atom_type[n0 + src] : 0, o.sys_atom_map[q] = max(src, 0);
    if (o.sys_pos)
      for (int c = 0; c < 3; ++c) o.sys_pos[3 * q + c] = src >= 0 ? o.atom_pos[3 * (n0 + src) + c] : 0.f;
    const bool rec = tid < n_sys;  // the record of system tid
    o.sys_atom_ptr[q] = rec ? (int)(n0 + first_atom) : 0, o.sys_bond_ptr[q] = rec ? (int)(h0 + first_bond) : 0;
    o.sys_n_atoms[q] = rec ? na : 0, o.sys_n_bonds[q] = rec ? nbk : 0;
  }
  for (int e = tid; e < nb; e += 256) {
    const long long q = h0 + e;
    o.bond_role[q] = s.brole[e];
    int x = 0, y = 0, t = 0;
    if (e < n_fw_bonds) {
      const int src = s.fw_bond_inv[e];
      const unsigned bd = s.bond[src];
      x = s.fw_atom[mol_bond_i(bd)], y = s.fw_atom[mol_bond_j(bd)], t = generic ? 1 : bt[src];
    }
    o.fw_bond_index[q] = x, o.fw_bond_index[A.mol.E_cap + q] = y, o.fw_bond_type[q] = t;
    x = y = t = 0;
    if (e < n_ring_bonds) {
      const int src = s.sys_bond_inv[e];
      const unsigned bd = s.bond[src];
      const int base = s.sys_a0[s.bsys[src]];
      x = s.sys_atom[mol_bond_i(bd)] - base, y = s.sys_atom[mol_bond_j(bd)] - base, t = generic ? 1 : bt[src];
    }
    o.sys_bond_index[q] = x, o.sys_bond_index[A.mol.E_cap + q] = y, o.sys_bond_type[q] = t;
  }
  if (tid < A.sys_bins) o.sys_hist[(size_t)m * A.sys_bins + tid] = s.hist[tid];
  if (tid < FW_STATS) {
    const int val[FW_STATS] = {0, n_fw, n_fw_bonds, n_sys, n_linker, n_side, n_exo, n_fusion, s.top[0], s.top[1]};
    int out = 0;
    for (int k = 0; k < FW_STATS; ++k) out = tid == k ? val[k] : out;  // a select chain: no array indexed at run time
    o.mol_stats[(size_t)m * FW_STATS + tid] = out;
  }
}

}  // namespace

extern "C" int mdx_mol_framework(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms,
                                 const int32_t* n_bonds, const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type,
                                 const int32_t* bond_index, int64_t Eh_stride, const int32_t* select, const float* atom_pos,
                                 const int32_t* bond_ring_min, const int32_t* ring_status, int32_t mode, int32_t sys_bins,
                                 int32_t* atom_role, int32_t* atom_system, int32_t* bond_role, int32_t* mol_stats, int32_t* sys_hist,
                                 int32_t* fw_atom_type, int32_t* fw_atom_map, float* fw_pos, int32_t* fw_bond_index,
                                 int32_t* fw_bond_type, int32_t* sys_atom_ptr, int32_t* sys_bond_ptr, int32_t* sys_n_atoms,
                                 int32_t* sys_n_bonds, int32_t* sys_atom_type, int32_t* sys_atom_map, float* sys_pos,
                                 int32_t* sys_bond_index, int32_t* sys_bond_type, void* stream) {
  FwArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  a.o = FrameworkOperands{atom_pos,     bond_ring_min, ring_status,  atom_role,    atom_system,  bond_role,     mol_stats,
                          sys_hist,     fw_atom_type,  fw_atom_map,  fw_bond_index, fw_bond_type, sys_atom_ptr,  sys_bond_ptr,
                          sys_n_atoms,  sys_n_bonds,   sys_atom_type, sys_atom_map, sys_bond_index, sys_bond_type, fw_pos,
                          sys_pos};
  if (const char* why = framework_check(a.o, mode, sys_bins)) return mdx_set_error(MDX_ERR_ARG, why);
  a.mode = mode, a.sys_bins = sys_bins;
  return mol_launch(mol_framework_kernel, "mol_framework_kernel", B, stream, a);
}
