// Symmetry-aware best RMSD between conformers on the device (mdx_mol_bestrms): for a probe molecule and each of its targets of the same
// constitution, the mean squared deviation after optimal rigid superposition, minimised over every atom map that the symmetry of the
// labelled graph allows -- what rdMolAlign.GetBestRMS reports as a root.  The quantity and every output are stated in
// include/moldiff_hip.h; moldiff_amd/rmsd.py restates it (best_rms_ref: numpy's SVD) and the GPU tests compare against that.
//
// One workgroup of 256 threads (4 waves) per probe, thread a = atom a, as mol_canon_kernel, and the same walk: the staging, the
// refinement and the tree of mdx_canon_body.h, so nodes, depth and leaves are canon's.  This file is the geometry and the leaf.
//   Once per probe: the canonical certificate is rebuilt from the given rank and sorted (as mdx_stereo.hip does); the float32 positions
//   are read into float64, centred and kept in LDS with Ga = sum |p|^2.
//   Once per pair: the target's centroid and Gb.  When the pairs of the probe fit (at most 64 pairs and 1,024 atoms in all) the centred
//   targets are staged in LDS; otherwise a leaf reads them from global memory and centres them again, with the same sums.
//   A leaf is optimal iff every bond word of it stands in the canonical certificate (find_word).  At an optimal leaf wave w takes the
//   pairs w, w + 4, ...: each lane sums its atoms a = lane, lane + 64, ... of the 9 entries of H = sum p_a q_{c[a]}^T in that order, a
//   butterfly (wave_sum) adds the lanes, and every lane solves Horn's 4 x 4 quaternion matrix by cyclic Jacobi (mdx_bestrms_args.h): the
//   largest eigenvalue gives msd, the smallest the mirror value.  No block barrier inside the leaf.  The order of every sum is fixed, so
//   the results repeat bit by bit and do not depend on the probe's place in the batch.
//   The running minima of a pair live in its output row and are read and written by lane 0 of the wave that owns the pair.
// LDS: 58,864 B (the walk 25,328, the probe 6,144, the staged targets 24,576 + 512, the certificate and the given rank 2,304), so two
// workgroups share a CU; 90 VGPRs.  No workspace, no global atomics, no scratch: H and the 4 x 4 matrix are indexed with constants only.  All
// outputs are plain stores by the probe's own workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_bestrms_args.h"
#include "mdx_canon_body.h"
#include "mdx_mol.h"

namespace {

enum { R_STATUS, R_NODES, R_AUT };
static_assert(R_AUT + 1 == BR_STATS && BR_STATS == MDX_BESTRMS_STATS, "the columns of mol_stats");
constexpr int BR_STAGE_ATOMS = 1024, BR_STAGE_PAIRS = 64;

struct BrArgs {
  MolArrays mol;
  BestrmsOperands o;
  long long P_cap, tgt_atoms;
  int T, max_nodes;
};

struct BrShared {
  CnGraph g;                         // the walk's own state (mdx_canon_body.h)
  double p[3][MOL_ATOMS];            // the probe, centred
  double q[3][BR_STAGE_ATOMS];       // the staged targets, centred: pair k at k n
  double Gb[BR_STAGE_PAIRS];
  unsigned cw[MOL_BONDS];            // the canonical certificate, from the given rank
  unsigned char crank[MOL_ATOMS];
};

struct Frame {
  double cx, cy, cz, G;  // the centroid and the sum of the squared distances from it
};

// centroid and G of the n >= 1 points at pos (3 floats each) by one wave: lane l adds its points l, l + 64, ... in turn, then the lanes
// are added by the butterfly.  The same in every lane.
__device__ inline Frame wave_frame(const float* pos, int n, int lane) {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int a = lane; a < n; a += 64) sx += (double)pos[3 * a], sy += (double)pos[3 * a + 1], sz += (double)pos[3 * a + 2];
  Frame f;
  f.cx = wave_sum(sx) / (double)n, f.cy = wave_sum(sy) / (double)n, f.cz = wave_sum(sz) / (double)n;
  double g = 0.0;
  for (int a = lane; a < n; a += 64) {
    const double dx = (double)pos[3 * a] - f.cx, dy = (double)pos[3 * a + 1] - f.cy, dz = (double)pos[3 * a + 2] - f.cz;
    g += (dx * dx + dy * dy) + dz * dz;
  }
  f.G = wave_sum(g);
  return f;
}

// the target of pair `pr` when it can be read as n atoms, else nullptr (status 3)
__device__ inline const float* pair_target_pos(const BrArgs& A, long long pr, int n) {
  const int t = A.o.pair_target[pr];
  if ((unsigned)t >= (unsigned)A.T) return nullptr;
  const long long q0 = A.o.tgt_ptr[t];
  if (A.o.tgt_n[t] != n || q0 < 0 || q0 + n > A.tgt_atoms) return nullptr;
  return A.o.tgt_pos + 3 * q0;
}

// msd and its mirror value of the atom map a -> rank[a] for pair k of the probe (its target at tq), by one wave; the same in every lane
__device__ inline void pair_eval(const BrShared& s, const unsigned char* rank, int n, int lane, bool staged, int k, const float* tq, double Ga,
                                 double& msd, double& mirror) {
  double h[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double Gb;
  if (staged) {
    Gb = s.Gb[k];
    const double *qx = s.q[0] + k * n, *qy = s.q[1] + k * n, *qz = s.q[2] + k * n;
    for (int a = lane; a < n; a += 64) {
      const int c = rank[a];
      const double px = s.p[0][a], py = s.p[1][a], pz = s.p[2][a], x = qx[c], y = qy[c], z = qz[c];
      h[0] += px * x, h[1] += px * y, h[2] += px * z, h[3] += py * x, h[4] += py * y, h[5] += py * z, h[6] += pz * x, h[7] += pz * y, h[8] += pz * z;
    }
  } else {
    const Frame f = wave_frame(tq, n, lane);
    Gb = f.G;
    for (int a = lane; a < n; a += 64) {
      const int c = rank[a];
      const double px = s.p[0][a], py = s.p[1][a], pz = s.p[2][a];
      const double x = (double)tq[3 * c] - f.cx, y = (double)tq[3 * c + 1] - f.cy, z = (double)tq[3 * c + 2] - f.cz;
      h[0] += px * x, h[1] += px * y, h[2] += px * z, h[3] += py * x, h[4] += py * y, h[5] += py * z, h[6] += pz * x, h[7] += pz * y, h[8] += pz * z;
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = wave_sum(h[i]);
  double lmax, lmin;
  bestrms_solve(h, &lmax, &lmin);
  bestrms_msd(Ga + Gb, lmax, lmin, n, &msd, &mirror);
}

// zeros and `status` in the probe's row and in the rows of its pairs
__device__ inline void write_unmeasured(const BrArgs& A, int m, int status, long long p0, int np) {
  const int tid = threadIdx.x;
  if (tid < BR_STATS) A.o.mol_stats[(size_t)m * BR_STATS + tid] = tid == R_STATUS ? status : 0;
  for (long long pr = p0 + tid; pr < p0 + np; pr += 256) {
    A.o.msd[pr] = 0.0, A.o.msd_mirror[pr] = 0.0, A.o.msd_first[pr] = 0.0;
    A.o.pair_stats[2 * pr] = 0, A.o.pair_stats[2 * pr + 1] = status;
  }
}

__global__ __launch_bounds__(256) void mol_bestrms_kernel(const BrArgs A) {
  __shared__ BrShared s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MolView v = mol_view(A.mol, m);
  if (v.outside) return;  // uniform; nothing of the molecule may be read, and nothing is written for it
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  long long p0 = A.o.pair_ptr[m];
  const long long p1 = A.o.pair_ptr[m + 1];
  const int np = p0 < 0 || p1 < p0 || p1 > A.P_cap ? 0 : (int)(p1 - p0);  // a pair extent that leaves the arrays is no pair at all
  if (np == 0) p0 = 0;
  if (v.masked) {  // uniform
    write_unmeasured(A, m, 0, p0, np);
    return;
  }
  if (A.o.canon_status[m] != 0 || n > MOL_ATOMS || nb > MOL_BONDS) {  // uniform
    write_unmeasured(A, m, 1, p0, np);
    return;
  }
  const bool in = tid < n;
  const int label = in ? (A.o.atom_label ? A.o.atom_label[n0 + tid] : A.mol.atom_type[n0 + tid]) : 0;
  const int given = in ? A.o.rank[n0 + tid] : 0;
  const int nbv = stage_molecule(s.g, A.mol, h0, n, nb, label);      // the valid bonds
  if (__syncthreads_or(in && (unsigned)given >= (unsigned)n)) {  // not a rank of mdx_mol_canon: nothing may be indexed with it
    write_unmeasured(A, m, 1, p0, np);
    return;
  }
  s.crank[tid] = (unsigned char)given;

  // ---- the canonical certificate from the given rank
  int P = 2;
  while (P < nb) P <<= 1;
  __syncthreads();
  for (int e = tid; e < P; e += 256) s.cw[e] = bond_word(e < nb ? s.g.bond[e] : 0u, s.crank);
  sort_words(s.cw, P);

  // ---- the probe, centred; every wave computes the same frame
  const float* pos = A.o.atom_pos + 3 * n0;
  double Ga = 0.0;
  if (n > 0) {
    const Frame f = wave_frame(pos, n, lane);
    Ga = f.G;
    if (in) s.p[0][tid] = (double)pos[3 * tid] - f.cx, s.p[1][tid] = (double)pos[3 * tid + 1] - f.cy, s.p[2][tid] = (double)pos[3 * tid + 2] - f.cz;
  }
  // ---- the targets: staged when they fit, and the value of the given rank's own map
  const bool staged = np <= BR_STAGE_PAIRS && (long long)np * n <= BR_STAGE_ATOMS;
  if (staged && n > 0)
    for (int k = wave; k < np; k += 4) {
      const float* tq = pair_target_pos(A, p0 + k, n);
      if (!tq) continue;  // uniform over the wave
      const Frame f = wave_frame(tq, n, lane);
      if (lane == 0) s.Gb[k] = f.G;
      for (int a = lane; a < n; a += 64)
        s.q[0][k * n + a] = (double)tq[3 * a] - f.cx, s.q[1][k * n + a] = (double)tq[3 * a + 1] - f.cy, s.q[2][k * n + a] = (double)tq[3 * a + 2] - f.cz;
    }
  __syncthreads();
  for (int k = wave; k < np; k += 4) {
    const float* tq = pair_target_pos(A, p0 + k, n);
    double msd = 0.0, mirror = 0.0;
    if (tq && n > 0) pair_eval(s, s.crank, n, lane, staged, k, tq, Ga, msd, mirror);
    if (lane == 0) A.o.msd[p0 + k] = msd, A.o.msd_mirror[p0 + k] = mirror, A.o.msd_first[p0 + k] = msd;
  }

  int nodes = 1, n_aut = 0;  // uniform
  const int status = canon_walk(s.g, n, A.max_nodes, nodes, [&]() {
    // ---- is the leaf optimal: every bond word stands in the canonical certificate
    bool miss = false;
    for (int e = tid; e < nb; e += 256) {
      const unsigned bd = s.g.bond[e];
      if (bd && find_word(s.cw, nbv, bond_word(bd, s.g.col)) < 0) miss = true;
    }
    if (__syncthreads_or(miss)) return;
    ++n_aut;
    if (n == 0) return;
    // ---- its atom map a -> col[a], pair by pair; the walk's next barrier comes before col changes
    for (int k = wave; k < np; k += 4) {
      const float* tq = pair_target_pos(A, p0 + k, n);
      if (!tq) continue;  // uniform over the wave
      double msd, mirror;
      pair_eval(s, s.g.col, n, lane, staged, k, tq, Ga, msd, mirror);
      if (lane == 0) {
        if (msd < A.o.msd[p0 + k]) A.o.msd[p0 + k] = msd;
        if (mirror < A.o.msd_mirror[p0 + k]) A.o.msd_mirror[p0 + k] = mirror;
      }
    }
  });
  __syncthreads();
  if (status != 0 || n_aut == 0) {  // uniform; no optimal leaf: the rank given is not canon's for these arrays
    write_unmeasured(A, m, status != 0 ? status : 1, p0, np);
    return;
  }
  for (long long pr = p0 + tid; pr < p0 + np; pr += 256) {
    const bool ok = pair_target_pos(A, pr, n) != nullptr;
    A.o.pair_stats[2 * pr] = ok ? n_aut : 0, A.o.pair_stats[2 * pr + 1] = ok ? 0 : 3;
  }
  if (tid < BR_STATS) A.o.mol_stats[(size_t)m * BR_STATS + tid] = tid == R_STATUS ? 0 : tid == R_NODES ? nodes : n_aut;
}

}  // namespace

extern "C" int mdx_mol_bestrms(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                               const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                               const int32_t* select, const float* atom_pos, const int32_t* atom_label, const int32_t* rank,
                               const int32_t* canon_status, const int32_t* pair_ptr, const int32_t* pair_target, int64_t P_cap, int32_t T,
                               const int32_t* tgt_ptr, const int32_t* tgt_n, const float* tgt_pos, int64_t tgt_atoms, int32_t max_nodes,
                               double* msd, double* msd_mirror, double* msd_first, int32_t* pair_stats, int32_t* mol_stats, void* stream) {
  BrArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  a.o = BestrmsOperands{atom_pos, atom_label, rank, canon_status, pair_ptr, pair_target, tgt_ptr, tgt_n, tgt_pos, msd, msd_mirror, msd_first, pair_stats, mol_stats};
  if (const char* why = bestrms_check(a.o, P_cap, T, tgt_atoms, max_nodes)) return mdx_set_error(MDX_ERR_ARG, why);
  a.P_cap = P_cap, a.tgt_atoms = tgt_atoms, a.T = T, a.max_nodes = max_nodes;
  return mol_launch(mol_bestrms_kernel, "mol_bestrms_kernel", B, stream, a);
}
