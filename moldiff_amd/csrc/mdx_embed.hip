// Coordinates from distance bounds on the device (mdx_mol_embed): for every (molecule, conformer) random 4D coordinates are minimised
// against the smoothed bounds of mdx_mol_bounds by L-BFGS in two stages, the fourth coordinate is dropped, and the conformer is accepted
// when no 1-2, 1-3 or van der Waals bound is violated by more than viol_tol; otherwise the next attempt draws new coordinates.  Distance
// geometry with random starting coordinates: THIS PROJECT'S OWN MODEL, not ETKDG and unverified against RDKit.  include/moldiff_hip.h
// states it, moldiff_amd/embed.py (embed_ref) restates it operation by operation, and this file is built with -ffp-contract=off so that
// the float64 arithmetic is the restatement's.
//
// One workgroup of 256 threads per (molecule, conformer); thread a owns atom a.  The point and the trial point are four arrays of 256
// doubles each in LDS; the bounds stay in global memory (L2-resident), thread a reading entry [b][a] of the symmetric matrices, so that
// the 64 lanes of a wave read 64 consecutive words.  DETERMINISM: no floating-point atomic; thread a gathers its own gradient over
// b = 0 .. n_all - 1, the error of a pair is added by its lower atom, and every sum over threads is wave_sum, then the four wave totals
// in order.  The minimiser is mdx_lbfgs.h's, over four coordinates; its history lives in the caller's workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_allatom.h"
#include "mdx_embed_args.h"
#include "mdx_lbfgs.h"
#include "mdx_philox.h"

namespace {

enum { E_STATUS, E_ATTEMPTS, E_ITERS_A, E_ITERS_B, E_EVALS };
static_assert(E_EVALS + 1 == EM_STATS && EM_STATS == MDX_EMBED_STATS && EM_VALUES == MDX_EMBED_VALUES, "the columns of the tables");

struct EmArgs {
  MolArrays mol;
  EmbedParams p;
  EmbedOperands o;
};

using Pos4 = double[4][MOL_ATOMS];

struct EmShared {
  Pos4 x, xt;
  LbfgsShared lb;
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS], wave_total[4];
};

// The error at X and the gradient on this thread's atom.  L, U: this thread's column of the bounds (entry b at b * cap).
__device__ inline double evaluate(EmShared& s, const Pos4& X, const double* L, const double* U, int cap, int n_all, double w4, D4& g) {
  const int a = threadIdx.x;
  double e = 0.0;
  g = {};
  if (a < n_all) {
    const D4 pa = at(X, a);
    for (int b = 0; b < n_all; ++b) {
      const double lb = L[(size_t)b * cap], ub = U[(size_t)b * cap];
      const D4 d = sub(pa, at(X, b));
      const double d2 = dot(d, d), ub2 = ub * ub, lb2 = lb * lb;
      double en, pre;
      if (d2 > ub2) {
        const double v = d2 / ub2 - 1.0;
        en = v * v, pre = (4.0 * v) / ub2;
      } else if (d2 < lb2) {
        const double q = lb2 + d2;
        const double v = (2.0 * lb2) / q - 1.0;
        en = v * v, pre = -(((8.0 * lb2) * v) / (q * q));
      } else {
        continue;
      }
      g = each<4>([&](int k) { return g[k] + pre * d[k]; });
      if (a < b) e = e + en;
    }
    e = e + w4 * (pa[3] * pa[3]);
    g[3] = g[3] + (2.0 * w4) * pa[3];
  }
  return block_sum(s.lb, e);
}

__device__ inline void write_unmeasured(const EmArgs& A, int m, int c, int status, const MolView& v) {
  const int tid = threadIdx.x;
  const size_t row = (size_t)m * A.p.n_confs + c;
  if (tid < EM_STATS) A.o.conf_stats[row * EM_STATS + tid] = tid == E_STATUS ? status : 0;
  if (tid < EM_VALUES) A.o.conf_values[row * EM_VALUES + tid] = 0.0;
  if (v.outside) return;
  const size_t base = (size_t)c * (size_t)A.mol.N_cap;
  for (long long a = v.n0 + tid; a < v.n0 + v.n; a += 256) {
    for (int q = 0; q < 3; ++q) A.o.pos_out[3 * (base + a) + q] = 0.0;
    for (int q = 0; q < 3 * RX_MAX_H; ++q) A.o.h_pos_out[3 * RX_MAX_H * (base + a) + q] = 0.0;
  }
}

__global__ __launch_bounds__(256) void mol_embed_kernel(const EmArgs A) {
  __shared__ EmShared s;
  const int K = A.p.n_confs;
  const int m = blockIdx.x / K, c = blockIdx.x % K, tid = threadIdx.x;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0;
  const int n = v.n;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, c, unmeasured, v);
    return;
  }
  const AllAtomCount aa = allatom_count(A.o.h_count + n0, n, s.off, s.cur, s.wave_total);
  const int n_all = aa.n_all, cap = A.p.na_cap;
  const int bstatus = A.o.bounds_stats[(size_t)m * EB_STATS];
  if (n_all > cap || bstatus != EM_OK) {  // uniform; n_all <= cap <= 256 past this line
    write_unmeasured(A, m, c, n_all > cap || bstatus == EM_TOO_LARGE ? EM_TOO_LARGE : bstatus == EM_INCONSISTENT ? EM_INCONSISTENT : EM_NONFINITE, v);
    return;
  }
  const bool live = tid < n_all;
  const size_t plane = (size_t)cap * (size_t)cap;
  const int col = live ? tid : 0;  // a thread past the molecule reads nothing through these
  const double* L = A.o.bounds + (size_t)m * 2u * plane + col;
  const double* U = L + plane;
  const unsigned char* C = A.o.cls + (size_t)m * plane + col;

  double top = 0.0;
  if (live)
    for (int b = 0; b < n_all; ++b)
      if (C[(size_t)b * cap] != EB_OTHER) top = fmax(top, U[(size_t)b * cap]);
  const double box = EM_BOX * block_max(s.lb, top);

  const size_t row = (size_t)m * K + c;
  double* hist = A.o.hist + row * (size_t)EM_HIST_PER_ATOM * cap + col;  // vector q (slot, s or y), coordinate k of this atom: hist[(4 q + k) * cap]
  auto hget = [&](int q, int which) {
    const double* p = hist + (size_t)(4 * (2 * q + which)) * cap;
    return each<4>([&](int k) { return p[(size_t)k * cap]; });
  };
  auto hput = [&](int q, int which, D4 u) {
    double* p = hist + (size_t)(4 * (2 * q + which)) * cap;
#pragma unroll
    for (int k = 0; k < 4; ++k) p[(size_t)k * cap] = u[k];
  };
  const long long id = A.o.mol_ids ? A.o.mol_ids[m] : (long long)m;
  const uint32_t k0 = (uint32_t)A.p.seed, k1 = (uint32_t)(A.p.seed >> 32);
  const double gtol = A.p.gtol, max_step = A.p.max_step;
  const int max_iters = A.p.max_iters;

  int status = EM_FAILED, attempts = 0, evals = 0, iters_ab[2] = {0, 0};
  double err_ab[2] = {0.0, 0.0}, viol = 0.0;
  for (int attempt = 0; attempt < A.p.max_attempts; ++attempt) {
    ++attempts;
    D4 x0 = {};
    if (live) {
      const uint32_t hi = (uint32_t)((unsigned long long)id >> 32) << 8 | (uint32_t)attempt;
      const u4 ra = philox4x32_10(u4{2u * (uint32_t)tid, (uint32_t)c, (uint32_t)id, hi}, k0, k1);
      const u4 rb = philox4x32_10(u4{2u * (uint32_t)tid + 1u, (uint32_t)c, (uint32_t)id, hi}, k0, k1);
      x0 = {{(embed_u53(ra.x, ra.y) - 0.5) * box, (embed_u53(ra.z, ra.w) - 0.5) * box, (embed_u53(rb.x, rb.y) - 0.5) * box,
             (embed_u53(rb.z, rb.w) - 0.5) * box}};
    }
    __syncthreads();  // nobody still reads the point of the attempt before
    put(s.x, tid, x0);
    __syncthreads();
    bool finite = true;
    for (int stage = 0; stage < 2 && finite; ++stage) {
      const double w4 = stage == 0 ? EM_W4_A : EM_W4_B;
      D4 g;
      const double E = evaluate(s, s.x, L, U, cap, n_all, w4, g);
      const double gg = block_sum(s.lb, dot(g, g));
      if (!isfinite(E) || !isfinite(gg)) {  // uniform
        finite = false;
        break;
      }
      const Lbfgs<4> r = lbfgs_minimise(
          s.lb, s.x, s.xt, n_all, gtol, max_step, max_iters, E, g, gg, [&](const Pos4& P, D4& gp) { return evaluate(s, P, L, U, cap, n_all, w4, gp); }, [] {},
          hget, hput);
      evals += 1 + r.evals, iters_ab[stage] = r.iters, err_ab[stage] = r.E;
    }
    if (!finite) {  // uniform
      write_unmeasured(A, m, c, EM_NONFINITE, v);
      return;
    }
    // ---- the largest violation in three dimensions
    double worst = 0.0;
    if (live) {
      const D4 pa = at(s.x, tid);
      for (int b = 0; b < n_all; ++b) {
        const int cls = C[(size_t)b * cap];
        if (b == tid || cls == EB_14) continue;
        const double lb = L[(size_t)b * cap], ub = U[(size_t)b * cap];
        const D4 pb = at(s.x, b);
        const double dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
        const double d = sqrt((dx * dx + dy * dy) + dz * dz);
        if (d < lb) worst = fmax(worst, (lb - d) / lb);
        else if (cls != EB_OTHER && d > ub) worst = fmax(worst, (d - ub) / ub);
      }
    }
    viol = block_max(s.lb, worst);
    if (viol <= A.p.viol_tol) {
      status = EM_OK;
      break;
    }
  }

  // ---- the outputs
  const size_t base = (size_t)c * (size_t)A.mol.N_cap;
  if (tid < n) allatom_write(s.x, n, aa, A.o.pos_out + 3 * (base + n0 + tid), A.o.h_pos_out + 3 * RX_MAX_H * (base + n0 + tid));
  if (tid == 0) {
    int* st = A.o.conf_stats + row * EM_STATS;
    st[E_STATUS] = status, st[E_ATTEMPTS] = attempts, st[E_ITERS_A] = iters_ab[0], st[E_ITERS_B] = iters_ab[1], st[E_EVALS] = evals;
    double* va = A.o.conf_values + row * EM_VALUES;
    va[0] = err_ab[0], va[1] = err_ab[1], va[2] = viol;
  }
}

}  // namespace

extern "C" int mdx_mol_embed(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                             const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                             const int32_t* select, const int32_t* h_count, const int64_t* mol_ids, const void* bounds_ws, size_t ws_bytes,
                             int32_t na_cap, const int32_t* bounds_stats, int32_t n_confs, uint64_t seed, int32_t max_iters, int32_t max_attempts,
                             double gtol, double max_step, double viol_tol, double* pos_out, double* h_pos_out, int32_t* conf_stats,
                             double* conf_values, double* hist, size_t hist_bytes, void* stream) {
  EmArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  if (!h_count || !bounds_stats || !pos_out || !h_pos_out || !conf_stats || !conf_values || !hist) return mdx_set_error(MDX_ERR_ARG, "null argument");
  if (const char* why = bounds_ws_check(B, na_cap, bounds_ws, ws_bytes)) return mdx_set_error(MDX_ERR_ARG, why);
  if (const char* why = embed_prepare(&a.p, B, na_cap, n_confs, seed, max_iters, max_attempts, gtol, max_step, viol_tol, hist_bytes))
    return mdx_set_error(MDX_ERR_ARG, why);
  if ((int64_t)B * n_confs > 0x7fffffffLL) return mdx_set_error(MDX_ERR_ARG, "B x n_confs must stay below 2^31");
  a.o = EmbedOperands{h_count, mol_ids, (const double*)bounds_ws, (const unsigned char*)bounds_ws + (size_t)B * 16u * (size_t)na_cap * (size_t)na_cap,
                      bounds_stats, pos_out, h_pos_out, conf_stats, conf_values, hist};
  return mol_launch(mol_embed_kernel, "mol_embed_kernel", B * n_confs, stream, a);
}
