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
// in order.  The minimiser is a second copy of mdx_relax.hip's, over four coordinates; its history lives in the caller's workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_mol.h"
#include "mdx_embed_args.h"
#include "mdx_philox.h"

namespace {

constexpr double EM_ARMIJO = 1e-4, EM_CURVATURE = 1e-10;
constexpr int EM_TRIALS = 20;
enum { E_STATUS, E_ATTEMPTS, E_ITERS_A, E_ITERS_B, E_EVALS };
static_assert(E_EVALS + 1 == EM_STATS && EM_STATS == MDX_EMBED_STATS && EM_VALUES == MDX_EMBED_VALUES, "the columns of the tables");

struct EmArgs {
  MolArrays mol;
  EmbedParams p;
  EmbedOperands o;
};

struct D4 {
  double x, y, z, w;
};

struct EmShared {
  double x[4][MOL_ATOMS], xt[4][MOL_ATOMS];
  double red[4];
  double hsy[RX_HISTORY], hyy[RX_HISTORY], alpha[RX_HISTORY];
  int off[MOL_ATOMS + 1], cur[MOL_ATOMS], wave_total[4];
};

__device__ inline D4 sub(D4 a, D4 b) { return {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w}; }
__device__ inline double dot(D4 a, D4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }
__device__ inline D4 scaled(double f, D4 a) { return {f * a.x, f * a.y, f * a.z, f * a.w}; }
__device__ inline D4 at(const double (*X)[MOL_ATOMS], int a) { return {X[0][a], X[1][a], X[2][a], X[3][a]}; }
__device__ inline void put(double (*X)[MOL_ATOMS], int a, D4 v) { X[0][a] = v.x, X[1][a] = v.y, X[2][a] = v.z, X[3][a] = v.w; }

__device__ inline double block_sum(EmShared& s, double v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double w = wave_sum(v);
  if (lane == 0) s.red[wave] = w;
  __syncthreads();
  const double r = ((s.red[0] + s.red[1]) + s.red[2]) + s.red[3];
  __syncthreads();
  return r;
}

__device__ inline double block_max(EmShared& s, double v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if (lane == 0) s.red[wave] = v;
  __syncthreads();
  const double r = fmax(fmax(s.red[0], s.red[1]), fmax(s.red[2], s.red[3]));
  __syncthreads();
  return r;
}

// The error at X and the gradient on this thread's atom.  L, U: this thread's column of the bounds (entry b at b * cap).
__device__ inline double evaluate(EmShared& s, const double (*X)[MOL_ATOMS], const double* L, const double* U, int cap, int n_all, double w4, D4& g) {
  const int a = threadIdx.x;
  double e = 0.0;
  g = {0.0, 0.0, 0.0, 0.0};
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
      g = {g.x + pre * d.x, g.y + pre * d.y, g.z + pre * d.z, g.w + pre * d.w};
      if (a < b) e = e + en;
    }
    e = e + w4 * (pa.w * pa.w);
    g.w = g.w + (2.0 * w4) * pa.w;
  }
  return block_sum(s, e);
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
  const bool in = tid < n;
  const int h = in ? min(max(A.o.h_count[n0 + tid], 0), RX_MAX_H) : 0;
  s.cur[tid] = h;
  __syncthreads();
  block_exclusive_scan_256(s.off, s.cur, s.wave_total);
  __syncthreads();
  const int hoff = s.off[tid], n_all = n + s.off[MOL_ATOMS];
  __syncthreads();
  const int cap = A.p.na_cap;
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
  const double box = EM_BOX * block_max(s, top);

  const size_t row = (size_t)m * K + c;
  double* hist = A.o.hist + row * (size_t)EM_HIST_PER_ATOM * cap + col;  // vector q (slot, s or y), coordinate k of this atom: hist[(4 q + k) * cap]
  auto hget = [&](int q, int which) {
    const double* p = hist + (size_t)(4 * (2 * q + which)) * cap;
    return D4{p[0], p[cap], p[2 * (size_t)cap], p[3 * (size_t)cap]};
  };
  auto hput = [&](int q, int which, D4 u) {
    double* p = hist + (size_t)(4 * (2 * q + which)) * cap;
    p[0] = u.x, p[cap] = u.y, p[2 * (size_t)cap] = u.z, p[3 * (size_t)cap] = u.w;
  };
  const long long id = A.o.mol_ids ? A.o.mol_ids[m] : (long long)m;
  const uint32_t k0 = (uint32_t)A.p.seed, k1 = (uint32_t)(A.p.seed >> 32);
  const double gtol = A.p.gtol, max_step = A.p.max_step;
  const int max_iters = A.p.max_iters;

  int status = EM_FAILED, attempts = 0, evals = 0, iters_ab[2] = {0, 0};
  double err_ab[2] = {0.0, 0.0}, viol = 0.0;
  for (int attempt = 0; attempt < A.p.max_attempts; ++attempt) {
    ++attempts;
    D4 x0 = {0.0, 0.0, 0.0, 0.0};
    if (live) {
      const uint32_t hi = (uint32_t)((unsigned long long)id >> 32) << 8 | (uint32_t)attempt;
      const u4 ra = philox4x32_10(u4{2u * (uint32_t)tid, (uint32_t)c, (uint32_t)id, hi}, k0, k1);
      const u4 rb = philox4x32_10(u4{2u * (uint32_t)tid + 1u, (uint32_t)c, (uint32_t)id, hi}, k0, k1);
      x0 = {(embed_u53(ra.x, ra.y) - 0.5) * box, (embed_u53(ra.z, ra.w) - 0.5) * box, (embed_u53(rb.x, rb.y) - 0.5) * box,
            (embed_u53(rb.z, rb.w) - 0.5) * box};
    }
    __syncthreads();  // nobody still reads the point of the attempt before
    put(s.x, tid, x0);
    __syncthreads();
    bool finite = true;
    for (int stage = 0; stage < 2 && finite; ++stage) {
      const double w4 = stage == 0 ? EM_W4_A : EM_W4_B;
      D4 g;
      double E = evaluate(s, s.x, L, U, cap, n_all, w4, g);
      ++evals;
      double gg = block_sum(s, dot(g, g));
      if (!isfinite(E) || !isfinite(gg)) {  // uniform
        finite = false;
        break;
      }
      int hc = 0, head = 0, iters = 0;
      for (;;) {
        const double rms = n_all ? sqrt(gg / (4.0 * (double)n_all)) : 0.0;
        if (rms <= gtol) break;
        if (iters >= max_iters) break;
        D4 d = {-g.x, -g.y, -g.z, -g.w};
        if (hc > 0) {  // the two-loop recursion
          D4 q = g;
          for (int t = hc - 1; t >= 0; --t) {
            const int slot = (head + t) & (RX_HISTORY - 1);
            const D4 sv = live ? hget(slot, 0) : D4{0.0, 0.0, 0.0, 0.0}, yv = live ? hget(slot, 1) : D4{0.0, 0.0, 0.0, 0.0};
            const double al = block_sum(s, live ? dot(sv, q) : 0.0) / s.hsy[slot];
            s.alpha[slot] = al;  // every thread stores the same value and reads its own store
            q = {q.x - al * yv.x, q.y - al * yv.y, q.z - al * yv.z, q.w - al * yv.w};
          }
          const int newest = (head + hc - 1) & (RX_HISTORY - 1);
          const double gamma = s.hsy[newest] / s.hyy[newest];
          D4 r = scaled(gamma, q);
          for (int t = 0; t < hc; ++t) {
            const int slot = (head + t) & (RX_HISTORY - 1);
            const D4 sv = live ? hget(slot, 0) : D4{0.0, 0.0, 0.0, 0.0}, yv = live ? hget(slot, 1) : D4{0.0, 0.0, 0.0, 0.0};
            const double co = s.alpha[slot] - block_sum(s, live ? dot(yv, r) : 0.0) / s.hsy[slot];
            r = {r.x + co * sv.x, r.y + co * sv.y, r.z + co * sv.z, r.w + co * sv.w};
          }
          const D4 dl = {-r.x, -r.y, -r.z, -r.w};
          const double gd = block_sum(s, live ? dot(g, dl) : 0.0);
          if (gd < 0.0) d = dl;
          else hc = 0;
        }
        bool accepted = false;
        D4 gt = g, xo = at(s.x, tid), xn = xo;
        double Et = E;
        for (;;) {
          const double big = sqrt(block_max(s, live ? dot(d, d) : 0.0));
          if (big > max_step) d = scaled(max_step / big, d);
          const double gd = block_sum(s, live ? dot(g, d) : 0.0);
          double t = 1.0;
          for (int trial = 0; trial < EM_TRIALS; ++trial) {
            xn = {xo.x + t * d.x, xo.y + t * d.y, xo.z + t * d.z, xo.w + t * d.w};
            put(s.xt, tid, xn);
            __syncthreads();
            Et = evaluate(s, s.xt, L, U, cap, n_all, w4, gt);
            ++evals;
            if (isfinite(Et) && Et <= E + (EM_ARMIJO * t) * gd) {
              accepted = true;
              break;
            }
            t = t * 0.5;
          }
          if (accepted || hc == 0) break;
          hc = 0;
          d = {-g.x, -g.y, -g.z, -g.w};
        }
        if (!accepted) break;
        const D4 sv = sub(xn, xo), yv = sub(gt, g);
        const double sy = block_sum(s, live ? dot(sv, yv) : 0.0), ss = block_sum(s, live ? dot(sv, sv) : 0.0), yy = block_sum(s, live ? dot(yv, yv) : 0.0);
        if (sy > EM_CURVATURE * sqrt(ss * yy)) {
          int slot;
          if (hc == RX_HISTORY) slot = head, head = (head + 1) & (RX_HISTORY - 1);
          else slot = (head + hc) & (RX_HISTORY - 1), ++hc;
          if (live) hput(slot, 0, sv), hput(slot, 1, yv);
          s.hsy[slot] = sy, s.hyy[slot] = yy;
        }
        put(s.x, tid, xn);  // nobody reads x before the barriers of the next sum
        g = gt, E = Et;
        ++iters;
        gg = block_sum(s, dot(g, g));
      }
      iters_ab[stage] = iters, err_ab[stage] = E;
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
        const double dx = pa.x - pb.x, dy = pa.y - pb.y, dz = pa.z - pb.z;
        const double d = sqrt((dx * dx + dy * dy) + dz * dz);
        if (d < lb) worst = fmax(worst, (lb - d) / lb);
        else if (cls != EB_OTHER && d > ub) worst = fmax(worst, (d - ub) / ub);
      }
    }
    viol = block_max(s, worst);
    if (viol <= A.p.viol_tol) {
      status = EM_OK;
      break;
    }
  }

  // ---- the outputs
  const size_t base = (size_t)c * (size_t)A.mol.N_cap;
  if (in) {
    const D4 px = at(s.x, tid);
    double* po = A.o.pos_out + 3 * (base + n0 + tid);
    po[0] = px.x, po[1] = px.y, po[2] = px.z;
    double* ho = A.o.h_pos_out + 3 * RX_MAX_H * (base + n0 + tid);
    for (int k = 0; k < RX_MAX_H; ++k) {
      const bool there = k < h;
      const D4 qx = at(s.x, there ? n + hoff + k : 0);
      ho[3 * k] = there ? qx.x : 0.0, ho[3 * k + 1] = there ? qx.y : 0.0, ho[3 * k + 2] = there ? qx.z : 0.0;
    }
  }
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
