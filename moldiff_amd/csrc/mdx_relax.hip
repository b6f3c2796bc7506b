// Force-field relaxation of all-atom molecules on the device (mdx_mol_relax): every decoded molecule with the hydrogens that
// mdx_mol_hydrogens placed is relaxed by L-BFGS in a UFF-form force field, and the energy before and after, the final gradient and the
// displacement of the heavy atoms are reported.  It is THIS PROJECT'S OWN MODEL over a small, UNVERIFIED parameter table: not RDKit's
// UFFOptimizeMolecule and unverified against it.  The energy, the minimiser and every order of accumulation are stated in
// include/moldiff_hip.h, moldiff_amd/relax.py restates them (energy_ref, relax_ref) operation by operation, and this file is built with
// -ffp-contract=off so that the float64 arithmetic is the restatement's.
//
// One workgroup of 256 threads (4 waves) per molecule over the compact arrays of mdx_mol.h; thread a owns atom a of the all-atom
// molecule (heavy atoms, then the hydrogens in (atom, k) order; at most 256 in all).  Staged once in LDS: the molecule of
// mdx_allatom.h (rows sorted by neighbour, the derived parameter rows, rest length and force constant per bond), and the 1-2 / 1-3
// exclusions as a 256-bit mask per atom, word-major so that the 64 lanes of a wave read 64 consecutive words.  Positions and the trial
// point are kept as three arrays of 256 doubles each (a lane's own entry: consecutive 8-byte words, no bank conflict; a neighbour's
// entry: a gather).  The minimiser is mdx_lbfgs.h's; this file holds the terms, their evaluation and the outputs.
//
// DETERMINISM.  There is no floating-point atomic and no scatter: thread a GATHERS the gradient on atom a by walking every term atom a
// takes part in, in the order the header states, so a term is evaluated by each of its atoms; the energy of a term is added by one
// owner (the lower atom of a bond or a pair, the centre of an angle or inversion, the lower central atom of a torsion).  Every sum over
// the threads is a per-thread partial, wave_sum (xor butterfly 32 .. 1), then the four wave totals in order.  The 2 x 8 history vectors
// live in the caller's workspace, each thread touching only its own atom's entries.  About 53 KB of static LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/moldiff_hip.h"
#include "mdx_allatom.h"
#include "mdx_lbfgs.h"

namespace {

// the columns of mol_stats and mol_energy: MDX_RELAX_* of include/moldiff_hip.h
enum { R_STATUS, R_REASON, R_ITERS, R_EVALS, R_NALL, R_BONDS, R_ANGLES, R_TORSIONS, R_INVERSIONS, R_PAIRS, R_FALLBACK };
static_assert(R_FALLBACK + 1 == RX_STATS && RX_STATS == MDX_RELAX_STATS && RX_ENERGIES == MDX_RELAX_ENERGIES, "the columns of the tables");
enum { STATUS_OK = 0, STATUS_TOO_LARGE = 1, STATUS_NONFINITE = 2 };
enum { ANGLE_LINEAR = 0, ANGLE_TRIGONAL = 1, ANGLE_GENERAL = 2 };
enum { TORSION_TT = 0, TORSION_PP = 1, TORSION_MIXED = 2 };

struct RxArgs {
  MolArrays mol;
  RelaxTable tab;
  RelaxOperands o;
};

using Pos3 = double[3][MOL_ATOMS];

struct RxShared : AllAtomShared {
  Pos3 x, xt;                   // the point and the trial point
  Pos3 g;                       // the final gradient: the parent writes out its hydrogens' (gradient, direction and the vectors of
                                // the recursion are a thread's own atom's and stay in its registers)
  double bk[AA_BONDS];          // force constant per bond
  double red[5][4];             // the wave totals of the five components
  LbfgsShared lb;
  unsigned mask[8][MOL_ATOMS];  // bit b of word [b >> 5][a]: the pair (a, b) is excluded
  int ired[4][8];
};

__device__ inline D3 add(D3 a, D3 b) {
  return each<3>([&](int k) { return a[k] + b[k]; });
}
__device__ inline D3 cross(D3 a, D3 b) { return {{a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}}; }

// ---- the terms: the same operations in the same order as moldiff_amd/relax.py

__device__ inline void bond_term(D3 pa, D3 pb, double r0, double k, double& e, D3& ga) {
  const D3 d = sub(pa, pb);
  const double r = sqrt(dot(d, d)), dr = r - r0, f = (k * dr) / r;
  e = (0.5 * k) * (dr * dr);
  ga = scaled(f, d);
}

__device__ inline double angle_k(double zi, double zk, double rij, double rjk, double c0) {
  const double rik2 = (rij * rij + rjk * rjk) - ((2.0 * rij) * rjk) * c0;
  const double rik = sqrt(rik2);
  return (((664.12 * zi) * zk) / ((rik2 * rik2) * rik)) * (((3.0 * rij) * rjk) * (1.0 - c0 * c0) - rik2 * c0);
}

__device__ inline void angle_term(D3 pi, D3 pj, D3 pk, double K, int kind, double c0, double& e, D3& gi, D3& gk) {
  const D3 u = sub(pi, pj), v = sub(pk, pj);
  const double uu = dot(u, u), vv = dot(v, v);
  const double luv = sqrt(uu) * sqrt(vv);
  const double c = dot(u, v) / luv;
  double de;
  if (kind == ANGLE_LINEAR) {
    e = K * (1.0 + c), de = K;
  } else if (kind == ANGLE_TRIGONAL) {
    const double k9 = K / 9.0, c2 = c * c;
    e = k9 * (1.0 - ((4.0 * c2) * c - 3.0 * c)), de = -(k9 * (12.0 * c2 - 3.0));
  } else {
    const double c2 = 1.0 / (4.0 * (1.0 - c0 * c0));
    const double c1 = (-4.0 * c2) * c0;
    e = K * ((c2 * ((2.0 * c0) * c0 + 1.0) + c1 * c) + c2 * ((2.0 * c) * c - 1.0)), de = K * (c1 + (4.0 * c2) * c);
  }
  const double fu = c / uu, fv = c / vv;
  gi = each<3>([&](int x) { return de * (v[x] / luv - fu * u[x]); });
  gk = each<3>([&](int x) { return de * (u[x] / luv - fv * v[x]); });
}

// -> false for a collinear triple; g0, g1: the gradients on p0 and p1
__device__ inline bool torsion_term(D3 p0, D3 p1, D3 p2, D3 p3, int kind, double vq, double deg_tol, double& e, D3& g0, D3& g1) {
  const D3 F = sub(p0, p1), G = sub(p1, p2), H = sub(p3, p2);
  const D3 A = cross(F, G), B = cross(H, G);
  const double aa = dot(A, A), bb = dot(B, B);
  const double la = sqrt(aa), lb = sqrt(bb);
  if (!(la >= deg_tol) || !(lb >= deg_tol)) return false;
  const double lab = la * lb;
  const double c = dot(A, B) / lab;
  const double c2 = c * c, hv = 0.5 * vq;
  double de;
  if (kind == TORSION_TT) {
    e = hv * (1.0 + ((4.0 * c2) * c - 3.0 * c)), de = hv * (12.0 * c2 - 3.0);
  } else if (kind == TORSION_PP) {
    e = hv * (1.0 - (2.0 * c2 - 1.0)), de = hv * (-4.0 * c);
  } else {
    const double c4 = c2 * c2;
    e = hv * (1.0 - ((((32.0 * c4) * c2 - 48.0 * c4) + 18.0 * c2) - 1.0)), de = -(hv * (((192.0 * c4) * c - (192.0 * c2) * c) + 36.0 * c));
  }
  const double fa = c / aa, fb = c / bb;
  const D3 tA = each<3>([&](int x) { return B[x] / lab - fa * A[x]; });
  const D3 tB = each<3>([&](int x) { return A[x] / lab - fb * B[x]; });
  const D3 GA = cross(G, tA), AF = cross(tA, F), BH = cross(tB, H);
  g0 = scaled(de, GA);
  g1 = each<3>([&](int x) { return de * ((AF[x] - GA[x]) + BH[x]); });
  return true;
}

// -> false for a collinear plane or an apex on the centre; gradients on i, k and the apex l
__device__ inline bool inversion_term(D3 pj, D3 pi, D3 pk, D3 pl, double k3, double deg_tol, double& e, D3& gi, D3& gk, D3& gl) {
  const D3 u = sub(pi, pj), v = sub(pk, pj), w = sub(pl, pj);
  const D3 n = cross(u, v);
  const double nn = dot(n, n), ww = dot(w, w);
  const double ln = sqrt(nn), lw = sqrt(ww);
  if (!(ln >= deg_tol) || !(lw > 0.0)) return false;
  const double lnw = ln * lw;
  const double y = dot(n, w) / lnw;
  const double sq = sqrt(1.0 - y * y);
  e = k3 * (1.0 - sq);
  const double de = (k3 * y) / sq;
  const double fn = y / nn, fw = y / ww;
  const D3 tn = each<3>([&](int x) { return w[x] / lnw - fn * n[x]; });
  const D3 tw = each<3>([&](int x) { return n[x] / lnw - fw * w[x]; });
  gi = scaled(de, cross(v, tn)), gk = scaled(de, cross(tn, u)), gl = scaled(de, tw);
  return true;
}

__device__ inline void vdw_term(D3 pa, D3 pb, double x2, double dij, double& e, D3& ga) {
  const D3 d = sub(pa, pb);
  const double r2 = dot(d, d);
  const double q2 = x2 / r2;
  const double q6 = (q2 * q2) * q2;
  const double q12 = q6 * q6;
  const double f = ((12.0 * dij) * (q6 - q12)) / r2;
  e = dij * (q12 - 2.0 * q6);
  ga = scaled(f, d);
}

// ---- the staged molecule

__device__ inline bool planar(int var) { return var == RX_TRIGONAL || var == RX_RESONANT; }

__device__ inline void angle_at(const RxShared& s, const Pos3& X, int i, int j, int k, int ei, int ek, double& e, D3& gi, D3& gk) {
  const double* pj = s.par[s.typ[j]];
  const double c0 = pj[RX_C0];
  const double K = angle_k(s.par[s.typ[i]][RX_Z], s.par[s.typ[k]][RX_Z], s.br0[ei], s.br0[ek], c0);
  const int var = s.var[j];
  const int kind = var == RX_LINEAR || c0 == -1.0 ? ANGLE_LINEAR : planar(var) ? ANGLE_TRIGONAL : ANGLE_GENERAL;
  angle_term(at(X, i), at(X, j), at(X, k), K, kind, c0, e, gi, gk);
}

// whether the bond e between j and k carries torsions -> their kind and V per quadruple
__device__ inline bool torsion_bond(const RxShared& s, int j, int k, int e, int& kind, double& vq) {
  const int dj = s.off[j + 1] - s.off[j], dk = s.off[k + 1] - s.off[k];
  const int vj = s.var[j], vk = s.var[k];
  if (dj < 2 || dk < 2 || vj == RX_LINEAR || vk == RX_LINEAR) return false;
  const double nq = (double)((dj - 1) * (dk - 1));
  const double *pj = s.par[s.typ[j]], *pk = s.par[s.typ[k]];
  const bool fj = planar(vj), fk = planar(vk);
  if (!fj && !fk) {
    kind = TORSION_TT, vq = sqrt(pj[RX_V] * pk[RX_V]) / nq;
  } else if (fj && fk) {
    kind = TORSION_PP, vq = ((5.0 * sqrt(pj[RX_U] * pk[RX_U])) * (1.0 + 4.18 * s.ln_order[mol_bond_payload(s.bond[e]) & 3u])) / nq;
  } else {
    kind = TORSION_MIXED, vq = 1.0 / nq;
  }
  return true;
}

__device__ inline bool inverts(const RxShared& s, int j) {
  return planar(s.var[j]) && s.off[j + 1] - s.off[j] == 3 && s.par[s.typ[j]][RX_KINV] > 0.0;
}

// apex choice t of the inversion centred at j: -> false when it is skipped; wi, wk, wl: the atoms i, k and the apex
__device__ inline bool inversion_at(const RxShared& s, const Pos3& X, int j, int t, double deg_tol, int& wi, int& wk, int& wl, double& e, D3& gi, D3& gk,
                                    D3& gl) {
  const int r0 = s.off[j];
  const int n0 = row_nbr(s.adj[r0]), n1 = row_nbr(s.adj[r0 + 1]), n2 = row_nbr(s.adj[r0 + 2]);
  wi = t == 0 ? n1 : n0, wk = t == 2 ? n1 : n2, wl = t == 0 ? n0 : t == 1 ? n1 : n2;
  return inversion_term(at(X, j), at(X, wi), at(X, wk), at(X, wl), s.par[s.typ[j]][RX_KINV] / 3.0, deg_tol, e, gi, gk, gl);
}

// The gradient on atom a and the energies this atom owns, at the point X.  e, cnt: bond, angle, torsion, inversion, van der Waals.
__device__ inline void eval_atom(const RxShared& s, const Pos3& X, int a, int n_all, double deg_tol, D3& gout, double* e, int* cnt) {
  D3 g = {};
#pragma unroll
  for (int c = 0; c < 5; ++c) e[c] = 0.0, cnt[c] = 0;
  const int r0 = s.off[a], r1 = s.off[a + 1];
  const D3 pa = at(X, a);
  double en;
  D3 ga, gb;
  for (int q = r0; q < r1; ++q) {  // bonds
    const int b = row_nbr(s.adj[q]), eb = row_bond(s.adj[q]);
    bond_term(pa, at(X, b), s.br0[eb], s.bk[eb], en, ga);
    g = add(g, ga);
    if (a < b) e[0] = e[0] + en, ++cnt[0];
  }
  for (int q1 = r0; q1 < r1; ++q1)  // angles centred here
    for (int q2 = q1 + 1; q2 < r1; ++q2) {
      angle_at(s, X, row_nbr(s.adj[q1]), a, row_nbr(s.adj[q2]), row_bond(s.adj[q1]), row_bond(s.adj[q2]), en, ga, gb);
      g = sub(g, add(ga, gb));
      e[1] = e[1] + en, ++cnt[1];
    }
  for (int q = r0; q < r1; ++q) {  // angles that end here
    const int j = row_nbr(s.adj[q]), ej = row_bond(s.adj[q]);
    for (int p = s.off[j]; p < s.off[j + 1]; ++p) {
      const int k = row_nbr(s.adj[p]);
      if (k == a) continue;
      angle_at(s, X, a, j, k, ej, row_bond(s.adj[p]), en, ga, gb);
      g = add(g, ga);
    }
  }
  for (int q = r0; q < r1; ++q) {  // torsions about a bond of this atom
    const int k = row_nbr(s.adj[q]);
    int kind;
    double vq;
    if (!torsion_bond(s, a, k, row_bond(s.adj[q]), kind, vq)) continue;
    const D3 pk = at(X, k);
    for (int qi = r0; qi < r1; ++qi) {
      const int i = row_nbr(s.adj[qi]);
      if (i == k) continue;
      const D3 pi = at(X, i);
      for (int p = s.off[k]; p < s.off[k + 1]; ++p) {
        const int l = row_nbr(s.adj[p]);
        if (l == a || l == i) continue;
        if (!torsion_term(pi, pa, pk, at(X, l), kind, vq, deg_tol, en, ga, gb)) continue;
        g = add(g, gb);
        if (a < k) e[2] = e[2] + en, ++cnt[2];
      }
    }
  }
  for (int q = r0; q < r1; ++q) {  // torsions that end here
    const int j = row_nbr(s.adj[q]);
    const D3 pj = at(X, j);
    for (int pk_ = s.off[j]; pk_ < s.off[j + 1]; ++pk_) {
      const int k = row_nbr(s.adj[pk_]);
      if (k == a) continue;
      int kind;
      double vq;
      if (!torsion_bond(s, j, k, row_bond(s.adj[pk_]), kind, vq)) continue;
      const D3 pk = at(X, k);
      for (int p = s.off[k]; p < s.off[k + 1]; ++p) {
        const int l = row_nbr(s.adj[p]);
        if (l == j || l == a) continue;
        if (!torsion_term(pa, pj, pk, at(X, l), kind, vq, deg_tol, en, ga, gb)) continue;
        g = add(g, ga);
      }
    }
  }
  int wi, wk, wl;
  D3 gc;
  if (inverts(s, a))  // inversions centred here
    for (int t = 0; t < 3; ++t) {
      if (!inversion_at(s, X, a, t, deg_tol, wi, wk, wl, en, ga, gb, gc)) continue;
      g = sub(g, add(add(ga, gb), gc));
      e[3] = e[3] + en, ++cnt[3];
    }
  for (int q = r0; q < r1; ++q) {  // inversions of a neighbour
    const int j = row_nbr(s.adj[q]);
    if (!inverts(s, j)) continue;
    for (int t = 0; t < 3; ++t) {
      if (!inversion_at(s, X, j, t, deg_tol, wi, wk, wl, en, ga, gb, gc)) continue;
      const D3 mine = wi == a ? ga : wk == a ? gb : gc;
      g = add(g, mine);
    }
  }
  const double* qa = s.par[s.typ[a]];
  const double xa = qa[RX_X], da = qa[RX_SQRT_D];
  unsigned word = 0u;
  for (int b = 0; b < n_all; ++b) {  // van der Waals
    if ((b & 31) == 0) word = s.mask[b >> 5][a];
    if ((word >> (b & 31)) & 1u) continue;
    const double* qb = s.par[s.typ[b]];
    vdw_term(pa, at(X, b), xa * qb[RX_X], da * qb[RX_SQRT_D], en, ga);
    g = add(g, ga);
    if (a < b) e[4] = e[4] + en, ++cnt[4];
  }
  gout = g;
}

// Energy and gradient at X: the gradient into g (this thread's atom), the five component sums into comp, -> the total
__device__ inline double evaluate(RxShared& s, const Pos3& X, int n_all, double deg_tol, D3& g, double* comp, int* cnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double e[5];
  g = {};
#pragma unroll
  for (int c = 0; c < 5; ++c) e[c] = 0.0, cnt[c] = 0;
  if (tid < n_all) eval_atom(s, X, tid, n_all, deg_tol, g, e, cnt);
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const double w = wave_sum(e[c]);
    if (lane == 0) s.red[c][wave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 5; ++c) comp[c] = ((s.red[c][0] + s.red[c][1]) + s.red[c][2]) + s.red[c][3];
  __syncthreads();
  return (((comp[0] + comp[1]) + comp[2]) + comp[3]) + comp[4];
}

// status and zeros for a molecule that is not relaxed; its per-atom slots only when they are inside the arrays
__device__ inline void write_unmeasured(const RxArgs& A, int m, int status, const MolView& v) {
  const int tid = threadIdx.x;
  if (tid < RX_STATS) A.o.mol_stats[(size_t)m * RX_STATS + tid] = tid == R_STATUS ? status : 0;
  if (tid < RX_ENERGIES) A.o.mol_energy[(size_t)m * RX_ENERGIES + tid] = 0.0;
  if (v.outside) return;
  for (long long a = v.n0 + tid; a < v.n0 + v.n; a += 256) {
    for (int q = 0; q < 3; ++q) A.o.pos_out[3 * a + q] = 0.0, A.o.grad_out[3 * a + q] = 0.0;
    for (int q = 0; q < 3 * RX_MAX_H; ++q) A.o.h_pos_out[3 * RX_MAX_H * a + q] = 0.0, A.o.h_grad_out[3 * RX_MAX_H * a + q] = 0.0;
  }
}

__global__ __launch_bounds__(256) void mol_relax_kernel(const RxArgs A) {
  __shared__ RxShared s;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n;
  if (const int unmeasured = mol_guard(v); unmeasured != MOL_MEASURE) {  // uniform
    write_unmeasured(A, m, unmeasured, v);
    return;
  }
  const bool in = tid < n;
  const AllAtomCount aa = allatom_count(A.o.h_count + n0, n, s.off, s.cur, s.wave_total);
  const int n_all = aa.n_all;
  if (n_all > MOL_ATOMS) {  // uniform
    write_unmeasured(A, m, STATUS_TOO_LARGE, v);
    return;
  }
  const double deg_tol = A.tab.deg_tol;
  if (tid >= n_all) put(s.x, tid, D3{});
  if (in) {  // every entry of x has one writer; the barriers of the staging publish them
    const float* q = A.o.atom_pos + 3 * (n0 + tid);
    put(s.x, tid, D3{{(double)q[0], (double)q[1], (double)q[2]}});
    const double* hp = A.o.h_pos + 3 * RX_MAX_H * (n0 + tid);
    for (int k = 0; k < aa.h; ++k) put(s.x, n + aa.hoff + k, D3{{hp[3 * k], hp[3 * k + 1], hp[3 * k + 2]}});  // n + hoff + k < n_all <= 256
  }
  const int fallback = allatom_stage(s, A.mol, v, A.tab, A.o.order + h0, A.o.atom_flag + n0, aa, s.bk);
  {  // the excluded pairs of this atom: itself, its neighbours and theirs
    unsigned w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    auto mark = [&](int b) {
#pragma unroll
      for (int c = 0; c < 8; ++c) w[c] |= (b >> 5) == c ? 1u << (b & 31) : 0u;
    };
    if (tid < n_all) {
      mark(tid);
      for (int q = s.off[tid]; q < s.off[tid + 1]; ++q) {
        const int b = row_nbr(s.adj[q]);
        mark(b);
        for (int p = s.off[b]; p < s.off[b + 1]; ++p) mark(row_nbr(s.adj[p]));
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) s.mask[c][tid] = w[c];
  }
  __syncthreads();

  // ---- the starting point, then the minimiser
  double comp0[5], comp[5], compt[5];
  int cnt0[5], cnt[5];
  D3 g0;
  const double E0 = evaluate(s, s.x, n_all, deg_tol, g0, comp0, cnt0);
  const double gg0 = block_sum(s.lb, dot(g0, g0));
  if (!isfinite(E0) || !isfinite(gg0)) {  // uniform
    write_unmeasured(A, m, STATUS_NONFINITE, v);
    return;
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) comp[c] = comp0[c];
  double* hist = A.o.ws + (size_t)m * RX_WS_DOUBLES + tid;  // slot q: s at hist[(2 q) * 768 + c * 256], y at hist[(2 q + 1) * 768 + c * 256]
  const Lbfgs<3> r = lbfgs_minimise(
      s.lb, s.x, s.xt, n_all, A.tab.gtol, A.tab.max_step, A.tab.max_iters, E0, g0, gg0,
      [&](const Pos3& P, D3& gp) { return evaluate(s, P, n_all, deg_tol, gp, compt, cnt); },
      [&] {
#pragma unroll
        for (int c = 0; c < 5; ++c) comp[c] = compt[c];
      },
      [&](int q, int which) { return each<3>([&](int k) { return hist[(2 * q + which) * 768 + k * 256]; }); },
      [&](int q, int which, D3 u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) hist[(2 * q + which) * 768 + k * 256] = u[k];
      });

  // ---- the outputs
  put(s.g, tid, r.g);
  double moved = 0.0;
  if (in) {
    const float* q = A.o.atom_pos + 3 * (n0 + tid);
    const D3 dx = sub(at(s.x, tid), D3{{(double)q[0], (double)q[1], (double)q[2]}});
    moved = dot(dx, dx);
  }
  moved = block_sum(s.lb, moved);  // its barriers also publish x and g
  const int counted[6] = {cnt0[0], cnt0[1], cnt0[2], cnt0[3], cnt0[4], fallback};  // R_BONDS .. R_FALLBACK
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int sum = wave_sum(counted[c]);
    if (lane == 0) s.ired[wave][c] = sum;
  }
  __syncthreads();
  if (tid < 6) A.o.mol_stats[(size_t)m * RX_STATS + R_BONDS + tid] = (s.ired[0][tid] + s.ired[1][tid]) + (s.ired[2][tid] + s.ired[3][tid]);
  if (in) {
    allatom_write(s.x, n, aa, A.o.pos_out + 3 * (n0 + tid), A.o.h_pos_out + 3 * RX_MAX_H * (n0 + tid));
    allatom_write(s.g, n, aa, A.o.grad_out + 3 * (n0 + tid), A.o.h_grad_out + 3 * RX_MAX_H * (n0 + tid));
  }
  if (tid == 0) {
    int* st = A.o.mol_stats + (size_t)m * RX_STATS;
    st[R_STATUS] = STATUS_OK, st[R_REASON] = r.reason, st[R_ITERS] = r.iters, st[R_EVALS] = 1 + r.evals, st[R_NALL] = n_all;
    double* en = A.o.mol_energy + (size_t)m * RX_ENERGIES;
    for (int c = 0; c < 5; ++c) en[c] = comp0[c], en[6 + c] = comp[c];
    en[5] = E0, en[11] = r.E, en[12] = r.rms, en[13] = n ? sqrt(moved / (double)n) : 0.0;
  }
}

}  // namespace

extern "C" int mdx_mol_relax(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms, const int32_t* n_bonds,
                             const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type, const int32_t* bond_index, int64_t Eh_stride,
                             const int32_t* select, const float* atom_pos, const int32_t* order, const double* h_pos, const int32_t* h_count,
                             const int32_t* atom_flag, int32_t num_element, int32_t num_bond_types, const double* ff_rows, int32_t n_rows,
                             double deg_tol, double gtol, double max_step, int32_t max_iters, double* pos_out, double* h_pos_out, double* grad_out,
                             double* h_grad_out, int32_t* mol_stats, double* mol_energy, double* ws, size_t ws_bytes, void* stream) {
  RxArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  a.o = RelaxOperands{atom_pos, order, h_pos, h_count, atom_flag, pos_out, h_pos_out, grad_out, h_grad_out, mol_stats, mol_energy, ws};
  if (const char* why = relax_check(a.o, B, ws_bytes)) return mdx_set_error(MDX_ERR_ARG, why);
  const char* why = "";
  if (relax_prepare(&a.tab, ff_rows, n_rows, num_element, num_bond_types, deg_tol, gtol, max_step, max_iters, &why) != RX_PREP_OK)
    return mdx_set_error(MDX_ERR_ARG, why);
  return mol_launch(mol_relax_kernel, "mol_relax_kernel", B, stream, a);
}
