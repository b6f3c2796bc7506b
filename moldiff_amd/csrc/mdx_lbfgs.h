// The L-BFGS of mdx_mol_relax (three coordinates per atom) and mdx_mol_embed (four), once: one workgroup of 256 threads, thread a owns
// atom a, the point and the trial point are D arrays of 256 doubles in LDS, and every sum over the threads is a per-thread partial,
// wave_sum (xor butterfly 32 .. 1), then the four wave totals in order.  include/moldiff_hip.h states the iteration, relax.lbfgs_ref
// restates it operation by operation, and the files that include this are built with -ffp-contract=off so that the float64 arithmetic
// is the restatement's: the sequence of block reductions below IS that arithmetic, and their barriers are what order the LDS stores
// between them.  Device only.
#pragma once
#include "mdx_mol.h"
#include "mdx_relax_args.h"

constexpr double LB_ARMIJO = 1e-4, LB_CURVATURE = 1e-10;
constexpr int LB_TRIALS = 20;
enum { STOP_CONVERGED = 0, STOP_MAXITER = 1, STOP_LINESEARCH = 2 };

// the coordinates of one atom; the helpers associate left to right: (x x' + y y') + z z', then + w w'
template <int D>
struct Vec {
  double c[D];
  __device__ double& operator[](int k) { return c[k]; }
  __device__ double operator[](int k) const { return c[k]; }
};
using D3 = Vec<3>;
using D4 = Vec<4>;

template <int D, class F>
__device__ inline Vec<D> each(F&& f) {  // {f(0), f(1), ..}
  Vec<D> r;
#pragma unroll
  for (int k = 0; k < D; ++k) r.c[k] = f(k);
  return r;
}
template <int D>
__device__ inline Vec<D> sub(Vec<D> a, Vec<D> b) {
  return each<D>([&](int k) { return a[k] - b[k]; });
}
template <int D>
__device__ inline Vec<D> scaled(double f, Vec<D> a) {
  return each<D>([&](int k) { return f * a[k]; });
}
template <int D>
__device__ inline double dot(Vec<D> a, Vec<D> b) {
  double r = a[0] * b[0];
#pragma unroll
  for (int k = 1; k < D; ++k) r = r + a[k] * b[k];
  return r;
}
template <int D>
__device__ inline Vec<D> at(const double (&X)[D][MOL_ATOMS], int a) {
  return each<D>([&](int k) { return X[k][a]; });
}
template <int D>
__device__ inline void put(double (&X)[D][MOL_ATOMS], int a, Vec<D> v) {
#pragma unroll
  for (int k = 0; k < D; ++k) X[k][a] = v[k];
}

// the LDS words of the reductions and of the history's scalars; a kernel embeds one in its __shared__ struct
struct LbfgsShared {
  double red[4], hsy[RX_HISTORY], hyy[RX_HISTORY], alpha[RX_HISTORY];
};

// the sum of one value per thread: a butterfly in each wave, then ((w0 + w1) + w2) + w3.  Two barriers.
__device__ inline double block_sum(LbfgsShared& s, double v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double w = wave_sum(v);
  if (lane == 0) s.red[wave] = w;
  __syncthreads();
  const double r = ((s.red[0] + s.red[1]) + s.red[2]) + s.red[3];
  __syncthreads();
  return r;
}

__device__ inline double block_max(LbfgsShared& s, double v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if (lane == 0) s.red[wave] = v;
  __syncthreads();
  const double r = fmax(fmax(s.red[0], s.red[1]), fmax(s.red[2], s.red[3]));
  __syncthreads();
  return r;
}

template <int D>
struct Lbfgs {
  double E, rms;  // at the last accepted point
  Vec<D> g;       // this thread's atom
  int iters, evals, reason;
};

// Minimises from the point in X, where the caller has evaluated E, g and gg = block_sum(g . g) and found them finite (a start that is
// not is the caller's uniform early exit), and leaves the last accepted point in X.  evals counts the evaluations made here.
//   eval(P, g) -> the energy at the point P (X or XT), the gradient on this thread's atom into g (zeros past n_all); uniform, it may
//                 hold barriers of its own, and the barrier before it has published P
//   accepted()    runs after the evaluation that a line search accepts: what else that evaluation left becomes the current point's
//   hget(slot, which) / hput(slot, which, v): vector s (which 0) or y (1) of history slot 0 .. 7, this thread's atom; called only
//                 by the threads below n_all, so a layout whose stride is the molecule's own size is never left
template <int D, class Eval, class Accepted, class HGet, class HPut>
__device__ inline Lbfgs<D> lbfgs_minimise(LbfgsShared& s, double (&X)[D][MOL_ATOMS], double (&XT)[D][MOL_ATOMS], int n_all, double gtol, double max_step,
                                          int max_iters, double E, Vec<D> g, double gg, Eval&& eval, Accepted&& accepted, HGet&& hget, HPut&& hput) {
  const int tid = threadIdx.x;
  const bool live = tid < n_all;
  auto neg = [](Vec<D> a) { return each<D>([&](int k) { return -a[k]; }); };
  auto sum = [&](Vec<D> a, Vec<D> b) { return block_sum(s, live ? dot(a, b) : 0.0); };
  int hc = 0, head = 0;  // the history holds slots head .. head + hc - 1 (mod 8), oldest first
  int iters = 0, evals = 0, reason = STOP_CONVERGED;
  double rms = 0.0;
  for (;;) {
    rms = n_all ? sqrt(gg / ((double)D * (double)n_all)) : 0.0;
    if (rms <= gtol) {
      reason = STOP_CONVERGED;
      break;
    }
    if (iters >= max_iters) {
      reason = STOP_MAXITER;
      break;
    }
    Vec<D> d = neg(g);
    if (hc > 0) {  // the two-loop recursion
      Vec<D> q = g;
      for (int t = hc - 1; t >= 0; --t) {
        const int slot = (head + t) & (RX_HISTORY - 1);
        Vec<D> sv = {}, yv = {};
        if (live) sv = hget(slot, 0), yv = hget(slot, 1);
        const double al = sum(sv, q) / s.hsy[slot];
        s.alpha[slot] = al;  // every thread stores the same value and reads its own store
        q = each<D>([&](int k) { return q[k] - al * yv[k]; });
      }
      const int newest = (head + hc - 1) & (RX_HISTORY - 1);
      const double gamma = s.hsy[newest] / s.hyy[newest];
      Vec<D> r = scaled(gamma, q);
      for (int t = 0; t < hc; ++t) {
        const int slot = (head + t) & (RX_HISTORY - 1);
        Vec<D> sv = {}, yv = {};
        if (live) sv = hget(slot, 0), yv = hget(slot, 1);
        const double co = s.alpha[slot] - sum(yv, r) / s.hsy[slot];
        r = each<D>([&](int k) { return r[k] + co * sv[k]; });
      }
      const Vec<D> dl = neg(r);
      const double gd = sum(g, dl);
      if (gd < 0.0) d = dl;
      else hc = 0;
    }
    bool ok = false;
    Vec<D> gt = g;
    const Vec<D> xo = at(X, tid);
    Vec<D> xn = xo;
    double Et = E;
    for (;;) {
      const double big = sqrt(block_max(s, live ? dot(d, d) : 0.0));
      if (big > max_step) d = scaled(max_step / big, d);
      const double gd = sum(g, d);
      double t = 1.0;
      for (int trial = 0; trial < LB_TRIALS; ++trial) {
        xn = each<D>([&](int k) { return xo[k] + t * d[k]; });
        put(XT, tid, xn);
        __syncthreads();
        Et = eval(XT, gt);
        ++evals;
        if (isfinite(Et) && Et <= E + (LB_ARMIJO * t) * gd) {
          ok = true;
          break;
        }
        t = t * 0.5;
      }
      if (ok || hc == 0) break;
      hc = 0;  // once more along the steepest descent
      d = neg(g);
    }
    if (!ok) {
      reason = STOP_LINESEARCH;
      break;
    }
    accepted();
    const Vec<D> sv = sub(xn, xo), yv = sub(gt, g);
    const double sy = sum(sv, yv), ss = sum(sv, sv), yy = sum(yv, yv);
    if (sy > LB_CURVATURE * sqrt(ss * yy)) {
      int slot;
      if (hc == RX_HISTORY) slot = head, head = (head + 1) & (RX_HISTORY - 1);
      else slot = (head + hc) & (RX_HISTORY - 1), ++hc;
      if (live) hput(slot, 0, sv), hput(slot, 1, yv);
      s.hsy[slot] = sy, s.hyy[slot] = yy;
    }
    put(X, tid, xn);  // nobody reads X before the barriers of the next sum
    g = gt, E = Et;
    ++iters;
    gg = block_sum(s, dot(g, g));
  }
  return {E, rms, g, iters, evals, reason};
}
