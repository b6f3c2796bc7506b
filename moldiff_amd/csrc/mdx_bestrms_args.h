// Host-side validation of mdx_mol_bestrms (mdx_bestrms.hip) and the small float64 solve its leaf runs: the operands behind the shared
// compact-molecule prefix, and the eigenvalues of Horn's quaternion matrix by cyclic Jacobi.  Plain C++ without HIP, so that it can be
// built on its own under a host sanitizer (tools/bestrms_host_check.cpp); the kernel compiles the same solver for the device.  rank,
// canon_status, the pair list and the target pointers live on the device and are the caller's word there; the kernel keeps every index
// it forms from them inside the arrays.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BR_HD __host__ __device__
#else
#define BR_HD
#endif

constexpr int BR_MAX_NODES = 1 << 20;
constexpr int BR_STATS = 3;        // = MDX_BESTRMS_STATS of include/moldiff_hip.h
constexpr int BR_SWEEPS = 16;      // the most Jacobi sweeps; a 4 x 4 matrix is done after 5 to 7
constexpr double BR_OFF = 1e-36;   // a sweep is run while the squared off-diagonal part is above this share of the squared norm

// The inputs behind the compact arrays and every output of one call.
struct BestrmsOperands {
  const float* atom_pos;
  const int32_t* atom_label;  // or nullptr: the label is atom_type
  const int32_t *rank, *canon_status;
  const int32_t *pair_ptr, *pair_target;
  const int32_t *tgt_ptr, *tgt_n;
  const float* tgt_pos;
  double *msd, *msd_mirror, *msd_first;
  int32_t *pair_stats, *mol_stats;
};

// -> nullptr, or the reason the call is refused
inline const char* bestrms_check(const BestrmsOperands& o, int64_t P_cap, int32_t T, int64_t tgt_atoms, int32_t max_nodes) {
  if (!o.atom_pos || !o.rank || !o.canon_status || !o.pair_ptr || !o.pair_target || !o.tgt_ptr || !o.tgt_n || !o.tgt_pos || !o.msd ||
      !o.msd_mirror || !o.msd_first || !o.pair_stats || !o.mol_stats)
    return "null argument";
  if (P_cap < 0 || T < 0 || tgt_atoms < 0) return "negative size";
  if (P_cap >= (int64_t)1 << 31 || tgt_atoms >= (int64_t)1 << 31) return "pair_ptr and tgt_ptr are int32: fewer than 2^31 pairs and target atoms";
  if (max_nodes < 1 || max_nodes > BR_MAX_NODES) return "max_nodes must lie in 1 .. 2^20";
  return nullptr;
}

// one Jacobi rotation of the symmetric 4 x 4 matrix `a` (upper triangle) that makes a[P][Q] zero; R1 and R2 are the other two indices.
// Every index is a constant, so the matrix stays in registers on the device.
template <int P, int Q, int R>
BR_HD inline void br_turn(double (&a)[4][4], double s, double tau) {
  double &g = a[P < R ? P : R][P < R ? R : P], &h = a[Q < R ? Q : R][Q < R ? R : Q];
  const double g0 = g, h0 = h;
  g = g0 - s * (h0 + tau * g0);
  h = h0 + s * (g0 - tau * h0);
}
template <int P, int Q, int R1, int R2>
BR_HD inline void br_rotate(double (&a)[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));  // theta^2 = inf gives t = 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = 0.0;
  br_turn<P, Q, R1>(a, s, tau);
  br_turn<P, Q, R2>(a, s, tau);
}

// H = sum p q^T (row-major, h[3 i + j] = sum p_i q_j) -> the largest and the smallest eigenvalue of Horn's symmetric quaternion matrix
// of H: s1 + s2 + sign(det H) s3 and -(s1 + s2 - sign(det H) s3), s1 >= s2 >= s3 >= 0 the singular values of H.  The second is the
// first of -H with its sign changed: the mirror image.  Cyclic Jacobi in the fixed order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), eigenvalues
// only.  Build without floating-point contraction where the result has to repeat bit by bit.
BR_HD inline void bestrms_solve(const double* h, double* lmax, double* lmin) {
  const double xx = h[0], xy = h[1], xz = h[2], yx = h[3], yy = h[4], yz = h[5], zx = h[6], zy = h[7], zz = h[8];
  double a[4][4] = {{(xx + yy) + zz, yz - zy, zx - xz, xy - yx},
                    {0.0, (xx - yy) - zz, xy + yx, zx + xz},
                    {0.0, 0.0, (yy - xx) - zz, yz + zy},
                    {0.0, 0.0, 0.0, (zz - xx) - yy}};
  const double diag = (a[0][0] * a[0][0] + a[1][1] * a[1][1]) + (a[2][2] * a[2][2] + a[3][3] * a[3][3]);
  double off =((a[0][1] * a[0][1] + a[0][2] * a[0][2]) + (a[0][3] * a[0][3] + a[1][2] * a[1][2])) + (a[1][3] * a[1][3] + a[2][3] * a[2][3]);
  const double bound = BR_OFF * (diag + 2.0 * off);
  for (int sweep = 0; sweep < BR_SWEEPS; ++sweep) {
    off = ((a[0][1] * a[0][1] + a[0][2] * a[0][2]) + (a[0][3] * a[0][3] + a[1][2] * a[1][2])) + (a[1][3] * a[1][3] + a[2][3] * a[2][3]);
    if (!(off > bound)) break;  // also with a NaN
    br_rotate<0, 1, 2, 3>(a);
    br_rotate<0, 2, 1, 3>(a);
    br_rotate<0, 3, 1, 2>(a);
    br_rotate<1, 2, 0, 3>(a);
    br_rotate<1, 3, 0, 2>(a);
    br_rotate<2, 3, 0, 1>(a);
  }
  *lmax = fmax(fmax(a[0][0], a[1][1]), fmax(a[2][2], a[3][3]));
  *lmin = fmin(fmin(a[0][0], a[1][1]), fmin(a[2][2], a[3][3]));
}

// the two mean squared deviations of one atom map from G = Ga + Gb, the eigenvalues and the atom count (n >= 1)
BR_HD inline void bestrms_msd(double G, double lmax, double lmin, int n, double* msd, double* mirror) {
  *msd = fmax(0.0, G - 2.0 * lmax) / (double)n;
  *mirror = fmax(0.0, G + 2.0 * lmin) / (double)n;
}
