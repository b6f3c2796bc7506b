// Host-side preparation of mdx_mol_relax (mdx_relax.hip): validation of the caller's force-field rows and of the minimiser's scalars,
// and their packing into the block that travels as kernel arguments: one row of derived parameters per atom type (cosine of the rest
// angle, square roots of chi and D: every transcendental is taken here, on the host), the (class, variant) -> row map with its
// fall-back marks, and the logarithms of the four bond orders.  relax_pair gives the rest length and force constant of a bond
// between two rows from those, with + - x / only: the kernel fills its per-bond table with it and tools/relax_host_check.cpp prints
// the same table on the host.  Plain C++ without HIP, so that it can be built on its own under a host sanitizer.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RX_BOTH __host__ __device__
#else
#define RX_BOTH
#endif

constexpr int RX_MAX_ELEMENTS = 32, RX_MAX_BOND_TYPES = 16, RX_MAX_TYPES = 32, RX_MAX_H = 4;
constexpr int RX_STATS = 11, RX_ENERGIES = 14;  // = MDX_RELAX_STATS, MDX_RELAX_ENERGIES of include/moldiff_hip.h
constexpr int RX_HISTORY = 8, RX_WS_DOUBLES = 2 * RX_HISTORY * 768;  // per molecule: 8 x (s, y) x 3 x 256
constexpr int RX_MAX_ITERS = 100000;
// a caller's row: class (-1 = hydrogen), variant, r, theta0 in degrees, x, D, Z, chi, V, U, K_inv
enum { RX_IN_CLASS, RX_IN_VARIANT, RX_IN_R, RX_IN_THETA, RX_IN_X, RX_IN_D, RX_IN_Z, RX_IN_CHI, RX_IN_V, RX_IN_U, RX_IN_KINV, RX_IN };
// a packed row
enum { RX_R, RX_C0, RX_X, RX_SQRT_D, RX_Z, RX_CHI, RX_SQRT_CHI, RX_V, RX_U, RX_KINV, RX_NPAR };
enum { RX_TETRAHEDRAL = 0, RX_TRIGONAL = 1, RX_LINEAR = 2, RX_RESONANT = 3, RX_HYDROGEN = 4 };
constexpr unsigned char RX_FALLBACK = 0x80;

enum { RX_PREP_OK = 0, RX_PREP_ARG = 1 };  // = MDX_OK, MDX_ERR_ARG

struct RelaxTable {
  double par[RX_MAX_TYPES][RX_NPAR];
  double ln_order[4];                         // ln 1, ln 1.5, ln 2, ln 3: the order index of a bond
  double deg_tol, gtol, max_step;
  unsigned char type_of[RX_MAX_ELEMENTS][4];  // row of (class, variant) | RX_FALLBACK when it is the class's tetrahedral row instead
  int32_t h_type, n_types, max_iters, num_element, num_bond_types;
};

// the caller's device operands beside the compact arrays: what is read, then what is written
struct RelaxOperands {
  const float* atom_pos;
  const int32_t* order;
  const double* h_pos;
  const int32_t *h_count, *atom_flag;
  double *pos_out, *h_pos_out, *grad_out, *h_grad_out;
  int32_t* mol_stats;
  double *mol_energy, *ws;
};

inline const char* relax_check(const RelaxOperands& o, int32_t B, size_t ws_bytes) {
  if (!o.atom_pos || !o.order || !o.h_pos || !o.h_count || !o.atom_flag || !o.pos_out || !o.h_pos_out || !o.grad_out || !o.h_grad_out ||
      !o.mol_stats || !o.mol_energy || !o.ws)
    return "null argument";
  if (B > 0 && ws_bytes / (sizeof(double) * RX_WS_DOUBLES) < (size_t)B) return "workspace too small: B x 16 x 768 doubles";
  return nullptr;
}

// Rest length and force constant of a bond of order index o (0: 1, 1: 1.5, 2: 2, 3: 3) between rows a and b:
//   r = (ri + rj) - (0.1332 (ri + rj)) ln n - (ri rj) (si - sj)^2 / (chi_i ri + chi_j rj),   k = 664.12 Zi Zj / r^3
RX_BOTH inline void relax_pair(const double* a, const double* b, double ln_n, double* r0, double* k) {
  const double sum = a[RX_R] + b[RX_R];
  const double ds = a[RX_SQRT_CHI] - b[RX_SQRT_CHI];
  const double en = ((a[RX_R] * b[RX_R]) * (ds * ds)) / (a[RX_CHI] * a[RX_R] + b[RX_CHI] * b[RX_R]);
  const double r = (sum - (0.1332 * sum) * ln_n) - en;
  *r0 = r;
  *k = ((664.12 * a[RX_Z]) * b[RX_Z]) / ((r * r) * r);
}

// Validates the HOST rows and the scalars and fills `t`.  On failure *why names the cause and `t` may be partly written.
inline int relax_prepare(RelaxTable* t, const double* rows, int32_t n_rows, int32_t num_element, int32_t num_bond_types, double deg_tol,
                         double gtol, double max_step, int32_t max_iters, const char** why) {
  if (num_element < 1 || num_element > RX_MAX_ELEMENTS || num_bond_types < 1 || num_bond_types > RX_MAX_BOND_TYPES)
    return *why = "num_element must lie in 1 .. 32 and num_bond_types in 1 .. 16", RX_PREP_ARG;
  if (!rows) return *why = "null argument", RX_PREP_ARG;
  if (n_rows < 1 || n_rows > RX_MAX_TYPES) return *why = "the force field holds 1 .. 32 rows", RX_PREP_ARG;
  if (!(deg_tol > 0.0 && deg_tol < 1.0)) return *why = "deg_tol must lie in (0, 1)", RX_PREP_ARG;  // NaN fails
  if (!(gtol > 0.0 && gtol <= 1.0e6)) return *why = "gtol must lie in (0, 1e6]", RX_PREP_ARG;
  if (!(max_step > 0.0 && max_step <= 10.0)) return *why = "max_step must lie in (0, 10]", RX_PREP_ARG;
  if (max_iters < 0 || max_iters > RX_MAX_ITERS) return *why = "max_iters must lie in 0 .. 100000", RX_PREP_ARG;
  for (int c = 0; c < RX_MAX_ELEMENTS; ++c)
    for (int v = 0; v < 4; ++v) t->type_of[c][v] = 0xff;
  t->h_type = -1;
  for (int q = 0; q < RX_MAX_TYPES; ++q)
    for (int p = 0; p < RX_NPAR; ++p) t->par[q][p] = 0.0;
  for (int q = 0; q < n_rows; ++q) {
    const double* in = rows + (size_t)q * RX_IN;
    const double cd = in[RX_IN_CLASS], vd = in[RX_IN_VARIANT];
    if (!(cd >= -1.0 && cd < (double)num_element && cd == floor(cd))) return *why = "a row's class must be -1 (hydrogen) or lie below num_element", RX_PREP_ARG;
    if (!(vd >= 0.0 && vd <= 3.0 && vd == floor(vd))) return *why = "a row's variant must lie in 0 .. 3", RX_PREP_ARG;
    const int c = (int)cd, v = (int)vd;
    if (c < 0) {
      if (t->h_type >= 0 || v != 0) return *why = "one hydrogen row, of variant 0", RX_PREP_ARG;
      t->h_type = q;
    } else {
      if (t->type_of[c][v] != 0xff) return *why = "two rows for one (class, variant)", RX_PREP_ARG;
      t->type_of[c][v] = (unsigned char)q;
    }
    const double r = in[RX_IN_R], th = in[RX_IN_THETA], x = in[RX_IN_X], D = in[RX_IN_D], Z = in[RX_IN_Z], chi = in[RX_IN_CHI];
    if (!(r > 0.0 && r <= 4.0)) return *why = "r must lie in (0, 4]", RX_PREP_ARG;
    if (!(th > 0.0 && th <= 180.0)) return *why = "theta0 must lie in (0, 180]", RX_PREP_ARG;
    if (!(x > 0.0 && x <= 10.0)) return *why = "x must lie in (0, 10]", RX_PREP_ARG;
    if (!(D >= 0.0 && D <= 10.0)) return *why = "D must lie in [0, 10]", RX_PREP_ARG;
    if (!(Z > 0.0 && Z <= 100.0)) return *why = "Z must lie in (0, 100]", RX_PREP_ARG;
    if (!(chi > 0.0 && chi <= 100.0)) return *why = "chi must lie in (0, 100]", RX_PREP_ARG;
    for (int p = RX_IN_V; p <= RX_IN_KINV; ++p)
      if (!(in[p] >= 0.0 && in[p] <= 1.0e3)) return *why = "V, U and K_inv must lie in [0, 1000]", RX_PREP_ARG;
    double* o = t->par[q];
    o[RX_R] = r, o[RX_C0] = th == 180.0 ? -1.0 : cos(th * (M_PI / 180.0)), o[RX_X] = x, o[RX_SQRT_D] = sqrt(D), o[RX_Z] = Z, o[RX_CHI] = chi;
    o[RX_SQRT_CHI] = sqrt(chi), o[RX_V] = in[RX_IN_V], o[RX_U] = in[RX_IN_U], o[RX_KINV] = in[RX_IN_KINV];
  }
  if (t->h_type < 0) return *why = "no hydrogen row", RX_PREP_ARG;
  for (int c = 0; c < num_element; ++c) {
    if (t->type_of[c][0] == 0xff) return *why = "every class needs its tetrahedral row", RX_PREP_ARG;
    for (int v = 1; v < 4; ++v)
      if (t->type_of[c][v] == 0xff) t->type_of[c][v] = (unsigned char)(t->type_of[c][0] | RX_FALLBACK);
  }
  t->ln_order[0] = 0.0, t->ln_order[1] = log(1.5), t->ln_order[2] = log(2.0), t->ln_order[3] = log(3.0);
  t->deg_tol = deg_tol, t->gtol = gtol, t->max_step = max_step, t->max_iters = max_iters, t->n_types = n_rows;
  t->num_element = num_element, t->num_bond_types = num_bond_types;
  return RX_PREP_OK;
}
