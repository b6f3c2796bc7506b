// Host-side preparation of mdx_mol_bounds (mdx_bounds.hip) and mdx_mol_embed (mdx_embed.hip): validation of the scalars and of the
// workspaces, the ring cosines (every transcendental is taken here, on the host; the force-field rows are those of mdx_relax_args.h),
// and the two distance formulas of the bounds model, which the kernel and tools/embed_host_check.cpp share.  Plain C++ without HIP, so
// that it can be built on its own under a host sanitizer.
#pragma once
#include "mdx_relax_args.h"

constexpr int EB_STATS = 7, EM_STATS = 5, EM_VALUES = 3;  // = MDX_BOUNDS_STATS, MDX_EMBED_STATS, MDX_EMBED_VALUES of include/moldiff_hip.h
constexpr int EM_HIST_PER_ATOM = 2 * RX_HISTORY * 4;      // the history of one (molecule, conformer): 8 x (s, y) x 4 x na_cap doubles
constexpr int EB_MAX_ATOMS = 256, EM_MAX_CONFS = 65535, EM_MAX_ATTEMPTS = 64;
constexpr double EB_FAR = 1000.0;                         // the upper bound of a pair beyond 1-4
constexpr double EM_BOX = 2.0;                            // the box is this factor x the largest 1-2 / 1-3 / 1-4 upper bound
constexpr double EM_W4_A = 0.1, EM_W4_B = 1.0;            // the weight of the fourth coordinate in stages A and B
enum { EM_OK = 0, EM_TOO_LARGE = 1, EM_NONFINITE = 2, EM_INCONSISTENT = 3, EM_FAILED = 4 };
enum { EB_OTHER = 0, EB_12 = 1, EB_13 = 2, EB_14 = 3 };

struct BoundsParams {
  double tol12, tol13, tol14, vdw_scale;
  double ring_c0[3];  // cos 60, 90, 108 degrees: the angle in a ring of 3, 4, 5
  int32_t na_cap;
};

struct BoundsOperands {
  const int32_t *order, *h_count, *atom_flag;
  double* bounds;      // [m][0 lower, 1 upper][na_cap][na_cap]
  unsigned char* cls;  // [m][na_cap][na_cap]
  int32_t* mol_stats;
};

inline size_t bounds_ws_bytes(int32_t B, int32_t na_cap) { return (size_t)B * 17u * (size_t)na_cap * (size_t)na_cap; }

inline const char* bounds_ws_check(int32_t B, int32_t na_cap, const void* ws, size_t ws_bytes) {
  if (na_cap < 1 || na_cap > EB_MAX_ATOMS) return "na_cap must lie in 1 .. 256";
  if (!ws) return "null argument";
  if (B > 0 && ws_bytes < bounds_ws_bytes(B, na_cap)) return "workspace too small: 17 x B x na_cap^2 bytes";
  return nullptr;
}

// -> nullptr, or the reason the call is refused
inline const char* bounds_prepare(BoundsParams* p, double tol12, double tol13, double tol14, double vdw_scale, int32_t na_cap) {
  if (!(tol12 >= 0.0 && tol12 <= 1.0) || !(tol13 >= 0.0 && tol13 <= 1.0) || !(tol14 >= 0.0 && tol14 <= 1.0))  // NaN fails
    return "tol12, tol13 and tol14 must lie in [0, 1]";
  if (!(vdw_scale > 0.0 && vdw_scale <= 2.0)) return "vdw_scale must lie in (0, 2]";
  if (na_cap < 1 || na_cap > EB_MAX_ATOMS) return "na_cap must lie in 1 .. 256";
  p->tol12 = tol12, p->tol13 = tol13, p->tol14 = tol14, p->vdw_scale = vdw_scale, p->na_cap = na_cap;
  p->ring_c0[0] = cos(60.0 * (M_PI / 180.0)), p->ring_c0[1] = cos(90.0 * (M_PI / 180.0)), p->ring_c0[2] = cos(108.0 * (M_PI / 180.0));
  return nullptr;
}

// the 1-3 distance of two bonds r1, r2 that enclose an angle of cosine c
RX_BOTH inline double bounds_13(double r1, double r2, double c) { return sqrt((r1 * r1 + r2 * r2) - ((2.0 * r1) * r2) * c); }

// the 1-4 distances of the planar chain r1, r2, r3 with the cosines c1, c2 at its two inner atoms: both ends on one side, on opposite sides
RX_BOTH inline void bounds_14(double r1, double r2, double r3, double c1, double c2, double* cis, double* trans) {
  const double s1 = sqrt(1.0 - c1 * c1), s2 = sqrt(1.0 - c2 * c2);
  const double dx = (r2 - r3 * c2) - r1 * c1;
  const double yc = r3 * s2 - r1 * s1, yt = r3 * s2 + r1 * s1;
  *cis = sqrt(dx * dx + yc * yc);
  *trans = sqrt(dx * dx + yt * yt);
}

struct EmbedParams {
  double gtol, max_step, viol_tol;
  uint64_t seed;
  int32_t na_cap, n_confs, max_iters, max_attempts;
};

struct EmbedOperands {
  const int32_t* h_count;
  const int64_t* mol_ids;
  const double* bounds;
  const unsigned char* cls;
  const int32_t* bounds_stats;
  double *pos_out, *h_pos_out;
  int32_t* conf_stats;
  double *conf_values, *hist;
};

inline const char* embed_prepare(EmbedParams* p, int32_t B, int32_t na_cap, int32_t n_confs, uint64_t seed, int32_t max_iters, int32_t max_attempts,
                                 double gtol, double max_step, double viol_tol, size_t hist_bytes) {
  if (na_cap < 1 || na_cap > EB_MAX_ATOMS) return "na_cap must lie in 1 .. 256";
  if (n_confs < 1 || n_confs > EM_MAX_CONFS) return "n_confs must lie in 1 .. 65535";
  if (max_iters < 0 || max_iters > RX_MAX_ITERS) return "max_iters must lie in 0 .. 100000";
  if (max_attempts < 1 || max_attempts > EM_MAX_ATTEMPTS) return "max_attempts must lie in 1 .. 64";
  if (!(gtol > 0.0 && gtol <= 1.0e6)) return "gtol must lie in (0, 1e6]";
  if (!(max_step > 0.0 && max_step <= 10.0)) return "max_step must lie in (0, 10]";
  if (!(viol_tol > 0.0 && viol_tol <= 10.0)) return "viol_tol must lie in (0, 10]";
  if (B > 0 && hist_bytes / (sizeof(double) * EM_HIST_PER_ATOM * (size_t)na_cap) < (size_t)B * (size_t)n_confs)
    return "history too small: B x n_confs x 64 x na_cap doubles";
  p->gtol = gtol, p->max_step = max_step, p->viol_tol = viol_tol, p->seed = seed;
  p->na_cap = na_cap, p->n_confs = n_confs, p->max_iters = max_iters, p->max_attempts = max_attempts;
  return nullptr;
}

// two Philox words -> a double in [0, 1), exactly: 27 bits of p and 26 bits of q
RX_BOTH inline double embed_u53(uint32_t p, uint32_t q) {
  return ((double)(p >> 5) * 67108864.0 + (double)(q >> 6)) * 1.1102230246251565e-16;  // 2^26, 2^-53
}
