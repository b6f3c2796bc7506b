// Stand-alone check of the host-side validation of mdx_mol_bestrms and of the float64 solve its kernel runs
// (moldiff_amd/csrc/mdx_bestrms_args.h, and the shared operand prefix of moldiff_amd/csrc/mdx_mol.h).  No HIP, no GPU; meant to be
// built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/bestrms_host_check.cpp -o /tmp/bestrms_host_check
//     /tmp/bestrms_host_check
//
// The validation reads no operand: every pointer below is a heap block of one element, so a dereference past it is an AddressSanitizer
// report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../moldiff_amd/csrc/mdx_bestrms_args.h"
#include "../moldiff_amd/csrc/mdx_mol.h"

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static bool near(double a, double b, double scale) { return std::fabs(a - b) <= 1e-14 * scale; }

int main() {
  int32_t* i32 = (int32_t*)std::malloc(sizeof(int32_t));
  float* f32 = (float*)std::malloc(sizeof(float));
  double* f64 = (double*)std::malloc(sizeof(double));
  const BestrmsOperands full{f32, i32, i32, i32, i32, i32, i32, i32, f32, f64, f64, f64, i32, i32};
  EXPECT(bestrms_check(full, 0, 0, 0, 1) == nullptr && bestrms_check(full, 10, 3, 100, 1 << 20) == nullptr);
  const char* why = bestrms_check(full, 10, 3, 100, 0);
  EXPECT(why && std::strstr(why, "max_nodes"));
  EXPECT(bestrms_check(full, 10, 3, 100, (1 << 20) + 1) && bestrms_check(full, 10, 3, 100, -1));
  EXPECT((why = bestrms_check(full, -1, 3, 100, 100)) && std::strstr(why, "negative"));
  EXPECT((why = bestrms_check(full, 10, -3, 100, 100)) && std::strstr(why, "negative"));
  EXPECT((why = bestrms_check(full, 10, 3, -100, 100)) && std::strstr(why, "negative"));
  EXPECT((why = bestrms_check(full, (int64_t)1 << 31, 3, 100, 100)) && std::strstr(why, "2^31"));
  EXPECT((why = bestrms_check(full, 10, 3, (int64_t)1 << 31, 100)) && std::strstr(why, "2^31"));
  BestrmsOperands o = full;
  o.atom_label = nullptr;
  EXPECT(bestrms_check(o, 10, 3, 100, 100) == nullptr);  // the one optional operand
  const float* BestrmsOperands::*floats[] = {&BestrmsOperands::atom_pos, &BestrmsOperands::tgt_pos};
  for (auto member : floats) {
    o = full, o.*member = nullptr;
    EXPECT((why = bestrms_check(o, 10, 3, 100, 100)) && std::strstr(why, "null"));
  }
  const int32_t* BestrmsOperands::*inputs[] = {&BestrmsOperands::rank,        &BestrmsOperands::canon_status, &BestrmsOperands::pair_ptr,
                                               &BestrmsOperands::pair_target, &BestrmsOperands::tgt_ptr,      &BestrmsOperands::tgt_n};
  for (auto member : inputs) {
    o = full, o.*member = nullptr;
    EXPECT((why = bestrms_check(o, 10, 3, 100, 100)) && std::strstr(why, "null"));
  }
  double* BestrmsOperands::*columns[] = {&BestrmsOperands::msd, &BestrmsOperands::msd_mirror, &BestrmsOperands::msd_first};
  for (auto member : columns) {
    o = full, o.*member = nullptr;
    EXPECT((why = bestrms_check(o, 10, 3, 100, 100)) && std::strstr(why, "null"));
  }
  int32_t* BestrmsOperands::*tables[] = {&BestrmsOperands::pair_stats, &BestrmsOperands::mol_stats};
  for (auto member : tables) {
    o = full, o.*member = nullptr;
    EXPECT((why = bestrms_check(o, 10, 3, 100, 100)) && std::strstr(why, "null"));
  }

  // the solve: H = diag(3, 2, 1) has s = (3, 2, 1) and det > 0; a reflection of it changes the sign of s3's term
  double lmax, lmin;
  const double d[9] = {3, 0, 0, 0, 2, 0, 0, 0, 1};
  bestrms_solve(d, &lmax, &lmin);
  EXPECT(near(lmax, 6.0, 6.0) && near(lmin, -4.0, 6.0));
  const double r[9] = {3, 0, 0, 0, 2, 0, 0, 0, -1};
  bestrms_solve(r, &lmax, &lmin);
  EXPECT(near(lmax, 4.0, 6.0) && near(lmin, -6.0, 6.0));
  // a rotation about z by 0.3 times diag(3, 2, 1): the same singular values
  const double c = std::cos(0.3), s = std::sin(0.3);
  const double rot[9] = {3 * c, -2 * s, 0, 3 * s, 2 * c, 0, 0, 0, 1};
  bestrms_solve(rot, &lmax, &lmin);
  EXPECT(near(lmax, 6.0, 6.0) && near(lmin, -4.0, 6.0));
  // degenerate: zero, rank one (collinear), rank two (planar), tiny and huge scales, and a NaN (the sweeps end)
  const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  bestrms_solve(zero, &lmax, &lmin);
  EXPECT(lmax == 0.0 && lmin == 0.0);
  const double line[9] = {0, 0, 0, 0, 0, 5, 0, 0, 0};
  bestrms_solve(line, &lmax, &lmin);
  EXPECT(near(lmax, 5.0, 5.0) && near(lmin, -5.0, 5.0));
  const double plane[9] = {0, 4, 0, 1, 0, 0, 0, 0, 0};
  bestrms_solve(plane, &lmax, &lmin);
  EXPECT(near(lmax, 5.0, 5.0) && near(lmin, -5.0, 5.0));
  for (double scale : {1e-150, 1e150}) {
    double h[9];
    for (int i = 0; i < 9; ++i) h[i] = rot[i] * scale;
    bestrms_solve(h, &lmax, &lmin);
    EXPECT(near(lmax, 6.0 * scale, 6.0 * scale) && near(lmin, -4.0 * scale, 6.0 * scale));
  }
  double bad[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  bad[4] = std::nan("");
  bestrms_solve(bad, &lmax, &lmin);  // ends; the values are unspecified
  double msd, mirror;
  bestrms_msd(14.0 + 14.0, 14.0, -12.0, 3, &msd, &mirror);
  EXPECT(msd == 0.0 && near(mirror, 4.0 / 3.0, 2.0));
  bestrms_msd(1.0, 0.5 + 1e-17, -0.6, 2, &msd, &mirror);  // a rounding below zero is cut
  EXPECT(msd == 0.0 && mirror == 0.0);

  // the shared prefix
  MolArrays a;
  EXPECT(mol_arrays_fill(&a, 3, i32, i32, i32, i32, i32, 10, i32, i32, 7, nullptr) == nullptr);
  EXPECT(a.bond_j == i32 + 7 && a.N_cap == 10 && a.E_cap == 7 && a.select == nullptr);
  EXPECT((why = mol_arrays_fill(&a, 3, i32, nullptr, i32, i32, i32, 10, i32, i32, 7, nullptr)) && std::strstr(why, "null"));
  std::free(i32), std::free(f32), std::free(f64);
  std::printf(failures ? "%d FAILED\n" : "bestrms_host_check ok\n", failures);
  return failures != 0;
}
