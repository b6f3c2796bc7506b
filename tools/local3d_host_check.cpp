// Stand-alone check of the host-side preparation of mdx_mol_local3d (moldiff_amd/csrc/mdx_local3d_args.h): validation of the pattern
// table and bins, canonical keys, histogram layout.  No HIP, no GPU; meant to be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/local3d_host_check.cpp -o /tmp/local3d_host_check
//     /tmp/local3d_host_check
//
// Every table is heap-allocated at its exact size, so a read past a row, past kind_ptr[3] rows or past the three bin entries is an
// AddressSanitizer report.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moldiff_amd/csrc/mdx_local3d_args.h"

static int failures = 0;
#define EXPECT(c)                                                    \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);             \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static int prep(Local3DArgs* a, const std::vector<int32_t>& rows, const std::vector<int32_t>& kptr, const std::vector<float>& range,
                const std::vector<int32_t>& count, int ne = 7, int nb = 4) {
  // exact-size heap copies: the vectors' capacity may exceed their size
  int32_t* r = (int32_t*)std::malloc(rows.size() * sizeof(int32_t) + 1);
  int32_t* k = (int32_t*)std::malloc(kptr.size() * sizeof(int32_t));
  float* g = (float*)std::malloc(range.size() * sizeof(float));
  int32_t* c = (int32_t*)std::malloc(count.size() * sizeof(int32_t));
  if (!rows.empty()) std::memcpy(r, rows.data(), rows.size() * sizeof(int32_t));
  std::memcpy(k, kptr.data(), kptr.size() * sizeof(int32_t));
  std::memcpy(g, range.data(), range.size() * sizeof(float));
  std::memcpy(c, count.data(), count.size() * sizeof(int32_t));
  const char* why = "";
  const int rc = local3d_prepare(a, r, k, g, c, ne, nb, &why);
  std::free(r), std::free(k), std::free(g), std::free(c);
  return rc;
}

int main() {
  const std::vector<float> range{1.0f, 2.2f, 0.f, 180.f, -180.f, 180.f};
  const std::vector<int32_t> count{120, 180, 180};
  Local3DArgs a{};
  // N-C:C and a length, an angle, a dihedral: keys are canonical (the smaller of chain and reverse), layout is kind by kind
  std::vector<int32_t> rows{1, 1, 0, 0, 0, 0, 0, /* N-C */ 1, 1, 0, 4, 0, 0, 0, /* N-C:C */ 0, 1, 0, 1, 0, 1, 2 /* C-C-C-O */};
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, range, count) == L3_PREP_OK);
  EXPECT(a.keys[0] == 0x000101ull);            // C-N
  EXPECT(a.keys[1] == 0x0004000101ull);        // C:C-N
  EXPECT(a.keys[2] == 0x00010001000102ull);    // C-C-C-O
  EXPECT(a.kptr[0] == 0 && a.kptr[1] == 1 && a.kptr[2] == 2 && a.kptr[3] == 3);
  EXPECT(a.hoff[0] == 0 && a.hoff[1] == 120 && a.hoff[2] == 300 && a.total_bins == 480 && a.lds_hist == 1);
  EXPECT(a.nbins[2] == 180 && a.lo[2] == -180.f && a.hi[2] == 180.f && a.scale[2] == 0.5f && a.scale[1] == 1.0f);
  // no rows at all
  EXPECT(prep(&a, {}, {0, 0, 0, 0}, range, count) == L3_PREP_OK && a.total_bins == 0);
  // 64 rows of a kind pass, 65 do not; the bin budget decides the histogram path
  std::vector<int32_t> many;
  for (int r = 0; r < 65; ++r) {
    const int32_t row[7] = {r % 7, 1 + r / 49, (r / 7) % 7, 3, 6, 0, 0};   // distinct angle chains; the second bond differs from the first
    many.insert(many.end(), row, row + 7);
  }
  std::vector<int32_t> m64(many.begin(), many.begin() + 64 * 7);
  EXPECT(prep(&a, m64, {0, 0, 64, 64}, range, count) == L3_PREP_OK && a.total_bins == 64 * 180 && a.lds_hist == 0);
  EXPECT(prep(&a, many, {0, 0, 65, 65}, range, count) == L3_PREP_UNSUPPORTED);
  EXPECT(prep(&a, m64, {0, 0, 64, 64}, range, {120, 128, 180}) == L3_PREP_OK && a.total_bins == 8192 && a.lds_hist == 1);
  // refusals
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, {1.f, 1.f, 0.f, 180.f, -180.f, 180.f}, count) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, {1.f, 2.f, 180.f, 0.f, -180.f, 180.f}, count) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, {1.f, 2.f, 0.f, 180.f, -180.f, NAN}, count) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, range, {120, 0, 180}) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, range, {120, -3, 180}) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {1, 1, 2, 3}, range, count) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 2, 1, 3}, range, count) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, range, count, 0, 4) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, range, count, 256, 4) == L3_PREP_ARG);
  EXPECT(prep(&a, rows, {0, 1, 2, 3}, range, count, 7, 255) == L3_PREP_ARG);
  for (int f = 0; f < 7; ++f)
    for (int32_t v : {-1, (f & 1) ? 0 : 7, (f & 1) ? 5 : 7, 1 << 30}) {
      std::vector<int32_t> bad(rows);
      bad[14 + f] = v;   // a field of the dihedral row
      EXPECT(prep(&a, bad, {0, 1, 2, 3}, range, count) == L3_PREP_ARG);
    }
  std::vector<int32_t> tail(rows);
  tail[3] = tail[4] = tail[5] = tail[6] = -77;   // fields past a length row's three are not read
  EXPECT(prep(&a, tail, {0, 1, 2, 3}, range, count) == L3_PREP_OK);
  EXPECT(prep(&a, {0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0}, {0, 2, 2, 2}, range, count) == L3_PREP_ARG);   // C-N and N-C
  EXPECT(prep(&a, {0, 1, 1, 0, 0, 0, 0, 0, 2, 1, 0, 0, 0, 0}, {0, 2, 2, 2}, range, count) == L3_PREP_OK);    // C-N and C=N
  EXPECT(local3d_ws_bytes(0, 0) == 12 && local3d_ws_bytes(10, 5) == 80);
  std::printf(failures ? "local3d host check: %d FAILED\n" : "local3d_host_check ok\n", failures);
  return failures != 0;
}
