// Stand-alone check of the index maps of the persistent row-owner kernels (moldiff_amd/csrc/mdx_plan.h, the header the kernels and
// their launchers compile): the static plan of edge kernel A, its work-queue item map, the pairs' ranges, the XCD remap and the equal
// split of kernel B / the guidance backward / linear_rows.  No HIP, no GPU; tests/test_work_plan_host.py builds and runs it, and it
// can be built with a host sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/work_plan_host_check.cpp -o /tmp/work_plan_host_check
//     /tmp/work_plan_host_check
//
// Everything is enumerated: a unit computed twice or never, or a section dropped, is wrong only at particular (units, slots) pairs.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "../moldiff_amd/csrc/mdx_plan.h"

static int failures = 0;
#define EXPECT(c, ...)                                       \
  do {                                                       \
    if (!(c)) {                                              \
      if (++failures <= 20) {                                \
        std::printf("FAILED line %d: %s  [", __LINE__, #c);  \
        std::printf(__VA_ARGS__);                            \
        std::printf("]\n");                                  \
      }                                                      \
    }                                                        \
  } while (0)

// section bits of an item's mode: 1 message path, 2 left BondFFN, 8 right BondFFN, 4 owner of the He' store
static const int BITS[4] = {1, 2, 8, 4};
// cost of the item of a split round, with the unit costs of mdx_plan.h: message path incl. edge_embs 0.72, left BondFFN 0.13, right
// BondFFN 0.15, edge_embs recomputed by an item without the message path 0.03
static double mode_cost(int mode) {
  return (mode & 1 ? 0.72 : 0.03) + (mode & 2 ? 0.13 : 0.0) + (mode & 8 ? 0.15 : 0.0);
}

struct Cover {  // how often each unit received each section bit
  std::vector<int> n[4];
  explicit Cover(int units) {
    for (auto& v : n) v.assign(units, 0);
  }
  bool add(int unit, int mode) {
    if (unit < 0 || unit >= (int)n[0].size() || (mode & ~15) || !mode) return false;
    for (int b = 0; b < 4; ++b) n[b][unit] += (mode & BITS[b]) ? 1 : 0;
    return true;
  }
  bool once() const {
    for (auto& v : n)
      for (int c : v)
        if (c != 1) return false;
    return true;
  }
};

static long plans_checked = 0, split1 = 0, split2 = 0;

static void check_plan(int nunits, int nslots, bool can_split) {
  const EdgePlan p = make_plan(nunits, nslots, can_split);
  ++plans_checked;
  split1 += p.split == 1, split2 += p.split == 2;
  EXPECT(p.nslots == nslots && p.nf * nslots + p.rem == nunits && p.rem >= 0 && p.rem < nslots, "%d %d", nunits, nslots);
  EXPECT(can_split || p.split == 0, "%d %d", nunits, nslots);
  EXPECT(p.split == 0 || (p.rem > 0 && p.m >= 1 && p.m <= (p.split == 1 ? 2 : 5) && (nslots - p.rem) * p.m >= p.rem), "%d %d", nunits, nslots);
  Cover cover(nunits);
  for (int slot = 0; slot < nslots; ++slot) {
    const int items = plan_items(p, slot);
    // the items plan_item serves this slot: the full rounds, then pieces of the last round while they name a unit of the batch and
    // stay inside the slot's share (one unit, or m units for a BondFFN slot of a split round)
    const int share = p.split && slot >= p.rem ? p.m : 1;
    int served = p.nf;
    for (int j = 0; j < share; ++j) {
      int mode = 0;
      if (plan_item(p, slot, p.nf + j, mode) >= nunits) break;
      ++served;
    }
    EXPECT(items == served, "units %d slots %d split %d slot %d: plan_items %d, plan_item serves %d", nunits, nslots, p.split, slot, items, served);
    double cost = 0;
    for (int it = 0; it < items; ++it) {
      int mode = 0;
      const int unit = plan_item(p, slot, it, mode);
      EXPECT(cover.add(unit, mode), "units %d slots %d split %d slot %d item %d -> unit %d mode %d", nunits, nslots, p.split, slot, it, unit, mode);
      EXPECT(it >= p.nf || mode == 15, "a full round is not cut");
      cost += it < p.nf ? 1.0 : mode_cost(mode);
    }
    if (p.split) EXPECT(cost <= p.nf + 1 + 1e-9, "units %d slots %d split %d m %d slot %d costs %.2f", nunits, nslots, p.split, p.m, slot, cost);
  }
  EXPECT(cover.once(), "units %d slots %d split %d m %d: a section of a unit is computed twice or never", nunits, nslots, p.split, p.m);
}

// slots a wave of kernel B / the backward takes its range by (XCD-contiguous), and linear_rows' plain ones
static void check_static_range(int nunits, int grid) {
  const int nslots = 4 * grid;
  for (int remap = 0; remap < 2; ++remap) {
    std::vector<int> n(nunits, 0);
    bool ok = true;
    for (int b = 0; b < grid; ++b)
      for (int wave = 0; wave < 4; ++wave) {
        const int slot = (remap ? xcd_remap(b, grid) : b) * 4 + wave;
        int ubeg, uend;
        static_range(nunits, nslots, slot, ubeg, uend);
        ok = ok && ubeg >= 0 && uend <= nunits;
        for (int u = ubeg; u < uend && ok; ++u) ++n[u];
      }
    EXPECT(ok && std::all_of(n.begin(), n.end(), [](int c) { return c == 1; }), "units %d grid %d remap %d", nunits, grid, remap);
  }
}

int main() {
  // ---- static plan and equal split ----
  std::vector<int> slots;
  for (int s = 4; s <= 64; s += 4) slots.push_back(s);
  slots.push_back(1024);
  slots.push_back(2048);
  for (int nslots : slots) {
    const bool thin = nslots > 64;
    for (int nunits = 1; nunits <= 6 * nslots; ++nunits) {
      if (thin) {
        // every boundary of make_plan in rem / nslots (0, 1/2, 2/3, 3/4, 4/5, 5/6, 1) with its neighbours, and every 37th count
        const int rem = nunits % nslots;
        bool near = nunits % 37 == 0;
        for (int k = 0; k <= 6 && !near; ++k) {
          const int edge = k == 0 ? 0 : k == 6 ? nslots : nslots * k / (k + 1);
          near = rem >= edge - 3 && rem <= edge + 3;
        }
        if (!near) continue;
      }
      check_plan(nunits, nslots, true);
      check_plan(nunits, nslots, false);
      check_static_range(nunits, nslots / 4);
    }
  }
  EXPECT(split1 > 100 && split2 > 100, "%ld %ld", split1, split2);
  // the boundaries themselves, on 24 slots: rem 12 -> split 1 m 1, 16 -> m 2, 17 -> split 2 m 3, 19 -> m 4, 20 -> m 5, 21 -> none
  {
    const int rem[6] = {12, 16, 17, 19, 20, 21}, split[6] = {1, 1, 2, 2, 2, 0}, m[6] = {1, 2, 3, 4, 5, 0};
    for (int i = 0; i < 6; ++i) {
      const EdgePlan p = make_plan(48 + rem[i], 24, true);
      EXPECT(p.nf == 2 && p.rem == rem[i] && p.split == split[i] && p.m == m[i], "rem %d: split %d m %d", rem[i], p.split, p.m);
    }
  }

  // ---- work-queue item map of edge kernel A ----
  for (int waves = 4; waves <= 8; waves += 4)
    for (int cnt = 0; cnt <= 40; ++cnt) {
      const int nt = std::min(cnt, waves * 10 >> 3);
      EXPECT(wq_tail(cnt, waves, EA_WQ_TAIL8) == nt, "cnt %d waves %d", cnt, waves);
      Cover cover(cnt);
      for (int i = 0; i < cnt + nt; ++i) {
        int mode = 0;
        const int unit = wq_item(i, cnt, nt, mode);
        EXPECT(cover.add(unit, mode), "cnt %d nt %d item %d -> unit %d mode %d", cnt, nt, i, unit, mode);
      }
      EXPECT(cover.once(), "cnt %d nt %d", cnt, nt);
      // without a tail (kernels that are not cut by section) the list is the units themselves
      for (int i = 0; i < cnt; ++i) {
        int mode = 0;
        EXPECT(wq_item(i, cnt, 0, mode) == i && mode == 15, "cnt %d item %d", cnt, i);
      }
    }

  // ---- pairs of the work queue ----
  const int cus[4] = {1, 2, 3, 256};
  for (int ncus : cus)
    for (int grid = 1; grid <= 600; ++grid) {
      const int counts[] = {1, grid - 1, grid, grid + 1, 4 * grid - 3, 4 * grid, 4 * grid + 1, 7 * grid + 5, 40 * grid + 3};
      for (int nunits : counts) {
        if (nunits < 1) continue;
        const WorkQ w = make_workq(nullptr, nunits, grid, ncus);
        EXPECT(w.npairs == std::min(std::min(grid, ncus), MDX_WQ_PAIRS) && w.nunits == nunits, "grid %d cus %d", grid, ncus);
        std::vector<std::pair<int, int>> ranges;
        long waves = 0;
        for (int p = 0; p < w.npairs; ++p) {
          int beg, end;
          wq_range(w, xcd_remap(p, w.npairs), beg, end);
          ranges.emplace_back(beg, end);
          const int wv = wq_waves(w, 4, (unsigned)grid, p);
          EXPECT(wv >= 4 && wv % 4 == 0, "grid %d cus %d pair %d waves %d", grid, ncus, p, wv);
          waves += wv;
        }
        // the workgroups b with b % npairs == p are the pair's
        std::sort(ranges.begin(), ranges.end());
        int at = 0;
        bool ok = true;
        for (auto& r : ranges) {
          ok = ok && r.first == at && r.second >= r.first;
          at = r.second;
        }
        EXPECT(ok && at == nunits, "units %d grid %d cus %d: the pairs' ranges do not partition the units", nunits, grid, ncus);
        EXPECT(waves == 4L * grid, "units %d grid %d cus %d: %ld waves", nunits, grid, ncus, waves);
      }
    }

  // ---- XCD remap ----
  for (int n = 1; n <= 600; ++n) {
    std::vector<int> seen(n, 0);
    bool ok = true;
    for (int b = 0; b < n; ++b) {
      const int t = xcd_remap(b, n);
      ok = ok && t >= 0 && t < n && !seen[t]++;
    }
    EXPECT(ok, "xcd_remap is no permutation of [0, %d)", n);
  }

  // ---- grid of a launch ----
  for (int ncus : cus)
    for (int wps = 1; wps <= 2; ++wps)
      for (int nunits = 1; nunits <= 5000; ++nunits) {
        const int grid = row_owner_grid(nunits, ncus, wps);
        EXPECT(grid >= 1 && grid <= ncus * wps && (4 * grid >= nunits || grid == ncus * wps) && 4 * (grid - 1) < nunits, "%d %d %d", nunits, ncus, wps);
      }

  if (failures) std::printf("%d FAILED\n", failures);
  else std::printf("work_plan_host_check ok (%ld plans)\n", plans_checked);
  return failures != 0;
}
