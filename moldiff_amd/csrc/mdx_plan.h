// Index maps of the persistent row-owner kernels (mdx_edge2_body.h, mdx_edge2b_body.h, mdx_bwd2_body.h, mdx_linear_rows.hip): which
// units a wave ("slot") computes and which sections of them.  Pure integer logic and plain C++: the kernels and their launchers
// include it through mdx_tile.h / mdx_row.h / mdx_edge2_plan.h, and tools/work_plan_host_check.cpp builds it on its own with a host
// compiler and enumerates it (every unit exactly once, every section bit exactly once).
#pragma once
#include <algorithm>

#if defined(__HIPCC__)
#define MDX_HD __host__ __device__ __forceinline__
#else
#define MDX_HD inline
#endif

// Grid of a row-owner launch: one wave per unit, four waves per workgroup, at most `wps` workgroups per CU (the waves per SIMD the
// kernel is compiled for); beyond that the waves are persistent and loop over their units.
inline int row_owner_grid(int nunits, int ncus, int wps) { return std::min((nunits + 3) / 4, ncus * wps); }

// XCD-aware tile remap (MI355X: 8 XCDs, block b is dispatched to XCD b % 8): give every XCD a
// contiguous range of tiles so neighbouring tiles (same molecule -> same node rows) share an L2.
// Bijective for any ntiles.
MDX_HD int xcd_remap(int bid, int ntiles) {
  const int q = ntiles >> 3, r = ntiles & 7;
  const int xcd = bid & 7, k = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + k;
}

// Static equal split of kernel B, the guidance backward and linear_rows: slot s owns the contiguous range [ubeg, uend) of
// per = ceil(nunits / nslots) units (empty for the last slots when nunits is small).
MDX_HD void static_range(int nunits, int nslots, int slot, int& ubeg, int& uend) {
  const int per = (nunits + nslots - 1) / nslots;
  ubeg = slot * per;
  uend = nunits < ubeg + per ? nunits : ubeg + per;
}

// ---- static plan of edge kernel A ---------------------------------------------------------------------------------------
// Work list of a persistent wave ("slot"): nf full units (a contiguous range), then its share of the last, partial round.
// When the last round is short and the kernel runs both sections, that round is cut by SECTION instead of by rows (a
// 16-row MFMA tile cannot be split further).  Unit costs measured with tools/trace_edge2.py (fractions of a unit): message path
// incl. edge_embs 0.72, left BondFFN 0.13, right BondFFN 0.15 (with its in-kernel segment sum), edge_embs recomputed by a slot
// that only runs BondFFNs 0.03.  Two cuts:
//   split 1: the first `rem` slots run the message path of one unit each (0.72), the other slots both BondFFNs of `m` <= 2 units
//            each (0.31 m);
//   split 2: the first `rem` slots run the message path AND the right BondFFN of one unit each (0.87), the other slots the left
//            BondFFN of `m` <= 5 units each (0.16 m)   -- covers rem up to 5/6 of the slots (split 1 with m = 3 would take 0.93).
struct EdgePlan {
  int nslots, nf, rem, split, m;
};
MDX_HD int plan_items(const EdgePlan& p, int slot) {
  if (!p.split) return p.nf + (slot < p.rem ? 1 : 0);
  if (slot < p.rem) return p.nf + 1;
  const int k = slot - p.rem, left = p.rem - k * p.m;
  return p.nf + (left < 0 ? 0 : left < p.m ? left : p.m);
}
// item it of a slot -> unit index; mode bits: 1 message path, 2 left BondFFN, 8 right BondFFN, 4 this item owns the He' store
MDX_HD int plan_item(const EdgePlan& p, int slot, int it, int& mode) {
  if (it < p.nf) {
    mode = 15;
    return slot * p.nf + it;
  }
  const int base = p.nf * p.nslots;
  if (!p.split || slot < p.rem) {
    mode = p.split == 0 ? 15 : p.split == 1 ? 5 : 13;
    return base + slot;
  }
  mode = p.split == 1 ? 10 : 2;
  return base + (slot - p.rem) * p.m + (it - p.nf);
}
inline EdgePlan make_plan(int nunits, int nslots, bool can_split) {
  EdgePlan p{nslots, nunits / nslots, nunits % nslots, 0, 0};
  if (can_split && p.rem > 0 && p.rem < nslots) {
    const int m = (p.rem + (nslots - p.rem) - 1) / (nslots - p.rem);
    if (m <= 2) {
      p.split = 1;
      p.m = m;
    } else if (m <= 5) {
      p.split = 2;
      p.m = m;
    }
  }
  return p;
}

// ---- per-pair work queue (mdx_row.h: why pairs, how the counters are kept) -----------------------------------------------
constexpr int MDX_WQ_STRIDE = 32;  // ints per pair: [0] next unit (relative to the pair's first), [1] waves that have left
struct WorkQ {
  int* ctr;     // MDX_WQ_PAIRS lines of MDX_WQ_STRIDE ints; nullptr: static split
  int npairs;   // min(grid, #CUs): workgroup b belongs to pair b % npairs
  int nunits;
};
constexpr int MDX_WQ_PAIRS = 512;  // lines per counter set (>= #CUs)

inline WorkQ make_workq(int* ctr, int nunits, int grid, int ncus) {
  WorkQ w{};
  w.npairs = std::max(1, std::min(std::min(grid, ncus), MDX_WQ_PAIRS));
  w.ctr = ctr;
  w.nunits = nunits;
  return w;
}
// unit range [beg, end) of the pair whose XCD-ordered index is ri = xcd_remap(p, npairs): the nunits % npairs first ranges are one longer
MDX_HD void wq_range(const WorkQ& w, int ri, int& beg, int& end) {
  const int q = w.nunits / w.npairs, r = w.nunits % w.npairs;
  beg = ri * q + (ri < r ? ri : r);
  end = beg + q + (ri < r ? 1 : 0);
}
// waves of pair p: wg_waves per workgroup, the workgroups b of the grid with b % npairs == p
MDX_HD int wq_waves(const WorkQ& w, unsigned wg_waves, unsigned grid, int p) {
  return wg_waves * (grid / w.npairs + (p < (int)(grid % w.npairs) ? 1 : 0));
}

// Work queue of edge kernel A: a pair of workgroups hands out its units in order; the last few of them (tail8 eighths of a unit per
// wave) are cut by section so that the waves, which arrive at the end of the list up to one unit apart, finish close together:
// first the message-path halves of those units (0.72 of a unit), then their BondFFN halves (0.31).  Largest pieces first: the
// spread at the end is bounded by the smallest piece.
struct WorkQA {
  WorkQ q;
  int tail8;
};
constexpr int EA_WQ_TAIL8 = 10;  // measured: none 6.99 ms per step, 8 eighths 6.92, 10 6.91, 16 7.01
// units cut at the end of a pair's list of cnt units
MDX_HD int wq_tail(int cnt, int waves, int tail8) {
  const int nt = waves * tail8 >> 3;
  return cnt < nt ? cnt : nt;
}
// item i of a pair's list of cnt units, the last nt of them cut -> unit (relative to the pair's first) and mode
MDX_HD int wq_item(int i, int cnt, int nt, int& mode) {
  if (i < cnt) {
    mode = i < cnt - nt ? 15 : 5;
    return i;
  }
  mode = 10;
  return i - nt;
}
