// Host and device helpers of the row-owner edge kernel A (mdx_edge2_body.h; exact build mdx_edge2.hip, split build mdx_edge2s.hip):
// the LDS constant budget and the one-unit-ahead prologue loads.  The static work plan with its section-cut tail and the
// work-queue item map are in mdx_plan.h.
#pragma once
#include "mdx_kernels.h"
#include "mdx_row.h"

namespace {

constexpr int EA_CONST_FLOATS = 96 + 2560 + 2 * 640;

// (EdgePlan, make_plan, plan_items, plan_item, WorkQA and wq_item are plain integer logic: mdx_plan.h)

// rows of the He tile + edge length of one unit: loaded one unit ahead by the persistent loop
struct Prolog {
  RowTile t;
  f32x4 x[4][RR];
  float d[RR];
};

__device__ __forceinline__ void prolog_rows(Prolog& p, const EdgeAArgs& a, int q) {
  row_gather<4, RR>(p.x, a.He_in, p.t.row, 64, q);
  if (a.flags & EA_EMB) {
#pragma unroll
    for (int rt = 0; rt < RR; ++rt) {
      if (a.dist_in) {
        p.d[rt] = a.dist_in[p.t.row[rt]];
      } else {
        const float dx = a.pos[3 * p.t.li[rt] + 0] - a.pos[3 * p.t.ri[rt] + 0];
        const float dy = a.pos[3 * p.t.li[rt] + 1] - a.pos[3 * p.t.ri[rt] + 1];
        const float dz = a.pos[3 * p.t.li[rt] + 2] - a.pos[3 * p.t.ri[rt] + 2];
        p.d[rt] = sqrtf(dx * dx + dy * dy + dz * dz);
      }
    }
  }
}

}  // namespace
