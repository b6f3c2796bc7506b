// Split-precision build of the row-owner edge kernel B (gfx950) -- round 4, opt-in; see mdx_edge2s.hip / mdx_split.h.
// The kernel's text is mdx_edge2b_body.h, shared with the exact build (mdx_edge2b.hip): same argument block, work decomposition
// and outputs; this file binds it to the split float16 GEMMs (rgemm_s) and the split stream packs.
#include "mdx_kernels.h"
// Decomposition of the split build (measured on the bench workload, ms per sampling step, kernel A / kernel B): 16 rows x 2 waves per
// SIMD like the exact kernels 2.80 / 0.96 -- there the per-wave weight stream (the same bytes as fp32, 11.9 GB per kernel-A launch)
// runs at the L1/L2 limit (~25 TB/s) and IS the kernel time; 32 rows x 1 wave (every weight fragment feeds two row tiles: half the
// stream) 2.46 / 0.83 with a ring of 4 half-steps, 2.30 / 0.82 with 8 (a lone wave per SIMD has only its own prefetch depth to
// cover the L2 latency).  The exact fp32 kernels measured the other way round (4.66 vs 4.97 ms): they are bound by the matrix pipe.
#ifndef MDX_RR
#define MDX_RR 2
#endif
#ifndef MDX_WPS
#define MDX_WPS 1
#endif
#ifndef MDX_RING
#define MDX_RING 4  // half-steps of 2 KiB in flight per wave (seamless: 133.0 us per launch; 8: 135.5; the primed ring of 8: 135.6)
#endif
#ifndef MDX_SPLIT_SEAMLESS
#define MDX_SPLIT_SEAMLESS 1  // the weight ring runs through GEMM boundaries (mdx_split.h); at 4 half-steps no GEMM of this kernel idles
#endif
#include "mdx_row.h"
#include "mdx_split.h"
#include "../../include/moldiff_hip.h"
#include <algorithm>
int mdx_set_error(int code, const char* msg);

#define STAMPB(i) ((void)0)

namespace {
#define E2_KERNEL edge_b2s_kernel
#define E2_S ss
#define E2_GEMM(KT, FT) rgemm_s<((KT) + 1) / 2, FT>
#define E2_X(KT, x) XS<((KT) + 1) / 2> x
#define E2_OPERAND(KT, x, y) E2_X(KT, x); to_xs<KT>(x, y)
#define E2_PUT_PAIR(x, ftp, xb, xn)                                \
  _Pragma("unroll") for (int rt = 0; rt < RR; ++rt)                \
    _Pragma("unroll") for (int t = 0; t < 8; ++t) {                \
      const float v = xb[t / 4][rt][t % 4] * xn[t / 4][rt][t % 4]; \
      const _Float16 h = (_Float16)v;                              \
      x.hi[ftp][rt][t] = h;                                        \
      x.lo[ftp][rt][t] = (_Float16)((v - (float)h) * MDX_LO_UP);   \
    }
#include "mdx_edge2b_body.h"
static_assert(EB_PAIR_FLOATS == split_stream_pair_floats(64), "pair stride of the split Wbl / Wnl packs");
}  // namespace

RowOwnerShape shape_edge_b2s() { return {ROWS, MDX_WPS}; }  // rows per unit and workgroups per CU of this build (mdx_debug_launch_units_host)

int launch_edge_b2s(const EdgeBArgs& a, hipStream_t s) {
  if (a.E <= 0) return MDX_OK;
  switch (a.flags & ~EB_SPLIT) {
    case EB_EDGE | EB_POS: launch_b2<EB_EDGE | EB_POS>(a, s); return MDX_OK;
    case EB_EDGE: launch_b2<EB_EDGE>(a, s); return MDX_OK;
    default: return mdx_set_error(MDX_ERR_UNSUPPORTED, "split-precision edge kernel B: unsupported section flags");
  }
}
