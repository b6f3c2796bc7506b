// Row-owner edge kernel B of one NodeEdgeNet block (gfx950), exact fp32 build: edge_b2_kernel.  The kernel's text is
// mdx_edge2b_body.h (shared with the split float16 build, mdx_edge2bs.hip); this file binds it to v_mfma_f32_16x16x4_f32 (rgemm,
// mdx_row.h) and the fp32 stream packs, and holds the dispatch over the section flags.
#include "mdx_kernels.h"
#ifndef MDX_RING
#define MDX_RING 4  // weight-ring depth in steps (kernel B: 1.743 / 1.727 / 1.723 ms per step at depth 2 / 3 / 4)
#endif
#include "mdx_row.h"
#include "../../include/moldiff_hip.h"
#include <algorithm>
int mdx_set_error(int code, const char* msg);

// phase trace, see mdx_edge2.hip (tools/trace_edge2.py b); compiled out of the library
#ifdef MDX_TRACE2
__device__ unsigned long long* mdx_trace2b_buf = nullptr;
extern "C" int mdx_debug_set_trace2b(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(mdx_trace2b_buf), &p, sizeof(p)); }
#define STAMPB(i)                                                                                           \
  do {                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    if (lane == 0 && mdx_trace2b_buf) mdx_trace2b_buf[(size_t)unit * 48 + (i)] = ((i) >= 46) ? wall_clock64() : clock64(); \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
  } while (0)
#else
#define STAMPB(i) ((void)0)
#endif

namespace {
#define E2_KERNEL edge_b2_kernel
#define E2_S s
#define E2_GEMM(KT, FT) rgemm<KT, FT, RR>
#define E2_X(KT, x) f32x4 x[KT][RR]
#define E2_OPERAND(KT, x, y) auto& x = y
#define E2_PUT_PAIR(x, ftp, xb, xn)             \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) \
    _Pragma("unroll") for (int rt = 0; rt < RR; ++rt) x[2 * (ftp) + j][rt] = xb[j][rt] * xn[j][rt]
#include "mdx_edge2b_body.h"
}  // namespace

RowOwnerShape shape_edge_b2() { return {ROWS, MDX_WPS}; }  // rows per unit and workgroups per CU of this build (mdx_debug_launch_units_host)

int launch_edge_b2(const EdgeBArgs& a, hipStream_t s) {
  if (a.E <= 0) return MDX_OK;
  switch (a.flags) {
    case EB_EDGE | EB_POS: launch_b2<EB_EDGE | EB_POS>(a, s); return MDX_OK;      // MolDiff denoiser
    case EB_EDGE: launch_b2<EB_EDGE>(a, s); return MDX_OK;                        // bond predictor (update_pos = False)
    case EB_EDGE | EB_DELTA: launch_b2<EB_EDGE | EB_DELTA>(a, s); return MDX_OK;  // EdgeBlock.forward
    case EB_POS: launch_b2<EB_POS>(a, s); return MDX_OK;                          // PosUpdate.forward
    default: return mdx_set_error(MDX_ERR_UNSUPPORTED, "edge kernel B: unsupported section flags");
  }
}

int launch_edge_b(const EdgeBArgs& a, hipStream_t s) {
  if (a.E <= 0) return MDX_OK;
  return (a.flags & EB_SPLIT) ? launch_edge_b2s(a, s) : launch_edge_b2(a, s);
}
