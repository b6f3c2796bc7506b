// Row-owner edge kernel A of one NodeEdgeNet block (gfx950), exact fp32 build: edge_a2_kernel.  The kernel's text and design notes
// are mdx_edge2_body.h (shared with the split float16 build, mdx_edge2s.hip); this file binds it to v_mfma_f32_16x16x4_f32 (rgemm,
// mdx_row.h) and the fp32 stream packs, and holds the dispatch over the section flags.
#include "mdx_kernels.h"
#ifndef MDX_RING
#define MDX_RING 4  // weight-ring depth in steps (kernel A: 4.65 / 4.58 / 4.56 ms per step at depth 2 / 3 / 4)
#endif
#include "mdx_row.h"
#include "mdx_edge2_plan.h"
#include "../../include/moldiff_hip.h"
#include <algorithm>
int mdx_set_error(int code, const char* msg);

// Phase trace (tools/trace_edge2.py; build with EXTRA=-DMDX_TRACE2): lane 0 of every wave stamps the shader clock at each
// phase boundary into a 48-slot record per unit (slot 46/47: 100 MHz wall clock at entry/exit).  Compiled out of the library.
#ifdef MDX_TRACE2
__device__ unsigned long long* mdx_trace2_buf = nullptr;
__device__ int mdx_trace2_sel = 0;  // 0: edge_a2, 1: edge_b2
extern "C" int mdx_debug_set_trace2(void* p, int which) {
  hipMemcpyToSymbol(HIP_SYMBOL(mdx_trace2_sel), &which, sizeof(which));
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(mdx_trace2_buf), &p, sizeof(p));
}
#define STAMP_K(k, i)                                                                                       \
  do {                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
    if (lane == 0 && mdx_trace2_buf && mdx_trace2_sel == (k))                                               \
      mdx_trace2_buf[(size_t)unit * 48 + (i)] = ((i) >= 46) ? wall_clock64() : clock64();                   \
    __builtin_amdgcn_sched_barrier(0);                                                                      \
  } while (0)
#else
#define STAMP_K(k, i) ((void)0)
#endif
#define STAMP(i) STAMP_K(0, i)

namespace {
#define E2_KERNEL edge_a2_kernel
#define E2_S s
#define E2_GEMM(KT, FT) rgemm<KT, FT, RR>
#define E2_X(KT, x) f32x4 x[KT][RR]
#define E2_OPERAND(KT, x, y) auto& x = y
#include "mdx_edge2_body.h"
}  // namespace

RowOwnerShape shape_edge_a2() { return {ROWS, MDX_WPS}; }  // rows per unit and workgroups per CU of this build (mdx_debug_launch_units_host)

int launch_edge_a2(const EdgeAArgs& a, hipStream_t s) {
  if (a.E <= 0) return MDX_OK;
  switch (a.flags) {
    case EA_EMB | EA_NODE | EA_FFN | EA_AGG: launch_a2<EA_EMB | EA_NODE | EA_FFN | EA_AGG>(a, s); return MDX_OK;  // product path
    case EA_EMB | EA_NODE | EA_FFN | EA_AGG | EA_TAPE | EA_TAPE_FFN:
      launch_a2<EA_EMB | EA_NODE | EA_FFN | EA_AGG | EA_TAPE | EA_TAPE_FFN>(a, s); return MDX_OK;                     // + BondFFN tape
    case EA_NODE: launch_a2<EA_NODE>(a, s); return MDX_OK;                                    // NodeBlock.forward
    case EA_FFN: launch_a2<EA_FFN>(a, s); return MDX_OK;                                      // EdgeBlock.forward
    default: return mdx_set_error(MDX_ERR_UNSUPPORTED, "edge kernel A: unsupported section flags");
  }
}

// the entry point the host API uses: this build or, with EA_SPLIT in the flags, the split float16 build (mdx_edge2s.hip)
int launch_edge_a(const EdgeAArgs& a, hipStream_t s) {
  if (a.E <= 0) return MDX_OK;
  return (a.flags & EA_SPLIT) ? launch_edge_a2s(a, s) : launch_edge_a2(a, s);
}
