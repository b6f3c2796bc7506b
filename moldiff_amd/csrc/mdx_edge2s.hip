// Split-precision build of the row-owner edge kernel A (gfx950) -- round 4, opt-in (mdx_model_set_matrix_path(m, 1)).
//
// The kernel's text is mdx_edge2_body.h, shared with the exact build (mdx_edge2.hip): same sections, work decomposition, argument
// block and outputs.  This file binds it to v_mfma_f32_16x16x32_f16 with operands split into float16 hi / lo halves (mdx_split.h:
// three products per k-group, fp32 accumulation, ~22 significand bits per operand) and to the split stream packs.
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
#define MDX_RING 8  // half-steps of 2 KiB in flight per wave
#endif
#include "mdx_row.h"
#ifndef MDX_SPLIT_SEAMLESS
#define MDX_SPLIT_SEAMLESS 1  // the weight ring runs through GEMM boundaries (mdx_split.h)
#endif
#include "mdx_split.h"
#include "mdx_edge2_plan.h"
#include "../../include/moldiff_hip.h"
#include <algorithm>
int mdx_set_error(int code, const char* msg);

// phase trace of the split kernel (tools/trace_edge2s.py; build with EXTRA=-DMDX_TRACE2S): the body's stamps, one 48-slot record
// per work item; compiled out of the library
#ifdef MDX_TRACE2S
__device__ unsigned long long* mdx_trace2s_buf = nullptr;
extern "C" int mdx_debug_set_trace2s(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(mdx_trace2s_buf), &p, sizeof(p)); }
#define STAMP(i)                                                                                                            \
  do {                                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                                      \
    if (lane == 0 && mdx_trace2s_buf) mdx_trace2s_buf[(size_t)unit * 48 + (i)] = ((i) >= 46) ? wall_clock64() : clock64();  \
    __builtin_amdgcn_sched_barrier(0);                                                                                      \
  } while (0)
#else
#define STAMP(i) ((void)0)
#endif

namespace {
#define E2_KERNEL edge_a2s_kernel
#define E2_S ss
#define E2_GEMM(KT, FT) rgemm_s<((KT) + 1) / 2, FT>
#define E2_X(KT, x) XS<((KT) + 1) / 2> x
#define E2_OPERAND(KT, x, y) E2_X(KT, x); to_xs<KT>(x, y)
#include "mdx_edge2_body.h"
}  // namespace

// same dispatch contract as launch_edge_a2 (flags without EA_SPLIT)
RowOwnerShape shape_edge_a2s() { return {ROWS, MDX_WPS}; }  // rows per unit and workgroups per CU of this build (mdx_debug_launch_units_host)

int launch_edge_a2s(const EdgeAArgs& a, hipStream_t s) {
  if (a.E <= 0) return MDX_OK;
  switch (a.flags & ~EA_SPLIT) {
    case EA_EMB | EA_NODE | EA_FFN | EA_AGG: launch_a2<EA_EMB | EA_NODE | EA_FFN | EA_AGG>(a, s); return MDX_OK;
    case EA_EMB | EA_NODE | EA_FFN | EA_AGG | EA_TAPE | EA_TAPE_FFN:
      launch_a2<EA_EMB | EA_NODE | EA_FFN | EA_AGG | EA_TAPE | EA_TAPE_FFN>(a, s); return MDX_OK;
    default: return mdx_set_error(MDX_ERR_UNSUPPORTED, "split-precision edge kernel A: unsupported section flags");
  }
}
