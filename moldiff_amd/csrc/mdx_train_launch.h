// Host-side helpers shared by the two files of the layer-level training operators (mdx_train.hip: contractions and reductions;
// mdx_train_rows.hip: row operators).  The inlines are static: each file gets its own copy and nothing here is a symbol of the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>

#include "../../include/moldiff_hip.h"

int mdx_set_error(int code, const char* msg);  // mdx_api.hip

// out (M x N, ld) = bias + sum over the S partial copies in P; more than RED_CHUNK copies go through `scratch`
// (ceil(S / RED_CHUNK) * M * N floats) in two fixed-order stages.  rkind: round_kind of the sum.  Defined in mdx_train.hip; internal to
// the library (hidden: not an exported symbol).
__attribute__((visibility("hidden"))) void launch_reduce_partials(const float* P, int S, int M, int N, const float* bias, float* out, int ld,
                                                                  float* scratch, hipStream_t s, int rkind = 0);

static inline unsigned nblk(size_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }
static inline int bad(const char* m) { return mdx_set_error(MDX_ERR_ARG, m); }
static inline int launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDX_OK : mdx_set_error(MDX_ERR_HIP, hipGetErrorString(e));
}
// A run-time integer as a template argument: calls f(std::integral_constant<int, V>{}) for the V among Vs that equals v; false if none does.
template <int... Vs, class F>
static inline bool pick(int v, F&& f) {
  return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
