// Typed access to the tensors of the training operators (mdx_train.hip, mdx_train_rows.hip): a tensor is stored as fp32 (h = 0) or as
// float16 (h = 1; the mixed-precision mode keeps every Linear / LayerNorm / product result -- float16 VALUES anyway -- in float16
// containers).  The flag is wave-uniform, one scalar branch per access; offsets are in elements; arithmetic is always fp32.
//   ldv<W>(t, i)      W consecutive elements from element i:  W = 1 float, W = 4 f32x4 (16 bytes of fp32 / 8 of float16),
//                     W = 8 f32x8 from ONE 16-byte float16 load (float16 containers only; there is no 8-wide store)
//   stv<W>(t, i, v)   W = 1, 4: converts to the container on the way out (round to nearest even)
// The vector forms need naturally aligned rows (tp_vec_ok; the 8-wide load 16 bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdx_tile.h"

typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
struct TP {
  const void* p;
  int h;
};
struct TPW {
  void* p;
  int h;
};
__host__ __device__ inline bool tp_vec_ok(const void* p, int h, int ld) {  // rows of 4 elements are naturally aligned
  return ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(p) & (h ? 7 : 15)) == 0);
}

// W lanes of fp32 values
template <int W>
struct TVec;
template <>
struct TVec<1> {
  typedef float type;
};
template <>
struct TVec<4> {
  typedef f32x4 type;
};
template <>
struct TVec<8> {
  typedef f32x8 type;
};
template <int W>
using tvec_t = typename TVec<W>::type;

template <int W>
__device__ __forceinline__ tvec_t<W> ldv(const TP& t, size_t i) {
  if constexpr (W == 1) {
    return t.h ? (float)reinterpret_cast<const _Float16*>(t.p)[i] : reinterpret_cast<const float*>(t.p)[i];
  } else if constexpr (W == 4) {
    if (t.h) {
      const f16x4_t v = *reinterpret_cast<const f16x4_t*>(reinterpret_cast<const _Float16*>(t.p) + i);
      f32x4 r = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
      return r;
    }
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(t.p) + i);
  } else {
    static_assert(W == 8, "ldv: W is 1, 4 or 8");
    // PRECONDITION: t.h == 1 and 16-byte alignment -- t.h is not looked at, an fp32 tensor would be read as float16 (the one caller,
    // mdx_op_segsum_rows_t, takes W = 8 for float16 rows only)
    const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(t.p) + i);
    const f16x4_t lo = __builtin_bit_cast(f16x4_t, uint2{u.x, u.y}), hi = __builtin_bit_cast(f16x4_t, uint2{u.z, u.w});
    f32x8 r = {(float)lo[0], (float)lo[1], (float)lo[2], (float)lo[3], (float)hi[0], (float)hi[1], (float)hi[2], (float)hi[3]};
    return r;
  }
}
template <int W>
__device__ __forceinline__ void stv(const TPW& t, size_t i, tvec_t<W> v) {
  if constexpr (W == 1) {
    if (t.h) reinterpret_cast<_Float16*>(t.p)[i] = (_Float16)v;
    else reinterpret_cast<float*>(t.p)[i] = v;
  } else {
    static_assert(W == 4, "stv: W is 1 or 4");
    if (t.h) {
      f16x4_t r = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
      *reinterpret_cast<f16x4_t*>(reinterpret_cast<_Float16*>(t.p) + i) = r;
    } else {
      *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(t.p) + i) = v;
    }
  }
}
__device__ __forceinline__ f32x4 lo4(f32x8 v) { return __builtin_shufflevector(v, v, 0, 1, 2, 3); }
__device__ __forceinline__ f32x4 hi4(f32x8 v) { return __builtin_shufflevector(v, v, 4, 5, 6, 7); }

// A value rounded to the low-precision type of the mixed-precision modes and back (round to nearest even; a float16 overflows to
// infinity): HT = 0 bfloat16, 1 float16.  round_kind is the run-time form: kind 0 = keep fp32, 1 = bfloat16, 2 = float16.
__device__ __forceinline__ uint16_t to_bf16(float a) {
  uint32_t u = __float_as_uint(a);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
template <int HT>
__device__ __forceinline__ float round_half(float a) {
  if constexpr (HT == 1) return (float)(_Float16)a;
  else return __uint_as_float((uint32_t)to_bf16(a) << 16);
}
__device__ __forceinline__ float round_kind(float a, int kind) { return kind == 2 ? round_half<1>(a) : kind == 1 ? round_half<0>(a) : a; }
