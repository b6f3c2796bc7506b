// Layer-level operators of the training path (gfx950): every O(rows x features) piece of the loss forward/backward
// (reference models/model.py:128-201 get_loss + torch.autograd) as an explicit forward/backward kernel pair, driven one
// layer at a time from moldiff_amd/train_ops.py and csrc/mdx_fast.cpp.  Unlike the sampling path these are NOT fused across
// layers (the fused training kernels are in mdx_train_fused.hip): activations live in HBM between operators so that every
// parameter gradient is a plain contraction over stored tensors.  Three precisions share the file: exact fp32 (contractions on
// v_mfma_f32_16x16x4_f32), and bfloat16 / float16 operands with fp32 accumulation (v_mfma_f32_16x16x32_*), the float16 mode also
// with float16 CONTAINERS (`_t` entry points: a bit mask names the tensors stored as float16).
//
//   sgemm_nt / xgemm_nt     C[M,N] = A[M,K] B[N,K]^T + bias + addend: forward of nn.Linear and dgrad (B = W^T).  fp32 tiled kernel;
//                           half tiled kernel (hgemm_nt_kernel, 64- or 128-wide column tile); row-owner kernel for float16 rows with
//                           the whole weight in LDS (hgemm_nt_rows_kernel), optionally with the LayerNorm(+ReLU) that follows (xgemm_nt_ln)
//   sgemm_tn / xgemm_tn     dW[N,K] = G[M,N]^T X[M,K] (+ db = column sums of G) over split row ranges: fp32 kernel, converting half
//                           kernel (64 x 64 tiles), transpose-read kernel for float16 containers; partials summed in a fixed order
//   wgrad_grouped           a device table of queued weight gradients, one launch per tile class (classes: mdx_train_plan.h)
//   reduce_deferred         every split partial of a step (weights, biases, LayerNorm parameters) summed into the flat gradient buffer
//   transpose(_batch)       out[C,R] = in[R,C]^T: W^T for the dgrad GEMMs
//   colreduce               out[N] = sum_rows X (* Y): bias / LayerNorm-parameter gradients (two deterministic stages)
//   ln_relu                 y = relu(LN(x) * gamma + beta): forward (saves mean, rstd), backward (dx, partial rows of dgamma | dbeta)
//                           and the backward fused with a rank-1 Linear in front of it; generic fp32 kernels and 4-wide typed ones
//   ew, sum_n               add / sub / mul / a * sigmoid(b), forward and backward; sum of up to 12 tensors
//   gather / segsum, mul_gather, plan_flip      y = x[idx]; out[r] = sum_{j in seg r} src[order[j]] (each is the other's backward; no atomics)
//   edge_geom, smear, force                     rel / dist of an edge, Gaussian smearing, w * rel / d / (d + 1), with backwards
//   sumsq, adamw, amp_adamw                     gradient norm and the optimizer step (with the loss scaler's decision on the device)
//
// The host side's shared arithmetic -- split-partial layout, the queue's plan, LayerNorm partial rows, the deferred reduction's record
// table, the row-owner GEMM's shapes -- is in mdx_train_plan.h (plain C++, also built by the host compiler alone).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "../../include/moldiff_hip.h"
#include "mdx_tile.h"
#include "mdx_train_plan.h"

int mdx_set_error(int code, const char* msg);  // mdx_api.hip

namespace {

// ------------------------------------------------------------------------------------------------------------------
// SGEMM  C = A B^T: workgroup tile 128 rows x 64 features, K consumed in chunks of 32 through LDS; wave w owns rows
// 32w..32w+31 (2 row tiles) x all 64 features (4 feature tiles) -> acc[4][2].  Operand roles follow gemm_tile: the
// MFMA A-operand is the B matrix (features), the B-operand the A matrix (rows), so acc[ft][et][r] =
// C[row 16 et + c][feature 16 ft + 4 q + r] and stores are 16-byte vectors along the feature axis.
// gridDim.z > 1 = split-K: split z handles k in [z*kper, (z+1)*kper) and writes its partial to P[z][M][N].
// ------------------------------------------------------------------------------------------------------------------
constexpr int G_TM = 128, G_TN = 64, G_KC = 32, G_LD = G_KC + 8;

// Half storage (round 3): a tensor of the training operators is stored as fp32 (h = 0) or as float16 (h = 1; the mixed-precision
// mode keeps every Linear / LayerNorm / product result -- float16 VALUES anyway -- in float16 containers).  The flag is wave-uniform,
// one scalar branch per access; offsets are in elements.
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
struct TP {
  const void* p;
  int h;
};
struct TPW {
  void* p;
  int h;
};
__device__ __forceinline__ f32x4 ld4(const TP& t, size_t i) {
  if (t.h) {
    const f16x4_t v = *reinterpret_cast<const f16x4_t*>(reinterpret_cast<const _Float16*>(t.p) + i);
    f32x4 r = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    return r;
  }
  return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(t.p) + i);
}
__device__ __forceinline__ float ld1(const TP& t, size_t i) {
  return t.h ? (float)reinterpret_cast<const _Float16*>(t.p)[i] : reinterpret_cast<const float*>(t.p)[i];
}
__device__ __forceinline__ void st4(const TPW& t, size_t i, f32x4 v) {
  if (t.h) {
    f16x4_t r = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    *reinterpret_cast<f16x4_t*>(reinterpret_cast<_Float16*>(t.p) + i) = r;
  } else {
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(t.p) + i) = v;
  }
}
__device__ __forceinline__ void st1(const TPW& t, size_t i, float v) {
  if (t.h) reinterpret_cast<_Float16*>(t.p)[i] = (_Float16)v;
  else reinterpret_cast<float*>(t.p)[i] = v;
}
// 4 consecutive k-values of row `row_off` (element offset of the row), zero beyond K or outside the matrix
__device__ __forceinline__ f32x4 load4_guard_t(const TP& t, size_t row_off, int k, int K, bool row_ok, bool vec_ok) {
  if (!row_ok || k >= K) return splat4(0.f);
  if (vec_ok && k + 3 < K) return ld4(t, row_off + k);
  f32x4 v = splat4(0.f);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (k + j < K) v[j] = ld1(t, row_off + k + j);
  return v;
}
__host__ __device__ inline bool tp_vec_ok(const void* p, int h, int ld) {  // rows of 4 elements are naturally aligned
  return ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(p) & (h ? 7 : 15)) == 0);
}

__device__ __forceinline__ f32x4 load4_guard(const float* __restrict__ p, int k, int K, bool row_ok, bool vec_ok) {
  // 4 consecutive k-values of one row, zero beyond K or outside the matrix
  if (!row_ok || k >= K) return splat4(0.f);
  if (vec_ok && k + 3 < K) return ldg4(p + k);
  f32x4 v = splat4(0.f);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (k + j < K) v[j] = p[k + j];
  return v;
}

__global__ __launch_bounds__(256) void sgemm_nt_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                        const float* __restrict__ bias, const float* __restrict__ addend,
                                                        int ldd, float* __restrict__ C, int ldc, int M, int N, int K, int kper,
                                                        float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) float As[G_TM * G_LD];
  __shared__ __attribute__((aligned(16))) float Bs[G_TN * G_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.y * G_TM, n0 = blockIdx.x * G_TN;
  const int kbeg = blockIdx.z * kper, kend = min(K, kbeg + kper);
  const bool veca = ((lda & 3) == 0) && ((reinterpret_cast<uintptr_t>(A) & 15) == 0);
  const bool vecb = ((ldb & 3) == 0) && ((reinterpret_cast<uintptr_t>(B) & 15) == 0);
  f32x4 acc[4][2];
  acc_zero<4, 2>(acc);
  // tile slots of this thread (8 float4 per row): A 128 rows -> 4 slots, B 64 rows -> 2 slots; the next chunk's global
  // loads are issued before the MFMA block of the current one (register double buffering)
  f32x4 ra[4], rb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int slot = tid + 256 * j, row = slot >> 3, k4 = (slot & 7) * 4;
      const int gm = m0 + row;
      ra[j] = load4_guard(A + (size_t)gm * lda, k0 + k4, kend, gm < M, veca);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int slot = tid + 256 * j, row = slot >> 3, k4 = (slot & 7) * 4;
      const int gn = n0 + row;
      rb[j] = load4_guard(B + (size_t)gn * ldb, k0 + k4, kend, gn < N, vecb);
    }
  };
  if (kbeg < kend) fetch(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += G_KC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int slot = tid + 256 * j;
      sts4(As + (slot >> 3) * G_LD + (slot & 7) * 4, ra[j]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int slot = tid + 256 * j;
      sts4(Bs + (slot >> 3) * G_LD + (slot & 7) * 4, rb[j]);
    }
    __syncthreads();
    if (k0 + G_KC < kend) fetch(k0 + G_KC);
#pragma unroll
    for (int g = 0; g < G_KC / 16; ++g) {
      f32x4 a[4], b[2];
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) a[ft] = lds4(Bs + (16 * ft + c) * G_LD + 16 * g + 4 * q);
#pragma unroll
      for (int et = 0; et < 2; ++et) b[et] = lds4(As + (32 * wave + 16 * et + c) * G_LD + 16 * g + 4 * q);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
#pragma unroll
          for (int et = 0; et < 2; ++et)
            acc[ft][et] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ft][s], b[et][s], acc[ft][et], 0, 0, 0);
    }
    __syncthreads();
  }
  float* out = P ? P + (size_t)blockIdx.z * M * N : C;
  const int ldo = P ? N : ldc;
  const bool veco = ((ldo & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
#pragma unroll
  for (int ft = 0; ft < 4; ++ft) {
    const int col = n0 + 16 * ft + 4 * q;
    f32x4 bv = splat4(0.f);
    if (bias && !P) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (col + r < N) bv[r] = bias[col + r];
    }
#pragma unroll
    for (int et = 0; et < 2; ++et) {
      const int row = m0 + 32 * wave + 16 * et + c;
      if (row >= M || col >= N) continue;
      f32x4 v = acc[ft][et] + bv;
      if (addend && !P) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col + r < N) v[r] += addend[(size_t)row * ldd + col + r];
      }
      float* o = out + (size_t)row * ldo + col;
      if (veco && col + 3 < N) {
        stg4(o, v);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col + r < N) o[r] = v[r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// bf16 variants of the two GEMMs for mixed-precision training (the reference trains under fp16 autocast, use_amp: True in
// its train configs): operands are rounded to bf16 (RNE) while they are staged into LDS, products run on
// v_mfma_f32_16x16x32_bf16 (16x the fp32 matrix rate), accumulation and outputs stay fp32.  Tensors in HBM stay fp32, so
// these kernels are bound by streaming their operands.  Lane (c = lane & 15, q = lane >> 4) feeds 8 consecutive k-values
// starting at 8 q of its row/column; C/D mapping is the same as the fp32 16x16x4 form.
// ------------------------------------------------------------------------------------------------------------------
constexpr int W_T = 64, W_LD = W_T + 4;  // weight-gradient tile (both precisions; rows per step W_MC / HW_MC: mdx_train_plan.h)
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  uint32_t ua = __float_as_uint(a), ub = __float_as_uint(b);
  ua += 0x7fffu + ((ua >> 16) & 1u);
  ub += 0x7fffu + ((ub >> 16) & 1u);
  return (ua >> 16) | (ub & 0xffff0000u);
}
__device__ __forceinline__ uint16_t to_bf16(float a) {
  uint32_t u = __float_as_uint(a);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// The low-precision operand type of the mixed-precision GEMMs: HT = 0 bfloat16 (round 2's mode), HT = 1 IEEE half -- the type the
// reference's torch.autocast(dtype=torch.float16) casts Linear operands to (scripts/train_drug3d.py:93).  cvt rounds to nearest
// even; a float16 overflows to infinity beyond 65504 like the cast autocast inserts (GradScaler's found_inf then skips the step).
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
template <int HT>
struct HalfT;
template <>
struct HalfT<0> {
  typedef bf16x8_t v8;
  static __device__ __forceinline__ uint16_t cvt(float a) { return to_bf16(a); }
  static __device__ __forceinline__ float back(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct HalfT<1> {
  typedef f16x8_t v8;
  static __device__ __forceinline__ uint16_t cvt(float a) { return __builtin_bit_cast(uint16_t, (_Float16)a); }
  static __device__ __forceinline__ float back(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <int HT>
__device__ __forceinline__ float round_half(float a) { return HalfT<HT>::back(HalfT<HT>::cvt(a)); }
template <int HT>
__device__ __forceinline__ typename HalfT<HT>::v8 lds_h8(const uint16_t* p) { return *reinterpret_cast<const typename HalfT<HT>::v8*>(p); }
// run-time form for the element-wise kernels: kind 0 = keep fp32, 1 = bf16, 2 = fp16
__device__ __forceinline__ float round_kind(float a, int kind) { return kind == 2 ? round_half<1>(a) : kind == 1 ? round_half<0>(a) : a; }

constexpr int H_KC = 64, H_LD = H_KC + 8;  // bf16 elements per staged row (+8 = 16 bytes of padding)

// TN = width of the workgroup's column tile (64 or 128; the launcher picks 64 for N <= 64): fewer passes over the big operand A
// (rows x K); the weight slab (TN x 64 halves per K step) sits in LDS.
template <int HT, bool ROUND, int TN, bool AH>
__global__ __launch_bounds__(256) void hgemm_nt_kernel(const TP A, int lda, const float* __restrict__ B, int ldb,
                                                        const float* __restrict__ bias, const TP addend,
                                                        int ldd, const TPW C, int ldc, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) uint16_t As[G_TM * H_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[TN * H_LD];
  constexpr int FT = TN / 16, BJ = TN / 16;   // feature tiles per wave; B staging slots per thread (TN rows x 16 float4 / 256)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.y * G_TM, n0 = blockIdx.x * TN;
  const bool veca = tp_vec_ok(A.p, A.h, lda);
  const bool vecb = ((ldb & 3) == 0) && ((reinterpret_cast<uintptr_t>(B) & 15) == 0);
  f32x4 acc[FT][2];
  acc_zero<FT, 2>(acc);
  f32x4 ra[8], rb[BJ];   // 16 float4 per row of 64 k: A 128 rows -> 8 slots per thread, B TN rows -> BJ
  uint4 rah[AH ? 4 : 1];  // A already stored as float16: 8 slots of 8 halves per row, copied to LDS as they are (no conversion either way)
  constexpr bool ah = AH;   // compile-time: the fp32-container variant must not carry the half path's registers (occupancy 3 -> 2)
  const bool veca8 = ((lda & 7) == 0) && ((reinterpret_cast<uintptr_t>(A.p) & 15) == 0);
  auto fetch = [&](int k0) {
    if (ah) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int slot = tid + 256 * j, row = slot >> 3, k8 = (slot & 7) * 8;
        const int gm = m0 + row, kk = k0 + k8;
        const uint16_t* src = reinterpret_cast<const uint16_t*>(A.p) + (size_t)gm * lda + kk;
        uint4 v = {0u, 0u, 0u, 0u};
        if (gm < M && kk < K) {
          if (veca8 && kk + 7 < K) {
            v = *reinterpret_cast<const uint4*>(src);
          } else {
            uint16_t e[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) e[u] = kk + u < K ? src[u] : (uint16_t)0;
            v.x = e[0] | ((uint32_t)e[1] << 16); v.y = e[2] | ((uint32_t)e[3] << 16);
            v.z = e[4] | ((uint32_t)e[5] << 16); v.w = e[6] | ((uint32_t)e[7] << 16);
          }
        }
        rah[j] = v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int slot = tid + 256 * j, row = slot >> 4, k4 = (slot & 15) * 4;
        const int gm = m0 + row;
        ra[j] = load4_guard(reinterpret_cast<const float*>(A.p) + (size_t)gm * lda, k0 + k4, K, gm < M, veca);  // AH == false: fp32 container
      }
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int slot = tid + 256 * j, row = slot >> 4, k4 = (slot & 15) * 4;
      const int gn = n0 + row;
      rb[j] = load4_guard(B + (size_t)gn * ldb, k0 + k4, K, gn < N, vecb);
    }
  };
  if (K > 0) fetch(0);
  for (int k0 = 0; k0 < K; k0 += H_KC) {
    if (ah) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int slot = tid + 256 * j;
        *reinterpret_cast<uint4*>(As + (slot >> 3) * H_LD + (slot & 7) * 8) = rah[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int slot = tid + 256 * j;
        uint2 v = {(uint32_t)HalfT<HT>::cvt(ra[j][0]) | ((uint32_t)HalfT<HT>::cvt(ra[j][1]) << 16),
                   (uint32_t)HalfT<HT>::cvt(ra[j][2]) | ((uint32_t)HalfT<HT>::cvt(ra[j][3]) << 16)};
        *reinterpret_cast<uint2*>(As + (slot >> 4) * H_LD + (slot & 15) * 4) = v;
      }
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int slot = tid + 256 * j;
      uint2 v = {(uint32_t)HalfT<HT>::cvt(rb[j][0]) | ((uint32_t)HalfT<HT>::cvt(rb[j][1]) << 16),
                 (uint32_t)HalfT<HT>::cvt(rb[j][2]) | ((uint32_t)HalfT<HT>::cvt(rb[j][3]) << 16)};
      *reinterpret_cast<uint2*>(Bs + (slot >> 4) * H_LD + (slot & 15) * 4) = v;
    }
    __syncthreads();
    if (k0 + H_KC < K) fetch(k0 + H_KC);
#pragma unroll
    for (int ks = 0; ks < H_KC / 32; ++ks) {
      typename HalfT<HT>::v8 a[FT], b[2];
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) a[ft] = lds_h8<HT>(Bs + (16 * ft + c) * H_LD + 32 * ks + 8 * q);
#pragma unroll
      for (int et = 0; et < 2; ++et) b[et] = lds_h8<HT>(As + (32 * wave + 16 * et + c) * H_LD + 32 * ks + 8 * q);
#pragma unroll
      for (int ft = 0; ft < FT; ++ft)
#pragma unroll
        for (int et = 0; et < 2; ++et) acc[ft][et] = HalfT<HT>::mfma(a[ft], b[et], acc[ft][et]);
    }
    __syncthreads();
  }
  const bool veco = tp_vec_ok(C.p, C.h, ldc);
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) {
    const int col = n0 + 16 * ft + 4 * q;
    f32x4 bv = splat4(0.f);
    if (bias) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (col + r < N) bv[r] = bias[col + r];
    }
#pragma unroll
    for (int et = 0; et < 2; ++et) {
      const int row = m0 + 32 * wave + 16 * et + c;
      if (row >= M || col >= N) continue;
      f32x4 v = acc[ft][et] + bv;
      if (addend.p) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col + r < N) v[r] += ld1(addend, (size_t)row * ldd + col + r);
      }
      if (ROUND) {  // the Linear's output in the low-precision type, like autocast's fp16 / bf16 result (held in an fp32 container)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = round_half<HT>(v[r]);
      }
      const size_t o = (size_t)row * ldc + col;
      if (veco && col + 3 < N) {
        st4(C, o, v);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col + r < N) st1(C, o + r, v[r]);
      }
    }
  }
}

// Row-owner float16 Linear for MANY rows (round 3): Y (M,N) = X (M,K) W^T + bias + addend with X in a float16 container, K <= 256,
// N <= 256.  hgemm_nt_kernel walks a short K loop per 128-row tile with two barriers per 64-wide chunk and one chunk in flight per
// workgroup: at these widths it is bound by that latency chain (256 -> 256 on 154,666 rows: 84 us against 32 us of traffic).  Here
// the whole weight sits in LDS as float16 for the lifetime of a persistent workgroup (8 waves, one per CU), every wave owns 16-row
// tiles and needs nobody else: the MFMA's activation operand -- 8 consecutive k of one row per lane -- is a plain 16-byte global
// load in exactly that layout (no LDS round trip, no barrier in the loop), the next tile's rows are requested before the current
// tile's MFMAs, weight fragments are conflict-free 16-byte LDS reads.  X is read once, Y written once.
// Same products, same accumulation order per output as hgemm_nt_kernel (k ascending in chunks of 32): bit-identical results.
// LayerNorm(+ReLU) epilogue (round 5): the wave owns whole rows, so the LayerNorm that follows the Linear in every common.MLP
// (reference models/common.py:191-196) is applied to the tile in registers -- the Linear's result is still stored (the backward needs
// it), and so are the row statistics and the normalised, activated rows: what goes away is the LayerNorm launch and its read of the
// Linear's result.  Same arithmetic as ln_relu_fwd4_kernel on the values the Linear stores (rounded first when it rounds).
struct LnEpi {
  const float *gamma, *beta;   // (N)
  TPW post;                    // (M,N) relu(LN(C)), row stride ldp
  int ldp;
  float* stats;                // (M,2) mean, rstd
  int relu;
};
__device__ __forceinline__ float sum_q4(float v) {   // sum over the four lanes c, c + 16, c + 32, c + 48 (every lane gets it)
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Two adjacent feature tiles of a float16 output row as one 16-byte store per lane (round 6; see csrc/mdx_train_fused.hip sth8_pair): the
// lane rows q / q ^ 1 exchange their 8-byte chunks with v_permlane16_swap, an instruction then writes 16 rows x 64 contiguous bytes
// instead of 16 x 32.  Every lane of the wave's active rows must call it.
__device__ __forceinline__ void st8h_pair(_Float16* row_base, int g2, f32x4 va, f32x4 vb, int q) {
  const f16x4_t ha = {(_Float16)va[0], (_Float16)va[1], (_Float16)va[2], (_Float16)va[3]};
  const f16x4_t hb = {(_Float16)vb[0], (_Float16)vb[1], (_Float16)vb[2], (_Float16)vb[3]};
  const uint2 ua = __builtin_bit_cast(uint2, ha), ub = __builtin_bit_cast(uint2, hb);
  const auto sx = __builtin_amdgcn_permlane16_swap(ua.x, ub.x, false, false);
  const auto sy = __builtin_amdgcn_permlane16_swap(ua.y, ub.y, false, false);
  const uint4 v = {sx[0], sy[0], sx[1], sy[1]};
  const int col = (q & 1) ? 32 * g2 + 16 + 4 * (q - 1) : 32 * g2 + 4 * q;
  *reinterpret_cast<uint4*>(row_base + col) = v;
}

template <int KT, int FT, bool ROUND, bool LN = false>
__global__ __launch_bounds__(512) void hgemm_nt_rows_kernel(const _Float16* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                             const float* __restrict__ bias, const TP addend, int ldd, const TPW C,
                                                             int ldc, int M, const LnEpi ln = LnEpi{}) {
  constexpr int K = 32 * KT, N = 16 * FT, LD = K + 8;
  // blockIdx.y = column group (round 6; not with the LayerNorm epilogue): a Linear over the ~5,500 NODE rows needs only ~43 workgroups
  // for its rows, each of which used to stage the WHOLE weight; cut into groups of N output columns the same rows are served by
  // gridDim.y times the workgroups, each staging 1 / gridDim.y of the weight (A is re-read from L2).
  const int col0 = N * (int)blockIdx.y;
  B += (size_t)col0 * ldb;
  if (bias) bias += col0;
  extern __shared__ __attribute__((aligned(16))) uint16_t hr_smem[];
  uint16_t* Ws = hr_smem;                                   // [N][LD] float16
  float* bs = reinterpret_cast<float*>(hr_smem + N * LD);   // [N] (+ [N] gamma, [N] beta with the LayerNorm epilogue)
  if (LN)
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
      bs[N + i] = ln.gamma[i];
      bs[2 * N + i] = ln.beta[i];
    }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const bool vecb = ((ldb & 3) == 0) && ((reinterpret_cast<uintptr_t>(B) & 15) == 0);
  // weight -> LDS as float16.  Eight 16-byte loads in flight per thread (round 6): with one, a workgroup needed ~20 us for a 256 x 256
  // weight -- the whole cost of a Linear over the N node rows (43 workgroups, one tile per wave): 25 us per launch, ~100 launches a step.
  {
    constexpr int NV = N * (K / 4), U = NV >= 8 * 512 ? 8 : (NV >= 4 * 512 ? 4 : 1);
    for (int i0 = tid; i0 < NV; i0 += U * (int)blockDim.x) {
      f32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * (int)blockDim.x;
        if (i < NV) v[u] = load4_guard(B + (size_t)(i / (K / 4)) * ldb, (i % (K / 4)) * 4, K, true, vecb);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * (int)blockDim.x;
        if (i < NV) {
          const uint2 h = {(uint32_t)HalfT<1>::cvt(v[u][0]) | ((uint32_t)HalfT<1>::cvt(v[u][1]) << 16),
                           (uint32_t)HalfT<1>::cvt(v[u][2]) | ((uint32_t)HalfT<1>::cvt(v[u][3]) << 16)};
          *reinterpret_cast<uint2*>(Ws + (i / (K / 4)) * LD + (i % (K / 4)) * 4) = h;
        }
      }
    }
  }
  for (int i = tid; i < N; i += blockDim.x) bs[i] = bias ? bias[i] : 0.f;
  __syncthreads();  // the only barrier

  const int nw = gridDim.x * (blockDim.x >> 6), ntiles = (M + 15) >> 4;
  int tile = blockIdx.x * (blockDim.x >> 6) + wave;
  uint4 x[KT], xn[KT];
  auto load = [&](uint4 (&d)[KT], int t) {
    const int row = min(16 * t + c, M - 1);   // clamped: loads stay inside the matrix, stores are predicated
    const _Float16* p = A + (size_t)row * lda + 8 * q;
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) d[ks] = *reinterpret_cast<const uint4*>(p + 32 * ks);
  };
  if (tile < ntiles) load(x, tile);
  const bool veco = tp_vec_ok(C.p, C.h, ldc) && (col0 & 3) == 0, vecd = addend.p && tp_vec_ok(addend.p, addend.h, ldd) && (col0 & 3) == 0;
  // float16 rows on 16 bytes: pairs of feature tiles leave as 16-byte stores (st8h_pair)
  const bool pairc = (FT % 2 == 0) && C.h && (ldc & 7) == 0 && (reinterpret_cast<uintptr_t>(C.p) & 15) == 0 && (col0 & 7) == 0;
  const bool pairp = LN && (FT % 2 == 0) && ln.post.h && (ln.ldp & 7) == 0 && (reinterpret_cast<uintptr_t>(ln.post.p) & 15) == 0;
  const uint16_t* wl = Ws + c * LD + 8 * q;
#pragma unroll 1
  for (; tile < ntiles; tile += nw) {
    if (tile + nw < ntiles) load(xn, tile + nw);
    f32x4 acc[FT];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) acc[ft] = splat4(0.f);
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      const f16x8_t b = __builtin_bit_cast(f16x8_t, x[ks]);
#pragma unroll
      for (int ft = 0; ft < FT; ++ft)
        acc[ft] = __builtin_amdgcn_mfma_f32_16x16x32_f16(lds_h8<1>(wl + 16 * ft * LD + 32 * ks), b, acc[ft], 0, 0, 0);
      // one k-step's weight fragments at a time (hoisting all FT x KT reads ahead of the MFMAs spills; the other wave of the SIMD
      // covers the read latency and the kernel streams rows, it does not live on the matrix pipe)
      __builtin_amdgcn_sched_barrier(0);
    }
    const int row = 16 * tile + c;
    if (row < M) {
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) {
        const int col = 16 * ft + 4 * q;
        f32x4 v = acc[ft] + lds4(bs + col);
        if (addend.p) {
          if (vecd) {
            v = v + ld4(addend, (size_t)row * ldd + col0 + col);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += ld1(addend, (size_t)row * ldd + col0 + col + r);
          }
        }
        if (ROUND) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = round_half<1>(v[r]);
        }
        const size_t o = (size_t)row * ldc + col0 + col;
        if (pairc) {
          if (ft & 1) st8h_pair(reinterpret_cast<_Float16*>(C.p) + (size_t)row * ldc + col0, ft >> 1, acc[ft - 1], v, q);
        } else if (veco) {
          st4(C, o, v);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) st1(C, o + r, v[r]);
        }
        if (LN || pairc) acc[ft] = v;     // (the finished values: the LayerNorm epilogue / the pair store of the next tile reads them)
      }
    }
    if (LN) {   // (every lane takes part in the cross-lane sums; rows past M hold clamped duplicates and store nothing)
      float sm = 0.f;
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) sm += (acc[ft][0] + acc[ft][1]) + (acc[ft][2] + acc[ft][3]);
      const float mean = sum_q4(sm) * (1.0f / N);
      float d2 = 0.f;
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) {
        acc[ft] = acc[ft] - splat4(mean);
        d2 = fmaf(acc[ft][0], acc[ft][0], fmaf(acc[ft][1], acc[ft][1], fmaf(acc[ft][2], acc[ft][2], fmaf(acc[ft][3], acc[ft][3], d2))));
      }
      const float rstd = 1.0f / sqrtf(sum_q4(d2) * (1.0f / N) + MDX_LN_EPS);
      if (row < M) {
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) {
          const int col = 16 * ft + 4 * q;
          f32x4 y = acc[ft] * splat4(rstd) * lds4(bs + N + col) + lds4(bs + 2 * N + col);
          if (ln.relu) y = relu4(y);
          if (pairp) {
            if (ft & 1) st8h_pair(reinterpret_cast<_Float16*>(ln.post.p) + (size_t)row * ln.ldp, ft >> 1, acc[ft - 1], y, q);
            acc[ft] = y;
          } else {
            st4(ln.post, (size_t)row * ln.ldp + col, y);
          }
        }
        if (q == 0) {
          ln.stats[2 * (size_t)row] = mean;
          ln.stats[2 * (size_t)row + 1] = rstd;
        }
      }
    }
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) x[ks] = xn[ks];
  }
}

}  // namespace
int mdx_num_cus();  // mdx_api.hip
namespace {
template <int KT, int FT, bool ROUND, bool LN = false>
static void launch_hgemm_nt_rows(const _Float16* A, int lda, const float* B, int ldb, const float* bias, const TP& addend, int ldd,
                                 const TPW& C, int ldc, int M, hipStream_t s, const LnEpi& ln = LnEpi{}, int groups = 1) {
  constexpr int lds = 16 * FT * (32 * KT + 8) * 2 + 16 * FT * 4 * (LN ? 3 : 1);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)hgemm_nt_rows_kernel<KT, FT, ROUND, LN>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr = true;
  }
  static int per_cu = 0;   // resident workgroups per CU: one where the weight fills the LDS, more for the narrow layers
  if (!per_cu) {
    int nb = 0;
    per_cu = (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hgemm_nt_rows_kernel<KT, FT, ROUND, LN>, 512, lds) == hipSuccess && nb > 0)
                 ? std::min(nb, 4) : 1;
  }
  const int ntiles = (M + 15) / 16;
  const int grid = std::max(1, std::min(mdx_num_cus() * per_cu, (ntiles + 7) / 8));
  hipLaunchKernelGGL((hgemm_nt_rows_kernel<KT, FT, ROUND, LN>), dim3(grid, groups), dim3(512), lds, s, A, lda, B, ldb, bias, addend, ldd, C, ldc, M,
                     ln);
}

// bf16 weight gradient: HW_MC = 64 rows of G and X per step are transposed into LDS ([column][row], so that the 8 consecutive
// contraction values a lane needs are one 16-byte read); otherwise the structure of sgemm_tn_split_kernel.
// Workgroup tile TNW (columns of G) x TKW (columns of X) = 64 x 64; wave w owns a 32 x 32 quadrant.  (128-wide tiles for this conversion
// kernel measured slower: 47.9 vs 44.0 ms per step, occupancy 4 -> 2; the transpose-read kernel below has them.)
template <int HT>
__device__ __forceinline__ void hgemm_tn_split_body(const TP G, int ldg, const TP X, int ldx, int M, int N, int K, int mper,
                                                    float* __restrict__ P, float* __restrict__ Pb, const int bx, const int by,
                                                    const int bz) {
  constexpr int TNW = 64, TKW = 64;
  __shared__ __attribute__((aligned(16))) uint16_t Gt[TNW * H_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Xt[TKW * H_LD];
  constexpr int IN = TNW / 32, IK = TKW / 32;      // 16 x 16 tiles per wave along n / k
  constexpr int NBG = TNW / 64, NBX = TKW / 64;    // 4 x 4 staging blocks per thread and step
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int n0 = by * TNW, k0 = bx * TKW;
  const int mbeg = bz * mper, mend = min(M, mbeg + mper);
  const int wn = (wave >> 1) * (TNW / 2), wk = (wave & 1) * (TKW / 2);
  const bool vecg = tp_vec_ok(G.p, G.h, ldg) && ((n0 & 3) == 0);
  const bool vecx = tp_vec_ok(X.p, X.h, ldx) && ((k0 & 3) == 0);
  f32x4 acc[IN][IK];
  acc_zero<IN, IK>(acc);
  const bool do_bias = Pb && bx == 0 && tid < TNW;
  float bsum = 0.f;
  // 4 x 4 blocks: block b of a W-wide tile = rows 4 (b / (W/4)) ..+3, columns 4 (b % (W/4)) ..+3; transposed in registers, they leave
  // as four 8-byte LDS stores ([column][4 consecutive rows]) -- round 2 wrote sixteen 2-byte stores per block, which (with the
  // conversions) bound this kernel, not its traffic.
  f32x4 rg[NBG][4], rx[NBX][4];
  auto fetch = [&](int m0) {
#pragma unroll
    for (int u = 0; u < NBG; ++u) {
      const int bq = tid + 256 * u, r4 = 4 * (bq / (TNW / 4)), c4 = 4 * (bq % (TNW / 4));
#pragma unroll
      for (int j = 0; j < 4; ++j) rg[u][j] = load4_guard_t(G, (size_t)(m0 + r4 + j) * ldg + n0, c4, N - n0, m0 + r4 + j < mend, vecg);
    }
#pragma unroll
    for (int u = 0; u < NBX; ++u) {
      const int bq = tid + 256 * u, r4 = 4 * (bq / (TKW / 4)), c4 = 4 * (bq % (TKW / 4));
#pragma unroll
      for (int j = 0; j < 4; ++j) rx[u][j] = load4_guard_t(X, (size_t)(m0 + r4 + j) * ldx + k0, c4, K - k0, m0 + r4 + j < mend, vecx);
    }
  };
  auto stage = [&](uint16_t* dst, const f32x4 (&r)[4], int r4, int c4) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint2 v = {(uint32_t)HalfT<HT>::cvt(r[0][e]) | ((uint32_t)HalfT<HT>::cvt(r[1][e]) << 16),
                       (uint32_t)HalfT<HT>::cvt(r[2][e]) | ((uint32_t)HalfT<HT>::cvt(r[3][e]) << 16)};
      *reinterpret_cast<uint2*>(dst + (c4 + e) * H_LD + r4) = v;
    }
  };
  if (mbeg < mend) fetch(mbeg);
  for (int m0 = mbeg; m0 < mend; m0 += HW_MC) {
#pragma unroll
    for (int u = 0; u < NBG; ++u) {
      const int bq = tid + 256 * u;
      stage(Gt, rg[u], 4 * (bq / (TNW / 4)), 4 * (bq % (TNW / 4)));
    }
#pragma unroll
    for (int u = 0; u < NBX; ++u) {
      const int bq = tid + 256 * u;
      stage(Xt, rx[u], 4 * (bq / (TKW / 4)), 4 * (bq % (TKW / 4)));
    }
    __syncthreads();
    if (m0 + HW_MC < mend) fetch(m0 + HW_MC);
    if (do_bias) {  // bias gradient partial: column tid of the staged (half-rounded) G tile, fp32 sum
      float sacc = 0.f;
#pragma unroll 8
      for (int r = 0; r < HW_MC; ++r) sacc += HalfT<HT>::back(Gt[tid * H_LD + r]);
      bsum += sacc;
    }
#pragma unroll
    for (int ks = 0; ks < HW_MC / 32; ++ks) {
      typename HalfT<HT>::v8 a[IN], b[IK];
#pragma unroll
      for (int i = 0; i < IN; ++i) a[i] = lds_h8<HT>(Gt + (wn + 16 * i + c) * H_LD + 32 * ks + 8 * q);
#pragma unroll
      for (int j = 0; j < IK; ++j) b[j] = lds_h8<HT>(Xt + (wk + 16 * j + c) * H_LD + 32 * ks + 8 * q);
#pragma unroll
      for (int i = 0; i < IN; ++i)
#pragma unroll
        for (int j = 0; j < IK; ++j) acc[i][j] = HalfT<HT>::mfma(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  if (do_bias && n0 + tid < N) Pb[(size_t)bz * N + n0 + tid] = bsum;
  float* out = P + (size_t)bz * N * K;
#pragma unroll
  for (int i = 0; i < IN; ++i)
#pragma unroll
    for (int j = 0; j < IK; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * i + 4 * q + r, k = k0 + wk + 16 * j + c;
        if (n < N && k < K) out[(size_t)n * K + k] = acc[i][j][r];
      }
}

template <int HT>
__global__ __launch_bounds__(256) void hgemm_tn_split_kernel(const TP G, int ldg, const TP X, int ldx,
                                                              int M, int N, int K, int mper, float* __restrict__ P,
                                                              float* __restrict__ Pb) {
  hgemm_tn_split_body<HT>(G, ldg, X, ldx, M, N, K, mper, P, Pb, blockIdx.x, blockIdx.y, blockIdx.z);
}

// float16 weight gradient on float16 CONTAINERS (half storage, round 3): P[z][n][k] = sum_{m in split z} G[m][n] * X[m][k].
// The contraction runs over ROWS, so an MFMA operand (8 contraction values of one column per lane) is a column walk through a
// row-major tile.  hgemm_tn_split_kernel transposes 4 x 4 blocks in registers while staging and is bound by those instructions
// (a 256 x 256 gradient over 154,666 rows: 204 us against 32 us of operand streaming).  Here the tiles go global -> LDS as they
// are (16-byte copies, no conversion, no shuffles) and the operands come out of ds_read_b64_tr_b16, gfx950's LDS transpose
// read: within a group of 16 lanes, lane p supplies the address of 4 consecutive halves and lane i receives element i % 4 of the
// loads of lanes 4 j + i / 4 (j = 0..3).  With lane p pointing at row 4 g + p / 4, columns 4 (p % 4).. of a 16-column subtile, lane i
// of group g gets rows 4 g .. 4 g + 3 of column i -- two such reads (rows +0 and +16) are the 8 contraction values of a
// 16x16x32 MFMA operand.  Which 8 of the 32 rows a lane group holds is irrelevant as long as both operands agree.
// LDS image: [16-column subtile][64 rows][16 halves] (32-byte rows: the conflict-free layout for the transpose read; a group's
// four rows are 128 bytes, the wave's four groups 512 consecutive bytes).  Staging lanes 8 s .. 8 s + 7 write 128 consecutive
// bytes of subtile s (4 rows x 32 bytes): conflict-free 16-byte stores.
typedef __fp16 fh4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef _Float16 f16x4v_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f16x8_t lds_tr8(const _Float16* p) {
  typedef __attribute__((address_space(3))) fh4_t* lds_ptr;
  const fh4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_ptr)(p));
  const fh4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_ptr)(p + 16 * 16));
  return __builtin_shufflevector(__builtin_bit_cast(f16x4v_t, lo), __builtin_bit_cast(f16x4v_t, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}
template <int TNW, int TKW>
__device__ __forceinline__ void hgemm_tn_tr_body(const _Float16* __restrict__ G, int ldg, const _Float16* __restrict__ X, int ldx, int M,
                                                 int N, int K, int mper, float* __restrict__ P, float* __restrict__ Pb, const int bx,
                                                 const int by, const int bz) {
  constexpr int SUB = HW_MC * 16;                  // halves per 16-column subtile
  __shared__ __attribute__((aligned(16))) _Float16 Gt[(TNW / 16) * SUB];
  __shared__ __attribute__((aligned(16))) _Float16 Xt[(TKW / 16) * SUB];
  constexpr int IN = TNW / 32, IK = TKW / 32;      // 16 x 16 tiles per wave along n / k
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int n0 = by * TNW, k0 = bx * TKW;
  const int mbeg = bz * mper, mend = min(M, mbeg + mper);
  const int wn = (wave >> 1) * (TNW / 2), wk = (wave & 1) * (TKW / 2);
  f32x4 acc[IN][IK];
  acc_zero<IN, IK>(acc);
  const bool do_bias = Pb && bx == 0 && tid < TNW;
  float bsum = 0.f;
  // staging: W / 32 16-byte pieces per thread and tile; lanes 8 s .. 8 s + 7 of a wave fill 4 rows of subtile s
  uint4 rg[TNW / 32], rx[TKW / 32];
  auto piece = [&](int W, int u, int& row, int& col) {   // u-th piece of this thread in a W-column tile
    const int nsub = W / 16, sel = lane >> 3;
    row = 4 * (8 / nsub) * (wave + 4 * u) + 4 * (sel / nsub) + ((lane >> 1) & 3);
    col = 16 * (sel % nsub) + 8 * (lane & 1);
  };
  auto fetch = [&](int m0) {
#pragma unroll
    for (int u = 0; u < TNW / 32; ++u) {
      int row, col;
      piece(TNW, u, row, col);
      rg[u] = m0 + row < mend ? *reinterpret_cast<const uint4*>(G + (size_t)(m0 + row) * ldg + n0 + col) : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int u = 0; u < TKW / 32; ++u) {
      int row, col;
      piece(TKW, u, row, col);
      rx[u] = m0 + row < mend ? *reinterpret_cast<const uint4*>(X + (size_t)(m0 + row) * ldx + k0 + col) : uint4{0, 0, 0, 0};
    }
  };
  if (mbeg < mend) fetch(mbeg);
  for (int m0 = mbeg; m0 < mend; m0 += HW_MC) {
#pragma unroll
    for (int u = 0; u < TNW / 32; ++u) {
      int row, col;
      piece(TNW, u, row, col);
      *reinterpret_cast<uint4*>(Gt + (col >> 4) * SUB + row * 16 + (col & 15)) = rg[u];
    }
#pragma unroll
    for (int u = 0; u < TKW / 32; ++u) {
      int row, col;
      piece(TKW, u, row, col);
      *reinterpret_cast<uint4*>(Xt + (col >> 4) * SUB + row * 16 + (col & 15)) = rx[u];
    }
    __syncthreads();
    if (m0 + HW_MC < mend) fetch(m0 + HW_MC);
    if (do_bias) {  // bias gradient partial: column tid of the staged G tile, fp32 sum in row order
      float sacc = 0.f;
      const _Float16* col = Gt + (tid >> 4) * SUB + (tid & 15);
#pragma unroll 8
      for (int r = 0; r < HW_MC; ++r) sacc += (float)col[r * 16];
      bsum += sacc;
    }
    const int lrow = (4 * q + (c >> 2)) * 16 + 4 * (c & 3);   // this lane's address inside a 32-row block of a subtile
#pragma unroll
    for (int ks = 0; ks < HW_MC / 32; ++ks) {
      f16x8_t a[IN], b[IK];
#pragma unroll
      for (int i = 0; i < IN; ++i) a[i] = lds_tr8(Gt + ((wn >> 4) + i) * SUB + 32 * 16 * ks + lrow);
#pragma unroll
      for (int j = 0; j < IK; ++j) b[j] = lds_tr8(Xt + ((wk >> 4) + j) * SUB + 32 * 16 * ks + lrow);
#pragma unroll
      for (int i = 0; i < IN; ++i)
#pragma unroll
        for (int j = 0; j < IK; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  if (do_bias && n0 + tid < N) Pb[(size_t)bz * N + n0 + tid] = bsum;
  float* out = P + (size_t)bz * N * K;
#pragma unroll
  for (int i = 0; i < IN; ++i)
#pragma unroll
    for (int j = 0; j < IK; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * i + 4 * q + r, k = k0 + wk + 16 * j + c;
        if (n < N && k < K) out[(size_t)n * K + k] = acc[i][j][r];
      }
}

template <int TNW, int TKW>
__global__ __launch_bounds__(256) void hgemm_tn_tr_kernel(const _Float16* __restrict__ G, int ldg, const _Float16* __restrict__ X, int ldx,
                                                           int M, int N, int K, int mper, float* __restrict__ P,
                                                           float* __restrict__ Pb) {
  hgemm_tn_tr_body<TNW, TKW>(G, ldg, X, ldx, M, N, K, mper, P, Pb, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Grouped weight gradients (round 6): the ~260 weight-gradient contractions of a training step do not feed anything before the
// optimizer, so the host queues them (train_ops.sgemm_tn with an active gradient sink) and ONE launch per tile class runs a whole
// table of them.  Record (16 x int64): G, X, P, Pb, ldg, ldx, M, N, K, mper, gx (tiles along K), gy (tiles along N), S (row ranges),
// dt (bit 0 G float16, bit 1 X float16), first_block, unused.  A job's blocks are numbered like its own grid would be (k tile
// fastest, then n tile, then row range: the blocks that share rows of G and X are neighbours, L2 serves the re-reads); the bodies are
// the stand-alone kernels', so a job's partials are bit-identical to a stand-alone launch with the same `mper`.
// KIND 0..3: transpose-read kernel with tiles 128x128, 128x64, 64x128, 64x64; 4: converting kernel, 64x64 tiles, float16 products;
// 5 / 6: transpose-read kernel with 32x64 / 64x32 tiles; 7: one output row or one input column (wgrad_colsum_body).
// Weight gradient with ONE output row or ONE input column (a Linear to a scalar: PosUpdate's 256 -> 1 and its gate's 32 -> 1; the time
// column of a gate's first Linear): dW[c] = sum_m s[m] A[m][c] with (s, A) = (dY (M,1), X (M,C)) or (X (M,1), dY (M,C)) -- a scaled column
// sum, not a matrix product (the 64 x 64 MFMA tile of the converting kernel spent 20 us per call on 63/64 zero columns).  256 threads =
// 256 / (C/4) rows x C/4 lanes of four columns; row groups are combined through LDS in a fixed order.  Bias partials: the plain column
// sums of dY (A = dY) or sum_m s[m] (s = dY).  C % 4 == 0, C <= 256.
__device__ __forceinline__ void wgrad_colsum_body(const TP s_, int lds, const TP A_, int lda, int C, bool bias_is_A, int M, int mper, float* __restrict__ P,
                                                  float* __restrict__ Pb, const int bz) {
  // a thread owns 8 columns of float16 rows (one 16-byte load) or 4 of fp32 rows, and every (256 / lanes-per-row)-th row of the range
  __shared__ f32x4 red[2][256];
  __shared__ f32x4 redb[2][256];
  const int tid = threadIdx.x;
  const bool wide = A_.h && (C & 7) == 0 && (lda & 7) == 0 && ((reinterpret_cast<uintptr_t>(A_.p) & 15) == 0);
  const int cpt = wide ? 8 : 4, lpr = C / cpt, rows_it = 256 / lpr;
  const int cl = tid % lpr, rl = tid / lpr;
  const int mbeg = bz * mper, mend = min(M, mbeg + mper);
  const bool vec = tp_vec_ok(A_.p, A_.h, lda);
  f32x4 acc[2] = {splat4(0.f), splat4(0.f)}, accb[2] = {splat4(0.f), splat4(0.f)};
  if (rl < rows_it) {
#pragma unroll 4
    for (int m = mbeg + rl; m < mend; m += rows_it) {
      float sv = ld1(s_, (size_t)m * lds);   // (the scalar operand may be one column of a wider matrix)
      // autocast arithmetic: operands of a Linear's contraction are float16 VALUES (the converting kernel rounds fp32 containers the same way)
      if (!s_.h) sv = round_half<1>(sv);
      f32x4 a0, a1 = splat4(0.f);
      if (wide) {
        const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const _Float16*>(A_.p) + (size_t)m * lda + 8 * cl);
        const f16x4_t lo = __builtin_bit_cast(f16x4_t, uint2{u.x, u.y}), hi = __builtin_bit_cast(f16x4_t, uint2{u.z, u.w});
        a0 = f32x4{(float)lo[0], (float)lo[1], (float)lo[2], (float)lo[3]};
        a1 = f32x4{(float)hi[0], (float)hi[1], (float)hi[2], (float)hi[3]};
      } else {
        if (vec) {
          a0 = ld4(A_, (size_t)m * lda + 4 * cl);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) a0[r] = ld1(A_, (size_t)m * lda + 4 * cl + r);
        }
        if (!A_.h) {
#pragma unroll
          for (int r = 0; r < 4; ++r) a0[r] = round_half<1>(a0[r]);
        }
      }
      acc[0] = acc[0] + a0 * splat4(sv);
      acc[1] = acc[1] + a1 * splat4(sv);
      accb[0] = accb[0] + (bias_is_A ? a0 : splat4(sv));
      accb[1] = accb[1] + (bias_is_A ? a1 : splat4(sv));
    }
  }
  red[0][tid] = acc[0], red[1][tid] = acc[1];
  redb[0][tid] = accb[0], redb[1][tid] = accb[1];
  __syncthreads();
  if (tid < lpr) {
    f32x4 r[2] = {splat4(0.f), splat4(0.f)}, rb[2] = {splat4(0.f), splat4(0.f)};
    for (int g = 0; g < rows_it; ++g) {
      r[0] = r[0] + red[0][g * lpr + tid], r[1] = r[1] + red[1][g * lpr + tid];
      rb[0] = rb[0] + redb[0][g * lpr + tid], rb[1] = rb[1] + redb[1][g * lpr + tid];
    }
    float* out = P + (size_t)bz * C;
    const int nh = cpt / 4;
    for (int h = 0; h < nh; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) out[cpt * tid + 4 * h + e] = r[h][e];
    if (Pb) {
      if (bias_is_A) {
        for (int h = 0; h < nh; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e) Pb[(size_t)bz * C + cpt * tid + 4 * h + e] = rb[h][e];
      } else if (tid == 0) {
        Pb[bz] = rb[0][0];   // (every lane of a row added s[m] once: lane 0's sum over the row groups is sum_m s[m])
      }
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void wgrad_grouped_kernel(const long long* __restrict__ desc, int n) {
  const long long blk = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[16 * mid + 14] <= blk) lo = mid; else hi = mid - 1;
  }
  const long long* d = desc + 16 * lo;
  const int rel = (int)(blk - d[14]);
  const int gx = (int)d[10], gy = (int)d[11];
  // XCD-aware numbering: workgroup ids go round-robin over the 8 XCDs (id % 8) and each XCD has its own L2, so the gx * gy tiles of
  // one row range -- which read the same rows of G and X -- must sit on ids that are EQUAL mod 8, close in dispatch order.  Blocks are
  // dealt in chunks of 8 row ranges: inside a chunk, id i works on row range i % 8 and tile i / 8 (the last, short chunk deals over
  // what is left; with one tile per row range this is the plain order).  Which block computes a (tile, row range) does not change its result.
  const int T = gx * gy, S = (int)d[12];
  const int chunk = rel / (8 * T), i = rel - chunk * 8 * T;
  const int w = min(8, S - 8 * chunk);
  const int bz = 8 * chunk + i % w, t = i / w;
  const int bx = t % gx, by = t / gx;
  float* P = reinterpret_cast<float*>(d[2]);
  float* Pb = reinterpret_cast<float*>(d[3]);
  const int ldg = (int)d[4], ldx = (int)d[5], M = (int)d[6], N = (int)d[7], K = (int)d[8], mper = (int)d[9];
  if constexpr (KIND < 4) {
    const _Float16* G = reinterpret_cast<const _Float16*>(d[0]);
    const _Float16* X = reinterpret_cast<const _Float16*>(d[1]);
    hgemm_tn_tr_body<(KIND < 2 ? 128 : 64), ((KIND & 1) ? 64 : 128)>(G, ldg, X, ldx, M, N, K, mper, P, Pb, bx, by, bz);
  } else if constexpr (KIND == 5 || KIND == 6) {   // 32-wide layers (the gates' hidden width): 32 x 64 / 64 x 32 tiles of the same kernel
    const _Float16* G = reinterpret_cast<const _Float16*>(d[0]);
    const _Float16* X = reinterpret_cast<const _Float16*>(d[1]);
    hgemm_tn_tr_body<(KIND == 5 ? 32 : 64), (KIND == 5 ? 64 : 32)>(G, ldg, X, ldx, M, N, K, mper, P, Pb, bx, by, bz);
  } else if constexpr (KIND == 7) {                // N == 1 or K == 1: scaled column sums
    const int dt = (int)d[13];
    const TP G{reinterpret_cast<const void*>(d[0]), dt & 1}, X{reinterpret_cast<const void*>(d[1]), (dt >> 1) & 1};
    if (N == 1) wgrad_colsum_body(G, ldg, X, ldx, K, false, M, mper, P, Pb, bz);
    else wgrad_colsum_body(X, ldx, G, ldg, N, true, M, mper, P, Pb, bz);
  } else {
    const int dt = (int)d[13];
    const TP G{reinterpret_cast<const void*>(d[0]), dt & 1}, X{reinterpret_cast<const void*>(d[1]), (dt >> 1) & 1};
    hgemm_tn_split_body<1>(G, ldg, X, ldx, M, N, K, mper, P, Pb, bx, by, bz);
  }
}

// Weight gradient without transposes: P[z][n][k] = sum_{m in split z} G[m][n] * X[m][k]   (G = dY (M,N), X (M,K) row-major).
// Workgroup tile 64 (n) x 64 (k); 32 rows of G and X are staged per step in their memory layout [m][cols] (coalesced
// 16-byte loads); the MFMA contraction index runs over m, so operands are read from LDS as scalars down a column
// (leading dimension 68: the four row groups of a wave land in disjoint banks).  Wave w owns a 32 x 32 quadrant.
// Pb != NULL: the workgroups of the first k-tile also produce the bias gradient partials Pb[z][n] = sum_m G[m][n] of their
// row range from the G tile they stage anyway (saves a second pass over dY).
__global__ __launch_bounds__(256) void sgemm_tn_split_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ X, int ldx,
                                                              int M, int N, int K, int mper, float* __restrict__ P,
                                                              float* __restrict__ Pb) {
  __shared__ __attribute__((aligned(16))) float Gs[W_MC * W_LD];
  __shared__ __attribute__((aligned(16))) float Xs[W_MC * W_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.y * W_T, k0 = blockIdx.x * W_T;
  const int mbeg = blockIdx.z * mper, mend = min(M, mbeg + mper);
  const int wn = (wave >> 1) * 32, wk = (wave & 1) * 32;
  const bool vecg = ((ldg & 3) == 0) && ((reinterpret_cast<uintptr_t>(G) & 15) == 0);
  const bool vecx = ((ldx & 3) == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
  f32x4 acc[2][2];
  acc_zero<2, 2>(acc);
  const bool do_bias = Pb && blockIdx.x == 0 && tid < W_T;
  float bsum = 0.f;
  // 32 rows x 16 float4 per tile = 512 slots -> 2 per thread per tile
  f32x4 rg[2], rx[2];
  auto fetch = [&](int m0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int slot = tid + 256 * j, row = slot >> 4, c4 = (slot & 15) * 4;
      const int gm = m0 + row;
      rg[j] = load4_guard(G + (size_t)gm * ldg + n0, c4, N - n0, gm < mend, vecg && ((n0 & 3) == 0));
      rx[j] = load4_guard(X + (size_t)gm * ldx + k0, c4, K - k0, gm < mend, vecx && ((k0 & 3) == 0));
    }
  };
  if (mbeg < mend) fetch(mbeg);
  for (int m0 = mbeg; m0 < mend; m0 += W_MC) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int slot = tid + 256 * j, row = slot >> 4, c4 = (slot & 15) * 4;
      sts4(Gs + row * W_LD + c4, rg[j]);
      sts4(Xs + row * W_LD + c4, rx[j]);
    }
    __syncthreads();
    if (m0 + W_MC < mend) fetch(m0 + W_MC);
    if (do_bias) {
#pragma unroll
      for (int r = 0; r < W_MC; ++r) bsum += Gs[r * W_LD + tid];   // rows past mend were staged as zeros
    }
#pragma unroll
    for (int mm = 0; mm < W_MC; mm += 16) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int r = mm + 4 * q + s;
        float a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = Gs[r * W_LD + wn + 16 * i + c];
          b[i] = Xs[r * W_LD + wk + 16 * i + c];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (do_bias && n0 + tid < N) Pb[(size_t)blockIdx.z * N + n0 + tid] = bsum;
  // acc[i][j][r] = P[n = n0 + wn + 16 i + 4 q + r][k = k0 + wk + 16 j + c]
  float* out = P + (size_t)blockIdx.z * N * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + 16 * i + 4 * q + r, k = k0 + wk + 16 * j + c;
        if (n < N && k < K) out[(size_t)n * K + k] = acc[i][j][r];
      }
}

// C[i][j] = bias[j] + sum_z P[z][i][j].  Block = 32 consecutive outputs x 8 split lanes: lane z sums splits z, z+8, ...
// of its chunk (coalesced 128-byte reads), the 8 lane sums are combined in lane order -> a fixed summation tree,
// deterministic.  blockIdx.y selects a chunk of `chunk` splits and writes row blockIdx.y of the output (two-stage use).
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ P, int S, int chunk, int M, int N,
                                                               const float* __restrict__ bias, float* __restrict__ C, int ldc,
                                                               int rkind = 0) {
  __shared__ float sh[8][32];
  const int o = threadIdx.x & 31, z = threadIdx.x >> 5;
  const size_t total = (size_t)M * N;
  const size_t i = (size_t)blockIdx.x * 32 + o;
  const int s0 = blockIdx.y * chunk, s1 = min(S, s0 + chunk);
  float s = 0.f;
  if (i < total)
    for (int k = s0 + z; k < s1; k += 8) s += P[(size_t)k * total + i];
  sh[z][o] = s;
  __syncthreads();
  if (z == 0 && i < total) {
    const int row = (int)(i / N), col = (int)(i % N);
    float r = bias ? bias[col] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) r += sh[k][o];
    C[(size_t)blockIdx.y * total + (size_t)row * ldc + col] = round_kind(r, rkind);
  }
}

// One launch for the two reductions a weight gradient needs (dW partials, then -- in the extra workgroups -- the bias partials):
// the same per-output summation as reduce_partials_kernel with S <= RED_CHUNK.
__global__ __launch_bounds__(256) void reduce_partials2_kernel(const float* __restrict__ P, int S, int M, int N, float* __restrict__ C,
                                                                int ldc, int gx_w, const float* __restrict__ Pb, int Nb,
                                                                float* __restrict__ db, int rkind = 0) {
  __shared__ float sh[8][32];
  const int o = threadIdx.x & 31, z = threadIdx.x >> 5;
  const bool bias_part = (int)blockIdx.x >= gx_w;
  const float* src = bias_part ? Pb : P;
  const size_t total = bias_part ? (size_t)Nb : (size_t)M * N;
  const size_t i = (size_t)(bias_part ? blockIdx.x - gx_w : blockIdx.x) * 32 + o;
  float s = 0.f;
  if (i < total)
    for (int k = z; k < S; k += 8) s += src[(size_t)k * total + i];
  sh[z][o] = s;
  __syncthreads();
  if (z == 0 && i < total) {
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) r += sh[k][o];
    r = round_kind(r, rkind);  // mixed precision: the gradient of a weight autocast cast to half arrives in half
    if (bias_part) {
      db[i] = r;
    } else {
      const int row = (int)(i / N), col = (int)(i % N);
      C[(size_t)row * ldc + col] = r;
    }
  }
}

__global__ void transpose_kernel(const float* __restrict__ in, int ldi, int R, int Cn, float* __restrict__ out, int ldo) {
  __shared__ float t[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, cc = c0 + tx;
    t[j][tx] = (r < R && cc < Cn) ? in[(size_t)r * ldi + cc] : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int cc = c0 + j, r = r0 + tx;
    if (cc < Cn && r < R) out[(size_t)cc * ldo + r] = t[tx][j];
  }
}

// stage kernel of the column reduction: block (bx, by) sums rows [by*rows_per, ...) of the 64-column strip bx of
// X (* Y).  256 threads = 64 columns x 4 row lanes, 4 independent partial sums per thread (memory-level parallelism),
// combined in a fixed order.
__global__ __launch_bounds__(256) void colreduce_kernel(const float* __restrict__ X, const float* __restrict__ Y, int ld, int M, int N,
                                                         int rows_per, float* __restrict__ out /* [gridDim.y][N] */) {
  __shared__ float sh[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + tx;
  const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < N) {
    int r = r0 + ty;
    if (Y) {
      for (; r + 12 < r1; r += 16) {
        s0 = fmaf(X[(size_t)r * ld + col], Y[(size_t)r * ld + col], s0);
        s1 = fmaf(X[(size_t)(r + 4) * ld + col], Y[(size_t)(r + 4) * ld + col], s1);
        s2 = fmaf(X[(size_t)(r + 8) * ld + col], Y[(size_t)(r + 8) * ld + col], s2);
        s3 = fmaf(X[(size_t)(r + 12) * ld + col], Y[(size_t)(r + 12) * ld + col], s3);
      }
      for (; r < r1; r += 4) s0 = fmaf(X[(size_t)r * ld + col], Y[(size_t)r * ld + col], s0);
    } else {
      for (; r + 12 < r1; r += 16) {
        s0 += X[(size_t)r * ld + col];
        s1 += X[(size_t)(r + 4) * ld + col];
        s2 += X[(size_t)(r + 8) * ld + col];
        s3 += X[(size_t)(r + 12) * ld + col];
      }
      for (; r < r1; r += 4) s0 += X[(size_t)r * ld + col];
    }
  }
  sh[ty][tx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ty == 0 && col < N) out[(size_t)blockIdx.y * N + col] = (sh[0][tx] + sh[1][tx]) + (sh[2][tx] + sh[3][tx]);
}

// ------------------------------------------------------------------------------------------------------------------
// LayerNorm (+ReLU), one wave per row, F <= 1024.  Lane holds features lane, lane+64, ...
// ------------------------------------------------------------------------------------------------------------------
constexpr int LN_MAXJ = 16;   // (rows per wave in the backward, MDX_LN_RPW: mdx_train_plan.h)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(256) void ln_relu_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int M, int F, int relu,
                                                           float* __restrict__ y, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int J = (F + 63) >> 6;
  float v[LN_MAXJ];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < LN_MAXJ; ++j) {
    const int f = lane + 64 * j;
    v[j] = (j < J && f < F) ? x[(size_t)row * F + f] : 0.f;
    s += v[j];
  }
  const float mean = wave_sum(s) / (float)F;
  float d2 = 0.f;
#pragma unroll
  for (int j = 0; j < LN_MAXJ; ++j) {
    const int f = lane + 64 * j;
    if (j < J && f < F) {
      const float d = v[j] - mean;
      d2 = fmaf(d, d, d2);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(d2) / (float)F + MDX_LN_EPS);
#pragma unroll
  for (int j = 0; j < LN_MAXJ; ++j) {
    const int f = lane + 64 * j;
    if (j < J && f < F) {
      const float o = (v[j] - mean) * rstd * gamma[f] + beta[f];
      y[(size_t)row * F + f] = relu ? fmaxf(o, 0.f) : o;
    }
  }
  if (lane == 0) {
    stats[2 * (size_t)row] = mean;
    stats[2 * (size_t)row + 1] = rstd;
  }
}

// The four waves' partials of [dgamma | dbeta] (ln_sh[4][2F], dynamic LDS) -> ONE partial row per workgroup, waves added in the fixed
// order ((0 + 1) + 2) + 3.  (Round 5: per-wave rows were 8 % of the backward's traffic and, read back, most of the deferred reduction's.)
extern __shared__ __attribute__((aligned(16))) float ln_sh[];
__device__ __forceinline__ void ln_part_combine(const float* sh, int F, float* __restrict__ row) {
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * F; i += 256) row[i] = ((sh[i] + sh[2 * F + i]) + sh[4 * F + i]) + sh[6 * F + i];
}

// each wave walks `rows_per` consecutive rows: dx per row, and its own partial of dgamma / dbeta (registers); the workgroup's four
// partials are combined and written to part[blockIdx.x][2F] (dgamma first); the caller column-reduces `part`.
__global__ __launch_bounds__(256) void ln_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ stats, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int M, int F, int relu, int rows_per,
                                                           float* __restrict__ dx, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int wg = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int r0 = wg * rows_per, r1 = min(M, r0 + rows_per);
  const int J = (F + 63) >> 6;
  float gm[LN_MAXJ], bt[LN_MAXJ], dg[LN_MAXJ], db[LN_MAXJ];
#pragma unroll
  for (int j = 0; j < LN_MAXJ; ++j) {
    const int f = lane + 64 * j;
    const bool ok = j < J && f < F;
    gm[j] = ok ? gamma[f] : 0.f;
    bt[j] = ok ? beta[f] : 0.f;
    dg[j] = db[j] = 0.f;
  }
  for (int row = r0; row < r1; ++row) {
    const float mean = stats[2 * (size_t)row], rstd = stats[2 * (size_t)row + 1];
    float xh[LN_MAXJ], gh[LN_MAXJ];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
      const int f = lane + 64 * j;
      xh[j] = gh[j] = 0.f;
      if (j < J && f < F) {
        xh[j] = (x[(size_t)row * F + f] - mean) * rstd;
        float g = dy[(size_t)row * F + f];
        if (relu && !(xh[j] * gm[j] + bt[j] > 0.f)) g = 0.f;
        dg[j] = fmaf(g, xh[j], dg[j]);
        db[j] += g;
        gh[j] = g * gm[j];
        s1 += gh[j];
        s2 = fmaf(gh[j], xh[j], s2);
      }
    }
    const float m1 = wave_sum(s1) / (float)F, m2 = wave_sum(s2) / (float)F;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
      const int f = lane + 64 * j;
      if (j < J && f < F) dx[(size_t)row * F + f] = rstd * (gh[j] - m1 - xh[j] * m2);
    }
  }
#pragma unroll
  for (int j = 0; j < LN_MAXJ; ++j) {
    const int f = lane + 64 * j;
    if (j < J && f < F) {
      ln_sh[(threadIdx.x >> 6) * 2 * F + f] = dg[j];
      ln_sh[(threadIdx.x >> 6) * 2 * F + F + f] = db[j];
    }
  }
  ln_part_combine(ln_sh, F, part + (size_t)blockIdx.x * 2 * F);
}


// ---- vectorised LayerNorm for the widths the networks use (F = 32, 64, 128, 256): a row is F/4 lanes x float4, a wave covers
// 64 / (F/4) rows per step; the row sums are DPP / permlane butterflies over the row's lanes (the generic kernels above spend
// twelve ds_bpermute round trips per row and a whole wave per row whatever its width).
template <int LPR>  // lanes per row: 8, 16, 32, 64
__device__ __forceinline__ float row_lanes_sum(float v) {
  auto dpp = [](float x, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, false));
  };
  v += dpp(v, std::integral_constant<int, 0xB1>{});   // quad_perm [1,0,3,2]
  v += dpp(v, std::integral_constant<int, 0x4E>{});   // quad_perm [2,3,0,1]
  v += dpp(v, std::integral_constant<int, 0x141>{});  // row_half_mirror: + the other quad of the 8-lane group
  if (LPR >= 16) v += dpp(v, std::integral_constant<int, 0x140>{});  // row_mirror: + the other half of the 16-lane row
  if (LPR >= 32) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  }
  if (LPR >= 64) {
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(b[0]) + __uint_as_float(b[1]);
  }
  return v;
}

template <int LPR>
__global__ __launch_bounds__(256) void ln_relu_fwd4_kernel(const TP x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int M, int relu, const TPW y,
                                                            float* __restrict__ stats) {
  constexpr int F = 4 * LPR, RPS = 64 / LPR;
  const int lane = threadIdx.x & 63, wg = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int row = wg * RPS + lane / LPR, c4 = lane % LPR;
  const bool ok = row < M;
  const f32x4 v = ok ? ld4(x, (size_t)row * F + 4 * c4) : splat4(0.f);
  const float mean = row_lanes_sum<LPR>((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / F);
  const f32x4 d = v - splat4(mean);
  const float rstd = 1.0f / sqrtf(row_lanes_sum<LPR>(fmaf(d[0], d[0], fmaf(d[1], d[1], fmaf(d[2], d[2], d[3] * d[3])))) * (1.0f / F) + MDX_LN_EPS);
  if (!ok) return;
  const f32x4 gmv = {gamma[4 * c4], gamma[4 * c4 + 1], gamma[4 * c4 + 2], gamma[4 * c4 + 3]};  // (parameters: any 4-byte offset)
  const f32x4 btv = {beta[4 * c4], beta[4 * c4 + 1], beta[4 * c4 + 2], beta[4 * c4 + 3]};
  f32x4 o = d * splat4(rstd) * gmv + btv;
  if (relu) o = relu4(o);
  st4(y, (size_t)row * F + 4 * c4, o);
  if (c4 == 0) {
    stats[2 * (size_t)row] = mean;
    stats[2 * (size_t)row + 1] = rstd;
  }
}

// backward: a wave walks `steps` consecutive row groups; dx per row; the workgroup's partial of dgamma / dbeta -> part[blockIdx.x][2F]
// r1w != NULL (round 6): the upstream gradient is the rank-1 product dy[row][c] = f16(g1[row] * f16(r1w[c])) -- the data gradient of a
// Linear to ONE output (PosUpdate's 256 -> 1) that follows this LayerNorm; dy.p then holds g1 (M values), and the (M,F) gradient
// tensor, the K = 1 GEMM that formed it and the transpose of its weight never exist.
template <int LPR>
__global__ __launch_bounds__(256) void ln_relu_bwd4_kernel(const TP dy, const TP x,
                                                            const float* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int M, int relu, int rows_per,
                                                            const TPW dx, float* __restrict__ part, const float* __restrict__ r1w = nullptr) {
  constexpr int F = 4 * LPR, RPS = 64 / LPR;
  const int lane = threadIdx.x & 63, wg = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int sub = lane / LPR, c4 = lane % LPR;
  const int r0 = wg * rows_per, r1 = min(M, r0 + rows_per);
  const f32x4 gm = {gamma[4 * c4], gamma[4 * c4 + 1], gamma[4 * c4 + 2], gamma[4 * c4 + 3]};  // (parameters: any 4-byte offset)
  const f32x4 bt = {beta[4 * c4], beta[4 * c4 + 1], beta[4 * c4 + 2], beta[4 * c4 + 3]};
  f32x4 w1 = splat4(0.f);
  if (r1w) w1 = f32x4{round_half<1>(r1w[4 * c4]), round_half<1>(r1w[4 * c4 + 1]), round_half<1>(r1w[4 * c4 + 2]), round_half<1>(r1w[4 * c4 + 3])};
  f32x4 dg = splat4(0.f), db = splat4(0.f);
#ifndef MDX_LNB_UNROLL
#define MDX_LNB_UNROLL 2
#endif
#pragma unroll MDX_LNB_UNROLL
  for (int rb = r0; rb < r1; rb += RPS) {
    const int row = rb + sub;
    const bool ok = row < r1;
    const size_t o = (size_t)(ok ? row : r0) * F + 4 * c4;
    const float mean = stats[2 * (size_t)(ok ? row : r0)], rstd = stats[2 * (size_t)(ok ? row : r0) + 1];
    const f32x4 xh = (ld4(x, o) - splat4(mean)) * splat4(rstd);
    f32x4 g = splat4(0.f);
    if (r1w) {
      if (ok) {
        const float gv = round_half<1>(ld1(dy, (size_t)row));
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = round_half<1>(gv * w1[k]);
      }
    } else if (ok) {
      g = ld4(dy, o);
    }
    if (relu) {
      const f32x4 yv = xh * gm + bt;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (!(yv[k] > 0.f)) g[k] = 0.f;
    }
    dg = dg + g * xh;
    db = db + g;
    const f32x4 gh = g * gm;
    const float m1 = row_lanes_sum<LPR>((gh[0] + gh[1]) + (gh[2] + gh[3])) * (1.0f / F);
    const float m2 = row_lanes_sum<LPR>(fmaf(gh[0], xh[0], fmaf(gh[1], xh[1], fmaf(gh[2], xh[2], gh[3] * xh[3])))) * (1.0f / F);
    if (ok) st4(dx, o, (gh - splat4(m1) - xh * splat4(m2)) * splat4(rstd));
  }
  // the 64 / LPR row groups of the wave hold the same features: combine them (lane bits >= LPR), then the first group writes
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float a = dg[k], b = db[k];
    if (LPR <= 8) {  // + lanes ^ 8 (row_ror:8 within the 16-lane row)
      a += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x128, 0xf, 0xf, false));
      b += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(b), 0x128, 0xf, 0xf, false));
    }
    if (LPR <= 16) {
      const auto sa = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
      const auto sb = __builtin_amdgcn_permlane16_swap(__float_as_uint(b), __float_as_uint(b), false, false);
      a = __uint_as_float(sa[0]) + __uint_as_float(sa[1]);
      b = __uint_as_float(sb[0]) + __uint_as_float(sb[1]);
    }
    if (LPR <= 32) {
      const auto sa = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(a), false, false);
      const auto sb = __builtin_amdgcn_permlane32_swap(__float_as_uint(b), __float_as_uint(b), false, false);
      a = __uint_as_float(sa[0]) + __uint_as_float(sa[1]);
      b = __uint_as_float(sb[0]) + __uint_as_float(sb[1]);
    }
    dg[k] = a;
    db[k] = b;
  }
  if (sub == 0) {
    float* w = ln_sh + (threadIdx.x >> 6) * 2 * F;
    *reinterpret_cast<f32x4*>(w + 4 * c4) = dg;
    *reinterpret_cast<f32x4*>(w + F + 4 * c4) = db;
  }
  ln_part_combine(ln_sh, F, part + (size_t)blockIdx.x * 2 * F);
}

// ------------------------------------------------------------------------------------------------------------------
// element-wise pairs.  op: 0 add, 1 sub, 2 mul, 3 gate (a * sigmoid(b))
// ------------------------------------------------------------------------------------------------------------------
// opr = op | (rkind << 8): rkind != 0 rounds the result (and the sigmoid of the gate) to bfloat16 / float16 -- the value the
// reference's fp16 tensors hold under autocast (both factors of these products are Linear outputs there)
template <typename V>
__device__ __forceinline__ V ew_apply(int op, V x, V y);
template <>
__device__ __forceinline__ f32x4 ew_apply<f32x4>(int op, f32x4 x, f32x4 y) {
  switch (op) {
    case 0: return x + y;
    case 1: return x - y;
    case 2: return x * y;
    default: return x * sigmoid4(y);
  }
}
__global__ void ew_fwd4_kernel(int opr, const TP a, const TP b, const TPW o, size_t n4) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const int op = opr & 255, rk = opr >> 8;
  const f32x4 x = ld4(a, 4 * i), y = ld4(b, 4 * i);
  if (rk == 0) {
    st4(o, 4 * i, ew_apply<f32x4>(op, x, y));
    return;
  }
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v = op == 0 ? x[j] + y[j] : op == 1 ? x[j] - y[j] : op == 2 ? x[j] * y[j] : x[j] * round_kind(sigmoidf_(y[j]), rk);
    r[j] = round_kind(v, rk);
  }
  st4(o, 4 * i, r);
}
// out = sum of up to 12 tensors of one shape (round 6): the gradient of a tensor with several consumers.  autograd would add the
// consumers' gradients pairwise (k - 1 launches of an element-wise add, each rounding to the container); here they are summed in
// fp32 in argument order and rounded ONCE.  Operands fp32 or float16 containers, 4 elements per thread.
struct SumN {
  const void* p[12];
  int h[12];
  int n;
};
__global__ void sum_n4_kernel(const SumN a, const TPW o, size_t n4) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  f32x4 s = ld4(TP{a.p[0], a.h[0]}, 4 * i);
  for (int j = 1; j < a.n; ++j) s = s + ld4(TP{a.p[j], a.h[j]}, 4 * i);
  st4(o, 4 * i, s);
}
__global__ void sum_n1_kernel(const SumN a, const TPW o, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = ld1(TP{a.p[0], a.h[0]}, i);
  for (int j = 1; j < a.n; ++j) s += ld1(TP{a.p[j], a.h[j]}, i);
  st1(o, i, s);
}
// any length / alignment, fp32 or float16 containers (round 6: an (E,1) gate product has E % 4 != 0 and used to go through two casts to
// fp32 and back); also what an unaligned or odd-length fp32 tensor takes
__global__ void ew_fwd1_kernel(int opr, const TP a, const TP b, const TPW o, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int op = opr & 255, rk = opr >> 8;
  const float x = ld1(a, i), y = ld1(b, i);
  const float v = op == 0 ? x + y : op == 1 ? x - y : op == 2 ? x * y : x * round_kind(sigmoidf_(y), rk);
  st1(o, i, round_kind(v, rk));
}
__global__ void ew_bwd1_kernel(int op, const TP a, const TP b, const TP g, const TPW da, const TPW db, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gv = ld1(g, i);
  float ga, gb;
  if (op == 0) { ga = gv; gb = gv; }
  else if (op == 1) { ga = gv; gb = -gv; }
  else if (op == 2) { ga = gv * ld1(b, i); gb = gv * ld1(a, i); }
  else { const float sg = sigmoidf_(ld1(b, i)); ga = gv * sg; gb = gv * ld1(a, i) * sg * (1.0f - sg); }
  if (da.p) st1(da, i, ga);
  if (db.p) st1(db, i, gb);
}
__global__ void ew_bwd4_kernel(int op, const TP a, const TP b, const TP g, const TPW da, const TPW db, size_t n4) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const f32x4 go = ld4(g, 4 * i);
  f32x4 ga, gb;
  switch (op) {
    case 0: ga = go; gb = go; break;
    case 1: ga = go; gb = splat4(0.f) - go; break;
    case 2: ga = go * ld4(b, 4 * i); gb = go * ld4(a, 4 * i); break;
    default: {
      const f32x4 sg = sigmoid4(ld4(b, 4 * i));
      ga = go * sg;
      gb = go * ld4(a, 4 * i) * sg * (splat4(1.f) - sg);
    }
  }
  if (da.p) st4(da, 4 * i, ga);
  if (db.p) st4(db, 4 * i, gb);
}

// y[i] = x[idx[i]]  (rows of F floats)
__global__ void gather_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx, int64_t M, int F,
                                   float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * F) return;
  const int64_t row = i / F;
  const int f = (int)(i % F);
  y[i] = x[(size_t)idx[row] * F + f];
}
// 16-byte variants (F % 4 == 0, 16-byte aligned bases): one thread per (row, 4 features)
__global__ void gather_rows4_kernel(const TP x, const int64_t* __restrict__ idx, int64_t M, int F4, const TPW y) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * F4) return;
  const int64_t row = i / F4;
  st4(y, 4 * i, ld4(x, 4 * ((size_t)idx[row] * F4 + (int)(i % F4))));
}
__global__ void segsum_rows4_kernel(const TP src, const int64_t* __restrict__ order, const int64_t* __restrict__ ptr,
                                    int64_t R, int F4, const TPW out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)R * F4) return;
  const int64_t r = i / F4;
  const int f = (int)(i % F4);
  f32x4 s = splat4(0.f);
  // four rows in flight (round 6): the loop was one dependent index load + one row load per iteration -- latency-bound at ~25 rows
  // per node (30 us for 79 MB).  The additions keep their order (s + v0) + v1 ...: bit-identical sums.
  int64_t j = ptr[r];
  const int64_t e = ptr[r + 1];
  for (; j + 4 <= e; j += 4) {
    const int64_t o0 = order[j], o1 = order[j + 1], o2 = order[j + 2], o3 = order[j + 3];
    const f32x4 v0 = ld4(src, 4 * ((size_t)o0 * F4 + f)), v1 = ld4(src, 4 * ((size_t)o1 * F4 + f));
    const f32x4 v2 = ld4(src, 4 * ((size_t)o2 * F4 + f)), v3 = ld4(src, 4 * ((size_t)o3 * F4 + f));
    s = s + v0;
    s = s + v1;
    s = s + v2;
    s = s + v3;
  }
  for (; j < e; ++j) s = s + ld4(src, 4 * ((size_t)order[j] * F4 + f));
  st4(out, 4 * i, s);
}
// The same sum with a segment's rows dealt to FOUR threads (round 6): thread k of an output element takes rows k, k + 4, ... of the segment
// (four in flight each: sixteen row gathers per element instead of four), the four partial sums are combined through LDS in the fixed
// order ((p0 + p1) + p2) + p3.  A node has ~28 rows; with one thread per element the kernel ran seven dependent gather rounds at ten
// waves per CU (25 us for 20-80 MB).  Deterministic; NOT the summation order of segsum_rows4_kernel: used for float16 rows (the autocast
// mode), fp32 rows keep the sequential order (see mdx_op_segsum_rows_t).
__global__ __launch_bounds__(256) void segsum_rows4s_kernel(const TP src, const int64_t* __restrict__ order, const int64_t* __restrict__ ptr,
                                                            int64_t R, int F4, const TPW out) {
  __shared__ f32x4 part[3][64];
  const int k = threadIdx.x >> 6, it = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * 64 + it;
  const bool live = i < (size_t)R * F4;
  f32x4 s = splat4(0.f);
  if (live) {
    const int64_t r = i / F4;
    const int f = (int)(i % F4);
    int64_t j = ptr[r] + k;
    const int64_t e = ptr[r + 1];
    for (; j + 12 < e; j += 16) {
      const int64_t o0 = order[j], o1 = order[j + 4], o2 = order[j + 8], o3 = order[j + 12];
      const f32x4 v0 = ld4(src, 4 * ((size_t)o0 * F4 + f)), v1 = ld4(src, 4 * ((size_t)o1 * F4 + f));
      const f32x4 v2 = ld4(src, 4 * ((size_t)o2 * F4 + f)), v3 = ld4(src, 4 * ((size_t)o3 * F4 + f));
      s = s + v0;
      s = s + v1;
      s = s + v2;
      s = s + v3;
    }
    for (; j < e; j += 4) s = s + ld4(src, 4 * ((size_t)order[j] * F4 + f));
  }
  if (k) part[k - 1][it] = s;
  __syncthreads();
  if (k == 0 && live) {
    s = s + part[0][it];
    s = s + part[1][it];
    s = s + part[2][it];
    st4(out, 4 * i, s);
  }
}
// CSR order of the RIGHT end points from that of the LEFT ones when the directed edge list is [half-edges ; flipped half-edges]
// (reference models/model.py:269, :143: edge_index = cat([he, he.flip(0)], 1)): right[i] = left[(i + Eh) mod E], so both index vectors
// hold the same multiset (same segment starts) and the stable order of `right` inside a node's segment is: the entries j >= Eh of
// the left order (as j - Eh, ascending), then the entries j < Eh (as j + Eh).  One thread per node; replaces a second stable sort
// (11 launches of torch.sort + searchsorted) per training step.
__global__ void plan_flip_kernel(const int64_t* __restrict__ order_l, const int64_t* __restrict__ ptr, int64_t R, int64_t Eh,
                                 int64_t* __restrict__ order_r) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t b = ptr[r], e = ptr[r + 1];
  int64_t c = b;                       // first position whose entry is >= Eh (entries ascend inside a segment)
  while (c < e && order_l[c] < Eh) ++c;
  int64_t w = b;
  for (int64_t j = c; j < e; ++j) order_r[w++] = order_l[j] - Eh;
  for (int64_t j = b; j < c; ++j) order_r[w++] = order_l[j] + Eh;
}
// The same with EIGHT float16 features per thread (one 16-byte load per row; F % 8 == 0, float16 rows, 16-byte aligned): the sums per
// feature and their order are those of segsum_rows4s_kernel (bit-identical), half the threads and load instructions.
__global__ __launch_bounds__(256) void segsum_rows8s_kernel(const _Float16* __restrict__ src, const int64_t* __restrict__ order,
                                                            const int64_t* __restrict__ ptr, int64_t R, int F8, const TPW out) {
  __shared__ f32x4 part[3][2][64];
  const int k = threadIdx.x >> 6, it = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * 64 + it;
  const bool live = i < (size_t)R * F8;
  f32x4 s0 = splat4(0.f), s1 = splat4(0.f);
  auto ld8 = [&](int64_t o, int f, f32x4& a, f32x4& b) {
    const uint4 u = *reinterpret_cast<const uint4*>(src + 8 * ((size_t)o * F8 + f));
    const f16x4_t lo = __builtin_bit_cast(f16x4_t, uint2{u.x, u.y}), hi = __builtin_bit_cast(f16x4_t, uint2{u.z, u.w});
    a = f32x4{(float)lo[0], (float)lo[1], (float)lo[2], (float)lo[3]};
    b = f32x4{(float)hi[0], (float)hi[1], (float)hi[2], (float)hi[3]};
  };
  if (live) {
    const int64_t r = i / F8;
    const int f = (int)(i % F8);
    int64_t j = ptr[r] + k;
    const int64_t e = ptr[r + 1];
    for (; j + 12 < e; j += 16) {
      const int64_t o0 = order[j], o1 = order[j + 4], o2 = order[j + 8], o3 = order[j + 12];
      f32x4 a0, b0, a1, b1, a2, b2, a3, b3;
      ld8(o0, f, a0, b0);
      ld8(o1, f, a1, b1);
      ld8(o2, f, a2, b2);
      ld8(o3, f, a3, b3);
      s0 = s0 + a0; s1 = s1 + b0;
      s0 = s0 + a1; s1 = s1 + b1;
      s0 = s0 + a2; s1 = s1 + b2;
      s0 = s0 + a3; s1 = s1 + b3;
    }
    for (; j < e; j += 4) {
      f32x4 a, b;
      ld8(order[j], f, a, b);
      s0 = s0 + a; s1 = s1 + b;
    }
  }
  if (k) part[k - 1][0][it] = s0, part[k - 1][1][it] = s1;
  __syncthreads();
  if (k == 0 && live) {
    s0 = s0 + part[0][0][it]; s1 = s1 + part[0][1][it];
    s0 = s0 + part[1][0][it]; s1 = s1 + part[1][1][it];
    s0 = s0 + part[2][0][it]; s1 = s1 + part[2][1][it];
    st4(out, 8 * i, s0);
    st4(out, 8 * i + 4, s1);
  }
}
// y[i] = a[i] * t[idx[i]] and its two gradients (da = g * t[idx];  dt[r] = sum_{j in seg r} g[order[j]] * a[order[j]]):
// the product with a gathered per-node row without materialising the gathered (rows x F) tensor.  F % 4 == 0.
__global__ void mulg_fwd_kernel(const TP a, const TP t, const int64_t* __restrict__ idx, int64_t M, int F4, const TPW y, int rk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * F4) return;
  const int64_t row = i / F4;
  const f32x4 tv = ld4(t, 4 * ((size_t)idx[row] * F4 + (int)(i % F4)));
  f32x4 r = ld4(a, 4 * i) * tv;      // forward: a * t[idx];  backward wrt a: g * t[idx] (the caller passes g as `a`)
  if (rk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = round_kind(r[j], rk);
  }
  st4(y, 4 * i, r);
}
__global__ void mulg_segsum_kernel(const TP g, const TP a, const int64_t* __restrict__ order,
                                   const int64_t* __restrict__ ptr, int64_t R, int F4, const TPW out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)R * F4) return;
  const int64_t r = i / F4;
  const int f = (int)(i % F4);
  f32x4 s = splat4(0.f);
  int64_t j = ptr[r];
  const int64_t e = ptr[r + 1];
  for (; j + 2 <= e; j += 2) {   // two rows in flight, additions in the same order
    const size_t o0 = 4 * ((size_t)order[j] * F4 + f), o1 = 4 * ((size_t)order[j + 1] * F4 + f);
    const f32x4 g0 = ld4(g, o0), a0 = ld4(a, o0), g1 = ld4(g, o1), a1 = ld4(a, o1);
    s = s + g0 * a0;
    s = s + g1 * a1;
  }
  for (; j < e; ++j) {
    const size_t o = 4 * ((size_t)order[j] * F4 + f);
    s = s + ld4(g, o) * ld4(a, o);
  }
  st4(out, 4 * i, s);
}
// out[r] = sum_{j in [ptr[r], ptr[r+1])} src[order[j]]   (sequential per element: bitwise deterministic)
__global__ void segsum_rows_kernel(const float* __restrict__ src, const int64_t* __restrict__ order, const int64_t* __restrict__ ptr,
                                   int64_t R, int F, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)R * F) return;
  const int64_t r = i / F;
  const int f = (int)(i % F);
  float s = 0.f;
  for (int64_t j = ptr[r]; j < ptr[r + 1]; ++j) s += src[(size_t)order[j] * F + f];
  out[i] = s;
}

// The scalar form dealt to four threads per element (round 6; any F, fp32): the (E,3) force / position-gradient sums of the float16
// mode ran one thread per (node, xyz) -- 19k threads, 28 dependent gathers each, 20 us per launch, 16 launches a step.  Only when the
// caller allows another summation order (dt bit 2 of mdx_op_segsum_rows_t: the autocast mode; fp32 training keeps the sequential
// order of the reference's index_add).
__global__ __launch_bounds__(256) void segsum_rows1s_kernel(const float* __restrict__ src, const int64_t* __restrict__ order,
                                                            const int64_t* __restrict__ ptr, int64_t R, int F, float* __restrict__ out) {
  __shared__ float part[3][64];
  const int k = threadIdx.x >> 6, it = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * 64 + it;
  const bool live = i < (size_t)R * F;
  float s = 0.f;
  if (live) {
    const int64_t r = i / F;
    const int f = (int)(i % F);
    int64_t j = ptr[r] + k;
    const int64_t e = ptr[r + 1];
    for (; j + 12 < e; j += 16) {
      const int64_t o0 = order[j], o1 = order[j + 4], o2 = order[j + 8], o3 = order[j + 12];
      const float v0 = src[(size_t)o0 * F + f], v1 = src[(size_t)o1 * F + f], v2 = src[(size_t)o2 * F + f], v3 = src[(size_t)o3 * F + f];
      s += v0;
      s += v1;
      s += v2;
      s += v3;
    }
    for (; j < e; j += 4) s += src[(size_t)order[j] * F + f];
  }
  if (k) part[k - 1][it] = s;
  __syncthreads();
  if (k == 0 && live) out[i] = ((s + part[0][it]) + part[1][it]) + part[2][it];
}

// ------------------------------------------------------------------------------------------------------------------
// edge geometry / smearing / force (reference models/graph.py:349-352, common.py GaussianSmearing, graph.py:391-394)
// ------------------------------------------------------------------------------------------------------------------
__global__ void edge_geom_fwd_kernel(const float* __restrict__ pos, const int64_t* __restrict__ l, const int64_t* __restrict__ r,
                                     int64_t E, float* __restrict__ rel, float* __restrict__ dist) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t a = l[e], b = r[e];
  const float dx = pos[3 * a] - pos[3 * b], dy = pos[3 * a + 1] - pos[3 * b + 1], dz = pos[3 * a + 2] - pos[3 * b + 2];
  rel[3 * e] = dx; rel[3 * e + 1] = dy; rel[3 * e + 2] = dz;
  dist[e] = sqrtf(dx * dx + dy * dy + dz * dz);
}
// g[e] = drel[e] + ddist[e] * rel[e] / dist[e]   (d|v|/dv = v/|v|; the reference's torch.norm has the 0/0 -> nan there too)
__global__ void edge_geom_bwd_kernel(const float* __restrict__ rel, const float* __restrict__ dist, const float* __restrict__ drel,
                                     const float* __restrict__ ddist, int64_t E, float* __restrict__ g) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float k = ddist ? ddist[e] / dist[e] : 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) g[3 * e + j] = (drel ? drel[3 * e + j] : 0.f) + k * rel[3 * e + j];
}
__global__ void smear_fwd_kernel(const float* __restrict__ d, const float* __restrict__ off, const float* __restrict__ coef, int G,
                                 float lo, float hi, int64_t E, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)E * G) return;
  const int64_t e = i / G;
  const int k = (int)(i % G);
  const float u = fminf(fmaxf(d[e], lo), hi) - off[k];
  out[i] = expf(coef[k] * (u * u));
}
__global__ void smear_bwd_kernel(const float* __restrict__ d, const float* __restrict__ off, const float* __restrict__ coef, int G,
                                 float lo, float hi, int64_t E, const float* __restrict__ gout, float* __restrict__ gd) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float dv = d[e];
  float s = 0.f;
  if (dv >= lo && dv <= hi) {  // clamp passes the gradient on the closed interval (torch.clamp semantics)
    for (int k = 0; k < G; ++k) {
      const float u = dv - off[k];
      s += gout[(size_t)e * G + k] * expf(coef[k] * (u * u)) * 2.0f * coef[k] * u;
    }
  }
  gd[e] = s;
}
// F = w * rel / d / (d + 1)
__global__ void force_fwd_kernel(const float* __restrict__ w, const float* __restrict__ rel, const float* __restrict__ d, int64_t E,
                                 float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float dv = d[e], dp = dv + 1.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[3 * e + j] = w[e] * rel[3 * e + j] / dv / dp;
}
__global__ void force_bwd_kernel(const float* __restrict__ w, const float* __restrict__ rel, const float* __restrict__ d,
                                 const float* __restrict__ g, int64_t E, float* __restrict__ gw, float* __restrict__ grel,
                                 float* __restrict__ gd) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float dv = d[e], dp = dv + 1.0f, wv = w[e];
  const float inv = 1.0f / (dv * dp);
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    dot = fmaf(g[3 * e + j], rel[3 * e + j], dot);
    grel[3 * e + j] = g[3 * e + j] * wv * inv;
  }
  gw[e] = dot * inv;
  // d/dd [1/(d (d+1))] = -(2d + 1) / (d (d+1))^2
  gd[e] = -wv * dot * (2.0f * dv + 1.0f) * inv * inv;
}

// ------------------------------------------------------------------------------------------------------------------
// optimizer step on the flat parameter buffer (torch.optim.AdamW semantics, utils/train.py:64-70 of the reference):
//   sumsq   : sum of squares of the flat gradient in two fixed-order stages (-> global norm for clip_grad_norm_)
//   adamw   : g *= gscale ; p *= 1 - lr*wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
//             p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, size_t n, float* __restrict__ out) {
  __shared__ float sh[4];
  const size_t per = ((n + gridDim.x - 1) / gridDim.x + 1023) / 1024 * 1024;
  const size_t i0 = min(n, (size_t)blockIdx.x * per), i1 = min(n, i0 + per);
  float s = 0.f;
  if ((per & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    // 16-byte loads, four in flight per thread (round 6: one scalar load in flight made the 40 MB gradient norm a 107-us kernel)
    f32x4 a0 = splat4(0.f), a1 = splat4(0.f), a2 = splat4(0.f), a3 = splat4(0.f);
    size_t i = i0 + 4 * (size_t)threadIdx.x;
    for (; i + 3 * 1024 + 3 < i1; i += 4096) {
      const f32x4 v0 = ldg4(x + i), v1 = ldg4(x + i + 1024), v2 = ldg4(x + i + 2048), v3 = ldg4(x + i + 3072);
      a0 = a0 + v0 * v0, a1 = a1 + v1 * v1, a2 = a2 + v2 * v2, a3 = a3 + v3 * v3;
    }
    for (; i + 3 < i1; i += 1024) {
      const f32x4 v = ldg4(x + i);
      a0 = a0 + v * v;
    }
    for (; i < i1; ++i) s = fmaf(x[i], x[i], s);     // (at most three elements of the buffer's tail, in the last block's last lane)
    const f32x4 a = (a0 + a1) + (a2 + a3);
    s += (a[0] + a[1]) + (a[2] + a[3]);
  } else {
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) s = fmaf(x[i], x[i], s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__global__ void sum_small_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += x[i];
    out[0] = s;
  }
}
// gnorm2: device scalar holding the squared global gradient norm (or NULL = no clipping)
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             size_t n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                             const float* __restrict__ gnorm2, float max_norm) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float gs = 1.0f;
  if (gnorm2) {
    // a non-finite gradient norm skips the whole update, like GradScaler / the reference's try-except around the
    // iteration (scripts/train_drug3d.py:93-119): fminf(NaN, 1) would be 1 and write NaNs into p, m and v for good
    if (!isfinite(gnorm2[0])) return;
    gs = fminf(max_norm / (sqrtf(gnorm2[0]) + 1e-6f), 1.0f);
  }
  const float gi = g[i] * gs;
  float pi = p[i] * (1.0f - lr * wd);
  const float mi = b1 * m[i] + (1.0f - b1) * gi;
  const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  pi -= (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
  p[i] = pi;
}

// ---- GradScaler-equivalent step with its state on the device (scripts/train_drug3d.py:105-109: scaler.scale(loss).backward(),
// unscale_, clip_grad_norm_, scaler.step, scaler.update) ----
// state: [0] loss scale S  [1] growth tracker  [2] optimizer steps taken  [3] steps skipped  [4] unscaled squared gradient norm of the
//        last step (inf / nan when a gradient overflowed)  [5] apply flag  [6] gradient multiplier (1/S x clip factor)  [7] 1 - b1^t
//        [8] sqrt(1 - b2^t)
constexpr int AMP_STATE = 16;
__global__ void amp_decide_kernel(const float* __restrict__ part, int nparts, float* __restrict__ st, float b1, float b2, float max_norm,
                                  float growth, float backoff, int growth_interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float tot = 0.f;
  for (int i = 0; i < nparts; ++i) tot += part[i];
  const float S = st[0], inv = 1.0f / S;
  const float n2 = tot * inv * inv;
  st[4] = n2;
  if (isfinite(n2)) {
    const float t = st[2] + 1.0f;
    st[2] = t;
    st[5] = 1.0f;
    st[6] = inv * fminf(max_norm / (sqrtf(n2) + 1e-6f), 1.0f);
    st[7] = 1.0f - powf(b1, t);
    st[8] = sqrtf(1.0f - powf(b2, t));
    const float tr = st[1] + 1.0f;
    if (growth_interval > 0 && tr >= (float)growth_interval) {
      st[0] = S * growth;
      st[1] = 0.f;
    } else {
      st[1] = tr;
    }
  } else {  // found_inf: the optimizer does not step (its step count and moments stay), the scale backs off
    st[5] = 0.f;
    st[3] += 1.0f;
    st[0] = S * backoff;
    st[1] = 0.f;
  }
}
__global__ void adamw_amp_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n,
                                 float lr, float b1, float b2, float eps, float wd, const float* __restrict__ st) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || st[5] == 0.f) return;
  const float gi = g[i] * st[6];
  float pi = p[i] * (1.0f - lr * wd);
  const float mi = b1 * m[i] + (1.0f - b1) * gi;
  const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  pi -= (lr / st[7]) * mi / (sqrtf(vi) / st[8] + eps);
  p[i] = pi;
}

inline unsigned nblk(size_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }
inline int bad(const char* m) { return mdx_set_error(MDX_ERR_ARG, m); }
// A run-time integer as a template argument: calls f(std::integral_constant<int, V>{}) for the V among Vs that equals v; false if none does.
template <int... Vs, class F>
inline bool pick(int v, F&& f) {
  return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
// out (M x N, ld) = bias + sum over the S partial copies in P; more than RED_CHUNK copies go through `scratch`
// (ceil(S / RED_CHUNK) * M * N floats) in two fixed-order stages.
inline void launch_reduce_partials(const float* P, int S, int M, int N, const float* bias, float* out, int ld, float* scratch,
                                   hipStream_t s, int rkind = 0) {
  const size_t total = (size_t)M * N;
  const unsigned gx = (unsigned)((total + 31) / 32);
  if (S <= RED_CHUNK || !scratch) {
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(gx, 1), dim3(256), 0, s, P, S, S, M, N, bias, out, ld, rkind);
    return;
  }
  const int nc = (int)ceil_div(S, RED_CHUNK);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(gx, nc), dim3(256), 0, s, P, S, RED_CHUNK, M, N, (const float*)nullptr, scratch, N, 0);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(gx, 1), dim3(256), 0, s, (const float*)scratch, nc, nc, M, N, bias, out, ld, rkind);
}
// The end of a split weight gradient: dW (N x K, ldw) and, with db, db (N) from the partials a SplitLayout places in `partial`.
inline void finish_split(float* partial, const SplitLayout& L, int N, int K, float* dW, int ldw, float* db, int rkind, hipStream_t s) {
  const int S = (int)L.S;
  float* pb = partial + L.bias_off;
  if (db && S <= RED_CHUNK) {  // both reductions in one launch
    const unsigned gxw = (unsigned)(((size_t)N * K + 31) / 32), gxb = (unsigned)((N + 31) / 32);
    hipLaunchKernelGGL(reduce_partials2_kernel, dim3(gxw + gxb), dim3(256), 0, s, (const float*)partial, S, N, K, dW, ldw, (int)gxw,
                       (const float*)pb, N, db, rkind);
  } else {
    launch_reduce_partials(partial, S, N, K, nullptr, dW, ldw, partial + L.stage_off, s, rkind);
    if (db) launch_reduce_partials(pb, S, 1, N, nullptr, db, N, pb + (size_t)S * N, s, rkind);
  }
}
inline int launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDX_OK : mdx_set_error(MDX_ERR_HIP, hipGetErrorString(e));
}

}  // namespace

extern "C" int mdx_op_sgemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, const float* addend,
                               int64_t ldd, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int32_t splits, float* partial,
                               void* stream) {
  if (M <= 0 || N <= 0) return MDX_OK;
  if (!A || !B || !C || K < 0) return bad("sgemm_nt: null operand");
  hipStream_t s = (hipStream_t)stream;
  if (splits <= 1) {
    dim3 grid((unsigned)((N + G_TN - 1) / G_TN), (unsigned)((M + G_TM - 1) / G_TM), 1);
    hipLaunchKernelGGL(sgemm_nt_kernel, grid, dim3(256), 0, s, A, (int)lda, B, (int)ldb, bias, addend, (int)ldd, C, (int)ldc, (int)M,
                       (int)N, (int)K, (int)((K + G_KC - 1) / G_KC * G_KC), (float*)nullptr);
    return launched();
  }
  if (!partial) return bad("sgemm_nt: split-K needs a partial buffer of splits*M*N floats");
  if (addend) return bad("sgemm_nt: addend is not supported together with split-K");
  int kper = (int)((K + splits - 1) / splits);
  kper = (kper + G_KC - 1) / G_KC * G_KC;
  const int S = (int)((K + kper - 1) / kper);
  dim3 grid((unsigned)((N + G_TN - 1) / G_TN), (unsigned)((M + G_TM - 1) / G_TM), (unsigned)S);
  hipLaunchKernelGGL(sgemm_nt_kernel, grid, dim3(256), 0, s, A, (int)lda, B, (int)ldb, (const float*)nullptr, (const float*)nullptr, 0, C,
                     (int)ldc, (int)M, (int)N, (int)K, kper, partial);
  launch_reduce_partials(partial, S, (int)M, (int)N, bias, C, (int)ldc, nullptr, s);
  return launched();
}

// Every weight matrix of a model transposed by ONE launch (the dgrad GEMMs read W^T; a step used to spend ~240 small launches
// on it).  desc: 4 int64 per matrix {src, dst, R, C} (row-major, contiguous); blockIdx.y = matrix, blockIdx.x = 32 x 32 tile.
__global__ void transpose_batch_kernel(const long long* __restrict__ desc) {
  __shared__ float t[32][33];
  const long long* d = desc + 4 * (size_t)blockIdx.y;
  const float* in = reinterpret_cast<const float*>(d[0]);
  float* out = reinterpret_cast<float*>(d[1]);
  const int R = (int)d[2], Cn = (int)d[3];
  const int tc = (Cn + 31) / 32, tr = (R + 31) / 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int tile = blockIdx.x; tile < tc * tr; tile += gridDim.x) {
    const int r0 = (tile / tc) * 32, c0 = (tile % tc) * 32;
    for (int j = ty; j < 32; j += 8) {
      const int r = r0 + j, cc = c0 + tx;
      t[j][tx] = (r < R && cc < Cn) ? in[(size_t)r * Cn + cc] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
      const int cc = c0 + j, r = r0 + tx;
      if (cc < Cn && r < R) out[(size_t)cc * R + r] = t[tx][j];
    }
    __syncthreads();
  }
}

extern "C" int mdx_op_transpose_batch(const int64_t* desc, int64_t n, int64_t max_tiles, void* stream) {
  if (n <= 0) return MDX_OK;
  if (!desc) return bad("transpose_batch: null descriptor table");
  const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(max_tiles, 64));
  hipLaunchKernelGGL(transpose_batch_kernel, dim3(gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(desc));
  return launched();
}

extern "C" int mdx_op_transpose(const float* in, int64_t ldi, int64_t R, int64_t Cn, float* out, int64_t ldo, void* stream) {
  if (R <= 0 || Cn <= 0) return MDX_OK;
  if (!in || !out) return bad("transpose: null operand");
  dim3 grid((unsigned)((Cn + 31) / 32), (unsigned)((R + 31) / 32));
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, (int)ldi, (int)R, (int)Cn, out, (int)ldo);
  return launched();
}

// out[N] = sum over the M rows of X (element-wise times Y when Y != NULL).  ws: ceil(M/512)*N floats.
extern "C" int mdx_op_colreduce(const float* X, const float* Y, int64_t ld, int64_t M, int64_t N, float* out, float* ws, void* stream) {
  if (N <= 0) return MDX_OK;
  hipStream_t s = (hipStream_t)stream;
  if (M <= 0) return hipMemsetAsync(out, 0, (size_t)N * 4, s) == hipSuccess ? MDX_OK : mdx_set_error(MDX_ERR_HIP, "memset");
  const int RP = 512;
  const int nb = (int)((M + RP - 1) / RP);
  const unsigned gx = (unsigned)((N + 63) / 64);
  if (nb == 1) {
    hipLaunchKernelGGL(colreduce_kernel, dim3(gx, 1), dim3(256), 0, s, X, Y, (int)ld, (int)M, (int)N, RP, out);
    return launched();
  }
  if (!ws) return bad("colreduce: workspace of ceil(M/512)*N floats required");
  hipLaunchKernelGGL(colreduce_kernel, dim3(gx, nb), dim3(256), 0, s, X, Y, (int)ld, (int)M, (int)N, RP, ws);
  hipLaunchKernelGGL(colreduce_kernel, dim3(gx, 1), dim3(256), 0, s, (const float*)ws, (const float*)nullptr, (int)N, nb, (int)N, nb, out);
  return launched();
}

// `_t` forms of the row operators: dt = bit mask of the tensors stored as float16 (ln_relu_fwd: bit 0 x, 1 y; ln_relu_bwd: bit 0 dy, 1 x,
// 2 dx; ew_fwd: 0 a, 1 b, 2 out; ew_bwd: 0 a, 1 b, 2 g, 3 da, 4 db; gather_rows: 0 x, 1 y; segsum_rows: 0 src, 1 out; mul_gather_fwd:
// 0 a, 1 t, 2 y; mul_gather_bwd: 0 g, 1 a, 2 t, 3 da, 4 dt).  Half storage needs the 4-wide kernels (F % 4 == 0, aligned rows).
extern "C" int mdx_op_ln_relu_fwd_t(const void* xv, const float* gamma, const float* beta, int64_t M, int32_t F, int32_t relu, void* yv,
                                    float* stats, int32_t dt, void* stream) {
  if (M <= 0) return MDX_OK;
  if (F <= 0 || F > 64 * LN_MAXJ) return bad("ln_relu: feature count must be in 1..1024");
  const TP x{xv, dt & 1};
  const TPW y{yv, (dt >> 1) & 1};
  const bool al = tp_vec_ok(xv, x.h, 4) && tp_vec_ok(yv, y.h, 4);
  if (al && F % 4 == 0 && pick<8, 16, 32, 64>(F / 4, [&](auto LPR) {   // LPR lanes per row, four features each
        hipLaunchKernelGGL(ln_relu_fwd4_kernel<LPR>, dim3((unsigned)((M + 4 * (64 / LPR) - 1) / (4 * (64 / LPR)))), dim3(256), 0,
                           (hipStream_t)stream, x, gamma, beta, (int)M, relu, y, stats);
      }))
    return launched();
  if (dt) return bad("ln_relu: half storage needs F in {32, 64, 128, 256} and aligned rows");
  hipLaunchKernelGGL(ln_relu_fwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float*)xv, gamma, beta,
                     (int)M, F, relu, (float*)yv, stats);
  return launched();
}

// The 4-wide backward kernel for F in {32, 64, 128, 256} (false: not built for F), one workgroup per partial row of ws; w1 != NULL is the
// rank-1 form (dy holds M values).  The callers check alignment.
static bool launch_ln_bwd4(const TP& dy, const TP& x, const float* stats, const float* gamma, const float* beta, int64_t M, int32_t F,
                           int32_t relu, const TPW& dx, float* ws, const float* w1, hipStream_t s) {
  return F % 4 == 0 && pick<8, 16, 32, 64>(F / 4, [&](auto LPR) {
    hipLaunchKernelGGL(ln_relu_bwd4_kernel<LPR>, dim3((unsigned)ln_bwd_rows(M)), dim3(256), 32 * F, s, dy, x, stats, gamma, beta, (int)M, relu,
                       MDX_LN_RPW, dx, ws, w1);
  });
}
// dx (M,F); dgb (2F) = [dgamma | dbeta].  ws: mdx_op_ln_relu_bwd_ws(M, F) bytes.
extern "C" int mdx_op_ln_relu_bwd_t(const void* dyv, const void* xv, const float* stats, const float* gamma, const float* beta, int64_t M,
                                    int32_t F, int32_t relu, void* dxv, float* dgb, float* ws, int32_t dt, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (F <= 0 || F > 64 * LN_MAXJ) return bad("ln_relu: feature count must be in 1..1024");
  if (M <= 0) return !dgb || hipMemsetAsync(dgb, 0, (size_t)F * 8, s) == hipSuccess ? MDX_OK : mdx_set_error(MDX_ERR_HIP, "memset");
  if (!ws) return bad("ln_relu_bwd: workspace required");
  const TP dy{dyv, dt & 1}, x{xv, (dt >> 1) & 1};
  const TPW dx{dxv, (dt >> 2) & 1};
  const int nr = (int)ln_bwd_rows(M);            // workgroups of four waves; `ws` gets one partial row from each
  const bool al = tp_vec_ok(xv, x.h, 4) && tp_vec_ok(dyv, dy.h, 4) && tp_vec_ok(dxv, dx.h, 4) && ((reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  if (!(al && launch_ln_bwd4(dy, x, stats, gamma, beta, M, F, relu, dx, ws, nullptr, s))) {
    if (dt) return bad("ln_relu_bwd: half storage needs F in {32, 64, 128, 256} and aligned rows");
    hipLaunchKernelGGL(ln_relu_bwd_kernel, dim3((unsigned)nr), dim3(256), 32 * F, s, (const float*)dyv, (const float*)xv, stats, gamma, beta,
                       (int)M, F, relu, MDX_LN_RPW, (float*)dxv, ws);
  }
  // [dgamma | dbeta] = sum over the per-workgroup partial rows, fixed-order parallel reduction (dgb == NULL: deferred, the partial rows
  // stay in ws for mdx_op_reduce_deferred)
  if (dgb) launch_reduce_partials(ws, nr, 1, 2 * F, nullptr, dgb, 2 * F, ws + (size_t)nr * 2 * F, s);
  return launched();
}
extern "C" int mdx_op_ln_relu_bwd_r1_t(const void* g1, const float* w1, const void* xv, const float* stats, const float* gamma, const float* beta,
                                       int64_t M, int32_t F, int32_t relu, void* dxv, float* ws, int32_t dt, void* stream) {
  if (M <= 0) return MDX_OK;
  if (!g1 || !w1 || !xv || !stats || !gamma || !beta || !dxv || !ws) return bad("ln_relu_bwd_r1: null operand");
  const TP dy{g1, dt & 1}, x{xv, (dt >> 1) & 1};
  const TPW dx{dxv, (dt >> 2) & 1};
  if (!(tp_vec_ok(xv, x.h, 4) && tp_vec_ok(dxv, dx.h, 4) && ((reinterpret_cast<uintptr_t>(ws) & 15) == 0)))
    return mdx_set_error(MDX_ERR_UNSUPPORTED, "ln_relu_bwd_r1: aligned rows required");
  if (!launch_ln_bwd4(dy, x, stats, gamma, beta, M, F, relu, dx, ws, w1, (hipStream_t)stream))
    return mdx_set_error(MDX_ERR_UNSUPPORTED, "ln_relu_bwd_r1: F must be 32, 64, 128 or 256");
  return launched();
}
extern "C" size_t mdx_op_ln_relu_bwd_ws(int64_t M, int32_t F) { return (size_t)ln_bwd_ws_floats(M, F) * sizeof(float); }
extern "C" int64_t mdx_op_ln_relu_bwd_rows(int64_t M) { return ln_bwd_rows(M); }  // partial rows mdx_op_ln_relu_bwd leaves in ws ([rows][2F])

extern "C" int mdx_op_ew_fwd_t(int32_t op, const void* a, const void* b, void* out, int64_t n, int32_t dt, void* stream) {
  if (n <= 0) return MDX_OK;
  if ((op & 255) > 3 || (op >> 8) < 0 || (op >> 8) > 2) return bad("ew: unknown op");
  const TP ta{a, dt & 1}, tb{b, (dt >> 1) & 1};
  const TPW to{out, (dt >> 2) & 1};
  if ((n & 3) == 0 && tp_vec_ok(a, ta.h, 4) && tp_vec_ok(b, tb.h, 4) && tp_vec_ok(out, to.h, 4)) {
    hipLaunchKernelGGL(ew_fwd4_kernel, dim3(nblk((size_t)n / 4)), dim3(256), 0, (hipStream_t)stream, op, ta, tb, to, (size_t)n / 4);
  } else {
    hipLaunchKernelGGL(ew_fwd1_kernel, dim3(nblk((size_t)n)), dim3(256), 0, (hipStream_t)stream, op, ta, tb, to, (size_t)n);
  }
  return launched();
}
extern "C" int mdx_op_plan_flip(const int64_t* order_left, const int64_t* ptr, int64_t R, int64_t Eh, int64_t* order_right, void* stream) {
  if (R <= 0) return MDX_OK;
  if (!order_left || !ptr || !order_right || Eh < 0) return bad("plan_flip: null argument");
  hipLaunchKernelGGL(plan_flip_kernel, dim3(nblk((size_t)R)), dim3(256), 0, (hipStream_t)stream, order_left, ptr, R, Eh, order_right);
  return launched();
}
extern "C" int mdx_op_sum_n(const void* const* srcs, const int32_t* half, int32_t k, int64_t n, void* out, int32_t out_half, void* stream) {
  if (n <= 0) return MDX_OK;
  if (k < 1 || k > 12 || !srcs || !half || !out) return bad("sum_n: 1..12 operands");
  SumN a;
  bool vec = (n & 3) == 0 && tp_vec_ok(out, out_half, 4);
  for (int j = 0; j < k; ++j) {
    if (!srcs[j]) return bad("sum_n: null operand");
    a.p[j] = srcs[j], a.h[j] = half[j] ? 1 : 0;
    vec = vec && tp_vec_ok(srcs[j], a.h[j], 4);
  }
  a.n = k;
  const TPW to{out, out_half ? 1 : 0};
  if (vec) hipLaunchKernelGGL(sum_n4_kernel, dim3(nblk((size_t)n / 4)), dim3(256), 0, (hipStream_t)stream, a, to, (size_t)n / 4);
  else hipLaunchKernelGGL(sum_n1_kernel, dim3(nblk((size_t)n)), dim3(256), 0, (hipStream_t)stream, a, to, (size_t)n);
  return launched();
}
extern "C" int mdx_op_ew_bwd_t(int32_t op, const void* a, const void* b, const void* g, void* da, void* db, int64_t n, int32_t dt,
                               void* stream) {
  if (n <= 0) return MDX_OK;
  if (op < 0 || op > 3) return bad("ew: unknown op");
  const TP ta{a, dt & 1}, tb{b, (dt >> 1) & 1}, tg{g, (dt >> 2) & 1};
  const TPW tda{da, (dt >> 3) & 1}, tdb{db, (dt >> 4) & 1};
  if ((n & 3) == 0 && tp_vec_ok(a, ta.h, 4) && tp_vec_ok(b, tb.h, 4) && tp_vec_ok(g, tg.h, 4) && tp_vec_ok(da, tda.h, 4) &&
      tp_vec_ok(db, tdb.h, 4)) {
    hipLaunchKernelGGL(ew_bwd4_kernel, dim3(nblk((size_t)n / 4)), dim3(256), 0, (hipStream_t)stream, op, ta, tb, tg, tda, tdb, (size_t)n / 4);
  } else {
    hipLaunchKernelGGL(ew_bwd1_kernel, dim3(nblk((size_t)n)), dim3(256), 0, (hipStream_t)stream, op, ta, tb, tg, tda, tdb, (size_t)n);
  }
  return launched();
}
extern "C" int mdx_op_gather_rows_t(const void* x, const int64_t* idx, int64_t M, int32_t F, void* y, int32_t dt, void* stream) {
  if (M <= 0 || F <= 0) return MDX_OK;
  const TP tx{x, dt & 1};
  const TPW ty{y, (dt >> 1) & 1};
  if ((F & 3) == 0 && tp_vec_ok(x, tx.h, 4) && tp_vec_ok(y, ty.h, 4)) {
    hipLaunchKernelGGL(gather_rows4_kernel, dim3(nblk((size_t)M * (F / 4))), dim3(256), 0, (hipStream_t)stream, tx, idx, M, F / 4, ty);
  } else {
    if (dt) return bad("gather_rows: half storage needs F % 4 == 0 and aligned rows");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(nblk((size_t)M * F)), dim3(256), 0, (hipStream_t)stream, (const float*)x, idx, M, F, (float*)y);
  }
  return launched();
}
extern "C" int mdx_op_segsum_rows_t(const void* src, const int64_t* order, const int64_t* ptr, int64_t R, int32_t F, void* out, int32_t dt,
                                    void* stream) {
  if (R <= 0 || F <= 0) return MDX_OK;
  const TP ts{src, dt & 1};
  const TPW to{out, (dt >> 1) & 1};
  if ((F & 3) == 0 && tp_vec_ok(src, ts.h, 4) && tp_vec_ok(out, to.h, 4)) {
    const size_t items = (size_t)R * (F / 4);
    // float16 rows only: the fp32 mode keeps the sequential CSR order -- the order of torch's index_add on the CPU, i.e. of the reference
    // and the oracle, which its parity tests rely on (a 32-wide LayerNorm gain's gradient moved from 4.8e-5 to 1.6e-4 of its norm at
    // 256 molecules with the dealt order; both are fp32 rounding, but the contract there is 1e-4)
    if (ts.h && (F & 7) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && items < ((size_t)1 << 22))
      hipLaunchKernelGGL(segsum_rows8s_kernel, dim3((unsigned)(((size_t)R * (F / 8) + 63) / 64)), dim3(256), 0, (hipStream_t)stream,
                         reinterpret_cast<const _Float16*>(src), order, ptr, R, F / 8, to);
    else if ((ts.h || (dt & 4)) && items < ((size_t)1 << 22))
      hipLaunchKernelGGL(segsum_rows4s_kernel, dim3((unsigned)((items + 63) / 64)), dim3(256), 0, (hipStream_t)stream, ts, order, ptr, R, F / 4, to);
    else
      hipLaunchKernelGGL(segsum_rows4_kernel, dim3(nblk(items)), dim3(256), 0, (hipStream_t)stream, ts, order, ptr, R, F / 4, to);
  } else {
    if (dt & 3) return bad("segsum_rows: half storage needs F % 4 == 0 and aligned rows");
    if (dt & 4)
      hipLaunchKernelGGL(segsum_rows1s_kernel, dim3((unsigned)(((size_t)R * F + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (const float*)src,
                         order, ptr, R, F, (float*)out);
    else
      hipLaunchKernelGGL(segsum_rows_kernel, dim3(nblk((size_t)R * F)), dim3(256), 0, (hipStream_t)stream, (const float*)src, order, ptr, R, F,
                         (float*)out);
  }
  return launched();
}
extern "C" int mdx_op_edge_geom_fwd(const float* pos, const int64_t* l, const int64_t* r, int64_t E, float* rel, float* dist, void* stream) {
  if (E <= 0) return MDX_OK;
  hipLaunchKernelGGL(edge_geom_fwd_kernel, dim3(nblk((size_t)E)), dim3(256), 0, (hipStream_t)stream, pos, l, r, E, rel, dist);
  return launched();
}
extern "C" int mdx_op_edge_geom_bwd(const float* rel, const float* dist, const float* drel, const float* ddist, int64_t E, float* g,
                                    void* stream) {
  if (E <= 0) return MDX_OK;
  hipLaunchKernelGGL(edge_geom_bwd_kernel, dim3(nblk((size_t)E)), dim3(256), 0, (hipStream_t)stream, rel, dist, drel, ddist, E, g);
  return launched();
}
extern "C" int mdx_op_smear_fwd(const float* d, const float* off, const float* coef, int32_t G, float lo, float hi, int64_t E, float* out,
                                void* stream) {
  if (E <= 0) return MDX_OK;
  hipLaunchKernelGGL(smear_fwd_kernel, dim3(nblk((size_t)E * G)), dim3(256), 0, (hipStream_t)stream, d, off, coef, G, lo, hi, E, out);
  return launched();
}
extern "C" int mdx_op_smear_bwd(const float* d, const float* off, const float* coef, int32_t G, float lo, float hi, int64_t E,
                                const float* gout, float* gd, void* stream) {
  if (E <= 0) return MDX_OK;
  hipLaunchKernelGGL(smear_bwd_kernel, dim3(nblk((size_t)E)), dim3(256), 0, (hipStream_t)stream, d, off, coef, G, lo, hi, E, gout, gd);
  return launched();
}
extern "C" int mdx_op_force_fwd(const float* w, const float* rel, const float* d, int64_t E, float* out, void* stream) {
  if (E <= 0) return MDX_OK;
  hipLaunchKernelGGL(force_fwd_kernel, dim3(nblk((size_t)E)), dim3(256), 0, (hipStream_t)stream, w, rel, d, E, out);
  return launched();
}
extern "C" int mdx_op_force_bwd(const float* w, const float* rel, const float* d, const float* g, int64_t E, float* gw, float* grel,
                                float* gd, void* stream) {
  if (E <= 0) return MDX_OK;
  hipLaunchKernelGGL(force_bwd_kernel, dim3(nblk((size_t)E)), dim3(256), 0, (hipStream_t)stream, w, rel, d, g, E, gw, grel, gd);
  return launched();
}

// out[0] = sum x[i]^2 over the flat buffer (two fixed-order stages; ws: 1024 floats).
extern "C" int mdx_op_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!out || !ws) return bad("sumsq: null output / workspace");
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (n + 8191) / 8192));
  hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, s, x, (size_t)std::max<int64_t>(n, 0), ws);
  hipLaunchKernelGGL(sum_small_kernel, dim3(1), dim3(64), 0, s, (const float*)ws, nb, out);
  return launched();
}
// One AdamW step over flat (p, g, m, v); step = 1, 2, ...  gnorm2 (device scalar, may be NULL) + max_norm apply
// torch.nn.utils.clip_grad_norm_ to g on the fly (g itself is left unscaled).
extern "C" int mdx_op_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int64_t step, const float* gnorm2, float max_norm, void* stream) {
  if (n <= 0) return MDX_OK;
  if (step < 1) return bad("adamw: step counts from 1");
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.0f - powf(beta2, (float)step));
  hipLaunchKernelGGL(adamw_kernel, dim3(nblk((size_t)n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (size_t)n, lr, beta1, beta2, eps,
                     weight_decay, bc1, bc2s, gnorm2, max_norm);
  return launched();
}

// One optimisation step with torch.cuda.amp.GradScaler semantics, state on the device (see amp_decide_kernel): g holds the
// gradient of (S x loss).  Unscales, measures the global norm (state[4], unscaled), clips to max_norm (<= 0 or inf: no clipping),
// and applies AdamW -- or, if any gradient is not finite, skips the update (the step count does not advance) and multiplies S by
// `backoff`; after `growth_interval` consecutive finite steps S is multiplied by `growth`.  With S = growth = backoff = 1 this is the
// plain fp32 step.  ws: 1024 floats.  No host synchronisation.
extern "C" int mdx_op_amp_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                float weight_decay, float max_norm, float* state, float growth, float backoff, int32_t growth_interval,
                                float* ws, void* stream) {
  if (n <= 0) return MDX_OK;
  if (!p || !g || !m || !v || !state || !ws) return bad("amp_adamw: null argument");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (n + 8191) / 8192));
  hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, s, g, (size_t)n, ws);
  const float mn = (max_norm > 0.f) ? max_norm : INFINITY;
  hipLaunchKernelGGL(amp_decide_kernel, dim3(1), dim3(64), 0, s, (const float*)ws, nb, state, beta1, beta2, mn, growth, backoff,
                     (int)growth_interval);
  hipLaunchKernelGGL(adamw_amp_kernel, dim3(nblk((size_t)n)), dim3(256), 0, s, p, g, m, v, (size_t)n, lr, beta1, beta2, eps, weight_decay,
                     (const float*)state);
  return launched();
}

// Weight gradient of a Linear layer: dW[N,K] = G[M,N]^T X[M,K] (row-major operands as stored by the forward/backward;
// no transposes).  The M rows are cut into `splits` ranges whose partial products are summed in a fixed order
// (partial: split_layout(M, N, K, splits, W_MC).total floats -- mdx_train_plan.h: the partial products plus the first reduction stage,
// for dW and for the optional bias gradient db[N] = column sums of G, which rides along in the first k-tile's workgroups).
extern "C" int mdx_op_sgemm_tn(const float* G, int64_t ldg, const float* X, int64_t ldx, float* dW, int64_t ldw, float* db, int64_t M,
                               int64_t N, int64_t K, int32_t splits, float* partial, void* stream) {
  if (N <= 0 || K <= 0) return MDX_OK;
  hipStream_t s = (hipStream_t)stream;
  if (!G || !X || !partial) return bad("sgemm_tn: null operand / partial buffer");
  const SplitLayout L = split_layout(M, N, K, splits, W_MC);
  dim3 grid((unsigned)((K + W_T - 1) / W_T), (unsigned)((N + W_T - 1) / W_T), (unsigned)L.S);
  hipLaunchKernelGGL(sgemm_tn_split_kernel, grid, dim3(256), 0, s, G, (int)ldg, X, (int)ldx, (int)M, (int)N, (int)K, (int)L.mper, partial,
                     db ? partial + L.bias_off : nullptr);
  // dW == NULL: deferred, the partials stay where mdx_op_wgrad_layout says and mdx_op_reduce_deferred sums them later
  if (dW) finish_split(partial, L, (int)N, (int)K, dW, (int)ldw, db, 0, s);
  return launched();
}

// ---- deferred gradient reduction (round 3) ----------------------------------------------------------------------------------------
// A training step has ~260 weight gradients and ~150 LayerNorm parameter gradients; each used to end in its own 7 us reduction launch
// (plus torch's accumulation kernels on the way into the flat gradient buffer).  With dW == NULL (LayerNorm: dgb == NULL) the
// operators leave their split partials in the caller's buffer; ONE launch of mdx_op_reduce_deferred per step then sums every record
// in the fixed order of the dedicated kernels and ADDS the result to its destination -- the parameter's slot of the flat gradient
// buffer.  Record (8 x int64): P, dst, S (partials), rows, cols, ld (dst row stride), pstride (floats between consecutive partials),
// rkind (0 fp32, 1 bfloat16, 2 float16 rounding of the sum, mixed precision) | first_block << 8.
extern "C" int mdx_op_wgrad_layout(int64_t M, int64_t N, int64_t K, int32_t splits, int32_t half, int64_t* S_out, int64_t* bias_off) {
  const SplitLayout L = split_layout(M, N, K, splits, half ? HW_MC : W_MC);
  if (S_out) *S_out = L.S;
  if (bias_off) *bias_off = L.bias_off;   // floats from `partial` to the [S][N] bias partials
  return MDX_OK;
}
namespace {
// One lane per FOUR consecutive output elements: eight running sums over the partials k = z, z + 8, ... (z = 0..7), added up in the
// order z = 0..7 -- the association of the per-layer reduction kernels.  History: one thread per (element, z) read 128 contiguous bytes
// per half wave (1.45 ms per training step); one thread per element with eight loads in flight: 1.13 ms -- and that time was not
// bandwidth: a LayerNorm over the E edge rows leaves E / 16 partial rows, so ONE thread walked ~10,000 partials in a dependent chain
// (1,250 iterations x ~0.9 us) while the weight records finished in a fraction of it.  The caller now splits a record with more than
// 256 partials is summed the way launch_reduce_partials does it (chunk sums into the scratch planes behind the partials -- a `chunked`
// record; then a second launch over the chunk sums), so no chain is longer than 32 + S/2048 iterations, and a lane takes four
// elements (one 16-byte load per partial when the record's planes are 16-byte aligned) so a wave reads 1 KB per partial and the
// record look-up is paid once per 128 elements.  rkind bit 6: chunked; bit 7: store the sum instead of adding it.  The record table's
// unit (`first_block`) is RED_ELEMS = 128 elements per block; a chunked record takes ceil(S / RED_CHUNK) times the blocks of a plain one
// (red_blocks, red_chunk_plane: mdx_train_plan.h, which the host's record table uses too).
template <bool VEC>
__device__ __forceinline__ f32x4 reduce_deferred_sum(const float* p, size_t pstride, int S, int ne) {
  f32x4 acc[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) acc[z] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto ldp = [&](int k) -> f32x4 {
    const float* q = p + (size_t)k * pstride;
    if constexpr (VEC) {
      return *reinterpret_cast<const f32x4*>(q);
    } else {
      f32x4 v{0.f, 0.f, 0.f, 0.f};
      v[0] = q[0];
      if (ne > 1) v[1] = q[1];
      if (ne > 2) v[2] = q[2];
      if (ne > 3) v[3] = q[3];
      return v;
    }
  };
  int k = 0;
  for (; k + 8 <= S; k += 8) {
    f32x4 v[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) v[z] = ldp(k + z);
#pragma unroll
    for (int z = 0; z < 8; ++z) acc[z] += v[z];
  }
#pragma unroll
  for (int z = 0; z < 8; ++z)
    if (k + z < S) acc[z] += ldp(k + z);
  f32x4 r{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int z = 0; z < 8; ++z) r += acc[z];
  return r;
}
__global__ __launch_bounds__(256) void reduce_deferred_kernel(const int64_t* __restrict__ desc, int n, long long total_blocks) {
  const long long blk = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (blk >= total_blocks) return;
  // binary search: last record whose first block is <= blk
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)(desc[8 * mid + 7] >> 8) <= blk) lo = mid; else hi = mid - 1;
  }
  const int64_t* d = desc + 8 * lo;
  const float* P = reinterpret_cast<const float*>(d[0]);
  float* dst = reinterpret_cast<float*>(d[1]);
  int S = (int)d[2], ld = (int)d[5];
  const int cols = (int)d[4];
  const size_t total = (size_t)d[3] * cols, pstride = (size_t)d[6];
  int rkind = (int)(d[7] & 63);
  bool store = (d[7] & 128) != 0;
  long long rel = blk - (long long)(d[7] >> 8);
  if (d[7] & 64) {
    // chunked record (S > RED_CHUNK): its blocks are [chunk][block]; chunk c sums partials 256 c .. 256 c + 255 and STORES the sum in
    // the scratch plane c behind the partials (red_chunk_plane: where launch_reduce_partials keeps its chunk sums, and what the
    // workspace / wgrad layouts reserve).  The caller's second table sums those planes into dst.
    const long long nblk = (long long)red_blocks((int64_t)total);
    const int chunk = (int)(rel / nblk);
    rel -= chunk * nblk;
    dst = const_cast<float*>(P) + (size_t)red_chunk_plane(S, chunk) * pstride;
    P += (size_t)chunk * RED_CHUNK * pstride;
    S = min(RED_CHUNK, S - chunk * RED_CHUNK);
    ld = cols;
    rkind = 0;
    store = true;
  }
  static_assert(RED_ELEMS == 32 * 4, "a block of the record table is 32 lanes of four elements");
  const size_t i = ((size_t)rel * 32 + (threadIdx.x & 31)) * 4;
  if (i >= total) return;
  const int ne = (int)min((size_t)4, total - i);
  const bool vec = ne == 4 && (pstride & 3) == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0;
  const f32x4 r = vec ? reduce_deferred_sum<true>(P + i, pstride, S, ne) : reduce_deferred_sum<false>(P + i, pstride, S, ne);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < ne) {
      const size_t row = (i + e) / cols, col = (i + e) % cols;
      float* o = dst + row * ld + col;
      const float x = round_kind(r[e], rkind);
      *o = store ? x : *o + x;
    }
}
}  // namespace
extern "C" int mdx_op_reduce_deferred(const int64_t* desc, int32_t n, int64_t total_blocks, void* stream) {
  if (n <= 0 || total_blocks <= 0) return MDX_OK;
  if (!desc) return bad("reduce_deferred: null record table");
  hipLaunchKernelGGL(reduce_deferred_kernel, dim3((unsigned)((total_blocks + 7) / 8)), dim3(256), 0, (hipStream_t)stream, desc, (int)n,
                     (long long)total_blocks);
  return launched();
}

// The row-owner GEMM takes this call: its shapes (mdx_train_plan.h), float16 arithmetic, A in a float16 container with rows on 16 bytes.
static bool rows_gemm_ok(const void* Av, int64_t lda, int a_half, int32_t half_kind, int64_t M, int64_t N, int64_t K) {
  return half_kind == 2 && a_half && rows_gemm_shape(M, N, K) && (lda & 7) == 0 && (reinterpret_cast<uintptr_t>(Av) & 15) == 0;
}
// Mixed-precision forms of sgemm_nt / sgemm_tn: operands rounded to `half_kind` (1 = bfloat16, 2 = float16) on their way into
// LDS, products on the 16x16x32 half MFMAs, fp32 accumulation.  round_out != 0: the result is rounded to the same type before it
// is stored (in an fp32 container) -- the value a Linear returns under torch.autocast (float16 overflows to infinity).  The forward
// form has no split-K.  mdx_op_hgemm_* = half_kind 1, round_out 0 (round 2's 'bf16 operands' mode).
// `_t` forms: dt is a bit mask of the tensors stored as float16 instead of fp32 (half storage): xgemm_nt bit 0 A, 1 addend, 2 C;
// xgemm_tn bit 0 G, 1 X (dW / db are always fp32).  A float16 C holds the rounded result by construction.
extern "C" int mdx_op_xgemm_nt_t(const void* Av, int64_t lda, const float* B, int64_t ldb, const float* bias, const void* addendv,
                                 int64_t ldd, void* Cv, int64_t ldc, int64_t M, int64_t N, int64_t K, int32_t half_kind, int32_t round_out,
                                 int32_t dt, void* stream) {
  if (M <= 0 || N <= 0) return MDX_OK;
  if (!Av || !B || !Cv || K < 0) return bad("xgemm_nt: null operand");
  if ((dt & 5) && half_kind != 2) return bad("xgemm_nt: float16 containers (A or C) need half_kind 2");
  const TP A{Av, dt & 1}, addend{addendv, (dt >> 1) & 1};
  const TPW C{Cv, (dt >> 2) & 1};
  if (half_kind != 1 && half_kind != 2) return bad("xgemm_nt: half_kind must be 1 (bfloat16) or 2 (float16)");
  hipStream_t s = (hipStream_t)stream;
  // float16 rows, widths the row-owner kernel is instantiated for: whole weight resident in LDS, no K loop over barriers (measured in
  // round 3: 84 -> 47 us on 256 -> 256 against the tiled kernel)
  if (rows_gemm_ok(Av, lda, A.h, half_kind, M, N, K)) {
    const _Float16* Ah = reinterpret_cast<const _Float16*>(Av);
    // few rows (the per-node layers): column groups, see the kernel -- 64 columns as 2 x 32, 128 as 4 x 32, 256 as 4 x 64
    const bool few = (M + 127) / 128 <= mdx_num_cus() / 2;
    pick<1, 2, 4, 8>((int)(K / 32), [&](auto KT) {
      pick<2, 4, 8, 16>((int)(N / 16), [&](auto FT) {
        pick<0, 1>(round_out ? 1 : 0, [&](auto R) {
          constexpr int kt = decltype(KT)::value, ft = decltype(FT)::value, g = ft == 2 ? 1 : ft == 16 ? 4 : ft / 2;
          constexpr bool r = decltype(R)::value != 0;
          if (few && g > 1)
            launch_hgemm_nt_rows<kt, ft / g, r>(Ah, (int)lda, B, (int)ldb, bias, addend, (int)ldd, C, (int)ldc, (int)M, s, LnEpi{}, g);
          else
            launch_hgemm_nt_rows<kt, ft, r>(Ah, (int)lda, B, (int)ldb, bias, addend, (int)ldd, C, (int)ldc, (int)M, s);
        });
      });
    });
    return launched();
  }
  // Column tile: 64 for N <= 64, else 128.  Measured on the training step (ms per step, fp16 mode) with tiles up to 64: 52.0, up to 128:
  // 51.5, up to 256: 54.7 (one workgroup per CU) -- the re-reads of A were L2 hits all along; the kernel is bound by its short K loop (one
  // 64-wide chunk in flight per workgroup)
  pick<0, 1>(half_kind - 1, [&](auto HT) {
    pick<0, 1>(round_out ? 1 : 0, [&](auto R) {
      pick<64, 128>(N <= 64 ? 64 : 128, [&](auto TN) {
        constexpr int ht = decltype(HT)::value, tn = decltype(TN)::value;
        constexpr bool r = decltype(R)::value != 0;
        dim3 grid((unsigned)((N + tn - 1) / tn), (unsigned)((M + G_TM - 1) / G_TM), 1);
        if constexpr (ht == 1) {   // a float16 A is copied to LDS as it is
          if (A.h) {
            hipLaunchKernelGGL((hgemm_nt_kernel<ht, r, tn, true>), grid, dim3(256), 0, s, A, (int)lda, B, (int)ldb, bias, addend, (int)ldd, C,
                               (int)ldc, (int)M, (int)N, (int)K);
            return;
          }
        }
        hipLaunchKernelGGL((hgemm_nt_kernel<ht, r, tn, false>), grid, dim3(256), 0, s, A, (int)lda, B, (int)ldb, bias, addend, (int)ldd, C,
                           (int)ldc, (int)M, (int)N, (int)K);
      });
    });
  });
  return launched();
}
// Linear + LayerNorm(+ReLU) in one launch (float16 rows on the row-owner kernel only; anything else: MDX_ERR_UNSUPPORTED, the caller
// runs the two operators).  C (M,N) = the Linear's result as mdx_op_xgemm_nt_t stores it, post (M,N) = relu(LN(C)) in the container
// dt bit 3 names, stats (M,2) = mean, rstd: the SAME FORMULA as mdx_op_ln_relu_fwd_t applied to C, in a different summation order (a lane
// sums its FT strided quads, then the four q-lanes are combined; the stand-alone operator sums LPR lanes of contiguous elements), so
// the two agree to rounding (a few fp32 ulp on the statistics), not bit for bit -- which one runs depends on M >= 1024 only.  It is
// what mdx_op_ln_relu_bwd_t reads.  A float16 C with round_out = 0 is refused: the LayerNorm would see the unrounded values while C
// stores rounded ones.
extern "C" int mdx_op_xgemm_nt_ln_supported(int64_t M, int64_t N, int64_t K) { return rows_gemm_shape(M, N, K) ? 1 : 0; }
extern "C" int mdx_op_xgemm_nt_ln_t(const void* Av, int64_t lda, const float* B, int64_t ldb, const float* bias, const void* addendv,
                                    int64_t ldd, void* Cv, int64_t ldc, const float* gamma, const float* beta, void* postv, int64_t ldp,
                                    float* stats, int32_t relu, int64_t M, int64_t N, int64_t K, int32_t half_kind, int32_t round_out,
                                    int32_t dt, void* stream) {
  if (M <= 0 || N <= 0) return MDX_OK;
  if (!Av || !B || !Cv || !gamma || !beta || !postv || !stats) return bad("xgemm_nt_ln: null operand");
  if (!rows_gemm_ok(Av, lda, dt & 1, half_kind, M, N, K)) return mdx_set_error(MDX_ERR_UNSUPPORTED, "xgemm_nt_ln: shape / container not built (use xgemm_nt + ln_relu_fwd)");
  if (((dt >> 2) & 1) && !round_out) return mdx_set_error(MDX_ERR_UNSUPPORTED, "xgemm_nt_ln: a float16 C needs round_out (LN must see the stored values)");
  const TP addend{addendv, (dt >> 1) & 1};
  const TPW C{Cv, (dt >> 2) & 1};
  const LnEpi ln{gamma, beta, TPW{postv, (dt >> 3) & 1}, (int)ldp, stats, relu};
  if (!tp_vec_ok(postv, ln.post.h, ldp)) return bad("xgemm_nt_ln: post rows must be vector-aligned");
  hipStream_t s = (hipStream_t)stream;
  const _Float16* Ah = reinterpret_cast<const _Float16*>(Av);
  pick<1, 2, 4, 8>((int)(K / 32), [&](auto KT) {
    pick<2, 4, 8, 16>((int)(N / 16), [&](auto FT) {
      pick<0, 1>(round_out ? 1 : 0, [&](auto R) {
        launch_hgemm_nt_rows<decltype(KT)::value, decltype(FT)::value, decltype(R)::value != 0, true>(Ah, (int)lda, B, (int)ldb, bias, addend, (int)ldd, C, (int)ldc, (int)M, s, ln);
      });
    });
  });
  return launched();
}
extern "C" int mdx_op_xgemm_tn_t(const void* Gv, int64_t ldg, const void* Xv, int64_t ldx, float* dW, int64_t ldw, float* db, int64_t M,
                                 int64_t N, int64_t K, int32_t splits, float* partial, int32_t half_kind, int32_t round_out, int32_t dt,
                                 void* stream) {
  if (N <= 0 || K <= 0) return MDX_OK;
  hipStream_t s = (hipStream_t)stream;
  if (!Gv || !Xv || !partial) return bad("xgemm_tn: null operand / partial buffer");
  const TP G{Gv, dt & 1}, X{Xv, (dt >> 1) & 1};
  if (half_kind != 1 && half_kind != 2) return bad("xgemm_tn: half_kind must be 1 (bfloat16) or 2 (float16)");
  const SplitLayout L = split_layout(M, N, K, splits, HW_MC);
  const int mper = (int)L.mper;
  float* pb = db ? partial + L.bias_off : nullptr;
  // float16 containers on both sides, tile-aligned widths: the transpose-read kernel (no conversion, no register transposes), 128-wide
  // tiles where the layer allows
  if (half_kind == 2 && G.h && X.h && N % 64 == 0 && K % 64 == 0 && ldg % 8 == 0 && ldx % 8 == 0 &&
      (reinterpret_cast<uintptr_t>(Gv) & 15) == 0 && (reinterpret_cast<uintptr_t>(Xv) & 15) == 0) {
    const _Float16 *Gh = reinterpret_cast<const _Float16*>(Gv), *Xh = reinterpret_cast<const _Float16*>(Xv);
    pick<64, 128>(N % 128 == 0 ? 128 : 64, [&](auto TN) {
      pick<64, 128>(K % 128 == 0 ? 128 : 64, [&](auto TK) {
        constexpr int tn = decltype(TN)::value, tk = decltype(TK)::value;
        hipLaunchKernelGGL((hgemm_tn_tr_kernel<tn, tk>), dim3((unsigned)(K / tk), (unsigned)(N / tn), (unsigned)L.S), dim3(256), 0, s, Gh,
                           (int)ldg, Xh, (int)ldx, (int)M, (int)N, (int)K, mper, partial, pb);
      });
    });
  } else {   // the converting kernel, 64 x 64 tiles
    const dim3 grid((unsigned)((K + 63) / 64), (unsigned)((N + 63) / 64), (unsigned)L.S);
    pick<0, 1>(half_kind - 1, [&](auto HT) {
      hipLaunchKernelGGL(hgemm_tn_split_kernel<HT>, grid, dim3(256), 0, s, G, (int)ldg, X, (int)ldx, (int)M, (int)N, (int)K, mper, partial, pb);
    });
  }
  // dW == NULL: deferred reduction (mdx_op_reduce_deferred)
  if (dW) finish_split(partial, L, (int)N, (int)K, dW, (int)ldw, db, round_out ? half_kind : 0, s);
  return launched();
}
// Queued weight gradients (float16 autocast mode; see wgrad_grouped_kernel).  mdx_op_wgrad_plan: which tile class a contraction takes
// and its block / partial layout (wgrad_plan, mdx_train_plan.h) -- out[0..7] = kind, gx, gy, S, mper, offset of the bias partials (floats
// from P), floats of the whole partial area (products, first reduction stage, bias partials and theirs: the layout of mdx_op_xgemm_tn_t),
// blocks.  `aligned` = both operands start on 16 bytes.  mdx_op_wgrad_grouped: one launch over a device table of `n` records of one kind
// (16 x int64 each, layout at the kernel), `total_blocks` = sum of their blocks; the partials are left for mdx_op_reduce_deferred.
extern "C" int mdx_op_wgrad_plan(int64_t M, int64_t N, int64_t K, int32_t splits, int32_t dt, int64_t ldg, int64_t ldx, int32_t aligned,
                                 int64_t* out) {
  if (!out || N <= 0 || K <= 0) return bad("wgrad_plan: bad arguments");
  const WgradPlan p = wgrad_plan(M, N, K, splits, dt, ldg, ldx, aligned != 0);
  out[0] = p.kind, out[1] = p.gx, out[2] = p.gy, out[3] = p.lay.S, out[4] = p.lay.mper;
  out[5] = p.lay.bias_off, out[6] = p.lay.total, out[7] = p.blocks;
  return MDX_OK;
}
extern "C" int mdx_op_wgrad_grouped(const int64_t* desc, int32_t n, int64_t total_blocks, int32_t kind, void* stream) {
  if (n <= 0 || total_blocks <= 0) return MDX_OK;
  if (!desc) return bad("wgrad_grouped: null record table");
  if (total_blocks > 0x7fffffffll) return bad("wgrad_grouped: too many blocks");
  const bool known = pick<0, 1, 2, 3, 4, 5, 6, 7>(kind, [&](auto KIND) {
    hipLaunchKernelGGL(wgrad_grouped_kernel<KIND>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(desc), (int)n);
  });
  return known ? launched() : bad("wgrad_grouped: kind must be 0..7");
}

// y = a * t[idx] (rows of F floats, F % 4 == 0) and its gradients; see mulg_*_kernel.
// F: feature count in its low 16 bits; bits 16.. = rounding kind of the product (0 fp32, 1 bfloat16, 2 float16; mixed precision)
extern "C" int mdx_op_mul_gather_fwd_t(const void* a, const void* t, const int64_t* idx, int64_t M, int32_t F, void* y, int32_t dt,
                                       void* stream) {
  const int rk = F >> 16;
  F &= 0xffff;
  if (M <= 0 || F <= 0) return MDX_OK;
  if (F & 3) return bad("mul_gather: F must be a multiple of 4");
  if (rk < 0 || rk > 2) return bad("mul_gather: unknown rounding kind");
  const TP ta{a, dt & 1}, tt{t, (dt >> 1) & 1};
  const TPW ty{y, (dt >> 2) & 1};
  if (!(tp_vec_ok(a, ta.h, 4) && tp_vec_ok(t, tt.h, 4) && tp_vec_ok(y, ty.h, 4))) return bad("mul_gather: rows must be aligned");
  hipLaunchKernelGGL(mulg_fwd_kernel, dim3(nblk((size_t)M * (F / 4))), dim3(256), 0, (hipStream_t)stream, ta, tt, idx, M, F / 4, ty, rk);
  return launched();
}
extern "C" int mdx_op_mul_gather_bwd_t(const void* g, const void* a, const void* t, const int64_t* idx, const int64_t* order,
                                       const int64_t* ptr, int64_t M, int64_t R, int32_t F, void* da, void* dtab, int32_t dt, void* stream) {
  if (F <= 0) return MDX_OK;
  if (F & 3) return bad("mul_gather: F must be a multiple of 4");
  hipStream_t s = (hipStream_t)stream;
  const TP tg{g, dt & 1}, ta{a, (dt >> 1) & 1}, tt{t, (dt >> 2) & 1};
  const TPW tda{da, (dt >> 3) & 1}, tdt{dtab, (dt >> 4) & 1};
  const bool want_da = da && M > 0, want_dt = dtab && R > 0;
  // operands of the launches below (no rows: every segment is empty and g / a are never read)
  if (want_da && (!g || !t || !idx)) return bad("mul_gather_bwd: null operand");
  if (want_dt && (!order || !ptr || (M > 0 && (!g || !a)))) return bad("mul_gather_bwd: null operand");
  // the 4-wide kernels read and write 16-byte (float16: 8-byte) vectors: refuse a misaligned base like the forward does
  if ((want_da && !(tp_vec_ok(g, tg.h, 4) && tp_vec_ok(t, tt.h, 4) && tp_vec_ok(da, tda.h, 4))) ||
      (want_dt && !(tp_vec_ok(g, tg.h, 4) && tp_vec_ok(a, ta.h, 4) && tp_vec_ok(dtab, tdt.h, 4))))
    return bad("mul_gather: rows must be aligned");
  if (want_da)
    hipLaunchKernelGGL(mulg_fwd_kernel, dim3(nblk((size_t)M * (F / 4))), dim3(256), 0, s, tg, tt, idx, M, F / 4, tda, 0);
  if (want_dt)
    hipLaunchKernelGGL(mulg_segsum_kernel, dim3(nblk((size_t)R * (F / 4))), dim3(256), 0, s, tg, ta, order, ptr, R, F / 4, tdt);
  return launched();
}
