// Layer-level operators of the training path (gfx950), part 1: the contractions and the reductions behind them.  Every
// O(rows x features) piece of the loss forward/backward (reference models/model.py:128-201 get_loss + torch.autograd) is an explicit
// forward/backward kernel pair, driven one layer at a time from moldiff_amd/train_ops.py and csrc/mdx_fast.cpp.  Unlike the sampling
// path these are NOT fused across layers (the fused training kernels are in mdx_train_fused.hip): activations live in HBM between
// operators so that every parameter gradient is a plain contraction over stored tensors.  The row operators between the contractions
// (LayerNorm, element-wise, gather / segment sums, geometry, optimizer) are in mdx_train_rows.hip.  Three precisions share the file: exact fp32 (contractions on
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
#include "mdx_train_launch.h"
#include "mdx_train_plan.h"
#include "mdx_typed.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// SGEMM  C = A B^T: workgroup tile 128 rows x 64 features, K consumed in chunks of 32 through LDS; wave w owns rows
// 32w..32w+31 (2 row tiles) x all 64 features (4 feature tiles) -> acc[4][2].  Operand roles follow gemm_tile: the
// MFMA A-operand is the B matrix (features), the B-operand the A matrix (rows), so acc[ft][et][r] =
// C[row 16 et + c][feature 16 ft + 4 q + r] and stores are 16-byte vectors along the feature axis.
// gridDim.z > 1 = split-K: split z handles k in [z*kper, (z+1)*kper) and writes its partial to P[z][M][N].
// ------------------------------------------------------------------------------------------------------------------
constexpr int G_TM = 128, G_TN = 64, G_KC = 32, G_LD = G_KC + 8;

// (typed operands -- fp32 or float16 containers: mdx_typed.h)
// 4 consecutive k-values of row `row_off` (element offset of the row), zero beyond K or outside the matrix
__device__ __forceinline__ f32x4 load4_guard_t(const TP& t, size_t row_off, int k, int K, bool row_ok, bool vec_ok) {
  if (!row_ok || k >= K) return splat4(0.f);
  if (vec_ok && k + 3 < K) return ldv<4>(t, row_off + k);
  f32x4 v = splat4(0.f);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (k + j < K) v[j] = ldv<1>(t, row_off + k + j);
  return v;
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
__device__ __forceinline__ typename HalfT<HT>::v8 lds_h8(const uint16_t* p) { return *reinterpret_cast<const typename HalfT<HT>::v8*>(p); }

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
          if (col + r < N) v[r] += ldv<1>(addend, (size_t)row * ldd + col + r);
      }
      if (ROUND) {  // the Linear's output in the low-precision type, like autocast's fp16 / bf16 result (held in an fp32 container)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = round_half<HT>(v[r]);
      }
      const size_t o = (size_t)row * ldc + col;
      if (veco && col + 3 < N) {
        stv<4>(C, o, v);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (col + r < N) stv<1>(C, o + r, v[r]);
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
            v = v + ldv<4>(addend, (size_t)row * ldd + col0 + col);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += ldv<1>(addend, (size_t)row * ldd + col0 + col + r);
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
          stv<4>(C, o, v);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) stv<1>(C, o + r, v[r]);
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
            stv<4>(ln.post, (size_t)row * ln.ldp + col, y);
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
      float sv = ldv<1>(s_, (size_t)m * lds);   // (the scalar operand may be one column of a wider matrix)
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
          a0 = ldv<4>(A_, (size_t)m * lda + 4 * cl);
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) a0[r] = ldv<1>(A_, (size_t)m * lda + 4 * cl + r);
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
}  // namespace

// out (M x N, ld) = bias + sum over the S partial copies in P; more than RED_CHUNK copies go through `scratch`
// (ceil(S / RED_CHUNK) * M * N floats) in two fixed-order stages.  (Declared in mdx_train_launch.h: the LayerNorm backward of
// mdx_train_rows.hip ends in it.)
void launch_reduce_partials(const float* P, int S, int M, int N, const float* bias, float* out, int ld, float* scratch, hipStream_t s,
                            int rkind) {
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
static void finish_split(float* partial, const SplitLayout& L, int N, int K, float* dW, int ldw, float* db, int rkind, hipStream_t s) {
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
