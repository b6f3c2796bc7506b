// Layer-level operators of the training path (gfx950), part 2: the row operators between the contractions of mdx_train.hip -- every
// O(rows x features) piece of the loss forward/backward that is not a matrix product, as an explicit forward/backward kernel pair
// (driven from moldiff_amd/train_ops.py and csrc/mdx_fast.cpp; activations live in HBM between operators).  The `_t` entry points
// take fp32 or float16 CONTAINERS per tensor (a bit mask names the tensors stored as float16; access: mdx_typed.h).
//
//   ln_relu                 y = relu(LN(x) * gamma + beta): forward (saves mean, rstd), backward (dx, partial rows of dgamma | dbeta)
//                           and the backward fused with a rank-1 Linear in front of it; generic fp32 kernels and 4-wide typed ones
//   ew, sum_n               add / sub / mul / a * sigmoid(b), forward and backward; sum of up to 12 tensors: one body each, 1 or 4 wide
//   gather / segsum         y = x[idx]; out[r] = sum_{j in seg r} src[order[j]] (each is the other's backward; no atomics): one body each;
//                           the segment sum in two summation orders (sequential, or dealt to four threads), 1 / 4 / 8 features per thread
//   mul_gather, plan_flip   a * t[idx] without the gathered tensor; the CSR order of the flipped half of an edge list
//   edge_geom, smear, force                     rel / dist of an edge, Gaussian smearing, w * rel / d / (d + 1), with backwards
//   sumsq, adamw, amp_adamw                     gradient norm and the optimizer step (with the loss scaler's decision on the device)
//
// LayerNorm partial rows and the deferred reduction's layout are in mdx_train_plan.h; the LayerNorm backward ends in
// launch_reduce_partials of mdx_train.hip (mdx_train_launch.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/moldiff_hip.h"
#include "mdx_tile.h"
#include "mdx_train_launch.h"
#include "mdx_train_plan.h"
#include "mdx_typed.h"

namespace {

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
  const f32x4 v = ok ? ldv<4>(x, (size_t)row * F + 4 * c4) : splat4(0.f);
  const float mean = row_lanes_sum<LPR>((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / F);
  const f32x4 d = v - splat4(mean);
  const float rstd = 1.0f / sqrtf(row_lanes_sum<LPR>(fmaf(d[0], d[0], fmaf(d[1], d[1], fmaf(d[2], d[2], d[3] * d[3])))) * (1.0f / F) + MDX_LN_EPS);
  if (!ok) return;
  const f32x4 gmv = {gamma[4 * c4], gamma[4 * c4 + 1], gamma[4 * c4 + 2], gamma[4 * c4 + 3]};  // (parameters: any 4-byte offset)
  const f32x4 btv = {beta[4 * c4], beta[4 * c4 + 1], beta[4 * c4 + 2], beta[4 * c4 + 3]};
  f32x4 o = d * splat4(rstd) * gmv + btv;
  if (relu) o = relu4(o);
  stv<4>(y, (size_t)row * F + 4 * c4, o);
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
    const f32x4 xh = (ldv<4>(x, o) - splat4(mean)) * splat4(rstd);
    f32x4 g = splat4(0.f);
    if (r1w) {
      if (ok) {
        const float gv = round_half<1>(ldv<1>(dy, (size_t)row));
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = round_half<1>(gv * w1[k]);
      }
    } else if (ok) {
      g = ldv<4>(dy, o);
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
    if (ok) stv<4>(dx, o, (gh - splat4(m1) - xh * splat4(m2)) * splat4(rstd));
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
// Every row operator below is ONE body over W elements per thread (mdx_typed.h: ldv<W> / stv<W>, operands fp32 or float16 containers):
// W = 4 needs lengths that are multiples of 4 and naturally aligned bases; W = 1 takes any length / alignment (an (E,1) gate product has
// E % 4 != 0; an unaligned or odd-length fp32 tensor).  The arithmetic per lane does not depend on W.
__device__ __forceinline__ float sigmoid_v(float v) { return sigmoidf_(v); }
__device__ __forceinline__ f32x4 sigmoid_v(f32x4 v) { return sigmoid4(v); }
__device__ __forceinline__ float round_v(float v, int rk) { return round_kind(v, rk); }
__device__ __forceinline__ f32x4 round_v(f32x4 v, int rk) {
  if (rk == 0) return v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = round_kind(v[j], rk);
  return v;
}
// (the sign of a zero gradient is what each width has always produced: -0 from the scalar form, +0 from the vector form)
__device__ __forceinline__ float neg_v(float v) { return -v; }
__device__ __forceinline__ f32x4 neg_v(f32x4 v) { return splat4(0.f) - v; }

// opr = op | (rkind << 8): rkind != 0 rounds the result (and the sigmoid of the gate) to bfloat16 / float16 -- the value the
// reference's fp16 tensors hold under autocast (both factors of these products are Linear outputs there).  n = groups of W elements.
template <int W>
__global__ void ew_fwd_kernel(int opr, const TP a, const TP b, const TPW o, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int op = opr & 255, rk = opr >> 8;
  const tvec_t<W> x = ldv<W>(a, W * i), y = ldv<W>(b, W * i);
  tvec_t<W> r;
  switch (op) {
    case 0: r = x + y; break;
    case 1: r = x - y; break;
    case 2: r = x * y; break;
    default: r = x * round_v(sigmoid_v(y), rk);
  }
  stv<W>(o, W * i, round_v(r, rk));
}
template <int W>
__global__ void ew_bwd_kernel(int op, const TP a, const TP b, const TP g, const TPW da, const TPW db, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const tvec_t<W> go = ldv<W>(g, W * i);
  tvec_t<W> ga, gb;
  switch (op) {
    case 0: ga = go; gb = go; break;
    case 1: ga = go; gb = neg_v(go); break;
    case 2: ga = go * ldv<W>(b, W * i); gb = go * ldv<W>(a, W * i); break;
    default: {
      const tvec_t<W> sg = sigmoid_v(ldv<W>(b, W * i));
      ga = go * sg;
      gb = go * ldv<W>(a, W * i) * sg * (1.0f - sg);
    }
  }
  if (da.p) stv<W>(da, W * i, ga);
  if (db.p) stv<W>(db, W * i, gb);
}
// out = sum of up to 12 tensors of one shape (round 6): the gradient of a tensor with several consumers.  autograd would add the
// consumers' gradients pairwise (k - 1 launches of an element-wise add, each rounding to the container); here they are summed in
// fp32 in argument order and rounded ONCE.
struct SumN {
  const void* p[12];
  int h[12];
  int n;
};
template <int W>
__global__ void sum_n_kernel(const SumN a, const TPW o, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  tvec_t<W> s = ldv<W>(TP{a.p[0], a.h[0]}, W * i);
  for (int j = 1; j < a.n; ++j) s = s + ldv<W>(TP{a.p[j], a.h[j]}, W * i);
  stv<W>(o, W * i, s);
}

// y[i] = x[idx[i]]  (rows of FW groups of W features; one thread per group)
template <int W>
__global__ void gather_rows_kernel(const TP x, const int64_t* __restrict__ idx, int64_t M, int FW, const TPW y) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * FW) return;
  const int64_t row = i / FW;
  stv<W>(y, W * i, ldv<W>(x, W * ((size_t)idx[row] * FW + (int)(i % FW))));
}
// out[r] = sum_{j in [ptr[r], ptr[r+1])} src[order[j]]: rows gathered in CSR order, no atomics, bitwise deterministic.  An output element
// is W features of one segment (W = 8: float16 rows on 16 bytes, one load per row -- half the threads and load instructions of W = 4).
//   DEAL = 1   one thread per element, four rows in flight (round 6: one dependent index load + one row load per iteration was
//              latency-bound at ~25 rows per node), additions strictly (((s + v0) + v1) + v2) + v3: the sequential CSR order of
//              torch's index_add on the CPU, i.e. of the reference and the oracle.
//   DEAL = 4   the segment's rows dealt to FOUR threads (round 6): thread k takes rows k, k + 4, ... (four in flight each: sixteen
//              row gathers per element), the partial sums are combined through LDS as ((p0 + p1) + p2) + p3; 64 elements per workgroup.
//              A node has ~28 rows; with one thread per element the kernel ran seven dependent gather rounds at ten waves per CU.
//              Deterministic, but NOT the sequential order: see mdx_op_segsum_rows_t for who takes it.
// The sums per feature and their order depend on DEAL alone, not on W.
template <int W, int DEAL>
__global__ __launch_bounds__(256) void segsum_rows_kernel(const TP src, const int64_t* __restrict__ order, const int64_t* __restrict__ ptr,
                                                          int64_t R, int FW, const TPW out) {
  static_assert(DEAL == 1 || DEAL == 4, "one thread per element, or four");
  constexpr int EPB = 256 / DEAL;                  // elements per workgroup
  constexpr int QW = W == 8 ? 4 : W, NQ = W / QW;  // an element leaves (and crosses LDS) as NQ pieces of QW features
  const int k = DEAL == 1 ? 0 : threadIdx.x / EPB, it = threadIdx.x % EPB;
  const size_t i = (size_t)blockIdx.x * EPB + it;
  const bool live = i < (size_t)R * FW;
  tvec_t<W> s{};
  if (live) {
    const int64_t r = i / FW;
    const int f = (int)(i % FW);
    int64_t j = ptr[r] + k;
    const int64_t e = ptr[r + 1];
    for (; j + 3 * DEAL < e; j += 4 * DEAL) {
      const int64_t o0 = order[j], o1 = order[j + DEAL], o2 = order[j + 2 * DEAL], o3 = order[j + 3 * DEAL];
      const tvec_t<W> v0 = ldv<W>(src, W * ((size_t)o0 * FW + f)), v1 = ldv<W>(src, W * ((size_t)o1 * FW + f));
      const tvec_t<W> v2 = ldv<W>(src, W * ((size_t)o2 * FW + f)), v3 = ldv<W>(src, W * ((size_t)o3 * FW + f));
      s = s + v0;
      s = s + v1;
      s = s + v2;
      s = s + v3;
    }
    for (; j < e; j += DEAL) s = s + ldv<W>(src, W * ((size_t)order[j] * FW + f));
  }
  tvec_t<QW> q[NQ];
  if constexpr (W == 8) q[0] = lo4(s), q[1] = hi4(s);
  else q[0] = s;
  if constexpr (DEAL == 4) {
    __shared__ tvec_t<QW> part[3][NQ][EPB];
#pragma unroll
    for (int h = 0; h < NQ; ++h)
      if (k) part[k - 1][h][it] = q[h];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < NQ; ++h)
      if (k == 0 && live) q[h] = ((q[h] + part[0][h][it]) + part[1][h][it]) + part[2][h][it];
  }
#pragma unroll
  for (int h = 0; h < NQ; ++h)
    if (k == 0 && live) stv<QW>(out, W * i + QW * h, q[h]);
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
// y[i] = a[i] * t[idx[i]] and its two gradients (da = g * t[idx];  dt[r] = sum_{j in seg r} g[order[j]] * a[order[j]]):
// the product with a gathered per-node row without materialising the gathered (rows x F) tensor.  F % 4 == 0.
__global__ void mulg_fwd_kernel(const TP a, const TP t, const int64_t* __restrict__ idx, int64_t M, int F4, const TPW y, int rk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)M * F4) return;
  const int64_t row = i / F4;
  const f32x4 tv = ldv<4>(t, 4 * ((size_t)idx[row] * F4 + (int)(i % F4)));
  f32x4 r = ldv<4>(a, 4 * i) * tv;      // forward: a * t[idx];  backward wrt a: g * t[idx] (the caller passes g as `a`)
  if (rk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = round_kind(r[j], rk);
  }
  stv<4>(y, 4 * i, r);
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
    const f32x4 g0 = ldv<4>(g, o0), a0 = ldv<4>(a, o0), g1 = ldv<4>(g, o1), a1 = ldv<4>(a, o1);
    s = s + g0 * a0;
    s = s + g1 * a1;
  }
  for (; j < e; ++j) {
    const size_t o = 4 * ((size_t)order[j] * F4 + f);
    s = s + ldv<4>(g, o) * ldv<4>(a, o);
  }
  stv<4>(out, 4 * i, s);
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

}  // namespace

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
  const bool vec = (n & 3) == 0 && tp_vec_ok(a, ta.h, 4) && tp_vec_ok(b, tb.h, 4) && tp_vec_ok(out, to.h, 4);
  pick<1, 4>(vec ? 4 : 1, [&](auto W) {
    hipLaunchKernelGGL(ew_fwd_kernel<W>, dim3(nblk((size_t)n / W)), dim3(256), 0, (hipStream_t)stream, op, ta, tb, to, (size_t)n / W);
  });
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
  pick<1, 4>(vec ? 4 : 1, [&](auto W) {
    hipLaunchKernelGGL(sum_n_kernel<W>, dim3(nblk((size_t)n / W)), dim3(256), 0, (hipStream_t)stream, a, to, (size_t)n / W);
  });
  return launched();
}
extern "C" int mdx_op_ew_bwd_t(int32_t op, const void* a, const void* b, const void* g, void* da, void* db, int64_t n, int32_t dt,
                               void* stream) {
  if (n <= 0) return MDX_OK;
  if (op < 0 || op > 3) return bad("ew: unknown op");
  const TP ta{a, dt & 1}, tb{b, (dt >> 1) & 1}, tg{g, (dt >> 2) & 1};
  const TPW tda{da, (dt >> 3) & 1}, tdb{db, (dt >> 4) & 1};
  const bool vec = (n & 3) == 0 && tp_vec_ok(a, ta.h, 4) && tp_vec_ok(b, tb.h, 4) && tp_vec_ok(g, tg.h, 4) && tp_vec_ok(da, tda.h, 4) &&
                   tp_vec_ok(db, tdb.h, 4);
  pick<1, 4>(vec ? 4 : 1, [&](auto W) {
    hipLaunchKernelGGL(ew_bwd_kernel<W>, dim3(nblk((size_t)n / W)), dim3(256), 0, (hipStream_t)stream, op, ta, tb, tg, tda, tdb, (size_t)n / W);
  });
  return launched();
}
extern "C" int mdx_op_gather_rows_t(const void* x, const int64_t* idx, int64_t M, int32_t F, void* y, int32_t dt, void* stream) {
  if (M <= 0 || F <= 0) return MDX_OK;
  const TP tx{x, dt & 1};
  const TPW ty{y, (dt >> 1) & 1};
  const bool vec = (F & 3) == 0 && tp_vec_ok(x, tx.h, 4) && tp_vec_ok(y, ty.h, 4);
  if (!vec && dt) return bad("gather_rows: half storage needs F % 4 == 0 and aligned rows");
  pick<1, 4>(vec ? 4 : 1, [&](auto W) {
    hipLaunchKernelGGL(gather_rows_kernel<W>, dim3(nblk((size_t)M * (F / W))), dim3(256), 0, (hipStream_t)stream, tx, idx, M, F / W, ty);
  });
  return launched();
}
extern "C" int mdx_op_segsum_rows_t(const void* src, const int64_t* order, const int64_t* ptr, int64_t R, int32_t F, void* out, int32_t dt,
                                    void* stream) {
  if (R <= 0 || F <= 0) return MDX_OK;
  const TP ts{src, dt & 1};
  const TPW to{out, (dt >> 1) & 1};
  const bool vec = (F & 3) == 0 && tp_vec_ok(src, ts.h, 4) && tp_vec_ok(out, to.h, 4);
  if (!vec && (dt & 3)) return bad("segsum_rows: half storage needs F % 4 == 0 and aligned rows");
  // The dealt order for float16 rows and where the caller allows another order (dt bit 2: the autocast mode; 4-wide and wider only below
  // 2^22 four-wide items).  The fp32 mode keeps the sequential CSR order -- the order of torch's index_add on the CPU, i.e. of the reference
  // and the oracle, which its parity tests rely on (a 32-wide LayerNorm gain's gradient moved from 4.8e-5 to 1.6e-4 of its norm at
  // 256 molecules with the dealt order; both are fp32 rounding, but the contract there is 1e-4)
  const bool dealt = vec ? (ts.h || (dt & 4)) && (size_t)R * (F / 4) < ((size_t)1 << 22) : (dt & 4) != 0;
  const int W = !vec ? 1 : (dealt && ts.h && (F & 7) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) ? 8 : 4;
  pick<1, 4, 8>(W, [&](auto Wc) {               // features per thread
    pick<1, 4>(dealt ? 4 : 1, [&](auto Dc) {    // threads per element
      constexpr int w = decltype(Wc)::value, deal = decltype(Dc)::value;
      if constexpr (w != 8 || deal == 4)        // (the 16-byte load exists dealt only)
        hipLaunchKernelGGL((segsum_rows_kernel<w, deal>), dim3(nblk((size_t)R * (F / w), 256 / deal)), dim3(256), 0, (hipStream_t)stream, ts,
                           order, ptr, R, F / w, to);
    });
  });
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
