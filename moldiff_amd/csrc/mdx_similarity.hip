// Set-level similarity of decoded molecules on the device: a hashed circular fingerprint and an isomorphism-invariant key per
// molecule (mdx_mol_fingerprint), and the Tanimoto similarity of every row of one fingerprint set against every row of another
// (mdx_fp_tanimoto).  They stand in, without RDKit, for the reference's `similarity` block (scripts/evaluate_all.py:164-174,
// utils/scoring_func.py:102-223): uniqueness, diversity, similarity to and novelty against a reference set.  The functions are
// DEFINED in include/moldiff_hip.h; moldiff_amd/similarity.py restates them in numpy and the GPU tests compare bit for bit.
//
// Fingerprint.  One workgroup of 256 threads per molecule over the compact arrays of mdx_mol.h.  Two arrays of one uint32
// per atom, `id` (the atom's identifier of the current round) and `acc` (the wrapping sum over its bonds of the hashed neighbour
// identifiers), play ping-pong: a bond pass reads id and adds into acc with one integer atomic per bond end, an atom pass reads both,
// writes the next id and clears acc.  A wrapping integer sum does not depend on the order the atomics land in, so there are no
// neighbour lists and no sort.  The arrays live in LDS for a molecule of at most FP_LDS_ATOMS atoms, else in the caller's workspace
// (what atomics update in global memory is read back with agent-scope loads); the bit row is always built in LDS with atomicOr and
// written out with plain stores.
//
// Tanimoto.  A workgroup owns a tile of 64 rows of A and walks tiles of 64 rows of B, both staged in LDS in chunks of at most 64
// words per row (zero-padded to a multiple of 4 words; zeros add nothing to a popcount).  Thread (ta, tb) of the 16 x 16 owns the 16
// pairs (ta + 16 i, tb + 16 j): rows 16 apart per thread make the 16 lanes of a ds_read_b128 group read 16 consecutive rows, and the
// row stride of 68 words puts those on 16 different 4-bank slots.  Per 4 words a thread reads 4 + 4 vectors and does 64 and +
// popcount-accumulate pairs.  Row partials (int64 fixed-point sum, packed maximum) stay in registers over all of the workgroup's B
// tiles, are reduced over the 16 lanes that share a row and leave as one 64-bit atomic add and one 64-bit atomic max per row and
// workgroup.  The packed maximum is (bits of q) << 32 | ~j: q >= 0, so unsigned order is numeric order, and among equal q the
// smallest j has the largest ~j.  Integer atomics only: the result does not depend on tiling or arrival order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/moldiff_hip.h"
#include "mdx_mol.h"

int mdx_set_error(int code, const char* msg);  // mdx_api.hip

namespace {

// ---- fingerprint ---------------------------------------------------------------------------------------------------------------------

constexpr int FP_LDS_ATOMS = 1024;   // 2 x 4 KB of ids + 4 KB of bits: the 8 workgroups a CU's 32 waves allow use 96 of its 160 KB
constexpr int FP_MAX_WORDS = 1024;   // nbits <= 32768
constexpr int FP_MAX_ROUNDS = 64;
constexpr unsigned FP_GOLD = 0x9e3779b9u, FP_PRIME = 0x01000193u, FP_HI = 0x5bd1e995u;

struct FpArgs {
  MolArrays mol;
  int radius, key_rounds, nbits;
  unsigned* bits;   // (B, nbits / 32)
  int* n_on;        // (B)
  long long* key;   // (B)
  unsigned *ws_id, *ws_acc;  // (N_cap) each
};

__device__ inline unsigned mix(unsigned h) {  // murmur3 fmix32
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// the rounds of one molecule (LDS: id and acc are in LDS, else in global memory: ld / st of mdx_mol.h); returns this thread's share of (key_lo, key_hi) and sets the bits of rounds 0 .. radius in s_bits
template <bool LDS>
__device__ inline void fp_rounds(const FpArgs& A, unsigned* id, unsigned* acc, unsigned* s_bits, int n, int nb, const int* atype,
                                 const int* bi, const int* bj, const int* bt, unsigned& klo, unsigned& khi) {
  const int tid = threadIdx.x;
  const unsigned nbits = (unsigned)A.nbits;
  auto tally = [&](unsigned v, int r) {
    if (r <= A.radius) atomicOr(&s_bits[(v % nbits) >> 5], 1u << (v & 31u));  // nbits % 32 == 0: (v % nbits) % 32 == v % 32
    klo += mix(v + (unsigned)r);
    khi += mix(v ^ FP_HI);
  };
  for (int i = tid; i < n; i += 256) st<LDS>(&acc[i], 0u);
  __syncthreads();
  for (int b = tid; b < nb; b += 256) {  // degrees
    const int i = bi[b], j = bj[b];
    if (!mol_bond_ok(i, j, n)) continue;
    atomicAdd(&acc[i], 1u);
    atomicAdd(&acc[j], 1u);
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const unsigned v = mix((unsigned)atype[i] + 1u + FP_GOLD * (ld<LDS>(&acc[i]) + 1u));
    st<LDS>(&id[i], v);
    st<LDS>(&acc[i], 0u);
    tally(v, 0);
  }
  __syncthreads();
  for (int r = 0; r < A.key_rounds; ++r) {
    for (int b = tid; b < nb; b += 256) {
      const int i = bi[b], j = bj[b];
      if (!mol_bond_ok(i, j, n)) continue;
      const unsigned t = FP_GOLD * (unsigned)bt[b];
      atomicAdd(&acc[i], mix(ld<LDS>(&id[j]) + t));
      atomicAdd(&acc[j], mix(ld<LDS>(&id[i]) + t));
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const unsigned v = mix(ld<LDS>(&id[i]) * FP_PRIME + (unsigned)(r + 1) + ld<LDS>(&acc[i]));
      st<LDS>(&id[i], v);
      st<LDS>(&acc[i], 0u);
      tally(v, r + 1);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void mol_fingerprint_kernel(const FpArgs A) {
  __shared__ unsigned s_id[FP_LDS_ATOMS], s_acc[FP_LDS_ATOMS], s_bits[FP_MAX_WORDS], s_red[3];
  const int m = blockIdx.x, tid = threadIdx.x, W = A.nbits >> 5;
  unsigned* row = A.bits + (size_t)m * W;
  const MolView v = mol_view(A.mol, m);
  const long long n0 = v.n0, h0 = v.h0;
  const int n = v.n, nb = v.nb;
  if (v.masked || v.outside) {  // uniform: zero row, n_on 0, key 0
    for (int w = tid; w < W; w += 256) row[w] = 0u;
    if (tid == 0) A.n_on[m] = 0, A.key[m] = 0;
    return;
  }
  for (int w = tid; w < W; w += 256) s_bits[w] = 0u;
  if (tid < 3) s_red[tid] = 0u;
  // the first barrier inside fp_rounds orders these before the first atomicOr
  unsigned klo = 0u, khi = 0u;
  const int *atype = A.mol.atom_type + n0, *bi = A.mol.bond_i + h0, *bj = A.mol.bond_j + h0, *bt = A.mol.bond_type + h0;
  if (n <= FP_LDS_ATOMS)  // uniform
    fp_rounds<true>(A, s_id, s_acc, s_bits, n, nb, atype, bi, bj, bt, klo, khi);
  else
    fp_rounds<false>(A, A.ws_id + n0, A.ws_acc + n0, s_bits, n, nb, atype, bi, bj, bt, klo, khi);
  unsigned on = 0u;
  for (int w = tid; w < W; w += 256) {
    const unsigned x = s_bits[w];
    row[w] = x;
    on += (unsigned)__popc(x);
  }
  on = wave_sum(on), klo = wave_sum(klo), khi = wave_sum(khi);
  if ((tid & 63) == 0) {
    atomicAdd(&s_red[0], on);
    atomicAdd(&s_red[1], klo);
    atomicAdd(&s_red[2], khi);
  }
  __syncthreads();
  if (tid == 0) {
    A.n_on[m] = (int)s_red[0];
    A.key[m] = (long long)((unsigned long long)s_red[2] << 32 | (unsigned long long)s_red[1]);
  }
}

// ---- Tanimoto ------------------------------------------------------------------------------------------------------------------------

constexpr int TN_T = 64;            // rows of A and rows of B per tile
constexpr int TN_W = 64;            // words per row staged at a time
constexpr int TN_S = TN_W + 4;      // row stride in LDS (words): 16 consecutive rows start on 16 different 16-byte slots of the 256
constexpr int TN_TARGET_WG = 2048;  // workgroups aimed at: 256 CUs x 4 resident x 2

struct TanArgs {
  const unsigned *A, *Bm;
  const int *na, *nb;
  long long Na, Nb;
  int W, exclude_diagonal, tiles_per_split;
  unsigned long long* pack;  // (Na) workspace: (bits of row_max) << 32 | ~row_argmax, 0 = no partner yet
  unsigned long long* sum;   // (Na) = row_sum
  float* row_max;
  int* row_argmax;
};

__global__ __launch_bounds__(256) void tanimoto_init_kernel(const TanArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < a.Na) a.pack[i] = 0ull, a.sum[i] = 0ull;
}

__global__ __launch_bounds__(256) void tanimoto_finish_kernel(const TanArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.Na) return;
  const unsigned long long p = a.pack[i];
  a.row_max[i] = __uint_as_float((unsigned)(p >> 32));
  a.row_argmax[i] = (int)~(unsigned)p;  // pack 0 (no partner): 0.0 and -1
}

// rows r0 .. r0 + 63 of g (N rows of W words), words w0 .. w0 + cw - 1, into s; rows past N and words past W read as zero
__device__ inline void tn_stage(unsigned* s, const unsigned* g, long long r0, long long N, int W, int w0, int cw) {
  for (int idx = threadIdx.x; idx < TN_T * cw; idx += 256) {
    const int r = idx / cw, w = idx - r * cw;
    const long long gr = r0 + r;
    const int gw = w0 + w;
    s[r * TN_S + w] = (gr < N && gw < W) ? g[(size_t)gr * (size_t)W + (size_t)gw] : 0u;
  }
}

__device__ inline unsigned long long shfl_xor64(unsigned long long v, int o) {
  const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
  return (unsigned long long)hi << 32 | lo;
}

__global__ __launch_bounds__(256) void tanimoto_kernel(const TanArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned sA[TN_T * TN_S];
  __shared__ __attribute__((aligned(16))) unsigned sB[TN_T * TN_S];
  const int tid = threadIdx.x, tb = tid & 15, ta = tid >> 4, W = a.W;
  const long long row0 = (long long)blockIdx.x * TN_T;
  const long long col_tiles = (a.Nb + TN_T - 1) / TN_T;
  const long long ct0 = (long long)blockIdx.y * a.tiles_per_split, ct1 = min(ct0 + a.tiles_per_split, col_tiles);
  const bool once = W <= TN_W;  // the A tile is staged once and kept
  int na[4];
  long long sum[4];
  unsigned long long best[4];
  for (int i = 0; i < 4; ++i) {
    const long long row = row0 + ta + 16 * i;
    na[i] = row < a.Na ? a.na[row] : 0;
    sum[i] = 0, best[i] = 0ull;
  }
  if (once) tn_stage(sA, a.A, row0, a.Na, W, 0, (W + 3) & ~3);
  for (long long ct = ct0; ct < ct1; ++ct) {
    const long long col0 = ct * TN_T;
    int c[4][4] = {};
    for (int w0 = 0; w0 < W; w0 += TN_W) {
      const int cw = min(TN_W, (W - w0 + 3) & ~3);
      if (!once) tn_stage(sA, a.A, row0, a.Na, W, w0, cw);
      tn_stage(sB, a.Bm, col0, a.Nb, W, w0, cw);
      __syncthreads();
      for (int w = 0; w < cw; w += 4) {
        uint4 x[4], y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const uint4*>(&sA[(ta + 16 * i) * TN_S + w]);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = *reinterpret_cast<const uint4*>(&sB[(tb + 16 * j) * TN_S + w]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            c[i][j] += __popc(x[i].x & y[j].x) + __popc(x[i].y & y[j].y) + __popc(x[i].z & y[j].z) + __popc(x[i].w & y[j].w);
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long col = col0 + tb + 16 * j;
      if (col >= a.Nb) continue;
      const int nbj = a.nb[col];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long row = row0 + ta + 16 * i;
        if (row >= a.Na || (a.exclude_diagonal && row == col)) continue;
        const int u = na[i] + nbj - c[i][j];
        const float q = u > 0 ? (float)c[i][j] / (float)u : 0.0f;  // one correctly rounded division
        sum[i] += (long long)(q * 1099511627776.0f);              // q * 2^40: an exact integer (see the header)
        const unsigned long long p = (unsigned long long)__float_as_uint(q) << 32 | (unsigned long long)(~(unsigned)col);
        best[i] = max(best[i], p);
      }
    }
  }
  for (int i = 0; i < 4; ++i) {
    unsigned long long s = (unsigned long long)sum[i], b = best[i];
    for (int o = 1; o < 16; o <<= 1) {  // the 16 lanes tb = 0 .. 15 of one ta are consecutive lanes of one wave
      s += shfl_xor64(s, o);
      b = max(b, shfl_xor64(b, o));
    }
    const long long row = row0 + ta + 16 * i;
    if (tb == 0 && row < a.Na) {
      if (s) atomicAdd(&a.sum[row], s);
      if (b) atomicMax(&a.pack[row], b);
    }
  }
}

}  // namespace

extern "C" size_t mdx_mol_fingerprint_ws_bytes(int64_t N_cap) { return 8 * (size_t)std::max<int64_t>(N_cap, 1); }

extern "C" int mdx_mol_fingerprint(int32_t B, const int32_t* atom_ptr, const int32_t* bond_ptr, const int32_t* n_atoms,
                                   const int32_t* n_bonds, const int32_t* atom_type, int64_t N_cap, const int32_t* bond_type,
                                   const int32_t* bond_index, int64_t Eh_stride, const int32_t* select, int32_t radius,
                                   int32_t key_rounds, int32_t nbits, int32_t* bits, int32_t* n_on, int64_t* key, void* ws,
                                   size_t ws_bytes, void* stream) {
  FpArgs a{};
  if (const char* why = mol_arrays_fill(&a.mol, B, atom_ptr, bond_ptr, n_atoms, n_bonds, atom_type, N_cap, bond_type, bond_index, Eh_stride, select))
    return mdx_set_error(MDX_ERR_ARG, why);
  if (!bits || !n_on || !key) return mdx_set_error(MDX_ERR_ARG, "null argument");
  if (nbits < 32 || nbits > 32 * FP_MAX_WORDS || nbits % 32) return mdx_set_error(MDX_ERR_ARG, "nbits must be a multiple of 32 in 32 .. 32768");
  if (radius < 0 || key_rounds < radius || key_rounds > FP_MAX_ROUNDS)
    return mdx_set_error(MDX_ERR_ARG, "rounds must satisfy 0 <= radius <= key_rounds <= 64");
  if (!ws || ws_bytes < mdx_mol_fingerprint_ws_bytes(N_cap)) return mdx_set_error(MDX_ERR_ARG, "workspace too small: need 8 * max(N_cap, 1) bytes");
  if (reinterpret_cast<uintptr_t>(ws) & 3) return mdx_set_error(MDX_ERR_ARG, "workspace must be 4-byte aligned");
  a.radius = radius, a.key_rounds = key_rounds, a.nbits = nbits;
  a.bits = reinterpret_cast<unsigned*>(bits), a.n_on = n_on, a.key = reinterpret_cast<long long*>(key);
  a.ws_id = reinterpret_cast<unsigned*>(ws), a.ws_acc = a.ws_id + std::max<int64_t>(N_cap, 1);
  return mol_launch(mol_fingerprint_kernel, "mol_fingerprint_kernel", B, stream, a);
}

extern "C" size_t mdx_fp_tanimoto_ws_bytes(int64_t Na) { return 8 * (size_t)std::max<int64_t>(Na, 1); }

extern "C" int mdx_fp_tanimoto(const int32_t* bits_a, const int32_t* n_on_a, int64_t Na, const int32_t* bits_b, const int32_t* n_on_b,
                               int64_t Nb, int32_t nbits, int32_t exclude_diagonal, float* row_max, int32_t* row_argmax,
                               int64_t* row_sum, void* ws, size_t ws_bytes, void* stream) {
  if (Na < 0 || Nb < 0) return mdx_set_error(MDX_ERR_ARG, "negative size");
  if (nbits < 32 || nbits > 32 * FP_MAX_WORDS || nbits % 32) return mdx_set_error(MDX_ERR_ARG, "nbits must be a multiple of 32 in 32 .. 32768");
  if (exclude_diagonal && Na != Nb) return mdx_set_error(MDX_ERR_ARG, "exclude_diagonal needs Na == Nb");
  if (Nb > (1ll << 22)) return mdx_set_error(MDX_ERR_UNSUPPORTED, "more than 2^22 columns: row_sum could leave int64");
  if (Na > (1ll << 30)) return mdx_set_error(MDX_ERR_UNSUPPORTED, "more than 2^30 rows");
  if ((Na > 0 && (!bits_a || !n_on_a || !row_max || !row_argmax || !row_sum)) || (Nb > 0 && (!bits_b || !n_on_b)))
    return mdx_set_error(MDX_ERR_ARG, "null argument");
  if (!ws || ws_bytes < mdx_fp_tanimoto_ws_bytes(Na)) return mdx_set_error(MDX_ERR_ARG, "workspace too small: need 8 * max(Na, 1) bytes");
  if (reinterpret_cast<uintptr_t>(ws) & 7) return mdx_set_error(MDX_ERR_ARG, "workspace must be 8-byte aligned");
  if (Na == 0) return MDX_OK;
  TanArgs a{};
  a.A = reinterpret_cast<const unsigned*>(bits_a), a.Bm = reinterpret_cast<const unsigned*>(bits_b);
  a.na = n_on_a, a.nb = n_on_b, a.Na = Na, a.Nb = Nb;
  a.W = nbits / 32, a.exclude_diagonal = exclude_diagonal != 0;
  a.pack = reinterpret_cast<unsigned long long*>(ws), a.sum = reinterpret_cast<unsigned long long*>(row_sum);
  a.row_max = row_max, a.row_argmax = row_argmax;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned flat = (unsigned)((Na + 255) / 256);
  hipLaunchKernelGGL(tanimoto_init_kernel, dim3(flat), dim3(256), 0, s, a);
  if (Nb > 0) {
    const int64_t row_tiles = (Na + TN_T - 1) / TN_T, col_tiles = (Nb + TN_T - 1) / TN_T;
    const int64_t splits = std::min<int64_t>(col_tiles, std::max<int64_t>(1, (TN_TARGET_WG + row_tiles - 1) / row_tiles));
    a.tiles_per_split = (int)((col_tiles + splits - 1) / splits);
    const unsigned gy = (unsigned)((col_tiles + a.tiles_per_split - 1) / a.tiles_per_split);
    hipLaunchKernelGGL(tanimoto_kernel, dim3((unsigned)row_tiles, gy), dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(tanimoto_finish_kernel, dim3(flat), dim3(256), 0, s, a);
  if (hipGetLastError() != hipSuccess) return mdx_set_error(MDX_ERR_HIP, "tanimoto kernels: launch failed");
  return MDX_OK;
}
